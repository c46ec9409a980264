"""Pose-error metrics of the reference's evaluation: ADD, ADD-S (BOP "adi") and their AUC.

Definitions follow tools/third_party/bop_pose_error.py:73-108 (add / adi, nearest neighbour from the
ground-truth points into the estimated points) and evaluation/metrics.py:303-344 (threshold 0.1 m ->
inf, sort, accuracy = cumsum(1)/n, VOCap * 100).  Pinned by tests/golden/bop_fixtures.json.
"""
import numpy as np
from scipy import spatial


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def add(R_est, t_est, R_gt, t_gt, pts):
    pe = pts @ np.asarray(R_est).T + np.asarray(t_est)
    pg = pts @ np.asarray(R_gt).T + np.asarray(t_gt)
    return float(np.linalg.norm(pe - pg, axis=1).mean())


def adds(R_est, t_est, R_gt, t_gt, pts):
    pe = pts @ np.asarray(R_est).T + np.asarray(t_est)
    pg = pts @ np.asarray(R_gt).T + np.asarray(t_gt)
    d, _ = spatial.cKDTree(pe).query(pg, k=1)
    return float(d.mean())


def auc(distances, threshold=0.1):
    d = np.array(distances, dtype=np.float64)
    d[d > threshold] = np.inf
    d = np.sort(d)
    n = len(d)
    if n == 0:
        return 0.0
    acc = np.cumsum(np.ones((n,), np.float32)) / n
    fin = np.isfinite(d)
    rec, prec = d[fin], acc[fin]
    if len(rec) == 0:
        return 0.0
    mrec = np.concatenate([[0.0], rec, [threshold]])
    mpre = np.concatenate([[0.0], prec, [prec[-1]]])
    mpre = np.maximum.accumulate(mpre)
    i = np.where(mrec[1:] != mrec[:-1])[0] + 1
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]) * 10.0 * 100.0)


def _trajectory(kind, pose_est, pose_ref, pts, backend):
    """Per-frame distances of a trajectory.  backend 'cpu': add / adds above, pose by pose; 'hip': the device
    (ops.pose_errors, no CPU fallback: RoftError without a device); 'auto': the device when there is one."""
    if backend not in ("cpu", "hip", "auto"):
        raise ValueError("backend must be 'cpu', 'hip' or 'auto'")
    if backend == "auto":
        from . import _lib
        backend = "hip" if _lib.lib().roft_device_count() > 0 else "cpu"
    pose_est, pose_ref = np.asarray(pose_est, float), np.asarray(pose_ref, float)
    if backend == "hip":
        from . import ops
        return ops.pose_errors(kind, pts, pose_est, pose_ref)
    f = add if kind == "add" else adds
    out = np.zeros(len(pose_est))
    for k in range(len(pose_est)):
        out[k] = f(quat_to_rot(pose_est[k, 3:]), pose_est[k, :3], quat_to_rot(pose_ref[k, 3:]), pose_ref[k, :3], pts)
    return out


def trajectory_adds(pose_est, pose_ref, pts, backend="cpu"):
    """pose_*: [F, 7] (x, q wxyz).  Returns the per-frame ADD-S distances."""
    return _trajectory("adi", pose_est, pose_ref, pts, backend)


def trajectory_add(pose_est, pose_ref, pts, backend="cpu"):
    """pose_*: [F, 7] (x, q wxyz).  Returns the per-frame ADD distances."""
    return _trajectory("add", pose_est, pose_ref, pts, backend)


# ---- BOP's symmetry-aware distances: MSSD and MSPD (include/roft_engine.h section 3h) -----------------------
def _rigid(row):
    """row x y z, q (w x y z) -> (the 9 entries of quat_to_rot(q) in row-major order, t)"""
    return quat_to_rot(row[3:7]).reshape(9), row[:3]


def _move(R, t, p):
    """R p + t for points p = (px, py, pz) as three arrays: each row R_i0 p_0 + R_i1 p_1 + R_i2 p_2 + t_i, left to right"""
    return [R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] + t[i] for i in range(3)]


def max_symmetric_distance(kind, est, ref, pts, symmetries, cam=None):
    """MSSD ('mssd') or MSPD ('mspd', cam = (fx, fy, cx, cy)) of ONE pose pair est / ref (rows x y z, q wxyz) under the group
    symmetries [n, 7], in numpy, in the operation order the header states: a = R_r (R_g p + t_g) + t_r, b = R_e p + t_e,
    sqrt(min_g max_i |b - a|^2); MSPD over the pixels fx X / Z + cx, fy Y / Z + cy, +inf when any point has Z <= 0."""
    p = np.asarray(pts, float).reshape(-1, 3).T
    Re, te = _rigid(np.asarray(est, float))
    Rr, tr = _rigid(np.asarray(ref, float))
    b = _move(Re, te, p)
    if kind == "mspd":
        fx, fy, cx, cy = cam
        bad = not np.all(b[2] > 0.0)
        with np.errstate(all="ignore"):
            ub, vb = fx * b[0] / b[2] + cx, fy * b[1] / b[2] + cy
    best = np.inf
    for el in np.asarray(symmetries, float).reshape(-1, 7):
        Rg, tg = _rigid(el)
        a = _move(Rr, tr, _move(Rg, tg, p))
        with np.errstate(all="ignore"):
            if kind == "mspd":
                bad = bad or not np.all(a[2] > 0.0)
                du, dv = ub - (fx * a[0] / a[2] + cx), vb - (fy * a[1] / a[2] + cy)
                d = du * du + dv * dv
            else:
                dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
                d = dx * dx + dy * dy + dz * dz
        best = np.minimum(best, np.max(d))   # (np.max and np.minimum keep a NaN, as the kernel does)
    if kind == "mspd" and bad:
        return np.inf
    return float(np.sqrt(best))


def _trajectory_sym(kind, pose_est, pose_ref, pts, symmetries, cam, backend):
    if backend not in ("numpy", "hip"):
        raise ValueError("backend must be 'numpy' or 'hip'")
    pose_est, pose_ref = np.asarray(pose_est, float).reshape(-1, 7), np.asarray(pose_ref, float).reshape(-1, 7)
    sym = np.array([[0.0, 0, 0, 1, 0, 0, 0]]) if symmetries is None else np.asarray(symmetries, float).reshape(-1, 7)
    if backend == "hip":
        from . import ops
        return ops.pose_errors_sym(kind, pts, pose_est, pose_ref, sym, cam)
    return np.array([max_symmetric_distance(kind, pose_est[k], pose_ref[k], pts, sym, cam) for k in range(len(pose_est))])


def trajectory_mssd(pose_est, pose_ref, pts, symmetries=None, backend="numpy"):
    """pose_*: [F, 7] (x, q wxyz); symmetries [n, 7], element 0 the identity.  Per-frame MSSD in metres.  backend 'numpy' or
    'hip' (ops.pose_errors_sym; no CPU fallback)."""
    return _trajectory_sym("mssd", pose_est, pose_ref, pts, symmetries, None, backend)


def trajectory_mspd(pose_est, pose_ref, pts, cam, symmetries=None, backend="numpy"):
    """... MSPD in pixels; cam = (fx, fy, cx, cy)."""
    return _trajectory_sym("mspd", pose_est, pose_ref, pts, symmetries, cam, backend)


# ---- BOP's Visible Surface Discrepancy and average recall (include/roft_engine.h section 3i) -----------------
BOP_VSD_TAUS = np.arange(0.05, 0.51, 0.05)           # misalignment tolerances, in object diameters
BOP_THRESHOLDS = np.arange(0.05, 0.51, 0.05)         # correctness thresholds of VSD, and of MSSD in object diameters
BOP_MSPD_THRESHOLDS = np.arange(5, 51, 5)            # ... of MSPD, in pixels of a 640-wide image


def _distance_image(depth, cam):
    """BOP's depth_im_to_dist_im_fast: the distance to the camera centre of every pixel's point; cam = (fx, fy, cx, cy)."""
    fx, fy, cx, cy = (float(v) for v in cam)
    d = np.asarray(depth, np.float32).astype(np.float64)
    a = ((np.arange(d.shape[1], dtype=np.float64) - cx) / fx)[None, :]
    b = ((np.arange(d.shape[0], dtype=np.float64) - cy) / fy)[:, None]
    return np.sqrt(((a * d) ** 2 + (b * d) ** 2) + d ** 2)


def _visible(model, test, delta):
    """BOP's visibility mask (mode bop19) of a model distance image against the measured one"""
    with np.errstate(invalid="ignore"):
        diff = model.astype(np.float32) - test.astype(np.float32)
        return ((test > 0) & (model > 0) & (diff <= np.float32(delta))) | ((test == 0) & (model > 0))


def vsd_from_depths(depth_est, depth_gt, depth_test, cam, delta=0.015, taus=None, diameter=None, counts=False):
    """VSD (BOP19: visibility mode bop19, cost `step`) of ONE pose pair from its two depth renders and the sensor's depth image,
    [H, W] float32 metres, 0 = nothing.  cam = (fx, fy, cx, cy); taus in object diameters when `diameter` is given (> 0), else
    metres; None: BOP_VSD_TAUS.  Returns errors [n_taus], with counts=True also the integer row n_union, n_inter, n_gt, n_est,
    fail[0 .. n_taus) -- what ops.pose_errors_vsd computes on the device from the poses."""
    taus = BOP_VSD_TAUS if taus is None else np.asarray(taus, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        T, G, E = (_distance_image(d, cam) for d in (depth_test, depth_gt, depth_est))
        vg = _visible(G, T, delta)
        ve = _visible(E, T, delta) | (vg & (E > 0))
        inter, union = vg & ve, vg | ve
        c = np.abs(G[inter] - E[inter])
        if diameter is not None and diameter > 0:
            c = c / float(diameter)
        fail = np.array([int(np.count_nonzero(c >= t)) for t in taus], np.int64)
    n_union, n_inter = int(np.count_nonzero(union)), int(np.count_nonzero(inter))
    errors = (fail + n_union - n_inter).astype(np.float64) / np.float64(n_union) if n_union > 0 else np.ones(len(taus))
    if counts:
        return errors, np.concatenate([[n_union, n_inter, int(np.count_nonzero(vg)), int(np.count_nonzero(ve))], fail]).astype(np.int32)
    return errors


def model_diameter(points, chunk=2048):
    """The largest distance between two of the points [P, 3] (BOP's object diameter over the model's vertices), chunked: no more
    than chunk x P distances at a time."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    best = 0.0
    for k in range(0, len(p), chunk):
        d = p[k:k + chunk, None, :] - p[None, :, :]
        best = max(best, float(np.sqrt((d * d).sum(axis=2).max())))
    return best


def bop_recall(errors, thresholds):
    """The mean over `thresholds` of the fraction of entries of `errors` (any shape) that are < the threshold: BOP's average
    recall of one pose-error function.  0 when there are no errors."""
    e = np.asarray(errors, np.float64).reshape(-1)
    th = np.asarray(thresholds, np.float64).reshape(-1)
    if e.size == 0:
        return 0.0
    return float(np.mean([np.count_nonzero(e < t) / e.size for t in th]))


def bop_average_recall(vsd, mssd, mspd, diameter, width):
    """BOP19's scores of one object's estimates: vsd [F, n_taus] (errors per tau), mssd [F] metres, mspd [F] pixels, the object's
    diameter (metres) and the image width.  VSD is correct when e < theta, theta in BOP_THRESHOLDS, averaged over taus x theta; MSSD
    when e < theta x diameter; MSPD when e < theta x width / 640, theta in BOP_MSPD_THRESHOLDS.
    Returns {"AR_VSD", "AR_MSSD", "AR_MSPD", "AR"}: AR the mean of the three."""
    out = {"AR_VSD": bop_recall(vsd, BOP_THRESHOLDS),
           "AR_MSSD": bop_recall(mssd, BOP_THRESHOLDS * float(diameter)),
           "AR_MSPD": bop_recall(mspd, BOP_MSPD_THRESHOLDS * (float(width) / 640.0))}
    out["AR"] = (out["AR_VSD"] + out["AR_MSSD"] + out["AR_MSPD"]) / 3.0
    return out


# ---- RMSE metrics of evaluation/metrics.py (the step right after the filtering path) -----------------------
def _rot_angle_deg(q_ref, q_sig):
    """Geodesic angle of R_ref R_sig^T in degrees (metrics.py:114-144)."""
    d = abs(float(np.dot(q_ref, q_sig))) / (np.linalg.norm(q_ref) * np.linalg.norm(q_sig))
    return np.degrees(2.0 * np.arccos(min(1.0, d)))


def rmse_cartesian_3d(ref_x, sig_x):
    """RMSE of the 3D position error in centimetres (metrics.py:102-111, 217-222)."""
    err = np.linalg.norm((np.asarray(ref_x) - np.asarray(sig_x)) * 100.0, axis=1)
    return float(np.linalg.norm(err) / np.sqrt(len(err)))


def rmse_angular(ref_q, sig_q):
    """RMSE of the orientation error in degrees (metrics.py:114-144, 243-248); quaternions (w,x,y,z)."""
    err = np.array([_rot_angle_deg(a, b) for a, b in zip(ref_q, sig_q)])
    return float(np.linalg.norm(err) / np.sqrt(len(err)))


def object_velocity_from_twist(twist, position):
    """The filter's linear velocity is that of the object point at the camera origin; the evaluation
    moves the pole to the object position before comparing: v = v_O + w x r (evaluate.py:514-521)."""
    twist = np.asarray(twist, float)
    out = twist.copy()
    out[:, :3] = twist[:, :3] + np.cross(twist[:, 3:], np.asarray(position, float))
    return out


def rmse_linear_velocity(ref_v, sig_v):
    """cm/s (metrics.py:165-174, 251-256)."""
    err = np.linalg.norm((np.asarray(ref_v) - np.asarray(sig_v)) * 100.0, axis=1)
    return float(np.linalg.norm(err) / np.sqrt(len(err)))


def rmse_angular_velocity(ref_w, sig_w):
    """deg/s (metrics.py:177-186, 259-264)."""
    err = np.linalg.norm(np.degrees(np.asarray(ref_w) - np.asarray(sig_w)), axis=1)
    return float(np.linalg.norm(err) / np.sqrt(len(err)))


def time_metrics(exec_ms):
    """Mean execution time and the number of frames above the 33 ms real-time budget (metrics.py:347-369)."""
    t = np.asarray(exec_ms, float)
    return float(t.mean()), int((t > 33.0).sum())


# ---- the reference's Metric interface (evaluation/metrics.py:20-369) ---------------------------------------------------
class Metric:
    """`Metric(name).evaluate(object_name, reference, signal, time)` as evaluation/evaluate.py calls it.  `reference` / `signal`:
    arrays whose rows are what evaluation/data_loader.py hands over -- poses `x y z axis angle` (7 columns) for the pose
    metrics, `v w` (6 columns) for the velocity metrics --, `time`: rows `[execution_ms, loading_ms]`; for the object name
    'ALL' all three are dicts name -> array and the rows of all objects are pooled (metrics.py:72-81).  `auc_points`: name ->
    [P, 3] model points for 'add' / 'adi' (the reference reads YCB_Video_Models/<name>/points.xyz, metrics.py:47-49).
    `backend`: where the ADD / ADD-S distances are computed, as in trajectory_adds ('cpu' by default)."""

    NAMES = ("rmse_cartesian_3d", "rmse_cartesian_x", "rmse_cartesian_y", "rmse_cartesian_z", "rmse_angular", "rmse_linear_velocity",
             "rmse_angular_velocity", "max_linear_velocity", "max_angular_velocity", "add", "adi", "time", "excess_33_ms")

    def __init__(self, name, auc_points=None, backend="cpu"):
        if name not in self.NAMES:
            raise ValueError("Metric " + name + " does not exist.")
        self.name = name
        self.auc_points = auc_points or {}
        self.backend = backend

    @staticmethod
    def _pool(object_name, x):
        if object_name == "ALL":
            return np.concatenate([np.asarray(x[k], float) for k in x], axis=0)
        return np.asarray(x, float)

    @staticmethod
    def _rot(aa):
        """axis (3) + angle -> rotation matrix, the axis used as given (pyquaternion normalises it; pose files hold unit axes)."""
        from .io import axis_angle_to_quat
        return quat_to_rot(axis_angle_to_quat(aa[:3], aa[3]))

    @staticmethod
    def _rms(err):
        return float(np.linalg.norm(err) / np.sqrt(err.shape[0]))

    def evaluate(self, object_name, reference, signal, time):
        n = self.name
        if n in ("time", "excess_33_ms"):
            t = self._pool(object_name, time)[:, 0]
            return float(t.mean()) if n == "time" else float((t > 33.0).sum())
        if n in ("add", "adi"):
            return self.auc(object_name, reference, signal, n)[1]
        ref, sig = self._pool(object_name, reference), self._pool(object_name, signal)
        if n == "rmse_cartesian_3d":
            return self._rms(np.linalg.norm((ref[:, :3] - sig[:, :3]) * 100.0, axis=1))                  # cm
        if n.startswith("rmse_cartesian_"):
            i = "xyz".index(n[-1])
            return self._rms((ref[:, i] - sig[:, i]) * 100.0)
        if n == "rmse_angular":
            err = np.empty(len(ref))
            for k in range(len(ref)):
                R = self._rot(ref[k, 3:7]) @ self._rot(sig[k, 3:7]).T
                err[k] = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))          # |log R|
            return self._rms(err)
        if n == "rmse_linear_velocity":
            return self._rms(np.linalg.norm((ref[:, :3] - sig[:, :3]) * 100.0, axis=1))                  # cm/s
        if n == "rmse_angular_velocity":
            return self._rms(np.linalg.norm(np.degrees(ref[:, 3:6] - sig[:, 3:6]), axis=1))              # deg/s
        if n == "max_linear_velocity":
            return float(np.linalg.norm(ref[:, :3], axis=1).max())                                       # of the REFERENCE (metrics.py:189-198)
        return float(np.degrees(np.linalg.norm(ref[:, 3:6], axis=1).max()))

    def auc(self, object_name, reference, signal, ad_name):
        """(distances, AUC x 100) of ADD ('add') or ADD-S ('adi'), pooled over the objects for 'ALL' (metrics.py:303-344)."""
        if object_name == "ALL":
            names = list(signal)
        else:
            names, signal, reference = [object_name], {object_name: signal}, {object_name: reference}
        dists = [self.distances(name, reference[name], signal[name], ad_name) for name in names]
        dists = np.concatenate(dists) if dists else np.zeros(0)
        return dists, auc(dists)

    @staticmethod
    def _poses(rows):
        """rows `x y z axis angle` -> [F, 7] `x y z q` (w x y z), converted once per trajectory."""
        from .io import axis_angle_to_quat
        rows = np.asarray(rows, float)
        out = np.empty((len(rows), 7))
        out[:, :3] = rows[:, :3]
        for k in range(len(rows)):
            out[k, 3:] = axis_angle_to_quat(rows[k, 3:6], rows[k, 6])
        return out

    def distances(self, name, reference, signal, ad_name):
        """Per-frame ADD ('add') or ADD-S ('adi') of one object's trajectory on auc_points[name]."""
        pts = np.asarray(self.auc_points[name], float)
        n = min(len(reference), len(signal))   # (rows are paired as far as both go)
        return _trajectory(ad_name, self._poses(signal[:n]), self._poses(reference[:n]), pts, self.backend)

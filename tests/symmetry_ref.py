"""Symmetric objects (include/roft_engine.h section 3h) restated in numpy, in the operation order the header states: the selection of
the equivalent pose nearest to a belief, and BOP's MSSD / MSPD.  Python floats are IEEE doubles and every product and sum below is
one rounded operation, so the selection rule is comparable bit for bit with roft_pose_nearest_equivalent.  Also the groups, the
flips and the streams the CPU and the GPU tests of the feature share."""
import copy
import math

import numpy as np

IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


# ---- the selection rule ---------------------------------------------------------------------------------------------------
def quat_mul(a, b):
    """Hamilton product, w x y z, the four terms of a component summed left to right"""
    a0, a1, a2, a3 = (float(v) for v in a)
    b0, b1, b2, b3 = (float(v) for v in b)
    return [a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
            a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
            a0 * b2 - a1 * b3 + a2 * b0 + a3 * b1,
            a0 * b3 + a1 * b2 - a2 * b1 + a3 * b0]


def quat_dot(a, b):
    return float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2]) + float(a[3]) * float(b[3])


def quat_to_rot(q):
    w, x, y, z = (float(v) for v in q)
    return [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
            2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
            2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]


def closeness(sym, qh, m):
    """c_g = | qh . (m (x) g) | of every element (a NaN counts as -1)"""
    out = []
    for el in np.asarray(sym, float).reshape(-1, 7):
        c = abs(quat_dot(qh, quat_mul(m, el[3:])))
        out.append(c if c == c else -1.0)
    return out


def nearest_equivalent(sym, qh, x, m):
    """(x', m', g*) of the rule; g* = 0 returns the inputs themselves"""
    sym = np.asarray(sym, float).reshape(-1, 7)
    c = closeness(sym, qh, m)
    best = 0
    for g in range(1, len(c)):
        if c[g] > c[best]:          # (the lowest index wins a tie)
            best = g
    if best == 0:
        return np.array(x, float), np.array(m, float), 0
    p = quat_mul(m, sym[best, 3:])
    if quat_dot(qh, p) < 0.0:
        p = [-v for v in p]
    R = quat_to_rot(m)
    t = [float(v) for v in sym[best, :3]]
    xo = [float(x[i]) + (R[3 * i] * t[0] + R[3 * i + 1] * t[1] + R[3 * i + 2] * t[2]) for i in range(3)]
    return np.array(xo), np.array(p), best


# ---- MSSD / MSPD ------------------------------------------------------------------------------------------------------------
def _move(R, t, p):
    return [R[3 * i] * p[0] + R[3 * i + 1] * p[1] + R[3 * i + 2] * p[2] + t[i] for i in range(3)]


def max_sym_distance(kind, pts, est, ref, sym, cam=None):
    """One pose pair: sqrt(min_g max_i d_i^2); a = R_r (R_g p + t_g) + t_r, b = R_e p + t_e; kind 'mssd' or 'mspd' (cam = fx, fy,
    cx, cy; +inf when a point has Z <= 0 on either side under any element).  np.max / np.minimum keep a NaN."""
    p = np.asarray(pts, float).reshape(-1, 3).T
    est, ref = np.asarray(est, float), np.asarray(ref, float)
    b = _move(quat_to_rot(est[3:]), est[:3], p)
    bad = False
    if kind == "mspd":
        fx, fy, cx, cy = cam
        bad = not np.all(b[2] > 0.0)
    best = np.inf
    with np.errstate(all="ignore"):
        for el in np.asarray(sym, float).reshape(-1, 7):
            a = _move(quat_to_rot(ref[3:]), ref[:3], _move(quat_to_rot(el[3:]), el[:3], p))
            if kind == "mspd":
                bad = bad or not np.all(a[2] > 0.0)
                du = (fx * b[0] / b[2] + cx) - (fx * a[0] / a[2] + cx)
                dv = (fy * b[1] / b[2] + cy) - (fy * a[1] / a[2] + cy)
                d = du * du + dv * dv
            else:
                dx, dy, dz = b[0] - a[0], b[1] - a[1], b[2] - a[2]
                d = dx * dx + dy * dy + dz * dz
            best = np.minimum(best, np.max(d))
    return np.inf if bad else float(np.sqrt(best))


def pose_errors_sym(kind, pts, est, ref, sym, cam=None):
    est, ref = np.asarray(est, float).reshape(-1, 7), np.asarray(ref, float).reshape(-1, 7)
    return np.array([max_sym_distance(kind, pts, est[f], ref[f], sym, cam) for f in range(len(est))])


# ---- groups -----------------------------------------------------------------------------------------------------------------
def half_turn(axis, centre=(0.0, 0.0, 0.0)):
    """the 180 degree rotation about coordinate axis `axis` (0, 1, 2) through `centre`: exact entries, t = c - R c"""
    q = [0.0, 0.0, 0.0, 0.0]
    q[1 + axis] = 1.0
    c = np.asarray(centre, float)
    Rc = np.array([c[i] if i == axis else -c[i] for i in range(3)])
    return list(c - Rc) + q


def d2_group():
    """a box's D2 group: the identity and the half turns about its three axes, no translation"""
    return np.array([IDENTITY, half_turn(0), half_turn(1), half_turn(2)])


def cyclic_group(n, axis=(0.0, 0.0, 1.0)):
    """n rotations about an axis through the origin (n = 16 is the filter's cap)"""
    ax = np.asarray(axis, float) / np.linalg.norm(axis)
    out = [list(IDENTITY)]
    for k in range(1, n):
        h = math.pi * k / n
        out.append([0.0, 0.0, 0.0, math.cos(h)] + list(math.sin(h) * ax))
    return np.array(out)


def flip_pose(x, q, el):
    """the pose (x, q) right-multiplied by a group element: (x + R(q) t, q (x) g) -- the equivalent pose a source may deliver"""
    R = np.array(quat_to_rot(q)).reshape(3, 3)
    return np.asarray(x, float) + R @ np.asarray(el[:3], float), np.array(quat_mul(q, el[3:]))


# ---- the setting of tests/test_symmetry_gpu.py, whose condition tests/test_symmetry_cpu.py shows with the oracle alone ----------
N_FRAMES = 20            # pose deliveries at frames 0, 6, 12, 18
SCALE = 4                # 160 x 120, the smallest camera of the engine tests
SEEDS = (7300, 7301, 7302)
OFFSET_B = np.array([0.0078125, -0.015625, 0.01953125])   # B's mesh origin is displaced by this much (metres; exact in float32)
OVER = dict(use_pose_resync=1, outlier_rejection=1)


def groups():
    """A: D2, B: the half turn about z through OFFSET_B's image in the displaced mesh (t = c - R c != 0), C: none"""
    return [d2_group(), np.array([IDENTITY, half_turn(2, OFFSET_B)]), None]


def streams():
    """three streams (objects A, B, C) without pose outliers and drops.  B's mesh is displaced by OFFSET_B and its poses moved so
    that it is the same body in the same place: x_B = x - R(q) c."""
    import util
    out = [util.stream(s, N_FRAMES, scale=SCALE, pose_outlier_prob=0.0, pose_drop_prob=0.0) for s in SEEDS]
    b = copy.copy(out[1])
    verts, tris = b.mesh
    b.mesh = (np.ascontiguousarray(verts + OFFSET_B.astype(np.float32)), tris)
    c = OFFSET_B
    b.pose_meas = b.pose_meas.copy()
    for k in range(len(b.pose_meas)):
        if b.pose_valid[k]:
            b.pose_meas[k, :3] -= np.array(quat_to_rot(b.pose_meas[k, 3:])).reshape(3, 3) @ c
    out[1] = b
    return out


def flip_schedule(n_elements, n_deliveries, seed):
    """the element each delivery is flipped by, from a seeded generator: every element at least once when there are enough
    deliveries (a permutation of the elements first), then uniform draws"""
    rng = np.random.default_rng(seed)
    order = list(rng.permutation(n_elements))
    while len(order) < n_deliveries:
        order.append(int(rng.integers(n_elements)))
    return [int(g) for g in order[:n_deliveries]]


def flipped(st, group, seed):
    """(a copy of the stream whose delivered poses are right-multiplied by drawn elements, {frame: element index})"""
    f = copy.copy(st)
    f.pose_meas = st.pose_meas.copy()
    frames = [k for k in range(len(st.pose_valid)) if st.pose_valid[k]]
    sched = flip_schedule(len(group), len(frames), seed)
    used = {}
    for k, g in zip(frames, sched):
        used[k] = g
        if g:
            x, q = flip_pose(st.pose_meas[k, :3], st.pose_meas[k, 3:], group[g])
            f.pose_meas[k, :3], f.pose_meas[k, 3:] = x, q
    return f, used


def initial_pose(st):
    """the CLEAN first pose: what every engine and oracle of the setting starts from (roft_amd.synth.initial_pose_from_stream)"""
    m = np.zeros(13)
    m[6:9], m[9:13] = st.pose_meas[0, :3], st.pose_meas[0, 3:]
    return m


def run_oracle(ob, st, fed=None, n_frames=N_FRAMES):
    """the oracle tracker started from st's clean first pose and fed the poses of `fed` (default: st's own)"""
    import util
    fed = fed if fed is not None else st
    cfg = util.oracle_config(ob, st, **OVER)
    trk = ob.Tracker(cfg, *st.mesh)
    out = []
    for k in range(n_frames):
        depth, flow, mask, pose = util.frame_inputs(fed, k)
        r = trk.step(st.dt, depth, flow, mask, pose)
        out.append(dict(pose=np.array(r.pose), twist=np.array(r.twist), n=r.n_flow_points, sel=r.outlier_selected,
                        L=np.array(r.outlier_L), mask=trk.mask()))
    trk.close()
    return out


def remedied(st_flipped, group, ref_clean, p0):
    """the flipped stream with every delivered pose replaced by what the selection rule returns for it, qh = the clean oracle's
    estimate of the frame before (the initial pose at frame 0); `nearest`: (sym, qh, x, q) -> (x', q', g)"""
    def apply(nearest):
        f = copy.copy(st_flipped)
        f.pose_meas = st_flipped.pose_meas.copy()
        chosen = {}
        for k in range(len(f.pose_valid)):
            if not f.pose_valid[k]:
                continue
            qh = p0[9:13] if k == 0 else ref_clean[k - 1]["pose"][9:13]
            x, q, g = nearest(group, qh, f.pose_meas[k, :3], f.pose_meas[k, 3:])
            f.pose_meas[k, :3], f.pose_meas[k, 3:] = x, q
            chosen[k] = g
        return f, chosen
    return apply

"""Operator-level host API over the C ABI: one function per reference operator, numpy in / out.

Names follow the reference's classes (hsp-iit/roft `src/roft-lib`):
  flow_measurement  <- ImageOpticalFlowMeasurement<T>::freeze
  kf_predict        <- bfl::KFPrediction(SpatialVelocityModel)
  skf_correct       <- SKFCorrection::correctStep
  mask_propagate    <- ImageSegmentationOFAidedSource<T>::map + cv::remap
  ukf_predict       <- bfl::UKFPrediction(CartesianQuaternionModel)
  ukf_correct       <- ROFT::UKFCorrection::correctStep(CartesianQuaternionMeasurement)
  render_depth      <- SICAD::superimpose(..., depth)
  depth_likelihood  <- ROFTFilter::pick_best_alternative (inner loop)
  optical_flow      <- ImageOpticalFlowNVOF::step_frame (the product contract; the algorithm is this project's own)
  pose_errors       <- add / adi of tools/third_party/bop_pose_error.py (the evaluation's ADD / ADD-S)
  render_scene      <- the evaluation's video / thumbnail renders (evaluation/results_renderer.py, tools/object_renderer)
All of them run on the GPU; none has a CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def mesh_of(verts, tris):
    """Arrays of any layout or dtype -> (L.Mesh, the C-contiguous (verts [n, 3] float32, tris [m, 3] int32) it points into: keep them)."""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    return L.Mesh(verts.ctypes.data, verts.shape[0], tris.ctypes.data, tris.shape[0]), (verts, tris)


def _mesh_array(meshes):
    """[(verts, tris), ...] -> (Mesh array, the arrays it points into)."""
    keep, arr = [], (L.Mesh * max(len(meshes), 1))()
    for k, (v, t) in enumerate(meshes):
        arr[k], arrays = mesh_of(v, t)
        keep.append(arrays)
    return arr, keep


def make_flow(arr, width):
    assert arr.flags["C_CONTIGUOUS"] and arr.ndim == 3 and arr.shape[2] == 2
    if arr.dtype == np.int16:
        typ, scale = L.FLOW_S16C2, 32.0
    elif arr.dtype == np.float32:
        typ, scale = L.FLOW_F32C2, 1.0
    else:
        raise TypeError("flow must be int16 (CV_16SC2) or float32 (CV_32FC2)")
    rows, cols = arr.shape[:2]
    return L.Flow(arr.ctypes.data, typ, cols, rows, width // cols, scale, 1)


def flow_measurement(cam, prev_mask, prev_depth, flow_arr, dt, radius=35.0, depth_max=2.0):
    H, W = prev_mask.shape
    cap = H * W // max(int(radius), 1) + 16
    uv = np.zeros((cap, 2), np.int32)
    y = np.zeros(2 * cap)
    Hm = np.zeros((2 * cap, 6))
    n = C.c_int(0)
    fl = make_flow(flow_arr, W)
    prev_mask = np.ascontiguousarray(prev_mask, np.uint8)
    prev_depth = np.ascontiguousarray(prev_depth, np.float32)
    L.check(L.lib().roft_flow_measurement(C.byref(cam), _p(prev_mask), _p(prev_depth), C.byref(fl), dt,
                                          np.float32(radius), depth_max, cap, _p(uv), _p(y), _p(Hm), C.byref(n)))
    n = n.value
    return n, uv[:n].copy(), y[:2 * n].copy(), Hm[:2 * n].copy()


def kf_predict(x, P, qdiag):
    x, P, qdiag = _f64(x), _f64(P), _f64(qdiag)
    xo, Po = np.zeros(6), np.zeros((6, 6))
    L.check(L.lib().roft_kf_predict(_p(x), _p(P), _p(qdiag), _p(xo), _p(Po)))
    return xo, Po


def skf_correct(x, P, y, Hm, rdiag=(1.0, 1.0), reweight=True):
    x, P, y, Hm, rd = _f64(x), _f64(P), _f64(y), _f64(Hm), _f64(rdiag)
    n = y.size // 2
    xo, Po = np.zeros(6), np.zeros((6, 6))
    st = C.c_int(0)
    L.check(L.lib().roft_skf_correct(_p(x), _p(P), n, _p(y), _p(Hm), _p(rd), int(reweight), _p(xo), _p(Po),
                                     C.byref(st)))
    return st.value, xo, Po


def skf_correct_points(cam, dt, x, P, uv, z, flow_xy, rdiag=(1.0, 1.0), reweight=True):
    """SKFCorrection::correctStep fed with the kept flow points (the engine's form: H rows rebuilt on the device)."""
    x, P, rd = _f64(x), _f64(P), _f64(rdiag)
    uv = np.ascontiguousarray(uv, np.int32)
    z = np.ascontiguousarray(z, np.float32)
    fxy = np.ascontiguousarray(flow_xy, np.float32)
    n = z.size
    xo, Po = np.zeros(6), np.zeros((6, 6))
    st = C.c_int(0)
    L.check(L.lib().roft_skf_correct_points(C.byref(cam), dt, _p(x), _p(P), n, _p(uv), _p(z), _p(fxy), _p(rd),
                                            int(reweight), _p(xo), _p(Po), C.byref(st)))
    return st.value, xo, Po


def mask_propagate(mask, flow_arrs, frames_between=6):
    mask = np.ascontiguousarray(mask, np.uint8).copy()
    H, W = mask.shape
    arr = (L.Flow * max(1, len(flow_arrs)))()
    for i, f in enumerate(flow_arrs):
        arr[i] = make_flow(f, W)
    L.check(L.lib().roft_mask_propagate(_p(mask), W, H, arr, len(flow_arrs), frames_between))
    return mask


def labels_to_masks(labels, values):
    """The masks {0, 255} [n, H, W] and pixel counts [n] of `values` in one label image (uint8 or uint16): mask i is
    (labels == values[i]) * 255, by the engine's own label ingest kernel (roft_labels_to_masks).  Values may repeat or be
    absent from the image; 0 (the background) is refused."""
    L.require_device()
    labels = np.ascontiguousarray(labels)
    if labels.dtype not in (np.uint8, np.uint16) or labels.ndim != 2:
        raise TypeError("a label image is a 2-D uint8 or uint16 array")
    H, W = labels.shape
    vals = np.ascontiguousarray(values, np.int32).reshape(-1)
    masks = np.zeros((len(vals), H, W), np.uint8)
    counts = np.zeros(len(vals), np.int32)
    L.check(L.lib().roft_labels_to_masks(_p(labels), L.LABEL_U8 if labels.dtype == np.uint8 else L.LABEL_U16, W, H,
                                         vals.ctypes.data_as(C.POINTER(C.c_int)), len(vals), _p(masks), counts.ctypes.data_as(C.POINTER(C.c_int))))
    return masks, counts


def pose_silhouette(cam, mesh, x, q, bands=0, vertex_cache=True):
    """The mask {0, 255} [H, W] and the pixel count of the silhouette of `mesh` at the pose (x, q = w x y z), by the
    engine's own kernel (roft_pose_silhouette; the contract: include/roft_engine.h, section 3e): a pixel is set where
    roft_render_depth at divider 1 is > 0.  bands 0: the library's choice of workgroups per image; vertex_cache False: the
    vertices are projected per triangle.  Neither changes a bit.
    mesh: (verts [n, 3], tris [m, 3]) arrays of any layout -- they are made float32 / int32 and C-contiguous here -- or an L.Mesh,
    whose pointers must name C-contiguous float32 / int32 memory (the address of a transposed or sliced array is not that)."""
    L.require_device()
    x, q = _f64(np.asarray(x).reshape(3)), _f64(np.asarray(q).reshape(4))
    if not isinstance(mesh, L.Mesh):
        mesh, keep = mesh_of(*mesh)
    mask = np.zeros((cam.height, cam.width), np.uint8)
    count = C.c_int(0)
    L.check(L.lib().roft_pose_silhouette(C.byref(cam), C.byref(mesh), _p(x), _p(q), int(bands), 1 if vertex_cache else 0, _p(mask), C.byref(count)))
    return mask, count.value


def pose_silhouettes_occluded(cam, meshes, xs, qs, bands=0, vertex_cache=True):
    """The masks {0, 255} [n, H, W] and the pixel counts [n] of n meshes of ONE scene at the poses (xs [n, 3], qs [n, 4] = w x y z),
    each keeping the pixels where it is the nearest surface -- the lower index on an exact tie -- by the engine's own kernels
    (roft_pose_silhouettes_occluded; the contract: include/roft_engine.h, section 3e).  bands and vertex_cache as for
    pose_silhouette: neither changes a bit.  meshes: a sequence of (verts, tris) array pairs, as for pose_silhouette."""
    L.require_device()
    n = len(meshes)
    xs, qs = _f64(np.asarray(xs).reshape(n, 3)), _f64(np.asarray(qs).reshape(n, 4))
    arr, keep = _mesh_array(meshes)
    masks = np.zeros((n, cam.height, cam.width), np.uint8)
    counts = np.zeros(n, np.int32)
    L.check(L.lib().roft_pose_silhouettes_occluded(C.byref(cam), arr, n, _p(xs), _p(qs), int(bands), 1 if vertex_cache else 0, _p(masks),
                                                   counts.ctypes.data_as(C.POINTER(C.c_int))))
    return masks, counts


def pose_silhouettes_gated(cam, meshes, xs, qs, depth, front_tolerance=0.02, behind_tolerance=0.0, bands=0, vertex_cache=True):
    """pose_silhouettes_occluded followed by the depth gate (roft_pose_silhouettes_gated; the contract: include/roft_engine.h, section
    3e): a pixel stays unless `depth` [H, W] float32 has a valid reading more than front_tolerance in front of the rendered surface,
    or (behind_tolerance > 0) more than behind_tolerance behind it.  With one mesh it is pose_silhouette followed by the gate.
    Returns masks {0, 255} [n, H, W], kept pixel counts [n] and removed [n, 2] = (front, behind)."""
    L.require_device()
    n = len(meshes)
    xs, qs = _f64(np.asarray(xs).reshape(n, 3)), _f64(np.asarray(qs).reshape(n, 4))
    depth = np.ascontiguousarray(depth, np.float32)
    if depth.shape != (cam.height, cam.width):
        raise ValueError("depth is an H x W image of the camera's size")
    arr, keep = _mesh_array(meshes)
    masks = np.zeros((n, cam.height, cam.width), np.uint8)
    counts = np.zeros(n, np.int32)
    removed = np.zeros((n, 2), np.int32)
    gate = L.PoseMaskGate(front_tolerance, behind_tolerance)
    ip = C.POINTER(C.c_int)
    L.check(L.lib().roft_pose_silhouettes_gated(C.byref(cam), arr, n, _p(xs), _p(qs), _p(depth), C.byref(gate), int(bands), 1 if vertex_cache else 0,
                                                _p(masks), counts.ctypes.data_as(ip), removed.ctypes.data_as(ip)))
    return masks, counts, removed


def process_noise(psd, sig_w, T):
    Q = np.zeros((9, 9))
    L.check(L.lib().roft_pose_process_noise(_p(_f64(psd)), _p(_f64(sig_w)), T, _p(Q)))
    return Q


def ukf_predict(mean, P, Q, T, ut=(1.0, 2.0, 0.0)):
    mean, P, Q = _f64(mean), _f64(P), _f64(Q)
    mo, Po = np.zeros(13), np.zeros((12, 12))
    u = L.UT(*ut)
    L.check(L.lib().roft_ukf_predict(_p(mean), _p(P), _p(Q), T, C.byref(u), _p(mo), _p(Po)))
    return mo, Po


def ukf_correct(mean, P, mtype, meas, rdiag, ut=(1.0, 2.0, 0.0)):
    mean, P, meas, rdiag = _f64(mean), _f64(P), _f64(meas), _f64(rdiag)
    mo, Po = np.zeros(13), np.zeros((12, 12))
    u = L.UT(*ut)
    st = C.c_int(0)
    L.check(L.lib().roft_ukf_correct(_p(mean), _p(P), mtype, _p(meas), _p(rdiag), C.byref(u), _p(mo), _p(Po),
                                     C.byref(st)))
    return st.value, mo, Po


def make_mesh(verts, tris):
    m, keep = mesh_of(verts, tris)
    m._keep = keep
    return m


def mesh_classify(verts, tris):
    """(closed, flip[n_tris]): is the mesh a closed orientable surface, which triangles are wound clockwise seen from outside
    (roft_mesh_classify: host code, the classification roft_object_add applies; rules in oracle/ro_meshclass.c)."""
    m = make_mesh(verts, tris)
    flip = np.zeros(max(m.n_tris, 1), np.uint8)
    closed = C.c_int(-1)
    L.check(L.lib().roft_mesh_classify(C.byref(m), _p(flip), C.byref(closed)))
    return bool(closed.value), flip[:m.n_tris]


def render_depth(mesh, x, q, cam, divider, mode=L.RENDER_CONTRACT):
    """mode: L.RENDER_CONTRACT (roft_render_depth) or L.RENDER_GL (the reference's GL numerics, roft_render_depth_mode)."""
    x, q = _f64(x), _f64(q)
    tile = np.zeros((cam.height // divider, cam.width // divider), np.float32)
    if mode == L.RENDER_CONTRACT:
        L.check(L.lib().roft_render_depth(C.byref(mesh), _p(x), _p(q), C.byref(cam), divider, _p(tile)))
    else:
        L.check(L.lib().roft_render_depth_mode(C.byref(mesh), _p(x), _p(q), C.byref(cam), divider, mode, _p(tile)))
    return tile


def depth_likelihood(cam, depth, mask, tile, divider):
    depth = np.ascontiguousarray(depth, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    tile = np.ascontiguousarray(tile, np.float32)
    Lv = C.c_double(0.0)
    ns = C.c_long(0)
    L.check(L.lib().roft_depth_likelihood(C.byref(cam), _p(depth), _p(mask), _p(tile), divider, C.byref(Lv),
                                          C.byref(ns)))
    return Lv.value, ns.value


def outlier_test(cam, divider, depth, mask, mesh, x2, q2, bands=0, vertex_cache=True, window_pixels=0, tiles=True, split=None,
                 mode=L.RENDER_CONTRACT):
    """ROFTFilter::pick_best_alternative (ROFTFilter.cpp:467-621) on the engine's own kernels (features_kernel,
    outlier_fused_kernel, the deciding pose chain segment).  x2 (2, 3), q2 (2, 4): the two alternatives.
    split: the workgroups of an alternative share its triangles (True) / the rows of its window (False); None: the library's choice.
    mode: L.RENDER_CONTRACT or L.RENDER_GL (the reference's GL numerics, roft_outlier_test_mode).
    Returns (L[2], samples[2], selected, tiles (2, H/d, W/d) or None)."""
    depth = np.ascontiguousarray(depth, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    x2, q2 = _f64(np.asarray(x2).reshape(6)), _f64(np.asarray(q2).reshape(8))
    Lv = np.zeros(2, np.float64)
    ns = np.zeros(2, np.int64)
    sel = C.c_int(-2)
    t = np.zeros((2, cam.height // divider, cam.width // divider), np.float32) if tiles else None
    # (split travels with the call -- roft_outlier_test_split -- not through a process-wide switch)
    sp = -1 if split is None else (1 if split else 0)
    if mode == L.RENDER_CONTRACT:
        L.check(L.lib().roft_outlier_test_split(C.byref(cam), divider, _p(depth), _p(mask), C.byref(mesh), _p(x2), _p(q2), bands,
                                                1 if vertex_cache else 0, window_pixels, sp, _p(Lv), _p(ns), C.byref(sel), _p(t) if tiles else None))
    else:
        L.check(L.lib().roft_outlier_test_mode(C.byref(cam), divider, _p(depth), _p(mask), C.byref(mesh), _p(x2), _p(q2), bands,
                                               1 if vertex_cache else 0, window_pixels, sp, mode, _p(Lv), _p(ns), C.byref(sel),
                                               _p(t) if tiles else None))
    return Lv, ns, sel.value, t


# numpy mirror of roft_quality_record (40 bytes)
QUALITY_DTYPE = np.dtype([("frame", np.int32), ("n_mask", np.int32), ("n_render", np.int32), ("n_both", np.int32), ("n_depth", np.int32),
                          ("n_front", np.int32), ("n_behind", np.int32), ("reserved", np.int32), ("depth_err", np.float64)])


def quality_overlap(rec):
    """Intersection over union of mask and render silhouette, n_both / (n_mask + n_render - n_both), of quality records (a structured
    array or one record); NaN where both are empty or there is no record."""
    rec = np.asarray(rec)
    union = rec["n_mask"].astype(np.float64) + rec["n_render"] - rec["n_both"]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((union > 0) & (rec["frame"] >= 0), rec["n_both"] / union, np.nan)


def track_quality(cam, divider, depth, mask, mesh, x, q, depth_tolerance=0.01, depth_maximum=2.0, window_pixels=0):
    """Silhouette overlap and depth residual of the pose (x, q) of `mesh` against a mask and a depth image, by the engine's own
    kernel on host buffers (roft_track_quality; the contract: include/roft_engine.h, section 3d).  mask: the pixels of value > 1 are
    the object.  window_pixels > 0 caps the kernel's LDS depth window (strips; no bit changes).  Returns one QUALITY_DTYPE record."""
    depth = np.ascontiguousarray(depth, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    x, q = _f64(np.asarray(x).reshape(3)), _f64(np.asarray(q).reshape(4))
    rec = L.QualityRecord()
    L.check(L.lib().roft_track_quality(C.byref(cam), divider, _p(depth), _p(mask), C.byref(mesh), _p(x), _p(q), float(depth_tolerance),
                                       float(depth_maximum), window_pixels, C.byref(rec)))
    return np.frombuffer(bytes(rec), QUALITY_DTYPE)[0].copy()


def hypothesis_poses(poses):
    """Candidate poses as the ABI takes them: [n, 7] float64 rows x y z, q = (w, x, y, z)."""
    poses = np.asarray(poses, np.float64)
    if poses.size % 7:
        raise ValueError("poses must hold 7 numbers per pose: x y z, q = (w, x, y, z)")
    return np.ascontiguousarray(poses.reshape(-1, 7))


def pose_hypotheses_score(cam, divider, depth, mask, mesh, poses, depth_tolerance=0.01, depth_maximum=2.0, window_pixels=0):
    """The track-quality record of each of n candidate poses [n, 7] (x y z, q = w x y z) of `mesh` against one mask and one depth
    image, in one launch (roft_pose_hypotheses_score; the contract: include/roft_engine.h, section 3j): entry i is, bit for bit,
    track_quality(..., poses[i, :3], poses[i, 3:], ...).  A pose with a non-finite component draws nothing.  Returns
    QUALITY_DTYPE[n]."""
    depth = np.ascontiguousarray(depth, np.float32)
    mask = np.ascontiguousarray(mask, np.uint8)
    poses = hypothesis_poses(poses)
    n = poses.shape[0]
    out = np.zeros(n, QUALITY_DTYPE)
    L.check(L.lib().roft_pose_hypotheses_score(C.byref(cam), divider, _p(depth), _p(mask), C.byref(mesh), _p(poses), n, float(depth_tolerance),
                                               float(depth_maximum), window_pixels, out.ctypes.data_as(C.POINTER(L.QualityRecord))))
    return out


POSE_ERROR_KINDS = {"add": L.POSE_ERROR_ADD, "adi": L.POSE_ERROR_ADDS, "adds": L.POSE_ERROR_ADDS,
                    "mssd": L.POSE_ERROR_MSSD, "mspd": L.POSE_ERROR_MSPD}


def pose_error_kind(kind):
    """'add' | 'adi' | 'adds' or L.POSE_ERROR_ADD | L.POSE_ERROR_ADDS -> the ABI's constant."""
    return POSE_ERROR_KINDS[kind] if isinstance(kind, str) else int(kind)


def pose_errors(kind, points, est, ref):
    """ADD ('add') or ADD-S ('adi' / 'adds') of F pose pairs over one point set, in double precision on the device
    (roft_pose_errors).  points [P, 3]; est, ref [F, 7] rows x y z, q = (w, x, y, z), the quaternion used as given.
    Returns ndarray[F] (metres); a non-finite pose gives a non-finite entry."""
    points = _f64(points).reshape(-1, 3)
    est, ref = _f64(est).reshape(-1, 7), _f64(ref).reshape(-1, 7)
    if est.shape != ref.shape:
        raise ValueError("est and ref must hold the same number of poses")
    out = np.zeros(est.shape[0])
    L.check(L.lib().roft_pose_errors(pose_error_kind(kind), _p(points), points.shape[0], _p(est), _p(ref), est.shape[0], _p(out)))
    return out


def symmetry_elements(symmetries):
    """A symmetry group as the ABI takes it: [n, 7] float64 rows x y z, q = (w, x, y, z), element 0 the identity.  None: the
    identity alone."""
    if symmetries is None:
        return np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
    return _f64(symmetries).reshape(-1, 7)


def pose_nearest_equivalent(symmetries, qh, x, q):
    """The pose equivalent to (x, q) under the object's symmetry group that is nearest to the belief quaternion qh
    (roft_pose_nearest_equivalent: the rule of the pose UKF in host arithmetic -- no device is needed).
    Returns (x' [3], q' [4], index of the chosen element); index 0 returns the input's bits."""
    sym = symmetry_elements(symmetries)
    qh, x, q = _f64(qh).reshape(4), _f64(x).reshape(3), _f64(q).reshape(4)
    x_out, q_out, index = np.zeros(3), np.zeros(4), C.c_int(-1)
    L.check(L.lib().roft_pose_nearest_equivalent(_p(sym), sym.shape[0], _p(qh), _p(x), _p(q), _p(x_out), _p(q_out), C.byref(index)))
    return x_out, q_out, index.value


def pose_errors_sym(kind, points, est, ref, symmetries=None, cam=None):
    """MSSD ('mssd', metres) or MSPD ('mspd', pixels; cam = L.Camera or (fx, fy, cx, cy)) of F pose pairs over one point set under
    a symmetry group [n, 7], on the device (roft_pose_errors_sym).  Shapes as pose_errors.  Returns ndarray[F]."""
    points = _f64(points).reshape(-1, 3)
    est, ref = _f64(est).reshape(-1, 7), _f64(ref).reshape(-1, 7)
    if est.shape != ref.shape:
        raise ValueError("est and ref must hold the same number of poses")
    sym = symmetry_elements(symmetries)
    if cam is not None and not isinstance(cam, L.Camera):
        fx, fy, cx, cy = (float(v) for v in cam)
        cam = L.Camera(0, 0, fx, fy, cx, cy)
    out = np.zeros(est.shape[0])
    L.check(L.lib().roft_pose_errors_sym(pose_error_kind(kind), _p(points), points.shape[0], _p(est), _p(ref), est.shape[0], _p(sym),
                                         sym.shape[0], None if cam is None else C.byref(cam), _p(out)))
    return out


def vsd_params(delta=0.015, taus=None, diameter=None, window_pixels=0):
    """roft_vsd_params: taus None -> np.arange(0.05, 0.51, 0.05); diameter None -> 0 (distances are not normalised)."""
    taus = np.arange(0.05, 0.51, 0.05) if taus is None else _f64(taus).reshape(-1)
    if len(taus) > L.VSD_MAX_TAUS:
        raise ValueError("at most %d taus" % L.VSD_MAX_TAUS)
    p = L.VsdParams()
    p.delta, p.n_taus = float(delta), len(taus)
    for k, t in enumerate(taus):
        p.taus[k] = float(t)
    p.diameter = 0.0 if diameter is None else float(diameter)
    p.window_pixels = int(window_pixels)
    return p


def pose_errors_vsd(cam, mesh, est, ref, depth, delta=0.015, taus=None, diameter=None, window_pixels=0, counts=False):
    """BOP's Visible Surface Discrepancy of F pose pairs of one mesh against depth images, on the device (roft_pose_errors_vsd; the
    contract: include/roft_engine.h, section 3i).  cam: L.Camera; mesh: make_mesh(verts, tris); est, ref [F, 7] rows x y z,
    q = (w, x, y, z); depth [F, H, W] float32 metres (0: no measurement), or [H, W] / [1, H, W]: one image under every pair.
    taus in object diameters when `diameter` is given, else in metres.  window_pixels > 0 caps the kernel's LDS depth windows
    (strips; no bit changes).  Returns errors [F, n_taus]; with counts=True also int32 [F, 4 + n_taus]: n_union, n_inter, n_gt,
    n_est, fail[0 .. n_taus)."""
    est, ref = _f64(est).reshape(-1, 7), _f64(ref).reshape(-1, 7)
    if est.shape != ref.shape:
        raise ValueError("est and ref must hold the same number of poses")
    depth = np.ascontiguousarray(depth, np.float32)
    if depth.ndim == 2:
        depth = depth[None]
    if depth.ndim != 3 or depth.shape[1:] != (cam.height, cam.width):
        raise ValueError("depth must be [F, H, W] or [H, W] of the camera's size")
    p = vsd_params(delta, taus, diameter, window_pixels)
    n = est.shape[0]
    errors = np.zeros((n, p.n_taus))
    rows = np.zeros((n, 4 + p.n_taus), np.int32) if counts else None
    L.check(L.lib().roft_pose_errors_vsd(C.byref(cam), C.byref(mesh), _p(est), _p(ref), n, _p(depth), depth.shape[0], C.byref(p),
                                         _p(errors), _p(rows) if counts else None))
    return (errors, rows) if counts else errors


def pose_errors_kernel_ms():
    """Device time (ms, HIP events) of the kernels of the last pose_errors call, without its copies."""
    ms = C.c_double(0.0)
    L.check(L.lib().roft_debug_pose_errors_kernel_ms(C.byref(ms)))
    return ms.value


def of_params(levels=3, radius=3, iterations=3, det_min=100.0):
    p = L.OFParams()
    L.check(L.lib().roft_default_of_params(C.byref(p)))
    p.levels, p.radius, p.iterations, p.det_min = levels, radius, iterations, det_min
    return p


def of_consistency(consistency):
    """The forward-backward check's tolerances (L.OFConsistency) of a `consistency` argument: None / False -> None (no check),
    True -> the library's defaults, (tolerance_abs, tolerance_rel) -> those."""
    if consistency is None or consistency is False:
        return None
    c = L.OFConsistency()
    if not hasattr(L.lib(), "roft_optical_flow_checked"):
        raise L.RoftError("this libroft_hip.so has no forward-backward check (roft_optical_flow_checked)")
    L.check(L.lib().roft_default_of_consistency(C.byref(c)))
    if consistency is not True:
        c.tolerance_abs, c.tolerance_rel = (float(v) for v in consistency)
    return c


def optical_flow(prev_gray, cur_gray, flow_type=L.FLOW_F32C2, consistency=None, **kw):
    """Forward flow of `prev_gray` pixels towards `cur_gray` (u8, H x W).  CV_32FC2: float (H, W, 2); CV_16SC2: int16
    (H/4, W/4, 2) S10.5 -- the two products of ImageOpticalFlowNVOF.cpp:19-80.  consistency: None, True (default tolerances) or
    (tolerance_abs, tolerance_rel) -- the forward-backward check of include/roft_engine.h section 3f, whose invalid pixels are NaN
    (CV_32FC2 only)."""
    prev = np.ascontiguousarray(prev_gray, np.uint8)
    cur = np.ascontiguousarray(cur_gray, np.uint8)
    if prev.shape != cur.shape or prev.ndim != 2:
        raise ValueError("two gray images of the same shape expected")
    H, W = prev.shape
    out = np.zeros((H, W, 2), np.float32) if flow_type == L.FLOW_F32C2 else np.zeros((H // 4, W // 4, 2), np.int16)
    p = of_params(**kw)
    c = of_consistency(consistency)
    if c is None:
        L.check(L.lib().roft_optical_flow(_p(prev), _p(cur), W, H, C.byref(p), flow_type, _p(out)))
    elif flow_type != L.FLOW_F32C2:
        raise ValueError("consistency needs flow_type FLOW_F32C2: CV_16SC2 has no representation of an invalid vector")
    else:
        L.check(L.lib().roft_optical_flow_checked(_p(prev), _p(cur), W, H, C.byref(p), C.byref(c), _p(out)))
    return out


def image_to_gray(image, image_type=None):
    """The gray image (H x W uint8) of an 8-bit camera image by the device's conversion (roft_image_to_gray): OpenCV's fixed-point
    COLOR_BGR2GRAY.  image: [H, W] (gray, passes through) or [H, W, 3]; image_type L.IMAGE_BGR8 / L.IMAGE_RGB8 (default RGB8,
    the order PNG stores)."""
    img = np.ascontiguousarray(image, np.uint8)
    if img.ndim == 2:
        image_type = L.IMAGE_GRAY8 if image_type is None else image_type
    elif img.ndim == 3 and img.shape[2] == 3:
        image_type = L.IMAGE_RGB8 if image_type is None else image_type
    else:
        raise ValueError("an [H, W] or [H, W, 3] uint8 image expected")
    H, W = img.shape[:2]
    out = np.zeros((H, W), np.uint8)
    L.check(L.lib().roft_image_to_gray(_p(img), image_type, W, H, _p(out)))
    return out


def depth_source(scale=0.001, cam=None, R=None, t=None):
    """L.DepthSource of a Z16 sensor: `scale` metres per unit.  cam None: the frames are already in the colour camera (align 0).
    Otherwise cam is the DEPTH camera (L.Camera, or anything with width, height, fx, fy, cx, cy) and P_colour = R P_depth + t
    (R [3, 3] row-major, default identity; t metres, default 0)."""
    src = L.DepthSource()
    src.type, src.scale, src.align = L.DEPTH_Z16, float(scale), 0 if cam is None else 1
    if cam is not None:
        src.cam = L.Camera(int(cam.width), int(cam.height), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy))
    src.R = (C.c_float * 9)(*np.asarray(np.eye(3) if R is None else R, np.float32).reshape(9))
    src.t = (C.c_float * 3)(*np.asarray(np.zeros(3) if t is None else t, np.float32).reshape(3))
    return src


def _raw_depth(raw):
    raw = np.ascontiguousarray(raw)
    if raw.dtype != np.uint16 or raw.ndim != 2:
        raise TypeError("a raw depth frame is [H, W] uint16")
    return raw


def depth_convert(raw, scale=0.001):
    """The float depth image (metres, [H, W] float32) of a 16-bit depth frame by the device's conversion (roft_depth_convert):
    (float)raw * scale, 0 stays 0."""
    raw = _raw_depth(raw)
    out = np.zeros(raw.shape, np.float32)
    L.check(L.lib().roft_depth_convert(_p(raw), raw.shape[1], raw.shape[0], float(scale), _p(out)))
    return out


def depth_align(raw, depth_cam, colour_cam, scale=0.001, R=None, t=None):
    """A 16-bit frame of the depth camera registered to the colour camera (roft_depth_align; the contract is in
    include/roft_engine.h section 3c): [colour H, colour W] float32 metres, 0 where no reading lands."""
    raw = _raw_depth(raw)
    if raw.shape != (depth_cam.height, depth_cam.width):
        raise ValueError("the raw frame does not have the depth camera's size")
    src = depth_source(scale, depth_cam, R, t)
    col = L.Camera(int(colour_cam.width), int(colour_cam.height), float(colour_cam.fx), float(colour_cam.fy), float(colour_cam.cx), float(colour_cam.cy))
    out = np.zeros((col.height, col.width), np.float32)
    L.check(L.lib().roft_depth_align(_p(raw), C.byref(src), C.byref(col), _p(out)))
    return out


def _camera(cam):
    return L.Camera(int(cam.width), int(cam.height), float(cam.fx), float(cam.fy), float(cam.cx), float(cam.cy))


def lens(cam, dist=(0.0, 0.0, 0.0, 0.0, 0.0)):
    """L.Lens of a sensor: cam is the SOURCE camera (L.Camera, or anything with width, height, fx, fy, cx, cy), dist its
    Brown-Conrady coefficients (k1, k2, p1, p2, k3) in OpenCV's order."""
    if isinstance(cam, L.Lens):
        return cam
    if hasattr(cam, "cam") and hasattr(cam, "k1"):     # anything shaped like a lens: cam, k1, k2, p1, p2, k3
        cam, dist = cam.cam, (cam.k1, cam.k2, cam.p1, cam.p2, cam.k3)
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    return L.Lens(_camera(cam), k1, k2, p1, p2, k3)


# the kind of an image by its dtype and shape, for ops.rectify: 8-bit images are resampled bilinearly unless nearest is asked for
def _rectify_kind(img, nearest):
    if img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and not nearest:
        return L.RECTIFY_RGB8
    if img.ndim != 2:
        raise TypeError("an image to rectify is [H, W] uint8 / uint16 / float32 or [H, W, 3] uint8")
    if img.dtype == np.uint8:
        return L.RECTIFY_U8 if nearest else L.RECTIFY_GRAY8
    if img.dtype == np.uint16:
        return L.RECTIFY_U16
    if img.dtype == np.float32:
        return L.RECTIFY_F32
    raise TypeError("an image to rectify is uint8, uint16 or float32, not %s" % img.dtype)


def rectify_map(source_lens, target_cam):
    """The map of roft_rectify_map (include/roft_engine.h section 3g): [H, W, 2] float32 (sx, sy), where in the distorted source
    image each pixel of the pinhole camera `target_cam` reads.  source_lens: ops.lens(...)."""
    ln, tgt = lens(source_lens), _camera(target_cam)
    out = np.zeros((tgt.height, tgt.width, 2), np.float32)
    L.check(L.lib().roft_rectify_map(C.byref(ln), C.byref(tgt), _p(out)))
    return out


def rectify(image, source_lens, target_cam, nearest=None, kind=None):
    """The distorted image of the sensor `source_lens` (ops.lens) resampled into the pinhole camera `target_cam` by the device
    (roft_rectify).  uint16 and float32 images (depth, labels) are sampled NEAREST; uint8 [H, W] images bilinearly unless
    nearest=True (masks, label images); [H, W, 3] uint8 bilinearly per channel.  kind: an L.RECTIFY_* value instead."""
    img = np.ascontiguousarray(image)
    ln, tgt = lens(source_lens), _camera(target_cam)
    if kind is None:
        kind = _rectify_kind(img, bool(nearest))
    if img.shape[:2] != (ln.cam.height, ln.cam.width):
        raise ValueError("the image does not have the source camera's size")
    out = np.zeros((tgt.height, tgt.width) + img.shape[2:], img.dtype)
    L.check(L.lib().roft_rectify(_p(img), int(kind), C.byref(ln), C.byref(tgt), _p(out)))
    return out


class FlowProducer:
    """Batched device-resident producer (roft_flow_producer_*): `run` takes lists of device pointers."""

    def __init__(self, width, height, max_pairs, flow_type=L.FLOW_F32C2, device=0, consistency=None, **kw):
        self._h = C.c_void_p()
        self.width, self.height, self.max_pairs, self.flow_type = width, height, max_pairs, flow_type
        p = of_params(**kw)
        L.check(L.lib().roft_flow_producer_create(width, height, max_pairs, C.byref(p), flow_type, device, C.byref(self._h)))
        if consistency is not None and consistency is not False:
            try:
                self.set_consistency(consistency)
            except L.RoftError:
                self.close()
                raise

    def set_consistency(self, consistency):
        """The forward-backward check for every later run (ops.optical_flow's `consistency`); None turns it off again."""
        c = of_consistency(consistency)
        L.check(L.lib().roft_flow_producer_set_consistency(self._h, None if c is None else C.byref(c)))

    def run(self, prev_ptrs, cur_ptrs, out_ptrs):
        n = len(prev_ptrs)
        arr = C.c_void_p * n
        L.check(L.lib().roft_flow_producer_run(self._h, arr(*prev_ptrs), arr(*cur_ptrs), arr(*out_ptrs), n))

    def sync(self):
        L.check(L.lib().roft_flow_producer_sync(self._h))

    @property
    def stream(self):
        return L.lib().roft_flow_producer_stream(self._h)

    def close(self):
        if self._h:
            L.lib().roft_flow_producer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- scene renderer (roft_scene_renderer_*, roft_render_scene) --------------------------------------------------
SCENE_OUTPUTS = ("rgb", "depth", "instance", "triangle")


def _scene_desc(width, height, mesh_index, poses, valid, background, gray_background, styles, window_pixels):
    """The description of a call and the arrays it points into.  poses [F, I, 7] (or [F, 7] with one instance)."""
    mesh_index = np.ascontiguousarray(mesh_index, np.int32).reshape(-1)
    n_inst = mesh_index.shape[0]
    poses = _f64(poses)
    poses = poses.reshape(-1, n_inst, 7) if n_inst else poses.reshape(poses.shape[0] if poses.ndim else 0, 0, 7)
    n_frames = poses.shape[0]
    d = L.SceneDesc()
    d.n_frames, d.n_instances = n_frames, n_inst
    d.mesh_index, d.poses = mesh_index.ctypes.data, poses.ctypes.data
    keep = [mesh_index, poses]
    if valid is not None:
        valid = np.ascontiguousarray(np.asarray(valid) != 0, np.uint8).reshape(n_frames, n_inst)
        d.valid = valid.ctypes.data
        keep.append(valid)
    if background is not None:
        background = np.ascontiguousarray(background, np.uint8)
        if background.ndim == 3:
            background = background[None]
        if background.shape[1:] != (height, width, 3) or background.shape[0] not in (1, n_frames):
            raise ValueError("background must be [H, W, 3] or [n_frames, H, W, 3] uint8")
        d.background, d.background_frames = background.ctypes.data, background.shape[0]
        keep.append(background)
    d.gray_background = 1 if gray_background else 0
    if styles is not None:
        if len(styles) != n_inst:
            raise ValueError("one style per instance")
        arr = (L.SceneStyle * max(n_inst, 1))()
        for i, (tint, opacity, ambient) in enumerate(styles):
            arr[i].tint[:] = [float(c) for c in tint]
            arr[i].opacity, arr[i].ambient = float(opacity), float(ambient)
        d.styles = C.cast(arr, C.c_void_p)
        keep.append(arr)
    d.window_pixels = int(window_pixels)
    return d, keep


def _scene_outputs(outputs, n_frames, height, width):
    unknown = set(outputs) - set(SCENE_OUTPUTS)
    if unknown:
        raise ValueError("unknown outputs: %s" % sorted(unknown))
    shape = (n_frames, height, width)
    out = {}
    if "rgb" in outputs:
        out["rgb"] = np.zeros(shape + (3,), np.uint8)
    if "depth" in outputs:
        out["depth"] = np.zeros(shape, np.float32)
    if "instance" in outputs:
        out["instance"] = np.zeros(shape, np.int32)
    if "triangle" in outputs:
        out["triangle"] = np.zeros(shape, np.int32)
    return out, [(_p(out[k]) if k in out else None) for k in SCENE_OUTPUTS]


class SceneRenderer:
    """Resident scene renderer (roft_scene_renderer_*): the meshes are uploaded once, `render` draws up to
    max_frames_per_call frames per call.  cam: L.Camera; meshes: [(verts [n, 3], tris [m, 3]), ...]."""

    def __init__(self, cam, meshes, max_frames_per_call=16, device=0):
        self._h = C.c_void_p()
        self.width, self.height, self.max_frames_per_call = cam.width, cam.height, int(max_frames_per_call)
        arr, keep = _mesh_array(meshes)
        L.check(L.lib().roft_scene_renderer_create(C.byref(cam), arr, len(keep), self.max_frames_per_call, device, C.byref(self._h)))

    def render(self, mesh_index, poses, valid=None, background=None, gray_background=False, styles=None, window_pixels=0,
               outputs=SCENE_OUTPUTS):
        """mesh_index [I]; poses [F, I, 7] rows x y z, q = (w, x, y, z); valid [F, I] or None; background [H, W, 3] or [F, H, W, 3]
        uint8 RGB or None; styles: one (tint rgb 0..255, opacity, ambient) per instance or None.  Returns a dict with the
        requested outputs: rgb [F, H, W, 3] u8, depth [F, H, W] f32 (0 = background), instance / triangle [F, H, W] i32 (-1)."""
        d, keep = _scene_desc(self.width, self.height, mesh_index, poses, valid, background, gray_background, styles, window_pixels)
        out, ptrs = _scene_outputs(outputs, d.n_frames, self.height, self.width)
        L.check(L.lib().roft_scene_render(self._h, C.byref(d), *ptrs))
        del keep
        return out

    def kernel_ms(self):
        """Device time (ms, HIP events) of the last render: (visibility pass, resolve pass), without the copies."""
        ms = (C.c_double * 2)()
        L.check(L.lib().roft_debug_scene_kernel_ms(self._h, ms))
        return ms[0], ms[1]

    def close(self):
        if self._h:
            L.lib().roft_scene_renderer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def render_scene(cam, meshes, mesh_index, poses, valid=None, background=None, gray_background=False, styles=None, window_pixels=0,
                 outputs=SCENE_OUTPUTS):
    """One-shot roft_render_scene: SceneRenderer(cam, meshes).render(...) without a resident handle."""
    arr, keep_m = _mesh_array(meshes)
    d, keep = _scene_desc(cam.width, cam.height, mesh_index, poses, valid, background, gray_background, styles, window_pixels)
    out, ptrs = _scene_outputs(outputs, d.n_frames, cam.height, cam.width)
    L.check(L.lib().roft_render_scene(C.byref(cam), arr, len(keep_m), C.byref(d), *ptrs))
    del keep, keep_m
    return out

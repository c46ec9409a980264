"""Shared cases of the pose-mask depth-gate tests (include/roft_engine.h, section 3e, "silhouettes gated against the depth of the
pose's own frame").  Every expected mask comes from the oracle's ro_render_depth on the CPU (pose_mask_occlusion_cases.render) and
the keep predicate of the header, evaluated here in numpy float32 -- never from the code under test.  Computed once, read-only.

Two tables:
 - the OPERATOR's: (mesh, pose) cases x depth images, each depth image with the AIM it was made for stated as a predicate on the
   reference result, so that retuning a pose or a tolerance cannot silently drop it;
 - the ENGINE's: the streams of the pose-mask tests (160 x 120, 14 frames, poses on frames 0, 6 and 12, each six frames old) with an
   occluder painted into every frame's depth, the gate frame of every delivery by a restatement of the source's flow buffer, and
   the conditions that keep a parity test from passing for the wrong reason."""
import functools

import numpy as np

import pose_mask_cases as pc
import pose_mask_occlusion_cases as oc
import util
from oracle import binding as ob

TF, TB = np.float32(0.02), np.float32(0.05)
FAR = np.float32(30.0)   # a background behind everything the tables draw
f32 = np.float32


# ---- the definition ----------------------------------------------------------------------------------------------------
def gate(R, D, tf=TF, tb=f32(0.0), owned=None):
    """(kept, front, behind) bool images: `owned` (default R > 0) split by keep(R, D) of the header.  float32 throughout; R - tf and
    R + tb each rounded once."""
    R, D, tf, tb = np.asarray(R, f32), np.asarray(D, f32), f32(tf), f32(tb)
    owned = (R > 0) if owned is None else owned
    with np.errstate(invalid="ignore"):
        lo, hi = (R - tf).astype(f32), (R + tb).astype(f32)
        front = owned & (D > 0) & (D < lo)
        behind = owned & ~front & bool(tb > 0) & (D > hi)
    assert not (front & behind).any()
    return owned & ~front & ~behind, front, behind


# ---- the operator's table ----------------------------------------------------------------------------------------------
def operator_cases():
    """name -> [(mesh, pose)]: every aimed case of pose_mask_cases and the two big meshes in front (one object each), and scenes of
    pose_mask_occlusion_cases (the resolve followed by the gate)"""
    out = {name: [(mesh, p)] for name, (mesh, p, _) in pc.AIMED.items()}
    out["cracker_box_front"] = [("cracker_box", pc.POSES["front"])]
    out["box_over_cache_front"] = [("box_over_cache", pc.POSES["front"])]
    for name in ("front_back", "three_deep", "over_cache"):
        out["scene_" + name] = oc.CASES[name][0]
    return out


LAUNCH_SHAPES = ((0, 1), (1, 0), (7, 1))   # (bands, vertex cache)


@functools.lru_cache(maxsize=None)
def rendered(name):
    R = np.stack([oc.render(mesh, p) for mesh, p in operator_cases()[name]])
    R.setflags(write=False)
    return R


def _far(R, own):
    """every owned pixel is farther than 0.1 m: R - tf is a positive number with room below it"""
    return bool(own.any() and R[own].min() > 0.1)


def _nearest(R):
    """the nearest rendered surface per pixel (0: none): what a sensor would see of the scene"""
    return np.where((R > 0).any(0), np.where(R > 0, R, f32(np.inf)).min(0), f32(0)).astype(f32)


# kind -> (depth(R [n, H, W]) -> D [H, W] float32, tb, aim(R, own, kept, front, behind) -> bool).  own / kept / front / behind: [n, H, W]
def _d_boundary(R):
    return np.where((R > 0).any(0), (_nearest(R) - TF).astype(f32), f32(0))


def _d_below(R):
    return np.nextafter(_d_boundary(R), f32(-np.inf)).astype(f32)


def _d_slab(R):
    D = _nearest(R).copy()
    D[:, : pc.W // 2] = f32(0.004)
    return D


def _d_patches(R):
    D = _d_below(R).copy()
    D[: pc.H // 2, : pc.W // 2] = f32(np.nan)
    D[pc.H // 2:, : pc.W // 2] = f32(np.inf)
    return D


def _d_background(R):
    D = _nearest(R).copy()
    D[:, pc.W // 2:] = FAR
    return D


def _half(a, left):
    return a[..., : pc.W // 2] if left else a[..., pc.W // 2:]


DEPTHS = {
    "zeros": (lambda R: np.zeros(R.shape[1:], f32), 0.0, lambda R, own, kept, front, behind: np.array_equal(kept, own)),
    "itself": (_nearest, TB, lambda R, own, kept, front, behind: np.array_equal(kept, own)),
    # the comparison is strict: a depth of exactly R - tf keeps the pixel (an object behind another sees the nearer one's bound: some
    # of ITS pixels go, the nearest object's never)
    "boundary": (_d_boundary, 0.0, lambda R, own, kept, front, behind: np.array_equal(kept[0], own[0])),
    # one ulp below: every owned pixel of the nearest surface with room below it goes
    "below": (_d_below, 0.0, lambda R, own, kept, front, behind: not _far(R, own) or (front.any() and not kept[own & (R == _nearest(R))].any()
                                                                                       and not behind.any())),
    "slab": (_d_slab, 0.0, lambda R, own, kept, front, behind: not _far(R, own) or not _half(own, True).any() or not _half(own, False).any()
             or (_half(front, True).any() and not _half(kept, True).any() and np.array_equal(_half(kept, False), _half(own, False)))),
    # NaN keeps; +inf keeps with the behind test off
    "patches": (_d_patches, 0.0, lambda R, own, kept, front, behind: np.array_equal(_half(kept, True), _half(own, True)) and not behind.any()),
    # ... and is "behind" with it on
    "patches_behind": (_d_patches, TB, lambda R, own, kept, front, behind: np.array_equal(kept[:, : pc.H // 2, : pc.W // 2], own[:, : pc.H // 2, : pc.W // 2])
                       and np.array_equal(behind[:, pc.H // 2:, : pc.W // 2], own[:, pc.H // 2:, : pc.W // 2])),
    "background_off": (_d_background, 0.0, lambda R, own, kept, front, behind: np.array_equal(kept, own)),
    "background_on": (_d_background, TB, lambda R, own, kept, front, behind: np.array_equal(_half(behind, False), _half(own & (R + TB < FAR), False))
                      and not front.any() and np.array_equal(_half(kept, True), _half(own, True))),
}


@functools.lru_cache(maxsize=None)
def operator_expected(name, kind):
    """(D [H, W], tb, masks uint8 [n, H, W], counts [n], removed [n, 2]) of a case under a depth image; asserts the kind's aim"""
    R = rendered(name)
    make, tb, aim = DEPTHS[kind]
    D = np.ascontiguousarray(make(R), f32)
    _, own = oc.resolve(R)
    res = [gate(R[i], D, TF, tb, own[i]) for i in range(R.shape[0])]
    kept, front, behind = (np.stack([r[j] for r in res]) for j in range(3))
    assert aim(R, own, kept, front, behind), ("the case misses its aim", name, kind)
    masks = np.ascontiguousarray(kept.astype(np.uint8) * 255)
    out = (D, float(tb), masks, kept.sum((1, 2)).astype(np.int32), np.stack([front.sum((1, 2)), behind.sum((1, 2))], 1).astype(np.int32))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def operator_table_hits_every_aim_strongly():
    """over the whole table: something removed and something kept in one case, a case emptied, a case with pixels behind"""
    seen = dict(partial=False, emptied=False, behind=False, front=False)
    for name in operator_cases():
        for kind in DEPTHS:
            _, _, masks, counts, removed = operator_expected(name, kind)
            own = oc.resolve(rendered(name))[1].sum((1, 2))
            for i in range(len(counts)):
                seen["partial"] |= bool(counts[i] > 0 and removed[i].sum() > 0)
                seen["emptied"] |= bool(own[i] > 0 and counts[i] == 0)
                seen["front"] |= bool(removed[i, 0] > 0)
                seen["behind"] |= bool(removed[i, 1] > 0)
    return seen


# ---- the engine's table ------------------------------------------------------------------------------------------------
N_FRAMES = 14
POSE_FRAMES = (0, 6, 12)
BAR_COLUMNS, BAR_IN_FRONT = 12, f32(0.15)


@functools.lru_cache(maxsize=None)
def streams(n_obj, seed0=1400):
    out = [util.stream(seed0 + i, N_FRAMES, scale=4) for i in range(n_obj)]
    assert all([k for k in range(N_FRAMES) if st.pose_valid[k]] == list(POSE_FRAMES) for st in out)
    return out


@functools.lru_cache(maxsize=None)
def oracle_mesh(i, seed0=1400):
    return ob.make_mesh(*streams(i + 1, seed0)[i].mesh)


def camera_tuple(st):
    c = st.camera
    return (c.width, c.height, c.fx, c.fy, c.cx, c.cy)


@functools.lru_cache(maxsize=None)
def depth(i, k, bar=True, seed0=1400):
    """object i's depth image of frame k; with the occluder: a vertical bar BAR_COLUMNS wide over the middle of the object's
    ground-truth mask, BAR_IN_FRONT metres in front of the nearest point of the object"""
    st = streams(i + 1, seed0)[i]
    d = np.ascontiguousarray(st.depth[k].numpy(), f32).copy()
    if bar:
        m = st.mask_gt[k].numpy() > 0
        cols = np.nonzero(m.any(0))[0]
        c = int(cols.min() + cols.max()) // 2
        z = f32(d[m & (d > 0)].min()) - BAR_IN_FRONT
        assert z > 0.05
        d[:, c - BAR_COLUMNS // 2: c + BAR_COLUMNS // 2] = z
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def render_pose(i, pose_bytes, seed0=1400):
    st = streams(i + 1, seed0)[i]
    R = oc.render(oracle_mesh(i, seed0), np.frombuffer(pose_bytes), camera_tuple(st))
    R.setflags(write=False)
    return R


def gate_frames(n_frames, has_mask, flow_valid, frames_between, start=0):
    """{delivering frame k: its gate frame}: the source's flow buffer restated (ImageSegmentationOFAidedSource::step_frame and
    oracle/ro_mask.c:44-48).  The buffer holds the frames whose flows arrived since the last consumed mask; a new mask is chased
    through the last frames_between of them (all when that is <= 0), and the chase starts on the frame before the oldest it uses.
    The first mask of a track is an initialisation: it chases nothing and leaves the buffer alone.  start: first frame of the track."""
    out, buf, first = {}, [], True
    for k in range(start, n_frames):
        if flow_valid(k) and k > start:
            buf.append(k)
        if has_mask(k):
            if first:
                out[k], first = k, False
            else:
                use = buf[-frames_between:] if frames_between > 0 else buf
                out[k] = use[0] - 1 if use else k
                buf = []
    return out


def check_conditions(n_obj, tf=TF, seed0=1400):
    """The conditions that keep the engine tests from hiding a failure, on the CPU reference: every delivering pair loses at least
    10 % and keeps at least 50 % of its silhouette; for the delayed pairs the mask gated against the DELIVERING frame's depth differs
    from the contract's in at least 100 pixels (a gate on the wrong frame cannot pass)."""
    g = gate_frames(N_FRAMES, lambda k: k in POSE_FRAMES, lambda k: k > 0, 6)
    assert g == {0: 0, 6: 0, 12: 6}
    for i, st in enumerate(streams(n_obj, seed0)):
        for k in POSE_FRAMES:
            R = render_pose(i, np.ascontiguousarray(st.pose_meas[k], np.float64).tobytes(), seed0)
            kept, front, behind = gate(R, depth(i, g[k], True, seed0), tf)
            raw = int((R > 0).sum())
            assert raw >= 500 and front.sum() >= 0.10 * raw and kept.sum() >= 0.50 * raw, (i, k, raw, int(front.sum()), int(kept.sum()))
            if g[k] != k:
                wrong = gate(R, depth(i, k, True, seed0), tf)[0]
                assert (wrong != kept).sum() >= 100, (i, k, int((wrong != kept).sum()))

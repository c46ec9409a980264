"""Shared cases of the pose-mask occlusion tests (include/roft_engine.h, section 3e, "enrolled objects of one scene hide each
other"): a table of scenes -- a list of (mesh, pose) per case, the object id is the index -- at 160 x 120 with the camera of
pose_mask_cases, each with the AIM it was chosen for stated as a predicate on the oracle's result, so that retuning a pose cannot
silently empty a case.  The expected masks always come from the oracle on the CPU: ro_render_depth(mesh, pose, cam, 1) per object,
resolved in numpy by the definition of the header -- the nearest surface keeps the pixel, the lower id on an exact tie.  Computed
once and never modified."""
import functools

import numpy as np

import pose_mask_cases as pc
from oracle import binding as ob
from roft_amd import synth

W, H, CAM = pc.W, pc.H, pc.CAM
Q0 = ([1, 2, 3], 0.7)


@functools.lru_cache(maxsize=None)
def meshes():
    out = dict(pc.meshes())
    v, t = out["box12"]
    out["small"] = (np.ascontiguousarray(v * np.float32(0.3)), t)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_mesh(name):
    return ob.make_mesh(*meshes()[name])


def render(mesh, p, cam=CAM):
    """R = ro_render_depth(mesh, x, q, cam, 1): the float image of the definition.  mesh: a name of meshes() or an oracle mesh."""
    m = _oracle_mesh(mesh) if isinstance(mesh, str) else mesh
    return np.array(ob.render_depth(m, p[:3], p[3:], pc.oracle_camera(cam), 1), np.float32)


def resolve(R):
    """R [n, H, W] float32 -> (raw [n, H, W] bool, resolved [n, H, W] bool) by the definition: object i keeps p when R_i(p) > 0 and no
    other object is nearer; argmin returns the FIRST minimum, the lowest id."""
    R = np.asarray(R, np.float32)
    raw = R > 0
    near = np.argmin(np.where(raw, R, np.float32(np.inf)), axis=0)
    return raw, raw & (near[None] == np.arange(R.shape[0])[:, None, None])


def _lost_only_to_nearer(R, raw, res):
    """every pixel an object lost went to an object that is nearer there (or as near, with a lower id)"""
    n = R.shape[0]
    for i in range(n):
        lost = raw[i] & ~res[i]
        owner = np.argmax(res, axis=0)
        if not (res.any(axis=0)[lost]).all():
            return False
        zo = np.take_along_axis(R, owner[None], 0)[0]
        if not ((zo[lost] < R[i][lost]) | ((zo[lost] == R[i][lost]) & (owner[lost] < i))).all():
            return False
    return True


def _aim_front_back(R, raw, res):
    return (np.array_equal(res[0], raw[0]) and res[1].any() and res[1].sum() < raw[1].sum() and not (res[0] & res[1]).any()
            and np.array_equal(res[0] | res[1], raw[0] | raw[1]))


def _aim_crossing(R, raw, res):
    both = raw[0] & raw[1]
    return (res[0] & both).any() and (res[1] & both).any()


def _aim_tie(R, raw, res):
    return np.array_equal(R[0], R[1]) and np.array_equal(res[0], raw[0]) and raw[1].any() and not res[1].any()


def _aim_hidden(R, raw, res):
    return raw[1].any() and not res[1].any()


def _aim_three_deep(R, raw, res):
    pairs = all((raw[i] & raw[j]).any() for i in range(3) for j in range(i + 1, 3))
    return pairs and all((raw[i] & ~res[i]).any() for i in (1, 2)) and np.array_equal(res[0], raw[0]) and _lost_only_to_nearer(R, raw, res)


def _aim_big_scene(R, raw, res):
    losers = sum(bool((raw[i] & ~res[i]).any()) for i in range(R.shape[0]))
    # an id >= 32 wins a pixel a lower id also covers
    high_wins = any((res[i] & raw[:i].any(axis=0)).any() for i in range(32, R.shape[0]))
    return R.shape[0] == 64 and losers >= 32 and high_wins


def _aim_over_cache(R, raw, res):
    return meshes()["box_over_cache"][0].shape[0] > pc.CACHE_VERTS and (raw[0] & raw[1]).any() and (raw[1] & ~res[1]).any() and res[1].any()


def _aim_near_plane(R, raw, res):
    p = pc.AIMED["straddles_near_plane"][1]
    return pc.AIMED["straddles_near_plane"][2](raw[0], p) and (raw[0] & raw[1]).any() and (raw[1] & ~res[1]).any() and res[1].any()


def _big_scene():
    out = []
    for r in range(8):
        for c in range(8):
            k = 8 * r + c
            # neighbours overlap (a box is ~50 x 65 pixels at 0.6 m, the grid step is 16 x 12), and depth does not follow the id:
            # ids >= 32 come nearer than some of their lower neighbours
            z = 0.55 + 0.013 * ((k * 37) % 64) / 8.0
            out.append(("box12", pc.pose([(c - 3.5) * 0.064, (r - 3.5) * 0.048, z], *Q0)))
    return out


# name -> ([(mesh, pose)], aim(R, raw, resolved) -> bool)
CASES = {
    "front_back": ([("box12", pc.pose([-0.03, 0.0, 0.40], *Q0)), ("box12", pc.pose([0.04, 0.01, 0.60], *Q0))], _aim_front_back),
    "crossing": ([("box12", pc.pose([0.0, 0.0, 0.45], [0, 1, 0], 0.6)), ("box12", pc.pose([0.0, 0.0, 0.45], [0, 1, 0], -0.6))], _aim_crossing),
    "tie": ([("box12", pc.pose([0.0, 0.0, 0.45], *Q0)), ("box12", pc.pose([0.0, 0.0, 0.45], *Q0))], _aim_tie),
    "hidden": ([("box12", pc.pose([0.0, 0.0, 0.35], *Q0)), ("small", pc.pose([0.0, 0.0, 0.7], *Q0))], _aim_hidden),
    "three_deep": ([("box12", pc.pose([-0.03, 0.0, 0.40], *Q0)), ("box12", pc.pose([0.02, 0.02, 0.55], *Q0)),
                    ("box12", pc.pose([0.06, -0.01, 0.70], *Q0))], _aim_three_deep),
    "big_scene": (_big_scene(), _aim_big_scene),
    "over_cache": ([("box_over_cache", pc.pose([-0.03, 0.0, 0.40], *Q0)), ("box12", pc.pose([0.04, 0.01, 0.60], *Q0))], _aim_over_cache),
    "near_plane": ([("box12", pc.AIMED["straddles_near_plane"][1]), ("box12", pc.pose([0.1, 0.0, 0.5], *Q0))], _aim_near_plane),
}


@functools.lru_cache(maxsize=None)
def rendered(name):
    """R [n, H, W] of a case (read-only)."""
    R = np.stack([render(mesh, p) for mesh, p in CASES[name][0]])
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def expected(name):
    """(raw silhouettes, resolved masks) of a case, uint8 {0, 255} [n, H, W] each (read-only)."""
    raw, res = resolve(rendered(name))
    out = tuple(np.ascontiguousarray(m.astype(np.uint8) * 255) for m in (raw, res))
    for m in out:
        m.setflags(write=False)
    return out

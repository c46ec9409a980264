"""Shared cases of the VSD tests (include/roft_engine.h, section 3i): meshes, cameras, pose pairs, the test depth image, and the
reference results, computed once per session and never modified."""
import functools

import numpy as np

import mesh_zoo
import scene_util
import vsd_ref
from oracle import binding as ob

SIZES = scene_util.SIZES          # (160, 120) and the awkward (93, 71); fx = fy = 150
MESHES = ("box", "torus")
DELTA = 0.015
TAUS = np.arange(0.05, 0.51, 0.05)   # the ten BOP taus
REFERENCE = scene_util.pose([0.01, -0.02, 0.45], [1, 2, 3], 0.7)
ESTIMATES = {
    "near": scene_util.pose([0.013, -0.018, 0.455], [1, 2, 3], 0.78),
    "far": scene_util.pose([0.03, -0.01, 0.47], [1, 2, 2], 1.1),
    "same": REFERENCE,
    "off": scene_util.pose([0.4, 0.3, 0.45], [1, 2, 3], 0.7),   # off screen
}
CLOSE = scene_util.POSES[2]   # vertices behind the near plane: the back-face rule is off
CACHE_VERTS = 10581           # the most vertices the kernel's LDS cache holds next to its two windows (raster_shape.h, vsd_shape)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts, tris).  big_box: the smallest subdivided box with more vertices than the vertex cache holds."""
    if name == "big_box":
        v, t = mesh_zoo.box(41)
        assert len(v) > CACHE_VERTS >= len(mesh_zoo.box(40)[0])
        return v, t
    v, t, _ = scene_util.zoo()[name]
    return v, t


@functools.lru_cache(maxsize=None)
def diameter(name):
    """the largest distance between two vertices"""
    if name == "big_box":
        return diameter("box")   # (the same eight corners)
    v = mesh(name)[0].astype(np.float64)
    best = 0.0
    for p in v:
        best = max(best, float(np.sqrt(((v - p) ** 2).sum(axis=1).max())))
    return best


@functools.lru_cache(maxsize=None)
def render(name, pose_key, size):
    """pose_key: 'reference', 'close' or a key of ESTIMATES"""
    p = REFERENCE if pose_key == "reference" else CLOSE if pose_key == "close" else ESTIMATES[pose_key]
    d = vsd_ref.render(ob, mesh(name), p, scene_util.cam(*size))
    d.setflags(write=False)
    return d


def pose_of(pose_key):
    return REFERENCE if pose_key == "reference" else CLOSE if pose_key == "close" else ESTIMATES[pose_key]


@functools.lru_cache(maxsize=None)
def sensor_depth(name, size):
    """The sensor's image of a case: the reference render pushed back and forth by up to 2 cm (some reference pixels thus sit 2 cm
    behind the measurement and are hidden), a wall at 0.9 m elsewhere, an occluder at 0.25 m and a patch of holes."""
    W, H = size
    Dg = render(name, "reference", size)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")   # i: column, j: row
    step = (((7 * ii + 13 * jj) % 5) - 2).astype(np.float32)
    d = np.where(Dg > 0, Dg + np.float32(0.01) * step, np.float32(0.9)).astype(np.float32)
    d[H // 2 - 6:H // 2 + 2, W // 2:W // 2 + 14] = 0.25
    d[H // 2 + 4:H // 2 + 9, W // 2 - 12:W // 2] = 0.0
    d.setflags(write=False)
    return d


def strange_depths(name, size):
    """all holes, all wall, and the case's image with NaN and negative pixels over the object"""
    W, H = size
    mixed = sensor_depth(name, size).copy()
    mixed[H // 2 - 10:H // 2 - 3, :] = np.nan
    mixed[:, W // 2 - 9:W // 2 - 4] = -0.4
    mixed[H // 2 + 10, :] = -np.inf
    return {"zeros": np.zeros((H, W), np.float32), "wall": np.full((H, W), 0.9, np.float32), "mixed": mixed}


@functools.lru_cache(maxsize=None)
def reference(name, est_key, size):
    """(errors, counts, margins) of the restatement for a base case"""
    margins = {}
    e, c = vsd_ref.vsd(render(name, est_key, size), render(name, "reference", size), sensor_depth(name, size), scene_util.cam(*size), DELTA, TAUS,
                       diameter(name), margins)
    e.setflags(write=False)
    c.setflags(write=False)
    return e, c, margins


def lib_mesh(name):
    from roft_amd import ops
    return ops.make_mesh(*mesh(name))


def device(name, est_keys, size, depth=None, **kw):
    """ops.pose_errors_vsd on base cases: (errors [n, 10], counts [n, 14]).  depth None: the case's test image under every pair."""
    from roft_amd import ops
    est = np.array([pose_of(k) for k in est_keys])
    ref = np.array([REFERENCE] * len(est_keys))
    depth = sensor_depth(name, size) if depth is None else depth
    kw.setdefault("diameter", diameter(name))
    kw.setdefault("taus", TAUS)
    return ops.pose_errors_vsd(scene_util.lib_cam(scene_util.cam(*size)), lib_mesh(name), est, ref, depth, delta=DELTA, counts=True, **kw)

"""The contract render of the outlier test walks a mesh cluster by cluster (roft_amd/csrc/mesh_clusters.h, outlier_fused_kernel<false>):
one wave projects the at most 64 vertices of a cluster and draws its at most 64 triangles, the window box and the `behind` flag come
from the corners of the mesh's box, and a cluster whose cone says so is skipped.  roft_render_depth and roft_outlier_test against
oracle/ro_render.c and the oracle's likelihood, as tests/test_parity_gpu.py compares them -- tiles and sample counts bit for bit, the
likelihood within that file's LIK_RTOL of the oracle's sequential sum and bit for bit the same in every launch shape -- on a 160 x 120
target with divider 1 and 2, with the smallest meshes and poses that reach every path of the kernel."""

import numpy as np
import pytest

import mesh_zoo
import util
from roft_amd import _lib as L
from roft_amd import ops, synth

pytestmark = pytest.mark.gpu

LIK_RTOL = 1e-12       # tree reduction vs sequential double accumulation of float terms (tests/test_parity_gpu.py)
TW, TH = 160, 120
IDENT = np.array([1.0, 0.0, 0.0, 0.0])


def _camera(div):
    """A camera whose render target at `div` is 160 x 120."""
    base = synth.Camera.shape_a()     # 640 x 480
    return base.scaled(4 // div)


def _meshes():
    zoo = mesh_zoo.zoo()
    one = (np.array([[-0.05, -0.04, 0.0], [0.06, -0.03, 0.01], [0.0, 0.05, -0.01]], np.float32), np.array([[0, 1, 2]], np.int32), False)
    return {
        "box": zoo["box"],                    # closed, 432 triangles over 218 vertices: the last cluster of a bucket is short in both counts
        "torus": zoo["torus"],                # closed, curved: cones with an opening angle, 288 vertices
        "box_reversed": zoo["box_reversed"],  # inside out: closed, every flip bit set
        "box_open": zoo["box_open"],          # open: no cones, every triangle drawn
        "torus_open": zoo["torus_open"],
        "projective_plane": (zoo["projective_plane"][0] * 2.0, zoo["projective_plane"][1], False),
        "one_triangle": one,
    }


def _quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _poses(name):
    """(label, x, q).  The box's half extents are 0.08 x 0.10 x 0.035."""
    rng = np.random.default_rng(41)
    out = [("in view", np.array([0.02, -0.01, 0.45]), _quat(rng)), ("in view, close", np.array([-0.03, 0.02, 0.22]), _quat(rng)),
           ("half off the target", np.array([0.27, 0.05, 0.5]), _quat(rng)), ("wholly off the target", np.array([5.0, 0.0, 0.6]), IDENT),
           ("behind the camera", np.array([0.0, 0.0, -1.0]), IDENT)]
    # A quaternion is taken as it is given (oracle/ro_la.c, make_pose): one that is not of unit length gives a matrix that is no
    # rotation, under which the per-triangle sign of area still culls exactly what it culled, but a normal cone does not hold: the
    # kernel must not ask the cones (2 % off), and may where the matrix is a rotation to within pose_is_rotation's tolerance.
    out.append(("q 2 % off unit length", np.array([-0.01, 0.02, 0.40]), _quat(rng) / 0.98))
    out.append(("q 3e-7 off unit length", np.array([0.03, 0.01, 0.42]), _quat(rng) * (1.0 + 3e-7)))
    if name.startswith("box"):
        # a vertex behind the near plane (the camera inside the box): the exact vertex pass, the back-face rule off
        out.append(("camera inside", np.array([0.0, 0.0, 0.02]), IDENT))
        # nearest vertices at z = 0.005: in front of the near plane (0.001), the corners below 0.01 settle nothing: the exact vertex
        # pass, the back-face rule on
        out.append(("corners inconclusive", np.array([0.0, 0.0, 0.040]), IDENT))
        # nearest vertices at z = 0.015: the corners settle it, a grazing, very close view
        out.append(("just in front", np.array([0.0, 0.0, 0.050]), IDENT))
    return out


@pytest.fixture(scope="module")
def refs(oracle):
    """Oracle renders, shared by the tests of this module: (div, mesh, pose label) -> tile."""
    cache = {}

    def get(div, name, label, x, q):
        key = (div, name, label)
        if key not in cache:
            v, t, _ = _meshes()[name]
            cache[key] = oracle.render_depth(oracle.make_mesh(v, t), x, q, util.oracle_camera(oracle, _camera(div)), div)
        return cache[key]
    return get


@pytest.mark.parametrize("div", [1, 2])
@pytest.mark.parametrize("name", sorted(_meshes()))
def test_render_depth_of_every_mesh_and_pose(oracle, refs, name, div):
    v, t, closed = _meshes()[name]
    assert ops.mesh_classify(v, t)[0] == closed
    cam = _camera(div)
    assert (cam.width // div, cam.height // div) == (TW, TH)
    dcam = L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    mesh = ops.make_mesh(v, t)
    drawn = {}
    for label, x, q in _poses(name):
        t0 = refs(div, name, label, x, q)
        t1 = ops.render_depth(mesh, x, q, dcam, div)
        assert np.array_equal(t0, t1), (name, div, label, int((t0 != t1).sum()))
        drawn[label] = int((t0 > 0).sum())
    assert drawn["in view"] > 30 and drawn["half off the target"] > 0, drawn
    assert drawn["q 2 % off unit length"] > 20 and drawn["q 3e-7 off unit length"] > 20, drawn
    assert drawn["wholly off the target"] == 0 and drawn["behind the camera"] == 0
    if name.startswith("box"):
        assert drawn["camera inside"] > 1000 and drawn["corners inconclusive"] > 1000 and drawn["just in front"] > 1000, drawn


SHAPES = [dict(bands=b, forced=f) for b in (1, 2, 3, 8) for f in (0, 1)] + [dict(bands=0, forced=-1), dict(bands=1, window_pixels=TW, forced=-1),
                                                                            dict(bands=8, window_pixels=TW, forced=1), dict(bands=2, window_pixels=3 * TW, forced=0)]
# The slab merge has a branch per number of other slabs (G - 1): bands 2, 3 and 8 above reach 1, 2 and 7, bands 6 and 7 the shared
# branch of five and six real slabs with the spare pointers repeated.
SHAPES += [dict(bands=6, forced=1), dict(bands=7, forced=1)]


@pytest.mark.parametrize("div", [1, 2])
@pytest.mark.parametrize("name,labels", [("box", ("in view", "in view, close")), ("box", ("half off the target", "in view")),
                                         ("box", ("camera inside", "corners inconclusive")), ("box", ("wholly off the target", "just in front")),
                                         ("torus", ("in view", "in view, close")), ("torus", ("q 2 % off unit length", "q 3e-7 off unit length")),
                                         ("box", ("q 2 % off unit length", "in view")), ("box_reversed", ("in view", "half off the target")),
                                         ("box_open", ("in view", "camera inside")), ("one_triangle", ("in view", "in view, close"))])
def test_outlier_test_in_every_launch_shape(oracle, refs, name, labels, div):
    """parts 1, 2, 3 and 8 with roft_debug_outlier_split 0 and 1, parts 6 and 7 with 1, the library's own choice, and windows forced down
    to one row and to three (strips); alternative k is the pose `labels[k]`, the scene shows the mesh at the first pose of the list."""
    v, t, _ = _meshes()[name]
    cam = _camera(div)
    ocam = util.oracle_camera(oracle, cam)
    dcam = L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    mesh = ops.make_mesh(v, t)
    poses = {label: (x, q) for label, x, q in _poses(name)}
    x2 = np.stack([poses[l][0] for l in labels])
    q2 = np.stack([poses[l][1] for l in labels])
    scene_x, scene_q = poses["in view"][0] + [0.004, -0.003, 0.006], poses["in view"][1]
    full = oracle.render_depth(oracle.make_mesh(v, t), scene_x, scene_q, ocam, 1)
    depth = np.where(full > 0, full, 1.5).astype(np.float32)
    # (the mask reaches past the silhouette: samples fall on window pixels nothing is drawn into, and outside the window)
    mask = np.zeros(full.shape, np.uint8)
    ys, xs = np.nonzero(full > 0)
    mask[max(ys.min() - 6, 0):ys.max() + 7, max(xs.min() - 6, 0):xs.max() + 7] = 255
    t_ref = [refs(div, name, labels[k], x2[k], q2[k]) for k in range(2)]
    ref = [oracle.depth_likelihood(ocam, depth, mask, t_ref[k], div) for k in range(2)]
    L_first = None
    try:
        for kw in SHAPES:
            kw = dict(kw)
            L.check(L.lib().roft_debug_outlier_split(kw.pop("forced")))
            Lv, ns, sel, tiles = ops.outlier_test(dcam, div, depth, mask, mesh, x2, q2, **kw)
            L_first = list(Lv) if L_first is None else L_first
            assert list(Lv) == L_first, (kw, list(Lv), L_first)     # exact integer sums: the same bits in every launch shape
            for k in range(2):
                assert np.array_equal(tiles[k], t_ref[k]), (name, div, kw, k, int((tiles[k] != t_ref[k]).sum()))
                assert ns[k] == ref[k][1], (kw, k)
                if ref[k][1] == 0:
                    assert Lv[k] == ref[k][0] == np.finfo(np.float64).max
                else:
                    assert abs(Lv[k] - ref[k][0]) <= LIK_RTOL * abs(ref[k][0]), (kw, k)
            assert sel == (1 if ref[0][0] > 2.0 * ref[1][0] else 0), kw
    finally:
        L.lib().roft_debug_outlier_split(-1)


def test_zero_samples(oracle):
    v, t, _ = _meshes()["box"]
    cam = _camera(2)
    dcam = L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    mesh = ops.make_mesh(v, t)
    (_, x, q) = _poses("box")[0]
    depth = np.full((cam.height, cam.width), 0.5, np.float32)
    big = np.finfo(np.float64).max
    for d, m in ((depth, np.zeros(depth.shape, np.uint8)), (np.full_like(depth, 2.5), np.full(depth.shape, 255, np.uint8))):
        for bands in (1, 8):
            Lv, ns, sel, _ = ops.outlier_test(dcam, 2, d, m, mesh, np.stack([x, x]), np.stack([q, q]), bands=bands, tiles=False)
            assert list(ns) == [0, 0] and Lv[0] == big and Lv[1] == big and sel == 0

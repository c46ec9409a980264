"""Render mode ROFT_RENDER_GL of the engine's rasteriser (outlier_fused_kernel<true>, roft_render_depth_mode /
roft_outlier_test_mode) against RO_RENDER_GL of oracle/ro_render.c: the numerics of the reference's OpenGL pipeline (every
triangle drawn, window z in a 24-bit depth buffer, the first triangle wins a tie, top-left rule).  Tiles bit exact, background
included, in every launch shape; the likelihood on the same samples within LIK_RTOL; the decision identical.  Mode 0 of the
new entry points is the render contract of roft_render_depth / roft_outlier_test_split, to the bit."""
import ctypes as C

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import ops, synth

import util

pytestmark = pytest.mark.gpu

LIK_RTOL = 1e-12
GL = L.RENDER_GL


def _dcam(cam):
    return L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)


def _rand_poses(rng, n, z=(0.35, 0.8)):
    out = []
    for _ in range(n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        out.append((np.array([rng.uniform(-0.12, 0.12), rng.uniform(-0.08, 0.08), rng.uniform(*z)]), q))
    return out


def _edge_poses():
    """A vertex off the target on every side, the object across the border, and the camera inside it (vertices behind the
    near plane: those triangles are dropped by both)."""
    one = np.array([1.0, 0.0, 0.0, 0.0])
    return [(np.array([0.25, 0.0, 0.5]), one), (np.array([-0.27, 0.1, 0.45]), one), (np.array([0.0, 0.2, 0.5]), one),
            (np.array([0.0, 0.0, 0.02]), one), (np.array([0.0, 0.05, 0.0]), one), (np.array([0.0, 0.0, -1.0]), one),
            (np.array([50.0, 0.0, 1.0]), one)]


def _check_render(oracle, verts, tris, cam, div, poses, min_drawn=0):
    omesh, mesh = oracle.make_mesh(verts, tris), ops.make_mesh(verts, tris)
    ocam, dcam = util.oracle_camera(oracle, cam), _dcam(cam)
    drawn = []
    for x, q in poses:
        t0 = oracle.render_depth_mode(omesh, x, q, ocam, div, oracle.RENDER_GL)
        t1 = ops.render_depth(mesh, x, q, dcam, div, mode=GL)
        assert np.array_equal(t0, t1), (x, q, div, int((t0 != t1).sum()))
        drawn.append(int((t0 > 0).sum()))
    assert max(drawn) >= min_drawn, drawn
    return drawn


def spike_mesh(half=(0.08, 0.10, 0.035), n=6, tip=0.2):
    """The closed mesh that intersects itself: a box whose centre vertex of the -z face is pushed along +z through the +z face
    to z = tip.  One connected, closed, orientable surface of positive volume; the part of the spike beyond the +z face
    encloses a pocket of winding number -1.  Seen from -z, the +z face is the nearest surface inside the spike's funnel -- a
    triangle that faces away, which the render contract leaves out."""
    v, t = synth.box_mesh(half, n)
    v = np.array(v, np.float32)
    t = np.ascontiguousarray(t, np.int32)
    face = np.where(np.abs(v[:, 2] + half[2]) < 1e-7)[0]
    c = face[np.argmin(np.abs(v[face, 0]) + np.abs(v[face, 1]))]
    assert abs(v[c, 0]) < 1e-7 and abs(v[c, 1]) < 1e-7
    v[c, 2] = tip
    return v, t


@pytest.mark.parametrize("div,shape", [(1, "A"), (2, "A"), (4, "A"), (2, "B"), (4, "B")])
def test_gl_render_bit_exact_on_synthetic_cuboids(oracle, div, shape):
    cam = synth.Camera.shape_a() if shape == "A" else synth.Camera.shape_b()
    rng = np.random.default_rng(40 + div)
    for half, n in (((0.08, 0.10, 0.035), 8), ((0.05, 0.09, 0.02), 14)):
        v, t = synth.box_mesh(half, n)
        _check_render(oracle, v, t, cam, div, _rand_poses(rng, 3) + _edge_poses(), min_drawn=50)


def test_gl_render_bit_exact_on_the_mesh_zoo(oracle):
    import mesh_zoo
    cam = synth.Camera.shape_a()
    rng = np.random.default_rng(41)
    for name, (verts, tris, closed) in mesh_zoo.zoo(14).items():
        if name == "projective_plane":
            verts = (verts * 2.0).astype(np.float32)
        assert ops.mesh_classify(verts, tris)[0] == closed
        drawn = _check_render(oracle, verts, tris, cam, 2, _rand_poses(rng, 3) + _edge_poses())
        if name != "box_nan_vertex":
            assert max(drawn) > 100, (name, drawn)


def test_gl_render_bit_exact_on_the_reference_meshes(oracle, tmp_path):
    import glob
    import os
    from roft_amd import io
    paths = sorted(glob.glob(os.path.join(util.ref_mesh_db(tmp_path), "DOPE", "*.obj")))
    assert len(paths) == 7
    rng = np.random.default_rng(42)
    for i, p in enumerate(paths):
        verts, tris = io.load_obj(p)
        cam, div = (synth.Camera.shape_a(), 2) if i % 2 == 0 else (synth.Camera.shape_b(), 4)
        _check_render(oracle, verts, tris, cam, div, _rand_poses(rng, 2, z=(0.5, 0.9)) + _edge_poses()[:3], min_drawn=200)


def test_self_intersecting_closed_mesh_is_drawn_as_the_reference_draws_it(oracle):
    verts, tris = spike_mesh()
    assert ops.mesh_classify(verts, tris)[0] and oracle.mesh_classify(verts, tris)[0]
    cam = synth.Camera.shape_a()
    ocam, dcam = util.oracle_camera(oracle, cam), _dcam(cam)
    omesh, mesh = oracle.make_mesh(verts, tris), ops.make_mesh(verts, tris)
    x, q = np.array([0.0, 0.0, 0.5]), np.array([1.0, 0.0, 0.0, 0.0])
    for div in (1, 2):
        contract = ops.render_depth(mesh, x, q, dcam, div)
        gl = ops.render_depth(mesh, x, q, dcam, div, mode=GL)
        assert np.array_equal(gl, oracle.render_depth_mode(omesh, x, q, ocam, div, oracle.RENDER_GL))
        # inside the funnel the contract leaves out the +z face (it faces away) and reads the spike's wall behind it
        lost = (gl > 0) & (contract > gl + 0.01)
        assert lost.sum() > 10, int(lost.sum())
    rng = np.random.default_rng(43)
    _check_render(oracle, verts, tris, cam, 2, [(x + rng.normal(scale=0.01, size=3), q) for _ in range(3)])


def _tri_mesh(verts, tris):
    return np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32)


def test_ties_go_to_the_lower_triangle_index(oracle):
    """Two coplanar triangles that overlap (the second's corners are affine combinations of the first's): their window z
    quantises alike over most of the overlap, where the triangle listed first is kept (GL_LESS) -- in both orders, bit exact
    against the oracle, every pixel of the overlap taken from one of the two."""
    cam = synth.Camera.shape_a()
    ocam, dcam = util.oracle_camera(oracle, cam), _dcam(cam)
    a = [[-0.05, -0.04, 0.6], [0.06, -0.03, 0.65], [0.0, 0.07, 0.62]]
    w = np.array([[1.2, -0.3, 0.1], [-0.2, 0.4, 0.8], [0.3, 1.1, -0.4]])   # (rows sum to 1)
    b = (w @ np.array(a, np.float64)).tolist()
    one = np.array([1.0, 0.0, 0.0, 0.0])
    for order in ((a, b), (b, a)):
        verts, tris = _tri_mesh(order[0] + order[1], [[0, 1, 2], [3, 4, 5]])
        omesh, mesh = oracle.make_mesh(verts, tris), ops.make_mesh(verts, tris)
        for div in (1, 2):
            t0 = oracle.render_depth_mode(omesh, np.zeros(3), one, ocam, div, oracle.RENDER_GL)
            t1 = ops.render_depth(mesh, np.zeros(3), one, dcam, div, mode=GL)
            assert (t0 > 0).sum() > 100 and np.array_equal(t0, t1)
            first = ops.render_depth(ops.make_mesh(verts, tris[:1]), np.zeros(3), one, dcam, div, mode=GL)
            second = ops.render_depth(ops.make_mesh(verts, tris[1:]), np.zeros(3), one, dcam, div, mode=GL)
            both = (first > 0) & (second > 0)
            assert both.sum() > 50 and np.all((t1[both] == first[both]) | (t1[both] == second[both]))


def test_shared_edge_on_pixel_centres_is_covered_once(oracle):
    """A vertical and a horizontal shared edge exactly on pixel centres (cx, cy at .5, the edge's vertices at X = 0 / Y = 0):
    every centre on an edge belongs to exactly one of the two triangles (top-left rule), and the render is the oracle's."""
    ocam = oracle.camera(320, 240, 300.0, 300.0, 160.5, 120.5)
    dcam = L.Camera(320, 240, 300.0, 300.0, 160.5, 120.5)
    one = np.array([1.0, 0.0, 0.0, 0.0])
    zero = np.zeros(3)
    a = 0.1
    # left / right of the edge X = 0 (pixel column 160), then above / below the edge Y = 0 (pixel row 120); the apexes at other
    # depths, so the triangles are not coplanar
    cases = [([[0.0, -a, 0.5], [0.0, a, 0.5], [-a, 0.0, 0.6], [a, 0.0, 0.4]], [[0, 1, 2], [0, 3, 1]], (slice(None), 160)),
             ([[-a, 0.0, 0.5], [a, 0.0, 0.5], [0.0, -a, 0.6], [0.0, a, 0.4]], [[0, 2, 1], [0, 1, 3]], (120, slice(None)))]
    for verts, tris, line in cases:
        verts, tris = _tri_mesh(verts, tris)
        t0 = oracle.render_depth_mode(oracle.make_mesh(verts, tris), zero, one, ocam, 1, oracle.RENDER_GL)
        t1 = ops.render_depth(ops.make_mesh(verts, tris), zero, one, dcam, 1, mode=GL)
        assert np.array_equal(t0, t1)
        for tt in (tris, tris[:, ::-1].copy()):   # (either winding)
            s0 = ops.render_depth(ops.make_mesh(verts, tt[:1]), zero, one, dcam, 1, mode=GL)[line]
            s1 = ops.render_depth(ops.make_mesh(verts, tt[1:]), zero, one, dcam, 1, mode=GL)[line]
            on = (t1[line] > 0)
            assert on.sum() > 50
            assert np.array_equal((s0 > 0) ^ (s1 > 0), on) and not ((s0 > 0) & (s1 > 0)).any()
            assert np.array_equal(s0, oracle.render_depth_mode(oracle.make_mesh(verts, tt[:1]), zero, one, ocam, 1, oracle.RENDER_GL)[line])


def _scene(oracle, omesh, ocam, x, q):
    full = oracle.render_depth_mode(omesh, x, q, ocam, 1, oracle.RENDER_GL)
    depth = np.where(full > 0, full, 1.5).astype(np.float32)
    mask = (full > 0).astype(np.uint8) * 255
    return depth, mask


def _turn(q, ang, axis):
    dq = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * np.asarray(axis, np.float64)])
    return np.array([dq[0] * q[0] - dq[1:] @ q[1:], *(dq[0] * q[1:] + q[0] * dq[1:] + np.cross(dq[1:], q[1:]))])


SHAPES = [dict(bands=1), dict(bands=2), dict(bands=3), dict(bands=8), dict(bands=0), dict(bands=1, vertex_cache=False),
          dict(bands=8, vertex_cache=False), dict(bands=1, window_pixels="tw"), dict(bands=2, window_pixels="3tw"),
          dict(bands=8, split=False), dict(bands=8, split=True), dict(bands=4, split=True, window_pixels="tw"),
          dict(bands=5, split=True, vertex_cache=False, window_pixels="3tw")]


@pytest.mark.parametrize("which", ["cuboid_A", "cuboid_B", "spike", "cracker_box"])
def test_gl_outlier_test_identical_across_launch_shapes(oracle, which, tmp_path):
    if which == "cracker_box":
        from roft_amd import io
        verts, tris = io.load_obj(util.ref_cracker_box(tmp_path))
    elif which == "spike":
        verts, tris = spike_mesh()
    else:
        verts, tris = synth.box_mesh((0.08, 0.10, 0.035), 10)
    cam, div = (synth.Camera.shape_b(), 4) if which == "cuboid_B" else (synth.Camera.shape_a(), 2)
    omesh, mesh = oracle.make_mesh(verts, tris), ops.make_mesh(verts, tris)
    ocam, dcam = util.oracle_camera(oracle, cam), _dcam(cam)
    tw = cam.width // div
    x = np.array([0.02, -0.01, 0.55])
    q = _turn(np.array([1.0, 0.0, 0.0, 0.0]), 0.4, [0.6, 0.8, 0.0]) if which != "spike" else np.array([1.0, 0.0, 0.0, 0.0])
    depth, mask = _scene(oracle, omesh, ocam, x, q)
    cases = [(np.stack([x + [0.03, -0.02, 0.04], x + [0.001, 0.0, 0.002]]), np.stack([_turn(q, 0.2, [0, 1, 0]), q])),
             (np.stack([x + [0.002, 0.0, 0.001], x + [0.004, 0.001, 0.0]]), np.stack([q, q])),
             (np.stack([x, x + [50.0, 0.0, 0.0]]), np.stack([q, q]))]     # alternative 1 off screen: no sample
    for x2, q2 in cases:
        t_ref = [oracle.render_depth_mode(omesh, x2[k], q2[k], ocam, div, oracle.RENDER_GL) for k in range(2)]
        ref = [oracle.depth_likelihood(ocam, depth, mask, t_ref[k], div) for k in range(2)]
        assert (t_ref[0] > 0).sum() > 50
        first = None
        for kw in SHAPES:
            kw = dict(kw)
            if "window_pixels" in kw:
                kw["window_pixels"] = {"tw": tw, "3tw": 3 * tw}[kw["window_pixels"]]
            Lv, ns, sel, tiles = ops.outlier_test(dcam, div, depth, mask, mesh, x2, q2, mode=GL, **kw)
            got = (list(Lv), list(ns), sel)
            first = got if first is None else first
            assert got == first, (which, kw, got, first)
            for k in range(2):
                assert np.array_equal(tiles[k], t_ref[k]), (which, kw, k, int((tiles[k] != t_ref[k]).sum()))
                assert ns[k] == ref[k][1], (which, kw, k)
                if ref[k][1] == 0:
                    assert Lv[k] == ref[k][0] == np.finfo(np.float64).max
                else:
                    assert abs(Lv[k] - ref[k][0]) <= LIK_RTOL * abs(ref[k][0]), (which, kw, k)
            assert sel == (1 if ref[0][0] > 2.0 * ref[1][0] else 0), (which, kw)


def test_mode_0_of_the_new_entry_points_is_the_contract(oracle):
    lib = L.lib()
    verts, tris = spike_mesh()   # (closed: the contract's back-face rule and walk order are in play)
    cam = synth.Camera.shape_a()
    dcam = _dcam(cam)
    mesh = ops.make_mesh(verts, tris)
    x, q = np.array([0.01, 0.0, 0.5]), _turn(np.array([1.0, 0.0, 0.0, 0.0]), 0.3, [1, 0, 0])
    for div in (1, 2):
        want = ops.render_depth(mesh, x, q, dcam, div)
        got = np.zeros_like(want)
        L.check(lib.roft_render_depth_mode(C.byref(mesh), x.ctypes.data, q.ctypes.data, C.byref(dcam), div, L.RENDER_CONTRACT, got.ctypes.data))
        assert np.array_equal(want, got) and (want > 0).sum() > 100
        assert not np.array_equal(want, ops.render_depth(mesh, x, q, dcam, div, mode=GL))
    bad = np.zeros((cam.height // 2, cam.width // 2), np.float32)
    assert lib.roft_render_depth_mode(C.byref(mesh), x.ctypes.data, q.ctypes.data, C.byref(dcam), 2, 2, bad.ctypes.data) == -1
    omesh, ocam = oracle.make_mesh(verts, tris), util.oracle_camera(oracle, cam)
    depth, mask = _scene(oracle, omesh, ocam, x, q)
    x2 = np.stack([x + [0.02, 0.0, 0.03], x + [0.001, 0.0, 0.0]])
    q2 = np.stack([_turn(q, 0.2, [0, 1, 0]), q])
    for kw in (dict(bands=1), dict(bands=4, split=True), dict(bands=8, split=False, window_pixels=320)):
        want = ops.outlier_test(dcam, 2, depth, mask, mesh, x2, q2, **kw)
        Lv, ns, sel, t = np.zeros(2), np.zeros(2, np.int64), C.c_int(-2), np.zeros_like(want[3])
        L.check(lib.roft_outlier_test_mode(C.byref(dcam), 2, depth.ctypes.data, mask.ctypes.data, C.byref(mesh), x2.ctypes.data,
                                           q2.ctypes.data, kw["bands"], 1, kw.get("window_pixels", 0),
                                           -1 if "split" not in kw else int(kw["split"]), L.RENDER_CONTRACT,
                                           Lv.ctypes.data, ns.ctypes.data, C.byref(sel), t.ctypes.data))
        assert list(Lv) == list(want[0]) and list(ns) == list(want[1]) and sel.value == want[2] and np.array_equal(t, want[3])

"""A bad mesh is refused before the device at every entry point that takes one, in the same words: each site runs the one host
check (check_mesh, roft_amd/csrc/engine_internal.h) ahead of anything that looks for a device, so the answer is ROFT_ERR_INVALID
with or without one -- and never ROFT_ERR_DEVICE.  An absent mesh (no vertices or no triangles) is the site's own policy: the pose
silhouettes, track quality and a restart on an engine that needs no mesh take it, the others refuse it.
And the one Python conversion (ops.mesh_of): arrays of any layout and dtype become the (n, 3) float32 / int32 arrays a roft_mesh names."""
import ctypes as C

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import ops, synth

INVALID, DEVICE = -1, -2
W, H = 64, 48
CAM = L.Camera(W, H, 150.0, 150.0, 32.0, 24.0)
VERTS, TRIS = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, 2)
VERTS, TRIS = np.ascontiguousarray(VERTS, np.float32), np.ascontiguousarray(TRIS, np.int32)
X, Q = np.array([0.0, 0.0, 0.6]), np.array([1.0, 0.0, 0.0, 0.0])
X2, Q2 = np.concatenate([X, X]), np.concatenate([Q, Q])
DEPTH, MASK = np.full((H, W), 0.6, np.float32), np.full((H, W), 255, np.uint8)


def _bad_index(row, col, value):
    t = TRIS.copy()
    t[row, col] = value
    return t


# name -> (verts or None, tris or None): every one has_mesh, none may reach the rasteriser
BAD_MESHES = {
    "null_verts": (None, TRIS),
    "null_tris": (VERTS, None),
    "minus_one_in_the_first_triangle": (VERTS, _bad_index(0, 0, -1)),
    "n_verts_in_the_last_triangle": (VERTS, _bad_index(len(TRIS) - 1, 2, len(VERTS))),
}


def _mesh(verts, tris):
    return L.Mesh(None if verts is None else verts.ctypes.data, len(VERTS), None if tris is None else tris.ctypes.data, len(TRIS))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _restart_check(mesh):
    cfg = E.default_config(320, 240)
    cfg.outlier_rejection = 0          # (an engine that needs no mesh: what is refused is the mesh itself)
    d = E.default_object()
    d.mesh = mesh
    one, zero, ids = (C.c_int * 1)(1), (C.c_int * 1)(0), (C.c_int * 1)(0)
    return L.lib().roft_debug_restart_check(C.byref(cfg), 1, one, zero, 0, ids, (L.ObjectDesc * 1)(d), 1, 0)


def _silhouette(mesh):
    out, n = np.zeros((H, W), np.uint8), C.c_int(0)
    return L.lib().roft_pose_silhouette(C.byref(CAM), C.byref(mesh), _p(X), _p(Q), 0, 1, _p(out), C.byref(n))


def _pair(mesh):
    return (L.Mesh * 2)(_mesh(VERTS, TRIS), mesh)   # (the second of two: the loop over the meshes goes on behind a good one)


def _occluded(mesh):
    out, n = np.zeros((2, H, W), np.uint8), np.zeros(2, np.int32)
    return L.lib().roft_pose_silhouettes_occluded(C.byref(CAM), _pair(mesh), 2, _p(X2), _p(Q2), 0, 1, _p(out), n.ctypes.data_as(C.POINTER(C.c_int)))


def _gated(mesh):
    out, n, removed = np.zeros((2, H, W), np.uint8), np.zeros(2, np.int32), np.zeros((2, 2), np.int32)
    gate, ip = L.PoseMaskGate(0.02, 0.0), C.POINTER(C.c_int)
    return L.lib().roft_pose_silhouettes_gated(C.byref(CAM), _pair(mesh), 2, _p(X2), _p(Q2), _p(DEPTH), C.byref(gate), 0, 1, _p(out),
                                               n.ctypes.data_as(ip), removed.ctypes.data_as(ip))


def _outlier(variant):
    def call(mesh):
        Lo, cnt, sel = np.zeros(2), (C.c_long * 2)(), C.c_int(0)
        head = (C.byref(CAM), 2, _p(DEPTH), _p(MASK), C.byref(mesh), _p(X2), _p(Q2), 0, 1, 0)
        tail = (_p(Lo), C.cast(cnt, C.c_void_p), C.byref(sel), None)
        if variant == "plain":
            return L.lib().roft_outlier_test(*head, *tail)
        if variant == "split":
            return L.lib().roft_outlier_test_split(*head, -1, *tail)
        return L.lib().roft_outlier_test_mode(*head, -1, L.RENDER_GL, *tail)
    return call


def _render_depth(mesh):
    tile = np.zeros((H // 2, W // 2), np.float32)
    return L.lib().roft_render_depth(C.byref(mesh), _p(X), _p(Q), C.byref(CAM), 2, _p(tile))


def _render_depth_mode(mesh):
    tile = np.zeros((H // 2, W // 2), np.float32)
    return L.lib().roft_render_depth_mode(C.byref(mesh), _p(X), _p(Q), C.byref(CAM), 2, L.RENDER_GL, _p(tile))


def _quality(mesh):
    rec = L.QualityRecord()
    return L.lib().roft_track_quality(C.byref(CAM), 2, _p(DEPTH), _p(MASK), C.byref(mesh), _p(X), _p(Q), 0.01, 2.0, 0, C.byref(rec))


def _scene_create(mesh):
    h = C.c_void_p()
    rc = L.lib().roft_scene_renderer_create(C.byref(CAM), _pair(mesh), 2, 1, 0, C.byref(h))
    if rc == 0:
        L.lib().roft_scene_renderer_destroy(h)
    return rc


def _render_scene(mesh):
    d, keep = ops._scene_desc(W, H, [0], np.concatenate([X, Q])[None, None], None, None, False, None, 0)
    rgb = np.zeros((1, H, W, 3), np.uint8)
    return L.lib().roft_render_scene(C.byref(CAM), _pair(mesh), 2, C.byref(d), _p(rgb), None, None, None)


# entry point -> (the call, does it take an absent mesh?)
ENTRY_POINTS = {
    "roft_debug_restart_check": (_restart_check, True),
    "roft_pose_silhouette": (_silhouette, True),
    "roft_pose_silhouettes_occluded": (_occluded, True),
    "roft_pose_silhouettes_gated": (_gated, True),
    "roft_outlier_test": (_outlier("plain"), False),
    "roft_outlier_test_split": (_outlier("split"), False),
    "roft_outlier_test_mode": (_outlier("mode"), False),
    "roft_render_depth": (_render_depth, False),
    "roft_render_depth_mode": (_render_depth_mode, False),
    "roft_track_quality": (_quality, True),
    "roft_scene_renderer_create": (_scene_create, False),
    "roft_render_scene": (_render_scene, False),
}


@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_a_bad_mesh_is_refused_before_the_device(entry):
    call, takes_absent = ENTRY_POINTS[entry]
    for name, (verts, tris) in BAD_MESHES.items():
        rc = call(_mesh(verts, tris))
        msg = L.lib().roft_last_error_string()
        assert rc == INVALID, (name, rc, msg)
        assert (b"refers to vertex" in msg) if name.endswith("triangle") else (b"null" in msg), (name, msg)
    # the report names the triangle and the vertex
    call(_mesh(VERTS, _bad_index(5, 1, len(VERTS) + 3)))
    assert b"triangle 5 refers to vertex %d of %d" % (len(VERTS) + 3, len(VERTS)) in L.lib().roft_last_error_string()
    for absent in (L.Mesh(None, 0, None, 0), L.Mesh(VERTS.ctypes.data, len(VERTS), TRIS.ctypes.data, 0), L.Mesh(VERTS.ctypes.data, 0, TRIS.ctypes.data, len(TRIS))):
        rc = call(absent)
        if takes_absent:
            assert rc != INVALID, (rc, L.lib().roft_last_error_string())   # (ROFT_OK on a device, ROFT_ERR_DEVICE without one)
        else:
            assert rc == INVALID, rc
    if L.lib().roft_device_count() <= 0 and entry != "roft_debug_restart_check":
        assert call(_mesh(VERTS, TRIS)) == DEVICE   # (what every refusal above came before)


# ---- ops.mesh_of: (verts, tris) -> (L.Mesh, the arrays it points into) -------------------------------------------------------------
def _bytes(mesh):
    return C.string_at(mesh.verts, 12 * mesh.n_verts), C.string_at(mesh.tris, 12 * mesh.n_tris)


@pytest.mark.parametrize("via", ["mesh_of", "make_mesh"])
def test_any_layout_and_dtype_gives_the_plain_arrays(via):
    def convert(v, t):
        if via == "mesh_of":
            return ops.mesh_of(v, t)
        m = ops.make_mesh(v, t)
        return m, m._keep

    want = (VERTS.tobytes(), TRIS.tobytes())
    transposed_v, transposed_t = np.asfortranarray(VERTS).T.copy().T, np.ascontiguousarray(TRIS.T).T   # (n, 3) views of (3, n) memory
    assert not transposed_v.flags["C_CONTIGUOUS"] and not transposed_t.flags["C_CONTIGUOUS"]
    cases = {
        "plain": (VERTS, TRIS),
        "flat_float64_and_int64": (VERTS.astype(np.float64).reshape(-1), TRIS.astype(np.int64).reshape(-1)),
        "lists": (VERTS.tolist(), TRIS.tolist()),
        "transposed_views": (transposed_v, transposed_t),
        "int64_triangles": (VERTS, TRIS.astype(np.int64)),
    }
    for name, (v, t) in cases.items():
        mesh, keep = convert(v, t)
        assert isinstance(mesh, L.Mesh) and (mesh.n_verts, mesh.n_tris) == (len(VERTS), len(TRIS)), name
        assert _bytes(mesh) == want, name
        assert keep[0].dtype == np.float32 and keep[1].dtype == np.int32 and keep[0].shape == VERTS.shape and keep[1].shape == TRIS.shape
        assert keep[0].flags["C_CONTIGUOUS"] and keep[1].flags["C_CONTIGUOUS"]
        assert (mesh.verts, mesh.tris) == (keep[0].ctypes.data, keep[1].ctypes.data)
    assert ops.make_mesh(VERTS, TRIS)._keep[0] is not None
    arr, keep = ops._mesh_array([cases["flat_float64_and_int64"], cases["transposed_views"]])
    assert [_bytes(arr[k]) for k in range(2)] == [want, want] and len(keep) == 2
    none, _ = ops.mesh_of(np.zeros((0, 3)), np.zeros((0, 3)))
    assert (none.n_verts, none.n_tris) == (0, 0)

"""Track quality without a GPU: the contract's declarations (include/roft_engine.h, section 3d) and their ctypes mirrors, the
refusals roft_track_quality makes before it looks for a device, the place of the launch in a batch's plan (batch_plan.h), and the
properties of the reference the GPU tests compare with (tests/quality_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi_header
import mesh_zoo
import quality_ref as qr
from roft_amd import _lib as L
from roft_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roft_amd", "csrc")
# (W, H, d): the shapes of the GPU tests and the engine's 320 x 240
SHAPES = [(128, 96, 4), (64, 64, 2), (64, 50, 4), (640, 480, 2), (320, 240, 4)]
Q0 = (1.0, 0.0, 0.0, 0.0)


def header_fields(name):
    return dict(abi_header.structs())[name]


def test_mirrors_have_the_headers_field_lists():
    assert [n for n, _ in L.QualityRecord._fields_] == header_fields("roft_quality_record") == list(ops.QUALITY_DTYPE.names) == list(qr.FIELDS)
    assert [n for n, _ in L.QualityParams._fields_] == header_fields("roft_quality_params")
    # the two structs every submit and every result go through: untouched
    assert [n for n, _ in L.FrameInput._fields_] == header_fields("roft_frame_input")
    assert [n for n, _ in L.ObjectOutput._fields_] == header_fields("roft_object_output")


def test_sizes_and_offsets_against_gcc(tmp_path):
    structs = {"roft_quality_record": L.QualityRecord, "roft_quality_params": L.QualityParams, "roft_frame_input": L.FrameInput,
               "roft_object_output": L.ObjectOutput}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "roft_engine.h"', 'int main(void) {', '  printf("%d\\n", ROFT_ABI_VERSION);']
    for cname, mirror in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in mirror._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(out[0]) == 2
    got = dict((k, int(v)) for k, v in (line.split() for line in out[1:] if line))
    for cname, mirror in structs.items():
        assert got[cname] == C.sizeof(mirror), cname
        for f, _ in mirror._fields_:
            assert got["%s.%s" % (cname, f)] == getattr(mirror, f).offset, (cname, f)
    assert got["roft_quality_record"] == 40 == ops.QUALITY_DTYPE.itemsize
    assert [ops.QUALITY_DTYPE.fields[f][1] for f in ops.QUALITY_DTYPE.names] == [getattr(L.QualityRecord, f).offset for f in ops.QUALITY_DTYPE.names]
    # roft_frame_input and roft_object_output as ABI version 2 has always had them
    assert got["roft_frame_input"] == 120 and got["roft_object_output"] == 176


def test_library_exports_the_symbols():
    lib = L.lib()
    assert lib.roft_abi_version() == 2
    p = L.QualityParams(0, 0.0)
    assert lib.roft_default_quality_params(C.byref(p)) == 0 and p.every == 1 and p.depth_tolerance == np.float32(0.01)
    assert lib.roft_default_quality_params(None) == -1


def test_track_quality_refuses_before_it_looks_for_a_device():
    lib = L.lib()
    W, H = 64, 64
    cam = L.Camera(W, H, 58.0, 58.0, 31.5, 31.5)
    v, t = mesh_zoo.box()
    mesh = ops.make_mesh(v, t)
    depth, mask = np.zeros((H, W), np.float32), np.zeros((H, W), np.uint8)
    x, q = np.array([0.0, 0.0, 0.5]), np.array(Q0)
    rec = L.QualityRecord()
    good = dict(cam=C.byref(cam), divider=2, depth=depth.ctypes.data, mask=mask.ctypes.data, mesh=C.byref(mesh), x=x.ctypes.data,
                q=q.ctypes.data, tol=0.01, dmax=2.0, win=0, out=C.byref(rec))

    def call(**over):
        a = dict(good, **over)
        return lib.roft_track_quality(a["cam"], a["divider"], a["depth"], a["mask"], a["mesh"], a["x"], a["q"], a["tol"], a["dmax"], a["win"], a["out"])

    for key in ("cam", "depth", "mask", "mesh", "x", "q", "out"):
        assert call(**{key: None}) == -1, key
    for bad in (dict(divider=0), dict(divider=-2), dict(tol=-0.001), dict(tol=float("nan")), dict(win=-1)):
        assert call(**bad) == -1, bad
        assert lib.roft_last_error_string()
    # (and the complete call is not refused for its arguments: it runs, or finds no device)
    assert call() in (0, -2)


def test_plan_adds_exactly_the_launch_and_its_event(tmp_path):
    exe = str(tmp_path / "quality_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "quality_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) > 10000


def test_launcher_shapes_equal_the_recorded_ones(tmp_path):
    """raster_shape.h's three launcher rules against tests/golden/raster_shapes.json, every field of every row"""
    exe = str(tmp_path / "raster_shape_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "raster_shape_check.cpp"), "-o", exe])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "raster_shapes.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == 3 * 224 + 224   # 8 meshes x 7 widths x 4 window_pixels, the scene's on two targets each


# ---- the reference's own properties --------------------------------------------------------------------------------------

def camera_of(oracle, W, H):
    f = 0.9 * W
    return oracle.camera(W, H, f, f, W / 2 - 0.5, H / 2 - 0.5)


@pytest.fixture(scope="module")
def aligned(oracle):
    """Per shape: (camera, d, tile at the pose, M = upsampled silhouette, D = upsampled tile)."""
    out = {}
    mesh = mesh_zoo.box()
    for W, H, d in SHAPES:
        cam = camera_of(oracle, W, H)
        x = np.array([0.01, -0.005, 0.5])
        tile = oracle.render_depth(oracle.make_mesh(*mesh), x, Q0, cam, d)
        r = qr.upsample(tile, d, H, W)
        out[(W, H, d)] = (cam, x, tile, r != 0, r.copy())
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_aligned(oracle, aligned, shape):
    cam, x, tile, M, D = aligned[shape]
    exact = []
    rec = qr.quality(oracle, cam, shape[2], D, M, mesh_zoo.box(), x, Q0, check_exact=exact)
    assert rec["n_both"] == rec["n_mask"] == rec["n_render"] > 0
    assert rec["n_depth"] == rec["n_both"] and rec["n_front"] == rec["n_behind"] == 0
    assert rec["depth_err"] == 0.0 and rec["frame"] == 0 and rec["reserved"] == 0
    assert exact and all(exact)


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_mask_moved(oracle, aligned, shape):
    cam, x, tile, M, D = aligned[shape]
    M2 = np.zeros_like(M)
    M2[2:, 3:] = M[:-2, :-3]
    rec = qr.quality(oracle, cam, shape[2], D, M2, mesh_zoo.box(), x, Q0)
    assert rec["n_mask"] == int(M2.sum()) and rec["n_render"] == int(M.sum())
    assert rec["n_both"] == rec["n_mask"] + rec["n_render"] - int((M2 | M).sum())
    assert 0 < rec["n_both"] < rec["n_render"]
    assert rec["n_depth"] == rec["n_both"] and rec["depth_err"] == 0.0   # (D is the render wherever the render is)


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_pose_moved_sideways(oracle, aligned, shape):
    cam, x, tile, M, D = aligned[shape]
    rec = qr.quality(oracle, cam, shape[2], D, M, mesh_zoo.box(), x + [0.30, 0.0, 0.0], Q0)
    assert rec["n_both"] == 0 and rec["n_render"] > 0 and rec["n_mask"] == int(M.sum())
    assert rec["n_depth"] == 0 and rec["depth_err"] == qr.DBL_MAX


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("x", [(0.0, 0.0, -0.5), (5.0, 0.0, 0.5), (0.0, -5.0, 0.5)], ids=["behind", "off_right", "off_top"])
def test_reference_nothing_rendered(oracle, aligned, shape, x):
    cam, _, tile, M, D = aligned[shape]
    rec = qr.quality(oracle, cam, shape[2], D, M, mesh_zoo.box(), np.array(x), Q0)
    assert rec["n_render"] == 0 and rec["n_both"] == 0 and rec["n_mask"] == int(M.sum()) and rec["depth_err"] == qr.DBL_MAX
    assert qr.same(rec, qr.quality(oracle, cam, shape[2], D, M, None, np.array(x), Q0))   # ... as an object without a mesh


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_validity(oracle, aligned, shape):
    cam, x, tile, M, D = aligned[shape]
    vs, us = np.nonzero(M)
    assert len(vs) >= 4
    D2 = D.copy()
    D2[vs[0], us[0]] = 0.0
    D2[vs[1], us[1]] = np.nan
    D2[vs[2], us[2]] = 2.0        # >= depth_maximum
    D2[vs[3], us[3]] = -0.3
    full = qr.quality(oracle, cam, shape[2], D, M, mesh_zoo.box(), x, Q0)
    rec = qr.quality(oracle, cam, shape[2], D2, M, mesh_zoo.box(), x, Q0)
    assert rec["n_both"] == full["n_both"] and rec["n_depth"] == full["n_depth"] - 4
    assert rec["depth_err"] == 0.0 and rec["n_front"] == rec["n_behind"] == 0
    below = np.nextafter(np.float32(2.0), np.float32(0.0))
    D2[vs[2], us[2]] = below      # the largest float below depth_maximum counts again
    assert qr.quality(oracle, cam, shape[2], D2, M, mesh_zoo.box(), x, Q0)["n_depth"] == full["n_depth"] - 3


def test_reference_tolerance_boundary():
    """e == -+tolerance exactly is neither in front nor behind; one ulp further it is."""
    tol = np.float32(2.0 ** -7)
    tile = np.full((4, 4), 0.5, np.float32)
    M = np.ones((8, 8), bool)
    D = np.full((8, 8), 0.5, np.float32)
    D[0, 0], D[0, 1] = 0.5 + tol, 0.5 - tol
    D[1, 0], D[1, 1] = np.nextafter(np.float32(0.5 + tol), np.float32(1)), np.nextafter(np.float32(0.5 - tol), np.float32(0))
    exact = []
    rec = qr.quality_from_tile(tile, 2, M, D, tol, 2.0, check_exact=exact)
    assert (D[0, 0] - np.float32(0.5)) == tol and (D[0, 1] - np.float32(0.5)) == -tol
    assert rec["n_depth"] == 64 and rec["n_behind"] == 1 and rec["n_front"] == 1
    assert all(exact)
    total = sum(abs(float(np.float32(D[v, u] - np.float32(0.5)))) for v in range(2) for u in range(2))   # exact in doubles: four small dyadic terms
    assert rec["depth_err"] == total / 64.0


def test_reference_fixed_point_is_exact_for_depths_in_metres():
    """Every |e| that float depths in metres produce is its own fixed-point image: millimetre readings against renders."""
    rng = np.random.default_rng(3)
    raw = rng.integers(1, 4000, 4096).astype(np.float32) * np.float32(0.001)
    render = rng.uniform(0.2, 3.0, 4096).astype(np.float32)
    for t in np.abs(raw - render).astype(np.float32):
        hi, lo = qr.term_integers(t)
        assert (hi << 32) + lo == int(float(t) * 2.0 ** 64) and float(t) * 2.0 ** 64 == float(int(float(t) * 2.0 ** 64))
        assert qr.value(hi, lo) == float(t)
    assert qr.term_integers(np.float32(1000.0)) == (256 << 32, 0)   # the cap

"""The scene renderer without a device: its CPU reference against the oracle, every argument refusal, and the pose
pre-processing and sheet geometry of tools/render_results.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import io, ops

import scene_ref
import scene_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("name", sorted(su.zoo()))
def test_reference_depth_is_the_oracles_bit_for_bit(name):
    """Keeps tests/scene_ref.py honest: its depth plane equals oracle/ro_render.c at divider 1 on every zoo mesh at three poses
    (one with the camera 2 cm from the object's centre), at 160 x 120."""
    for pose_id in range(len(su.POSES)):
        ref = su.reference(name, pose_id, su.SIZES[0])
        want = su.oracle_depth(name, pose_id, su.SIZES[0])
        assert su.same_bits(ref["depth"], want), (name, pose_id)
        assert np.array_equal(ref["instance"] >= 0, want > 0) and np.array_equal(ref["triangle"] >= 0, want > 0)
    assert any((su.oracle_depth(name, k, su.SIZES[0]) > 0).sum() > 500 for k in range(3)), "the cases draw something"


def test_header_library_and_binding_declare_the_entry_points():
    """(declarations, exports, rows, struct layouts and ROFT_SCENE_MAX_INSTANCES: tests/test_abi_cpu.py, for every name of the header)"""
    assert L.ABI_VERSION == 2 and L.lib().roft_abi_version() == 2, "no existing struct changed: the ABI version stays"


def _call(cam, meshes, n_meshes, desc, outs=None):
    outs = outs or [None] * 4
    return L.lib().roft_render_scene(cam, meshes, n_meshes, desc, *outs)


def _valid_case():
    v, t, _ = su.zoo()["box"]
    cam = su.lib_cam(su.cam(64, 48))
    meshes, keep = ops._mesh_array([(v, t)])
    desc, keep_d = ops._scene_desc(64, 48, [0], su.POSES[0][None, None], None, None, False, None, 0)
    return cam, meshes, desc, (keep, keep_d, v, t)


def _refused(rc):
    assert rc == -1, "expected ROFT_ERR_INVALID, got %d" % rc
    assert len(L.lib().roft_last_error_string()) > 0


def test_every_refusal_comes_before_the_device():
    """ROFT_ERR_INVALID with its reason for every bad argument, on a machine without a device as well: nothing here reaches it."""
    cam, meshes, desc, keep = _valid_case()
    v, t = keep[2], keep[3]
    rgb = np.full((1, 48, 64, 3), 7, np.uint8)
    outs = [rgb.ctypes.data, None, None, None]
    # NULL required pointers
    _refused(_call(None, meshes, 1, C.byref(desc), outs))
    _refused(_call(C.byref(cam), None, 1, C.byref(desc), outs))
    _refused(_call(C.byref(cam), meshes, 1, None, outs))
    h = C.c_void_p()
    _refused(L.lib().roft_scene_renderer_create(C.byref(cam), meshes, 1, 4, 0, None))
    _refused(L.lib().roft_scene_renderer_create(C.byref(cam), meshes, 1, 0, 0, C.byref(h)))
    _refused(L.lib().roft_scene_render(None, C.byref(desc), *outs))
    _refused(L.lib().roft_debug_scene_kernel_ms(None, None))

    def with_desc(**kw):
        d, k = ops._scene_desc(64, 48, [0], su.POSES[0][None, None], None, None, False, None, 0)
        for name, val in kw.items():
            setattr(d, name, val)
        return d, k

    for kw in (dict(mesh_index=None), dict(poses=None), dict(n_instances=-1), dict(n_instances=257), dict(n_frames=-1), dict(window_pixels=-1)):
        d, k = with_desc(**kw)
        _refused(_call(C.byref(cam), meshes, 1, C.byref(d), outs))
    # mesh_index out of range
    for bad in (1, -1):
        d, k = ops._scene_desc(64, 48, [bad], su.POSES[0][None, None], None, None, False, None, 0)
        _refused(_call(C.byref(cam), meshes, 1, C.byref(d), outs))
    # a background for another number of frames
    d, k = ops._scene_desc(64, 48, [0], su.POSES[0][None, None], None, np.zeros((1, 48, 64, 3), np.uint8), False, None, 0)
    d.background_frames = 2
    _refused(_call(C.byref(cam), meshes, 1, C.byref(d), outs))
    # styles: opacity / ambient outside [0, 1] or not finite
    for style in ((9, 9, 9), 1.5, 0.3), ((9, 9, 9), -0.1, 0.3), ((9, 9, 9), float("nan"), 0.3), ((9, 9, 9), 0.5, 1.01), ((9, 9, 9), 0.5, float("inf")), \
            ((9, 9, 9), 0.5, float("nan")):
        d, k = ops._scene_desc(64, 48, [0], su.POSES[0][None, None], None, None, False, [style], 0)
        _refused(_call(C.byref(cam), meshes, 1, C.byref(d), outs))
    # meshes: an index out of range, null arrays, 2^24 triangles (only the count is looked at before the refusal)
    t_bad = t.copy()
    t_bad[5, 1] = len(v)
    m_bad, k = ops._mesh_array([(v, t_bad)])
    _refused(_call(C.byref(cam), m_bad, 1, C.byref(desc), outs))
    assert b"vertex" in L.lib().roft_last_error_string()
    t_neg = t.copy()
    t_neg[0, 0] = -1
    m_bad, k = ops._mesh_array([(v, t_neg)])
    _refused(_call(C.byref(cam), m_bad, 1, C.byref(desc), outs))
    m_big = (L.Mesh * 1)(L.Mesh(v.ctypes.data, len(v), t.ctypes.data, 1 << 24))
    _refused(_call(C.byref(cam), m_big, 1, C.byref(desc), outs))
    assert b"2^24" in L.lib().roft_last_error_string()
    m_null = (L.Mesh * 1)(L.Mesh(None, len(v), t.ctypes.data, len(t)))
    _refused(_call(C.byref(cam), m_null, 1, C.byref(desc), outs))
    # the image: W * H >= 2^24, and sizes below 1
    for w, hgt in ((4096, 4096), (0, 48), (64, -1)):
        _refused(_call(C.byref(L.Camera(w, hgt, 150.0, 150.0, 32.0, 24.0)), meshes, 1, C.byref(desc), outs))
    assert np.all(rgb == 7), "a refused call touches nothing"


def test_no_frames_is_ok_and_there_is_no_cpu_path():
    cam, meshes, desc, keep = _valid_case()
    rgb = np.full((1, 48, 64, 3), 7, np.uint8)
    d0, k = ops._scene_desc(64, 48, [0], np.zeros((0, 1, 7)), None, None, False, None, 0)
    assert d0.n_frames == 0
    assert _call(C.byref(cam), meshes, 1, C.byref(d0), [rgb.ctypes.data, None, None, None]) == 0   # with or without a device
    assert np.all(rgb == 7)
    # an odd size is accepted: this path does not have the engine's multiple-of-32 rule (the refusal below is the device's)
    if L.lib().roft_device_count() > 0:
        return   # (tests/test_scene_gpu.py renders on it)
    assert _call(C.byref(cam), meshes, 1, C.byref(desc), [rgb.ctypes.data, None, None, None]) == -2
    assert b"no such HIP device" in L.lib().roft_last_error_string() or b"CPU" in L.lib().roft_last_error_string()
    odd = L.Camera(93, 71, 150.0, 150.0, 46.5, 35.5)
    assert _call(C.byref(odd), meshes, 1, C.byref(desc), [np.zeros((1, 71, 93, 3), np.uint8).ctypes.data, None, None, None]) == -2
    with pytest.raises(L.RoftError):
        ops.render_scene(cam, [(keep[2], keep[3])], [0], su.POSES[0][None, None])
    with pytest.raises(L.RoftError):
        ops.SceneRenderer(cam, [(keep[2], keep[3])])
    assert np.all(rgb == 7)


# ---- tools/render_results.py without a device ------------------------------------------------------------------
def test_invalid_rows_repeat_the_last_valid_pose_and_keep_their_place():
    import render_results as rr
    pose = np.zeros((7, 7))
    pose[:, 3] = 1.0
    valid = np.array([0, 0, 1, 0, 1, 0, 0], bool)
    pose[2, :3] = [0.1, 0.2, 0.5]
    pose[4, :3] = [0.3, 0.1, 0.6]
    out, drawn = rr.fill_poses(pose, valid)
    assert list(drawn) == [False, False, True, True, True, True, True], "leading invalid rows show the background only"
    assert np.array_equal(out[2], pose[2]) and np.array_equal(out[3], pose[2]), "an invalid row repeats the last valid one"
    assert np.array_equal(out[4], pose[4]) and np.array_equal(out[5], pose[4]) and np.array_equal(out[6], pose[4])
    assert len(out) == len(pose), "no row is dropped: frame i stays image i"
    none, drawn = rr.fill_poses(pose, np.zeros(7, bool))
    assert not drawn.any()


def test_dry_run_reads_both_file_kinds_and_shifts_nothing(tmp_path):
    import render_results as rr
    rng = np.random.default_rng(3)
    n = 6
    pose7 = np.concatenate([rng.uniform(-0.1, 0.1, (n, 2)), rng.uniform(0.4, 0.6, (n, 1)), rng.normal(size=(n, 4))], 1)
    pose7[:, 3:] /= np.linalg.norm(pose7[:, 3:], axis=1, keepdims=True)
    valid = np.array([0, 1, 1, 0, 1, 1], bool)
    io.write_poses(str(tmp_path / "poses.txt"), pose7, valid)
    pose13 = np.concatenate([np.zeros((n, 6)), pose7], 1)
    io.write_estimate_logs(str(tmp_path / "run_"), pose13, np.zeros((n, 6)))
    json.dump(dict(width=64, height=48, fx=150.0, fy=150.0, cx=32.0, cy=24.0), open(tmp_path / "cam_K.json", "w"))
    # a poses.txt (7 columns) and a pose_estimate log (13 columns) of the same poses read alike
    a, va = rr.load_pose_source(str(tmp_path / "poses.txt"))
    b, vb = rr.load_pose_source(str(tmp_path / "run_pose_estimate"))
    assert list(va) == list(valid) and vb.all()
    assert np.allclose(a[valid], b[valid], atol=1e-9) and np.allclose(a[valid, :3], pose7[valid, :3], atol=1e-12)
    argv = ["--root", str(tmp_path), "--mesh", "a.obj", "--poses", str(tmp_path / "poses.txt"), "--mesh", "b.obj", "--poses",
            str(tmp_path / "run_pose_estimate"), "--out", str(tmp_path / "o"), "--dry-run", "--frames-per-call", "4"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_results.py")] + argv, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["frames"] == list(range(n)) and rep["sources"] == 2 and rep["chunks"] == 2
    assert rep["background_only"] == [[0], []], "frame 0 of the detections has no pose yet; its index stays 0"
    assert not os.path.exists(tmp_path / "o"), "a dry run writes nothing"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_results.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "ffmpeg" in r.stdout and "mp4" in r.stdout


def test_thumbnail_geometry_three_frames_two_sources():
    import render_results as rr
    h, w = 20, 30
    rows = [[np.full((h, w, 3), 10 * r + c, np.uint8) for c in range(3)] for r in range(3)]   # the RGB row + two sources
    sheet = rr.thumbnail_sheet(rows)
    assert sheet.shape == (3 * h + 2 * 10, 3 * w + 2 * 10, 3) and sheet.dtype == np.uint8
    for r in range(3):
        for c in range(3):
            cell = sheet[(h + 10) * r:(h + 10) * r + h, (w + 10) * c:(w + 10) * c + w]
            assert np.all(cell == 10 * r + c)
    mask = np.ones(sheet.shape[:2], bool)
    for r in range(3):
        for c in range(3):
            mask[(h + 10) * r:(h + 10) * r + h, (w + 10) * c:(w + 10) * c + w] = False
    assert np.all(sheet[mask] == 255), "10-pixel white borders between the cells, none around the sheet"
    assert mask[:h, w:w + 10].all() and mask[h:h + 10, :].all()
    img = np.arange(48 * 64 * 3, dtype=np.uint8).reshape(48, 64, 3)
    assert rr.crop_image(img, (8, 4, 40, 30)).shape == (26, 32, 3) and rr.crop_image(img, None) is img
    assert rr.chunks(range(7), 3) == [[0, 1, 2], [3, 4, 5], [6]]

"""The scene renderer on the device (roft_scene_render / roft_render_scene, roft_amd/csrc/k_scene.hip) against the unchanged oracle
and tests/scene_ref.py: single meshes, occlusion between instances, the determinism contract, the edges of the interface, the path
from a tracked sequence to PNG files, and one large shape."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import io, ops, synth
from oracle import binding as ob

import mesh_zoo
import scene_ref
import scene_util as su
import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUTPUTS = ("rgb", "depth", "instance", "triangle")
RGB_LEVELS = 1   # per channel, against tests/scene_ref.py


def rgb_close(a, b):
    return a.shape == b.shape and np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= RGB_LEVELS


def same(a, b):
    return all(su.same_bits(a[k], b[k]) for k in a) and set(a) == set(b)


# ---- 1. one instance, every zoo mesh, three poses ---------------------------------------------------------------------
@pytest.mark.parametrize("size", su.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(su.zoo()))
def test_single_mesh_against_oracle_and_reference(name, size):
    """depth == oracle.render_depth(..., 1) bit for bit, triangle == scene_ref exactly, instance == 0 where covered, rgb within one
    level per channel of scene_ref: depth and ids are exact, so colour can differ only through the last ulp of the float shade, and
    floorf(c + 0.5f) turns that into at most one level."""
    v, t, _ = su.zoo()[name]
    cam = su.lib_cam(su.cam(*size))
    out = ops.render_scene(cam, [(v, t)], [0], np.stack(su.POSES)[:, None])
    for k in range(len(su.POSES)):
        want = su.oracle_depth(name, k, size)
        ref = su.reference(name, k, size)
        assert su.same_bits(out["depth"][k], want), (name, k)
        assert np.array_equal(out["triangle"][k], ref["triangle"]), (name, k)
        assert np.array_equal(out["instance"][k], np.where(want > 0, 0, -1)), (name, k)
        diff = np.abs(out["rgb"][k].astype(np.int32) - ref["rgb"].astype(np.int32))
        print("%s pose %d %dx%d: rgb max |diff| %d, pixels differing %d of %d covered" % (name, k, size[0], size[1], diff.max(),
                                                                                          int((diff.max(axis=2) > 0).sum()), int((want > 0).sum())))
        assert diff.max() <= RGB_LEVELS, (name, k)


# ---- 2. occlusion, decided by the oracle alone ------------------------------------------------------------------------
def _box(scale=1.0):
    v, t = mesh_zoo.box(6)
    return (v * np.float32(scale)).astype(np.float32), t


def _occlusion_scenes():
    box, small = _box(), _box(0.6)
    torus = su.zoo()["torus"][:2]
    return {
        "two_boxes_one_behind": ([box, box], [su.pose([0.0, 0.0, 0.40], [1, 2, 3], 0.5), su.pose([0.03, 0.01, 0.55], [2, 1, 0], 0.9)]),
        "three_boxes_in_a_row": ([box, small, box], [su.pose([0.04, 0.0, 0.60], [1, 0, 1], 0.3), su.pose([-0.01, 0.01, 0.35], [0, 1, 1], 1.2),
                                                     su.pose([-0.03, -0.01, 0.47], [1, 1, 1], 2.0)]),
        "box_pushed_through_box": ([box, box], [su.pose([0.0, 0.0, 0.42], [1, 2, 3], 0.5), su.pose([0.02, 0.0, 0.43], [3, 1, 2], 1.7)]),
        "same_box_twice": ([box, box], [su.pose([0.0, 0.0, 0.42], [1, 2, 3], 0.5), su.pose([0.0, 0.0, 0.42], [1, 2, 3], 0.5)]),
        "torus_around_box": ([small, torus], [su.pose([0.0, 0.0, 0.40], [1, 0, 0], 0.2), su.pose([0.0, 0.0, 0.40], [1, 0.3, 0], 1.1)]),
    }


@pytest.mark.parametrize("size", su.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("scene", sorted(_occlusion_scenes()))
def test_occlusion_is_the_oracles_per_pixel_nearest(scene, size):
    meshes, poses = _occlusion_scenes()[scene]
    c = su.cam(*size)
    singles = np.stack([ob.render_depth(ob.make_mesh(v, t), p[:3], p[3:], su.oracle_cam(c), 1) for (v, t), p in zip(meshes, poses)])
    far = np.where(singles > 0, singles, np.float32(np.inf))
    want_inst = np.where(np.isfinite(far.min(0)), far.argmin(0), -1)    # (argmin: the lowest instance among equal depths)
    want_depth = np.where(np.isfinite(far.min(0)), far.min(0), np.float32(0)).astype(np.float32)
    out = ops.render_scene(su.lib_cam(c), meshes, np.arange(len(meshes)), np.stack(poses)[None], outputs=("depth", "instance"))
    assert su.same_bits(out["depth"][0], want_depth)
    assert np.array_equal(out["instance"][0], want_inst)
    if scene == "same_box_twice":
        assert not (want_inst == 1).any(), "equal depths everywhere: the lower instance wins"
    else:
        assert len(np.unique(want_inst)) == len(meshes) + 1, "every instance and the background are seen"


# ---- 3. determinism contract ---------------------------------------------------------------------------------------
def _busy_frames(n):
    """n different frames of three instances over different backgrounds."""
    rng = np.random.default_rng(11)
    poses = np.stack([[su.pose([rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05), rng.uniform(0.3, 0.6)], rng.normal(size=3), rng.uniform(0, 3))
                       for _ in range(3)] for _ in range(n)])
    bg = rng.integers(0, 256, (n, 120, 160, 3), dtype=np.uint8)
    return poses, bg


def test_a_frame_does_not_depend_on_its_call():
    box, torus = _box(), su.zoo()["torus"][:2]
    cam = su.lib_cam(su.cam(160, 120))
    poses, bg = _busy_frames(7)
    styles = [((250, 40, 40), 0.6, 0.2), ((30, 200, 90), 1.0, 0.5), ((10, 20, 240), 0.3, 0.0)]
    r = ops.SceneRenderer(cam, [box, torus], max_frames_per_call=7)
    kw = dict(gray_background=True, styles=styles)
    alone = r.render([0, 1, 0], poses[2:3], background=bg[2:3], **kw)
    assert (alone["instance"] >= 0).sum() > 1000 and len(np.unique(alone["instance"])) == 4
    for pos in (0, 3, 6):
        order = [k for k in range(7) if k != 2]
        order.insert(pos, 2)
        batch = r.render([0, 1, 0], poses[order], background=bg[order], **kw)
        assert same({k: batch[k][pos:pos + 1] for k in batch}, alone), "position %d of a 7-frame call" % pos
    # window_pixels changes no bit (512 forces strips at 160 x 120), nor does another run
    full = r.render([0, 1, 0], poses, background=bg, **kw)
    for wp in (0, 512, 4096, 100):
        assert same(r.render([0, 1, 0], poses, background=bg, window_pixels=wp, **kw), full), wp
    r.close()
    assert same(ops.render_scene(cam, [box, torus], [0, 1, 0], poses, background=bg, **kw), full), "one-shot call, second run"


# ---- 4. edges ------------------------------------------------------------------------------------------------------
def test_objects_off_screen_and_behind_the_camera():
    v, t = _box()
    size = (93, 71)
    c = su.cam(*size)
    cam = su.lib_cam(c)
    cases = [su.pose([-0.14, 0.0, 0.3], [1, 2, 3], 0.5), su.pose([0.14, 0.0, 0.3], [1, 2, 3], 0.5), su.pose([0.0, -0.11, 0.3], [1, 2, 3], 0.5),
             su.pose([0.0, 0.11, 0.3], [1, 2, 3], 0.5), su.pose([2.0, 0.0, 0.3], [1, 2, 3], 0.5), su.pose([0.0, 0.0, -0.4], [1, 2, 3], 0.5)]
    out = ops.render_scene(cam, [(v, t)], [0], np.stack(cases)[:, None])
    m = ob.make_mesh(v, t)
    for k, p in enumerate(cases):
        want = ob.render_depth(m, p[:3], p[3:], su.oracle_cam(c), 1)
        assert su.same_bits(out["depth"][k], want), k
        covered = int((want > 0).sum())
        if k < 4:
            assert 0 < covered < 0.6 * want.size, "half off-screen on one side"
            edge = (want[:, 0], want[:, -1], want[0], want[-1])[k]
            assert (edge > 0).any(), "the object is cut by that border"
        else:
            assert covered == 0 and (out["instance"][k] == -1).all() and (out["triangle"][k] == -1).all() and (out["rgb"][k] == 0).all()


def test_nan_pose_and_invalid_flag_draw_nothing_and_disturb_nothing():
    box, torus = _box(), su.zoo()["torus"][:2]
    cam = su.lib_cam(su.cam(160, 120))
    poses, bg = _busy_frames(4)
    clean = ops.render_scene(cam, [box, torus], [0, 1, 0], poses, background=bg)
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 2, 3, 6):
            broken = poses.copy()
            broken[1, 1, col] = bad
            out = ops.render_scene(cam, [box, torus], [0, 1, 0], broken, background=bg)
            valid = np.ones((4, 3), np.uint8)
            valid[1, 1] = 0
            want = ops.render_scene(cam, [box, torus], [0, 1, 0], poses, valid=valid, background=bg)
            assert same(out, want), "a non-finite pose is an instance that is not drawn"
            for f in (0, 2, 3):
                assert same({k: out[k][f] for k in out}, {k: clean[k][f] for k in clean}), "other frames are untouched"
            assert not (out["instance"][1] == 1).any() and (clean["instance"][1] == 1).any()
    none = ops.render_scene(cam, [box, torus], [0, 1, 0], poses, valid=np.zeros((4, 3)), background=bg)
    assert (none["instance"] == -1).all() and (none["depth"] == 0).all() and np.array_equal(none["rgb"], bg)


def _box_columns(tile):
    cols = np.flatnonzero((tile > 0).any(axis=0))
    return int(cols[-1] - cols[0] + 1)


def test_column_runs_and_a_mesh_beyond_the_vertex_cache_at_64x48(tmp_path):
    """The two strip shapes and the two projection paths of the visibility kernel, each against the oracle's tile bit for bit, on the
    smallest target that reaches them.  window_pixels below the width of the object's box cuts its rows into column runs; two rows'
    worth draws strips of whole rows.  A mesh of more vertices than the LDS holds next to a window of the whole 64 x 48 target is
    projected per triangle: the launcher's own rule (scene_window_shape, roft_amd/csrc/raster_shape.h, through
    tests/cpp/raster_shape_check.cpp) says which of the two meshes it caches."""
    size = (64, 48)
    c = su.cam(*size)
    cam = su.lib_cam(c)
    exe = str(tmp_path / "raster_shape_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "roft_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "raster_shape_check.cpp"), "-o", exe])
    small, big = _box(), synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, n=43)

    def vcache_cap(mesh, wp):
        return int(subprocess.check_output([exe, str(mesh[0].shape[0]), str(size[0] * size[1]), str(wp)]))
    p = su.pose([0.01, -0.01, 0.9], [1, 2, 3], 0.7)
    for name, (v, t) in (("cached", small), ("per triangle", big)):
        want = ob.render_depth(ob.make_mesh(v, t), p[:3], p[3:], su.oracle_cam(c), 1)
        width = _box_columns(want)
        assert 12 <= width < size[0] and (want > 0).any(axis=1).sum() >= 8, "several column runs and several strips of two rows"
        whole = ops.render_scene(cam, [(v, t)], [0], p[None, None], outputs=("depth", "triangle"))
        assert su.same_bits(whole["depth"][0], want), name
        for wp in (0, width // 3, 2 * width + 1, 1):
            assert vcache_cap((v, t), wp) == (v.shape[0] if name == "cached" else 0), "the launcher caches the small mesh only"
        for wp in (width // 3, 2 * width + 1, 1):
            out = ops.render_scene(cam, [(v, t)], [0], p[None, None], outputs=("depth", "triangle"), window_pixels=wp)
            assert su.same_bits(out["depth"][0], want), (name, wp)
            assert np.array_equal(out["triangle"][0], whole["triangle"][0]), (name, wp)


def test_no_frames_each_output_alone_and_no_instances():
    box = _box()
    cam = su.lib_cam(su.cam(93, 71))
    poses = np.stack(su.POSES)[:2, None]
    rng = np.random.default_rng(4)
    bg = rng.integers(0, 256, (2, 71, 93, 3), dtype=np.uint8)
    r = ops.SceneRenderer(cam, [box], max_frames_per_call=2)
    empty = r.render([0], np.zeros((0, 1, 7)))
    assert empty["rgb"].shape == (0, 71, 93, 3) and empty["depth"].shape == (0, 71, 93)
    full = r.render([0], poses, background=bg)
    for key in OUTPUTS:
        one = r.render([0], poses, background=bg, outputs=(key,))
        assert list(one) == [key] and su.same_bits(one[key], full[key]), key
    # n_frames > max_frames_per_call is refused with its reason
    with pytest.raises(L.RoftError, match="max_frames_per_call"):
        r.render([0], np.stack(su.POSES)[:, None])
    # one background under every frame == the same image repeated
    assert same(r.render([0], poses, background=bg[:1]), r.render([0], poses, background=np.stack([bg[0], bg[0]])))
    # with no instance the output is exactly the background, grayed exactly as io.rgb_to_gray
    plain = r.render([], np.zeros((2, 0, 7)), background=bg)
    assert np.array_equal(plain["rgb"], bg) and (plain["instance"] == -1).all() and (plain["depth"] == 0).all()
    grayed = r.render([], np.zeros((2, 0, 7)), background=bg, gray_background=True)
    want = np.stack([io.rgb_to_gray(b) for b in bg])
    assert np.array_equal(grayed["rgb"], np.repeat(want[..., None], 3, axis=3))
    nothing = r.render([0], poses)
    assert (nothing["rgb"][nothing["instance"] < 0] == 0).all(), "no background given means zeros"
    # gray under an object: the reference blends over the same gray
    g = r.render([0], poses, background=bg, gray_background=True)
    ref = scene_ref.render(su.cam(93, 71), [su.zoo()["box"]], [0], poses[0], background=bg[0], gray_background=True)
    assert rgb_close(g["rgb"][0], ref["rgb"])
    r.close()


def test_styles_are_the_headers_formula():
    box, torus = su.zoo()["box"], su.zoo()["torus"]
    c = su.cam(160, 120)
    poses, bg = _busy_frames(1)
    styles = [((250, 40, 40), 0.6, 0.2), ((30, 200, 90), 1.0, 0.5), ((255, 255, 255), 0.0, 1.0)]
    out = ops.render_scene(su.lib_cam(c), [box[:2], torus[:2]], [0, 1, 0], poses, background=bg, styles=styles)
    ref = scene_ref.render(c, [box, torus], [0, 1, 0], poses[0], background=bg[0], styles=styles)
    assert rgb_close(out["rgb"][0], ref["rgb"]) and np.array_equal(out["triangle"][0], ref["triangle"])
    assert np.array_equal(out["rgb"][0][ref["instance"] == 2], bg[0][ref["instance"] == 2]), "opacity 0 leaves the background"


# ---- 5. the real path ------------------------------------------------------------------------------------------------
def test_tracked_sequence_to_overlay_files(tmp_path, capsys):
    from test_engine_gpu import make_engine
    import render_results as rr
    n = 12
    st = util.stream(702, n, 2, with_gray=True)
    root = str(tmp_path / "seq")
    mesh_path = io.write_sequence(root, st, "box")
    eng = make_engine([st])
    eng.enable_log(n)
    for k in range(n):
        depth, flow, mask, pose = util.frame_inputs(st, k)
        eng.submit([dict(depth=depth, flow=flow, mask=mask, pose=pose, dt=st.dt)])
        eng.step()
    gray = st.gray.cpu().numpy()[:n]
    bg = np.ascontiguousarray(np.repeat(gray[..., None], 3, axis=3))
    rows = eng.get_log_rows(0, n)
    pose13, twist, _, _ = eng.get_log(0, n)
    log = eng.render_log(0, n, background=bg, outputs=OUTPUTS, frames_per_call=5)
    eng.close()
    cam = L.Camera(st.camera.width, st.camera.height, st.camera.fx, st.camera.fy, st.camera.cx, st.camera.cy)
    direct = ops.render_scene(cam, [st.mesh], [0], rows[:, :, 6:13], background=bg, gray_background=True)
    assert same(log, direct), "render_log == render_scene on get_log_rows' poses"
    # the silhouette of the estimate lies on the sequence's own mask: frame and pose line up
    mask = st.mask_gt.cpu().numpy()[:n] > 0
    sil = log["instance"] >= 0
    iou = (mask & sil).sum(axis=(1, 2)) / np.maximum((mask | sil).sum(axis=(1, 2)), 1)
    assert iou.min() > 0.5, iou
    # the tool, from the files a run leaves: the mesh is read back from model.obj (%.9g: exact for float32)
    io.write_estimate_logs(str(tmp_path / "run_"), pose13[:, 0], twist[:, 0])
    argv = ["--root", root, "--mesh", mesh_path, "--poses", str(tmp_path / "run_pose_estimate"), "--out", str(tmp_path / "overlay"),
            "--ids", str(tmp_path / "ids"), "--thumbnail", str(tmp_path / "thumb.png"), "--frames-per-call", "5"]
    assert rr.main(argv) == 0
    capsys.readouterr()
    for k in range(n):
        assert np.array_equal(io.read_png(str(tmp_path / "overlay" / ("%d.png" % k))), log["rgb"][k]), k
        assert np.array_equal(io.read_png(str(tmp_path / "ids" / ("%d.png" % k))), np.where(log["instance"][k] < 0, 255, 0).astype(np.uint8)), k
    assert rr.main(argv[:6] + ["--thumbnail", str(tmp_path / "t3.png"), "--frames", "2,5,9", "--crop", "40", "30", "200", "150"]) == 0
    sheet = io.read_png(str(tmp_path / "t3.png"))
    assert sheet.shape == (2 * 120 + 10, 3 * 160 + 2 * 10, 3)
    assert np.array_equal(sheet[:120, :160], bg[2][30:150, 40:200]) and np.array_equal(sheet[130:, 340:], log["rgb"][9][30:150, 40:200])


# ---- 6. one large shape ----------------------------------------------------------------------------------------------
def test_large_shape_sixteen_instances_eight_frames():
    v, t = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS)
    v, t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)
    W, H, F, I = 1280, 720, 8, 16
    cam = L.Camera(W, H, 1229.4285612615463, 1229.4285612615463, 640.0, 360.0)
    rng = np.random.default_rng(21)
    poses = np.stack([[su.pose([-0.36 + 0.24 * (i % 4) + rng.uniform(-0.02, 0.02), -0.24 + 0.16 * (i // 4) + rng.uniform(-0.02, 0.02), rng.uniform(0.7, 1.0)],
                               rng.normal(size=3), rng.uniform(0, 3)) for i in range(I)] for _ in range(F)])
    r = ops.SceneRenderer(cam, [(v, t)], max_frames_per_call=F)
    out = r.render(np.zeros(I, np.int32), poses)
    assert len(np.unique(out["instance"][0])) == I + 1, "every instance is seen"
    for f in (0, 3, 7):
        one = r.render(np.zeros(I, np.int32), poses[f:f + 1])
        assert same({k: out[k][f:f + 1] for k in out}, one), f
    r.close()
    # (the bench mesh's vertices do not fit the LDS next to the window: this is the path that projects per triangle)
    m = ob.make_mesh(v, t)
    oc = ob.camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
    far = np.full((H, W), np.inf, np.float32)
    for i in range(I):
        d = ob.render_depth(m, poses[7, i, :3], poses[7, i, 3:], oc, 1)
        far = np.minimum(far, np.where(d > 0, d, np.float32(np.inf)))
    assert su.same_bits(out["depth"][7], np.where(np.isfinite(far), far, np.float32(0)).astype(np.float32))

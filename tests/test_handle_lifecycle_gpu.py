"""Every handle type of the library created, used, destroyed and created again in ONE process: the path on which a wrong order of
destruction or a memory block released twice shows -- the other tests build a handle, use it and let the process end.  Nothing here
is compared with a reference (the other files do that): a lifetime must leave the process as it found it, so every lifetime computes
the same bits as the one before, and as a handle created after all of them.

Shapes: the smallest geometry every part accepts, 64 x 32 (the engine wants a width that is a multiple of 32 and width * height a
multiple of 64; the flow producer at three levels a width that is a multiple of 16 and a height that is a multiple of 4), two
objects, 12 frames in batches of two -- poses on frames 0 and 6, so the silhouettes of two deliveries."""
import functools

import numpy as np
import pytest
import torch

from pose_error_util import make_engine
from roft_amd import _lib as L
from roft_amd import ops, synth

pytestmark = pytest.mark.gpu

W, H, N_OBJ, N_FRAMES, T = 64, 32, 2, 12, 2
CAM = synth.Camera(W, H, 61.47142806307731, 61.47142806307731, W / 2.0, H / 2.0)   # (shape A at a tenth, the centre on the image's)
DEPTH_SCALE = 0.001


@functools.lru_cache(maxsize=None)
def _streams():
    # (two frames more than a lifetime tracks: the batch the third lifetime leaves in flight when it closes)
    out = [synth.make_stream(2300 + i, N_FRAMES + T, CAM, with_gray=True, pose_drop_prob=0.0, mesh_n=6) for i in range(N_OBJ)]
    for st in out:
        assert [k for k in range(N_FRAMES) if st.pose_valid[k]] == [0, 6]
        assert all(int((st.mask_gt[k] > 0).sum()) >= 40 for k in range(N_FRAMES)), "the object is in the picture"
    return out


@functools.lru_cache(maxsize=None)
def _frame(k):
    """frame k for an engine with every producer on: the sensor's 16-bit depth, the camera image, no flow, no mask"""
    out = []
    for st in _streams():
        raw = np.clip(np.rint(st.depth[k].numpy() / DEPTH_SCALE), 0, 65535).astype(np.uint16)
        pose = (st.pose_meas[k, :3].copy(), st.pose_meas[k, 3:].copy()) if st.pose_valid[k] else None
        out.append(dict(depth=raw, image=np.ascontiguousarray(st.gray[k].numpy()), flow=None, mask=None, pose=pose, dt=st.dt))
    return out


def _plain_frame(k):
    """frame k for an engine without producers: HOST float depth, flow and delivered masks, staged by the engine"""
    out = []
    for st in _streams():
        mi = st.mask_delivery[k]
        pose = (st.pose_meas[k, :3].copy(), st.pose_meas[k, 3:].copy()) if st.pose_valid[k] else None
        out.append(dict(depth=st.depth[k].numpy(), flow=st.flow[k].numpy() if st.flow_valid[k] else None,
                        mask=st.mask_gt[mi].numpy() if mi >= 0 else None, pose=pose, dt=st.dt))
    return out


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


def _read_engine(eng, full):
    """everything a caller can read from an engine that has tracked N_FRAMES frames, as comparable bytes (timing: the names)"""
    out = {}
    for o in range(N_OBJ):
        out["state %d" % o] = _bits(*eng.state(o))
        out["mask %d" % o] = _bits(eng.mask(o))
        if full:
            out["flow %d" % o] = _bits(eng.produced_flow(o))
            out["depth %d" % o] = _bits(eng.depth(o))
    outs = eng.outputs()
    out["outputs"] = _bits(*[np.array(list(r.pose) + list(r.twist) + [r.n_flow_points, r.outlier_selected] + list(r.outlier_L)) for r in outs])
    out["log"] = _bits(eng.get_log_rows(0, N_FRAMES))
    out["timing"] = sorted(eng.timing())
    assert out["timing"], "timing level 2 names its launch groups"
    if full:
        out["quality"] = _bits(eng.quality(0, N_FRAMES))
        out["stats"] = (eng.flow_stats(), eng.depth_stats(), eng.pose_mask_stats(), eng.pose_mask_occlusion_stats(), eng.pose_mask_gate_stats())
        assert out["stats"][0]["pairs"] > 0 and out["stats"][1]["products"] > 0 and out["stats"][2]["silhouettes"] == 2 * N_OBJ
    npts = np.array([r.n_flow_points for r in outs])
    assert (npts > 0).all(), "the run tracks: the last frame measured flow points"
    return out


def _engine_lifetime(full, leave_in_flight=False):
    """create, enable, track, read, close.  full: every optional part that can be enabled together (none excludes another); otherwise
    the engine that is handed HOST flows and masks, whose inputs go through the staging ring.  leave_in_flight: behind the reads one
    more batch is stepped and the engine is closed without a sync, the caller's buffers outliving it."""
    eng = make_engine(_streams(), max_batch_frames=T, subsampling_radius=3.0)
    if full:
        eng.enable_flow(consistency=True)
        eng.enable_raw_depth(DEPTH_SCALE)
    eng.enable_log(N_FRAMES + T)
    if full:
        eng.enable_quality()
        eng.enable_pose_masks()
        eng.enable_pose_mask_occlusion()
        eng.enable_pose_mask_depth_gate()
    eng.enable_timing(2)
    frame = _frame if full else _plain_frame
    alive = []
    for k in range(0, N_FRAMES, T):
        eng.submit_batch([frame(k + j) for j in range(T)])
        alive.append(eng._keep)
        eng.step()
    out = _read_engine(eng, full)
    if leave_in_flight:
        eng.submit_batch([frame(N_FRAMES + j) for j in range(T)])
        alive.append(eng._keep)
        eng.step()
    eng.close()
    del alive   # (what the batches point into lived until the engine was gone)
    return out


@pytest.mark.parametrize("full", [True, False], ids=["every_part", "host_inputs"])
def test_engine_lifetimes_in_one_process_compute_the_same(full):
    a = _engine_lifetime(full)
    b = _engine_lifetime(full)
    c = _engine_lifetime(full, leave_in_flight=True)
    d = _engine_lifetime(full)
    for name, other in (("second", b), ("third", c), ("fourth, behind an engine closed with a batch in flight", d)):
        assert other.keys() == a.keys()
        for key in a:
            assert other[key] == a[key], "%s lifetime: %s differs from the first" % (name, key)


def test_flow_producer_lifetimes_in_one_process_compute_the_same():
    grays = torch.stack([_streams()[0].gray[k] for k in range(3)]).cuda().contiguous()
    prev, cur = [grays[0].data_ptr(), grays[1].data_ptr()], [grays[1].data_ptr(), grays[2].data_ptr()]

    def lifetime():
        out = torch.zeros(3, 2, H, W, 2, dtype=torch.float32, device="cuda")
        fp = ops.FlowProducer(W, H, 2, consistency=True)
        for run, check in enumerate([True, None, True]):
            if run:
                fp.set_consistency(check)
            fp.run(prev, cur, [out[run, 0].data_ptr(), out[run, 1].data_ptr()])
            fp.sync()
        fp.close()
        return out.cpu().numpy()

    first = lifetime()
    assert np.isnan(first[0]).any() and not np.isnan(first[1]).any(), "the check marks pixels, the plain product has none"
    assert _bits(first[2]) == _bits(first[0]), "the check switched off and on again"
    for again in (lifetime(), lifetime()):
        assert _bits(again) == _bits(first)


def test_scene_renderer_lifetimes_in_one_process_compute_the_same():
    cam = L.Camera(W, H, CAM.fx, CAM.fy, CAM.cx, CAM.cy)
    meshes = [st.mesh for st in _streams()]
    poses = np.array([[[-0.06, 0.0, 0.6, 1, 0, 0, 0], [0.05, 0.01, 0.7, 1, 0, 0, 0]],
                      [[-0.05, 0.0, 0.6, 1, 0, 0, 0], [0.04, 0.01, 0.7, 1, 0, 0, 0]]], np.float64)
    want = ops.render_scene(cam, meshes, [0, 1], poses)
    assert set(np.unique(want["instance"])) == {-1, 0, 1}, "both instances are in the picture"
    for _ in range(3):
        r = ops.SceneRenderer(cam, meshes, max_frames_per_call=2)
        got = [r.render([0, 1], poses[:1]), r.render([0, 1], poses[1:])]
        assert all(ms >= 0.0 for ms in r.kernel_ms())
        r.close()
        for key in ops.SCENE_OUTPUTS:
            assert _bits(got[0][key], got[1][key]) == _bits(want[key]), key


def test_one_shot_operators_repeated_in_one_process_compute_the_same():
    st = _streams()[0]
    a, b = st.gray[0].numpy(), st.gray[1].numpy()
    rgb = np.stack([a, b, a], -1)
    raw = np.clip(np.rint(st.depth[0].numpy() / DEPTH_SCALE), 0, 65535).astype(np.uint16)
    one_shots = [lambda: ops.optical_flow(a, b), lambda: ops.optical_flow(a, b, consistency=True), lambda: ops.image_to_gray(rgb),
                 lambda: ops.depth_convert(raw, DEPTH_SCALE), lambda: ops.depth_align(raw, CAM, CAM, DEPTH_SCALE, t=(0.01, 0.0, 0.0))]
    first = [_bits(f()) for f in one_shots]   # (between two calls of one operator the four others run)
    assert len(set(first)) == len(first)
    for _ in range(2):
        assert [_bits(f()) for f in one_shots] == first

"""Masks from poses without a GPU (include/roft_engine.h, section 3e): the case table keeps its aims, the ABI is what it was plus
the new entry points, what needs no device is refused before one is looked for, and the premise -- a tracker fed the silhouettes of
its delivered poses instead of network masks still tracks -- holds through the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi_header
import pose_mask_cases as pc
import util
from roft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every struct the header had before this section, with the ctypes mirror where the binding has one
OLD_STRUCTS = {"roft_camera": L.Camera, "roft_flow": L.Flow, "roft_ut_params": L.UT, "roft_mesh": L.Mesh, "roft_config": L.Config,
               "roft_object_desc": L.ObjectDesc, "roft_frame_input": L.FrameInput, "roft_label_mask": L.LabelMask,
               "roft_object_output": L.ObjectOutput, "roft_engine_stats": L.EngineStats, "roft_batch_trace": L.BatchTrace,
               "roft_of_params": L.OFParams, "roft_frame_image": L.FrameImage, "roft_engine_flow_stats": L.EngineFlowStats,
               "roft_depth_source": L.DepthSource, "roft_engine_depth_stats": L.EngineDepthStats, "roft_quality_record": L.QualityRecord,
               "roft_quality_params": L.QualityParams, "roft_scene_style": L.SceneStyle, "roft_scene_desc": L.SceneDesc}


# ---- the case table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.AIMED))
def test_case_keeps_its_aim(name):
    mesh, p, aim = pc.AIMED[name]
    assert aim(pc.expected(name) > 0, p), "the pose of case %r no longer does what the case is for" % name


def test_table_covers_every_mesh():
    used = {mesh for mesh, _ in pc.cases().values()}
    assert used == set(pc.meshes()) and len(used) == 16      # box12, the zoo's thirteen, the reference's cracker box, one over the cache
    assert pc.W // 32 == 5 and (pc.W * pc.H) % 64 == 0       # 64-pixel groups straddle rows
    counts = {name: int((pc.expected(name) > 0).sum()) for name in pc.cases()}
    assert sum(c == 0 for c in counts.values()) == 2 and sum(c == pc.W * pc.H for c in counts.values()) >= 3
    assert all(set(np.unique(pc.expected(name))) <= {0, 255} for name in pc.cases())


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_next_to_an_unchanged_abi():
    """(the calls, their rows and the new struct's fields: tests/test_abi_cpu.py, for every name of the header)"""
    assert L.ABI_VERSION == 2 and L.lib().roft_abi_version() == 2
    # every struct the header had is still declared (their sizes: the next test)
    names = {s.name for s in abi_header.structs()}
    assert set(OLD_STRUCTS) | {"roft_engine_pose_mask_stats"} <= names


def test_every_earlier_struct_has_the_size_gcc_gives_it(tmp_path):
    names = sorted(OLD_STRUCTS) + ["roft_engine_pose_mask_stats"]
    src = '#include <stdio.h>\n#include "roft_engine.h"\nint main(){' + "".join('printf("%%zu\\n", sizeof(%s));' % n for n in names) + "return 0;}"
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    mirrors = dict(OLD_STRUCTS, roft_engine_pose_mask_stats=L.EnginePoseMaskStats)
    assert got == [C.sizeof(mirrors[n]) for n in names]
    # the sizes of the parent commit (x86-64): no existing struct changed
    parent = {"roft_camera": 40, "roft_flow": 32, "roft_ut_params": 24, "roft_mesh": 32, "roft_config": 184, "roft_object_desc": 536,
              "roft_frame_input": 120, "roft_label_mask": 16, "roft_object_output": 176, "roft_engine_stats": 48, "roft_batch_trace": 80,
              "roft_of_params": 16, "roft_frame_image": 16, "roft_engine_flow_stats": 32, "roft_depth_source": 104,
              "roft_engine_depth_stats": 24, "roft_quality_record": 40, "roft_quality_params": 8, "roft_scene_style": 20, "roft_scene_desc": 64}
    assert set(parent) == set(OLD_STRUCTS)
    for n, size in parent.items():
        assert got[names.index(n)] == size, n


def test_box_mesh_arrays_are_c_contiguous():
    """A mesh's address is handed to the library as it is (L.Mesh): the arrays synth.box_mesh returns must be what it names."""
    from roft_amd import synth
    for n in (1, 12):
        v, t = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS, n)
        assert v.flags["C_CONTIGUOUS"] and t.flags["C_CONTIGUOUS"] and v.dtype == np.float32 and t.dtype == np.int32
        assert v.shape == (6 * (n + 1) ** 2, 3) and t.shape == (12 * n * n, 3)


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device():
    lib = L.lib()
    v, t = pc.meshes()["box12"]
    mesh = L.Mesh(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0])
    cam = L.Camera(*pc.CAM)
    x, q = np.array([0.0, 0.0, 0.5]), np.array([1.0, 0.0, 0.0, 0.0])
    mask = np.zeros((pc.H, pc.W), np.uint8)
    n = C.c_int(-7)

    def call(cam_=cam, mesh_=mesh, x_=x, q_=q, bands=0, vcache=1):
        return lib.roft_pose_silhouette(C.byref(cam_) if cam_ is not None else None, C.byref(mesh_) if mesh_ is not None else None,
                                        x_.ctypes.data if x_ is not None else None, q_.ctypes.data if q_ is not None else None,
                                        bands, vcache, mask.ctypes.data, C.byref(n))

    for kw in (dict(cam_=None), dict(mesh_=None), dict(x_=None), dict(q_=None), dict(bands=-1), dict(vcache=2), dict(vcache=-1)):
        assert call(**kw) == -1, kw
        assert len(lib.roft_last_error_string()) > 5
    bad = t.copy()
    bad[5, 1] = v.shape[0]
    assert call(mesh_=L.Mesh(v.ctypes.data, v.shape[0], bad.ctypes.data, bad.shape[0])) == -1
    assert call(mesh_=L.Mesh(None, v.shape[0], t.ctypes.data, t.shape[0])) == -1
    assert n.value == -7 and not mask.any(), "a refused call writes nothing"
    # a good call: its result, or the device error where there is no device -- never a quiet success without one
    rc = call()
    if lib.roft_device_count() <= 0:
        assert rc == -2 and b"no HIP device" in lib.roft_last_error_string()
    else:
        assert rc == 0
    # the engine's entry points refuse a null engine on the host
    ids = (C.c_int * 1)(0)
    st = L.EnginePoseMaskStats()
    ms = C.c_double(0.0)
    assert lib.roft_engine_enable_pose_masks(None, ids, 1) == -1
    assert lib.roft_engine_get_pose_mask_stats(None, C.byref(st)) == -1
    assert lib.roft_debug_pose_mask_kernel_ms(None, C.byref(ms)) == -1


# ---- the premise -----------------------------------------------------------------------------------------------------------
def test_tracking_with_silhouettes_of_the_delivered_poses(oracle):
    """The oracle tracker over a stream without pose outliers and drops, once with the stream's masks and once with
    ro_render_depth(pose_meas, divider 1) > 0 delivered on the pose frames: the mean position error against the ground truth with
    silhouettes is at most 1.5 x that with the stream's masks (measured: 0.0077 against 0.0085 m, 0.91 x)."""
    n = 50
    st = util.stream(1400, n, scale=4, pose_outlier_prob=0.0, pose_drop_prob=0.0)
    cam = (st.camera.width, st.camera.height, st.camera.fx, st.camera.fy, st.camera.cx, st.camera.cy)
    mesh = oracle.make_mesh(*st.mesh)

    def run(silhouettes):
        trk = oracle.Tracker(util.oracle_config(oracle, st), *st.mesh)
        err = []
        for k in range(n):
            depth, flow, mask, pose = util.frame_inputs(st, k)
            if silhouettes:
                mask = pc.silhouette(mesh, np.concatenate(pose), cam) if pose is not None else None
            r = trk.step(st.dt, depth, flow, mask, pose)
            err.append(np.linalg.norm(np.array(r.pose)[6:9] - st.gt.x[st.image(k)]))
        trk.close()
        return np.array(err)

    masks, sil = run(False), run(True)
    print("position error max / mean: stream masks %.4f / %.4f, silhouettes %.4f / %.4f" % (masks.max(), masks.mean(), sil.max(), sil.mean()))
    assert masks.mean() < 0.03, "the baseline tracks"
    assert sil.mean() <= 1.5 * masks.mean()

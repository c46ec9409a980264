"""Silhouettes gated against the depth of the pose's own frame (include/roft_engine.h, section 3e): what can be checked without a
GPU.  The gate-frame rule (roft_amd/csrc/pose_mask_gate.h) against a restatement of the reference's flow buffer and of
ro_mask_propagate's `start` (tests/cpp/pose_mask_gate_check.cpp, built against the host-only header alone); the aims of the case
tables (tests/pose_mask_gate_cases.py) and the conditions of the engine tests on the oracle's result; the ABI; and the refusals of
the operator that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_mask_gate_cases as gc
from roft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roft_amd", "csrc")


def test_gate_frame_rule_follows_the_reference_flow_buffer(tmp_path):
    exe = str(tmp_path / "pose_mask_gate_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pose_mask_gate_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) > 10000


def test_the_python_restatement_of_the_gate_frames():
    every = lambda k: k > 0
    poses = lambda k: k in gc.POSE_FRAMES
    assert gc.gate_frames(14, poses, every, 6) == {0: 0, 6: 0, 12: 6}
    assert gc.gate_frames(14, poses, every, 0) == {0: 0, 6: 0, 12: 6}            # all buffered flows: six each time
    assert gc.gate_frames(14, poses, every, 3) == {0: 0, 6: 3, 12: 9}            # only the last three
    assert gc.gate_frames(14, poses, lambda k: k not in (0, 1, 7), 6) == {0: 0, 6: 1, 12: 7}   # the chase starts behind the gap
    assert gc.gate_frames(14, poses, lambda k: k not in (0, 3, 9), 6) == {0: 0, 6: 0, 12: 6}   # a gap inside the window
    assert gc.gate_frames(14, lambda k: k in (5, 11), every, 6, start=5) == {5: 5, 11: 5}      # a track that starts on frame 5


@pytest.mark.parametrize("name", sorted(gc.operator_cases()))
def test_operator_case_serves_the_aim_of_every_depth_image(name):
    for kind in gc.DEPTHS:
        D, tb, masks, counts, removed = gc.operator_expected(name, kind)   # (asserts the aim)
        own = gc.oc.resolve(gc.rendered(name))[1].sum((1, 2))
        print(name, kind, "owned", own.tolist(), "kept", counts.tolist(), "removed", removed.tolist())
        assert (counts + removed.sum(1) == own).all()


def test_the_operator_table_shows_every_outcome():
    assert gc.operator_table_hits_every_aim_strongly() == dict(partial=True, emptied=True, behind=True, front=True)


def test_keep_predicate_in_float32():
    R = np.float32(0.5)
    lo = np.float32(R - gc.TF)
    k = lambda D, tb=0.0: bool(gc.gate(np.full((1, 1), R), np.full((1, 1), D, np.float32), gc.TF, tb)[0][0, 0])
    assert k(0.0) and k(np.nan) and k(lo) and not k(np.nextafter(lo, np.float32(0)))
    assert k(9.0) and not k(9.0, gc.TB) and k(np.float32(R + gc.TB), gc.TB) and k(np.inf) and not k(np.inf, gc.TB)


def test_conditions_of_the_engine_tests_hold_on_the_reference():
    gc.check_conditions(3)
    gc.check_conditions(4)
    # the figures the occluder was chosen with (seeds 1400 - 1402, tf = 0.02)
    sizes, removed, own_frame = [], [], []
    for i, st in enumerate(gc.streams(3)):
        for k, g in {0: 0, 6: 0, 12: 6}.items():
            R = gc.render_pose(i, np.ascontiguousarray(st.pose_meas[k], np.float64).tobytes())
            sizes.append(int((R > 0).sum()))
            removed.append(int(gc.gate(R, gc.depth(i, g))[1].sum()))
            own_frame.append(int(gc.gate(R, gc.depth(i, g, bar=False))[1].sum()))
    print("silhouettes", min(sizes), max(sizes), "removed by the bar", min(removed), max(removed), "without a bar", min(own_frame), max(own_frame))
    assert min(sizes) > 1000 and min(removed) > 300


def test_library_exports_the_symbols_and_the_structs_have_gccs_size():
    """(exports, rows, prototypes and struct layouts: tests/test_abi_cpu.py, for every name of the header)"""
    lib = L.lib()
    assert lib.roft_abi_version() == 2
    g = L.PoseMaskGate(-1.0, -1.0)
    assert lib.roft_default_pose_mask_gate(C.byref(g)) == 0 and (g.front_tolerance, g.behind_tolerance) == (np.float32(0.02), 0.0)
    assert lib.roft_default_pose_mask_gate(None) == -1


def test_operator_refusals_come_before_the_device():
    lib = L.lib()
    v, t = gc.pc.meshes()["box12"]
    n = 2
    meshes = (L.Mesh * n)(*[L.Mesh(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0]) for _ in range(n)])
    cam = L.Camera(*gc.pc.CAM)
    x = np.array([[0.0, 0.0, 0.5], [0.0, 0.0, 0.6]])
    q = np.array([[1.0, 0.0, 0.0, 0.0]] * 2)
    depth = np.zeros((gc.pc.H, gc.pc.W), np.float32)
    gate = L.PoseMaskGate(0.02, 0.0)
    masks = np.zeros((n, gc.pc.H, gc.pc.W), np.uint8)
    counts = np.full(n, -7, np.int32)
    removed = np.full((n, 2), -7, np.int32)
    ip = C.POINTER(C.c_int)

    def call(cam_=cam, meshes_=meshes, n_=n, x_=x, q_=q, depth_=depth, gate_=gate, bands=0, vcache=1):
        return lib.roft_pose_silhouettes_gated(C.byref(cam_) if cam_ is not None else None, meshes_, n_,
                                               x_.ctypes.data if x_ is not None else None, q_.ctypes.data if q_ is not None else None,
                                               depth_.ctypes.data if depth_ is not None else None, C.byref(gate_) if gate_ is not None else None,
                                               bands, vcache, masks.ctypes.data, counts.ctypes.data_as(ip), removed.ctypes.data_as(ip))

    bad_gates = [L.PoseMaskGate(0.0, 0.0), L.PoseMaskGate(-0.02, 0.0), L.PoseMaskGate(float("nan"), 0.0), L.PoseMaskGate(float("inf"), 0.0),
                 L.PoseMaskGate(0.02, float("nan")), L.PoseMaskGate(0.02, float("inf")), L.PoseMaskGate(0.02, float("-inf"))]
    for kw in [dict(cam_=None), dict(meshes_=None), dict(x_=None), dict(q_=None), dict(depth_=None), dict(gate_=None), dict(n_=0), dict(n_=-1),
               dict(n_=L.SCENE_MAX_INSTANCES + 1), dict(bands=-1), dict(vcache=2), dict(vcache=-1)] + [dict(gate_=g) for g in bad_gates]:
        assert call(**kw) == -1, kw
        assert len(lib.roft_last_error_string()) > 5
    bad = t.copy()
    bad[5, 1] = v.shape[0]
    second_bad = (L.Mesh * n)(meshes[0], L.Mesh(v.ctypes.data, v.shape[0], bad.ctypes.data, bad.shape[0]))
    assert call(meshes_=second_bad) == -1
    assert (counts == -7).all() and (removed == -7).all() and not masks.any(), "a refused call writes nothing"
    rc = call(gate_=L.PoseMaskGate(0.02, -3.0))   # (a behind tolerance <= 0 switches that test off)
    if lib.roft_device_count() <= 0:
        assert rc == -2 and b"no HIP device" in lib.roft_last_error_string()
    else:
        assert rc == 0
    # the engine's entry points refuse a null engine on the host
    st = L.EnginePoseMaskGateStats()
    assert lib.roft_engine_enable_pose_mask_depth_gate(None, C.byref(gate)) == -1
    assert lib.roft_engine_get_pose_mask_gate_stats(None, C.byref(st)) == -1

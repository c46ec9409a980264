"""Enrolled objects of one scene hide each other's silhouettes (include/roft_engine.h, section 3e): what can be checked without a
GPU.  The aims of the case table (tests/pose_mask_occlusion_cases.py) hold on the oracle's result; the numpy resolve the GPU tests
compare against is a partition of the plain silhouettes' union; the operator refuses bad arguments before it looks for a device; and
the launch plan's new fact (roft_amd/csrc/batch_plan.h) follows the rules tests/cpp/pose_mask_occlusion_plan_check.cpp states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_mask_occlusion_cases as oc
from roft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roft_amd", "csrc")


@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_case_serves_its_aim_and_resolves_to_a_partition(name):
    R = oc.rendered(name)
    raw, res = (m > 0 for m in oc.expected(name))
    print(name, "raw", raw.sum(axis=(1, 2))[:8], "resolved", res.sum(axis=(1, 2))[:8])
    assert oc.CASES[name][1](R, raw, res), "the case no longer shows what it was chosen for"
    assert res.sum(axis=0).max() <= 1, "the resolved masks of a scene are disjoint"
    assert np.array_equal(res.any(axis=0), raw.any(axis=0)), "their union is the union of the plain silhouettes"
    assert not (res & ~raw).any()
    assert oc._lost_only_to_nearer(R, raw, res)


def test_the_figures_the_cases_were_chosen_with():
    """the first four cases, as counted when they were written (box12, the camera of pose_mask_cases)"""
    counts = {name: [m.sum(axis=(1, 2)).tolist() for m in ((x > 0) for x in oc.expected(name))] for name in ("front_back", "crossing", "tie", "hidden")}
    assert counts["front_back"] == [[5660, 2469], [5660, 462]]
    raw, res = (m > 0 for m in oc.expected("crossing"))
    both = raw[0] & raw[1]
    assert counts["crossing"][0] == [4494, 4494] and both.sum() == 4124 and (res[0] & both).sum() == 2062 and (res[1] & both).sum() == 2062
    assert counts["tie"] == [[4437, 4437], [4437, 0]]
    assert counts["hidden"] == [[7421, 164], [7421, 0]]


def test_resolve_keeps_the_lower_id_on_a_tie_and_ignores_empty_pixels():
    R = np.zeros((3, 1, 4), np.float32)
    R[0, 0] = [0.5, 0.0, 0.7, 0.0]
    R[1, 0] = [0.5, 0.6, 0.6, 0.0]
    R[2, 0] = [0.4, 0.6, 0.0, 0.0]
    raw, res = oc.resolve(R)
    assert res[:, 0].tolist() == [[False, False, False, False], [False, True, True, False], [True, False, False, False]]


def test_operator_refusals_come_before_the_device():
    lib = L.lib()
    v, t = oc.meshes()["box12"]
    n = 2
    meshes = (L.Mesh * n)(*[L.Mesh(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0]) for _ in range(n)])
    cam = L.Camera(*oc.CAM)
    x = np.array([[0.0, 0.0, 0.5], [0.0, 0.0, 0.6]])
    q = np.array([[1.0, 0.0, 0.0, 0.0]] * 2)
    masks = np.zeros((n, oc.H, oc.W), np.uint8)
    counts = np.full(n, -7, np.int32)

    def call(cam_=cam, meshes_=meshes, n_=n, x_=x, q_=q, bands=0, vcache=1):
        return lib.roft_pose_silhouettes_occluded(C.byref(cam_) if cam_ is not None else None, meshes_, n_,
                                                  x_.ctypes.data if x_ is not None else None, q_.ctypes.data if q_ is not None else None,
                                                  bands, vcache, masks.ctypes.data, counts.ctypes.data_as(C.POINTER(C.c_int)))

    for kw in (dict(cam_=None), dict(meshes_=None), dict(x_=None), dict(q_=None), dict(n_=0), dict(n_=-1), dict(n_=L.SCENE_MAX_INSTANCES + 1),
               dict(bands=-1), dict(vcache=2), dict(vcache=-1)):
        assert call(**kw) == -1, kw
        assert len(lib.roft_last_error_string()) > 5
    bad = t.copy()
    bad[5, 1] = v.shape[0]
    second_bad = (L.Mesh * n)(meshes[0], L.Mesh(v.ctypes.data, v.shape[0], bad.ctypes.data, bad.shape[0]))
    assert call(meshes_=second_bad) == -1
    assert (counts == -7).all() and not masks.any(), "a refused call writes nothing"
    rc = call()
    if lib.roft_device_count() <= 0:
        assert rc == -2 and b"no HIP device" in lib.roft_last_error_string()
    else:
        assert rc == 0
    # the engine's entry points refuse a null engine on the host
    ids = (C.c_int * 1)(0)
    st = L.EnginePoseMaskOcclusionStats()
    assert lib.roft_engine_enable_pose_mask_occlusion(None, ids, ids, 1) == -1
    assert lib.roft_engine_get_pose_mask_occlusion_stats(None, C.byref(st)) == -1


def test_resolve_launch_only_with_pairs_to_resolve_and_last_of_the_preparation(tmp_path):
    exe = str(tmp_path / "pose_mask_occlusion_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pose_mask_occlusion_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) > 100000

"""Pose hypotheses without a GPU (include/roft_engine.h, section 3j): the refusals made before a device is looked for, the pose
arithmetic of roft_amd/relocalise.py against hand-written values, and the compass search over the exact CPU reference
(tests/quality_ref.py on the oracle's render) -- whose traces are tests/golden/relocalise_traces.json, the file the GPU tests
reproduce."""
import ctypes as C
import math

import numpy as np
import pytest

import mesh_zoo
import relocalise_cases as rc
from roft_amd import _lib as L
from roft_amd import ops, relocalise

INVALID, NO_DEVICE = -1, -2   # ROFT_ERR_INVALID, ROFT_ERR_DEVICE


def operator_args(n=2):
    cam = L.Camera(64, 64, 57.6, 57.6, 31.5, 31.5)
    depth = np.ones((64, 64), np.float32)
    mask = np.full((64, 64), 255, np.uint8)
    v, t = mesh_zoo.box()
    mesh = ops.make_mesh(v, t)
    poses = np.tile(np.array([0.0, 0.0, 0.5, 1.0, 0.0, 0.0, 0.0]), (max(n, 1), 1))
    out = (L.QualityRecord * max(n, 1))()
    keep = (depth, mask, v, t, poses)
    return dict(cam=C.byref(cam), divider=2, depth=depth.ctypes.data, mask=mask.ctypes.data, mesh=C.byref(mesh), poses=poses.ctypes.data, n=n,
                tol=0.01, dmax=2.0, window=0, out=out), (cam, mesh, keep)


def call(a):
    return L.lib().roft_pose_hypotheses_score(a["cam"], a["divider"], a["depth"], a["mask"], a["mesh"], a["poses"], a["n"], a["tol"], a["dmax"],
                                              a["window"], a["out"])


@pytest.mark.parametrize("field, value, words", [
    ("cam", None, "null argument"), ("depth", None, "null argument"), ("mask", None, "null argument"), ("mesh", None, "null argument"),
    ("poses", None, "null argument"), ("out", None, "null argument"),
    ("n", -1, "n must be in"), ("n", (1 << 20) + 1, "n must be in"),
    ("divider", 0, "divider must be > 0"), ("divider", -2, "divider must be > 0"),
    ("tol", -0.001, "depth_tolerance must be >= 0"), ("tol", float("nan"), "depth_tolerance must be >= 0"),
    ("window", -1, "window_pixels must be >= 0"),
])
def test_operator_refusals_before_a_device_is_looked_for(field, value, words):
    a, keep = operator_args()
    a[field] = value
    assert call(a) == INVALID
    assert words in L.lib().roft_last_error_string().decode()


def test_operator_refuses_what_check_mesh_refuses():
    lib = L.lib()
    v, t = mesh_zoo.box()
    a, keep = operator_args()
    bad_index = t.copy()
    bad_index[5, 1] = len(v)                                  # a corner that is no vertex
    for mesh in (ops.make_mesh(v, bad_index), L.Mesh(None, len(v), t.ctypes.data, len(t)), L.Mesh(v.ctypes.data, len(v), None, len(t))):
        a["mesh"] = C.byref(mesh)
        assert call(a) == INVALID and b"mesh" in lib.roft_last_error_string()
    assert lib.roft_track_quality(a["cam"], 2, a["depth"], a["mask"], a["mesh"], a["poses"], a["poses"] + 24, 0.01, 2.0, 0, a["out"]) == INVALID   # the sibling refuses it too


def test_n_zero_is_ok_and_touches_nothing():
    a, keep = operator_args(n=0)
    before = bytes(a["out"])
    assert call(a) == 0
    a["poses"] = a["out"] = a["cam"] = a["depth"] = a["mask"] = a["mesh"] = None   # nothing is read either
    assert call(a) == 0
    assert bytes(operator_args(n=0)[0]["out"]) == before
    cam, mesh, (depth, mask, v, t, poses) = keep
    assert ops.pose_hypotheses_score(cam, 2, depth, mask, mesh, np.zeros((0, 7))).shape == (0,)
    a, keep = operator_args(n=0)
    a["divider"] = 0                                          # ... but a bad argument is still one
    assert call(a) == INVALID


def test_a_well_formed_call_without_a_device_is_a_device_error():
    if L.lib().roft_device_count() > 0:
        return                                                # (with a device: tests/test_pose_hypotheses_gpu.py)
    a, keep = operator_args()
    assert call(a) == NO_DEVICE and b"no HIP device" in L.lib().roft_last_error_string()


def test_engine_entry_refuses_without_an_engine():
    out = (L.QualityRecord * 1)()
    poses = np.zeros(7)
    assert L.lib().roft_engine_score_hypotheses(None, 0, poses.ctypes.data, 1, 0.01, out) == INVALID
    assert b"null engine" in L.lib().roft_last_error_string()


def test_ops_raises_the_refusals():
    a, (cam, mesh, (depth, mask, v, t, poses)) = operator_args()
    for kw in (dict(divider=0), dict(depth_tolerance=-1.0), dict(depth_tolerance=float("nan")), dict(window_pixels=-1)):
        args = dict(divider=2, depth_tolerance=0.01, window_pixels=0)
        args.update(kw)
        with pytest.raises(L.RoftError, match="error -1"):
            ops.pose_hypotheses_score(cam, args["divider"], depth, mask, mesh, poses, args["depth_tolerance"], 2.0, args["window_pixels"])
    with pytest.raises(ValueError):
        ops.pose_hypotheses_score(cam, 2, depth, mask, mesh, np.zeros(6))


# ---- roft_amd/relocalise.py ----------------------------------------------------------------------------------------------------------
def test_disagreement_by_hand():
    rec = dict(n_mask=100, n_render=90, n_both=70, n_depth=60, n_front=5, n_behind=7, depth_err=0.0)
    assert relocalise.disagreement(rec) == 100 + 90 - 140 + 5 + 7 and isinstance(relocalise.disagreement(rec), int)
    arr = np.zeros(2, ops.QUALITY_DTYPE)
    arr[0] = (0, 100, 90, 70, 60, 5, 7, 0, 0.0)
    arr[1] = (0, 2 ** 30, 2 ** 30, 0, 0, 0, 0, 0, 0.0)       # no int32 overflow
    d = relocalise.disagreement(arr)
    assert d.tolist() == [62, 2 ** 31] and relocalise.disagreement(arr[0]) == 62


def test_compass_candidates_by_hand():
    x = np.array([0.1, -0.2, 0.5])
    t, r = 0.008, math.radians(4.0)
    c, s = math.cos(r / 2), math.sin(r / 2)
    cand = relocalise.compass_candidates(x, [1.0, 0.0, 0.0, 0.0], t, r)
    assert cand.shape == (13, 7)
    want_x = [[0.1, -0.2, 0.5], [0.1 + t, -0.2, 0.5], [0.1 - t, -0.2, 0.5], [0.1, -0.2 + t, 0.5], [0.1, -0.2 - t, 0.5], [0.1, -0.2, 0.5 + t],
              [0.1, -0.2, 0.5 - t]] + [[0.1, -0.2, 0.5]] * 6
    assert cand[:, :3].tolist() == want_x
    want_q = [[1.0, 0.0, 0.0, 0.0]] * 7 + [[c, s, 0, 0], [c, -s, 0, 0], [c, 0, s, 0], [c, 0, -s, 0], [c, 0, 0, s], [c, 0, 0, -s]]
    assert np.abs(cand[:, 3:] - np.array(want_q)).max() <= 1e-16
    # dq (x) q, not q (x) dq: a quarter turn about the camera's x applied to a quarter turn about z
    h = math.sqrt(0.5)
    cand = relocalise.compass_candidates(x, [h, 0.0, 0.0, h], t, math.pi / 2)
    assert np.abs(cand[7, 3:] - np.array([0.5, 0.5, -0.5, 0.5])).max() <= 1e-15      # (h, h, 0, 0) (x) (h, 0, 0, h)
    assert np.abs(cand[8, 3:] - np.array([0.5, -0.5, 0.5, 0.5])).max() <= 1e-15      # (h, -h, 0, 0) (x) (h, 0, 0, h)
    assert np.abs(cand[11, 3:] - np.array([0.0, 0.0, 0.0, 1.0])).max() <= 1e-15      # (h, 0, 0, h) (x) (h, 0, 0, h)
    # unit norm kept over a long chain of turns
    q = rc.CASES["rotated_9deg"][1]
    for i in range(200):
        q = relocalise.compass_candidates(x, q, t, r)[7 + i % 6, 3:]
        assert abs(math.sqrt(float(q @ q)) - 1.0) <= 1e-15


def test_compass_search_halves_and_stops():
    """a scorer with its minimum at a known translation: the search walks there, halves max_halvings + 1 times and stops"""
    target = np.array([0.016, 0.0, -0.008])
    calls = []

    def score(poses):
        calls.append(len(poses))
        rec = np.zeros(len(poses), ops.QUALITY_DTYPE)
        rec["n_mask"] = np.rint(np.abs(poses[:, :3] - target).sum(axis=1) * 1000).astype(np.int32)
        return rec

    x, q, trace = relocalise.compass_search(score, np.zeros(3), [1.0, 0.0, 0.0, 0.0], t_step=0.008, r_step=0.1, max_halvings=2)
    assert [w for w, _ in trace] == [1, 1, 6, 0, 0, 0] and [d for _, d in trace] == [16, 8, 0, 0, 0, 0]
    assert x.tolist() == [0.016, 0.0, -0.008] and q.tolist() == [1.0, 0.0, 0.0, 0.0] and calls == [13] * 6
    _, _, trace = relocalise.compass_search(score, np.zeros(3), [1.0, 0.0, 0.0, 0.0], t_step=0.001, r_step=0.1, rounds=5)
    assert len(trace) == 5 and all(w == 1 for w, _ in trace)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_compass_search_over_the_exact_reference(oracle, name):
    """the two start poses of the issue: the trace's disagreement never increases, the mean vertex distance to the true pose at least
    halves (the exact reference reaches 1/36 and 1/10), and the run is the committed one"""
    mask, depth = rc.scene(oracle, name)
    _, ocam = rc.cameras(oracle)
    mesh = mesh_zoo.box()
    x0, q0 = rc.start_pose(name)
    x, q, trace = relocalise.compass_search(rc.cpu_scorer(oracle, ocam, rc.D, depth, mask > 1, mesh), x0, q0)
    dis = [d for _, d in trace]
    assert all(b <= a for a, b in zip(dis, dis[1:])) and len(trace) <= 40
    xt, qt = rc.CASES[name][:2]
    before, after = rc.mean_vertex_distance(mesh[0], x0, q0, xt, qt), rc.mean_vertex_distance(mesh[0], x, q, xt, qt)
    print(name, "mean vertex distance: start %.2f mm, end %.2f mm, %d rounds" % (before * 1e3, after * 1e3, len(trace)))
    assert before > 0.02 and after <= 0.5 * before
    gold = rc.golden()[name]
    assert [list(t) for t in trace] == gold["trace"]
    assert [float.hex(float(v)) for v in x] == gold["x"] and [float.hex(float(v)) for v in q] == gold["q"]

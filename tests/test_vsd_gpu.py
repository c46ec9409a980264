"""VSD on the device (roft_pose_errors_vsd; include/roft_engine.h section 3i) against the restatement tests/vsd_ref.py over the
oracle's renders.  Counts must be equal exactly, and errors to the last bit: both sides divide the same integers.  The cases
(tests/vsd_cases.py) keep every decision away from its threshold -- tests/test_vsd_cpu.py checks that by the oracle alone -- so a
last-bit difference could neither hide nor fake a failure."""
import itertools
import json
import os
import sys

import numpy as np
import pytest

from roft_amd import io, metrics, ops

import scene_util
import symmetry_ref
import vsd_cases as VC
import vsd_ref
from oracle import binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = list(VC.ESTIMATES)
BASE = list(itertools.product(VC.MESHES, VC.SIZES))


def same(got, want):
    """(errors, counts) pairs, rows or whole calls: the errors' bits and the counts"""
    return np.array_equal(vsd_ref.bits(got[0]), vsd_ref.bits(want[0])) and np.array_equal(np.asarray(got[1]), np.asarray(want[1]))


def want_rows(name, keys, size):
    refs = [VC.reference(name, k, size) for k in keys]
    return np.array([r[0] for r in refs]), np.array([r[1] for r in refs])


def restated(name, est_key, size, depth=None, taus=VC.TAUS, diameter=None, est_pose=None, ref_pose=None):
    """the restatement for anything but a base case"""
    cam = scene_util.cam(*size)
    De = VC.render(name, est_key, size) if est_pose is None else vsd_ref.render(ob, VC.mesh(name), est_pose, cam)
    Dg = VC.render(name, "reference", size) if ref_pose is None else vsd_ref.render(ob, VC.mesh(name), ref_pose, cam)
    depth = VC.sensor_depth(name, size) if depth is None else depth
    return vsd_ref.vsd(De, Dg, depth, cam, VC.DELTA, taus, VC.diameter(name) if diameter is None else diameter)


@pytest.mark.parametrize("name,size", BASE)
def test_base_cases_against_the_restatement(name, size):
    got = VC.device(name, KEYS, size)
    want = want_rows(name, KEYS, size)
    for f, key in enumerate(KEYS):
        print("%s %s %s: counts %s" % (name, size, key, got[1][f]))
    assert got[1].dtype == np.int32 and got[0].shape == (4, 10) and got[1].shape == (4, 14)
    assert same(got, want), (got, want)


@pytest.mark.parametrize("name,size", BASE)
def test_an_estimate_with_vertices_behind_the_near_plane(name, size):
    got = VC.device(name, ["close"], size)
    want = restated(name, "close", size)
    if name == "box":   # (the torus is a ring around this camera: next to nothing of it is drawn)
        assert want[1][3] > want[1][2], "the estimate fills the screen"
    assert same((got[0][0], got[1][0]), want), (got, want)


@pytest.mark.parametrize("size", VC.SIZES)
def test_strips_change_no_bit(size):
    keys = KEYS + ["close"]
    whole = VC.device("torus", keys, size)
    assert same((whole[0][:4], whole[1][:4]), want_rows("torus", KEYS, size))
    assert same((whole[0][4], whole[1][4]), restated("torus", "close", size))
    for window_pixels in (size[0], 257, 1):   # one row's worth; a strip boundary inside the object; one row per strip whatever its width
        assert same(VC.device("torus", keys, size, window_pixels=window_pixels), whole), window_pixels


def test_a_mesh_larger_than_the_vertex_cache():
    size = VC.SIZES[1]
    assert len(VC.mesh("big_box")[0]) == VC.CACHE_VERTS + 3
    got = VC.device("big_box", ["near", "far", "close"], size)
    for f, key in enumerate(("near", "far", "close")):
        want = restated("big_box", key, size)
        assert want[1][1] > 0 and same((got[0][f], got[1][f]), want), (key, got[1][f], want[1])
    assert same(VC.device("big_box", ["near", "far", "close"], size, window_pixels=257), got)


def test_one_image_under_every_pair():
    name, size = "box", VC.SIZES[1]
    one = VC.device(name, KEYS, size)
    repeated = VC.device(name, KEYS, size, depth=np.repeat(VC.sensor_depth(name, size)[None], len(KEYS), axis=0))
    assert same(one, repeated) and same(one, VC.device(name, KEYS, size, depth=VC.sensor_depth(name, size)[None]))


def test_a_row_depends_on_its_own_pair_alone():
    """70 pairs with an image each (more than one chunk of 64): the probe pair alone, first, in the middle and last; two runs"""
    name, size = "torus", VC.SIZES[1]
    n = 70
    cam, mesh = scene_util.lib_cam(scene_util.cam(*size)), VC.lib_mesh(name)
    base = VC.sensor_depth(name, size)
    probe_depth = np.roll(base, 3, axis=1)
    want = restated(name, "near", size, depth=probe_depth)
    for at in (0, 35, 63, 64, n - 1):
        keys = [KEYS[f % 4] for f in range(n)]
        keys[at] = "near"
        est = np.array([VC.pose_of(k) for k in keys])
        ref = np.tile(VC.REFERENCE, (n, 1))
        depth = np.repeat(base[None], n, axis=0)
        depth[at] = probe_depth
        runs = [ops.pose_errors_vsd(cam, mesh, est, ref, depth, delta=VC.DELTA, taus=VC.TAUS, diameter=VC.diameter(name), counts=True) for _ in range(2)]
        assert same(runs[0], runs[1]), "equal inputs, equal bits"
        assert same((runs[0][0][at], runs[0][1][at]), want), at
        others = [f for f in range(n) if f != at]
        assert same((runs[0][0][others], runs[0][1][others]), want_rows(name, [keys[f] for f in others], size)), at
    alone = ops.pose_errors_vsd(cam, mesh, VC.ESTIMATES["near"][None], VC.REFERENCE[None], probe_depth, delta=VC.DELTA, taus=VC.TAUS,
                                diameter=VC.diameter(name), counts=True)
    assert same((alone[0][0], alone[1][0]), want)


def test_a_non_finite_pose_draws_nothing_and_changes_no_other_row():
    name, size = "box", VC.SIZES[1]
    cam, mesh = scene_util.lib_cam(scene_util.cam(*size)), VC.lib_mesh(name)
    clean = want_rows(name, KEYS, size)
    for bad, col in ((np.nan, 1), (np.inf, 5), (-np.inf, 2)):
        est = np.array([VC.pose_of(k) for k in KEYS])
        ref = np.tile(VC.REFERENCE, (4, 1))
        est[1, col] = bad
        got = ops.pose_errors_vsd(cam, mesh, est, ref, VC.sensor_depth(name, size), delta=VC.DELTA, taus=VC.TAUS, diameter=VC.diameter(name), counts=True)
        want = restated(name, None, size, est_pose=est[1])
        assert want[1][3] == 0 and np.all(want[0] == 1.0) and want[1][0] == want[1][2] > 0, "only the reference is seen"
        assert same((got[0][1], got[1][1]), want), (bad, got[1][1], want[1])
        assert same((got[0][[0, 2, 3]], got[1][[0, 2, 3]]), (clean[0][[0, 2, 3]], clean[1][[0, 2, 3]])), bad
        # ... and a reference that draws nothing: the estimate where the image lets it be seen, no intersection
        ref[2, col] = bad
        got = ops.pose_errors_vsd(cam, mesh, est, ref, VC.sensor_depth(name, size), delta=VC.DELTA, taus=VC.TAUS, diameter=VC.diameter(name), counts=True)
        want = restated(name, "same", size, ref_pose=ref[2])
        assert want[1][1] == 0 and want[1][2] == 0 and np.all(want[0] == 1.0)
        assert same((got[0][2], got[1][2]), want), (bad, got[1][2], want[1])
        assert same((got[0][[0, 3]], got[1][[0, 3]]), (clean[0][[0, 3]], clean[1][[0, 3]])), bad
    both = np.full((1, 7), np.nan)
    got = ops.pose_errors_vsd(cam, mesh, both, both, VC.sensor_depth(name, size), delta=VC.DELTA, taus=VC.TAUS, counts=True)
    assert np.all(got[0] == 1.0) and not np.any(got[1]), "nothing drawn: n_union == 0"


@pytest.mark.parametrize("kind", ["zeros", "wall", "mixed"])
def test_depth_images_without_measurements(kind):
    name, size = "box", VC.SIZES[1]
    depth = VC.strange_depths(name, size)[kind]
    got = VC.device(name, ["near", "far", "off"], size, depth=depth)
    for f, key in enumerate(("near", "far", "off")):
        want = restated(name, key, size, depth=depth)
        print(kind, key, want[1])
        assert same((got[0][f], got[1][f]), want), (kind, key, got[1][f], want[1])
    if kind == "zeros":   # every pixel a hole: both renders are visible wherever they draw
        assert got[1][0][2] == np.count_nonzero(VC.render(name, "reference", size)) and got[1][0][3] == np.count_nonzero(VC.render(name, "near", size))


def test_one_tau_sixteen_taus_and_taus_in_metres():
    name, size = "torus", VC.SIZES[0]
    for taus in (np.array([0.2]), np.arange(1, 17) * 0.031):
        got = VC.device(name, ["near", "far"], size, taus=taus)
        assert got[0].shape == (2, len(taus)) and got[1].shape == (2, 4 + len(taus))
        for f, key in enumerate(("near", "far")):
            assert same((got[0][f], got[1][f]), restated(name, key, size, taus=taus)), (len(taus), key)
    metres = VC.TAUS * 0.05
    for diameter in (None, 0.0):
        got = VC.device(name, ["near", "far"], size, taus=metres, diameter=diameter)
        for f, key in enumerate(("near", "far")):
            want = restated(name, key, size, taus=metres, diameter=0.0)
            assert len(set(want[0].tolist())) >= 3 and same((got[0][f], got[1][f]), want), key


def test_without_counts():
    name, size = "box", VC.SIZES[0]
    errors = ops.pose_errors_vsd(scene_util.lib_cam(scene_util.cam(*size)), VC.lib_mesh(name), np.array([VC.pose_of(k) for k in KEYS]),
                                 np.tile(VC.REFERENCE, (4, 1)), VC.sensor_depth(name, size), delta=VC.DELTA, taus=VC.TAUS, diameter=VC.diameter(name))
    assert isinstance(errors, np.ndarray) and np.array_equal(vsd_ref.bits(errors), vsd_ref.bits(want_rows(name, KEYS, size)[0]))
    assert ops.pose_errors_vsd(scene_util.lib_cam(scene_util.cam(*size)), VC.lib_mesh(name), np.zeros((0, 7)), np.zeros((0, 7)),
                               VC.sensor_depth(name, size)).shape == (0, 10)


def axis_angle_rows(poses):
    return np.array([np.concatenate([p[:3], *[np.atleast_1d(v) for v in io.quat_to_axis_angle(p[3:])]]) for p in poses])


def test_evaluate_results_ar_on_a_synthetic_results_tree(tmp_path, capsys):
    """tools/evaluate_results.py --ar on two objects, three frames each, 160 x 120: its columns are bop_average_recall over the
    restatements' numbers (VSD: vsd_ref over oracle renders; MSSD / MSPD: symmetry_ref)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_results
    size = VC.SIZES[0]
    W, H = size
    cam = scene_util.cam(*size)
    dataset, results = str(tmp_path / "dataset"), str(tmp_path / "results")
    frames = ("near", "far", "same")
    want, pooled = {}, dict(vsd=[], mssd=[], mspd=[])
    for name in VC.MESHES:
        for d in (os.path.join(dataset, name, "depth"), os.path.join(dataset, name, "gt"), os.path.join(results, name)):
            os.makedirs(d)
        io.write_cam_k(os.path.join(dataset, name, "cam_K.json"), cam)
        io.write_obj(os.path.join(dataset, name, "model.obj"), *VC.mesh(name))
        depths = [np.roll(VC.sensor_depth(name, size), k, axis=0) for k in range(len(frames))]
        for k, d in enumerate(depths):
            io.write_depth(os.path.join(dataset, name, "depth", "%d.float" % k), d)
        np.savetxt(os.path.join(dataset, name, "gt", "poses.txt"), axis_angle_rows([VC.REFERENCE] * len(frames)), fmt="%.17g")
        np.savetxt(os.path.join(results, name, "pose_estimate.txt"),
                   np.concatenate([np.zeros((len(frames), 6)), axis_angle_rows([VC.ESTIMATES[k] for k in frames])], axis=1), fmt="%.17g")
        # what the tool will see: the files' numbers
        verts, tris = io.load_obj(os.path.join(dataset, name, "model.obj"))
        est = metrics.Metric._poses(io.read_log(os.path.join(results, name, "pose_estimate.txt"), skip_cols=6))
        ref = metrics.Metric._poses(np.loadtxt(os.path.join(dataset, name, "gt", "poses.txt"), ndmin=2))
        diameter = metrics.model_diameter(verts)
        mesh = (np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32))
        vsd = np.array([vsd_ref.vsd(vsd_ref.render(ob, mesh, est[k], cam), vsd_ref.render(ob, mesh, ref[k], cam), depths[k], cam, 0.015,
                                    np.arange(0.05, 0.51, 0.05), diameter)[0] for k in range(len(frames))])
        pts = verts.astype(np.float64)
        identity = np.array([symmetry_ref.IDENTITY])
        mssd = symmetry_ref.pose_errors_sym("mssd", pts, est, ref, identity)
        mspd = symmetry_ref.pose_errors_sym("mspd", pts, est, ref, identity, (cam.fx, cam.fy, cam.cx, cam.cy))
        want[name] = metrics.bop_average_recall(vsd, mssd, mspd, diameter, W)
        assert 0.0 < want[name]["AR_VSD"] < 1.0 and 0.0 < want[name]["AR"] < 1.0, want[name]
        pooled["vsd"].append(vsd.reshape(-1))
        pooled["mssd"].append(mssd / diameter)
        pooled["mspd"].append(mspd * (640.0 / W))
    want["ALL"] = metrics.bop_average_recall(*(np.concatenate(pooled[k]) for k in ("vsd", "mssd", "mspd")), 1.0, 640)
    out = str(tmp_path / "table.json")
    assert evaluate_results.main(["--results", results, "--dataset", dataset, "--metrics", "rmse_cartesian_3d", "--all-points", "--ar", "--json", out]) == 0
    table = json.load(open(out))
    text = capsys.readouterr().out
    for key in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert key + " (recall)" in text
        assert table[key] == {n: want[n][key] for n in list(VC.MESHES) + ["ALL"]}, (key, table[key], want)
    assert evaluate_results.main(["--results", results, "--dataset", dataset, "--metrics", "rmse_cartesian_3d", "--vsd", "--json", out]) == 0
    table_vsd = json.load(open(out))
    assert table_vsd["AR_VSD"] == table["AR_VSD"] and "AR" not in table_vsd and "AR_MSSD" not in table_vsd
    capsys.readouterr()
    assert evaluate_results.main(["--results", results, "--dataset", dataset, "--metrics", "rmse_cartesian_3d"]) == 0
    assert "AR" not in capsys.readouterr().out

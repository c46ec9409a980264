"""The VSD score without a device (include/roft_engine.h, section 3i): every refusal of roft_pose_errors_vsd is made on the host, the
defaults are BOP19's, the numpy form in roft_amd/metrics.py equals the restatement tests/vsd_ref.py bit for bit, BOP's recalls on
a table computed by hand -- and the shared cases of the GPU test (tests/vsd_cases.py) discriminate by the oracle alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import metrics, ops

import scene_util
import vsd_cases as VC
import vsd_ref

BASE = list(itertools.product(VC.MESHES, VC.SIZES))


def call(cam=None, mesh=None, est=None, ref=None, n_poses=2, depth=None, n_depth=None, params=None, errors=None, counts=None, null=()):
    """roft_pose_errors_vsd on a well-formed call, with the named arguments replaced; null: the pointers handed over as NULL"""
    W, H = 64, 48
    cam = L.Camera(W, H, 60.0, 60.0, 32.0, 24.0) if cam is None else cam
    mesh = VC.lib_mesh("box") if mesh is None else mesh
    n = max(n_poses, 1)
    est = np.tile(VC.REFERENCE, (n, 1)) if est is None else est
    ref = np.tile(VC.REFERENCE, (n, 1)) if ref is None else ref
    n_depth = n_poses if n_depth is None else n_depth
    depth = np.zeros((max(n_depth, 1), H, W), np.float32) if depth is None else depth
    params = ops.vsd_params() if params is None else params
    errors = np.full((n, L.VSD_MAX_TAUS), -7.0) if errors is None else errors
    args = dict(cam=C.byref(cam), mesh=C.byref(mesh), est=est.ctypes.data, ref=ref.ctypes.data, depth=depth.ctypes.data, params=C.byref(params),
                errors=errors.ctypes.data, counts=None if counts is None else counts.ctypes.data)
    for name in null:
        args[name] = None
    rc = L.lib().roft_pose_errors_vsd(args["cam"], args["mesh"], args["est"], args["ref"], n_poses, args["depth"], n_depth, args["params"],
                                      args["errors"], args["counts"])
    return rc, errors


def no_device():
    return L.lib().roft_device_count() <= 0


def test_default_params_are_bop19s():
    p = L.VsdParams()
    p.n_taus, p.diameter, p.window_pixels = 99, 5.0, 7
    assert L.lib().roft_default_vsd_params(C.byref(p)) == L.OK
    assert p.delta == np.float32(0.015) and p.n_taus == 10 and p.diameter == 0.0 and p.window_pixels == 0
    assert list(p.taus)[:10] == [k / 20.0 for k in range(1, 11)], "each the double nearest to k * 0.05"
    assert list(p.taus)[10:] == [0.0] * 6
    assert L.lib().roft_default_vsd_params(None) == L.ERR_INVALID
    assert L.VSD_MAX_TAUS == 16


@pytest.mark.parametrize("name", ["cam", "mesh", "est", "ref", "depth", "params", "errors"])
def test_a_null_pointer_is_refused(name):
    rc, _ = call(null=(name,))
    assert rc == L.ERR_INVALID and b"null" in L.lib().roft_last_error_string()


def test_counts_may_be_null_and_an_empty_call_touches_nothing():
    errors = np.full((1, L.VSD_MAX_TAUS), -7.0)
    counts = np.full((1, 4 + L.VSD_MAX_TAUS), -7, np.int32)
    rc, _ = call(n_poses=0, n_depth=5, errors=errors, counts=counts)   # (n_depth is not looked at without pairs)
    assert rc == L.OK and np.all(errors == -7.0) and np.all(counts == -7)
    rc, _ = call(n_poses=0, n_depth=0)
    assert rc == L.OK


def test_a_well_formed_call_needs_a_device():
    for n_depth in (2, 1):
        rc, errors = call(n_depth=n_depth)
        if no_device():
            assert rc == L.ERR_DEVICE and np.all(errors == -7.0), "there is no CPU path"
        else:
            assert rc == L.OK and np.all(errors.reshape(-1)[:20] != -7.0)   # (two rows of ten, packed)
    if no_device():
        with pytest.raises(L.RoftError):
            VC.device("box", ["near"], VC.SIZES[0])


def refused(**kw):
    rc, errors = call(**kw)
    return rc == L.ERR_INVALID and len(L.lib().roft_last_error_string()) > 0 and np.all(errors == -7.0)


def test_counts_of_poses_and_images():
    assert refused(n_poses=-1, n_depth=1)
    assert refused(n_poses=3, n_depth=2)
    assert refused(n_poses=3, n_depth=0)
    assert refused(n_poses=3, n_depth=4)
    assert refused(n_poses=2, n_depth=-1)


def params(**kw):
    p = ops.vsd_params()
    for k, v in kw.items():
        if k == "tau":
            p.taus[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


def test_parameters():
    for n_taus in (0, -1, 17):
        assert refused(params=params(n_taus=n_taus)), n_taus
    for bad in (0.0, -0.05, np.nan, np.inf, -np.inf):
        assert refused(params=params(tau=(0, bad))), bad
        assert refused(params=params(tau=(9, bad))), bad
    p = params(tau=(10, np.nan))   # (beyond n_taus: not read)
    assert call(params=p)[0] != L.ERR_INVALID
    for bad in (-1e-6, np.nan, np.inf):
        assert refused(params=params(delta=bad)), bad
        assert refused(params=params(diameter=bad)), bad
    assert refused(params=params(window_pixels=-1))
    assert call(params=params(delta=0.0, diameter=0.0, window_pixels=1))[0] != L.ERR_INVALID


def test_meshes_the_other_operators_refuse():
    v, t = VC.mesh("box")
    assert refused(mesh=L.Mesh(v.ctypes.data, 0, t.ctypes.data, len(t)))
    assert refused(mesh=L.Mesh(v.ctypes.data, len(v), t.ctypes.data, 0))
    assert refused(mesh=L.Mesh(None, len(v), t.ctypes.data, len(t)))
    assert refused(mesh=L.Mesh(v.ctypes.data, len(v), None, len(t)))
    bad = t.copy()
    bad[5, 1] = len(v)
    assert refused(mesh=L.Mesh(v.ctypes.data, len(v), bad.ctypes.data, len(bad)))
    assert b"triangle 5" in L.lib().roft_last_error_string()
    bad[5, 1] = -1
    assert refused(mesh=L.Mesh(v.ctypes.data, len(v), bad.ctypes.data, len(bad)))


def test_image_sizes_the_scene_renderer_refuses():
    one = np.zeros((1, 1, 1), np.float32)
    for w, h in ((0, 48), (64, 0), (-64, 48), (4096, 4096), (1 << 24, 1)):
        assert refused(cam=L.Camera(w, h, 60.0, 60.0, 32.0, 24.0), depth=one, n_depth=1), (w, h)
    # what the scene renderer accepts but no on-chip window holds a row of: refused as well, not launched
    assert refused(cam=L.Camera(30000, 2, 60.0, 60.0, 32.0, 24.0), depth=one, n_depth=1)
    assert b"row" in L.lib().roft_last_error_string()


@pytest.mark.parametrize("name,size", BASE)
def test_numpy_form_equals_the_restatement(name, size):
    cam = scene_util.cam(*size)
    for key in VC.ESTIMATES:
        want_e, want_c, _ = VC.reference(name, key, size)
        for diameter in (VC.diameter(name), None):
            got_e, got_c = metrics.vsd_from_depths(VC.render(name, key, size), VC.render(name, "reference", size), VC.sensor_depth(name, size),
                                                   (cam.fx, cam.fy, cam.cx, cam.cy), VC.DELTA, VC.TAUS, diameter, counts=True)
            if diameter is None:
                want_e, want_c = vsd_ref.vsd(VC.render(name, key, size), VC.render(name, "reference", size), VC.sensor_depth(name, size), cam,
                                             VC.DELTA, VC.TAUS, 0.0)
            assert np.array_equal(vsd_ref.bits(got_e), vsd_ref.bits(want_e)) and np.array_equal(got_c, want_c), (key, diameter)
            assert got_c.dtype == np.int32 and got_e.dtype == np.float64
    plain = metrics.vsd_from_depths(VC.render(name, "near", size), VC.render(name, "reference", size), VC.sensor_depth(name, size),
                                    (cam.fx, cam.fy, cam.cx, cam.cy), diameter=VC.diameter(name))
    assert np.array_equal(vsd_ref.bits(plain), vsd_ref.bits(VC.reference(name, "near", size)[0])), "the defaults are BOP19's"


def test_numpy_form_on_depths_that_are_no_measurement():
    name, size = "box", VC.SIZES[1]
    cam = scene_util.cam(*size)
    for depth in VC.strange_depths(name, size).values():
        want = vsd_ref.vsd(VC.render(name, "far", size), VC.render(name, "reference", size), depth, cam, VC.DELTA, VC.TAUS, VC.diameter(name))
        got = metrics.vsd_from_depths(VC.render(name, "far", size), VC.render(name, "reference", size), depth, (cam.fx, cam.fy, cam.cx, cam.cy),
                                      VC.DELTA, VC.TAUS, VC.diameter(name), counts=True)
        assert np.array_equal(vsd_ref.bits(got[0]), vsd_ref.bits(want[0])) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("name,size", BASE)
def test_the_cases_discriminate_by_the_oracle_alone(name, size):
    drawn = int(np.count_nonzero(VC.render(name, "reference", size)))
    for key in ("near", "far"):
        errors, counts, margins = VC.reference(name, key, size)
        n_union, n_inter, n_gt, n_est = (int(v) for v in counts[:4])
        print("%s %s %s: union %d inter %d gt %d of %d drawn, est %d; errors %s; margins delta %.3g m, tau %.3g"
              % (name, size, key, n_union, n_inter, n_gt, drawn, n_est, np.round(errors, 4), margins["delta"], margins["tau"]))
        assert 0 < n_inter < n_union
        assert n_gt < drawn, "part of the reference is hidden"
        assert len(set(errors.tolist())) >= 3
        assert margins["delta"] >= 1e-7 and margins["tau"] >= 1e-9, "no decision near a threshold (move the pose, not the bar)"
    errors, counts, margins = VC.reference(name, "same", size)
    assert np.all(errors == 0.0) and counts[0] == counts[1] > 0 and margins["delta"] >= 1e-7
    errors, counts, margins = VC.reference(name, "off", size)
    assert np.all(errors == 1.0) and counts[3] == 0 and counts[0] == counts[2] > 0 and margins["delta"] >= 1e-7
    assert not np.any(VC.render(name, "off", size)), "off screen"


def test_model_diameter():
    for name in VC.MESHES:
        v = VC.mesh(name)[0]
        assert metrics.model_diameter(v) == VC.diameter(name)
        assert metrics.model_diameter(v, chunk=7) == VC.diameter(name)
    assert metrics.model_diameter([[0, 0, 0], [3, 4, 0], [1, 1, 1]]) == 5.0
    assert metrics.model_diameter([[1, 2, 3]]) == 0.0


def test_recalls_on_a_table_computed_by_hand():
    assert metrics.bop_recall([0.1, 0.2, 0.3, 0.4], [0.25, 0.35]) == (2 / 4 + 3 / 4) / 2
    assert metrics.bop_recall([0.25], [0.25]) == 0.0, "correct means strictly below"
    assert metrics.bop_recall([], [0.25]) == 0.0
    assert metrics.bop_recall([np.inf, np.nan, 0.0], [1.0]) == 1 / 3
    # two estimates, two taus.  VSD errors below theta = 0.05 k: (0.0 -> 10, 0.12 -> 8, 0.33 -> 4, 1.0 -> 0) of 10 thetas
    vsd = np.array([[0.0, 0.12], [0.33, 1.0]])
    ar_vsd = (10 + 8 + 4 + 0) / (4 * 10)
    # diameter 0.2 m: MSSD thresholds 0.01 k m.  0.025 m -> k >= 3: 8 thetas; 0.2 m -> none
    mssd = np.array([0.025, 0.2])
    ar_mssd = (8 + 0) / (2 * 10)
    # width 320: MSPD thresholds 2.5 k px.  2.4 px -> 10; 13 px -> k >= 6: 5
    mspd = np.array([2.4, 13.0])
    ar_mspd = (10 + 5) / (2 * 10)
    got = metrics.bop_average_recall(vsd, mssd, mspd, 0.2, 320)
    assert got == {"AR_VSD": ar_vsd, "AR_MSSD": ar_mssd, "AR_MSPD": ar_mspd, "AR": (ar_vsd + ar_mssd + ar_mspd) / 3.0}, got
    assert np.array_equal(metrics.BOP_VSD_TAUS, np.arange(0.05, 0.51, 0.05)) and len(metrics.BOP_MSPD_THRESHOLDS) == 10

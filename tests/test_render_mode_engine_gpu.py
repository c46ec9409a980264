"""The batched engine with roft_config::render_mode = ROFT_RENDER_GL against the oracle tracker, whose every outlier test also
scores its alternatives on RO_RENDER_GL renders (Tracker.shadow_render): the engine's likelihoods are the oracle's shadow GL
likelihoods, its decisions theirs.  On these workloads no decision differs between the two render modes (checked on the
CPU with the oracle alone, tools/render_gap.py's method), so the trajectories are the oracle's within test_engine_gpu.py's bars.
The GL-mode output does not depend on the launch shape."""
import copy

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import synth

import util
from test_render_gl_gpu import spike_mesh

pytestmark = pytest.mark.gpu

POS_TOL = 1e-6    # m         (tests/test_engine_gpu.py)
ROT_TOL = 1e-6    # rad
TWIST_TOL = 1e-6  # m/s, rad/s
# the alternatives' poses differ from the oracle's by ~1e-11 (test_engine_gpu.py::LIK_ENGINE_RTOL); the kernel itself is bit
# exact on identical poses (test_render_gl_gpu.py)
LIK_ENGINE_RTOL = 1e-9
N_FRAMES = 14


def _streams(which):
    if which == "cfg3":    # config #3 shape: 1280 x 720, CV_16SC2, two objects
        return [util.stream(3100 + o, N_FRAMES, scale=1, shape="B", flow_type=synth.FLOW_S16C2) for o in range(2)]
    if which == "cfg4":    # config #4 shape: 640 x 480, CV_32FC2, eight objects
        return [util.stream(4100 + o, N_FRAMES, scale=1, shape="A") for o in range(8)]
    st = copy.copy(util.stream(4200, N_FRAMES, scale=1, shape="A"))   # one object with the self-intersecting mesh
    st.mesh = spike_mesh(half=(0.08, 0.1, 0.035), n=8, tip=0.15)
    return [st]


def _oracle_run(streams):
    from oracle import binding as ob
    out = []
    for st in streams:
        trk = ob.Tracker(util.oracle_config(ob, st), *st.mesh)
        trk.shadow_render(True)
        rows = []
        for k in range(N_FRAMES):
            depth, flow, mask, pose = util.frame_inputs(st, k)
            r = trk.step(st.dt, depth, flow, mask, pose)
            sh = trk.shadow_L() if r.outlier_selected >= 0 else None
            rows.append(dict(pose=np.array(r.pose), twist=np.array(r.twist), sel=r.outlier_selected, L=np.array(r.outlier_L),
                             L_gl=None if sh is None else sh[1].copy()))
        trk.close()
        out.append(rows)
    return out


@pytest.fixture(scope="module", params=["cfg3", "cfg4", "spike"])
def workload(request):
    streams = _streams(request.param)
    return request.param, streams, _oracle_run(streams)


def _make_engine(streams, **over):
    st0 = streams[0]
    cfg = E.default_config(st0.camera.width, st0.camera.height, st0.flow_type, max_objects=len(streams), render_mode=L.RENDER_GL)
    c = st0.camera
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = c.fx, c.fy, c.cx, c.cy
    cfg.flow_grid, cfg.flow_scale = st0.flow_grid, st0.flow_scale
    for k, v in over.items():
        setattr(cfg, k, v)
    eng = E.ROFTFilterBatch(cfg)
    for st in streams:
        d = E.default_object()
        m0 = synth.initial_pose_from_stream(st)
        for i in range(13):
            d.p_mean0[i] = m0[i]
        eng.add_object(d, *st.mesh)
    return eng


def _run_engine(streams, **over):
    eng = _make_engine(streams, **over)
    rows = []
    for k in range(N_FRAMES):
        eng.submit([util.device_frame(st, k) for st in streams])
        eng.step()
        rows.append([(np.array(o.pose), np.array(o.twist), o.outlier_selected, np.array(o.outlier_L), o.n_flow_points) for o in eng.outputs()])
    eng.close()
    return rows


def test_engine_gl_mode_matches_the_oracle_shadow_gl(workload):
    name, streams, ref = workload
    dev = [util.to_device(st) for st in streams]
    rows = _run_engine(dev)
    n_tests = 0
    for k in range(N_FRAMES):
        for o, r in enumerate(ref):
            pose, twist, sel, Lv, _ = rows[k][o]
            exp = r[k]
            assert sel == exp["sel"], (name, k, o, list(Lv), exp["L"], exp["L_gl"])
            if exp["sel"] >= 0:
                n_tests += 1
                L_gl = exp["L_gl"]
                np.testing.assert_allclose(Lv, L_gl, rtol=LIK_ENGINE_RTOL, err_msg="%s frame %d obj %d" % (name, k, o))
                # the decision on the GL likelihoods is the oracle's own (no decision moves on these workloads)
                assert sel == (1 if L_gl[0] > 2.0 * L_gl[1] else 0) == exp["sel"]
            np.testing.assert_allclose(pose[:9], exp["pose"][:9], rtol=0, atol=POS_TOL, err_msg="%s frame %d obj %d" % (name, k, o))
            assert 2.0 * np.arccos(min(1.0, abs(float(np.dot(pose[9:], exp["pose"][9:]))))) < ROT_TOL, (name, k, o)
            np.testing.assert_allclose(twist, exp["twist"], rtol=0, atol=TWIST_TOL)
    assert n_tests >= 2 * len(streams)


def test_engine_gl_mode_samples_match_the_oracle(workload):
    """Sample counts of every test: the engine's likelihood is a mean over exactly the oracle's samples -- checked through the
    operator-level test on the engine's own alternatives would need them; here: a test without samples in the oracle has none in
    the engine (DBL_MAX), and the likelihoods agree to LIK_ENGINE_RTOL (a different sample set would move them by far more)."""
    name, streams, ref = workload
    rows = _run_engine([util.to_device(st) for st in streams])
    big = np.finfo(np.float64).max
    for k in range(N_FRAMES):
        for o, r in enumerate(ref):
            if r[k]["sel"] >= 0:
                Lv = rows[k][o][3]
                for a in range(2):
                    assert (Lv[a] == big) == (r[k]["L_gl"][a] >= 1e300), (name, k, o, a)


def test_engine_gl_mode_identical_across_launch_shapes(workload):
    name, streams, _ = workload
    dev = [util.to_device(st) for st in streams]
    base = _run_engine(dev, outlier_bands_per_alternative=1)

    def same(rows):
        for k in range(N_FRAMES):
            for o in range(len(streams)):
                a, b = rows[k][o], base[k][o]
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]), (name, k, o)

    same(_run_engine(dev, outlier_bands_per_alternative=2))
    same(_run_engine(dev, outlier_bands_per_alternative=0))
    L.check(L.lib().roft_debug_outlier_split(0))
    try:
        same(_run_engine(dev, outlier_bands_per_alternative=0))
    finally:
        L.lib().roft_debug_outlier_split(-1)
    # batches of 8 frames: the device-side log of the same run
    log8, _, _ = util.run_engine_logged(lambda s, **kw: _make_engine(s, outlier_bands_per_alternative=1, **kw), dev, N_FRAMES, T=8)
    pose8, twist8, _, sel8 = log8
    for k in range(N_FRAMES):
        for o in range(len(streams)):
            assert np.array_equal(pose8[k, o], base[k][o][0]) and np.array_equal(twist8[k, o], base[k][o][1]) and sel8[k, o] == base[k][o][2], (name, k, o)


def test_engine_refuses_an_unknown_render_mode():
    st = util.stream(4100, 2, scale=2)
    cfg = E.default_config(st.camera.width, st.camera.height, st.flow_type, max_objects=1)
    cfg.render_mode = 2
    with pytest.raises(L.RoftError):
        E.ROFTFilterBatch(cfg)
    cfg.render_mode = -1
    with pytest.raises(L.RoftError):
        E.ROFTFilterBatch(cfg)

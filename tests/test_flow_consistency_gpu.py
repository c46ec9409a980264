"""The forward-backward check on the device (include/roft_engine.h section 3f; of_check_kernel in k_opticalflow.hip).  Everything
is compared bit for bit, as uint32 views (an invalid pixel is a NaN, which equals nothing):
  - the operator against flow_consistency_ref.check over the CPU oracle's flows of both directions,
  - the batched producer against the operator, across the boundary of a chunk of kOfChunk / 2 pairs,
  - an engine fed images, with the check on, against the same engine fed HOST buffers of the operator's checked flows.

Shapes: the fixtures are 64 x 96 (2 x 8 Lucas-Kanade tiles at level 0, 24 blocks of the check kernel); the engine runs are
util.stream(seed, n, scale=2, with_gray=True), 320 x 240."""
import numpy as np
import pytest
import torch

from roft_amd import _lib as L
from roft_amd import ops

import flow_consistency_cases as cases
import flow_consistency_ref as ref
import util
from oracle import binding as ob
from pose_error_util import make_engine
from test_engine_flow_gpu import _first_frame, _full_log, _gray, _stream, always, run, same

pytestmark = pytest.mark.gpu

F32, S16 = L.FLOW_F32C2, L.FLOW_S16C2
ON = dict(consistency=True)
_oracle = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pair(name):
    return cases.rolled() if name == "rolled" else getattr(cases, name)(1)


def _oracle_flows(name, levels, radius, iterations):
    key = (name, levels, radius, iterations)
    if key not in _oracle:
        a, b = _pair(name)
        _oracle[key] = (ob.optical_flow(a, b, levels, radius, iterations, 100.0), ob.optical_flow(b, a, levels, radius, iterations, 100.0))
    return _oracle[key]


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "occluded", "rolled"])
@pytest.mark.parametrize("levels,radius,iterations", [(3, 3, 3), (2, 1, 5)])
def test_operator_equals_the_reference(name, levels, radius, iterations):
    a, b = _pair(name)
    F, B = _oracle_flows(name, levels, radius, iterations)
    for tol in (True, (0.0, 0.0), (1e30, 0.0)):
        want = ref.check(F, B) if tol is True else ref.check(F, B, *tol)
        got = ops.optical_flow(a, b, levels=levels, radius=radius, iterations=iterations, det_min=100.0, consistency=tol)
        assert np.array_equal(bits(got), bits(want)), (tol, int((bits(got) != bits(want)).any(axis=2).sum()))
    inv = ref.invalid(want)                     # (1e30, 0): the `inside` rule alone
    assert (inv.any() or name != "rolled") and not inv.all()


def test_operator_generic_radius():
    a, b = _pair("occluded")
    F, B = _oracle_flows("occluded", 3, 5, 2)
    want = ref.check(F, B)
    got = ops.optical_flow(a, b, levels=3, radius=5, iterations=2, det_min=100.0, consistency=True)
    assert np.array_equal(bits(got), bits(want))
    assert ref.invalid(want).any() and not ref.invalid(want).all()


def test_operator_without_the_check_is_unchanged():
    a, b = _pair("occluded")
    F, _ = _oracle_flows("occluded", 3, 3, 3)
    assert np.array_equal(bits(ops.optical_flow(a, b)), bits(F))
    assert np.array_equal(bits(ops.optical_flow(a, b, consistency=None)), bits(F))


# ---- 2. the batched producer -------------------------------------------------------------------------------------------------
def test_batched_producer_equals_single_calls():
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (64, 96), dtype=np.uint8)]
    for _ in range(5):
        imgs.append(np.roll(imgs[-1], (1, 2), (0, 1)))
    n, (H, W) = 5, imgs[0].shape
    g = torch.from_numpy(np.stack(imgs)).cuda()
    outs = [torch.zeros((n, H, W, 2), dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    fp = ops.FlowProducer(W, H, n, consistency=True)      # five pairs: a full chunk of four and a chunk of one
    ptrs = lambda t: [t[k].data_ptr() for k in range(n)]
    for out in outs[:2]:                                  # ... twice on the same workspaces
        fp.run(ptrs(g), ptrs(g[1:]), ptrs(out))
        fp.sync()
    fp.set_consistency(None)
    fp.run(ptrs(g), ptrs(g[1:]), ptrs(outs[2]))
    fp.sync()
    fp.close()
    first, second, off = (o.cpu().numpy() for o in outs)
    assert np.array_equal(bits(first), bits(second))
    some_invalid = 0
    for k in range(n):
        single = ops.optical_flow(imgs[k], imgs[k + 1], consistency=True)
        assert np.array_equal(bits(single), bits(first[k])), k
        assert np.array_equal(bits(ops.optical_flow(imgs[k], imgs[k + 1])), bits(off[k])), k
        some_invalid += int(ref.invalid(single).sum())
    assert some_invalid > 0 and not np.isnan(off).any()


def test_s16_producer_refuses():
    with pytest.raises(L.RoftError, match="error -1.*CV_16SC2"):
        ops.FlowProducer(96, 64, 2, S16, consistency=True)
    fp = ops.FlowProducer(96, 64, 2, F32)
    for tol in ((np.nan, 0.0), (0.5, -1.0), (np.inf, 0.0)):
        with pytest.raises(L.RoftError, match="error -1.*tolerance"):
            fp.set_consistency(tol)
    fp.close()


# ---- 3. the engine -----------------------------------------------------------------------------------------------------------
N = 12


def _npts(r, obj=0):
    return [row[obj][2] for row in r["log"]]


def test_engine_single_frames():
    st = _stream(2100, N, F32)
    ref_run = run([(st, always("img"))], N, F32, as_flows=True, of=ON)
    got = run([(st, always("img"))], N, F32, of=ON, flows_at=(1, N - 1))
    same(got, ref_run)
    for k in (1, N - 1):
        want = ops.optical_flow(_gray(st, k - 1), _gray(st, k), consistency=True)
        assert np.array_equal(bits(got["flows"][(k, 0)]), bits(want)), k
        assert ref.invalid(want).any()
    # the check is seen by the filter: some frame draws another number of flow samples than without it
    off = run([(st, always("img"))], N, F32)
    assert _npts(got) != _npts(off)
    assert sum(1 for v in _npts(got)[1:] if v > 0) >= N - 3
    assert got["fstats"] == off["fstats"] == dict(images=N, image_bytes=N * 320 * 240, pyramids=N, pairs=N - 1)


def test_engine_one_batch_of_eight():
    st = _stream(2101, 8, F32)
    objs = [(st, always("img"))]
    got = run(objs, 8, F32, splits=[8], of=ON, dev=True)      # seven pairs: a chunk of four and one of three
    same(got, run(objs, 8, F32, splits=[8], as_flows=True, of=ON, dev=True))
    same(got, run(objs, 8, F32, of=ON))
    assert got["fstats"]["pairs"] == 7


def test_engine_shared_scene_and_own_stream():
    F = 10
    a, b = _stream(2102, F, F32), _stream(2103, F, F32)
    objs = [(a, always("img"))] * 2 + [(b, always("img"))]
    got = run(objs, F, F32, splits=[4], of=ON)
    same(got, run(objs, F, F32, splits=[4], as_flows=True, of=ON))
    off = run(objs, F, F32, splits=[4])
    assert got["fstats"] == off["fstats"] and got["fstats"]["pairs"] == 2 * (F - 1)     # flows, not Lucas-Kanade problems
    assert _npts(got, 0) != _npts(off, 0) or _npts(got, 2) != _npts(off, 2)


def test_engine_explicit_tolerances_reach_the_kernel():
    st = _stream(2100, N, F32)
    of = dict(levels=2, radius=1, iterations=5, consistency=(0.25, 0.0))
    got = run([(st, always("img"))], 3, F32, of=of, flows_at=(2,))
    want = ops.optical_flow(_gray(st, 1), _gray(st, 2), **of)
    assert np.array_equal(bits(got["flows"][(2, 0)]), bits(want))
    assert not np.array_equal(bits(want), bits(ops.optical_flow(_gray(st, 1), _gray(st, 2), levels=2, radius=1, iterations=5, consistency=True)))


# ---- 4. a gap ----------------------------------------------------------------------------------------------------------------
def test_gap_starts_over():
    F, gap = 10, 4
    a, b = _stream(2102, F, F32), _stream(2103, F, F32)
    duo = lambda k: "none" if k == gap else "img"
    objs = [(a, duo)] * 2 + [(b, always("img"))]
    got = run(objs, F, F32, splits=[4], of=ON)
    same(got, run(objs, F, F32, splits=[4], as_flows=True, of=ON))
    for f in (gap, gap + 1):
        assert all(got["log"][f][o][2] <= 0 for o in range(2)), "no flow, no flow points"
    assert got["log"][gap + 2][0][2] > 0
    assert got["fstats"]["pairs"] == 2 * (F - 1) - 2


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def _feed_images(eng, st, n):
    eng.enable_log(n)
    for k in range(n):
        depth, _, mask, pose = util.frame_inputs(st, k)
        eng.submit([dict(depth=depth, mask=mask, pose=pose, dt=st.dt, image=_gray(st, k))])
        eng.step()
    return _full_log(eng, n)


def test_refusals():
    n = 5
    st = _stream(2100, N, F32)
    plain = make_engine([st])
    plain.enable_flow()
    want = _feed_images(plain, st, n)
    with pytest.raises(L.RoftError, match="error -4.*first frame"):
        plain.enable_flow_consistency(True)             # after the first frame
    plain.close()

    eng = make_engine([st])
    with pytest.raises(L.RoftError, match="error -4.*roft_engine_enable_flow"):
        eng.enable_flow_consistency(True)               # before enable_flow
    eng.enable_flow()
    for tol in ((np.nan, 0.01), (0.5, np.nan), (-1.0, 0.01), (0.5, -0.01), (np.inf, 0.01), (0.5, np.inf)):
        with pytest.raises(L.RoftError, match="error -1.*tolerance"):
            eng.enable_flow_consistency(tol)
    assert _feed_images(eng, st, n) == want             # every call was refused: the engine of before
    eng.close()

    s16 = _stream(2100, N, S16)
    eng = make_engine([s16])
    eng.enable_flow()
    with pytest.raises(L.RoftError, match="error -1.*CV_16SC2"):
        eng.enable_flow_consistency(True)
    with pytest.raises(L.RoftError, match="error -1.*CV_16SC2"):
        eng.enable_flow(consistency=True)
    eng.submit([_first_frame(s16, image=_gray(s16, 0))])     # ... and it still takes images
    eng.step()
    eng.sync()
    assert eng.flow_stats()["images"] == 1
    eng.close()


# ---- 6. tracking -------------------------------------------------------------------------------------------------------------
def test_tracker_fed_by_the_checked_flow():
    """test_opticalflow_gpu.test_tracker_fed_by_the_produced_flow with the check on, inside that test's own bounds."""
    from test_engine_gpu import make_engine as make
    st = util.stream(75, 48, 1, with_gray=True, device="cuda")
    gray = st.gray.cpu().numpy()
    H, W = gray.shape[1:]
    g = torch.from_numpy(gray).cuda()
    n = st.n_frames
    flow = torch.zeros((n, H, W, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fp = ops.FlowProducer(W, H, n - 1, consistency=True)
    fp.run([g[k - 1].data_ptr() for k in range(1, n)], [g[k].data_ptr() for k in range(1, n)], [flow[k].data_ptr() for k in range(1, n)])
    fp.sync()
    fp.close()
    assert bool(torch.isnan(flow[1:]).any()) and not bool(torch.isnan(flow[1:]).all())
    errs = {}
    for name, fl in (("analytic", st.flow.cuda()), ("checked", flow)):
        eng = make([st])
        depth, masks = st.depth.cuda(), st.mask_gt.cuda()
        torch.cuda.synchronize()
        for k in range(n):
            mi = st.mask_delivery[k]
            pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
            eng.submit([dict(depth=depth[k].data_ptr(), flow=fl[k].data_ptr() if st.flow_valid[k] else None,
                             mask=masks[mi].data_ptr() if mi >= 0 else None, pose=pose, dt=st.dt, mem_kind=L.MEM_DEVICE)])
            eng.step()
        eng.sync()
        pose, _, _, _ = eng.state(0)
        errs[name] = float(np.linalg.norm(pose[6:9] - st.gt.x[n - 1]))
        eng.close()
    print("final position error (m):", errs)
    assert errs["checked"] < 0.02, errs
    assert errs["checked"] < errs["analytic"] + 0.01, errs

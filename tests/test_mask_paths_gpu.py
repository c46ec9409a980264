"""The mask chain (roft_amd/csrc/k_mask.hip) on every walk, window and flow format, bit for bit against tests/mask_ref.py.

The cases are mask_ref.cases(): far targets (direct ORs into the destination plane, overlapping margins), poison flows (NaN, inf,
1e10, 3e9, -0.0, S16 extremes, steps to (-1, 0) and to W), the (0,0) corner (fill with ones, clear00, a background of 1), dense
planes (two rounds of walk_single_aligned; one workgroup walking two chunks), formats off the beaten path (MODE 1 combinations,
MODE 0's true divisions), three-valued masks in a running engine across batch cuts, the schedule decisions (decide_mode /
next_fbuf), and a 1024 x 1280 plane whose one window is capped by the LDS.  tests/test_mask_ref_cpu.py shows without a GPU that the
reference equals the C oracle, that each case reaches its branch and that each defect a walk could have moves a case.

Every comparison is np.array_equal over the whole image: no tolerance, no pixel left out.
"""
import ctypes as C

import numpy as np
import pytest
import torch   # (before the library is loaded: the two share one HIP runtime, torch's when it comes first)

from roft_amd import _lib as L
from roft_amd import engine as E

import mask_ref as R

pytestmark = pytest.mark.gpu

ENGINE_CASES = [n for n, c in R.cases().items() if c.engine]
REFUSED_CASES = [n for n, c in R.cases().items() if not c.engine]
DT = 1.0 / 30.0


def _same(got, want, what):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        pytest.fail("%s: %d pixels differ, (row, col) %s ... %s; got %s, expected %s there" % (
            what, len(d), tuple(d[0]), tuple(d[-1]), got[tuple(d[0])], want[tuple(d[0])]))


def _engine(c, T):
    cfg = E.default_config(c.W, c.H, L.FLOW_S16C2 if c.fmt.kind == "s16" else L.FLOW_F32C2, max_objects=c.n_obj, max_batch_frames=T)
    cfg.cam.fx = cfg.cam.fy = 1.5 * c.W
    cfg.cam.cx, cfg.cam.cy = c.W / 2, c.H / 2
    cfg.flow_grid, cfg.flow_scale = c.fmt.grid, c.fmt.scale
    for k, v in c.over.items():
        setattr(cfg, k, v)
    eng = E.ROFTFilterBatch(cfg)
    for _ in range(c.n_obj):
        d = E.default_object()
        d.p_mean0[6:9] = R.POSE0[0]
        d.p_mean0[9:13] = R.POSE0[1]
        eng.add_object(d, *R.small_mesh())
    return eng


def _inputs(name, device):
    """frames[k][o]: the engine's input dicts.  The rest of the engine is kept idle: all-zero depth, a pose on frame 0 only."""
    c = R.cases()[name]
    keep = []
    if device:
        def put(a):
            t = torch.from_numpy(np.array(a)).cuda()
            keep.append(t)
            return t.data_ptr()
    else:
        put = lambda a: a
    depth = put(np.zeros((c.H, c.W), np.float32))
    out = []
    for k, row in enumerate(R.frames(name)):
        out.append([dict(depth=depth, flow=None if f is None else put(f.data), mask=None if m is None else put(m),
                         pose=R.POSE0 if k == 0 else None, dt=DT, mem_kind=L.MEM_DEVICE if device else L.MEM_HOST) for m, f in row])
    return out, keep


def _run(name, splits=None, device=False):
    """The case through the engine, frame by frame (splits None) or in batches of the given sizes, repeated.  Returns
    [(k, [mask of every object after frame k])] for the last frame of every step."""
    c = R.cases()[name]
    frames, keep = _inputs(name, device)
    eng = _engine(c, max(splits) if splits else 1)
    out = []
    try:
        k = i = 0
        while k < len(frames):
            t = min(splits[i % len(splits)], len(frames) - k) if splits else 1
            i += 1
            if splits:
                eng.submit_batch(frames[k:k + t])
            else:
                eng.submit(frames[k])
            eng.step()
            k += t
            out.append((k - 1, [eng.mask(o) for o in range(c.n_obj)]))
    finally:
        eng.close()
    del keep
    return out


def _check(name, got, what):
    want = R.expected(name)
    for k, masks in got:
        for o, m in enumerate(masks):
            _same(m, want[k][o], "%s %s frame %d object %d" % (name, what, k, o))
    # the objects are told apart: their masks differ in the reference, so a mix-up of object indices cannot pass
    assert len(got[-1][1]) < 2 or not np.array_equal(want[-1][0], want[-1][1])


# ---------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENGINE_CASES)
def test_engine_frame_by_frame(name):
    got = _run(name)
    assert len(got) == len(R.frames(name))
    _check(name, got, "T = 1")


@pytest.mark.parametrize("name,splits", [(n, s) for n in ENGINE_CASES for s in R.cases()[n].splits])
def test_engine_batched(name, splits):
    _check(name, _run(name, splits), "batches %s" % (splits,))


@pytest.mark.parametrize("name,splits", [("far_64x128_s16_g4_s32", (4, 8, 2)), ("three_valued_64x128_f32_g1_s1", (5, 2, 7)),
                                         ("poison_96x64_f32_g1_s1", (3, 8))])
def test_engine_batched_device_inputs(name, splits):
    _check(name, _run(name, splits, device=True), "DEVICE batches %s" % (splits,))


@pytest.mark.parametrize("name", REFUSED_CASES)
def test_engine_refuses_a_stream_that_starts_without_a_mask(name):
    """The schedule "no mask for the first frames" exists for the reference and the oracle (test_mask_ref_cpu.py); the engine's
    contract is that an object's first frame brings its mask: a state error, nothing stepped."""
    c = R.cases()[name]
    frames, _ = _inputs(name, False)
    assert frames[0][0]["mask"] is None
    eng = _engine(c, 1)
    try:
        with pytest.raises(L.RoftError):
            eng.submit(frames[0])
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["far_96x64_f32_g1_s1", "three_valued_96x64_s16_g4_s32"])
def test_masks_do_not_depend_on_the_order_of_the_atomics(name):
    """The OR into window and plane, and the atomicMax / atomicExch map of the three-valued path: two runs, identical masks."""
    a, b = _run(name, (4, 8, 2)), _run(name, (4, 8, 2))
    for (k, ma), (_, mb) in zip(a, b):
        for o in range(len(ma)):
            _same(ma[o], mb[o], "%s second run, frame %d object %d" % (name, k, o))
    _check(name, a, "first run")


# ---------------------------------------------------------------------------------------------
# operator: roft_mask_propagate with hand-built flow descriptors (any grid and scale)
# ---------------------------------------------------------------------------------------------
def _op_propagate(mask, flows, frames_between):
    out = np.array(mask, np.uint8)
    H, W = out.shape
    arr = (L.Flow * max(1, len(flows)))()
    for i, f in enumerate(flows):
        rows, cols = f.data.shape[:2]
        arr[i] = L.Flow(f.data.ctypes.data, L.FLOW_S16C2 if f.data.dtype == np.int16 else L.FLOW_F32C2, cols, rows, f.grid, f.scale, 1)
    L.check(L.lib().roft_mask_propagate(out.ctypes.data_as(C.c_void_p), W, H, arr, len(flows), frames_between))
    return out


@pytest.mark.parametrize("name", [n for n, c in R.cases().items() if c.family in ("formats", "poison", "corner")])
def test_operator_against_reference(name):
    """Every mask the case delivers (three-valued ones and those with (0,0) set included), through the first 1, 3 and 6 flows
    of its object -- unthresholded, as the operator returns {0, 1, 255} -- and through the last 2 of 6."""
    c = R.cases()[name]
    fr = R.frames(name)
    n_checked = 0
    for o in range(c.n_obj):
        flows = [row[o][1] for row in fr[1:] if row[o][1] is not None]
        for m in (row[o][0] for row in fr if row[o][0] is not None):
            for n, fb in ((1, 6), (3, 6), (min(6, len(flows)), 6), (min(6, len(flows)), 2)):
                _same(_op_propagate(m, flows[:n], fb), R.propagate(m, flows[:n], fb),
                      "%s object %d, %d flows, frames_between %d" % (name, o, n, fb))
                n_checked += 1
    assert n_checked >= 8

"""The inputs of tests/test_mask_paths_gpu.py are sound, aimed and sharp -- checked without a GPU.

  * sound: tests/mask_ref.py (numpy, written from the contract) and the C oracle (oracle/ro_mask.c, oracle/ro_tracker.c) are two
    independent restatements of ImageSegmentationOFAidedSource; they agree bit for bit on every propagation of every case and,
    frame by frame, on every case in one of the two formats the oracle's tracker can be given.
  * aimed: each case reaches the branch of roft_amd/csrc/k_mask.hip it is there for, computed from the reference walk and the
    band / margin / thread figures of launch_mask_chain written down in mask_ref (retune them there and here it fails loudly).
  * sharp: each of mask_ref.DEFECTS, put into the reference, changes the expected masks of at least one case, and every case is
    moved by at least one of them.

Run with -s for the figures (lines MASKAIM and MASKSHARP); docs/notebook.md keeps a copy.
"""
import ctypes as C

import numpy as np
import pytest

import mask_ref as R

CASES = list(R.cases())
SMALL = [n for n in CASES if R.cases()[n].family != "capped_window"]


# ---------------------------------------------------------------------------------------------
# sound
# ---------------------------------------------------------------------------------------------
def oracle_flows(ob, flows):
    arr = (ob.Flow * max(1, len(flows)))()
    for i, f in enumerate(flows):
        rows, cols = f.data.shape[:2]
        arr[i] = ob.Flow(f.data.ctypes.data, ob.FLOW_S16C2 if f.data.dtype == np.int16 else ob.FLOW_F32C2, cols, rows, f.grid, f.scale, 1)
    return arr


def oracle_propagate(ob, mask, flows, frames_between):
    out = np.array(mask, np.uint8)
    H, W = out.shape
    scratch = np.zeros(H * W, np.int32)
    ob.lib().ro_mask_propagate(out.ctypes.data_as(C.c_void_p), W, H, oracle_flows(ob, flows), len(flows), frames_between,
                               scratch.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("name", CASES)
def test_propagate_equals_the_oracle(oracle, name):
    """Every propagation the reference does on the case -- the held mask through one flow, a delivered one through the
    buffered flows -- against ro_mask_propagate on the same inputs, unthresholded."""
    c = R.cases()[name]
    _, logs = R.run(name, keep_info=True)
    n = 0
    for o, log in enumerate(logs):
        for k, rec in enumerate(log):
            if rec["mode"] == 0:
                continue
            want = oracle_propagate(oracle, rec["in_mask"], rec["in_flows"], R.frames_between(c))
            assert np.array_equal(rec["out"], want), (name, k, o, rec["mode"], rec["n_flows"])
            n += 1
    assert n >= 2


def test_propagate_is_fast_enough_for_the_large_case():
    import time
    name = [n for n in CASES if R.cases()[n].family == "capped_window"][0]
    m, _ = R.frames(name)[2][0]
    flows = [R.frames(name)[k][0][1] for k in (1, 2)]
    t0 = time.perf_counter()
    R.propagate(m, flows, 6)
    assert time.perf_counter() - t0 < 1.0


def tracker_masks(ob, name):
    c = R.cases()[name]
    cfg = ob.default_config(c.W, c.H)
    cfg.cam.width, cfg.cam.height = c.W, c.H
    cfg.cam.fx = cfg.cam.fy = 1.5 * c.W
    cfg.cam.cx, cfg.cam.cy = c.W / 2, c.H / 2
    cfg.p_mean0[6:9] = (0.0, 0.0, 0.6)
    cfg.p_mean0[9:13] = (1.0, 0.0, 0.0, 0.0)
    cfg.mask_frames_between = R.frames_between(c)
    if not c.engine:
        cfg.use_pose_resync = 0      # (with it the tracker, like the engine, wants a mask on its first frame)
    verts, tris = R.small_mesh()
    trks = [ob.Tracker(cfg, verts, tris) for _ in range(c.n_obj)]
    depth = np.zeros((c.H, c.W), np.float32)
    out = []
    for k, row in enumerate(R.frames(name)):
        got = []
        for o, (m, f) in enumerate(row):
            trks[o].step(1.0 / 30.0, depth, None if f is None else f.data, m, R.POSE0 if k == 0 else None)
            got.append(trks[o].mask())
        out.append(got)
    for t in trks:
        t.close()
    return out


@pytest.mark.parametrize("name", [n for n in SMALL if R.cases()[n].fmt in R.STANDARD])
def test_source_equals_the_oracle_tracker(oracle, name):
    """Frame by frame: Source.step against ob.Tracker(...).mask() (the oracle's tracker derives grid and scale from the
    array: only the two standard formats)."""
    want = tracker_masks(oracle, name)
    for k, row in enumerate(R.expected(name)):
        for o, m in enumerate(row):
            assert np.array_equal(np.zeros_like(want[k][o]) if m is None else m, want[k][o]), (name, k, o)


def test_every_family_has_both_standard_formats():
    fams = {}
    for c in R.cases().values():
        fams.setdefault(c.family, set()).add(c.fmt)
    assert set(fams) == {"far_targets", "poison", "corner", "dense_rounds", "formats", "three_valued", "schedule", "capped_window"}
    for f in ("far_targets", "poison", "corner", "dense_rounds", "three_valued", "schedule"):
        assert set(R.STANDARD) <= fams[f], f
    assert {R.format_mode(f) for f in fams["formats"]} == {0, 1, 2}       # (2: S16 with grid 1 and scale 1)
    assert sum(R.cases()[n].W * R.cases()[n].H > 100 * 300 for n in CASES) == 1      # one large case


def test_objects_of_a_case_differ():
    for name in SMALL:
        fr = R.frames(name)
        if R.cases()[name].n_obj < 2:
            continue
        assert any(a[1] is not None and b[1] is not None and not np.array_equal(a[1].data, b[1].data) for a, b, *_ in fr), name
        last = R.expected(name)[-1]
        assert not np.array_equal(last[0], last[1]), name


# ---------------------------------------------------------------------------------------------
# aimed
# ---------------------------------------------------------------------------------------------
def _print_aim(name, a):
    print("MASKAIM %-44s out %6d in %7d | delivering out %6d in %7d | listed %3d per wave %2d rounds %d chunks %2d | fill %s clear00 %s "
          "bg1 %s general %d mid-chase drops %d" % (name, a["outside"], a["inside"], a["outside_delivering"], a["inside_delivering"],
                                                     a["groups_listed"], a["groups_per_wave"], a["rounds"], a["chunks"],
                                                     a["fill_frames"], a["clear00_frames"][:3], a["bg_one_frames"],
                                                     len(a["general_frames"]), a["mid_chase_drops"]))


@pytest.mark.parametrize("name", CASES)
def test_case_reaches_its_branch(name):
    c = R.cases()[name]
    a = R.aim(name)
    _print_aim(name, a)
    fam = c.family
    modes = {(k, o): (m, n) for k, o, m, n in a["modes"]}
    if fam in ("far_targets", "capped_window"):
        assert a["outside"] >= 64 and a["inside"] >= 64
    if fam == "far_targets":
        assert a["outside_delivering"] >= 64 and a["inside_delivering"] >= 64
    if fam == "capped_window":
        # the window of the one workgroup ends before the image does, on ordinary and on delivering frames, and the
        # pixels counted above are on both sides of it
        for fresh in (False, True):
            b = R.Bands(c.W, c.H, fresh, 1)
            assert b.n_wg == 1 and 0 < b.capped_row < c.H and c.H - b.capped_row <= 64
        assert a["outside_delivering"] >= 64 and a["inside_delivering"] >= 64 and a["chunks"] >= 80
    if fam == "dense_rounds":
        if c.over.get("mask_workgroups_per_object") == 1:
            assert a["chunks"] == 3 and a["groups_per_wave"] == 64 and a["groups_listed"] == 256     # (3: the delivering frame's)
            ordinary = R.Bands(c.W, c.H, False, 1)
            assert len(ordinary.lists(np.ones(c.W * c.H, bool))[0]) == 2
        else:
            assert a["groups_listed"] == 80 and a["groups_per_wave"] == 20 and a["rounds"] == 2 and a["chunks"] == 1
    if fam == "poison":
        assert a["kinds"] >= R.poison_kinds(c.fmt), R.poison_kinds(c.fmt) - a["kinds"]
        assert a["mid_chase_drops"] >= 16
    if fam == "corner":
        if "_fill_" in name:
            assert a["fill_frames"] == [(3, 0), (3, 1)]
            assert {(4, 0), (4, 1)} <= set(a["clear00_frames"])
            full = R.Bands(c.W, c.H, False).lists(np.ones(c.W * c.H, bool))
            assert a["groups_listed"] == max(max(q) for q in full)          # frame 4 lists every group of its bands
        if "_land_" in name:
            assert a["clear00_frames"] == [(3, 0), (3, 1)]
        if "_bg_one_" in name:
            assert a["bg_one_frames"] == [(3, 0), (3, 1)] and {(4, 0), (5, 0)} <= set(a["general_frames"])
    if fam == "three_valued":
        g = set(a["general_frames"])
        assert {(k, 0) for k in range(3, 13)} <= g and (13, 0) not in g
        assert (1, 1) in g and (5, 1) in g and (10, 1) in g and not any(o == 2 for _, o in g)
        assert a["kinds"] >= R.poison_kinds(c.fmt) - {"neg_fraction", "edge_in", "edge_out"}
    if fam == "formats":
        assert {n for (k, o), (m, n) in modes.items() if m == 2} >= {3, 4}
        assert any(m == 1 for m, _ in modes.values())
    if fam == "schedule":
        if "no_mask_first" in name:
            assert modes[(0, 0)] == (0, 0) and modes[(3, 0)] == (1, 1) and modes[(7, 0)] == (2, 6) and not c.engine
        if "consecutive" in name:
            assert [modes[(k, 0)] for k in (1, 2, 3)] == [(2, 1)] * 3
        if "delivery_without_flow" in name:
            assert modes[(2, 0)] == (2, 0) and modes[(6, 0)] == (2, 3) and modes[(5, 1)] == (2, 4) and modes[(7, 1)] == (0, 0)
        if "missing_flows" in name:
            assert [modes[(k, 0)][0] for k in (3, 4, 5, 8)] == [0] * 4 and modes[(9, 0)] == (2, 5)
        if "empty_delivery" in name:
            fb = R.frames_between(c)
            assert modes[(4, 0)] == (1, 1) and modes[(7, 0)] == (2, 6 if fb > 0 else 4)
        if "8_buffered" in name:
            assert modes[(8, 0)] == (2, 8) and modes[(9, 1)] == (2, 9)
        if "%d_buffered" % R.MAX_FLOW_CHASE in name:
            assert modes[(R.MAX_FLOW_CHASE, 0)] == (2, R.MAX_FLOW_CHASE)


# ---------------------------------------------------------------------------------------------
# sharp
# ---------------------------------------------------------------------------------------------
def _moved(name, defect):
    got, _ = R.run(name, defect=defect)
    want = R.expected(name)
    return sum(not np.array_equal(a, b) for ra, rb in zip(got, want) for a, b in zip(ra, rb) if b is not None)


@pytest.fixture(scope="module")
def sharpness():
    return {d: {n: _moved(n, d) for n in CASES} for d in R.DEFECTS}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_moves_a_case(sharpness, defect):
    hit = {n: v for n, v in sharpness[defect].items() if v}
    fams = sorted({R.cases()[n].family for n in hit})
    print("MASKSHARP %-24s moves %2d cases (%3d masks) of families %s" % (defect, len(hit), sum(hit.values()), ", ".join(fams)))
    assert hit, defect


# the family a defect must move: the one that aims at it
@pytest.mark.parametrize("defect,family", [
    ("outside_window_dropped", "far_targets"), ("outside_window_dropped", "capped_window"), ("clear00_omitted", "corner"),
    ("clear00_in_mode2", "corner"), ("unmapped_zero", "corner"), ("nan_as_zero", "poison"), ("floor", "poison"),
    ("newest_first", "formats"), ("smallest_wins", "three_valued"), ("reciprocal", "formats"),
    ("first_flow_buffered", "schedule"), ("buffer_kept_on_empty", "schedule")])
def test_defect_moves_the_family_that_aims_at_it(sharpness, defect, family):
    assert any(v for n, v in sharpness[defect].items() if R.cases()[n].family == family)


def test_every_case_is_moved_by_a_defect(sharpness):
    idle = [n for n in CASES if not any(sharpness[d][n] for d in R.DEFECTS)]
    assert not idle, idle


def test_reciprocal_shows_only_where_the_scale_is_no_power_of_two(sharpness):
    for n, v in sharpness["reciprocal"].items():
        if v:
            assert R.format_mode(R.cases()[n].fmt) == 0, n


def test_empty_delivery_depends_on_frames_between():
    """The same inputs with frames_between 6, 0 and -1: known -> the buffer survives the empty mask; unknown -> dropped."""
    for s in ("f32_g1_s1", "s16_g4_s32"):
        e6, e0, em = (R.expected("schedule_empty_delivery_fb%d_%s" % (fb, s)) for fb in (6, 0, -1))
        assert all(np.array_equal(a, b) for ra, rb in zip(e0, em) for a, b in zip(ra, rb))
        assert any(not np.array_equal(a, b) for ra, rb in zip(e6, e0) for a, b in zip(ra, rb))

"""Drivers of the restart tests (roft_objects_restart): an engine run is described slot by slot as a list of TRACKS -- which stream
a slot follows from which engine frame on, and the description it is (re)started with -- so that the run with restarts, the run
without, the new engines and the oracle are all fed from one description."""
import numpy as np

from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import synth

import util

RAW_SCALE = 0.001
LABEL = 7


class Track:
    """From engine frame F on the slot follows stream `st` from its frame k0 on.  m0: the initial pose mean (13 doubles; None: the
    stream's first delivered pose, as the reference initialises).  first_mask_gt: the track's first frame delivers the ground-truth
    mask of that very frame (a re-acquisition inside a sequence: the caller detected the object anew).  drop_first_pose: the first
    frame hands no pose.  keep_mesh: the restart that starts the track passes ROFT_RESTART_KEEP_MESH."""

    def __init__(self, F, st, k0=0, m0=None, first_mask_gt=False, drop_first_pose=False, keep_mesh=False):
        self.F, self.st, self.k0, self.first_mask_gt, self.drop_first_pose, self.keep_mesh = F, st, k0, first_mask_gt, drop_first_pose, keep_mesh
        self.m0 = np.array(synth.initial_pose_from_stream(st) if m0 is None else m0, np.float64)

    def desc(self):
        d = E.default_object()
        for i in range(13):
            d.p_mean0[i] = self.m0[i]
        return d

    def inputs(self, f):
        """(depth, flow, mask, pose) of engine frame f >= F, as the oracle and the engine take them"""
        k = self.k0 + f - self.F
        depth, flow, mask, pose = util.frame_inputs(self.st, k)
        if f == self.F:
            if self.first_mask_gt:
                mask = self.st.mask_gt[self.st.image(k)].numpy()
            if self.drop_first_pose:
                pose = None
        return depth, flow, mask, pose


def gt_mean(st, k):
    m = np.zeros(13)
    m[6:9], m[9:13] = st.gt.x[st.image(k)], st.gt.q[st.image(k)]
    return m


def track_at(plan, f):
    return [t for t in plan if t.F <= f][-1]


def _shared(cache, key, make):
    if key not in cache:
        cache[key] = make()
    return cache[key]


def frame_dict(track, f, mode, cache, dev=None):
    """The engine's frame dict of engine frame f.  mode: "plain" host arrays | "nomask" | "device" (tensors in HBM: dev maps id(stream) to
    util.to_device(stream)) | "images" (camera image instead of the flow, 16-bit raw depth, the mask as a label image: ONE array per
    stream frame, so that the slots of a shared scene name one host pointer)."""
    depth, flow, mask, pose = track.inputs(f)
    st, k = track.st, track.k0 + f - track.F
    if mode == "plain":
        return dict(depth=depth, flow=flow, mask=mask, pose=pose, dt=st.dt)
    if mode == "nomask":   # (pose masks: the stream's masks are withheld; only a track's first_mask_gt mask is delivered)
        return dict(depth=depth, flow=flow, mask=mask if (f == track.F and track.first_mask_gt) else None, pose=pose, dt=st.dt)
    if mode == "device":
        d = util.device_frame(dev[id(st)], k)
        if f == track.F and track.first_mask_gt:
            d["mask"] = dev[id(st)].mask_gt[st.image(k)].data_ptr()
        if f == track.F and track.drop_first_pose:
            d["pose"] = None
        return d
    i = st.image(k)
    out = dict(dt=st.dt, pose=pose)
    out["depth"] = _shared(cache, (id(st), "raw", i), lambda: np.clip(np.rint(st.depth[i].numpy() / RAW_SCALE), 0, 65535).astype(np.uint16))
    out["image"] = _shared(cache, (id(st), "gray", i), lambda: np.ascontiguousarray(st.gray[i].numpy()))
    if mask is not None:
        mi = i if (f == track.F and track.first_mask_gt) else int(st.mask_delivery[k])
        out["labels"] = _shared(cache, (id(st), "lab", mi), lambda: np.where(st.mask_gt[mi].numpy() > 0, LABEL, 0).astype(np.uint8))
        out["label"] = LABEL
    return out


def full_log(eng, first, n):
    """[n][objects] of (pose bytes, twist bytes, n_flow_points, outlier_selected, outlier_L bytes): equal records are equal bits"""
    outs = (L.ObjectOutput * (n * eng.n_objects))()
    L.check(L.lib().roft_engine_get_log(eng._h, first, n, outs))
    rows = [(np.array(r.pose[:]).tobytes(), np.array(r.twist[:]).tobytes(), r.n_flow_points, r.outlier_selected, np.array(r.outlier_L[:]).tobytes())
            for r in outs]
    return [rows[f * eng.n_objects:(f + 1) * eng.n_objects] for f in range(n)]


def make_engine(plans, cam_stream, log_frames, setup=None, max_batch_frames=1, before_first=None, **over):
    """An engine whose object i is added with the description and mesh of plans[i]'s first track.  before_first(eng): called when
    the objects are there, ahead of the log and of `setup` (the other enable calls)."""
    st0 = cam_stream
    cfg = E.default_config(st0.camera.width, st0.camera.height, st0.flow_type, max_objects=len(plans), max_batch_frames=max_batch_frames)
    c = st0.camera
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = c.fx, c.fy, c.cx, c.cy
    cfg.flow_grid, cfg.flow_scale = st0.flow_grid, st0.flow_scale
    for k, v in over.items():
        setattr(cfg, k, v)
    eng = E.ROFTFilterBatch(cfg)
    for plan in plans:
        eng.add_object(plan[0].desc(), *plan[0].st.mesh)
    if before_first:
        before_first(eng)
    eng.enable_log(log_frames)   # (ahead of the enable calls: the quality ring takes the log's capacity)
    if setup:
        setup(eng)
    return eng


def run(plans, n, splits=None, mode="plain", setup=None, between=None, before_first=None, per_step=None, read_masks=True, after_restart=None,
        after_submit=None, finish=None, **over):
    """Runs n engine frames: slot i follows plans[i]; every track with F > 0 starts by ONE roft_objects_restart call per engine
    frame F for all slots that start one there (F must be a batch boundary).  splits: batch sizes, cycled (None: one-frame submits).
    Hooks: between(eng, f) at every batch boundary f, before the restarts of f; after_restart(eng, f) behind them; after_submit(eng, f)
    between the submit and the step of the batch that starts at f; per_step(eng, f_last, got) behind every step; finish(eng, got)
    before the engine is closed.  Returns dict(log=[n][slots] records, rows=get_log_rows, masks={(f, slot)} at every batch's last frame (read_masks False: the run's last), stats)."""
    st0 = plans[0][0].st
    eng = make_engine(plans, st0, max(n, 1), setup, max(splits) if splits else 1, before_first, **over)
    cache, dev = {}, {}
    if mode == "device":
        for plan in plans:
            for t in plan:
                dev.setdefault(id(t.st), util.to_device(t.st))
    got = dict(masks={}, extra={})
    f, i = 0, 0
    while f < n:
        if between:
            between(eng, f)
        starting = [(slot, track_at(plan, f)) for slot, plan in enumerate(plans) if f > 0 and any(t.F == f for t in plan)]
        if starting:
            keep = [t.keep_mesh for _, t in starting]
            assert all(keep) or not any(keep)
            eng.restart_objects([(slot, t.desc(), t.st.mesh[0], t.st.mesh[1]) for slot, t in starting], keep_mesh=keep[0])
            if after_restart:
                after_restart(eng, f)
        T = min(splits[i % len(splits)] if splits else 1, n - f)
        i += 1
        frames = [[frame_dict(track_at(plan, f + j), f + j, mode, cache, dev) for plan in plans] for j in range(T)]
        if T == 1 and not splits:
            eng.submit(frames[0])
        else:
            eng.submit_batch(frames)
        if after_submit:
            after_submit(eng, f)
        eng.step()
        f += T
        if read_masks or f >= n:   # (reading a mask waits for the device: without it batches are in flight when a restart comes)
            for slot in range(len(plans)):
                got["masks"][(f - 1, slot)] = eng.mask(slot)
        if per_step:
            per_step(eng, f - 1, got)
    got["log"] = full_log(eng, 0, n)
    got["rows"] = eng.get_log_rows(0, n)
    got["stats"] = eng.stats()
    got["restart_stats"] = eng.restart_stats()
    if finish:
        finish(eng, got)
    eng.close()
    return got


def oracle_track(ob, track, n, **over):
    """A fresh oracle tracker over the track's first n frames: the list util.run_oracle_tracker returns."""
    st = track.st
    cfg = util.oracle_config(ob, st, **over)
    for i in range(13):
        cfg.p_mean0[i] = track.m0[i]
    trk = ob.Tracker(cfg, *st.mesh)
    out = []
    for f in range(track.F, track.F + n):
        depth, flow, mask, pose = track.inputs(f)
        r = trk.step(st.dt, depth, flow, mask, pose)
        out.append(dict(pose=np.array(r.pose), twist=np.array(r.twist), n=r.n_flow_points, sel=r.outlier_selected, L=np.array(r.outlier_L),
                        mask=trk.mask()))
    trk.close()
    return out


def rot_err(qa, qb):
    return 2.0 * np.arccos(min(1.0, abs(float(np.dot(qa, qb)))))


def assert_matches_oracle(log, masks, slot, F, ref, tol=1e-6, lik_rtol=1e-9):
    """Engine frames F .. F + len(ref) - 1 of `slot` against the oracle's track, at the bars of tests/test_engine_gpu.py: point counts,
    decisions and masks exact, likelihoods rtol 1e-9, position / rotation / twist 1e-6.  Returns the number of outlier tests."""
    n_tests = 0
    for k, exp in enumerate(ref):
        pose_b, twist_b, npts, sel, L_b = log[F + k][slot]
        pose, twist, lik = np.frombuffer(pose_b), np.frombuffer(twist_b), np.frombuffer(L_b)
        assert npts == exp["n"], (F + k, slot)
        assert sel == exp["sel"], (F + k, slot, list(lik), exp["L"])
        if exp["sel"] >= 0:
            n_tests += 1
            np.testing.assert_allclose(lik, exp["L"], rtol=lik_rtol)
        np.testing.assert_allclose(pose[:9], exp["pose"][:9], rtol=0, atol=tol, err_msg="frame %d slot %d" % (F + k, slot))
        assert rot_err(pose[9:], exp["pose"][9:]) < tol, (F + k, slot)
        np.testing.assert_allclose(twist, exp["twist"], rtol=0, atol=tol)
        if (F + k, slot) in masks:
            assert np.array_equal(masks[(F + k, slot)], exp["mask"]), (F + k, slot)
    return n_tests


def assert_same_bits(a, slot_a, Fa, b, slot_b, Fb, n, what="", need_mask=True):
    """n frames of slot_a from frame Fa of run a equal those of slot_b from Fb of run b: log records, and the masks both runs read"""
    for k in range(n):
        assert a["log"][Fa + k][slot_a] == b["log"][Fb + k][slot_b], "%s: record of frame %d (+%d)" % (what, Fa + k, k)
    assert np.array_equal(a["rows"][Fa:Fa + n, slot_a].view(np.uint64), b["rows"][Fb:Fb + n, slot_b].view(np.uint64)), what
    shared = 0
    for k in range(n):
        if (Fa + k, slot_a) in a["masks"] and (Fb + k, slot_b) in b["masks"]:
            assert np.array_equal(a["masks"][(Fa + k, slot_a)], b["masks"][(Fb + k, slot_b)]), "%s: mask of frame %d (+%d)" % (what, Fa + k, k)
            shared += 1
    assert shared > 0 or not need_mask, what + ": no mask to compare"

"""Label-image masks on the device (roft_frames_submit_labels, roft_labels_to_masks; label_ingest_kernel in
roft_amd/csrc/k_mask.hip): an object that names a label image and a value behaves, bit for bit, as if it had been handed the mask
(labels == value) * 255 through roft_frame_input::mask.  So every engine test here runs two engines on identical inputs -- one
gets the expanded masks through the existing call, one the label image -- and asks for EQUAL logs and masks.

Shapes: util.stream(seed, n, scale=4) is 160 x 120 = 300 groups of 64 pixels, one full 256-thread workgroup of the ingest and a
partial one."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import io, ops

import util
from test_engine_gpu import make_engine

pytestmark = pytest.mark.gpu

N_FRAMES = 14          # deliveries at frames 0, 6 and 12
SPLITS = [4, 8, 2]     # batches: a delivery first in a batch, in the middle of one, and twice in one (frames 4 .. 11 hold 6 only;
                       # 12 opens the last) -- together with frame-by-frame submits


# ---- 1. the operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_operator_against_numpy(dtype):
    rng = np.random.default_rng(5)
    H, W = 120, 160
    if dtype == np.uint8:
        lab = rng.choice(np.array([0, 1, 2, 3, 5, 255], np.uint8), size=(H, W))
        values = [1, 2, 3, 5, 255, 4, 3, 254]          # 4 and 254 are absent, 3 is repeated
    else:
        # 259 = 0x0103 and 3 share the low byte, 768 = 0x0300 and 3 << 8 the high one: a comparison of one byte confuses them
        lab = rng.choice(np.array([0, 1, 3, 259, 768, 65535, 515], np.uint16), size=(H, W))
        values = [3, 259, 768, 65535, 1, 515, 2, 3, 258, 256]   # 2, 258 and 256 are absent, 3 is repeated
    masks, counts = ops.labels_to_masks(lab, values)
    assert masks.shape == (len(values), H, W) and masks.dtype == np.uint8
    for i, v in enumerate(values):
        want = (lab == v).astype(np.uint8) * 255
        assert np.array_equal(masks[i], want), (dtype, v)
        assert counts[i] == int((lab == v).sum()), (dtype, v)
    absent = [i for i, v in enumerate(values) if not (lab == v).any()]
    assert len(absent) >= 2 and all(counts[i] == 0 and not masks[i].any() for i in absent)
    # a single value, and an image whose every pixel is the value (every bit of every plane word set)
    full = np.full((H, W), 7, dtype)
    m, c = ops.labels_to_masks(full, [7])
    assert c[0] == H * W and (m == 255).all()


# ---- the two-engine harness --------------------------------------------------------------------------------------------
def _streams():
    return [util.stream(1400 + i, N_FRAMES, scale=4) for i in range(3)]


def _delivered(st, k):
    return st.mask_gt[st.mask_delivery[k]].numpy() if st.mask_delivery[k] >= 0 else None


@functools.lru_cache(maxsize=None)
def _label_images(dtype_name, skip=(6, 1), values=(1, 2, 3)):
    """Per delivering frame: the label image composed by writing object i's delivered mask with values[i], in order (a later
    object overwrites an earlier one where they overlap), and the masks expanded from it.  skip = (frame, object): that object
    is left out of that frame's image, so its label does not occur there."""
    streams = _streams()
    out = {}
    for k in range(N_FRAMES):
        masks = [_delivered(st, k) for st in streams]
        if masks[0] is None:
            assert all(m is None for m in masks)
            continue
        lab = np.zeros(masks[0].shape, np.dtype(dtype_name))
        for i, m in enumerate(masks):
            if (k, i) != tuple(skip):
                lab[m > 0] = values[i]
        out[k] = (lab, [np.ascontiguousarray((lab == v).astype(np.uint8) * 255) for v in values])
    assert sorted(out) == [0, 6, 12]
    assert not out[6][1][1].any() and all(out[6][1][i].any() for i in (0, 2))      # the absent label: an empty new mask
    assert all(m.any() for k in (0, 12) for m in out[k][1])
    return out


class Holder:
    """Inputs of one run in the memory kind under test; keeps every buffer alive until the engines are closed (DEVICE inputs
    are read in place)."""

    def __init__(self, mem):
        self.mem = mem
        self.kept = []

    def put(self, arr):
        """numpy array -> what a frame dict takes for it"""
        if arr is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(arr).view(np.int16) if arr.dtype == np.uint16 else np.ascontiguousarray(arr))
        if self.mem == "device":
            t = t.cuda()
            self.kept.append(t)
            return t.data_ptr()
        if self.mem == "pinned":
            t = t.pin_memory()
            assert t.is_pinned()
            self.kept.append(t)
            a = t.numpy()
            return a.view(np.uint16) if arr.dtype == np.uint16 else a
        return arr

    @property
    def kind(self):
        return L.MEM_DEVICE if self.mem == "device" else L.MEM_HOST


def _frames(holder, k, mask_of, labels_of=None):
    """The frame dicts of frame k.  mask_of(i) -> per-object mask array or None; labels_of(i) -> (label array as put() returned
    it, dtype, value) or None."""
    streams = _streams()
    frames = []
    for i, st in enumerate(streams):
        depth, flow, _, pose = util.frame_inputs(st, k)
        f = dict(depth=holder.put(depth), flow=holder.put(flow), mask=holder.put(mask_of(i)), pose=pose, dt=st.dt, mem_kind=holder.kind)
        lab = labels_of(i) if labels_of else None
        if lab is not None:
            f["labels"], f["label"] = lab[0], lab[2]
            if isinstance(lab[0], int):
                f["label_type"] = L.LABEL_U8 if lab[1] == np.uint8 else L.LABEL_U16
        frames.append(f)
    return frames


def _read_log(eng, n):
    outs = (L.ObjectOutput * (n * eng.n_objects))()
    L.check(L.lib().roft_engine_get_log(eng._h, 0, n, outs))
    rows = [outs[i] for i in range(n * eng.n_objects)]
    return dict(pose=np.array([r.pose[:] for r in rows]), twist=np.array([r.twist[:] for r in rows]),
                npts=np.array([r.n_flow_points for r in rows]), sel=np.array([r.outlier_selected for r in rows]),
                lik=np.array([r.outlier_L[:] for r in rows]))


def _run(frames_of, splits, n=N_FRAMES, max_batch=8):
    """frames_of(k) -> frame dicts.  Returns (log, final masks, stats)."""
    eng = make_engine(_streams(), max_batch_frames=max_batch)
    eng.enable_log(n)
    k = i = 0
    while k < n:
        t = 1 if splits is None else min(splits[i % len(splits)], n - k)
        i += 1
        if splits is None:
            eng.submit(frames_of(k))
        else:
            eng.submit_batch([frames_of(k + j) for j in range(t)])
        eng.step()
        k += t
    log = _read_log(eng, n)
    masks = [eng.mask(o) for o in range(eng.n_objects)]
    stats = eng.stats()
    eng.close()
    return log, masks, stats


def _assert_same(a, b, what=""):
    (la, ma, _), (lb, mb, _) = a, b
    for key in ("pose", "twist", "npts", "sel", "lik"):
        assert np.array_equal(la[key], lb[key], equal_nan=True), (what, key)
    for o, (x, y) in enumerate(zip(ma, mb)):
        assert np.array_equal(x, y), (what, "mask", o)


@functools.lru_cache(maxsize=None)
def _expanded_run(mem, batched):
    """Engine A: the masks expanded from the label images (the same for 8- and 16-bit images), through the existing calls."""
    images = _label_images("uint8")
    holder = Holder(mem)
    out = _run(lambda k: _frames(holder, k, lambda i: images[k][1][i] if k in images else None), SPLITS if batched else None)
    assert (out[0]["sel"] >= 0).any() and (out[0]["npts"] > 0).any(), "the run tracks: outlier tests and flow points"
    return out


# ---- 2. engine parity, exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
@pytest.mark.parametrize("mem", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("batched", [False, True], ids=["frame_by_frame", "splits_4_8_2"])
def test_engine_parity_with_expanded_masks(batched, mem, dtype):
    images = _label_images(np.dtype(dtype).name)
    holder = Holder(mem)
    per_frame = {}

    def labels_of(k):
        if k not in images:
            return lambda i: None
        if k not in per_frame:
            per_frame[k] = holder.put(images[k][0])     # ONE buffer per delivery, named by all three objects
        return lambda i: (per_frame[k], dtype, i + 1)

    got = _run(lambda k: _frames(holder, k, lambda i: None, labels_of(k)), SPLITS if batched else None)
    want = _expanded_run(mem, batched)
    _assert_same(got, want, (batched, mem, dtype))
    # the empty-mask rule held for object 1 at frame 6 (its label is absent there): its mask went on from the one before, and is
    # not empty at the end
    assert got[1][1].any()


# ---- 3. mixed frame ----------------------------------------------------------------------------------------------------
def test_mixed_frame_three_valued_mask_next_to_labels():
    """Object 0: an ordinary mask with pixels of value 1 (the general, map-based propagation: nz plane != obj plane); objects 1
    and 2: from one label image in the same frames."""
    streams = _streams()
    images = {}
    for k in range(N_FRAMES):
        m = [_delivered(st, k) for st in streams]
        if m[0] is None:
            continue
        three = m[0].copy()
        vs, us = np.nonzero(three)
        three[vs[::3], us[::3]] = 1
        lab = np.zeros(three.shape, np.uint8)
        for i in (1, 2):
            lab[m[i] > 0] = i + 1
        images[k] = (lab, [three] + [np.ascontiguousarray((lab == i + 1).astype(np.uint8) * 255) for i in (1, 2)])
        assert (three == 1).any() and (three == 255).any()
    for batched in (False, True):
        ha, hb = Holder("pageable"), Holder("pageable")
        want = _run(lambda k: _frames(ha, k, lambda i: images[k][1][i] if k in images else None), SPLITS if batched else None)
        got = _run(lambda k: _frames(hb, k, lambda i: images[k][1][0] if (k in images and i == 0) else None,
                                     (lambda i: (images[k][0], np.uint8, i + 1) if i > 0 else None) if k in images else None),
                   SPLITS if batched else None)
        _assert_same(got, want, batched)


# ---- 4. no labels ------------------------------------------------------------------------------------------------------
def test_null_labels_is_exactly_frames_submit():
    images = _label_images("uint8")

    def run(through_labels_call):
        holder = Holder("device")
        eng = make_engine(_streams(), max_batch_frames=8)
        eng.enable_log(N_FRAMES)
        k = 0
        for t in SPLITS:
            arr, keep, T = eng.build_batch([_frames(holder, k + j, lambda i: images[k + j][1][i] if k + j in images else None) for j in range(t)])
            assert eng.batch_labels(keep) is None
            if through_labels_call:
                L.check(L.lib().roft_frames_submit_labels(eng._h, arr, None, eng.n_objects, T))
            else:
                L.check(L.lib().roft_frames_submit(eng._h, arr, eng.n_objects, T))
            eng.step()
            k += t
        out = _read_log(eng, N_FRAMES), [eng.mask(o) for o in range(3)], eng.stats()
        eng.close()
        return out

    a, b = run(False), run(True)
    _assert_same(a, b)
    assert a[2]["launches"] == b[2]["launches"] and a[2]["event_ops"] == b[2]["event_ops"]
    assert a[2]["launches"] > 0


def test_ingest_launches_do_not_grow_with_the_objects():
    """A batch with label masks enqueues ONE launch more than the same batch without a delivery would spend on ingest, however
    many objects name the image: launches of a run with 1 object and with 3 differ by nothing the ingest adds."""
    images = _label_images("uint8")
    st = _streams()

    def launches(n_obj, form):
        holder = Holder("device")
        eng = make_engine(st[:n_obj], max_batch_frames=8)
        k = 0
        for t in SPLITS:
            batch = []
            for j in range(t):
                kk = k + j
                lab = holder.put(images[kk][0]) if (form == "labels" and kk in images) else None
                fr = _frames(holder, kk, (lambda i: images[kk][1][i] if kk in images else None) if form == "masks" else (lambda i: None),
                             (lambda i: (lab, np.uint8, i + 1)) if lab is not None else None)
                batch.append(fr[:n_obj])
            eng.submit_batch(batch)
            eng.step()
            k += t
        eng.sync()
        n = eng.stats()["launches"]
        eng.close()
        return n

    # per-object masks in this burst ride in the control-block launch (no launch of their own); labels add one per batch that
    # delivers, i.e. 3 here (frames 0, 6 and 12 fall into the three batches) -- for one object and for three
    assert launches(1, "labels") - launches(1, "masks") == launches(3, "labels") - launches(3, "masks") == 3


# ---- 5. bytes on the bus -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_one_upload_per_label_image(dtype, mem):
    """n objects that share one depth, one flow and one label image per frame: the image crosses the bus once per delivery."""
    st = _streams()[0]
    images = _label_images(np.dtype(dtype).name)
    n, W, H = 3, st.camera.width, st.camera.height
    depth_b, flow_b = W * H * 4, W * H * 8
    flows = int(sum(bool(st.flow_valid[k]) for k in range(N_FRAMES)))
    D = len(images)
    assert 0 < flows < N_FRAMES and D == 3

    def run(form):
        holder = Holder(mem)
        eng = make_engine([st] * n)
        for k in range(N_FRAMES):
            depth, flow, _, pose = util.frame_inputs(st, k)
            d, f = holder.put(depth), holder.put(flow)
            lab = holder.put(images[k][0]) if (k in images and form == "labels") else None
            frames = []
            for i in range(n):
                fr = dict(depth=d, flow=f, mask=None, pose=pose, dt=st.dt)
                if k in images:
                    if form == "labels":
                        fr["labels"], fr["label"] = lab, i + 1
                    else:
                        fr["mask"] = holder.put(images[k][1][i])
                frames.append(fr)
            eng.submit(frames)
            eng.step()
        eng.sync()
        s = eng.stats()
        eng.close()
        return s

    scene = N_FRAMES * (depth_b + flow_b) - (N_FRAMES - flows) * flow_b
    s = run("labels")
    assert s["h2d_bytes"] == scene + D * W * H * np.dtype(dtype).itemsize
    if mem == "pageable":
        assert s["h2d_copies"] == N_FRAMES + flows + D       # one hipMemcpyAsync per distinct image
    else:
        assert s["h2d_copies"] == N_FRAMES                   # pinned: one gather launch per submit, the label image in it
    if dtype == np.uint8:
        s = run("masks")
        assert s["h2d_bytes"] == scene + D * n * W * H


# ---- 6. errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["pageable", "device"])
def test_refusals_consume_nothing(mem):
    images = _label_images("uint8")
    want = _expanded_run(mem, False)
    holder = Holder(mem)
    streams = _streams()
    eng = make_engine(streams)
    eng.enable_log(N_FRAMES)
    n_refused = 0
    for k in range(N_FRAMES):
        lab = holder.put(images[k][0]) if k in images else None
        lab16 = holder.put(images[k][0].astype(np.uint16)) if k in images else None

        def good():
            return _frames(holder, k, lambda i: None, (lambda i: (lab, np.uint8, i + 1)) if k in images else None)

        if k in images:
            bad = []
            f = good(); f[1]["mask"] = holder.put(images[k][1][1]); bad.append(("a label image AND a mask", f))
            f = good(); f[2]["label"] = 0; bad.append(("label 0", f))
            f = good(); f[0]["label"] = 256; bad.append(("label outside u8", f))
            f = good(); f[0]["label"] = -3; bad.append(("negative label", f))
            f = good()
            for i in range(3):
                f[i]["labels"], f[i]["label_type"] = (lab16 if mem == "device" else lab16.ctypes.data), L.LABEL_U16
            f[1]["label"] = 65536; bad.append(("label outside u16", f))
            f = good()
            for i in range(3):
                f[i]["labels"], f[i]["label_type"] = (lab if mem == "device" else lab.ctypes.data), (7 if i == 2 else L.LABEL_U8)
            bad.append(("unknown label_type", f))
            if mem == "device":
                f = good(); f[1]["labels"] = lab + 8; f[1]["label_type"] = L.LABEL_U8; bad.append(("misaligned DEVICE image", f))
            for what, frames in bad:
                with pytest.raises(L.RoftError) as err:
                    eng.submit(frames)
                assert "error -1:" in str(err.value) and len(str(err.value).split(":", 1)[1].strip()) > 10, what
                n_refused += 1
        eng.submit(good())
        eng.step()
    assert n_refused == 3 * (7 if mem == "device" else 6)
    got = _read_log(eng, N_FRAMES), [eng.mask(o) for o in range(3)], eng.stats()
    eng.close()
    _assert_same(got, want, mem)


# ---- 7. closing the loop with the renderer -----------------------------------------------------------------------------
def test_instance_map_of_the_scene_renderer_as_label_image():
    import mesh_zoo
    import scene_util as su
    v, t = mesh_zoo.box(6)
    box = (v.astype(np.float32), t)
    W, H = 160, 120
    cam = su.lib_cam(su.cam(W, H))
    poses = np.stack([su.pose([0.0, 0.0, 0.40], [1, 2, 3], 0.5), su.pose([0.09, 0.01, 0.55], [2, 1, 0], 0.9)])[None]
    inst = ops.render_scene(cam, [box, box], [0, 1], poses, outputs=("instance",))["instance"][0]
    assert (inst == 0).sum() > 200 and (inst == 1).sum() > 200, "both boxes are visible"
    # they overlap: the box behind is cut by the one in front, so its visible pixels are not the footprint of a box drawn alone
    alone = ops.render_scene(cam, [box], [0], poses[:, 1:], outputs=("instance",))["instance"][0]
    assert ((alone == 0) & (inst == 0)).any() and (inst == 1).sum() < (alone == 0).sum()
    lab = io.labels_from_instances(inst)
    cfg = E.default_config(W, H, L.FLOW_F32C2, max_objects=2)
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
    eng = E.ROFTFilterBatch(cfg)
    for i in range(2):
        d = E.default_object()
        d.p_mean0[6:9] = list(poses[0, i, :3])
        d.p_mean0[9:13] = list(poses[0, i, 3:])
        eng.add_object(d, *box)
    depth = np.full((H, W), 0.5, np.float32)
    eng.submit([dict(depth=depth, flow=None, labels=lab, label=i + 1, pose=None) for i in range(2)])
    eng.step()
    for i in range(2):
        assert np.array_equal(eng.mask(i), (inst == i).astype(np.uint8) * 255), i
    eng.close()

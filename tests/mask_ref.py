"""A plain numpy restatement of optical-flow-aided mask propagation, and the case table of tests/test_mask_ref_cpu.py and
tests/test_mask_paths_gpu.py.

Written from the contract -- ImageSegmentationOFAidedSource<T>::step_frame / map (ImageSegmentationOFAidedSource.hpp:127-281),
cv::remap with an integer map, the threshold of ImageSegmentationMeasurement::freeze -- and from nothing else: no bit planes, no
bands, no windows, no lists.  It shares no code with oracle/ro_mask.c or oracle/ro_tracker.c either; test_mask_ref_cpu.py shows
that the two restatements agree bit for bit, which is what makes either trustworthy.

  propagate(mask, flows, frames_between)   map() + remap() of one mask through a list of flows
  Source(frames_between).step(mask, flow)  the non-stamped step_frame state machine, output thresholded (> 1 -> 255)
  cases() / frames(name) / expected(name)  the named inputs, generated from fixed seeds, and what the reference makes of them

The ONLY place that knows anything about the kernels is the section "what the launches look like": the band, margin and thread
figures of launch_mask_chain (roft_amd/csrc/k_mask.hip) as named constants, used to check -- on the reference side -- that each
case reaches the branch it aims at (aim(name)).  The expected masks never depend on them.

`defect=` puts one named mistake into the reference (DEFECTS); the CPU test uses it to show that every mistake moves at least one
case's expected masks, i.e. that the table would notice it.
"""
import functools
from collections import namedtuple

import numpy as np

F32 = np.float32

# ---------------------------------------------------------------------------------------------
# flows
# ---------------------------------------------------------------------------------------------
# data: [H / grid, W / grid, 2] int16 or float32 (dx, dy); the step of a pixel is float32(raw) / float32(scale)
Flow = namedtuple("Flow", "data grid scale")
Fmt = namedtuple("Fmt", "kind grid scale")       # kind: "f32" | "s16"
F32_1_1 = Fmt("f32", 1, 1.0)                     # the reference's CV_32FC2 flow
S16_4_32 = Fmt("s16", 4, 32.0)                   # the reference's NVOF flow
STANDARD = (F32_1_1, S16_4_32)

DEFECTS = ("outside_window_dropped", "clear00_omitted", "clear00_in_mode2", "nan_as_zero", "floor", "newest_first",
           "smallest_wins", "reciprocal", "unmapped_zero", "first_flow_buffered", "buffer_kept_on_empty")


def encode(disp, fmt):
    """Displacements in pixels [rows, cols, 2] (float64) -> a Flow of the format."""
    raw = np.asarray(disp, np.float64) * fmt.scale
    if fmt.kind == "s16":
        return Flow(np.ascontiguousarray(np.clip(np.rint(raw), -32768, 32767).astype(np.int16)), fmt.grid, fmt.scale)
    return Flow(np.ascontiguousarray(raw.astype(F32)), fmt.grid, fmt.scale)


def _int_x86(x, defect=None):
    """(int)x of an x86-64 build (cvttss2si): truncation toward zero; NaN and |x| >= 2^31 give `outside` (the instruction
    answers INT_MIN, which fails every `< 0` test).  Returns (value as int64, outside)."""
    nan = np.isnan(x)
    if defect == "nan_as_zero":
        x = np.where(nan, F32(0), x)
        nan = np.zeros_like(nan)
    with np.errstate(invalid="ignore"):
        outside = nan | ~((x > F32(-2147483904.0)) & (x < F32(2147483648.0)))
    safe = np.where(outside, F32(0), x)
    v = (np.floor(safe) if defect == "floor" else np.trunc(safe)).astype(np.int64)
    return v, outside


def propagate(mask, flows, frames_between=6, defect=None, window=None, info=None):
    """out = remap(mask, map(flows)): every set pixel (!= 0), in row-major order, walks through the flows (oldest first, only
    the last frames_between of them when that number is > 0) in float32; a pixel that is outside the image before a flow, or
    after the last, is dropped; map[target] = source, the later (= largest) source wins; out = mask[map], unmapped targets
    sample mask(0, 0).
    window: only for the defect "outside_window_dropped" -- fn(source index, target index) -> inside.
    info: a dict that receives src / tgt (surviving sources and their targets), dropped_before (per flow: pixels found
    outside before it), and per flow the raw elements read and the position after the step (`reads`, `after`)."""
    mask = np.ascontiguousarray(mask, np.uint8)
    H, W = mask.shape
    flows = list(flows)
    if frames_between > 0:
        flows = flows[max(0, len(flows) - frames_between):]
    if defect == "newest_first":
        flows = flows[::-1]
    flat = mask.reshape(-1)
    src = np.flatnonzero(flat)
    tx = (src % W).astype(F32)
    ty = (src // W).astype(F32)
    alive = np.ones(src.size, bool)
    if info is not None:
        info.update(dropped_before=[], reads=[], after=[], alive=[])

    def inside(tx, ty):
        ix, ox = _int_x86(tx, defect)
        iy, oy = _int_x86(ty, defect)
        return ix, iy, ~ox & ~oy & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)

    with np.errstate(all="ignore"):
        for fl in flows:
            _, _, ok = inside(tx, ty)
            if info is not None:
                info["dropped_before"].append(int(np.count_nonzero(alive & ~ok)))
            alive &= ok
            g, s = F32(fl.grid), F32(fl.scale)
            if defect == "reciprocal":
                fr, _ = _int_x86(ty * (F32(1) / g))
                fc, _ = _int_x86(tx * (F32(1) / g))
            else:
                fr, _ = _int_x86(ty / g)
                fc, _ = _int_x86(tx / g)
            fr = np.where(alive, fr, 0)
            fc = np.where(alive, fc, 0)
            raw = fl.data[fr, fc].astype(F32)
            step = raw * (F32(1) / s) if defect == "reciprocal" else raw / s
            tx = np.where(alive, tx + step[:, 0], tx).astype(F32)
            ty = np.where(alive, ty + step[:, 1], ty).astype(F32)
            if info is not None:
                info["reads"].append(fl.data[fr[alive], fc[alive]])
                info["after"].append(np.stack([tx[alive], ty[alive]], 1))
                info["alive"].append(src[alive])
        ix, iy, ok = inside(tx, ty)
    alive &= ok
    s, t = src[alive], (iy[alive] * W + ix[alive])
    if defect == "outside_window_dropped" and window is not None and s.size:
        keep = window(s, t)
        s, t = s[keep], t[keep]
    if info is not None:
        info.update(src=s, tgt=t)
    m = np.zeros(H * W, np.int64)              # 0 = untouched = (0, 0), as the zero-initialised cv::Mat map
    if defect == "smallest_wins":
        big = np.full(H * W, H * W, np.int64)
        np.minimum.at(big, t, s)
        m = np.where(big == H * W, 0, big)
    else:
        np.maximum.at(m, t, s)
    out = flat[m]
    if defect == "unmapped_zero":
        touched = np.zeros(H * W, bool)
        touched[t] = True
        out = np.where(touched, out, 0).astype(np.uint8)
    return out.reshape(H, W)


def binarise(mask):
    return np.where(mask > 1, 255, 0).astype(np.uint8)


class Source:
    """ImageSegmentationOFAidedSource::step_frame without stamps.  step(mask or None, flow or None) -> the thresholded mask
    after the frame.  `log` gets one dict per frame: mode (0 nothing moved, 1 one step of the held mask, 2 a delivered mask
    through the buffered flows), n_flows, and for modes 1 and 2 what propagate() reports."""

    def __init__(self, frames_between, defect=None, window=None, keep_info=True):
        self.frames_between, self.defect, self.window, self.keep_info = frames_between, defect, window, keep_info
        self.mask = None
        self.buffer = []
        self.first_frame = True
        self.log = []

    def _propagate(self, mask, flows, fresh, rec):
        info = {} if self.keep_info else None
        win = (lambda s, t: self.window(s, t, fresh)) if self.window else None
        out = propagate(mask, flows, self.frames_between, self.defect, win, info)
        if info is not None:
            rec.update(info, in_mask=mask, in_flows=list(flows), out=out)
        return out

    def step(self, mask, flow):
        rec = dict(mode=0, n_flows=0, fresh=mask is not None)
        new = mask is not None
        if new and self.mask is None:
            self.mask = np.array(mask, np.uint8)          # the first mask is an initialisation: latched as it is
            new = False
        if new and not mask.any():
            new = False                                    # an empty mask is not informative
            if self.frames_between <= 0 and self.defect != "buffer_kept_on_empty":
                self.buffer = []
        has_flow = flow is not None and (not self.first_frame or self.defect == "first_flow_buffered")
        if has_flow:
            self.buffer.append(flow)
        if new:
            src = np.array(mask, np.uint8)
            if self.defect == "clear00_in_mode2":
                src[0, 0] = 0
            used = len(self.buffer) if self.frames_between <= 0 else min(len(self.buffer), self.frames_between)
            rec.update(mode=2, n_flows=used, src00=int(src[0, 0]), general=bool((src == 1).any()))
            self.mask = self._propagate(src, self.buffer, True, rec)
            self.buffer = []
        elif has_flow and self.mask is not None:
            src = self.mask.copy()
            rec.update(mode=1, n_flows=1, src00=int(src[0, 0]), general=bool((src == 1).any()))
            if self.defect != "clear00_omitted":
                src[0, 0] = 0
            self.mask = self._propagate(src, [flow], mask is not None, rec)
        self.first_frame = False
        self.log.append(rec)
        return None if self.mask is None else binarise(self.mask)     # (None: no mask yet -- an all-zero image downstream)


# ---------------------------------------------------------------------------------------------
# what the launches look like (launch_mask_chain in roft_amd/csrc/k_mask.hip): used by aim() only
# ---------------------------------------------------------------------------------------------
Launch = namedtuple("Launch", "band_rows margin threads")
ORDINARY = Launch(20, 16, 256)       # a frame that delivers no mask: kBandRows, kMargin, kFrameThreads
DELIVERING = Launch(6, 48, 128)      # a frame on which some object receives a mask: kBandRowsFresh, kMarginFresh, kFreshThreads
LDS_CAP = 160 * 1024 - 4096          # lds_cap; a workgroup's list and plane words take 12 bytes per thread of it
SINGLE_WALKS = 12                    # kSingleWalks: groups per wave whose flow loads are in flight together
MAX_FLOW_CHASE = 30                  # ROFT_MAX_FLOW_CHASE


class Bands:
    """The bands and LDS windows of one frame's launch: image W x H, `fresh` = a delivering frame, wgs =
    roft_config::mask_workgroups_per_object (0: automatic)."""

    def __init__(self, W, H, fresh, wgs=0):
        L = DELIVERING if fresh else ORDINARY
        self.W, self.H, self.L = W, H, L
        self.n_grp = W * H // 64
        self.per = -(-self.n_grp // wgs) if wgs > 0 else min(max(1, L.band_rows * W // 64), self.n_grp)
        self.wpr = W // 32
        cap = (min(H, (self.per * 64 + W - 1) // W + 1 + 2 * L.margin) * self.wpr + 1) & ~1
        self.win_cap = min(cap, ((LDS_CAP - L.threads * 12) // 4) & ~1)
        self.n_wg = -(-self.n_grp // self.per)
        q = np.arange(self.n_wg)
        g0 = q * self.per
        g1 = np.minimum(self.n_grp, g0 + self.per)
        r_lo = np.maximum(0, g0 * 64 // W - L.margin)
        r_hi = np.minimum(H - 1, (g1 * 64 - 1) // W + L.margin)
        self.off = r_lo * self.wpr
        self.words = np.minimum(self.win_cap, (r_hi - r_lo + 1) * self.wpr)
        self.capped_row = int((self.off[0] + self.words[0]) // self.wpr) if self.n_wg == 1 else None

    def in_window(self, src, tgt):
        q = (src // 64) // self.per
        wi = tgt // 32 - self.off[q]
        return (wi >= 0) & (wi < self.words[q])

    def lists(self, plane):
        """Per workgroup and chunk of `threads` groups: the number of non-empty 64-pixel groups of the source (bool [H*W])."""
        ne = plane.reshape(-1, 64).any(1)
        out = []
        for q in range(self.n_wg):
            g0, g1 = q * self.per, min(self.n_grp, (q + 1) * self.per)
            out.append([int(ne[c0:min(g1, c0 + self.L.threads)].sum()) for c0 in range(g0, g1, self.L.threads)])
        return out


def _window_fn(W, H, wgs):
    b = {False: Bands(W, H, False, wgs), True: Bands(W, H, True, wgs)}
    return lambda s, t, fresh: b[bool(fresh)].in_window(s, t)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
# build(case) -> frames[k][o] = (mask or None, Flow or None); over: engine settings (mask_frames_between,
# mask_workgroups_per_object); splits: batch sizes of the batched engine test; engine: False = the engine refuses the schedule
Case = namedtuple("Case", "name family W H fmt n_obj over splits build engine")

_CASES = {}


def _case(name, family, W, H, fmt, n_obj, build, over=None, splits=((4, 8, 2),), engine=True):
    assert W % 32 == 0 and (W * H) % 64 == 0 and W % fmt.grid == 0 and H % fmt.grid == 0
    assert name not in _CASES
    _CASES[name] = Case(name, family, W, H, fmt, n_obj, dict(over or {}), splits, build, engine)


def _fname(fmt):
    return "%s_g%d_s%g" % (fmt.kind, fmt.grid, fmt.scale)


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


def _blob(rng, W, H, fill=0.5, value=255):
    """A few random rectangles and discs covering about `fill` of the image."""
    m = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    while m.mean() < fill:
        cx, cy = rng.integers(0, W), rng.integers(0, H)
        rx, ry = rng.integers(W // 8, W // 2), rng.integers(H // 8, H // 2)
        if rng.random() < 0.5:
            m |= (abs(xx - cx) <= rx // 2) & (abs(yy - cy) <= ry // 2)
        else:
            m |= ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 0.25
    out = np.where(m, value, 0).astype(np.uint8)
    out[0, 0] = 0
    return out


def _three_valued(rng, W, H, fill=0.4, corner=0):
    """{0, 1, 255}: a blob of 255 with a rim and a sprinkle of 1s (a 1 is non-zero for the walk, background after the threshold)."""
    m = _blob(rng, W, H, fill)
    obj = m == 255
    rim = np.zeros_like(obj)
    rim[1:] |= obj[:-1]; rim[:-1] |= obj[1:]; rim[:, 1:] |= obj[:, :-1]; rim[:, :-1] |= obj[:, 1:]
    m[rim & ~obj] = 1
    m[(rng.random((H, W)) < 0.05)] = 1
    m[0, 0] = corner
    return m


def _tame(rng, W, H, fmt, amp=1.5):
    r, c = H // fmt.grid, W // fmt.grid
    return rng.uniform(-amp, amp, 2) + rng.uniform(-0.7, 0.7, (r, c, 2))


def _far(rng, W, H, fmt, share, reach):
    """Tame displacements with `share` of the elements thrown more than `reach` rows up or down, some of them and some others
    out of the left and right borders; a few far up / down enough to leave the image."""
    d = _tame(rng, W, H, fmt)
    r, c = d.shape[:2]
    far = rng.random((r, c)) < share
    n = int(far.sum())
    d[far, 1] = rng.choice([-1.0, 1.0], n) * rng.uniform(reach, max(reach + 8, H * 1.1), n)
    side = rng.random((r, c)) < share / 3
    n = int(side.sum())
    d[side, 0] = rng.choice([-1.0, 1.0], n) * rng.uniform(W * 0.3, W * 1.3, n)
    return d


def _schedule_frames(n_frames, n_obj, mask_at, flow_at, make_mask, make_flow):
    """frames[k][o]; mask_at[o] / flow_at[o]: sets of frames (flow_at None: every frame)."""
    out = []
    for k in range(n_frames):
        row = []
        for o in range(n_obj):
            m = make_mask(k, o) if k in mask_at[o] else None
            f = make_flow(k, o) if (flow_at is None or k in flow_at[o]) else None
            row.append((m, f))
        out.append(row)
    return out


# ---- far_targets ---------------------------------------------------------------------------------
def _build_far(c):
    rng = np.random.default_rng(_seed(c.name))
    reach = ORDINARY.band_rows + ORDINARY.margin + 2
    return _schedule_frames(8, c.n_obj, [{0, 3, 6}, {0, 4}], None,
                            lambda k, o: _blob(rng, c.W, c.H, 0.6),
                            lambda k, o: encode(_far(rng, c.W, c.H, c.fmt, 0.35, reach), c.fmt))


for _W, _H in ((64, 128), (96, 64)):
    for _f in STANDARD:
        _case("far_%dx%d_%s" % (_W, _H, _fname(_f)), "far_targets", _W, _H, _f, 2, _build_far)


# ---- poison ----------------------------------------------------------------------------------------
POISON_F32 = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "+1e10": 1e10, "-1e10": -1e10, "+3e9": 3e9, "-3e9": -3e9,
              "-0.0": -0.0}
POISON_S16 = {"+32767": 32767, "-32767": -32767, "-32768": -32768}
POISON_EDGES = ("neg_fraction", "edge_in", "edge_out")   # a step to (-1, 0): inside; to W - 1 + 0.9..: inside; to W: outside


def _poisoned(rng, c, base):
    """base displacements -> Flow with ~12 % of the elements replaced by poison, one or both components, and the three edge
    steps written for the first pixel of a few elements, in x and in y."""
    fl = encode(base, c.fmt)
    data = fl.data.copy()
    r, cc = data.shape[:2]
    table = POISON_S16 if c.fmt.kind == "s16" else POISON_F32
    vals = np.array(list(table.values()), data.dtype)
    hit = rng.random((r, cc)) < 0.12
    n = int(hit.sum())
    comp = rng.integers(0, 3, n)                     # 0: x, 1: y, 2: both
    v = vals[rng.integers(0, len(vals), (n, 2))]
    cur = data[hit]
    cur[comp != 1, 0] = v[comp != 1, 0]
    cur[comp != 0, 1] = v[comp != 0, 1]
    data[hit] = cur
    g, s = c.fmt.grid, c.fmt.scale
    frac_in = 31.0 / 32.0 if c.fmt.kind == "s16" else 0.99
    for kind in POISON_EDGES:
        for axis, size in ((0, c.W), (1, c.H)):
            for _ in range(12):
                er, ec = rng.integers(0, r), rng.integers(0, cc)
                p = (ec if axis == 0 else er) * g           # the element's first pixel along the axis
                to = {"neg_fraction": -0.5, "edge_in": size - 1 + frac_in, "edge_out": float(size)}[kind]
                data[er, ec, axis] = np.array((to - p) * s).astype(data.dtype)
                data[er, ec, 1 - axis] = 0
    return Flow(data, g, s)


def _build_poison(c):
    rng = np.random.default_rng(_seed(c.name))
    reach = ORDINARY.band_rows + ORDINARY.margin + 2
    return _schedule_frames(8, c.n_obj, [{0, 3, 6}, {0, 4}], None,
                            lambda k, o: _blob(rng, c.W, c.H, 0.7),
                            lambda k, o: _poisoned(rng, c, _far(rng, c.W, c.H, c.fmt, 0.1, reach)))


for _W, _H in ((64, 128), (96, 64)):
    for _f in STANDARD:
        _case("poison_%dx%d_%s" % (_W, _H, _fname(_f)), "poison", _W, _H, _f, 2, _build_poison)


# ---- corner ----------------------------------------------------------------------------------------
def _build_corner_fill(c):
    """frame 3 delivers a mask with (0,0) set that is chased through three flows: every target samples a set pixel.  Frame 4
    then walks a full plane (every group listed) with (0,0) cleared."""
    rng = np.random.default_rng(_seed(c.name))

    def mask(k, o):
        m = _blob(rng, c.W, c.H, 0.3 + 0.1 * o)
        m[0, 0] = 255 if k == 3 else 0
        return m
    return _schedule_frames(6, c.n_obj, [{0, 3}] * c.n_obj, None, mask, lambda k, o: encode(_tame(rng, c.W, c.H, c.fmt, 2.5), c.fmt))


def _build_corner_land(c):
    """frame 2: the pixels of a small square at (1..3, 1..3) step by (-1, -1): one lands on (0,0).  Frame 3 must drop it: its
    flow would carry (0,0) alone to (10 + o, 12)."""
    rng = np.random.default_rng(_seed(c.name))
    g = c.fmt.grid

    def mask(k, o):
        m = np.zeros((c.H, c.W), np.uint8)
        m[1:4, 1:4] = 255
        m[c.H // 2:c.H // 2 + 8 + o, c.W // 2:c.W // 2 + 9] = 255
        return m

    def flow(k, o):
        d = _tame(rng, c.W, c.H, c.fmt, 0.4) * 0.0 + rng.uniform(-0.2, 0.2, 2)
        if k == 1:
            d[:] = 0.0
        if k == 2:
            d[0:(8 // g), 0:(8 // g)] = (-1.0, -1.0)
        if k == 3:
            d[0:(8 // g), 0:(8 // g)] = (10.0 + o, 12.0)
        return encode(d, c.fmt)
    return _schedule_frames(5, c.n_obj, [{0}] * c.n_obj, None, mask, flow)


def _build_corner_bg_one(c):
    """frame 3 delivers a {0, 1, 255} mask with mask(0,0) == 1: the background of the propagated mask is 1 -- non-zero for the
    next walks, clear after the threshold."""
    rng = np.random.default_rng(_seed(c.name))
    return _schedule_frames(7, c.n_obj, [{0, 3}] * c.n_obj, None,
                            lambda k, o: _three_valued(rng, c.W, c.H, 0.3, corner=1) if k == 3 else _blob(rng, c.W, c.H, 0.4),
                            lambda k, o: encode(_far(rng, c.W, c.H, c.fmt, 0.1, 30), c.fmt))


for _n, _b, _g in (("fill", _build_corner_fill, ((64, 128, F32_1_1), (96, 64, S16_4_32))),
                   ("land", _build_corner_land, ((96, 64, F32_1_1), (64, 128, S16_4_32))),
                   ("bg_one", _build_corner_bg_one, ((64, 128, S16_4_32), (96, 64, F32_1_1)))):
    for _W, _H, _f in _g:
        _case("corner_%s_%dx%d_%s" % (_n, _W, _H, _fname(_f)), "corner", _W, _H, _f, 2, _b)


# ---- dense_rounds ------------------------------------------------------------------------------------
def _build_dense(c):
    """Full planes (first mask: all of it; the delivered one without (0,0), which would fill instead of walking) and tame flows."""
    rng = np.random.default_rng(_seed(c.name))

    def mask(k, o):
        m = np.full((c.H, c.W), 255, np.uint8)
        if k > 0:
            m[0, 0] = 0
            m[rng.integers(0, c.H, 9 + o), rng.integers(0, c.W, 9 + o)] = 0
        return m
    return _schedule_frames(6, c.n_obj, [{0, 3}] * c.n_obj, None, mask, lambda k, o: encode(_tame(rng, c.W, c.H, c.fmt, 0.8), c.fmt))


for _f in STANDARD:
    _case("dense_256x96_%s" % _fname(_f), "dense_rounds", 256, 96, _f, 2, _build_dense)
    _case("dense_128x192_one_wg_%s" % _fname(_f), "dense_rounds", 128, 192, _f, 2, _build_dense,
          over=dict(mask_workgroups_per_object=1))


# ---- formats -----------------------------------------------------------------------------------------
def _lattice(rng, c, d):
    """Whole-pixel steps into the first columns, in the left quarter of the image: float32(raw) / scale is exact there while
    raw * (1 / scale) is not at a scale that is no power of two."""
    r, cc = d.shape[:2]
    cols = np.arange(cc // 4) * c.fmt.grid
    to = rng.integers(1, 7, (r, cc // 4))
    d[:, :cc // 4, 0] = to - cols[None, :]
    d[:, :cc // 4, 1] = rng.integers(-2, 3, (r, cc // 4))
    return d


def _build_formats(c):
    rng = np.random.default_rng(_seed(c.name))

    def flow(k, o):
        d = _far(rng, c.W, c.H, c.fmt, 0.1, 30)
        if c.fmt.scale not in (1.0, 32.0, 0.5) and k % 2 == 1:
            d = _lattice(rng, c, d)
        return _poisoned(rng, c, d) if k in (2, 5) else encode(d, c.fmt)
    return _schedule_frames(8, c.n_obj, [{0, 4}, {0, 3, 7}], None, lambda k, o: _blob(rng, c.W, c.H, 0.6), flow)


for _W, _H, _f in ((64, 128, Fmt("f32", 4, 32.0)), (96, 64, Fmt("s16", 1, 1.0)), (64, 128, Fmt("f32", 8, 1.0)),
                   (96, 64, Fmt("f32", 1, 0.5)),                                                       # MODE 1
                   (160, 120, Fmt("f32", 5, 1.0)), (160, 120, Fmt("s16", 5, 32.0)), (64, 128, Fmt("s16", 4, 20.0)),
                   (96, 64, Fmt("f32", 1, 3.0))):                                                      # MODE 0
    _case("formats_%dx%d_%s" % (_W, _H, _fname(_f)), "formats", _W, _H, _f, 2, _build_formats)


def format_mode(fmt):
    """2: grid 1 and scale 1; 1: both powers of two; 0: true divisions (ChaseGeo::mode)."""
    p2 = lambda v: v > 0 and float(np.frexp(v)[0]) == 0.5
    if fmt.grid & (fmt.grid - 1) or not p2(fmt.scale):
        return 0
    return 2 if (fmt.grid == 1 and fmt.scale == 1.0) else 1


# ---- three_valued ------------------------------------------------------------------------------------
def _build_three(c):
    """Object 0: binary first mask, a {0,1,255} mask on frame 3, binary again on frame 13: frames 3 .. 12 are general, which
    with batches of (4, 8, 2) puts one on t = T-1 (frame 3), t = 0 (4), T-2 (10) and T-1 (11), with (5, 2, 7) on T-2 (3, 5).
    Object 1: a three-valued FIRST mask, binary on 6, three-valued on 10.  Object 2 stays binary."""
    rng = np.random.default_rng(_seed(c.name))
    tv = [{3}, {0, 10}, set()]
    reach = ORDINARY.band_rows + ORDINARY.margin + 2
    return _schedule_frames(15, c.n_obj, [{0, 3, 13}, {0, 6, 10}, {0, 7}], None,
                            lambda k, o: _three_valued(rng, c.W, c.H, 0.45) if k in tv[o] else _blob(rng, c.W, c.H, 0.5),
                            lambda k, o: _poisoned(rng, c, _far(rng, c.W, c.H, c.fmt, 0.15, reach)) if k % 2 else
                            encode(_far(rng, c.W, c.H, c.fmt, 0.15, reach), c.fmt))


for _W, _H, _f in ((64, 128, F32_1_1), (96, 64, S16_4_32)):
    _case("three_valued_%dx%d_%s" % (_W, _H, _fname(_f)), "three_valued", _W, _H, _f, 3, _build_three,
          splits=((4, 8, 2), (5, 2, 7)))


# ---- schedule ----------------------------------------------------------------------------------------
def _build_schedule(mask_at, flow_at, n_frames, empty_at=()):
    def build(c):
        rng = np.random.default_rng(_seed(c.name))

        def mask(k, o):
            if (k, o) in empty_at or (k, None) in empty_at:
                return np.zeros((c.H, c.W), np.uint8)
            return _blob(rng, c.W, c.H, 0.35)
        return _schedule_frames(n_frames, c.n_obj, mask_at, flow_at, mask, lambda k, o: encode(_tame(rng, c.W, c.H, c.fmt, 2.0), c.fmt))
    return build


_ALL = lambda n: set(range(n))
for _f in STANDARD:
    _s = _fname(_f)
    # the engine refuses a stream whose first frame brings no mask (ROFT_ERR_STATE): reference and oracle only
    _case("schedule_no_mask_first_" + _s, "schedule", 64, 64, _f, 2,
          _build_schedule([{3, 7}, {2}], None, 10), engine=False)
    _case("schedule_consecutive_masks_" + _s, "schedule", 64, 64, _f, 2,
          _build_schedule([{0, 1, 2, 3, 7, 8}, {0, 4, 5}], None, 11))
    # deliveries on frames without a flow: 2 right after a delivery (no buffered flow: mode 2 through none), 6 with 3, 4, 5 buffered
    _case("schedule_delivery_without_flow_" + _s, "schedule", 64, 64, _f, 2,
          _build_schedule([{0, 1, 2, 6}, {0, 5}], [_ALL(10) - {2, 6}, _ALL(10) - {5, 7}], 10))
    _case("schedule_missing_flows_" + _s, "schedule", 64, 64, _f, 2,
          _build_schedule([{0, 9}, {0, 5}], [{1, 2, 6, 7, 9, 10}, {0, 4, 8, 10, 11}], 12))
    for _fb in (6, 0, -1):
        _case("schedule_empty_delivery_fb%d_%s" % (_fb, _s), "schedule", 64, 64, _f, 2,
              _build_schedule([{0, 4, 7}, {0, 3, 5, 9}], None, 11, empty_at={(4, 0), (5, 1)}),
              over=dict(mask_frames_between=_fb))
    _case("schedule_8_buffered_fb0_" + _s, "schedule", 64, 64, _f, 2,
          _build_schedule([{0, 8}, {0, 9}], None, 11), over=dict(mask_frames_between=0))
    _case("schedule_%d_buffered_fb0_%s" % (MAX_FLOW_CHASE, _s), "schedule", 64, 64, _f, 1,
          _build_schedule([{0, MAX_FLOW_CHASE}], None, MAX_FLOW_CHASE + 2), over=dict(mask_frames_between=0))


# ---- capped_window -----------------------------------------------------------------------------------
def _build_capped(c):
    """One workgroup walks the whole 1024 x 1280 plane; its LDS window cannot hold the last rows.  A slab above them moves
    down by 20 .. 200 rows, a slab inside them moves about: targets on both sides of the capped row."""
    rng = np.random.default_rng(_seed(c.name))
    W, H = c.W, c.H

    def mask(k, o):
        m = np.zeros((H, W), np.uint8)
        m[H - 260:H - 90, 100 + 64 * k:700 + 64 * k] = 255
        m[H - 40:H - 8, 300:900] = 255
        m[40:90, 500:560] = 255
        m[rng.random((H, W)) < 0.0005] = 255
        m[0, 0] = 0
        return m

    def flow(k, o):
        d = _tame(rng, W, H, c.fmt, 1.0)
        r = d.shape[0]
        d[:, :, 1] += np.where(rng.random(d.shape[:2]) < 0.5, rng.uniform(20, 200, d.shape[:2]), 0.0)
        d[:r // 8, :, 1] = rng.uniform(-3, 3, (r // 8, d.shape[1]))
        return encode(d, c.fmt)
    return _schedule_frames(4, 1, [{0, 2}], None, mask, flow)


_case("capped_window_1024x1280_" + _fname(F32_1_1), "capped_window", 1024, 1280, F32_1_1, 1, _build_capped,
      over=dict(mask_workgroups_per_object=1), splits=((4,),))


def cases():
    return _CASES


# the rest of a tracker kept idle: all-zero depth (no flow point, the twist belief stays), a pose on frame 0 only, a small cube
POSE0 = ((0.0, 0.0, 0.6), (1.0, 0.0, 0.0, 0.0))


def small_mesh():
    verts = np.array([[x, y, z] for x in (-0.03, 0.03) for y in (-0.03, 0.03) for z in (-0.03, 0.03)], np.float32)
    tris = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                     [1, 5, 7], [1, 7, 3]], np.int32)
    return verts, tris


def frames_between(c):
    return c.over.get("mask_frames_between", 6)


@functools.lru_cache(maxsize=None)
def frames(name):
    """frames[k][o] = (mask or None, Flow or None): the bytes every test of the case sees."""
    c = _CASES[name]
    fr = c.build(c)
    for row in fr:
        for m, f in row:
            if m is not None:
                m.setflags(write=False)
            if f is not None:
                f.data.setflags(write=False)
    return fr


def run(name, defect=None, keep_info=False):
    """The reference over the case: (masks[k][o], logs[o])."""
    c = _CASES[name]
    win = _window_fn(c.W, c.H, c.over.get("mask_workgroups_per_object", 0)) if defect == "outside_window_dropped" else None
    srcs = [Source(frames_between(c), defect, win, keep_info) for _ in range(c.n_obj)]
    masks = [[srcs[o].step(*row[o]) for o in range(c.n_obj)] for row in frames(name)]
    return masks, [s.log for s in srcs]


@functools.lru_cache(maxsize=None)
def expected(name):
    masks, _ = run(name)
    for row in masks:
        for m in row:
            if m is not None:
                m.setflags(write=False)
    return masks


# ---------------------------------------------------------------------------------------------
# aim: does the case reach the branch it is there for?  (reference walk + the launch constants above)
# ---------------------------------------------------------------------------------------------
def aim(name):
    """Figures of the case, over all frames and objects whose source is binary (a three-valued source takes the map kernel:
    one workgroup, no window): pixels that survive and land outside / inside their band's LDS window on ordinary and on
    delivering frames, the largest number of listed groups per wave and of chunks per workgroup, (0,0) events, poison kinds
    read under live pixels, pixels dropped in the middle of a chase."""
    c = _CASES[name]
    wgs = c.over.get("mask_workgroups_per_object", 0)
    fr = frames(name)
    _, logs = run(name, keep_info=True)
    bands = {False: Bands(c.W, c.H, False, wgs), True: Bands(c.W, c.H, True, wgs)}
    a = dict(outside=0, inside=0, outside_delivering=0, inside_delivering=0, groups_per_wave=0, rounds=0, chunks=0,
             groups_listed=0, fill_frames=[], clear00_frames=[], bg_one_frames=[], kinds=set(), mid_chase_drops=0,
             general_frames=[], modes=[], capped_row=bands[False].capped_row)
    for k, row in enumerate(fr):
        fresh = any(m is not None for m, _ in row)       # the launch is the delivering one when ANY object receives a mask
        b = bands[fresh]
        for o in range(c.n_obj):
            rec = logs[o][k]
            a["modes"].append((k, o, rec["mode"], rec["n_flows"]))
            if rec["mode"] == 0:
                continue
            if rec["general"]:
                a["general_frames"].append((k, o))
                if rec["mode"] == 2 and rec["src00"] == 1:
                    a["bg_one_frames"].append((k, o))
            elif rec["mode"] == 2 and rec["src00"]:
                a["fill_frames"].append((k, o))
            else:
                inw = b.in_window(rec["src"], rec["tgt"]) if rec["src"].size else np.zeros(0, bool)
                key = "_delivering" if fresh else ""
                a["outside" + key] += int((~inw).sum())
                a["inside" + key] += int(inw.sum())
                plane = np.zeros(c.W * c.H, bool)
                plane[rec["alive"][0] if rec["alive"] else rec["src"]] = True     # the set pixels of the source
                waves = b.L.threads // 64
                for chunks in b.lists(plane):
                    a["chunks"] = max(a["chunks"], len(chunks))
                    for n in chunks:
                        a["groups_listed"] = max(a["groups_listed"], n)
                        per_wave = -(-n // waves)
                        a["groups_per_wave"] = max(a["groups_per_wave"], per_wave)
                        if rec["n_flows"] == 1:
                            a["rounds"] = max(a["rounds"], -(-per_wave // SINGLE_WALKS))
            if rec["mode"] == 1 and rec["src00"]:
                a["clear00_frames"].append((k, o))
            if rec["mode"] == 2 and rec["n_flows"] > 2:
                a["mid_chase_drops"] += sum(rec["dropped_before"][1:])
            for raw, after in zip(rec["reads"], rec["after"]):
                a["kinds"] |= _kinds(c, raw, after)
    return a


def _kinds(c, raw, after):
    out = set()
    if c.fmt.kind == "s16":
        for k, v in POISON_S16.items():
            if (raw == v).any():
                out.add(k)
    else:
        for k, v in POISON_F32.items():
            if k == "nan":
                hit = np.isnan(raw)
            elif k == "-0.0":
                hit = (raw == 0) & np.signbit(raw)
            else:
                hit = raw == F32(v)
            if hit.any():
                out.add(k)
    for axis, size in ((0, c.W), (1, c.H)):
        t = after[:, axis]
        with np.errstate(invalid="ignore"):
            if ((t > -1) & (t < 0)).any():
                out.add("neg_fraction")
            if ((t > size - 1 + 0.9) & (t < size)).any():
                out.add("edge_in")
            if (t == size).any():
                out.add("edge_out")
    return out


def poison_kinds(fmt):
    return set(POISON_S16 if fmt.kind == "s16" else POISON_F32) | set(POISON_EDGES)

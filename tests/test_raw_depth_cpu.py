"""Raw sensor depth without a device (include/roft_engine.h section 3c): the ABI version and roft_frame_input are unchanged, the stand-alone
operators refuse bad arguments before they look for a device -- and the numpy restatement the GPU tests compare against
(tests/depth_ref.py) has the properties the contract promises, on inputs that take every one of its branches.  Last: 16-bit gray
PNGs, the form YCB-Video and HO-3D ship depth in."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header
from roft_amd import _lib as L
from roft_amd import io

import depth_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_structs_and_constants():
    """(calls, structs and the constants' values: tests/test_abi_cpu.py, for every name of the header)"""
    assert L.DEPTH_ALIGN_MAX_SPAN == D.MAX_SPAN, "the numpy restatement clips footprints where the contract does"


def test_abi_version_and_frame_input_are_unchanged():
    code = abi_header.code()
    assert re.search(r"#define\s+ROFT_ABI_VERSION\s+2\b", code)
    assert L.ABI_VERSION == 2 and L.lib().roft_abi_version() == 2
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*roft_frame_input\s*;", code)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*;", m.group(1)) == ["dt", "depth", "flow", "mask", "pose_valid", "pose_x", "pose_q", "mem_kind", "stamp",
                                                                 "mask_stamp"] == [f for f, _ in L.FrameInput._fields_]
    assert not re.search(r"\bint\s+roft_frames_submit_\w*depth", code), "no new submit call: the raw frame travels in inputs[].depth"


def _source(**over):
    src = L.DepthSource()
    src.type, src.scale, src.align = L.DEPTH_Z16, 0.001, 1
    src.cam = L.Camera(8, 4, 30.0, 30.0, 3.5, 1.5)
    src.R = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    for k, v in over.items():
        setattr(src, k, v)
    return src


def test_operators_refuse_bad_arguments_before_they_need_a_device():
    lib = L.lib()
    raw = np.ones((4, 8), np.uint16)
    out = np.zeros((4, 8), np.float32)
    rp, op = raw.ctypes.data, out.ctypes.data
    for args in ((None, 8, 4, 0.001, op), (rp, 8, 4, 0.001, None), (rp, 0, 4, 0.001, op), (rp, 8, -1, 0.001, op), (rp, 8, 4, 0.0, op),
                 (rp, 8, 4, -0.001, op), (rp, 8, 4, float("nan"), op), (rp, 8, 4, float("inf"), op)):
        assert lib.roft_depth_convert(*args) == -1, args          # ROFT_ERR_INVALID
        assert lib.roft_last_error_string()
    col = L.Camera(8, 4, 30.0, 30.0, 3.5, 1.5)
    nan_R = (C.c_float * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)
    inf_t = (C.c_float * 3)(0, float("inf"), 0)
    bad_sources = [_source(type=0), _source(type=2), _source(scale=0.0), _source(scale=float("nan")), _source(R=nan_R), _source(t=inf_t),
                   _source(cam=L.Camera(8, 4, 0.0, 30.0, 3.5, 1.5)), _source(cam=L.Camera(8, 4, 30.0, float("inf"), 3.5, 1.5)),
                   _source(cam=L.Camera(8, 4, -30.0, 30.0, 3.5, 1.5)), _source(cam=L.Camera(0, 4, 30.0, 30.0, 3.5, 1.5)),
                   _source(cam=L.Camera(4096, 4096, 30.0, 30.0, 3.5, 1.5))]
    for i, src in enumerate(bad_sources):
        assert lib.roft_depth_align(rp, C.byref(src), C.byref(col), op) == -1, i
        assert lib.roft_last_error_string()
    good = _source()
    for colour in (L.Camera(8, 4, 0.0, 30.0, 3.5, 1.5), L.Camera(8, 0, 30.0, 30.0, 3.5, 1.5), L.Camera(4096, 4096, 30.0, 30.0, 3.5, 1.5)):
        assert lib.roft_depth_align(rp, C.byref(good), C.byref(colour), op) == -1
    assert lib.roft_depth_align(None, C.byref(good), C.byref(col), op) == -1
    assert lib.roft_depth_align(rp, None, C.byref(col), op) == -1
    assert lib.roft_depth_align(rp, C.byref(good), None, op) == -1
    assert lib.roft_depth_align(rp, C.byref(good), C.byref(col), None) == -1
    # the engine calls refuse a null engine without touching a device
    st = L.EngineDepthStats()
    ms = C.c_double(0.0)
    assert lib.roft_engine_enable_raw_depth(None, C.byref(good)) == -1
    assert lib.roft_engine_get_depth(None, 0, op) == -1
    assert lib.roft_engine_get_depth_stats(None, C.byref(st)) == -1
    assert lib.roft_debug_depth_kernel_ms(None, C.byref(ms)) == -1
    if lib.roft_device_count() <= 0:
        assert lib.roft_depth_convert(rp, 8, 4, 0.001, op) == -2             # ROFT_ERR_DEVICE: there is no CPU path
        assert lib.roft_depth_align(rp, C.byref(good), C.byref(col), op) == -2


# ---- the restatement's own properties -------------------------------------------------------------------------------------------
def test_convert_is_one_float_multiply():
    raw = np.array([[0, 1, 65535, 1000]], np.uint16)
    for scale in (0.001, 0.00012498664727900177):
        got = D.convert(raw, scale)
        assert got.dtype == np.float32 and got[0, 0] == 0.0
        assert np.array_equal(got, np.array([[np.float32(v) * np.float32(scale) for v in (0, 1, 65535, 1000)]], np.float32))


@pytest.mark.parametrize("shape", [(37, 5), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_identity_equals_convert(shape):
    case = D.identity_case(*shape)
    counts = {}
    assert np.array_equal(D.run(case, counts), D.convert(case["raw"], case["scale"]))
    assert counts["multiply"] == 0


def test_times_two_replicates_every_reading_into_a_2x2_block():
    case = D.times_two_case()
    counts = {}
    out = D.run(case, counts)
    want = D.convert(case["raw"], case["scale"])
    assert np.array_equal(out[1:49, 1:65], np.repeat(np.repeat(want, 2, 0), 2, 1))
    assert counts["multiply"] == 0 and np.all(counts["cover"][1:49, 1:65] == 1)          # no overlaps, no holes
    assert counts["uncovered"] == 2 * 66 + 2 * 48 and not out[0].any() and not out[:, 0].any() and not out[-1].any() and not out[:, -1].any()


def test_a_nearer_reading_wins_a_collision():
    # two readings whose footprints land on the same colour pixels: a far one straight ahead and a near one that the baseline
    # shifts onto it (fx t_x / z = 40 * 0.05 / 0.5 = 4 pixels against 40 * 0.05 / 2.0 = 1)
    cam = D.Cam(16, 3, 40.0, 40.0, 7.5, 1.0)
    raw = np.zeros((3, 16), np.uint16)
    raw[1, 8], raw[1, 5] = 2000, 500
    counts = {}
    out = D.align(raw, 0.001, cam, cam, np.eye(3), (0.05, 0.0, 0.0), counts)
    assert counts["multiply"] == 1
    hit = np.argwhere(counts["cover"] == 2)[0]
    assert out[tuple(hit)] == np.float32(500) * np.float32(0.001)
    # ... and alone, the far reading lands on that very pixel
    raw[1, 5] = 0
    assert D.align(raw, 0.001, cam, cam, np.eye(3), (0.05, 0.0, 0.0))[tuple(hit)] == np.float32(2000) * np.float32(0.001)


def test_the_cases_take_every_branch_of_the_contract():
    case = D.general_case()
    assert {0, 1, 65535} <= set(np.unique(case["raw"]).tolist())
    counts = {}
    out = D.run(case, counts)
    assert counts["multiply"] > 0 and counts["uncovered"] > 0 and counts["offscreen"] > 0
    assert out.dtype == np.float32 and np.count_nonzero(out) > out.size // 2
    counts = {}
    D.run(D.general_case(t=(0.015, 0.002, -1.0)), counts)
    assert counts["behind"] > 0
    counts = {}
    D.run(D.general_case(f_colour=60 * 40.0), counts)
    assert counts["capped"] > 0


# ---- 16-bit PNG -----------------------------------------------------------------------------------------------------------------
def test_png16_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 65536, (7, 13), dtype=np.uint16)
    img[0, :4] = [0, 1, 255, 65535]
    path = str(tmp_path / "d.png")
    io.write_png(path, img)
    data = open(path, "rb").read()
    assert data[24] == 16 and data[25] == 0, "bit depth 16, colour type 0 (gray) in the IHDR chunk"
    back = io.read_png(path)
    assert back.dtype == np.uint16 and np.array_equal(back, img)
    # 8-bit images are what they were
    g8 = rng.integers(0, 256, (5, 6), dtype=np.uint8)
    io.write_png(path, g8)
    back = io.read_png(path)
    assert back.dtype == np.uint8 and np.array_equal(back, g8)


def test_png16_samples_are_big_endian(tmp_path):
    import zlib
    path = str(tmp_path / "d.png")
    io.write_png(path, np.array([[0x1234, 0x00ff]], np.uint16))
    data = open(path, "rb").read()
    i = data.index(b"IDAT")
    n = int.from_bytes(data[i - 4:i], "big")
    assert zlib.decompress(data[i + 4:i + 4 + n]) == bytes([0, 0x12, 0x34, 0x00, 0xff])    # filter 0, then the samples high byte first

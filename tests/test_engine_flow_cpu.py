"""Camera images on the engine without a device: the existing structs and the ABI version are unchanged, the ctypes mirrors have
the structs' sizes, and roft_image_to_gray refuses bad arguments before it looks for a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import abi_header
from roft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_existing_structs_and_the_abi_version_are_unchanged():
    code = abi_header.code()
    assert re.search(r"#define\s+ROFT_ABI_VERSION\s+2\b", code), "no existing struct changed: the ABI version stays"
    assert L.ABI_VERSION == 2 and L.lib().roft_abi_version() == 2
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*roft_frame_input\s*;", code)
    assert re.findall(r"(\w+)(?:\[\d+\])?\s*;", m.group(1)) == [f for f, _ in L.FrameInput._fields_]
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*roft_engine_stats\s*;", code)
    assert re.findall(r"(\w+)\s*;", m.group(1)) == [f for f, _ in L.EngineStats._fields_]


def test_struct_sizes_match_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "roft_engine.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(roft_frame_image), offsetof(roft_frame_image, image_type), sizeof(roft_engine_flow_stats), '
           'offsetof(roft_engine_flow_stats, pairs), sizeof(roft_frame_input), sizeof(roft_config), sizeof(roft_engine_stats), '
           'sizeof(roft_of_params));return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got == [C.sizeof(L.FrameImage), L.FrameImage.image_type.offset, C.sizeof(L.EngineFlowStats), L.EngineFlowStats.pairs.offset,
                   C.sizeof(L.FrameInput), C.sizeof(L.Config), C.sizeof(L.EngineStats), C.sizeof(L.OFParams)]


def test_image_to_gray_refuses_bad_arguments_before_it_needs_a_device():
    lib = L.lib()
    img = np.zeros((4, 4, 3), np.uint8)
    out = np.zeros((4, 4), np.uint8)
    for itype, W, H, src, dst in ((0, 4, 4, img, out), (4, 4, 4, img, out), (L.IMAGE_RGB8, 0, 4, img, out), (L.IMAGE_RGB8, 4, 0, img, out),
                                  (L.IMAGE_GRAY8, -1, 4, img, out), (L.IMAGE_RGB8, 4, 4, None, out), (L.IMAGE_RGB8, 4, 4, img, None)):
        rc = lib.roft_image_to_gray(None if src is None else src.ctypes.data, itype, W, H, None if dst is None else dst.ctypes.data)
        assert rc == -1, (itype, W, H)           # ROFT_ERR_INVALID
        assert lib.roft_last_error_string()
    if lib.roft_device_count() <= 0:
        assert lib.roft_image_to_gray(img.ctypes.data, L.IMAGE_RGB8, 4, 4, out.ctypes.data) == -2   # ROFT_ERR_DEVICE: no CPU path
        # ... and the engine-side calls refuse a null engine without touching a device
        assert lib.roft_engine_enable_flow(None, None) == -1
        assert lib.roft_engine_get_flow_stats(None, None) == -1

"""Label-image masks without a device: the ABI version is unchanged, the ctypes mirror has the struct's size, what
roft_labels_to_masks refuses needs no device, and io.labels_from_instances turns the scene renderer's instance
map into a label image."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_header
from roft_amd import _lib as L
from roft_amd import io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_is_still_two():
    assert re.search(r"#define\s+ROFT_ABI_VERSION\s+2\b", abi_header.code()), "no existing struct changed: the ABI version stays"
    assert L.ABI_VERSION == 2 and L.lib().roft_abi_version() == 2


def test_struct_size_matches_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "roft_engine.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(roft_label_mask), '
           'offsetof(roft_label_mask, labels), offsetof(roft_label_mask, label_type), offsetof(roft_label_mask, label), sizeof(roft_frame_input));return 0;}')
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert got == [C.sizeof(L.LabelMask), L.LabelMask.labels.offset, L.LabelMask.label_type.offset, L.LabelMask.label.offset, C.sizeof(L.FrameInput)]


def test_argument_refusals_need_no_device():
    """What roft_labels_to_masks refuses is refused before the device is looked for."""
    lib = L.lib()
    lab = np.zeros((64, 64), np.uint8)
    ip = C.POINTER(C.c_int)
    for ltype, vals in ((L.LABEL_U8, [0]), (L.LABEL_U8, [256]), (L.LABEL_U8, [-1]), (L.LABEL_U16, [65536]), (3, [1]), (0, [1])):
        v = np.array(vals, np.int32)
        assert lib.roft_labels_to_masks(lab.ctypes.data, ltype, 64, 64, v.ctypes.data_as(ip), len(v), None, None) == -1, (ltype, vals)
        assert lib.roft_last_error_string()
    assert lib.roft_labels_to_masks(None, L.LABEL_U8, 64, 64, None, 1, None, None) == -1


def test_labels_from_instances():
    inst = np.array([[-1, -1, 0, 0], [1, 1, 0, -1], [2, -1, -1, 254]], np.int32)
    lab = io.labels_from_instances(inst)
    assert lab.dtype == np.uint8 and lab.shape == inst.shape
    assert np.array_equal(lab, np.array([[0, 0, 1, 1], [2, 2, 1, 0], [3, 0, 0, 255]], np.uint8))
    for i in (0, 1, 2, 254):
        assert np.array_equal(lab == i + 1, inst == i)
    wide = inst.copy()
    wide[0, 0] = 255    # value 256 does not fit a byte
    lab16 = io.labels_from_instances(wide)
    assert lab16.dtype == np.uint16 and lab16[0, 0] == 256 and np.array_equal(lab16[1:], lab[1:].astype(np.uint16))
    assert io.labels_from_instances(np.full((2, 2), -1, np.int32)).max() == 0
    with pytest.raises(ValueError):
        io.labels_from_instances(np.array([[-2]], np.int32))
    with pytest.raises(ValueError):
        io.labels_from_instances(np.array([[65535]], np.int32))

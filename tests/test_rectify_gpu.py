"""Lens distortion on the GPU (include/roft_engine.h section 3g): the stand-alone operators roft_rectify_map and roft_rectify
against the numpy restatement tests/rectify_ref.py, for EQUAL bits -- every kind, targets whose width is and is not a multiple of
the four pixels a thread owns (64 x 48: whole words; 61 x 47, 3 x 5, 1 x 1: the tail path), sources larger and smaller than the
target, the identity, and a lens whose map is not finite."""
import numpy as np
import pytest

import rectify_ref as R
from roft_amd import ops

pytestmark = pytest.mark.gpu

SHAPES = [(64, 48), (61, 47), (3, 5), (1, 1)]
KINDS = (R.GRAY8, R.RGB8, R.U8, R.U16, R.F32)


def sources(tgt):
    """{name: the lens} for one target"""
    return {"A-pincushion": R.lens(R.SOURCE_A, R.PINCUSHION), "B-barrel": R.lens(R.SOURCE_B, R.BARREL), "identity": R.lens(tgt),
            "nonfinite": R.lens(R.SOURCE_A, R.NONFINITE)}


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def same_map(got, want):
    """equal bits wherever the value is a number; a NaN where the restatement has one (its sign and payload are the host's or the
    device's own)"""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("source", ["A-pincushion", "B-barrel", "identity", "nonfinite"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_operators_equal_the_restatement(shape, source):
    tgt = R.target(*shape)
    ln = sources(tgt)[source]
    sx, sy = R.rect_map(ln, tgt)
    same_map(ops.rectify_map(ln, tgt), np.stack([sx, sy], axis=2))
    for kind in KINDS:
        img = R.image(ln.cam, kind, seed=shape[0])
        want = R.rectify(img, kind, ln, tgt)
        same_bits(ops.rectify(img, ln, tgt, kind=kind), want)
    if source == "identity":
        assert np.array_equal(ops.rectify(img, ln, tgt), img)


def test_a_nan_in_the_map_gives_zero():
    """a principal point on a pixel centre: x = 0 on a column, 0 * inf"""
    tgt = R.TARGET._replace(cx=32.0, cy=24.0)
    ln = R.lens(R.SOURCE_A, R.NONFINITE)
    sx, sy = R.rect_map(ln, tgt)
    assert np.isnan(sx).any()
    same_map(ops.rectify_map(ln, tgt), np.stack([sx, sy], axis=2))
    for kind in KINDS:
        img = np.maximum(R.image(ln.cam, kind), 1)
        got = ops.rectify(img, ln, tgt, kind=kind)
        same_bits(got, R.rectify(img, kind, ln, tgt))
        assert not got[np.isnan(sx) | np.isnan(sy)].any()


def test_kind_follows_the_dtype_and_the_outside_is_zero():
    ln = R.lens(R.SOURCE_B, R.BARREL)
    depth = np.maximum(R.image(R.SOURCE_B, R.F32), 0.5)
    got = ops.rectify(depth, ln, R.TARGET)
    same_bits(got, R.nearest(depth, ln, R.TARGET))
    assert 0.2 < np.count_nonzero(got == 0) / got.size < 0.6
    mask = R.image(R.SOURCE_B, R.U8)
    same_bits(ops.rectify(mask, ln, R.TARGET, nearest=True), R.nearest(mask, ln, R.TARGET))
    same_bits(ops.rectify(mask, ln, R.TARGET), R.bilinear(mask, ln, R.TARGET))

"""roft_amd.engine.fill_frame / assemble_batch: the frame dicts of ROFTFilterBatch.submit -> the ctypes arrays of the C ABI.  ctypes
and numpy only: no engine, no device."""
import ctypes as C

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import engine as E

H, W = 6, 8


def arrays(n):
    return (L.FrameInput * n)(), (L.LabelMask * n)(), (L.FrameImage * n)()


def fields(s):
    return {k: (list(getattr(s, k)) if isinstance(getattr(s, k), C.Array) else getattr(s, k)) for k, _ in s._fields_}


def make_frames():
    """Three frames of two objects: object 0 brings HOST numpy images (a pose on frame 1, stamps on frame 2), object 1 integer
    addresses with MEM_DEVICE; frame 1 has neither flow nor mask."""
    rng = np.random.default_rng(3)
    out = []
    for t in range(3):
        host = dict(depth=rng.random((H, W), np.float32), flow=rng.random((H, W, 2), np.float32), mask=rng.integers(0, 2, (H, W), np.uint8),
                    dt=0.04 + t)
        dev = dict(depth=0x10000 + 0x100 * t, flow=0x20000 + 0x100 * t, mask=0x30000 + 0x100 * t, mem_kind=L.MEM_DEVICE, pose=None)
        if t == 1:
            host["flow"] = host["mask"] = dev["flow"] = dev["mask"] = None
            host["pose"] = ([0.1, 0.2, 0.3], [1.0, 0.0, 0.0, 0.0])
        if t == 2:
            host["stamp"], host["mask_stamp"] = 12.5, 12.25
        out.append([host, dev])
    return out


def test_filling_a_batch_at_a_base_index_equals_filling_each_frame():
    frames_list = make_frames()
    n = 2
    batch = arrays(3 * n)
    for t in (2, 0, 1):   # (any order: a fill touches its own frame's entries only)
        before = [[fields(a[i]) for i in range(3 * n) if i // n != t] for a in batch]
        keep, any_labels, any_images = E.fill_frame(frames_list[t], *batch, base=t * n)
        assert before == [[fields(a[i]) for i in range(3 * n) if i // n != t] for a in batch]
        one = arrays(n)
        keep1, any_labels1, any_images1 = E.fill_frame(frames_list[t], *one)
        assert (any_labels, any_images) == (any_labels1, any_images1) == (False, False)
        assert len(keep) == len(keep1) == (3 if t != 1 else 1) and all(x is y for x, y in zip(keep, keep1))
        for a, b in zip(batch, one):
            for i in range(n):
                assert fields(a[t * n + i]) == fields(b[i]), (t, i)
    fi = batch[0]
    assert fi[0].depth == frames_list[0][0]["depth"].ctypes.data and fi[0].mem_kind == L.MEM_HOST and fi[0].pose_valid == 0
    assert fi[1].depth == 0x10000 and fi[1].flow == 0x20000 and fi[1].mask == 0x30000 and fi[1].mem_kind == L.MEM_DEVICE
    assert fi[2].flow is None and fi[2].mask is None and fi[3].flow is None and fi[3].mask is None
    assert fi[2].pose_valid == 1 and list(fi[2].pose_x) == [0.1, 0.2, 0.3] and list(fi[2].pose_q) == [1.0, 0.0, 0.0, 0.0] and fi[3].pose_valid == 0
    assert (fi[2].dt, fi[4].dt, fi[4].stamp, fi[4].mask_stamp, fi[0].stamp) == (1.04, 2.04, 12.5, 12.25, 0.0)
    assert all(batch[1][i].labels is None and batch[2][i].image is None for i in range(3 * n))


@pytest.mark.parametrize("label_dtype, label_type", [(np.uint8, L.LABEL_U8), (np.uint16, L.LABEL_U16)])
def test_an_image_shared_by_the_objects_of_a_frame_is_one_pointer(label_dtype, label_type):
    lab = np.arange(H * W, dtype=label_dtype).reshape(H, W)
    rgb = np.zeros((H, W, 3), np.uint8)
    frames = [dict(depth=0x1000, labels=lab, label=3, image=rgb), dict(depth=0x1000, labels=lab, label=5, image=rgb, image_type=L.IMAGE_BGR8)]
    fi, lm, im = arrays(2)
    keep, any_labels, any_images = E.fill_frame(frames, fi, lm, im)
    assert any_labels and any_images
    assert len(keep) == 2 and keep[0] is rgb and keep[1] is lab             # one entry per shared array (depth is an address)
    assert lm[0].labels == lm[1].labels == lab.ctypes.data and im[0].image == im[1].image == rgb.ctypes.data
    assert (lm[0].label_type, lm[1].label_type, lm[0].label, lm[1].label) == (label_type, label_type, 3, 5)
    assert (im[0].image_type, im[1].image_type) == (L.IMAGE_RGB8, L.IMAGE_BGR8)   # three channels: RGB8 unless the frame says otherwise
    assert fi[0].mask is None and fi[0].flow is None
    # a view that is not contiguous is copied once, for both objects
    wide = np.zeros((H, 2 * W), np.uint8)
    keep, _, _ = E.fill_frame([dict(depth=1, image=wide[:, ::2])] * 2, fi, lm, im)
    assert len(keep) == 1 and keep[0].flags.c_contiguous and im[0].image == im[1].image == keep[0].ctypes.data
    assert (im[0].image_type, lm[0].labels, lm[0].label_type, lm[0].label) == (L.IMAGE_GRAY8, None, 0, 0)
    # addresses come with their type
    E.fill_frame([dict(depth=1, labels=0x500, label_type=L.LABEL_U16, label=2, image=0x700, image_type=L.IMAGE_GRAY8)] * 2, fi, lm, im)
    assert (lm[1].labels, lm[1].label_type, im[1].image, im[1].image_type) == (0x500, L.LABEL_U16, 0x700, L.IMAGE_GRAY8)


def test_wrong_dtypes_and_missing_keys_are_refused():
    fi, lm, im = arrays(1)
    lab = np.zeros((H, W), np.uint8)
    for bad in (dict(labels=lab.astype(np.float32), label=1), dict(labels=lab.astype(np.int32), label=1), dict(image=lab.astype(np.uint16)),
                dict(image=np.zeros((H, W, 4), np.uint8))):
        with pytest.raises(TypeError):
            E.fill_frame([dict(depth=1, **bad)], fi, lm, im)
    for bad in (dict(labels=lab), dict(labels=0x500, label=1), dict(image=0x700)):   # no label; an address without its type
        with pytest.raises(KeyError):
            E.fill_frame([dict(depth=1, **bad)], fi, lm, im)


@pytest.mark.parametrize("with_labels", [False, True])
@pytest.mark.parametrize("with_images", [False, True])
def test_batch_labels_and_batch_images_of_an_assembled_batch(with_labels, with_images):
    """Only frame 1 of three uses the forms: the batch's arrays are there for the whole batch, or None when no frame uses them."""
    lab = np.ones((H, W), np.uint16)
    gray = np.zeros((H, W), np.uint8)
    frames_list = [[dict(depth=0x1000 + t, mask=0x2000) for _ in range(2)] for t in range(3)]
    if with_labels:
        frames_list[1] = [dict(depth=0x1001, labels=lab, label=i + 1) for i in range(2)]
    if with_images:
        for f in frames_list[1]:
            f["image"] = gray
    arr, keep, T = E.assemble_batch(frames_list, 2)
    assert T == 3 and len(arr) == 6 and [arr[i].depth for i in range(6)] == [0x1000, 0x1000, 0x1001, 0x1001, 0x1002, 0x1002]
    labels, images = E.ROFTFilterBatch.batch_labels(keep), E.ROFTFilterBatch.batch_images(keep)
    assert (labels is not None) == with_labels and (images is not None) == with_images
    if with_labels:
        assert labels._type_ is L.LabelMask and len(labels) == 6
        assert [labels[i].label for i in range(6)] == [0, 0, 1, 2, 0, 0] and labels[2].labels == labels[3].labels != None and labels[0].labels is None
    if with_images:
        assert images._type_ is L.FrameImage and len(images) == 6
        assert images[2].image == images[3].image != None and images[2].image_type == L.IMAGE_GRAY8 and images[4].image is None
    assert E.ROFTFilterBatch.batch_labels([]) is None and E.ROFTFilterBatch.batch_images([]) is None
    with pytest.raises(AssertionError):
        E.assemble_batch([frames_list[0][:1]], 2)   # one dict per object

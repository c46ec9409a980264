"""Image pairs of the forward-backward check's tests, all 64 x 96 u8.

plain(seed)     a textured 28 x 40 box at rows 16.., columns 24.. of the first image, moved by (dy, dx) = (1, 2) in the second,
                over a static textured background
occluded(seed)  the same, with a 10 x 12 block of white noise over rows 26..35, columns 40..51 of the second image only
rolled()        uniform noise and its np.roll by (1, 2): the pair of test_opticalflow_gpu.test_noise_images_match_the_oracle, whose
                border vectors leave the image

A texture is Gaussian noise on a lattice of `cell` pixels, box-filtered (width `cell`) twice per axis, scaled to 128 +- 70."""
import numpy as np

H, W = 64, 96
BOX = (16, 24, 28, 40)        # top, left, height, width in the first image
SHIFT = (1, 2)                # (dy, dx)
OCCLUDER = (26, 40, 10, 12)   # top, left, height, width in the second image


def _box_filter(a, n, axis):
    k = np.ones(n) / n
    return np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), axis, a)


def texture(rng, h, w, cell):
    pad = 2 * cell
    g = rng.standard_normal(((h + 2 * pad + cell - 1) // cell, (w + 2 * pad + cell - 1) // cell))
    t = np.repeat(np.repeat(g, cell, 0), cell, 1)
    for axis in (0, 1):
        for _ in range(2):
            t = _box_filter(t, cell, axis)
    t = t[pad:pad + h, pad:pad + w]
    t = t - t.mean()
    return 128.0 + 70.0 * t / np.abs(t).max()


def _to_u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def plain(seed):
    rng = np.random.default_rng(seed)
    back = texture(rng, H, W, 4)
    top, left, bh, bw = BOX
    box = texture(rng, bh, bw, 3)
    a, b = back.copy(), back.copy()
    a[top:top + bh, left:left + bw] = box
    b[top + SHIFT[0]:top + SHIFT[0] + bh, left + SHIFT[1]:left + SHIFT[1] + bw] = box
    return _to_u8(a), _to_u8(b)


def occluded(seed):
    a, b = plain(seed)
    rng = np.random.default_rng(seed + 1000)
    top, left, oh, ow = OCCLUDER
    b = b.copy()
    b[top:top + oh, left:left + ow] = rng.integers(0, 256, (oh, ow), dtype=np.uint8)
    return a, b


def rolled():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return a, np.roll(a, (1, 2), (0, 1))


def box_mask(shift=(0, 0)):
    m = np.zeros((H, W), bool)
    top, left, bh, bw = BOX
    m[top + shift[0]:top + shift[0] + bh, left + shift[1]:left + shift[1] + bw] = True
    return m


def erode(m, n):
    """pixels at least n px inside m (Chebyshev), the image border counting as outside"""
    p = np.pad(m, n, constant_values=False)
    out = np.ones_like(m)
    for dy in range(-n, n + 1):
        for dx in range(-n, n + 1):
            out &= p[n + dy:n + dy + m.shape[0], n + dx:n + dx + m.shape[1]]
    return out


def dilate(m, n):
    p = np.pad(m, n, constant_values=False)
    out = np.zeros_like(m)
    for dy in range(-n, n + 1):
        for dx in range(-n, n + 1):
            out |= p[n + dy:n + dy + m.shape[0], n + dx:n + dx + m.shape[1]]
    return out


def covered_object_pixels():
    """first-image object pixels whose target (their position moved by SHIFT) lies at least 2 px inside the occluder"""
    occ = np.zeros((H, W), bool)
    top, left, oh, ow = OCCLUDER
    occ[top:top + oh, left:left + ow] = True
    core = erode(occ, 2)
    return box_mask() & np.roll(core, (-SHIFT[0], -SHIFT[1]), (0, 1))

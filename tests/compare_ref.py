"""Numpy statement of the comparison rule ("Comparison rule"; include/fpcdr.h, fpcdr_compare_u8), written for the test
suite, operation by operation; it imports nothing from the package.  tests/test_compare_ref.py checks the statement itself,
tests/test_gpu_compare.py holds the kernel to it bit for bit.

    r  = flip_rows ? H-1-i : i                       (the flip applies to img only)
    q  = img is uint8 ? img[n,r,j] : x = img[n,r,j] * scale in float32; NaN -> 0; else clip(rint(x), 0, 255), rint = half to even
    d  = q - ref[n,i,j]
    s  = max(255 - 2 |d|, 0)
    heat[n,i,j,:] = colour: d >= 0 ? (255, s, s) : (s, s, 255);  grey: (s, s, s)
    row_sums[n,i] = sum over j in [col0, col1) and [0, W) of |d|        (int32)
"""
import numpy as np


def quantise(img, scale=255.0):
    """uint8 images as they are; float32 images by one float32 multiply, NaN -> 0, round half to even, clip to [0, 255]."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.copy()
    assert img.dtype == np.float32, img.dtype
    with np.errstate(invalid='ignore', over='ignore'):
        x = img * np.float32(scale)                      # float32 * float32 -> float32
    assert x.dtype == np.float32
    y = np.clip(np.rint(x), np.float32(0), np.float32(255))       # np.rint rounds half to even; +-inf clip like any value
    y = np.where(np.isnan(x), np.float32(0), y)
    return y.astype(np.uint8)


def difference(img, ref, scale=255.0, flip_rows=False):
    """d [N,H,W] int32: quantised img (rows flipped if asked) minus ref."""
    q = quantise(img, scale)
    ref = np.asarray(ref)
    assert ref.dtype == np.uint8 and q.shape == ref.shape and q.ndim == 3, (q.shape, ref.shape)
    if flip_rows:
        q = q[:, ::-1]
    return q.astype(np.int32) - ref.astype(np.int32)


def heat_map(d, mode='colour'):
    """[..., 3] uint8 from integer differences."""
    d = np.asarray(d, dtype=np.int32)
    s = np.maximum(255 - 2 * np.abs(d), 0)
    full = np.full_like(s, 255)
    if mode == 'colour':
        out = np.stack([np.where(d >= 0, full, s), s, np.where(d >= 0, s, full)], axis=-1)
    else:
        assert mode == 'grey', mode
        out = np.stack([s, s, s], axis=-1)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def row_sums(d, cols=(100, 1100)):
    """[N,H] int32: sum of |d| over the columns [col0, col1) that lie inside the image."""
    d = np.asarray(d, dtype=np.int32)
    W = d.shape[-1]
    c0, c1 = max(int(cols[0]), 0), min(int(cols[1]), W)
    if c0 >= c1:
        return np.zeros(d.shape[:-1], dtype=np.int32)
    total = np.abs(d[..., c0:c1]).astype(np.int64).sum(axis=-1)
    assert total.max(initial=0) < 2 ** 31
    return total.astype(np.int32)


def compare(img, ref, mode='colour', cols=(100, 1100), scale=255.0, flip_rows=False):
    """(heat [N,H,W,3] uint8, row_sums [N,H] int32) of the rule."""
    d = difference(img, ref, scale, flip_rows)
    return heat_map(d, mode), row_sums(d, cols)


# ---- inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
# float values with scale = 1: exact ties, both ends of the range and beyond, not-a-number, infinities, negative zero, a denormal
SPECIAL = np.array([0.5, 1.5, 2.5, 3.5, 126.5, 127.5, 253.5, 254.5, 255.5, -0.5, -1.5, 0.0, -0.0, 255.0, 256.0, 1e9, -1e9, 3e38, -3e38,
                    np.nan, -np.nan, np.inf, -np.inf, 0.49999997, 0.50000006, 254.49998, 254.50002, 1e-40, 127.0, 128.0],
                   dtype=np.float32)


def u8_pair(N, H, W, seed):
    """Random uint8 images; about a quarter of the pixels have |d| > 127 and some d = 0."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    img = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    same = rng.uniform(size=(N, H, W)) < 0.1
    img[same] = ref[same]
    return img, ref


def float_pair(N, H, W, seed):
    """Float images for scale = 1: uniform in [-40, 300] (values below 0 and above 255), with every fourth pixel or so replaced by an
    entry of SPECIAL."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    img = rng.uniform(-40.0, 300.0, size=(N, H, W)).astype(np.float32)
    pick = rng.uniform(size=(N, H, W)) < 0.25
    img[pick] = SPECIAL[rng.integers(0, SPECIAL.size, size=int(pick.sum()))]
    img.reshape(-1)[:SPECIAL.size] = SPECIAL[:img.size]           # every special value at least once where the image is large enough
    return img, ref

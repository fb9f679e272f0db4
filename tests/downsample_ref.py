"""The Downsample rule in numpy, operation by operation: what fpcdr_downsample_u8 / ops.downsample_images must give bit
for bit.

  src [..., H, W] uint8, factor s in 2..16, H % s == 0, W % s == 0
  S[..., i, j]   = sum of src[..., i * s + a, j * s + b] over 0 <= a, b < s        (an integer, at most 255 * 16 * 16 = 65 280)
  out[..., i, j] = (2 * S + s * s) // (2 * s * s)                                   (the exact mean, rounded half up, rounded once)

Rows are not flipped.  Every level of a pyramid is made from the full-size image: a cascade rounds more than once."""
import numpy as np


def block_sums(src, s):
    """S of the rule as int64 [..., H / s, W / s]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim >= 2
    s = int(s)
    assert 2 <= s <= 16, s
    H, W = src.shape[-2:]
    assert H > 0 and W > 0 and H % s == 0 and W % s == 0, (H, W, s)
    blocks = src.reshape(src.shape[:-2] + (H // s, s, W // s, s)).astype(np.int64)
    return blocks.sum(axis=(-3, -1))


def downsample(src, s):
    """The rule: uint8 [..., H / s, W / s]."""
    s = int(s)
    S = block_sums(src, s)
    out = (2 * S + s * s) // (2 * s * s)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def tie_image(s, rows=2, cols=3):
    """Blocks whose sum S makes 2 S + s^2 an exact multiple of 2 s^2 (the mean is k + 1/2: s even): block (i, j) has mean k + 1/2 for
    k = 0, 1, ...; the s^2 / 2 larger bytes sit on a checkerboard (for s = 2 and k = 0 the block (1, 0, 0, 1))."""
    assert s % 2 == 0
    a, b = np.meshgrid(np.arange(s), np.arange(s), indexing='ij')
    board = ((a + b) % 2 == 0).astype(np.int64)                         # s^2 / 2 ones
    img = np.zeros((rows * s, cols * s), dtype=np.uint8)
    want = np.zeros((rows, cols), dtype=np.uint8)
    for i in range(rows):
        for j in range(cols):
            k = (i * cols + j) * 50
            img[i * s:(i + 1) * s, j * s:(j + 1) * s] = (k + board).astype(np.uint8)
            want[i, j] = k + 1                                         # half UP
    return img, want

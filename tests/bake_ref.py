"""The Bake rule stated in numpy, operation by operation: the yardstick of tests/test_gpu_bake.py (torch.equal, no
tolerance), itself checked on the CPU by tests/test_bake_ref.py.  Nothing here imports fpc_diffrend_amd or oracle.

accumulate: every covered pixel splats its capture into the four texels the 'linear' texture lookup reads for it (taps(): make_taps of
csrc/texsample.h in float32, operation by operation), with the bilinear weights quantised to 1/256 per axis, into unsigned 64-bit sums
(num, den) per texel.  resolve: num / (den * color_scale) in double, rounded once to float32.  dilate: one Jacobi pass of the gutter.
"""
import numpy as np

F32 = np.float32


def prep(u, mode):
    """prep_coord: float32 in, float32 out."""
    if mode == 'wrap':
        return (u - np.floor(u)).astype(F32)
    assert mode == 'clamp', mode
    return np.minimum(np.maximum(u, F32(0.0)), F32(1.0)).astype(F32)      # (finite coordinates only reach the taps)


def axis_taps(u, n, mode):
    """One axis of make_taps for FINITE float32 coordinates u: (index of the first texel, of the second, fraction), int64 / float32."""
    x = (prep(u, mode) * F32(n)).astype(F32) - F32(0.5)                   # one multiply, one subtraction, each rounded to float32
    x = x.astype(F32)
    x0f = np.floor(x)
    f = (x - x0f).astype(F32)
    x0 = x0f.astype(np.int64)
    if mode == 'wrap':
        return np.mod(x0, n), np.mod(x0 + 1, n), f
    return np.clip(x0, 0, n - 1), np.clip(x0 + 1, 0, n - 1), f


def weights(ax, ay):
    """The four integer weights (00, 10, 01, 11) of the quantised fractions ax, ay in 0..256: they sum to 65536."""
    ax, ay = np.asarray(ax, dtype=np.int64), np.asarray(ay, dtype=np.int64)
    return (256 - ax) * (256 - ay), ax * (256 - ay), (256 - ax) * ay, ax * ay


def quantise_fraction(f):
    """(int)floorf(f * 256.0f) of a float32 fraction in [0, 1]: the product is exact (a power of two), 0..256."""
    return np.floor((f.astype(F32) * F32(256.0)).astype(F32)).astype(np.int64)


def contributes(texc, rast, interior_only=False):
    """ok [N,H,W]: covered (rast.w > 0; a NaN is not), both coordinates finite and, with interior_only, the neighbours up, down, left and
    right that lie inside the image covered too."""
    with np.errstate(invalid='ignore'):
        cov = rast[..., 3] > 0
    ok = cov & np.isfinite(texc[..., 0]) & np.isfinite(texc[..., 1])
    if interior_only:
        inner = np.ones_like(cov)
        inner[:, 1:, :] &= cov[:, :-1, :]
        inner[:, :-1, :] &= cov[:, 1:, :]
        inner[:, :, 1:] &= cov[:, :, :-1]
        inner[:, :, :-1] &= cov[:, :, 1:]
        ok &= inner
    return ok


def contributions(texc, rast, ref, Ht, Wt, mode='wrap', interior_only=False, flip_rows=False):
    """The (pixel, tap) pairs of a batch: (texel [P,4] flat indices, w [P,4] integer weights, c [P] captures) over the P contributing
    pixels in (n, i, j) order.  A tap of weight 0 stays in the list with w = 0: it adds nothing."""
    texc, rast, ref = np.asarray(texc), np.asarray(rast), np.asarray(ref)
    assert texc.dtype == F32 and rast.dtype == F32 and ref.dtype == np.uint8
    N, H, W, _ = texc.shape
    assert rast.shape == (N, H, W, 4) and ref.shape == (N, H, W)
    ok = contributes(texc, rast, interior_only)
    cap = ref[:, ::-1] if flip_rows else ref                              # the flip applies to ref only
    c = cap[ok].astype(np.int64)
    u, v = texc[..., 0][ok], texc[..., 1][ok]
    ix0, ix1, fx = axis_taps(u, Wt, mode)
    iy0, iy1, fy = axis_taps(v, Ht, mode)
    w = np.stack(weights(quantise_fraction(fx), quantise_fraction(fy)), axis=1)
    texel = np.stack([iy0 * Wt + ix0, iy0 * Wt + ix1, iy1 * Wt + ix0, iy1 * Wt + ix1], axis=1)
    return texel, w, c


def accumulate(texc, rast, ref, acc, mode='wrap', interior_only=False, flip_rows=False):
    """acc [Ht,Wt,2] uint64 (num, den) is ADDED to, in place, and returned."""
    assert acc.dtype == np.uint64 and acc.ndim == 3 and acc.shape[2] == 2
    Ht, Wt = acc.shape[:2]
    texel, w, c = contributions(texc, rast, ref, Ht, Wt, mode, interior_only, flip_rows)
    flat = acc.reshape(-1, 2)
    for k in range(4):                    # (in clamp mode two taps may name the same texel: both add)
        np.add.at(flat[:, 0], texel[:, k], (w[:, k] * c).astype(np.uint64))
        np.add.at(flat[:, 1], texel[:, k], w[:, k].astype(np.uint64))
    return acc


def min_den_of(min_weight):
    return max(1, int(round(float(min_weight) * 65536)))


def resolve(acc, color_scale=255.0, min_den=1):
    """(tex float32 [Ht,Wt], filled bool [Ht,Wt]): one double multiply, one double division, one rounding to float32."""
    assert acc.dtype == np.uint64 and min_den >= 1
    num, den = acc[..., 0], acc[..., 1]
    filled = den >= np.uint64(min_den)
    q = np.zeros(num.shape, dtype=np.float64)
    q[filled] = num[filled].astype(np.float64) / (den[filled].astype(np.float64) * np.float64(color_scale))
    return q.astype(F32), filled


def dilate(tex, filled):
    """One Jacobi pass: an unfilled texel with filled ones among its eight neighbours inside the texture (no wrap) becomes their float32
    sum -- added in the order dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner), starting from 0 -- divided by float32(count), and is marked
    filled; everything else is copied.  Reads its inputs only."""
    assert tex.dtype == F32 and filled.dtype == np.bool_ and tex.shape == filled.shape
    Ht, Wt = tex.shape
    tp = np.zeros((Ht + 2, Wt + 2), dtype=F32)
    fp = np.zeros((Ht + 2, Wt + 2), dtype=np.bool_)
    tp[1:-1, 1:-1], fp[1:-1, 1:-1] = tex, filled
    total = np.zeros((Ht, Wt), dtype=F32)
    count = np.zeros((Ht, Wt), dtype=np.int32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            t = tp[1 + dy:1 + dy + Ht, 1 + dx:1 + dx + Wt]
            f = fp[1 + dy:1 + dy + Ht, 1 + dx:1 + dx + Wt]
            total = np.where(f, (total + t).astype(F32), total)           # (the centre of an unfilled texel is not filled: no term)
            count = count + f
    new = ~filled & (count > 0)
    out = tex.copy()
    out[new] = (total[new] / count[new].astype(F32)).astype(F32)
    return out, filled | new


def bake(acc, color_scale=255.0, min_weight=0.0, passes=8, hole_value=0.5):
    """ops.bake_resolve: (tex, filled before the dilation)."""
    tex, filled = resolve(acc, color_scale, min_den_of(min_weight))
    f = filled
    for _ in range(passes):
        tex, f = dilate(tex, f)
    return np.where(f, tex, F32(hole_value)).astype(F32), filled


# ---- the inputs of the rule grid (tests/test_gpu_bake.py; the CPU file checks that they hold what the grid is for) ----------------------
def grid_inputs(N, H, W, Ht, Wt, seed):
    """texc uniform in [-0.5, 1.5], seeded with exact texel centres (k + 1/2) / n, texel borders k / n, 0, 1, NaN and +-inf; rast.w a
    mix of 0, positive, negative and NaN; ref uniform over 0..255."""
    rng = np.random.default_rng(seed)
    texc = rng.uniform(-0.5, 1.5, size=(N, H, W, 2)).astype(F32)
    flat = texc.reshape(-1, 2)
    P = flat.shape[0]
    special = []
    for axis, n in ((0, Wt), (1, Ht)):
        k = np.arange(-1, n + 2, dtype=np.float64)
        special += [(axis, val) for val in ((k + 0.5) / n).astype(F32)] + [(axis, val) for val in (k / n).astype(F32)]
        special += [(axis, F32(0.0)), (axis, F32(1.0)), (axis, F32(-1e-9)), (axis, F32(np.nan)), (axis, F32(np.inf)), (axis, F32(-np.inf))]
    where = rng.permutation(P)
    for s, (axis, val) in enumerate(special):
        for rep in range(2):              # twice where the image has the room: the first is covered for certain (below)
            q = s * 2 + rep
            if q < P:
                flat[where[q], axis] = val
    rast = rng.uniform(-1.0, 1.0, size=(N, H, W, 4)).astype(F32)
    kind = rng.integers(0, 10, size=(N, H, W))
    w = np.where(kind < 6, rng.integers(1, 2000, size=(N, H, W)).astype(F32), F32(0.0))      # covered: triangle id + 1
    w = np.where(kind == 8, F32(-3.0), w)
    w = np.where(kind == 9, F32(np.nan), w).astype(F32)
    w.reshape(-1)[where[0:min(2 * len(special), P):2]] = F32(7.0)
    # both coordinates special at once, covered, on the last pixels of the permutation: a centre (one tap has all the weight), a corner,
    # (0, 0) and (1, 1)
    both = [((0.5) / Wt, (Ht - 0.5) / Ht), (1.0 / Wt, 1.0 / Ht), (0.0, 0.0), (1.0, 1.0)]
    for s, (u, v) in enumerate(both[:max(0, min(len(both), P - 1))]):
        flat[where[P - 1 - s]] = (F32(u), F32(v))
        w.reshape(-1)[where[P - 1 - s]] = F32(7.0)
    rast[..., 3] = w
    ref = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    return texc, rast, ref

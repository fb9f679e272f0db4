"""The Exposure rule in numpy and Python integers, operation by operation and from the rule's text: what
fpcdr_exposure_sums / ops.exposure_sums, exposure.fit_gains, fpcdr_apply_lut_u8 / ops.apply_lut_u8 and exposure.compose must give bit for
bit.  `sums` is the statement by array operations, `sums_loops` the same by a brute-force loop over images, pixels and channels
(tests/test_exposure_ref.py holds the two to each other).  Imports nothing of fpc_diffrend_amd."""
import math

import numpy as np


def quantise(colour):
    """The Comparison rule's byte of a float32 value at scale 255: the float32 product, NaN -> 0, round half to even, clip to 0..255."""
    x = np.asarray(colour, dtype=np.float32) * np.float32(255.0)
    with np.errstate(invalid='ignore'):
        y = np.clip(np.rint(x), np.float32(0.0), np.float32(255.0))
    return np.where(np.isnan(x), np.float32(0.0), y).astype(np.int64)


def counted(rast, ref, mask=None, face_w=None, lo=1, hi=254):
    """bool [B,H,W]: the pixels whose samples count."""
    w = np.asarray(rast, dtype=np.float32)[..., 3]
    with np.errstate(invalid='ignore'):
        cov = w > 0                                   # (a NaN is not covered)
    B, H, W = cov.shape
    pad = np.ones((B, H + 2, W + 2), dtype=bool)      # a neighbour outside the image asks nothing
    pad[:, 1:-1, 1:-1] = cov
    ok = cov & pad[:, :-2, 1:-1] & pad[:, 2:, 1:-1] & pad[:, 1:-1, :-2] & pad[:, 1:-1, 2:]
    t = np.asarray(ref).astype(np.int64)
    ok &= (t >= lo) & (t <= hi)
    if mask is not None:
        ok &= np.asarray(mask) >= 128
    if face_w is not None:
        fw = np.asarray(face_w, dtype=np.float32)
        ids = np.where(cov, w, 0).astype(np.int64)    # the triangle id + 1 of a covered pixel
        inside = (ids >= 1) & (ids <= fw.shape[0])
        with np.errstate(invalid='ignore'):
            ok &= inside & (fw[np.clip(ids - 1, 0, fw.shape[0] - 1)] > 0)
    return ok


def sums(colour, rast, ref, mask=None, face_w=None, lo=1, hi=254, into=None):
    """int64 [B,6] = (n, sum r, sum t, sum r^2, sum t^2, sum r t) per image, added to `into` when given."""
    ok = counted(rast, ref, mask, face_w, lo, hi)
    r = quantise(colour)                              # [B,H,W,C]
    t = np.broadcast_to(np.asarray(ref).astype(np.int64)[..., None], r.shape)
    k = np.broadcast_to(ok[..., None], r.shape).astype(np.int64)
    out = np.stack([(k * q).sum(axis=(1, 2, 3)) for q in (np.ones_like(r), r, t, r * r, t * t, r * t)], axis=1)
    return out if into is None else np.asarray(into, dtype=np.int64) + out


def sums_loops(colour, rast, ref, mask=None, face_w=None, lo=1, hi=254):
    """`sums` by one loop over images, pixels and channels, every condition spelt out."""
    colour, rast, ref = np.asarray(colour, dtype=np.float32), np.asarray(rast, dtype=np.float32), np.asarray(ref)
    B, H, W, C = colour.shape
    cov = lambda b, y, x: bool(rast[b, y, x, 3] > 0)
    out = [[0] * 6 for _ in range(B)]
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if not cov(b, y, x):
                    continue
                if any(0 <= yy < H and 0 <= xx < W and not cov(b, yy, xx) for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1))):
                    continue
                t = int(ref[b, y, x])
                if not lo <= t <= hi:
                    continue
                if mask is not None and int(mask[b, y, x]) < 128:
                    continue
                if face_w is not None:
                    tri = int(rast[b, y, x, 3]) - 1
                    if not (0 <= tri < len(face_w) and float(face_w[tri]) > 0):
                        continue
                for k in range(C):
                    v = np.float32(colour[b, y, x, k]) * np.float32(255.0)
                    r = 0 if math.isnan(v) else int(min(max(np.rint(v), 0), 255))
                    for q, term in enumerate((1, r, t, r * r, t * t, r * t)):
                        out[b][q] += term
    return np.array(out, dtype=np.int64)


def fit_gains(sums, method='regression', anchor=None, max_gain=4.0, keep_from=256):
    """The fit of the rule from per-camera sums [Nc,6] (any integers): {'a', 'b', 'rho', 'g' float64 [Nc], 'usable' bool [Nc], 'lut' uint8
    [Nc,256]}; ValueError for an anchor that is not usable.  The order of the float64 operations is the rule's."""
    rows = [[int(v) for v in row] for row in np.asarray(sums).tolist()]
    Nc = len(rows)
    a, b, rho, g = ([math.nan] * Nc for _ in range(4))
    usable = [False] * Nc
    for c, (n, Sr, St, Srr, Stt, Srt) in enumerate(rows):
        Vr, Vt, Cv = n * Srr - Sr ** 2, n * Stt - St ** 2, n * Srt - Sr * St
        if n >= 2 and Vr > 0 and Vt > 0:
            rho[c] = float(Cv) / math.sqrt(float(Vr * Vt))
        if not (n >= 2 and Vr > 0 and Vt > 0 and Cv > 0):
            continue
        usable[c] = True
        a[c] = Cv / Vr if method == 'regression' else math.sqrt(Vt / Vr)      # (int / int: the exact quotient, rounded once)
        b[c] = (float(St) - a[c] * float(Sr)) / float(n)
    lut = np.tile(np.arange(256, dtype=np.uint8), (Nc, 1))
    if anchor is not None:
        if not usable[anchor]:
            raise ValueError("the anchor camera is not usable")
        a_bar, b_bar = a[anchor], b[anchor]
    else:
        live = [c for c in range(Nc) if usable[c]]
        if live:
            sa = sb = 0.0
            for c in live:
                sa, sb = sa + a[c], sb + b[c]
            a_bar, b_bar = sa / float(len(live)), sb / float(len(live))
    for c in range(Nc):
        if not usable[c]:
            continue
        g[c] = a_bar / a[c]
        if not 1.0 / max_gain <= g[c] <= max_gain:
            usable[c] = False
            continue
        for v in range(min(keep_from, 256)):
            m = math.floor(((float(v) - b[c]) * g[c] + b_bar) + 0.5)
            lut[c, v] = min(min(max(m, 0), 255), keep_from - 1)
    return {'a': np.array(a), 'b': np.array(b), 'rho': np.array(rho), 'g': np.array(g), 'usable': np.array(usable), 'lut': lut}


def apply(images, lut, cam_of_image):
    """images[b] <- lut[cam_of_image[b]][images[b]] as a new array; an image whose camera is outside the table stays as it is."""
    images, lut = np.asarray(images), np.asarray(lut)
    out = images.copy()
    for b, c in enumerate(np.asarray(cam_of_image).tolist()):
        if 0 <= c < lut.shape[0]:
            out[b] = lut[c][images[b]]
    return out


def compose(total, lut):
    """The table of `total` followed by `lut`, per camera."""
    total, lut = np.asarray(total), np.asarray(lut)
    return np.stack([lut[c][total[c]] for c in range(total.shape[0])]).astype(np.uint8)


IDENTITY = lambda n: np.tile(np.arange(256, dtype=np.uint8), (n, 1))


# ---- the small cases the CPU self-check and the GPU test share ---------------------------------------------------------------------------
SIZES = ((1, 1), (3, 17), (5, 16), (7, 33), (72, 96))


def case(B, H, W, C, seed, n_faces=40):
    """(colour [B,H,W,C] f32, rast [B,H,W,4] f32, ref [B,H,W] u8, mask [B,H,W] u8, face_w [n_faces - 1] f32): coverage with uncovered
    pixels on the border, in the corners and singly inside (the interior rule fires on all four sides, and on none at the border of a
    covered image edge); ids 1..n_faces with a table one short of the largest id and some weights 0; mask bytes 0, 127, 128, 255; colour
    with NaN, +-inf, negatives and values above 1; captures over the whole byte range."""
    rng = np.random.default_rng(seed)
    colour = rng.uniform(-0.1, 1.1, size=(B, H, W, C)).astype(np.float32)
    flat = colour.reshape(-1)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -3.0, 7.5, 0.5 / 255.0, 1.5 / 255.0, 2.5 / 255.0)):      # (ties: half to even)
        flat[(k * 7919) % flat.size] = v
    ids = rng.integers(1, n_faces + 1, size=(B, H, W)).astype(np.float32)
    cov = rng.random((B, H, W)) < 0.93                           # single holes inside
    if H > 2 and W > 2:
        cov[:, 0, ::3] = False                                   # holes along the borders
        cov[:, -1, 1::4] = False
        cov[:, ::3, 0] = False
        cov[:, 1::2, -1] = False
        cov[0, 0, 0], cov[0, -1, -1], cov[-1, 0, -1], cov[-1, -1, 0] = False, False, True, True
        cov[-1, H // 2, W // 2] = False
        cov[-1, H // 2 - 1: H // 2 + 2, W // 2 - 1] = True       # the hole's four neighbours are covered themselves
        cov[-1, H // 2 - 1: H // 2 + 2, W // 2 + 1] = True
        cov[-1, H // 2 - 1, W // 2], cov[-1, H // 2 + 1, W // 2] = True, True
    if B > 1:
        cov[1] = True                                            # a fully covered image: the border asks nothing
    rast = rng.uniform(0.0, 1.0, size=(B, H, W, 4)).astype(np.float32)
    rast[..., 3] = np.where(cov, ids, 0.0)
    if H > 2 and W > 2:
        rast[0, 1, 1, 3] = np.nan                                # not covered
    ref = rng.integers(0, 256, size=(B, H, W)).astype(np.uint8)
    ends = min(4, ref.size)
    ref.reshape(-1)[:ends] = (0, 1, 254, 255)[:ends]                 # both ends of (lo, hi) = (1, 254), and just outside
    mask = rng.choice(np.array([0, 127, 128, 255], dtype=np.uint8), size=(B, H, W), p=(0.1, 0.1, 0.4, 0.4))
    face_w = rng.uniform(0.1, 2.0, size=n_faces - 1).astype(np.float32)
    face_w[::5] = 0.0
    return colour, rast, ref, mask, face_w

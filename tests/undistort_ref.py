"""Float64 numpy statement of the undistortion rule ("Undistortion rule"; include/fpcdr.h, fpcdr_undistort_u8), written
operation by operation: numpy evaluates every line below as ONE correctly rounded IEEE double operation per element, never fused, which
is what the kernel is built to do (-ffp-contract=off).  Also the forward model on normalised coordinates and an iterative inverse of it,
from which the tests synthesise distorted raw images."""
import numpy as np


def camera_row(intr, dist):
    """fx, fy, cx, cy, k1, k2, p1, p2, k3 as doubles (the widened float32 values when the calibration holds float32)."""
    K = np.asarray(intr).astype(np.float64)
    d = np.asarray(dist).astype(np.float64).reshape(5)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2]) + tuple(d)


def distort_points(x, y, dist):
    """Forward model: normalised pinhole coordinates -> normalised distorted coordinates (OpenCV's five coefficients)."""
    k1, k2, p1, p2, k3 = (np.float64(c) for c in np.asarray(dist, dtype=np.float64).reshape(5))
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    xx = x * x
    yy = y * y
    r2 = xx + yy
    t = r2 * k3
    t = k2 + t
    t = r2 * t
    t = k1 + t
    t = r2 * t
    rad = 1.0 + t
    xy = x * y
    tx = (2.0 * p1) * xy
    sx = 2.0 * xx
    sx = r2 + sx
    sx = p2 * sx
    tx = tx + sx
    xd = x * rad
    xd = xd + tx
    sy = 2.0 * yy
    sy = r2 + sy
    sy = p1 * sy
    ty = (2.0 * p2) * xy
    ty = sy + ty
    yd = y * rad
    yd = yd + ty
    return xd, yd


def undistort_points(xd, yd, dist, iterations=60):
    """Inverse of distort_points by fixed-point iteration (x <- (xd - tangential(x)) / radial(x)); test-side only."""
    k1, k2, p1, p2, k3 = np.asarray(dist, dtype=np.float64).reshape(5)
    xd = np.asarray(xd, dtype=np.float64)
    yd = np.asarray(yd, dtype=np.float64)
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x = (xd - dx) / rad
        y = (yd - dy) / rad
    return x, y


def source_coordinates(H, W, intr, dist):
    """(u, v): where in the raw image the output pixel (row i from the top, column j) looks; two [H,W] float64 arrays."""
    fx, fy, cx, cy = camera_row(intr, dist)[:4]
    j = np.arange(W, dtype=np.float64)[None, :]
    i = np.arange(H, dtype=np.float64)[:, None]
    x = (j - cx) / fx
    y = (i - cy) / fy
    x, y = np.broadcast_arrays(x, y)
    xd, yd = distort_points(x, y, camera_row(intr, dist)[4:])
    u = fx * xd
    u = u + cx
    v = fy * yd
    v = v + cy
    return u, v


def undistort_values(img, intr, dist):
    """`val` of the rule, [H,W] float64, before rounding and clipping, and the mask of pixels whose four taps are inside."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    u, v = source_coordinates(H, W, intr, dist)
    with np.errstate(invalid='ignore'):
        u0 = np.floor(u)
        v0 = np.floor(v)
        a = u - u0
        b = v - v0
        near = (u0 >= -1.0) & (u0 < W) & (v0 >= -1.0) & (v0 < H)     # at least one tap inside (false where u, v are not numbers)
    iu = np.where(near, u0, 0.0).astype(np.int64)
    iv = np.where(near, v0, 0.0).astype(np.int64)
    src = img.astype(np.float64)

    def tap(r, c):
        ok = near & (r >= 0) & (r < H) & (c >= 0) & (c < W)
        return np.where(ok, src[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)], 0.0)

    t00, t01, t10, t11 = tap(iv, iu), tap(iv, iu + 1), tap(iv + 1, iu), tap(iv + 1, iu + 1)
    a = np.where(near, a, 0.0)
    b = np.where(near, b, 0.0)
    top = t01 - t00
    top = a * top
    top = t00 + top
    bot = t11 - t10
    bot = a * bot
    bot = t10 + bot
    val = bot - top
    val = b * val
    val = top + val
    inside = near & (iu >= 0) & (iu + 1 < W) & (iv >= 0) & (iv + 1 < H)
    return val, inside


def undistort_image(img, intr, dist, clip_max=255, flip_rows=False):
    """The rule: uint8 [H,W] raw image -> uint8 [H,W]."""
    val, _ = undistort_values(img, intr, dist)
    out = np.minimum(np.floor(val + 0.5), float(clip_max)).astype(np.uint8)
    return np.ascontiguousarray(out[::-1]) if flip_rows else out


def undistort_batch(images, intr, dist, clip_max=255, flip_rows=False):
    """[N,H,W] or [F,Nc,H,W] uint8; image n uses camera row n % Nc."""
    images = np.asarray(images)
    flat = images.reshape(-1, *images.shape[-2:])
    Nc = len(intr)
    out = np.stack([undistort_image(flat[n], intr[n % Nc], dist[n % Nc], clip_max, flip_rows) for n in range(flat.shape[0])])
    return out.reshape(images.shape)


def rounding_margin(img, intr, dist):
    """Smallest |val - floor(val) - 0.5| over the image: how far the nearest pixel is from a rounding tie."""
    val, _ = undistort_values(img, intr, dist)
    return float(np.abs(val - np.floor(val) - 0.5).min())


def distort_image(ideal, intr, dist, fill=0.0):
    """Test-side synthesis of a raw capture: the raw pixel at the distorted position shows what the pinhole image `ideal` shows at
    the undistorted one (iterative inverse model, bilinear, `fill` outside); rounded to 8 bit.  [H,W] uint8."""
    ideal = np.asarray(ideal)
    H, W = ideal.shape
    fx, fy, cx, cy = camera_row(intr, dist)[:4]
    jd, id_ = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y = undistort_points((jd - cx) / fx, (id_ - cy) / fy, camera_row(intr, dist)[4:])
    u, v = fx * x + cx, fy * y + cy
    ok = np.isfinite(u) & np.isfinite(v) & (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    u0, v0 = np.minimum(np.floor(u), W - 2).astype(np.int64), np.minimum(np.floor(v), H - 2).astype(np.int64)
    a, b = u - u0, v - v0
    s = ideal.astype(np.float64)
    val = (s[v0, u0] * (1 - a) + s[v0, u0 + 1] * a) * (1 - b) + (s[v0 + 1, u0] * (1 - a) + s[v0 + 1, u0 + 1] * a) * b
    return np.where(ok, np.floor(val + 0.5), float(fill)).astype(np.uint8)


# ---- shared test inputs ------------------------------------------------------------------------------------------------------------
K_LONG = np.array([[9600, 0, 803.7], [0, 9590, 596.2], [0, 0, 1]], dtype=np.float32)       # the rig's long lenses, 1200 x 1600
K_WIDE = np.array([[1400, 0, 800], [0, 1400, 600], [0, 0, 1]], dtype=np.float32)
DIST = {
    'zero': np.zeros(5, dtype=np.float32),
    'mild': np.array([-0.35, 0.9, 1e-3, -7e-4, -2.0], dtype=np.float32),           # K_LONG: up to 4 px
    'strong': np.array([12.0, -300.0, 2e-2, 1e-2, 0.0], dtype=np.float32),         # K_LONG: up to 101 px, 12 % of the taps outside
    'tangential': np.array([0.0, 0.0, 3e-2, -2e-2, 0.0], dtype=np.float32),
    'wide': np.array([-0.28, 0.11, 1.5e-3, -8e-4, -0.02], dtype=np.float32),       # with K_WIDE
}


def intrinsics_for(H, W):
    """K_LONG for the rig's 1200 x 1600; otherwise a lens scaled so that the image spans the same field, with an off-centre
    principal point (values exact in float32)."""
    if (H, W) == (1200, 1600):
        return K_LONG
    f = np.float32(6.0 * max(H, W))
    return np.array([[f, 0, W / 2.0 + 0.25], [0, f * np.float32(0.9990234375), H / 2.0 - 0.375], [0, 0, 1]], dtype=np.float32)


def noise_image(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W), dtype=np.uint8)


def smooth_image(H, W, seed):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    ph = rng.uniform(0, 2 * np.pi, size=4)
    val = 127.5 + 60.0 * np.sin(i / 17.3 + ph[0]) * np.cos(j / 23.1 + ph[1]) + 55.0 * np.sin((i + j) / 41.7 + ph[2]) + 10.0 * np.sin(j / 3.3 + ph[3])
    return np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)


# The single-image cases of the bit-exact GPU test: (name, H, W, coefficient set, clip_max, flip_rows, image kind, seed).  Every size,
# coefficient set, clip, flip and image kind the check asks for appears; tests/test_undistort_ref.py checks each image's rounding margin.
GPU_CASES = [
    ('rig-noise-mild', 1200, 1600, 'mild', 140, True, 'noise', 11),
    ('rig-noise-strong', 1200, 1600, 'strong', 255, False, 'noise', 12),
    ('rig-smooth-strong', 1200, 1600, 'strong', 140, False, 'smooth', 13),
    ('hd-noise-mild', 1080, 1920, 'mild', 255, True, 'noise', 14),
    ('hd-smooth-tangential', 1080, 1920, 'tangential', 140, True, 'smooth', 15),
    ('hd-noise-zero', 1080, 1920, 'zero', 255, False, 'noise', 16),
    ('odd-noise-strong', 37, 53, 'strong', 255, True, 'noise', 17),
    ('odd-noise-tangential', 37, 53, 'tangential', 140, False, 'noise', 18),
    ('odd-smooth-mild', 37, 53, 'mild', 255, False, 'smooth', 19),
    ('odd-noise-zero', 37, 53, 'zero', 140, True, 'noise', 20),
    ('column-noise-strong', 5, 1, 'strong', 255, True, 'noise', 21),
    ('column-noise-tangential', 5, 1, 'tangential', 140, False, 'noise', 22),
]


def gpu_case_inputs(case):
    name, H, W, dset, clip_max, flip, kind, seed = case
    img = noise_image(H, W, seed) if kind == 'noise' else smooth_image(H, W, seed)
    return img, intrinsics_for(H, W), DIST[dset]


def batch_case():
    """The [3,9,H,W] batch with nine different camera rows: images, intr [9,3,3], dist [9,5]."""
    H, W = 120, 176
    rng = np.random.default_rng(31)
    images = rng.integers(0, 256, size=(3, 9, H, W), dtype=np.uint8)
    base = intrinsics_for(H, W)
    intr = np.stack([base + np.array([[8 * c, 0, 0.5 * c], [0, 6 * c, -0.25 * c], [0, 0, 0]], dtype=np.float32) for c in range(9)])
    dist = np.stack([np.array([4.0 * (c - 4), -40.0 * c, 1e-2 * (c % 3), -5e-3 * (c % 4), 10.0 * (c % 2)], dtype=np.float32) for c in range(9)])
    return images, intr, dist

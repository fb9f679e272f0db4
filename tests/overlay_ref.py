"""Numpy statement of the overlay rule ("Overlay rule"; include/fpcdr.h, fpcdr_overlay_u8), written for the test suite,
operation by operation; it imports nothing from the package (and no torch).  tests/test_overlay_ref.py checks the statement itself,
tests/test_gpu_overlay.py holds the kernel to it bit for bit.

    r   = flip_rows ? H-1-i : i                       (the flip applies to img, rast and rast_db, never to ref / out)
    q   = the Comparison rule's q of img[n,r,j]       (compare_ref.quantise)
    c   = ref[n,i,j]
    t   = w*q + (256-w)*c;  m = t >> 8;  rem = t & 255;  m += (rem > 128) | (rem == 128 & (m & 1))
    cov = rast given ? rast[n,r,j,3] > 0 : true
    if rast given and outside_capture and not cov:  m = c
    out[n,i,j,:] = (m, m, m)
    if hw2 > 0 and cov:
        u, v = rast[n,r,j,0:2];  ux, uy, vx, vy = rast_db[n,r,j,:]
        s = (1 - u) - v;  b2 = s < 0 ? 0 : s;  gx = ux + vx;  gy = uy + vy
        on(b, x, y) := b*b < hw2 * ((x*x) + (y*y))                 float32, unfused, in this order
        if on(u, ux, uy) or on(v, vx, vy) or on(b2, gx, gy):  out[n,i,j,:] = wire_rgb
"""
import numpy as np

from compare_ref import quantise

F32 = np.float32


def blend(q, c, w):
    """Integer blend of two uint8 arrays: (w*q + (256-w)*c) / 256 rounded half to even, w an integer in [0, 256]."""
    w = int(w)
    assert 0 <= w <= 256
    t = w * np.asarray(q).astype(np.int32) + (256 - w) * np.asarray(c).astype(np.int32)
    m = t >> 8
    rem = t & 255
    m = m + ((rem > 128) | ((rem == 128) & ((m & 1) == 1))).astype(np.int32)
    assert m.min(initial=0) >= 0 and m.max(initial=0) <= 255
    return m.astype(np.uint8)


def _on(b, x, y, hw2):
    """b*b < hw2 * ((x*x) + (y*y)) on float32 arrays with a float32 scalar hw2: every operation float32, a NaN compares false."""
    assert b.dtype == F32 and x.dtype == F32 and y.dtype == F32 and type(hw2) is F32
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        lhs = b * b
        rhs = hw2 * ((x * x) + (y * y))
        assert lhs.dtype == F32 and rhs.dtype == F32
        return lhs < rhs


def wire_mask(rast, rast_db, hw2):
    """[...] bool from rast [...,4] and rast_db [...,4] (float32): the wire test of a covered pixel (coverage is NOT applied here)."""
    rast, rast_db = np.asarray(rast), np.asarray(rast_db)
    assert rast.dtype == F32 and rast_db.dtype == F32
    hw2 = F32(hw2)
    u, v = rast[..., 0], rast[..., 1]
    ux, uy, vx, vy = (rast_db[..., k] for k in range(4))
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        s = (F32(1.0) - u) - v
        b2 = np.where(s < F32(0.0), F32(0.0), s)            # a select: a NaN stays a NaN
        gx = ux + vx
        gy = uy + vy
    assert s.dtype == F32 and b2.dtype == F32 and gx.dtype == F32
    return _on(u, ux, uy, hw2) | _on(v, vx, vy, hw2) | _on(b2, gx, gy, hw2)


def hw2_of(half_width):
    """The squared half width as ops.overlay_images forms it on the host."""
    return F32(half_width) * F32(half_width)


def overlay(img, ref, rast=None, rast_db=None, w=128, outside_capture=False, hw2=0.0, wire_rgb=(0, 255, 0), scale=255.0,
            flip_rows=False):
    """out [N,H,W,3] uint8 of the rule.  img [N,H,W] uint8 or float32, ref [N,H,W] uint8, rast / rast_db [N,H,W,4] float32 or None."""
    ref = np.asarray(ref)
    q = quantise(img, scale)
    assert ref.dtype == np.uint8 and q.shape == ref.shape and q.ndim == 3, (q.shape, ref.shape)
    hw2 = F32(hw2)
    assert np.isfinite(hw2) and hw2 >= 0
    assert not (hw2 > 0) or (rast is not None and rast_db is not None)
    assert not outside_capture or rast is not None
    if flip_rows:
        q = q[:, ::-1]
        rast = None if rast is None else np.asarray(rast)[:, ::-1]
        rast_db = None if rast_db is None else np.asarray(rast_db)[:, ::-1]
    m = blend(q, ref, w)
    if rast is not None:
        with np.errstate(invalid='ignore'):
            cov = np.asarray(rast)[..., 3] > F32(0.0)
    else:
        cov = np.ones(ref.shape, dtype=bool)
    if rast is not None and outside_capture:
        m = np.where(cov, m, ref)
    out = np.repeat(m[..., None], 3, axis=-1).astype(np.uint8)
    if hw2 > 0:
        wire = cov & wire_mask(rast, rast_db, hw2)
        out[wire] = np.asarray(wire_rgb, dtype=np.uint8)
    return out


# ---- inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
def float_image(N, H, W, rng):
    """[0,1]-range render for scale = 255: uniform in [-0.2, 1.2], with NaN, +-inf and exact halves (k + 0.5) / 255 planted."""
    img = rng.uniform(-0.2, 1.2, size=(N, H, W)).astype(F32)
    flat = img.reshape(-1)
    pick = rng.uniform(size=flat.size) < 0.2
    halves = ((rng.integers(0, 255, size=flat.size).astype(F32) + F32(0.5)) / F32(255.0)).astype(F32)
    flat[pick] = halves[pick]
    special = np.array([np.nan, np.inf, -np.inf, 0.5 / 255, 1.5 / 255, 2.5 / 255, 127.5 / 255, 254.5 / 255, 0.0, 1.0], dtype=F32)
    flat[:special.size] = special[:flat.size]
    return img


def raster_inputs(N, H, W, rng, db_scale=0.04):
    """(rast, rast_db) [N,H,W,4] float32: ids with ~40 % zeros; u uniform in [0,1], v = (1-u) * uniform (b2 reaches exact 0 and tiny
    negatives before the clamp); a few planted u = 0, v = 0, NaN; derivatives normal * db_scale (20-40 % of the covered pixels are
    wire at half width 0.5); uncovered pixels carry garbage in u, v and the derivatives, NaN and inf among it."""
    ids = rng.integers(1, 500, size=(N, H, W)).astype(F32)
    ids[rng.uniform(size=(N, H, W)) < 0.4] = 0.0
    u = rng.uniform(size=(N, H, W)).astype(F32)
    f = rng.uniform(size=(N, H, W)).astype(F32)
    f[rng.uniform(size=(N, H, W)) < 0.03] = 1.0             # v = 1 - u as float32 rounds it: b2 is 0 or a last-bit negative
    v = ((F32(1.0) - u) * f).astype(F32)
    db = (rng.normal(size=(N, H, W, 4)) * db_scale).astype(F32)
    flat_u, flat_v, flat_db, flat_id = u.reshape(-1), v.reshape(-1), db.reshape(-1, 4), ids.reshape(-1)
    n = flat_u.size
    plant = rng.integers(0, n, size=max(n // 30, 6))
    k = plant.size // 6
    flat_u[plant[:k]] = 0.0
    flat_v[plant[k:2 * k]] = 0.0
    flat_u[plant[2 * k:3 * k]] = np.nan
    flat_v[plant[3 * k:4 * k]] = np.nan
    flat_db[plant[4 * k:5 * k], rng.integers(0, 4, size=k)] = np.nan
    flat_db[plant[5 * k:6 * k], rng.integers(0, 4, size=plant[5 * k:6 * k].size)] = np.inf
    flat_id[plant[:6 * k]] = 7.0                             # the planted values are covered, so they are looked at
    # garbage off the mesh: it must not show; some of the empty ids are negative or NaN instead of 0
    off = flat_id == 0.0
    flat_id[off] = np.array([0.0, 0.0, 0.0, -0.0, -2.0, np.nan], dtype=F32)[rng.integers(0, 6, size=int(off.sum()))]
    garbage = np.array([np.nan, np.inf, -np.inf, 0.0, 1e30, -3.0, 0.25], dtype=F32)
    flat_u[off] = garbage[rng.integers(0, garbage.size, size=int(off.sum()))]
    flat_v[off] = garbage[rng.integers(0, garbage.size, size=int(off.sum()))]
    flat_db[off] = garbage[rng.integers(0, garbage.size, size=(int(off.sum()), 4))]
    rast = np.stack([u, v, rng.uniform(-1, 1, size=(N, H, W)).astype(F32), ids], axis=-1).astype(F32)
    return np.ascontiguousarray(rast), np.ascontiguousarray(db)

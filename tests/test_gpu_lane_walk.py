"""The lane walk of the bin rasteriser (bin_raster.h, bin_raster: one lane per small triangle, winners folded into the bin's LDS depth
buffer as 64-bit keys).  Its inner trip keeps a running float for the depth plane's x offset, a running LDS address that is also the
loop test, and a two-instruction depth key; this file pins what those may not change.  Every comparison is exact: ids against the CPU
oracle's rasteriser, through fpcdr_rasterize_fwd (k_bins), through the id planes of fpcdr_objective_fwd (the list kernels; with
and without per-bin triangle lists) and through fpcdr_render_fwd of the two-call library (the same raster phase under that library's own
read-out), whose rast must also equal fpcdr_rasterize_fwd's bit for bit.

Scenes are hand-built in pixel coordinates (w = 1 or 2, so that z / w is the z written down) with a random soup mixed in:
  depth keys   planes at z = w and z = -w (kept), one ulp beyond each (dropped), +0.0 against -0.0 under both index orders, several
               negative depths, coincident duplicates (rule R6);
  box shapes   boxes 1, 2, 3, 31 and 32 pixels wide and 1, 2 and 5 high, inside a bin, across its right and top edges and across the
               border of an image whose sides are no multiples of 32 (72 x 80 -- the other scenes are 64 x 64 or 96 x 96), in bins of
               <= 64 and of 65..128 triangles (4 and 2 lanes per triangle: a box of 1 or 2 rows leaves lanes without a row);
  batch sizes  1, 64, 65, 128, 129, 256 and 300 triangles in ONE bin (4 / 2 / 1 lanes per triangle, a second batch), in image 1 with
               one of them larger than LANE_MAX, so that lane path and tile path meet in one depth buffer;
  float range  slivers at the 16384 sub-pixel extent limit whose anchor vertex lies 64 pixels outside the bin their tip is walked in,
               in nearly coplanar pairs whose winner changes along a line through the tip: a depth that is one ulp off moves that line.
               rast[..., 2] is compared bit for bit with the oracle's as well.
The oracle's own image is checked first for every scene: pixels are covered, and the triangles a case is about show (or do not)."""
import numpy as np
import pytest
import torch

from helpers import random_soup
from objective_call import objective_ids

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ scene building (CPU)

def _pos_from_pixels(tris, res, w=None):
    """tris [B,T,3,3] float64 (x, y in pixels with pixel centres at i + 0.5, z = z / w) -> pos [B,3T,4] float32, tri [T,3]."""
    H, W = res
    tris = torch.as_tensor(tris, dtype=torch.float64)
    B, T = tris.shape[:2]
    w = torch.ones(B, T, 3, 1, dtype=torch.float64) if w is None else torch.as_tensor(w, dtype=torch.float64).reshape(B, T, 1, 1).expand(B, T, 3, 1)
    x = 2.0 * tris[..., 0:1] / W - 1.0
    y = 2.0 * tris[..., 1:2] / H - 1.0
    pos = torch.cat([x * w, y * w, tris[..., 2:3] * w, w], -1).reshape(B, 3 * T, 4).to(torch.float32).contiguous()
    return pos, torch.arange(3 * T, dtype=torch.int32).reshape(T, 3)


def _flat(x0, y0, sx, sy, z):
    """A right triangle with legs sx, sy at (x0, y0), constant depth z."""
    return [[x0, y0, z], [x0 + sx, y0, z], [x0, y0 + sy, z]]


def _with_soup(tris, res, seed, n=120, size=0.15, w=None):
    """Hand-built triangles FIRST (their indices are what the cases talk about), a random soup behind them."""
    pos, tri = _pos_from_pixels(tris, res, w)
    sp, _ = random_soup(pos.shape[0], n, seed, size=size)
    pos = torch.cat([pos, sp], 1).contiguous()
    return pos, torch.arange(pos.shape[1], dtype=torch.int32).reshape(-1, 3)


def _shown(ids, t):
    return int((ids == t + 1).sum())


# ------------------------------------------------------------------------------------------------ the three GPU paths

def _gpu_rast(pos, tri, res):
    import fpc_diffrend_amd.ops as dr
    ctx = dr.RasterizeGLContext(device='cuda')
    rast, _ = dr.rasterize(ctx, pos.cuda(), tri.cuda(), res)
    return rast.cpu()


def _gpu_rast_twocall(pos, tri, res):
    """rast of ops.render_textured (fpcdr_render_fwd, dense form): a 4 x 4 one-channel texture, uv_tri = tri."""
    import fpc_diffrend_amd.ops as dr
    ctx = dr.RasterizeGLContext(device='cuda')
    g = torch.Generator().manual_seed(3)
    uv = torch.rand(pos.shape[1], 2, generator=g).cuda()
    tex = torch.rand(4, 4, 1, generator=g).cuda()
    _, rast = dr.render_textured(ctx, pos.cuda(), tri.cuda(), uv, tri.cuda(), tex, res)
    return rast.cpu()


def _check_exact(pos, tri, res, ids_ref):
    assert int((ids_ref > 0).sum()) > 0, "the oracle's image is empty"
    rast = _gpu_rast(pos, tri, res)
    assert torch.equal(rast[..., 3].to(torch.int32), ids_ref), "fpcdr_rasterize_fwd: ids differ from the oracle"
    for bin_lists in (True, False):
        assert torch.equal(objective_ids(pos, tri, res, bin_lists), ids_ref), f"fpcdr_objective_fwd (bin lists: {bin_lists}): ids differ from the oracle"
    rast_tc = _gpu_rast_twocall(pos, tri, res)
    assert torch.equal(rast_tc[..., 3].to(torch.int32), ids_ref), "fpcdr_render_fwd: ids differ from the oracle"
    assert torch.equal(rast_tc[..., :3].contiguous().view(torch.int32), rast[..., :3].contiguous().view(torch.int32)), \
        "fpcdr_render_fwd: rast[..., :3] differs from fpcdr_rasterize_fwd's"
    return rast


# ------------------------------------------------------------------------------------------------ depth keys

UP1, DN1 = float(np.nextafter(np.float32(1.0), np.float32(2.0))), float(np.nextafter(np.float32(-1.0), np.float32(-2.0)))
# index of each hand-built triangle of the depth-key scene
K_PLUS1, K_MINUS1, K_OVER, K_UNDER, K_BACK, K_PZ_A, K_NZ_A, K_NZ_B, K_PZ_B = range(9)
K_NEG = (9, 10, 11, 12)
K_DUP = (13, 14, 15, 16)


def _depth_key_scene(shift):
    s = 12.0
    t = [None] * 17
    t[K_PLUS1] = _flat(2.25, 2.25, s, s, 1.0)                 # z = w: d = +1 exactly, kept (nothing behind it)
    t[K_MINUS1] = _flat(18.25, 2.25, s, s, -1.0)              # z = -w: d = -1, kept, in front of everything
    t[K_OVER] = _flat(34.25, 2.25, s, s, UP1)                 # one ulp beyond +1: dropped
    t[K_UNDER] = _flat(48.25, 2.25, s, s, DN1)                # one ulp beyond -1: dropped
    t[K_BACK] = _flat(33.25, 1.25, 14.0, 14.0, 0.75)          # behind K_OVER: shows through the dropped triangle
    t[K_PZ_A] = _flat(2.25, 18.25, s, s, 0.0)                 # +0.0 under the smaller index ...
    t[K_NZ_A] = _flat(5.25, 20.25, s, s, -0.0)                # ... against -0.0: a tie
    t[K_NZ_B] = _flat(20.25, 18.25, s, s, -0.0)               # -0.0 under the smaller index ...
    t[K_PZ_B] = _flat(23.25, 20.25, s, s, 0.0)                # ... against +0.0
    for i, (k, z) in enumerate(zip(K_NEG, (-0.25, -0.875, -0.5, -0.125))):                      # order among negative depths
        t[k] = _flat(36.25 + 3.0 * i, 18.25 + 2.0 * i, s, s, z)
    a = [[3.25, 36.25, -0.3], [17.25, 38.25, 0.4], [6.25, 50.25, 0.1]]                          # sloped planes, twice each (R6)
    b = [[22.25, 35.25, 0.6], [35.25, 37.25, -0.7], [27.25, 49.25, 0.2]]
    t[K_DUP[0]], t[K_DUP[1]], t[K_DUP[2]], t[K_DUP[3]] = a, b, b, a
    tris = torch.tensor(t, dtype=torch.float64)
    tris[..., 0] += shift[0]
    tris[..., 1] += shift[1]
    return tris


def test_depth_keys(oracle_ops):
    res = (64, 64)
    tris = torch.stack([_depth_key_scene((0.0, 0.0)), _depth_key_scene((3.5, 1.25))])
    w = torch.ones(2, 17)
    w[1] = 2.0                      # (z = w and z = -w with w = 2: the products and quotients stay exact)
    pos, tri = _with_soup(tris, res, seed=21, n=60, size=0.12, w=w)
    pos[:, 17 * 3:, 2] = 0.05 * pos[:, 17 * 3:, 2] + 0.9 * pos[:, 17 * 3:, 3]     # the soup: z / w in 0.9 +- 0.045, behind all but K_PLUS1
    ids = oracle_ops.rasterize_ids(pos, tri, res)
    for b in range(2):
        im = ids[b]
        assert _shown(im, K_PLUS1) > 20 and _shown(im, K_MINUS1) > 20
        assert _shown(im, K_OVER) == 0 and _shown(im, K_UNDER) == 0 and _shown(im, K_BACK) > 20
        for first, second in ((K_PZ_A, K_NZ_A), (K_NZ_B, K_PZ_B)):
            assert _shown(im, first) > 20 and _shown(im, second) > 5, "both triangles of a +0 / -0 tie must show somewhere"
        for k in K_NEG:
            assert _shown(im, k) > 5
        assert _shown(im, K_DUP[0]) > 20 and _shown(im, K_DUP[1]) > 20 and _shown(im, K_DUP[2]) == 0 and _shown(im, K_DUP[3]) == 0
        # the tie rule, stated directly: a pixel inside both triangles of a +0 / -0 pair shows the smaller index
        for first, (x, y) in ((K_PZ_A, (7, 22)), (K_NZ_B, (25, 22))):
            x, y = x + (3 if b else 0), y + (1 if b else 0)
            assert int(im[y, x]) == first + 1
    _check_exact(pos, tri, res, ids)


# ------------------------------------------------------------------------------------------------ box shapes

def _thin(x0, y0, k, h, g):
    """A triangle whose pixel box is k wide and h high with its lower-left pixel at (x0, y0); random depths."""
    z = (torch.rand(3, generator=g, dtype=torch.float64) * 1.6 - 0.8).tolist()
    return [[x0 + 0.25, y0 + 0.25, z[0]], [x0 + k - 0.25, y0 + 0.3, z[1]], [x0 + 0.5 * k, y0 + h - 0.25, z[2]]]


def _box_scene(res, seed):
    """Image 0 / 1: the same boxes at two offsets.  Bin (0, 0) holds <= 64 triangles (4 lanes each), bin (1, 0) 65..128 (2 lanes each);
    boxes straddle x = 32, y = 32 and the image's right and top borders."""
    H, W = res
    g = torch.Generator().manual_seed(seed)
    t = []
    widths, heights = (1, 2, 3, 31, 32), (1, 2, 5)
    for j, h in enumerate(heights):                                       # bin (0, 0): 15 boxes inside it
        for i, k in enumerate(widths):
            t.append(_thin(0 if k >= 31 else 2 + 5 * i, 1 + 10 * j + 2 * i, k, h, g))
    n_sparse = len(t)
    for j, h in enumerate(heights):                                       # bin (1, 0): the same shapes + filler, 65..128 in all
        for i, k in enumerate(widths):
            t.append(_thin(32 if k >= 31 else 34 + 5 * i, 1 + 10 * j + 2 * i, k, h, g))
    for i in range(70):
        t.append(_thin(33 + (i % 14) * 2, 3 + (i // 14) * 5, 1 + i % 3, 1 + (i // 3) % 3, g))
    n_mid = len(t)
    for i, k in enumerate(widths):                                        # across the bin's right edge (x = 32) and its top edge (y = 32)
        t.append(_thin(32 - (k + 1) // 2, 33 + 5 * i, k + 1, 2, g))
        t.append(_thin(1 + 3 * i if k < 31 else 0, 31 - (i % 2), min(k, 30), 3, g))
    for i, k in enumerate(widths):                                        # across the image's right and top borders
        t.append(_thin(W - (k + 1) // 2 - (1 if k >= 31 else 0), 34 + 5 * i, k + 1, 1 + i % 3, g))
        t.append(_thin(W - 33 + i if k >= 31 else 40 + 4 * i, H - 1 - (i % 2), k, 4, g))
    tris = torch.tensor(t, dtype=torch.float64)
    shifted = tris.clone()
    shifted[n_mid:, 0] += 0.5                                             # image 1: the edge cases half a pixel further
    return torch.stack([tris, shifted]), n_sparse, n_mid


@pytest.mark.parametrize("res", [(96, 96), (72, 80)])
def test_box_shapes(oracle_ops, res):
    tris, n_sparse, n_mid = _box_scene(res, seed=5)
    assert n_sparse <= 64 and 65 <= n_mid - n_sparse <= 128
    pos, tri = _pos_from_pixels(tris, res)
    ids = oracle_ops.rasterize_ids(pos, tri, res)
    T = tri.shape[0]
    seen = torch.unique(ids[ids > 0])
    assert len(seen) > 0.6 * T, "most boxes must show at least one pixel"
    assert int((ids[:, :, res[1] - 1] > 0).sum()) > 0 and int((ids[:, res[0] - 1, :] > 0).sum()) > 0, "the image's last column and row are covered"
    assert int((ids[:, 32:64, 31] > 0).sum()) > 0 and int((ids[:, 32:64, 32] > 0).sum()) > 0, "both sides of a bin's right edge are covered"
    assert int((ids[:, 31, :32] > 0).sum()) > 0 and int((ids[:, 32, :32] > 0).sum()) > 0, "both sides of a bin's top edge are covered"
    _check_exact(pos, tri, res, ids)
    # ... and with a soup mixed in (more triangles per bin, overdraw on the thin boxes)
    pos, tri = _with_soup(tris, res, seed=8, n=150, size=0.1)
    _check_exact(pos, tri, res, oracle_ops.rasterize_ids(pos, tri, res))


# ------------------------------------------------------------------------------------------------ batch sizes in one bin

@pytest.mark.parametrize("n", [1, 64, 65, 128, 129, 256, 300])
def test_batch_sizes_in_one_bin(oracle_ops, n):
    """n triangles, every box inside bin (1, 1) of a 96 x 96 image.  Image 1: the last of them has a box of 24 x 24 pixels
    (> LANE_MAX = 256): it takes the tile path, the others the lane path, into the same depth buffer."""
    res = (96, 96)
    g = torch.Generator().manual_seed(1000 + n)
    c = 35.0 + torch.rand(n, 1, 2, generator=g, dtype=torch.float64) * 22.0
    xy = c + torch.rand(n, 3, 2, generator=g, dtype=torch.float64) * 5.5
    z = torch.round((torch.rand(n, 3, 1, generator=g, dtype=torch.float64) * 1.8 - 0.9) * 16) / 16      # many exact depth ties
    z[::5] = z[::5, :1]
    small = torch.cat([xy, z], -1)
    assert float(xy.min()) > 32.6 and float(xy.max()) < 63.4
    mixed = small.clone()
    mixed[n - 1] = torch.tensor([[34.25, 34.25, 0.1], [58.25, 36.25, -0.2], [40.25, 58.25, 0.3]], dtype=torch.float64)
    pos, tri = _pos_from_pixels(torch.stack([small, mixed]), res)
    ids = oracle_ops.rasterize_ids(pos, tri, res)
    assert int((ids[0] > 0).sum()) > 0 and int((ids[1] > 0).sum()) > 0
    assert _shown(ids[1], n - 1) > 0, "the large triangle shows"
    if n > 1:
        assert len(torch.unique(ids[1][ids[1] > 0])) > 1, "small triangles show beside the large one"
    outside = ids.clone()
    outside[:, 32:64, 32:64] = 0
    assert int(outside.sum()) == 0, "every triangle lies in bin (1, 1)"
    _check_exact(pos, tri, res, ids)


# ------------------------------------------------------------------------------------------------ range of the running float

def test_float_range_at_the_extent_limit(oracle_ops):
    """Slivers of 64 x 64 pixels extent (16384 sub-pixel units, the limit of the 32-bit class; exact in a 64 x 64 image, whose
    sub-pixel grid is a power of two) from an anchor vertex at (-28.5, -28.5) and thereabouts to a tip just inside bin (1, 1): there
    the box is a few pixels (lane path) and the offsets from the anchor are 60..64 pixels; in bin (0, 0) the same triangle fills the
    box (tile path).  Each sliver comes twice, the second copy's plane tilted by a few float steps about a line through the tip, so
    the winner changes inside the tip's box."""
    res = (64, 64)
    H, W = res
    per_image = []
    for b, (ox, oy) in enumerate(((0.0, 0.0), (0.75, 0.5))):
        t = []
        for i in range(6):
            a = (-28.5 + ox - 0.25 * i, -28.5 + oy + 0.5 * i)
            dx, dy = 61.0 - 0.5 * i, 60.0 + 0.25 * i
            z0, z1, z2 = 0.9 - 0.1 * i, -0.85 + 0.05 * i, -0.8 + 0.03 * i
            t.append([[a[0], a[1], z0], [a[0] + 64.0, a[1] + dy, z1], [a[0] + dx, a[1] + 64.0, z2]])
            e = 3e-6 * (i + 1)
            t.append([[a[0], a[1], z0], [a[0] + 64.0, a[1] + dy, z1 - e], [a[0] + dx, a[1] + 64.0, z2 + e]])
        per_image.append(t)
    tris = torch.tensor(per_image, dtype=torch.float64)
    pos, tri = _with_soup(tris, res, seed=31, n=40, size=0.1)
    pos[:, 36:, 2] = 0.95 * pos[:, 36:, 3]                                # the soup: behind the slivers
    # the extent is at the limit, not beyond it: snapped as the set-up kernel snaps (rule R2)
    X = torch.floor((pos[:, :36, 0].double() / pos[:, :36, 3].double() * 0.5 + 0.5) * (W * 256) + 0.5).reshape(2, 12, 3)
    assert int((X.max(-1).values - X.min(-1).values).max()) == 16384
    ids, depth = oracle_ops.rasterize_ids(pos, tri, res, return_depth=True)
    tip = ids[:, 32:40, 32:40]
    for b in range(2):
        shown = set(torch.unique(tip[b][tip[b] > 0]).tolist())
        assert len(shown & set(range(1, 13))) >= 4, "several slivers show in the tip's bin"
        assert any(2 * i + 1 in shown and 2 * i + 2 in shown for i in range(6)), "both copies of a sliver show in the tip: the winner changes there"
    rast = _check_exact(pos, tri, res, ids)
    r_ref, _ = oracle_ops.rasterize(pos, tri, res)
    zg, zr = rast[..., 2].contiguous().view(torch.int32), r_ref[..., 2].detach().contiguous().view(torch.int32)
    assert torch.equal(zg, zr), f"rast[..., 2] differs from the oracle's in {int((zg != zr).sum())} of {int((ids > 0).sum())} covered pixels"

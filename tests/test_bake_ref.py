"""CPU: the numpy statement of the Bake rule (tests/bake_ref.py) is itself checked -- its weights exhaustively, a constant capture, the
float64 adjoint of the oracle's texture operator, hand-made arrays for every clause of the rule, and the stake end to end on the oracle
-- so that the bit-exact comparison of the kernels against it (tests/test_gpu_bake.py) means something.  Plus the binding."""
import os
import re

import numpy as np
import pytest
import torch

import bake_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- 1. the weights ----------------------------------------------------------------------------------------------------------------------
def test_weights_exhaustively():
    """ax, ay in 0..256: four weights >= 0 that sum to 65536.  For fx at both ends of its bucket [ax / 256, (ax + 1) / 256) -- the lower
    end and the last float32 below the upper one; ax = 256 is fx = 1 alone -- |w_k / 65536 - float product| <= 2/256: |ax / 256 - fx| <
    1/256 per factor, both factors <= 1, so the product moves by less than 1/256 + 1/256."""
    ax, ay = np.meshgrid(np.arange(257), np.arange(257), indexing='ij')
    w = R.weights(ax, ay)
    assert all((wk >= 0).all() for wk in w) and np.all(w[0] + w[1] + w[2] + w[3] == 65536)
    lo = (np.arange(257) / 256.0).astype(F32)
    hi = np.nextafter(((np.arange(257) + 1) / 256.0).astype(F32), F32(0.0))
    hi[256] = F32(1.0)
    assert np.array_equal(R.quantise_fraction(lo), np.arange(257)) and np.array_equal(R.quantise_fraction(hi), np.arange(257))
    worst = 0.0
    for fx in (lo, hi):
        for fy in (lo, hi):
            gx, gy = np.meshgrid(fx.astype(np.float64), fy.astype(np.float64), indexing='ij')
            prod = ((1 - gx) * (1 - gy), gx * (1 - gy), (1 - gx) * gy, gx * gy)
            for wk, pk in zip(w, prod):
                worst = max(worst, float(np.abs(wk / 65536.0 - pk).max()))
    print(f"largest |w / 65536 - product|: {worst:.6f} (bound {2 / 256:.6f})")
    assert worst <= 2.0 / 256


# ---- the oracle scene of 2, 3 and 5 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_scene(oracle_ops):
    """make_scene(resolution=(96, 96), texshape=(64, 64, 1), n_frames=2), cameras 0, 4 and 8 at the true geometry, through the oracle:
    rast and texc as float32 numpy, the 8-bit captures (the hidden texture rendered, clipped to [0, 140]) and what renders a texture."""
    from fpc_diffrend_amd import scene
    from oracle import fit as ofit
    sc = scene.make_scene(resolution=(96, 96), texshape=(64, 64, 1), n_frames=2)
    gt = ofit.State(sc, cams=[0, 4, 8])
    with torch.no_grad():
        gt.M1.copy_(torch.eye(2))
        gt.M2.copy_(torch.tensor(sc.weights_gt).t())
        gt.per_frame_t.copy_(torch.tensor(sc.t_gt))
        gt.per_frame_q.copy_(torch.tensor(sc.q_gt))
        pos_clip, _ = ofit.clip_positions(gt, torch.arange(2))
        rast, _ = oracle_ops.rasterize(pos_clip, gt.pos_idx, (96, 96))
        texc, _ = oracle_ops.interpolate(gt.uv[None], rast, gt.uv_idx)
        _, img, _ = ofit.forward_from_clip(gt, pos_clip, torch.zeros(6, 96, 96, dtype=torch.uint8))
        targets = torch.clamp(torch.round(img[..., 0] * 255), 0, 140).to(torch.uint8)

    def loss_of(texture):
        st = ofit.State(sc, cams=[0, 4, 8], texture=np.asarray(texture, dtype=F32).reshape(64, 64, 1))
        with torch.no_grad():
            return float(ofit.forward_from_clip(st, pos_clip, targets)[0])

    return dict(sc=sc, rast=rast.numpy(), texc=texc.numpy(), targets=targets.numpy(), loss_of=loss_of, ops=oracle_ops)


def test_constant_capture_resolves_to_the_constant(oracle_scene):
    """c = 77 everywhere: num = 77 den at every texel, so every filled texel is float32(77 / 255) exactly -- (double)(77 den) /
    ((double)den * 255) is the correctly rounded quotient of two exact doubles with the exact value 77 / 255 -- and the sum of den is
    65536 x the number of contributing pixels."""
    s = oracle_scene
    ref = np.full(s['targets'].shape, 77, dtype=np.uint8)
    acc = R.accumulate(s['texc'], s['rast'], ref, np.zeros((64, 64, 2), dtype=np.uint64))
    tex, filled = R.resolve(acc)
    n_px = int(R.contributes(s['texc'], s['rast']).sum())
    print(f"contributing pixels {n_px}, den sum {int(acc[..., 1].sum())}, filled texels {int(filled.sum())} of {filled.size}")
    assert n_px > 5000 and filled.sum() > 1000
    assert int(acc[..., 1].sum()) == 65536 * n_px
    assert np.array_equal(acc[..., 0], acc[..., 1] * np.uint64(77))
    assert np.all(tex[filled] == F32(77.0 / 255.0)) and np.all(tex[~filled] == 0)


def test_accumulator_against_float64_autograd(oracle_scene):
    """The adjoint of the oracle's texture operator (float64 texels, the float32 coordinates) for the gradient `capture on covered
    pixels` is the unquantised numerator.  Per texel |num / 65536 - adjoint| <= (2/256) * sum of c over the (pixel, tap) pairs that
    reach it (test 1's bound per pair).  Measured: largest deviation 2.91 at an adjoint of 1105.2 (bound there 32.2); largest
    deviation / bound 0.60."""
    s = oracle_scene
    O = s['ops']
    texc, rast, ref = s['texc'], s['rast'], s['targets']
    acc = R.accumulate(texc, rast, ref, np.zeros((64, 64, 2), dtype=np.uint64))
    tex = torch.zeros(1, 64, 64, 1, dtype=torch.float64, requires_grad=True)
    out = O.texture(tex, torch.from_numpy(texc), filter_mode='linear', boundary_mode='wrap')
    g = torch.from_numpy(np.where(R.contributes(texc, rast), ref, 0).astype(np.float64))[..., None]
    out.backward(g)
    adjoint = tex.grad[0, :, :, 0].numpy()
    texel, w, c = R.contributions(texc, rast, ref, 64, 64)
    reach = np.zeros(64 * 64, dtype=np.float64)
    for k in range(4):
        np.add.at(reach, texel[:, k], c.astype(np.float64))
    bound = (2.0 / 256) * reach.reshape(64, 64)
    dev = np.abs(acc[..., 0].astype(np.float64) / 65536.0 - adjoint)
    at = np.unravel_index(np.argmax(dev), dev.shape)
    print(f"largest deviation {dev[at]:.3f} at an adjoint of {adjoint[at]:.1f} (bound there {bound[at]:.3f}); "
          f"largest deviation / bound {float((dev / np.maximum(bound, 1e-300))[bound > 0].max()):.3f}")
    assert adjoint.max() > 1000
    assert np.all(dev <= bound)
    # and the denominators against the gradient 1
    tex.grad = None
    out = O.texture(tex, torch.from_numpy(texc), filter_mode='linear', boundary_mode='wrap')
    out.backward(torch.from_numpy(R.contributes(texc, rast).astype(np.float64))[..., None])
    count = np.zeros(64 * 64)
    for k in range(4):
        np.add.at(count, texel[:, k], 1.0)
    assert np.all(np.abs(acc[..., 1].astype(np.float64) / 65536.0 - tex.grad[0, :, :, 0].numpy()) <= (2.0 / 256) * count.reshape(64, 64))


# ---- 4. hand-made arrays -----------------------------------------------------------------------------------------------------------------
def _one_pixel(u, v, w=1.0, c=100, Ht=4, Wt=4, mode='wrap', **kw):
    texc = np.array([[[[u, v]]]], dtype=F32)
    rast = np.array([[[[0.2, 0.3, 0.5, w]]]], dtype=F32)
    return R.accumulate(texc, rast, np.array([[[c]]], dtype=np.uint8), np.zeros((Ht, Wt, 2), dtype=np.uint64), mode, **kw)


def test_accumulate_one_pixel_by_hand():
    # a texel centre: all the weight on one texel
    acc = _one_pixel(2.5 / 4, 1.5 / 4)
    assert acc[1, 2].tolist() == [65536 * 100, 65536] and int(acc[..., 1].sum()) == 65536 and np.count_nonzero(acc[..., 1]) == 1
    # a texel corner: a quarter each
    acc = _one_pixel(2.0 / 4, 1.0 / 4)
    for y, x in ((0, 1), (0, 2), (1, 1), (1, 2)):
        assert acc[y, x].tolist() == [16384 * 100, 16384]
    # fx = 1/4 + 1/1024: ax = 64 (the quantisation drops the 1/1024), fy = 1/2
    acc = _one_pixel((1.5 + 0.25 + 1 / 1024) / 4, 2.0 / 4)
    assert [acc[1, 1, 1], acc[1, 2, 1], acc[2, 1, 1], acc[2, 2, 1]] == [192 * 128, 64 * 128, 192 * 128, 64 * 128]
    # uncovered (0, negative, NaN), NaN / +-inf coordinates: nothing
    for kw in (dict(w=0.0), dict(w=-1.0), dict(w=np.nan)):
        assert not _one_pixel(0.3, 0.3, **kw).any()
    for u, v in ((np.nan, 0.3), (0.3, np.nan), (np.inf, 0.3), (0.3, -np.inf)):
        for mode in ('wrap', 'clamp'):
            assert not _one_pixel(u, v, mode=mode).any()
    # c = 0 adds weight and no colour
    acc = _one_pixel(2.5 / 4, 1.5 / 4, c=0)
    assert acc[1, 2].tolist() == [0, 65536]


def test_accumulate_boundary_modes_outside_the_unit_square():
    # u = 1.125 on 4 texels: wrap -> 0.125, x = 0: texel 0 alone; clamp -> 1, x = 3.5: texels 3 and 3 (both taps name it, both add)
    acc = _one_pixel(1.125, 0.375, mode='wrap')
    assert acc[1, 0].tolist() == [65536 * 100, 65536] and np.count_nonzero(acc[..., 1]) == 1
    acc = _one_pixel(1.125, 0.375, mode='clamp')
    assert acc[1, 3].tolist() == [65536 * 100, 65536] and np.count_nonzero(acc[..., 1]) == 1
    # u = 0.0625: x = -0.25: wrap -> texels 3 (1/4) and 0 (3/4); clamp -> texel 0 twice
    acc = _one_pixel(0.0625, 0.375, mode='wrap')
    assert acc[1, 3, 1] == 16384 and acc[1, 0, 1] == 49152
    acc = _one_pixel(0.0625, 0.375, mode='clamp')
    assert acc[1, 0, 1] == 65536 and np.count_nonzero(acc[..., 1]) == 1
    # u = -0.25: wrap -> 0.75, x = 2.5; clamp -> 0, x = -0.5: texel 0 with both halves
    assert _one_pixel(-0.25, 0.375, mode='wrap')[1, 2, 1] == 32768
    assert _one_pixel(-0.25, 0.375, mode='clamp')[1, 0, 1] == 65536
    # u - floor(u) rounds to 1.0f: x = 3.5, the second tap wraps to texel 0
    acc = _one_pixel(-1e-9, 0.375, mode='wrap')
    assert acc[1, 3, 1] == 32768 and acc[1, 0, 1] == 32768
    # one texel: every tap is it, the weights sum to 65536 whatever the coordinate
    for mode in ('wrap', 'clamp'):
        assert _one_pixel(0.3, 1.7, Ht=1, Wt=1, mode=mode)[0, 0].tolist() == [65536 * 100, 65536]


def _pixels(cover):
    """A batch of one image from a coverage map: every pixel at the centre of texel (1, 2) of a 4 x 4 texture, capture = 10 * i + j."""
    cover = np.asarray(cover, dtype=F32)
    H, W = cover.shape
    texc = np.empty((1, H, W, 2), dtype=F32)
    texc[..., 0], texc[..., 1] = 2.5 / 4, 1.5 / 4
    rast = np.zeros((1, H, W, 4), dtype=F32)
    rast[0, :, :, 3] = cover
    ref = (10 * np.arange(H)[:, None] + np.arange(W)[None, :]).astype(np.uint8)[None]
    return texc, rast, ref


def test_interior_only_and_flip_rows():
    full = np.ones((3, 4))
    texc, rast, ref = _pixels(full)
    z = lambda: np.zeros((4, 4, 2), dtype=np.uint64)
    # a fully covered image: the image border does not make a pixel a silhouette pixel
    acc = R.accumulate(texc, rast, ref, z(), interior_only=True)
    assert acc[1, 2].tolist() == [65536 * int(ref.sum()), 65536 * 12]
    # a hole at (1, 1) takes itself and its four neighbours out; the diagonal ones stay
    hole = full.copy()
    hole[1, 1] = 0
    texc, rast, ref = _pixels(hole)
    acc = R.accumulate(texc, rast, ref, z(), interior_only=True)
    kept = [(0, 0), (0, 2), (0, 3), (1, 3), (2, 0), (2, 2), (2, 3)]
    assert acc[1, 2].tolist() == [65536 * sum(10 * i + j for i, j in kept), 65536 * len(kept)]
    assert R.accumulate(texc, rast, ref, z())[1, 2, 1] == 65536 * 11
    # a NaN in rast.w is a hole as well
    rast[0, 1, 1, 3] = np.nan
    assert np.array_equal(R.accumulate(texc, rast, ref, z(), interior_only=True), acc)
    # flip_rows: raster row i takes the capture's row H - 1 - i; coverage and coordinates stay where they are
    cover = np.zeros((3, 4))
    cover[0, 1] = 1
    texc, rast, ref = _pixels(cover)
    assert R.accumulate(texc, rast, ref, z())[1, 2, 0] == 65536 * 1
    assert R.accumulate(texc, rast, ref, z(), flip_rows=True)[1, 2, 0] == 65536 * 21


def test_two_calls_equal_one_on_the_concatenation():
    a = R.grid_inputs(2, 5, 7, 5, 7, seed=1)
    b = R.grid_inputs(3, 5, 7, 5, 7, seed=2)
    for mode in ('wrap', 'clamp'):
        two = np.zeros((5, 7, 2), dtype=np.uint64)
        R.accumulate(*a, two, mode)
        R.accumulate(*b, two, mode)
        one = R.accumulate(*(np.concatenate([x, y]) for x, y in zip(a, b)), np.zeros((5, 7, 2), dtype=np.uint64), mode)
        assert np.array_equal(one, two) and one[..., 1].sum() > 0


def test_grid_inputs_hold_what_the_gpu_grid_needs():
    for (H, W) in ((48, 64), (5, 37), (3, 7)):
        for (Ht, Wt) in ((8, 8), (5, 7), (1, 1), (64, 32)):
            texc, rast, ref = R.grid_inputs(3, H, W, Ht, Wt, seed=H * 100 + W + Ht)
            w = rast[..., 3]
            assert np.isnan(w).any() and (w == 0).any() and (w < 0).any() and (w > 0).any()
            if H * W >= 48 * 64:
                assert np.isnan(texc).any() and np.isposinf(texc).any() and np.isneginf(texc).any()
                assert (texc == 0).any() and (texc == 1).any() and (texc < 0).any() and (texc > 1).any()
                texel, wts, _ = R.contributions(texc, rast, ref, Ht, Wt, 'wrap')
                assert (wts == 0).any() and (wts == 65536).any()          # exact centres among the covered pixels: skipped taps


def test_resolve_at_the_threshold():
    acc = np.zeros((1, 5, 2), dtype=np.uint64)
    acc[0, :, 1] = [0, 99, 100, 101, 1 << 41]
    acc[0, :, 0] = [0, 99 * 50, 100 * 50, 101 * 255, (1 << 41) * 140]
    tex, filled = R.resolve(acc, 255.0, 100)
    assert filled.tolist() == [[False, False, True, True, True]]
    assert tex[0].tolist() == [0.0, 0.0, float(F32(50 / 255)), 1.0, float(F32(140 / 255))]
    tex, filled = R.resolve(acc, 255.0, 1)
    assert filled.tolist() == [[False, True, True, True, True]] and tex[0, 0] == 0
    assert R.min_den_of(0.0) == 1 and R.min_den_of(1.0) == 65536 and R.min_den_of(1e-9) == 1 and R.min_den_of(0.25) == 16384
    with pytest.raises(AssertionError):
        R.resolve(acc, 255.0, 0)


def test_dilate_by_hand():
    tex = np.zeros((5, 5), dtype=F32)
    filled = np.zeros((5, 5), dtype=bool)
    tex[2, 2], filled[2, 2] = 0.75, True
    tex[0, 0] = 9.0                                   # an unfilled texel's value is never read
    for k in range(1, 4):                             # k passes reach Chebyshev distance k
        t, f = tex, filled
        for _ in range(k):
            t, f = R.dilate(t, f)
        yy, xx = np.mgrid[0:5, 0:5]
        want = np.maximum(np.abs(yy - 2), np.abs(xx - 2)) <= k
        assert np.array_equal(f, want) and np.all(t[want] == F32(0.75))
        assert np.all(t[~want] == tex[~want])
    # filled texels never change; the mean is over the filled neighbours only, in float32, in the stated order
    tex = np.array([[0.1, 0.0, 0.7], [0.0, 0.0, 0.0], [0.2, 0.0, 0.0]], dtype=F32)
    filled = tex > 0
    t, f = R.dilate(tex, filled)
    assert f.sum() == 8 and not f[2, 2] and np.array_equal(t[filled], tex[filled])      # (2, 2) has no filled neighbour
    assert t[1, 1] == ((F32(0.1) + F32(0.7)) + F32(0.2)) / F32(3.0)
    assert t[0, 1] == (F32(0.1) + F32(0.7)) / F32(2.0) and t[1, 0] == (F32(0.1) + F32(0.2)) / F32(2.0)
    assert t[1, 2] == F32(0.7) and t[2, 1] == F32(0.2) and t[2, 2] == 0
    # no wrap: a texel at the far border is not a neighbour
    tex = np.zeros((1, 5), dtype=F32)
    filled = np.zeros((1, 5), dtype=bool)
    tex[0, 0], filled[0, 0] = 0.5, True
    t, f = R.dilate(tex, filled)
    assert f.tolist() == [[True, True, False, False, False]]
    # nothing filled: nothing happens; holes get the hole value at the end of bake()
    acc = np.zeros((3, 3, 2), dtype=np.uint64)
    tex, filled = R.bake(acc, passes=4, hole_value=0.25)
    assert not filled.any() and np.all(tex == F32(0.25))
    acc[0, 0] = (65536 * 51, 65536)
    tex, filled = R.bake(acc, passes=1, hole_value=0.25)
    assert filled.sum() == 1 and np.all(tex[:2, :2] == F32(0.2)) and tex[2, 2] == F32(0.25) and tex[0, 2] == F32(0.25)


# ---- 5. the stake ------------------------------------------------------------------------------------------------------------------------
def test_baked_texture_beats_the_best_constant_on_the_oracle(oracle_scene):
    """The 96^2 / 64^2 / cameras (0, 4, 8) / frames (0, 1) scene at the true geometry, pixel loss of the oracle's forward (fit.py:579):
    the baked texture's is below that of the best constant texture, the mean covered capture.  Measured here: hidden texture 0.0175,
    baked 1.85, best constant 16.9, uniform noise 1018."""
    s = oracle_scene
    acc = R.accumulate(s['texc'], s['rast'], s['targets'], np.zeros((64, 64, 2), dtype=np.uint64))
    baked, filled = R.bake(acc)
    mean = float(s['targets'][R.contributes(s['texc'], s['rast'])].astype(np.float64).mean() / 255.0)
    losses = dict(hidden=s['loss_of'](s['sc'].texture), baked=s['loss_of'](baked), constant=s['loss_of'](np.full((64, 64), mean)),
                  noise=s['loss_of'](np.random.default_rng(0).uniform(size=(64, 64))))
    print("pixel losses:", {k: round(v, 4) for k, v in losses.items()}, f"filled {int(filled.sum())} of {filled.size}")
    assert losses['baked'] < losses['constant']


# ---- 6. the binding ----------------------------------------------------------------------------------------------------------------------
NAMES = ("fpcdr_bake_accumulate_u8", "fpcdr_bake_resolve", "fpcdr_bake_dilate")


def test_binding():
    """The three entries are declared in the header, bound in _lib.SYMBOLS and exported by the built library; the ABI version of the
    binding is the library's (the entries are pure additions: it stays what it was)."""
    from fpc_diffrend_amd import _lib
    header = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION == lib.fpcdr_abi_version()
    assert int(re.search(r"#define FPCDR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """The entries check their arguments on the host, so the rejections need no GPU (made-up addresses, never dereferenced)."""
    from fpc_diffrend_amd import _lib
    texc, rast, ref, acc, tex, fil, tex2, fil2 = (0x10000 * k for k in range(1, 9))
    good = (texc, rast, ref, acc, 2, 8, 12, 4, 4, 0, 0, 0)

    def variant(**kw):
        names = ("texc", "rast", "ref", "acc", "n", "H", "W", "Ht", "Wt", "mode", "interior", "flip")
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    for args, why in ((variant(texc=None), "null"), (variant(rast=None), "null"), (variant(ref=None), "null"), (variant(acc=None), "null"),
                      (variant(n=0), "sizes"), (variant(H=0), "sizes"), (variant(W=-1), "sizes"), (variant(Ht=0), "sizes"), (variant(Wt=0), "sizes"),
                      (variant(mode=2), "boundary_mode"), (variant(mode=-1), "boundary_mode"), (variant(acc=acc + 4), "8-byte"),
                      (variant(acc=acc + 1), "8-byte"), (variant(texc=texc + 2), "4-byte"), (variant(acc=rast + 16), "overlaps")):
        with pytest.raises(RuntimeError, match="fpcdr_bake_accumulate_u8.*" + why):
            _lib.call("fpcdr_bake_accumulate_u8", *args, None)
    for args, why in (((None, tex, fil, 4, 4, 255.0, 1), "null"), ((acc, None, fil, 4, 4, 255.0, 1), "null"), ((acc, tex, None, 4, 4, 255.0, 1), "null"),
                      ((acc, tex, fil, 0, 4, 255.0, 1), "sizes"), ((acc, tex, fil, 4, -4, 255.0, 1), "sizes"), ((acc, tex, fil, 4, 4, 255.0, 0), "min_den"),
                      ((acc + 4, tex, fil, 4, 4, 255.0, 1), "8-byte"), ((acc, acc + 8, fil, 4, 4, 255.0, 1), "overlap"),
                      ((acc, tex, fil, 4, 4, 0.0, 1), "color_scale"), ((acc, tex, fil, 4, 4, float('nan'), 1), "color_scale")):
        with pytest.raises(RuntimeError, match="fpcdr_bake_resolve.*" + why):
            _lib.call("fpcdr_bake_resolve", *args, None)
    for args, why in (((None, fil, tex2, fil2, 4, 4), "null"), ((tex, None, tex2, fil2, 4, 4), "null"), ((tex, fil, None, fil2, 4, 4), "null"),
                      ((tex, fil, tex2, None, 4, 4), "null"), ((tex, fil, tex2, fil2, 0, 4), "sizes"), ((tex, fil, tex2, fil2, 4, 0), "sizes"),
                      ((tex, fil, tex, fil2, 4, 4), "overlaps"), ((tex, fil, tex2, fil, 4, 4), "overlaps")):
        with pytest.raises(RuntimeError, match="fpcdr_bake_dilate.*" + why):
            _lib.call("fpcdr_bake_dilate", *args, None)


def test_bake_has_no_cpu_path():
    from fpc_diffrend_amd import ops
    z = torch.zeros
    with pytest.raises(ValueError, match="no CPU path"):
        ops.bake_accumulate(z(1, 4, 4, 2), z(1, 4, 4, 4), z(1, 4, 4, dtype=torch.uint8), z(4, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.bake_resolve(z(4, 4, 2, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.bake_accumulate(np.zeros((1, 4, 4, 2)), z(1, 4, 4, 4), z(1, 4, 4, dtype=torch.uint8), z(4, 4, 2, dtype=torch.int64))


def test_bake_kernels_have_no_private_segment():
    """a kernel with a private segment is dispatched several times slower.  The three kernels of bake.hip keep
    everything in registers and use no LDS; read from the built object (tests/codeobj.py)."""
    import codeobj
    recs = codeobj.kernels("bake.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = set()
    for name, private, lds in recs:
        for k in ("k_bake_accumulate", "k_bake_resolve", "k_bake_dilate"):
            if k in name:
                seen.add(k)
                assert private == 0, name
                assert lds == 0, name
    assert len(seen) == 3

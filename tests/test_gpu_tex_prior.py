"""GPU: the texture prior (csrc/tex_prior.hip k_tex_prior<C, VEC>, k_tex_prior_finish; fpcdr_tex_prior, ops.tex_prior_call,
fit.texture_prior, fit.chart_map, FitConfig.weight_tex_smooth / tex_smooth_scale / tex_smooth_weights / weight_tex_anchor /
tex_anchor_weights) entry by entry against float64 (tests/tex_prior_ref.py), and inside a Fitter: eager, under a captured graph, on the
second of two ranks, through a checkpoint.

The convention is tests/test_gpu_rest.py's and tests/test_gpu_motion.py's: the error of an output x with float64 reference r is
e = max_i |x_i - r_i| / S_i in units of u = 2^-24, S_i the sum of the absolute values of the terms of entry i (every subtraction charges
the absolute values of its operands: neighbouring texels cancel for real); entries with S_i = 0 have no term, must be exactly 0, and
their number must be the one the weights predict.  Every output -- part, the value, the gradient -- is a sum or a chain through a root
and a division: e <= 8 * e32 + 4, e32 the error of float32 torch on the CPU for the same expression against the same reference; beside
it the rel-L2 of the same outputs against float64 is held to the project's 1e-4.  Every line is printed as "TEXPRIOR case name e_gpu
e32 bound" (pytest -s).  The Charbonnier scale of a case is the median |t_p - t_q| of its live pairs, so both regimes occur.

Measured on an MI355X (units of u; the largest over the 327 cases of a row: 324 of the shapes {1x1, 1x5, 5x1, 2x2, 3x7, 64x64, 15x65,
17x63, 65x257} x C in {1, 3, 4} x with / without a scale x with / without the smoothness map x no anchor / an anchor / an anchor with
weights, one of 17x36x2 and two of 497x2050, more tiles than workgroups; the last column is the case that came closest to its own
bound).  The rel-L2 of the same outputs against float64, printed beside them, is at most 1.4e-7 (part), 1.2e-7 (value) and 1.1e-7
(gradient) over all cases, against the bar of 1e-4.  The whole file runs in 10 s there:

  output                 cases max e_gpu  max e32   closest to its bound (e_gpu / bound, case)
  part                     327      0.07     0.06   0.07 / 4.1  2x2x4/a
  value                    327      0.06     0.09   0.06 / 4.0  2x2x4/c/sw/a
  grad                     327      0.74     0.63   0.74 / 9.0  497x2050x3/c/sw/a/aw
  grad lazy                327      0.94     0.94   0.68 / 7.6  64x64x4/sw/a/aw
  grad eager_grad          327      0.94     0.94   0.68 / 7.6  64x64x4/sw/a/aw
  grad acc                 327      0.94     0.94   0.68 / 7.6  64x64x4/sw/a/aw

Chart (cfg1's UV mesh): 61 696 covered texels of 256 x 256, 63 616 after the dilation; 14 464 and 15 232 at 96 x 160; torch.equal to the
oracle's rasteriser with the numpy dilation.
Fitter (cfg1 at 128 x 128, cameras 0 and 3, three frames, init_near_truth(0.8), init_texture='truth'; W_S = 3e4 with 'chart', W_A = 1e5
against the anchor 0.9 t + 0.03 with a map that has zeros; "worst" is the largest error over the parameter tensors in units of its bar,
1e-4 (|g_on| + |g_off|) of that tensor, over three runs):
  case                       tex |g_on|   |g_off|   |g_term|   worst              l_on      l_off    l_term
  smooth, c = 0.1, chart     9.3022       2.5769    8.5873     2.6e-4 .. 2.9e-4   25.7039   4.2698   21.4341
  anchor                     5.0849       2.5769    4.2445     1.4e-4 .. 2.9e-4   6.47826   4.2698   2.20844
  both, L2                   12.337       2.5769    11.723     2.8e-4 .. 5.2e-4   29.2641   4.2698   24.9943
  rank 1 of 2, both / 2      6.5030       2.0233    5.9735     1.5e-4 .. 7.2e-4   15.7747   2.8237   12.9510
Captured steps (W_GRAPH_S = W_GRAPH_A = 1e3, twelve steps): eager and graphed losses 5.87116671, 4.23998833, 3.466277 .. 2.485768 both.
Weights at zero: the launches and everything a step computes before its backward are torch.equal to a Fitter built without the options;
the parameters after three steps are not torch.equal between two Fitters built WITHOUT the options either (the pixel term's backward
sums with float atomics), so the test holds them to that control pair's own standard (see the test).
Behaviour (init_texture='random', a mask over rows 96..175 x columns 96..159 of both cameras' 256 x 256 images, forty steps, lr_base
2e-2): 47 126 hidden chart texels; their mean squared neighbour difference stays 0.16617 with the term off (no gradient reaches them)
and falls to 0.09520 with weight_tex_smooth = 3e3 on the chart.  Only the ordering is asserted.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import fitstep_ref as R
import tex_prior_ref as T
from helpers import additive, fitter_grads, fitter_near_truth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tile():
    """(TY, TX) of the kernel's workgroup tile, from its source."""
    src = open(os.path.join(ROOT, "fpc_diffrend_amd", "csrc", "tex_prior.hip")).read()
    m = re.search(r"TEX_TX = (\d+), TEX_TY = (\d+)", src)
    return int(m.group(2)), int(m.group(1))


TY, TX = _tile()
# the degenerate shapes, one tile, the tile's edges from both sides, and several tiles of a width that is no multiple of the vector width
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (64, 64), (TY - 1, TX + 1), (TY + 1, TX - 1), (65, 257)]


def _report(case, name, e, e32, bound):
    print(f"TEXPRIOR {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={bound:.1f}")


def long_sum(case, name, x, ref, x32, zeros):
    r, Sc = ref
    e, nz = R.measure(x, r, Sc)
    e32, _ = R.measure(x32, r, Sc)
    _report(case, name, e, e32, 8 * e32 + 4)
    assert nz == zeros, (case, name, nz, zeros)
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _texture(Ht, Wt, C, seed):
    """A texture in 0..1: smooth waves, a step edge through the middle and noise of a twentieth of their size."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing='ij')
    ph = 6.28 * torch.rand(C, generator=g)
    t = 0.5 + 0.2 * torch.sin(0.3 * x[..., None] + ph) * torch.cos(0.2 * y[..., None] + 2.0 * ph)
    t = t + 0.2 * (x[..., None] > Wt / 2).float() + 0.02 * torch.randn(Ht, Wt, C, generator=g)
    return t.clamp(0.0, 1.0).float().contiguous()


def _map(Ht, Wt, seed):
    """Weights in (0.1, 2) with zeros in a whole row, a whole column and single texels (a 1 x 1 map keeps its texel)."""
    w = 0.1 + 1.9 * torch.rand(Ht, Wt, generator=torch.Generator().manual_seed(seed))
    if Ht > 2:
        w[Ht // 2, :] = 0.0
    if Wt > 2:
        w[:, Wt // 3] = 0.0
    w.reshape(-1)[3::7] = 0.0
    return w.float().contiguous()


def _call(t, a, sw, aw, inv_c, ws, wa, acc, grad=True):
    from fpc_diffrend_amd import _lib
    Ht, Wt, C = t.shape
    g = torch.full_like(t, float('nan')) if grad else None
    part = torch.full((2,), float('nan'), dtype=torch.float32, device='cuda')
    val = torch.full((), float('nan'), dtype=torch.float32, device='cuda')
    _lib.call("fpcdr_tex_prior", _ptr(t), _ptr(a), _ptr(sw), _ptr(aw), float(inv_c), float(ws), float(wa), _ptr(g), _ptr(acc), _ptr(part),
              _ptr(val), Ht, Wt, C, _stream())
    assert bool((acc == 0).all())                          # the call leaves its accumulators zeroed
    return part, val, g


def _case(Ht, Wt, C, use_c, use_sw, anchor_mode, seed):
    """anchor_mode: 0 none, 1 an anchor, 2 an anchor with weights."""
    from fpc_diffrend_amd import fit
    case = f"{Ht}x{Wt}x{C}" + ('/c' if use_c else '') + ('/sw' if use_sw else '') + ('', '/a', '/a/aw')[anchor_mode]
    t = _texture(Ht, Wt, C, seed)
    a = (_texture(Ht, Wt, C, seed + 1) * 0.9 + 0.03).contiguous() if anchor_mode else None
    sw = _map(Ht, Wt, seed + 2) if use_sw else None
    aw = _map(Ht, Wt, seed + 3) if anchor_mode == 2 else None
    ws, wa, upstream = 7.5, 2.25, 0.3
    inv_c, c = 0.0, None
    if use_c:      # near the median |t_p - t_q| of the live pairs: both regimes occur
        mh, mv = T.pair_weights(Ht, Wt, sw)
        tt = t.double()
        nrm = torch.cat([(tt[:, :-1] - tt[:, 1:]).norm(dim=2)[mh > 0], (tt[:-1] - tt[1:]).norm(dim=2)[mv > 0]])
        c = float(nrm.median()) if nrm.numel() and float(nrm.median()) > 0 else 0.05
        inv_c = fit.tex_prior_inv_scale(c)
    ref = T.tex_prior(t, ws, wa, a, sw, aw, inv_c)
    ref32 = T.tex_prior(t, ws, wa, a, sw, aw, inv_c, dtype=torch.float32)
    zg, zp, zv = ref['zeros']
    cu = lambda x: None if x is None else x.cuda()
    tc, ac, swc, awc = cu(t), cu(a), cu(sw), cu(aw)
    acc = torch.zeros(2, dtype=torch.float64, device='cuda')

    # (i) fpcdr_tex_prior into buffers prefilled with NaN: every entry is written; twice on one acc: bit-identical
    part, val, g = _call(tc, ac, swc, awc, inv_c, ws, wa, acc)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(part).all()) and bool(torch.isfinite(val))
    long_sum(case, 'part', part, ref['part'], ref32['part'][0], zp)
    long_sum(case, 'value', val.reshape(1), ref['value'], ref32['value'][0], zv)
    long_sum(case, 'grad', g, ref['grad'], ref32['grad'][0], zg)
    if not zv:
        rl2 = [R.rel_l2(part, ref['part'][0]), R.rel_l2(val, ref['value'][0]), R.rel_l2(g, ref['grad'][0])]
        print(f"TEXPRIOR {case} rel-L2 part={rl2[0]:.2e} value={rl2[1]:.2e} grad={rl2[2]:.2e}")
        assert max(rl2) <= 1e-4, (case, rl2)
    else:          # no pair and no anchor: exactly 0, all of it
        assert float(val) == 0.0 and float(part.abs().max()) == 0.0 and float(g.abs().max()) == 0.0
    part2, val2, g2 = _call(tc, ac, swc, awc, inv_c, ws, wa, acc)
    assert torch.equal(part2, part) and torch.equal(val2, val) and torch.equal(g2, g), case
    part3, val3, _ = _call(tc, ac, swc, awc, inv_c, ws, wa, acc, grad=False)      # grad_tex = NULL
    assert torch.equal(part3, part) and torch.equal(val3, val), case

    # (ii) fit.texture_prior: lazy, eager with a unit upstream, eager with a factor, on the caller's acc
    for kw, upv in ((dict(), upstream), (dict(eager_grad=True, unit_upstream=True), 1.0), (dict(eager_grad=True), upstream),
                    (dict(acc=acc), upstream)):
        leaf = t.cuda().requires_grad_(True)
        value = fit.texture_prior(leaf, ws, wa, anchor=ac, smooth_weights=swc, anchor_weights=awc, scale=c, **kw)
        (value * upv).backward() if upv != 1.0 else value.backward()
        assert torch.equal(value.detach(), val), (case, kw)                  # the same call
        if upv == 1.0:
            assert torch.equal(leaf.grad, g), (case, kw)
        else:
            up32 = float(np.float32(upv))
            long_sum(case, 'grad ' + (','.join(kw) or 'lazy'), leaf.grad, (upv * ref['grad'][0], upv * ref['grad'][1]),
                     up32 * ref32['grad'][0], zg)
            assert torch.equal(leaf.grad, g * torch.tensor(upv, dtype=torch.float32, device='cuda')), (case, kw)
        assert bool((acc == 0).all())
    with torch.no_grad():                                                    # no gradient asked for: value only
        assert torch.equal(fit.texture_prior(tc, ws, wa, anchor=ac, smooth_weights=swc, anchor_weights=awc, scale=c), val)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tex_prior_entries_against_float64(shape, C):
    Ht, Wt = shape
    for use_c in (False, True):
        for use_sw in (False, True):
            for anchor_mode in (0, 1, 2):
                _case(Ht, Wt, C, use_c, use_sw, anchor_mode, seed=1000 + 7 * Ht + Wt + C)


@pytest.mark.parametrize("C", [1, 3])
def test_more_tiles_than_workgroups(C):
    """The launch is capped at TEX_MAX_WGS workgroups, which walk the tiles in strides: a texture of 33 tile columns and the fewest tile
    rows that make more tiles than the cap, ragged both ways (1024 workgroups: 497 x 2050 texels)."""
    src = open(os.path.join(ROOT, "fpc_diffrend_amd", "csrc", "tex_prior.hip")).read()
    cap = int(re.search(r"TEX_MAX_WGS = (\d+)", src).group(1))
    Ht, Wt = TY * (cap // 33) + 1, TX * 32 + 2
    assert -(-Ht // TY) * -(-Wt // TX) > cap and -(-Wt // TX) == 33
    _case(Ht, Wt, C, True, True, 2, seed=77 + C)


def test_two_channels_and_unaligned_views_take_the_same_rule():
    """C = 2 has kernels of its own; a tensor whose storage starts 4 bytes off a 16-byte line takes the loads without vectors."""
    _case(17, 36, 2, True, True, 2, seed=5)
    from fpc_diffrend_amd import ops
    t = _texture(9, 16, 1, 6).cuda()
    sw, a = _map(9, 16, 7).cuda(), _texture(9, 16, 1, 8).cuda()
    good = ops.tex_prior_call(t, 2.0, 1.0, a, sw, None, 3.0)
    off = torch.empty(t.numel() + 1, dtype=torch.float32, device='cuda')[1:].reshape(t.shape)
    off.copy_(t)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    out = ops.tex_prior_call(off, 2.0, 1.0, a, sw, None, 3.0)
    assert torch.equal(out[0], good[0]) and torch.equal(out[1], good[1]) and torch.equal(out[2], good[2])


@pytest.mark.parametrize("C", [1, 3])
def test_a_nan_in_texels_whose_every_weight_is_zero_changes_nothing(C):
    """Zero weights are selects, not products: the planted texels sit in a zero row, a zero column and alone, next to tile borders."""
    Ht, Wt = TY + 3, TX + 5
    t, a = _texture(Ht, Wt, C, 21).cuda(), _texture(Ht, Wt, C, 22).cuda()
    sw = 0.5 + torch.rand(Ht, Wt, generator=torch.Generator().manual_seed(23))
    spots = [(0, 0), (TY - 1, TX - 1), (TY, TX), (Ht - 1, Wt - 1), (3, TX - 1), (TY, 7)]
    sw[5, :] = 0.0
    sw[:, TX] = 0.0
    for s in spots:
        sw[s] = 0.0
    sw = sw.cuda()
    aw = sw.clone()
    acc = torch.zeros(2, dtype=torch.float64, device='cuda')
    bad = t.clone()
    bad[5, :] = float('nan')
    bad[:, TX] = float('nan')
    for s in spots:
        bad[s] = float('nan')
    for inv_c in (0.0, 8.0):
        good = _call(t, a, sw, aw, inv_c, 2.0, 1.5, acc)
        out = _call(bad, a, sw, aw, inv_c, 2.0, 1.5, acc)
        assert all(bool(torch.isfinite(o).all()) for o in out)
        assert all(torch.equal(x, y) for x, y in zip(good, out))
        assert float(out[2][5].abs().max()) == 0.0 and float(out[2][:, TX].abs().max()) == 0.0


def test_a_second_term_on_the_shared_accumulator_gives_its_own_value():
    from fpc_diffrend_amd import fit
    t = _texture(33, 70, 3, 31).cuda()
    x = torch.randn(4, 50, 3, generator=torch.Generator().manual_seed(32)).cuda()
    acc = torch.zeros(5, dtype=torch.float64, device='cuda')
    alone_m, alone_t = fit.motion_penalty(x, 3.0), fit.texture_prior(t, 2.0, 0.0)
    for _ in range(2):
        vt = fit.texture_prior(t, 2.0, 0.0, acc=acc)
        assert bool((acc == 0).all())
        vm = fit.motion_penalty(x, 3.0, acc=acc)
        assert bool((acc == 0).all())
        assert torch.equal(vt, alone_t) and torch.equal(vm, alone_m)


def test_texture_prior_checks_its_maps_on_the_host_unless_told_not_to():
    from fpc_diffrend_amd import fit
    t = _texture(4, 5, 1, 3).cuda()
    w = torch.ones(4, 5, device='cuda')
    w[1, 1] = -1.0
    with pytest.raises(ValueError, match="finite and not negative"):
        fit.texture_prior(t, 1.0, 0.0, smooth_weights=w)
    with pytest.raises(ValueError, match="on the device of tex"):
        fit.texture_prior(t, 1.0, 0.0, smooth_weights=torch.ones(4, 5))
    with pytest.raises(ValueError, match="on the device of tex"):
        fit.texture_prior(t, 1.0, 1.0, anchor=t.cpu())
    fit.texture_prior(t, 1.0, 0.0, smooth_weights=w, validate=False)         # no read-back: a negative weight counts as 0


# ---------------------------------------------------------------------------------------------------------------------
# the chart
# ---------------------------------------------------------------------------------------------------------------------

def test_chart_map_equals_the_oracles_rasteriser_on_the_uv_triangles(oracle_ops):
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg1', n_frames=2)
    uv, uv_idx = torch.tensor(sc.uv, dtype=torch.float32), torch.tensor(sc.uv_idx, dtype=torch.int32)
    for Ht, Wt in ((256, 256), (96, 160)):
        pos = torch.stack([2.0 * uv[:, 0] - 1.0, 2.0 * uv[:, 1] - 1.0, torch.zeros(uv.shape[0]), torch.ones(uv.shape[0])], dim=1)
        ids = oracle_ops.rasterize_ids(pos[None], uv_idx, (Ht, Wt))[0].numpy()
        want = T.dilate3(ids > 0)
        got = fit.chart_map(uv.cuda(), uv_idx.cuda(), Ht, Wt)
        assert got.dtype == torch.float32 and tuple(got.shape) == (Ht, Wt) and got.is_cuda
        assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float32)))
        assert 0 < int(want.sum()) and int((ids > 0).sum()) < int(want.sum())
        print(f"TEXPRIOR chart {Ht}x{Wt}: {int((ids > 0).sum())} covered texels, {int(want.sum())} after the dilation")


# ---------------------------------------------------------------------------------------------------------------------
# inside a Fitter
# ---------------------------------------------------------------------------------------------------------------------

# weights at which the term's texture gradient is of the size of the pixel term's at init_near_truth(0.8) on cfg1 at 128 x 128 (printed
# below; asserted: at least a hundredth of it, a hundred times the bar of the comparison)
W_S, W_A, SCALE = 3.0e4, 1.0e5, 0.1
W_GRAPH_S, W_GRAPH_A = 1.0e3, 1.0e3      # the captured steps: the term is of the size of the pixel term's value and the fit still converges


def _fitter(n_frames=3, rank=0, world=1, **kw):
    return fitter_near_truth(n_frames, rank, world, **{'resolution': (128, 128), **kw})


def _anchor_of(ft):
    """An anchor that differs from the start texture, and weights with zeros, the same for every Fitter."""
    Ht, Wt, C = ft.tex_opt.shape
    return (ft.tex_opt.detach() * 0.9 + 0.03).contiguous(), _map(Ht, Wt, 77)


def _additive(tag, ft_on, ft_off, frames, world=1):
    """tex_opt.grad = g_off + g_term within 1e-4 (|g_on| + |g_off|), every other parameter's gradient the control's, the loss likewise."""
    from fpc_diffrend_amd import fit
    cfg = ft_on.cfg
    tex = len(ft_on.params) - 1
    assert ft_on.params[tex] is ft_on.tex_opt
    l_term, n_term = additive("TEXPRIOR", tag, ft_on, ft_off, frames, lambda v: fit.texture_prior(
        ft_on.tex_opt, cfg.weight_tex_smooth / world, cfg.weight_tex_anchor / world, anchor=ft_on._tex_anchor,
        smooth_weights=ft_on._tex_smooth_w, anchor_weights=ft_on._tex_anchor_w, scale=cfg.tex_smooth_scale), sized=False)
    n_off = float(fitter_grads(ft_off)[tex].norm())      # (the term reaches the texture alone: n_term is its texture gradient's)
    assert n_term >= 1e-2 * n_off > 0.0, (tag, n_term, n_off)
    return l_term


@pytest.mark.parametrize("which", ['smooth', 'anchor', 'both'])
def test_fitter_texture_gradient_is_the_pixel_terms_plus_the_prior(which):
    kw = dict(smooth=dict(weight_tex_smooth=W_S, tex_smooth_scale=SCALE, tex_smooth_weights='chart'),
              anchor=dict(weight_tex_anchor=W_A),
              both=dict(weight_tex_smooth=W_S, weight_tex_anchor=W_A, tex_smooth_weights='chart'))[which]
    ft_on, ft_off = _fitter(**kw), _fitter()
    assert ft_on._tex_prior_on and not ft_off._tex_prior_on and ft_off._tex_anchor is None and ft_off._tex_chart is None
    if which != 'smooth':
        assert torch.equal(ft_on._tex_anchor, ft_on.tex_opt.detach())        # the texture as it stands after init_texture
        a, w = _anchor_of(ft_on)
        ft_on.set_texture_anchor(a, w)
        assert torch.equal(ft_on._tex_anchor, a) and torch.equal(ft_on._tex_anchor_w.cpu(), w)
    else:
        assert ft_on._tex_anchor is None and torch.equal(ft_on._tex_smooth_w, ft_on.texture_chart())
    _additive(which, ft_on, ft_off, slice(0, 3))


def test_second_of_two_ranks_takes_the_term_times_a_half():
    ft_on, ft_off = _fitter(4, 1, 2, weight_tex_smooth=W_S, weight_tex_anchor=W_A), _fitter(4, 1, 2)
    assert (ft_on.frame_lo, ft_on.frame_hi) == (2, 4)
    ft_on.set_texture_anchor(*_anchor_of(ft_on))
    l_half = _additive("rank1of2", ft_on, ft_off, slice(2, 4), world=2)
    ref = T.tex_prior(ft_on.tex_opt.detach(), W_S / 2, W_A / 2, ft_on._tex_anchor, None, ft_on._tex_anchor_w)['value'][0]
    assert l_half > 0.0 and abs(l_half - float(ref)) <= 1e-4 * float(ref)


def test_hip_graph_steps_equal_eager_steps_with_the_texture_prior():
    """The configuration and tolerances of test_gpu_motion.test_hip_graph_steps_equal_eager_steps_with_the_motion_term, with the texture
    prior on (both parts, a scale, the chart): no host sync, no per-call fill, static maps and anchor, so it replays."""
    from fpc_diffrend_amd import fit, scene
    traj = {}
    for graph in (False, True):
        sc = scene.cfg('cfg1', n_frames=3)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=12, cam_idxs=(0, 3), resolution=(128, 128), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, hip_graph=graph,
                            weight_laplacian=20.0, weight_tex_smooth=W_GRAPH_S, tex_smooth_scale=SCALE, tex_smooth_weights='chart',
                            weight_tex_anchor=W_GRAPH_A)
        ft = fit.Fitter(sc, cfg, device='cuda')
        ft.init_near_truth(0.8)
        ft.set_texture_anchor(*_anchor_of(ft))
        traj[graph] = [float(ft.step()) for _ in range(12)]
        if graph:
            assert ft._graphs is not None
        assert bool((ft._reg_acc == 0).all())
    a, b = np.asarray(traj[False]), np.asarray(traj[True])
    print(f"TEXPRIOR graph eager {a[:3]} .. {a[-1]:.6e} graphed {b[:3]} .. {b[-1]:.6e}")
    assert np.isfinite(b).all()
    assert np.allclose(a, b, rtol=2e-3), (a, b)
    assert np.allclose(a[:5], b[:5], rtol=1e-5), (a, b)


def test_checkpoint_carries_the_anchor_and_one_without_it_leaves_the_anchor_as_constructed():
    kw = dict(weight_tex_smooth=W_GRAPH_S, weight_tex_anchor=W_GRAPH_A)
    ft = _fitter(**kw)
    a, w = _anchor_of(ft)
    ft.set_texture_anchor(a, w)
    for _ in range(2):
        ft.step()
    sd = ft.state_dict()
    assert torch.equal(sd["tex_anchor"], a) and torch.equal(sd["tex_anchor_weights"].cpu(), w)
    ft2 = _fitter(**kw)
    built = ft2._tex_anchor.clone()
    assert not torch.equal(built, a) and ft2._tex_anchor_w is None
    ft2.load_state_dict(sd)
    assert torch.equal(ft2._tex_anchor, a) and torch.equal(ft2._tex_anchor_w.cpu(), w) and torch.equal(ft2.tex_opt, ft.tex_opt)
    l1, l2 = float(ft.loss_and_backward(slice(0, 3))), float(ft2.loss_and_backward(slice(0, 3)))
    assert abs(l1 - l2) <= 1e-5 * abs(l1), (l1, l2)
    old = {k: v for k, v in sd.items() if k not in ("tex_anchor", "tex_anchor_weights")}      # a checkpoint from before the term
    ft3 = _fitter(**kw)
    ft3.load_state_dict(old)
    assert torch.equal(ft3._tex_anchor, built) and ft3._tex_anchor_w is None
    # a Fitter without the term carries None and loads either kind
    ft0 = _fitter()
    assert ft0.state_dict()["tex_anchor"] is None and ft0.state_dict()["tex_anchor_weights"] is None
    ft0.load_state_dict(sd)
    assert ft0._tex_anchor is None
    with pytest.raises(ValueError, match="weight_tex_anchor"):
        ft0.set_texture_anchor()


def test_a_baked_start_holds_only_the_texels_a_capture_reached():
    """init_texture='bake' with tex_anchor_weights=None: the anchor is the baked texture, its weights the bake's `filled` map."""
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg1', n_frames=2)
    kw = dict(max_iter=100, cam_idxs=(0, 3), resolution=(128, 128), weight_laplacian=0.0, init_texture='bake', weight_tex_anchor=W_A)
    ft = fit.Fitter(sc, fit.FitConfig(**kw), device='cuda')
    _, filled = ft.bake_texture(assign=False)                               # (the same parameters: the bake sums integers)
    assert torch.equal(ft._tex_anchor, ft.tex_opt.detach()) and torch.equal(ft._tex_anchor_w, filled.to(torch.float32))
    assert 0 < int(filled.sum()) < filled.numel()
    # explicit weights win over the bake's map
    ft = fit.Fitter(sc, fit.FitConfig(tex_anchor_weights='chart', **kw), device='cuda')
    assert torch.equal(ft._tex_anchor_w, ft.texture_chart())


def test_reg_log_gains_texs_and_texa_only_with_the_term_on(tmp_path):
    recs = {}
    for on in (False, True):
        path = str(tmp_path / f"log{int(on)}.jsonl")
        kw = dict(weight_tex_smooth=W_GRAPH_S, weight_tex_anchor=W_GRAPH_A) if on else dict()
        ft = _fitter(log_interval=1, reg_log_interval=1, log_path=path, **kw)
        if on:
            ft.set_texture_anchor(*_anchor_of(ft))
        ft.step()
        if on:      # (the record is written behind the update: the parts of the texture as it stands after the step)
            want = T.tex_prior(ft.tex_opt.detach(), 1.0, 1.0, ft._tex_anchor, None, ft._tex_anchor_w)['part'][0]
        recs[on] = json.loads(open(path).readline())
    assert "TEXS" not in recs[False] and "TEXA" not in recs[False] and "LAP" in recs[False]
    assert set(recs[True]) == set(recs[False]) | {"TEXS", "TEXA"}
    assert abs(recs[True]["TEXS"] - W_GRAPH_S * float(want[0])) <= 1e-4 * W_GRAPH_S * float(want[0])
    assert abs(recs[True]["TEXA"] - W_GRAPH_A * float(want[1])) <= 1e-4 * W_GRAPH_A * float(want[1])


def test_with_both_weights_at_zero_a_step_is_the_step_it_was():
    """weight_tex_smooth = weight_tex_anchor = 0 with every other option set: nothing built (no anchor, no chart, no maps), no launch,
    and the results of a Fitter built without the options.  What a step computes before its backward is torch.equal; the parameters
    after three steps are held to the control pair's own standard, as in tests/test_gpu_motion.py (the pixel term's backward sums with
    float atomics): bit-equal if two Fitters without the options are, else no further from the first control than 1e-5 of the
    parameter's size."""
    from fpc_diffrend_amd import _lib
    runs = []
    zero = dict(weight_tex_smooth=0.0, weight_tex_anchor=0.0, tex_smooth_scale=0.05, tex_smooth_weights='chart', tex_anchor_weights='chart')
    for kw in (dict(), dict(), zero):
        ft = _fitter(weight_laplacian=20.0, **kw)
        assert len(ft._reg_terms) == 1 and not ft._tex_prior_on
        assert ft._tex_anchor is None and ft._tex_chart is None and ft._tex_smooth_w is None and ft._tex_anchor_w is None
        v = ft.vertices(slice(0, 3)).detach().reshape(3, -1, 3).clone().requires_grad_(True)
        term = ft._reg_terms[0](v, None)
        term.backward()
        before = [v.detach(), term.detach().clone(), v.grad.clone(), ft.tex_opt.detach().clone()]
        _lib.TIMER = _lib.KernelTimer()
        try:
            losses = [torch.as_tensor(ft.step()).detach().clone() for _ in range(3)]
            calls = {k: n for k, (n, _) in _lib.TIMER.summary().items()}
        finally:
            _lib.TIMER = None
        assert "fpcdr_tex_prior" not in calls
        runs.append((calls, before + losses[:1], losses[1:] + [p.detach().clone() for p in ft.params] + [ft.result.clone()]))
    (c0, d0, r0), (c1, d1, r1), (c2, d2, r2) = runs
    assert c0 == c1 == c2, (c0, c1, c2)                                      # the same launches
    assert all(torch.equal(a, b) for a, b in zip(d0, d2)) and all(torch.equal(a, b) for a, b in zip(d0, d1))
    control_equal = all(torch.equal(a, b) for a, b in zip(r0, r1))
    print(f"TEXPRIOR off: two Fitters without the options are torch.equal after three steps: {control_equal}; "
          f"with the options at 0: {all(torch.equal(a, b) for a, b in zip(r0, r2))}")
    for k, (a, b) in enumerate(zip(r0, r2)):
        if control_equal:
            assert torch.equal(a, b), k
        else:
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), (k, float((a - b).abs().max()))


def test_smoothness_lowers_the_neighbour_differences_of_texels_a_mask_hides():
    """init_texture='random', a mask that hides a patch of the face in both cameras, forty steps: the hidden chart texels -- the pixel
    term's gradient there is exactly 0 -- keep their noise with the term off and lose some of it with weight_tex_smooth on.  Only the
    ordering of the mean squared neighbour difference over those texels is asserted."""
    import dataclasses
    from fpc_diffrend_amd import fit, scene
    steps, msd, hidden = 40, {}, None
    for ws in (0.0, 3.0e3):
        sc = scene.cfg('cfg1', n_frames=2)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        masks = np.full((2, len(sc.cams), 256, 256), 255, dtype=np.uint8)
        masks[:, :, 96:176, 96:160] = 0
        sc = dataclasses.replace(sc, masks=masks)
        cfg = fit.FitConfig(max_iter=steps, cam_idxs=(0, 3), resolution=(128, 128), init_texture='random', weight_laplacian=0.0,
                            lr_base=2e-2, weight_tex_smooth=ws, tex_smooth_weights='chart' if ws else None)
        ft = fit.Fitter(sc, cfg, device='cuda')
        ft.init_near_truth(1.0)
        if hidden is None:      # from the Fitter without the term: the chart texels the pixel term does not reach
            ft.loss_and_backward(slice(0, 2))
            hidden = ((ft.tex_opt.grad.abs().sum(dim=2) == 0) & (ft.texture_chart() > 0)).cpu()
            ft.optimizer.zero_grad(set_to_none=True)
            assert int(hidden.sum()) > 100, int(hidden.sum())
        start = T.neighbour_msd(ft.tex_opt, hidden)
        for _ in range(steps):
            ft.step()
        msd[ws] = T.neighbour_msd(ft.tex_opt, hidden)
        print(f"TEXPRIOR behaviour weight_tex_smooth={ws:g}: {int(hidden.sum())} hidden chart texels, mean squared neighbour difference "
              f"start {start:.5f} after {steps} steps {msd[ws]:.5f}")
    assert msd[3.0e3] < msd[0.0], msd

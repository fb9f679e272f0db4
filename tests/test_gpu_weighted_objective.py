"""GPU: the WEIGHTED one-pass objective (csrc/objective.hip: k_shade_list_w / k_fix_list_w and their sweeps, fpcdr_objective_weighted_fwd;
csrc/robust.hip: k_robust_bg, fpcdr_ref_bg_wsum; DESIGN.md 3, "Weighted objective rule") against autograd through the operators with
the Robust loss rule as a plain torch expression, and the FitConfig option that puts a Fitter's robust iterations on it.

Bars: value 1e-5 relative and gradients relative L2 < 1e-4, the project's bars (tests/test_gpu_robust.py); the sums of weights and the
background sums are long sums, held by that file's bar e <= 8 * e32 + 4 in units of u = 2^-24, e32 the error of a float32 sum on the CPU.
Inputs: tests/objective_ref.case_inputs -- two images of 45 x 70 (partial bins on both axes), silhouettes that cross bin borders (the
soups) and that lie against empty pixels (the islands).  The mask is random bytes with a block of 0 and a block of 255, stored one byte
off alignment; a fifth of the face weights is exactly 0.  Every line below is printed by a test as "WOBJ ..." (pytest -s).
These bars are relative over whole tensors: they see a wrong formula, not a wrong pixel.  The entry-by-entry bars against a float64 statement
of the weighted call -- exact zeros, every entry in units of its own scale, the value by an operation count, wsum, one-term texels bit for
bit, C = 4 -- live in tests/test_gpu_objective_weighted_ref.py (tests/objective_ref.py with inp['weights']); this file keeps the comparison
with the operator path, the Fitter, the background sums and the argument checks.

Measured on an MI355X at 17543e4 plus the change that adds this file (the largest over the cases of a row; 120 weighted calls against
autograd: six cases x five kinds and scales x four option sets).  The whole file runs in 6.6 s there, 2.2 s of them the first Fitter test:

  what                                        measured                                   bound
  value against autograd, relative            1.28e-07 .. 1.86e-07 (soup/C3/clamp)       1e-5
  grad_pos against autograd, relative L2      2.71e-07 .. 1.33e-06 (soup/C1/wrap)        1e-4
  grad_tex against autograd, relative L2      2.34e-07 .. 1.33e-06 (soup/C3/clamp)       1e-4
  wsum against fpcdr_robust_loss's sums[1]    e 0.64 u at most (islands/C1/wrap, w_out 0.25, sat 100; its own bound 4.5), 0.14 of its bound at most
  neutral weights against the plain call      value 0; grad_pos 0 .. 3.0e-08; grad_tex 3.1e-08 .. 1.2e-07       1e-4
          two plain calls against each other  value 0; grad_pos 0 .. 4.5e-09; grad_tex 4.9e-08 .. 1.2e-07       (for scale)
  hints frozen at (1, 1, 1): the sweeps       12 occupied bins, 12 with a deferred pixel in both cases; against autograd value 0 .. 8.3e-08,
    (Charbonnier c = 20, w_out 0.25, sat 100) grad_pos 1.5e-07 .. 2.1e-07, grad_tex 1.7e-07 .. 5.1e-07 (bounds as above); against the unfrozen
                                              call value 0, grad_pos 4.0e-09 .. 5.3e-08, grad_tex 6.1e-08 .. 8.3e-08 (1e-4); wsum e 0.30 u at most
                                              (its bound 6.7).  The same at the parent of the change that adds the row (2.1e-07 / 5.4e-07 at most)
  all weights 0 (three ways, three kinds)     value, grad_pos, grad_tex exactly 0
  texels no weighted pixel reaches            93 of 720 (12 of them under pixels of weight 0), 96 of 720 (15): exactly those are 0.0 in grad_tex
  background sums, 9 pixel counts x 2 bases   sum w0 rho e 0.60 u at most (0.08 of its bound), sum w0 2.90 u (n = 16, mask, w_out 0.25; 0.44 of its bound)
  record_slots = 1                            value nan, skip_out 1.0, plain and weighted alike
  Fitter, Charbonnier c = 10, all weights     loss 15.441944 on both paths, wsum 2724.908 on both; parameter gradients relative L2
                                              1.4e-08 (tex_opt) .. 1.2e-07 (t_opt), bound 1e-4
  Fitter, frame 1 and view 1 alone            loss 20.645264 against 20.645266 on the operator path, wsum 690.351 on both
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import fitstep_ref as R
import objective_ref as OR
import robust_ref as RR
from test_gpu_robust import FIT_KW, PARAMS, _at, _masked_scene

pytestmark = pytest.mark.gpu

# (name in the output, case of objective_ref, channels kept of its texture, boundary mode): C = 1 and 3; wrap, clamp and zero
CASES = [('soup/C1/wrap', 'soup/C1/wrap/seam', 1, 'wrap'), ('soup/C3/clamp', 'soup/C3/clamp', 3, 'clamp'), ('soup/C3/zero', 'soup/C4/zero', 3, 'zero'),
         ('soup/C1/zero', 'soup/C4/zero', 1, 'zero'), ('islands/C1/wrap', 'islands/wrap', 1, 'wrap'), ('islands/C3/clamp', 'islands/clamp', 3, 'clamp')]
KINDS = [('l2', None), ('charbonnier', 2.0), ('charbonnier', 20.0), ('geman_mcclure', 2.0), ('geman_mcclure', 20.0)]
OPTIONS = [(0.25, 0), (0.25, 100), (0.0, 0), (0.0, 100)]      # (weight_outside, saturation): the captures of the cases lie in 1 .. 140
_cache = {}


def long_sum(case, name, x, r, S, x32):
    e, _ = R.measure(x, r, S)
    e32, _ = R.measure(x32, r, S)
    print(f"WOBJ {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={8 * e32 + 4:.1f}")
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _inputs(tag, oracle_ops):
    """The case's tensors on the GPU with a mask and face weights of its own.  Cached: read-only."""
    if tag in _cache:
        return _cache[tag]
    _, name, C, boundary = next(c for c in CASES if c[0] == tag)
    inp = OR.case_inputs(name, oracle_ops)
    B, (H, W), T = inp['pos'].shape[0], inp['res'], inp['tri'].shape[0]
    g = torch.Generator().manual_seed(77)
    mask = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    mask[:, 5:14, 8:30] = 0
    mask[:, 20:40, 25:60] = 255
    face_w = torch.rand(T, generator=g) * 1.5
    face_w[torch.rand(T, generator=g) < 0.2] = 0.0
    face_w[0] = 0.0
    dev = 'cuda'
    out = dict(pos=inp['pos'].to(dev), tri=inp['tri'].to(dev), uv=inp['uv'].to(dev), uv_tri=inp['uv_tri'].to(dev),
               tex=inp['tex'][..., :C].contiguous().to(dev), ref=inp['ref_u8'].to(dev), mask=_at(mask, 1), face_w=face_w.to(dev), res=(H, W),
               boundary=boundary, C=C, tag=tag)
    assert out['mask'].data_ptr() % 16 == 1
    _cache[tag] = out
    return out


def _objective(dr, g, want_grad=True, **kw):
    ctx = dr.RasterizeGLContext(device='cuda')
    pos, tex = g['pos'].clone().requires_grad_(want_grad), g['tex'].clone().requires_grad_(want_grad)
    val = dr.pixel_objective(ctx, pos, g['tri'], g['uv'], g['uv_tri'], tex, g['ref'], g['res'], boundary_mode=g['boundary'], **kw)
    if want_grad:
        val.backward()
    return val.detach(), pos.grad, tex.grad


def _chain(dr, g):
    """The operators once per case: (pos, tex, rast, antialiased colour) with the graph kept."""
    key = ('chain', g['tag'])
    if key not in _cache:
        ctx = dr.RasterizeGLContext(device='cuda')
        pos, tex = g['pos'].clone().requires_grad_(True), g['tex'].clone().requires_grad_(True)
        rast, _ = dr.rasterize(ctx, pos, g['tri'], g['res'])
        texc, _ = dr.interpolate(g['uv'][None], rast, g['uv_tri'])
        col = dr.antialias(dr.texture(tex[None], texc, filter_mode='linear', boundary_mode=g['boundary']), rast, pos, g['tri'])
        _cache[key] = (pos, tex, rast, col)
    return _cache[key]


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_weighted_objective_against_autograd_through_the_operators(tag, oracle_ops):
    import fpc_diffrend_amd.ops as dr
    g = _inputs(tag, oracle_ops)
    pos, tex, rast, col = _chain(dr, g)
    assert int((rast[..., 3] > 0).sum()) > 200 and int((rast[..., 3] == 0).sum()) > 200
    worst = dict(value=0.0, g_pos=0.0, g_tex=0.0)
    dr.clear_hints()
    for j, (w_out, sat) in enumerate(OPTIONS):
        w32, _ = RR.weights(rast[..., 3], g['ref'], g['mask'], g['face_w'], w_out, sat, dtype=torch.float32)
        w64, _ = RR.weights(rast[..., 3], g['ref'], g['mask'], g['face_w'], w_out, sat)
        assert int((w64 == 0).sum()) > 50 and int((w64 > 0).sum()) > 200
        for kind, c in KINDS:
            loss = RR.loss_plain(col, rast[..., 3], g['ref'], kind, c, weight=w32.cuda())
            gp, gt = torch.autograd.grad(loss, (pos, tex), retain_graph=True)
            wsum = torch.zeros(1, dtype=torch.float64, device='cuda')
            val, g_pos, g_tex = _objective(dr, g, robust=(kind, c), mask=g['mask'], face_weights=g['face_w'], weight_outside=w_out,
                                           saturation=sat, wsum_out=wsum)
            ev = abs(float(val) - float(loss)) / abs(float(loss))
            ep, et = float(R.rel_l2(g_pos, gp)), float(R.rel_l2(g_tex, gt))
            print(f"WOBJ {tag} {kind} c={c} w_out={w_out} sat={sat} value {float(val):.6f} torch {float(loss):.6f} rel={ev:.2e} "
                  f"g_pos rel_l2={ep:.2e} g_tex rel_l2={et:.2e}")
            assert float(gp.abs().max()) > 0 and float(gt.abs().max()) > 0
            assert ev <= 1e-5 and ep < 1e-4 and et < 1e-4, (tag, kind, c, w_out, sat, ev, ep, et)
            worst = dict(value=max(worst['value'], ev), g_pos=max(worst['g_pos'], ep), g_tex=max(worst['g_tex'], et))
            if kind in ('l2', 'geman_mcclure') and c in (None, 20.0):
                # the sum of the weights against fpcdr_robust_loss's on the same rast, by the long-sum bar
                sums, _ = dr.robust_loss_call(col.detach(), rast, g['ref'], kind, c, 1.0, mask=g['mask'], face_weights=g['face_w'],
                                              weight_outside=w_out, saturation=sat, want_grad=False)
                x32 = (w32.sum(dtype=torch.float32) * g['C']).double()
                long_sum(f"{tag} {kind} w_out={w_out} sat={sat}", 'wsum', wsum[0], sums[1], sums[1], x32)
    dr.clear_hints()
    print(f"WOBJ worst {tag} value rel={worst['value']:.2e}/1e-5 g_pos={worst['g_pos']:.2e}/1e-4 g_tex={worst['g_tex']:.2e}/1e-4")


@pytest.mark.parametrize("tag", ['soup/C1/wrap', 'soup/C3/clamp'])
def test_neutral_weights_through_the_weighted_kernels_are_the_plain_objective(tag, oracle_ops, monkeypatch):
    import fpc_diffrend_amd.ops as dr
    g = _inputs(tag, oracle_ops)
    dr.clear_hints()
    plain, plain2 = _objective(dr, g), _objective(dr, g)
    for label in ('tri_uv', 'uv_indirect'):      # C = 1: k_shade_list_w<1, WRAP> and, through the index buffer, <1, -1>
        if label == 'uv_indirect':
            monkeypatch.setattr(dr, "_cached_tri_uv", lambda uv_, idx_: None)
        wsum = torch.zeros(1, dtype=torch.float64, device='cuda')
        got = _objective(dr, g, robust=('l2', None), wsum_out=wsum)
        for name, x, r, r2 in zip(('value', 'g_pos', 'g_tex'), got, plain, plain2):
            e, spread = float(R.rel_l2(x.reshape(-1), r.reshape(-1))), float(R.rel_l2(r2.reshape(-1), r.reshape(-1)))
            print(f"WOBJ neutral {tag} {label} {name} rel_l2={e:.2e} two plain runs {spread:.2e} bound=1e-4")
            assert e < 1e-4, (tag, label, name, e)
        assert float(wsum) == float(g['ref'].numel() * g['C'])      # every weight is 1: w - w0 is exactly 0 everywhere
    dr.clear_hints()


@pytest.mark.parametrize("tag", ['soup/C1/wrap', 'soup/C3/clamp'])
def test_weighted_sweeps_with_hints_frozen_at_one_entry(tag, oracle_ops):
    """Launch hints frozen at (1, 1, 1): k_shade_queue_w and k_fix_queue_w<CS, 0 / 1> take every entry of their lists but the first (12
    occupied bins, all 12 with a deferred pixel, in both cases: objective_ref.plan).  The twin of test_gpu_objective_ref.py's."""
    import fpc_diffrend_amd.ops as dr
    g = _inputs(tag, oracle_ops)
    pos, tex, rast, col = _chain(dr, g)
    kind, c, w_out, sat = 'charbonnier', 20.0, 0.25, 100
    kw = dict(robust=(kind, c), mask=g['mask'], face_weights=g['face_w'], weight_outside=w_out, saturation=sat)
    dr.clear_hints()
    free = _objective(dr, g, wsum_out=torch.zeros(1, dtype=torch.float64, device='cuda'), **kw)
    h = dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]
    h.poll()
    h.caps, h.frozen = (1, 1, 1), True
    wsum = torch.zeros(1, dtype=torch.float64, device='cuda')
    got = _objective(dr, g, wsum_out=wsum, **kw)
    torch.cuda.synchronize()
    n_def, n_occ = int(h.host[0]), int(h.host[3])
    # against autograd through the operators: the first test's bars
    w32, _ = RR.weights(rast[..., 3], g['ref'], g['mask'], g['face_w'], w_out, sat, dtype=torch.float32)
    loss = RR.loss_plain(col, rast[..., 3], g['ref'], kind, c, weight=w32.cuda())
    gp, gt = torch.autograd.grad(loss, (pos, tex), retain_graph=True)
    ev = abs(float(got[0]) - float(loss)) / abs(float(loss))
    ep, et = float(R.rel_l2(got[1], gp)), float(R.rel_l2(got[2], gt))
    # ... and against the unfrozen call (atomics reorder: the neutral-weights test's bar)
    ef = [float(R.rel_l2(x.reshape(-1), r.reshape(-1))) for x, r in zip(got, free)]
    print(f"WOBJ sweeps {tag} occupied bins {n_occ} with a deferred pixel {n_def}: value {float(got[0]):.6f} torch {float(loss):.6f} rel={ev:.2e} "
          f"g_pos rel_l2={ep:.2e} g_tex rel_l2={et:.2e}; against the unfrozen call value {ef[0]:.2e} g_pos {ef[1]:.2e} g_tex {ef[2]:.2e}")
    assert float(gp.abs().max()) > 0 and float(gt.abs().max()) > 0
    assert ev <= 1e-5 and ep < 1e-4 and et < 1e-4, (tag, ev, ep, et)
    assert all(e < 1e-4 for e in ef), (tag, ef)
    sums, _ = dr.robust_loss_call(col.detach(), rast, g['ref'], kind, c, 1.0, mask=g['mask'], face_weights=g['face_w'], weight_outside=w_out,
                                  saturation=sat, want_grad=False)
    long_sum(f"sweeps {tag}", 'wsum', wsum[0], sums[1], sums[1], (w32.sum(dtype=torch.float32) * g['C']).double())
    assert n_occ > 1 and n_def > 1, (tag, n_occ, n_def)      # the sweeps had work
    dr.clear_hints()


def test_zero_weights_give_exact_zeros(oracle_ops):
    import fpc_diffrend_amd.ops as dr
    g = _inputs('soup/C3/clamp', oracle_ops)
    dr.clear_hints()
    zero_w = torch.zeros_like(g['face_w'])
    for label, kw in (('faces 0, outside 0', dict(face_weights=zero_w, weight_outside=0.0)),
                      ('faces 0, outside 0, saturation 1', dict(face_weights=zero_w, weight_outside=0.0, saturation=1)),
                      ('saturation 1 alone', dict(face_weights=g['face_w'], weight_outside=0.25, saturation=1, mask=g['mask']))):
        for kind, c in (('l2', None), ('charbonnier', 2.0), ('geman_mcclure', 20.0)):
            val, g_pos, g_tex = _objective(dr, g, robust=(kind, c), **kw)
            print(f"WOBJ zeros {label} {kind}: value {float(val)} max|g_pos| {float(g_pos.abs().max())} max|g_tex| {float(g_tex.abs().max())}")
            assert float(val) == 0.0 and bool((g_pos == 0).all()) and bool((g_tex == 0).all()), (label, kind)
    # a texel whose every contributing pixel has weight 0 is exactly 0.0: the texels that pixels of positive weight reach, from the
    # operators (every term of d sum(colour) / d tex is a product of bilinear and blend weights: none is negative)
    pos, tex, rast, col = _chain(dr, g)
    for w_out, sat in ((0.25, 0), (0.0, 100)):
        w64, cov = RR.weights(rast[..., 3], g['ref'], g['mask'], g['face_w'], w_out, sat)
        reach, = torch.autograd.grad((col * ((w64 > 0) & cov).cuda()[..., None]).sum(), tex, retain_graph=True)
        everything, = torch.autograd.grad(col.sum(), tex, retain_graph=True)
        unreached = reach == 0
        n_new = int((unreached & (everything != 0)).sum())
        val, g_pos, g_tex = _objective(dr, g, robust=('charbonnier', 20.0), mask=g['mask'], face_weights=g['face_w'], weight_outside=w_out, saturation=sat)
        print(f"WOBJ zeros texels w_out={w_out} sat={sat}: {int(unreached.sum())} of {g_tex.numel()} without a weighted pixel "
              f"({n_new} of them under pixels of weight 0), exact zeros in grad_tex {int((g_tex == 0).sum())}")
        assert n_new > 0
        assert bool((g_tex[unreached] == 0).all()) and int((g_tex == 0).sum()) == int(unreached.sum())
    dr.clear_hints()


@pytest.mark.parametrize("n", [15, 16, 17, 255, 256, 257, 1023, 1024, 1025])
def test_background_sums_per_image_against_float64(n):
    import fpc_diffrend_amd.ops as dr
    gen = torch.Generator().manual_seed(100 + n)
    ref = torch.randint(0, 256, (2, 1, n), generator=gen, dtype=torch.uint8)
    mask = torch.randint(0, 256, (2, 1, n), generator=gen, dtype=torch.uint8)
    mask[:, :, : n // 3] = 255
    mask[:, :, n // 3: n // 2] = 0
    zeros = torch.zeros(2, 1, n)
    for off in (0, 3):      # the buffers' bases aligned and not (the second image starts n bytes on either way)
        ref_g, mask_g = _at(ref, off), _at(mask, off)
        for kind, c in KINDS:
            for use_mask, w_out, sat in ((False, 1.0, 0), (True, 0.25, 0), (True, 0.25, RR.SAT), (False, 0.0, RR.SAT)):
                out = dr.reference_background_weighted(ref_g, mask_g if use_mask else None, kind, c, w_out, sat, RR.BACKGROUND)
                assert tuple(out.shape) == (2, 2) and out.dtype == torch.float64
                for b in range(2):
                    kw = dict(mask=mask[b:b + 1] if use_mask else None, w_outside=w_out, sat=sat)
                    r64 = RR.robust_loss(zeros[b:b + 1, ..., None], zeros[b:b + 1], ref[b:b + 1], kind, c, **kw)['sums']
                    r32 = RR.robust_loss(zeros[b:b + 1, ..., None], zeros[b:b + 1], ref[b:b + 1], kind, c, dtype=torch.float32, **kw)['sums']
                    case = f"bg n={n} off={off} image {b} {kind} c={c} mask={use_mask} w_out={w_out} sat={sat}"
                    for k, name in ((0, 'sum w0 rho'), (1, 'sum w0')):
                        if float(r64[1][k]) == 0.0:
                            assert float(out[b, k]) == 0.0, case
                        else:
                            long_sum(case, name, out[b, k], r64[0][k], r64[1][k], r32[0][k])
    # L2 without weights: the plain background sum
    plain = dr.reference_background_sumsq(_at(ref, 0), RR.BACKGROUND)
    w = dr.reference_background_weighted(_at(ref, 0), None, 'l2', None, 1.0, 0, RR.BACKGROUND)
    assert float(R.rel_l2(w[:, 0], plain)) < 1e-6 and bool((w[:, 1] == float(n)).all())


def test_a_call_short_of_record_slots_says_so_as_the_plain_call_does(oracle_ops):
    """An input that needs more record slots than it is given is an ordinary input: NaN and skip_out = 1, no fault."""
    import fpc_diffrend_amd.ops as dr
    g = _inputs('soup/C1/wrap', oracle_ops)
    for kw in (dict(), dict(robust=('charbonnier', 20.0), mask=g['mask'], face_weights=g['face_w'], weight_outside=0.25)):
        dr.clear_hints()
        skip = torch.full((1,), -1.0, device='cuda')
        val, _, _ = _objective(dr, g, record_slots=1, skip_out=skip, **kw)
        print(f"WOBJ slots weighted={bool(kw)} record_slots=1: value {float(val)} skip_out {float(skip)}")
        assert bool(torch.isnan(val)) and float(skip) == 1.0
        dr.clear_hints()
        skip.fill_(-1.0)
        val, _, _ = _objective(dr, g, record_slots=4096, skip_out=skip, **kw)
        assert bool(torch.isfinite(val)) and float(skip) == 0.0
    dr.clear_hints()


def test_bad_arguments_are_rejected(oracle_ops):
    import fpc_diffrend_amd.ops as dr
    g = _inputs('soup/C1/wrap', oracle_ops)
    for bad in (dict(robust=('l2', None), one_pass=False), dict(mask=g['mask'], sparse=False), dict(saturation=100, enable_mip=True),
                dict(robust=('charbonnier', None)), dict(robust='charbonnier'), dict(weight_outside=-1.0), dict(saturation=256),
                dict(mask=g['mask'][:, :5]), dict(face_weights=g['face_w'][:-1]), dict(face_weights=-g['face_w'] - 1.0),
                dict(robust=('l2', None), ref_bg_sumsq=torch.zeros((), dtype=torch.float64)), dict(wsum_out=torch.zeros(1, device='cuda'))):
        with pytest.raises(ValueError):
            _objective(dr, g, want_grad=False, **bad)
    # the C entry refuses the mip branch and bad weights without a launch
    from fpc_diffrend_amd import _lib
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for over in (dict(kind=3), dict(kind=1, inv_c=0.0), dict(w_outside=-1.0), dict(sat=256), dict(face_w=ctypes.c_void_p(g['face_w'].data_ptr()), T_weights=0),
                 dict(wsum=None)):
        wsum = torch.zeros(_lib.WSUM_SLOTS, dtype=torch.float64, device='cuda')
        kw = dict(kind=0, inv_c=0.0, w_outside=1.0, sat=0, T_weights=0, wsum=ctypes.c_void_p(wsum.data_ptr()))
        kw.update(over)
        with pytest.raises(RuntimeError, match="fpcdr_objective_weighted_fwd"):
            _lib.call("fpcdr_objective_weighted_fwd", ctypes.byref(_lib.ObjectiveWeighted(**kw)), stream)
    p = _lib.ObjectiveWeighted(kind=0, w_outside=1.0, wsum=ctypes.c_void_p(wsum.data_ptr()))
    p.base.mip = 1
    with pytest.raises(RuntimeError, match="mip"):
        _lib.call("fpcdr_objective_weighted_fwd", ctypes.byref(p), stream)
    dr.clear_hints()


# ---- the Fitter -------------------------------------------------------------------------------------------------------------------------
def _fitter(fit, sc, **kw):
    ft = fit.Fitter(sc, fit.FitConfig(**dict(FIT_KW, **kw)), device='cuda')
    ft.init_near_truth(0.7)
    return ft


def test_fitter_weighted_one_pass_step_against_the_operator_path(monkeypatch):
    from fpc_diffrend_amd import fit
    sc, masks, face_w = _masked_scene()
    sc = dataclasses.replace(sc, masks=masks)
    kw = dict(robust='charbonnier', robust_scale=10.0, face_weights=face_w, weight_outside=0.25, saturation=130)
    calls = []
    real = fit.pixel_loss_robust
    monkeypatch.setattr(fit, "pixel_loss_robust", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    fr = slice(0, 2)
    ft, ft2 = _fitter(fit, sc, weighted_one_pass=True, **kw), _fitter(fit, sc, **kw)
    loss = ft.loss_and_backward(fr)
    assert calls == []                                          # the weighted one-pass call, not the operators
    wsum = float(ft._wsum)
    loss2 = ft2.loss_and_backward(fr)
    assert calls == ['charbonnier']
    print(f"WOBJ fitter loss {float(loss):.6f} operator path {float(loss2):.6f} wsum {wsum:.3f} operator path {float(ft2._wsum):.3f}")
    assert abs(float(loss) - float(loss2)) <= 1e-5 * abs(float(loss2))
    assert abs(wsum - float(ft2._wsum)) <= 1e-5 * float(ft2._wsum)
    seen = 0
    for name, p, p2 in zip(PARAMS, ft.params, ft2.params):
        assert (p.grad is None) == (p2.grad is None), name
        if p.grad is not None:
            err = float(R.rel_l2(p.grad, p2.grad))
            print(f"WOBJ fitter grad {name} rel_l2={err:.2e} bound=1e-4")
            assert float(p2.grad.abs().max()) > 0 and err < 1e-4, (name, err)
            seen += 1
    assert seen >= 6
    # a second step reuses the cached background sums; a subset of frames and views gathers them, and the masks, by row
    assert len(ft._bg_wsum) == 1
    ft.loss_and_backward(fr)
    assert len(ft._bg_wsum) == 1 and calls == ['charbonnier']
    frames, views = torch.tensor([1], device='cuda'), torch.tensor([1], device='cuda')
    sub, sub2 = ft.loss_and_backward(frames, views), ft2.loss_and_backward(frames, views)
    print(f"WOBJ fitter frame 1, view 1: loss {float(sub):.6f} operator path {float(sub2):.6f} wsum {float(ft._wsum):.3f} / {float(ft2._wsum):.3f}")
    assert calls == ['charbonnier'] * 2 and abs(float(sub) - float(sub2)) <= 1e-5 * abs(float(sub2))
    assert abs(float(ft._wsum) - float(ft2._wsum)) <= 1e-5 * float(ft2._wsum)


def test_fitter_pyramid_level_under_mip_stays_on_the_operator_path_and_robust_iters_ends_on_the_plain_step(monkeypatch, tmp_path):
    import json
    from fpc_diffrend_amd import fit
    sc, masks, face_w = _masked_scene()
    calls = []
    real = fit.pixel_loss_robust
    monkeypatch.setattr(fit, "pixel_loss_robust", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    fr = slice(0, 2)
    kw = dict(robust='charbonnier', robust_scale=10.0, weight_outside=0.25, saturation=130, weighted_one_pass=True)
    ft = _fitter(fit, dataclasses.replace(sc, masks=masks), pyramid=((2, 4),), **kw)
    ft.loss_and_backward(fr)                                    # iteration 0: factor 2 under pyramid_mip, the cheap level
    assert ft.resolution == (32, 32) and ft.enable_mip and calls == ['charbonnier']
    ft.iteration = 4
    ft.loss_and_backward(fr)                                    # full size, no mip: the weighted one-pass call
    assert ft.resolution == (64, 64) and not ft.enable_mip and calls == ['charbonnier'] and ft._wsum is not None
    # robust_iters = 1 without other weights: iteration 1 is the plain one-pass step of a default Fitter
    log = tmp_path / "steps.jsonl"
    ft = _fitter(fit, sc, robust='geman_mcclure', robust_scale=10.0, robust_iters=1, weighted_one_pass=True, log_interval=1, reg_log_interval=0,
                 log_path=str(log))
    ft0 = _fitter(fit, sc)
    ft.step()
    assert calls == ['charbonnier'] and ft._wsum is not None
    state = {k: v.clone() for k, v in zip(PARAMS, ft.params)}
    for p0, k in zip(ft0.params, PARAMS):
        p0.data.copy_(state[k])
    ft0.iteration = 1
    loss0 = ft0.loss_and_backward(fr)
    loss1 = ft.loss_and_backward(fr)
    assert ft._wsum is None and calls == ['charbonnier']
    assert abs(float(loss1) - float(loss0)) <= 1e-6 * abs(float(loss0)), (float(loss1), float(loss0))
    for name, p, p0 in zip(PARAMS, ft.params, ft0.params):
        if p.grad is not None:
            assert R.rel_l2(p.grad, p0.grad) < 1e-4, name
    ft.step()
    recs = [json.loads(l) for l in log.read_text().splitlines()]
    assert [r["it"] for r in recs] == [0, 1]
    assert recs[0]["wsum"] == float(2 * 2 * 64 * 64) and "wsum" not in recs[1]      # every weight is 1: the number of entries
    # hip_graph with weights keeps raising, flag or no flag
    with pytest.raises(ValueError):
        fit.Fitter(sc, fit.FitConfig(weighted_one_pass=True, hip_graph=True, saturation=140, **FIT_KW), device='cuda')

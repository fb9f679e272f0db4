"""GPU: the backward of the fused render pair (csrc/fused.hip: k_render_bwd behind fpcdr_render_bwd, after k_bins_shade behind
fpcdr_render_fwd) entry by entry against float64 (tests/render_ref.py), through fpc_diffrend_amd.ops.render_textured and
backward(dy), every case twice.  The pair is on a default fit path: Fitter.loss_and_backward renders through it on every step that is
not a one-shot objective (a blurred or locally normalised term, a robust / masked / weighted term without weighted_one_pass).
  preconditions  rast's ids equal the oracle's; rast and colour are bit-identical to ops.rasterize -> ops.interpolate ->
                 ops.texture('linear') on the same inputs; u, v and z/w are bit-identical to rasterize_ref.float32_in_kernel_order;
  zeros          every entry render_ref.predicted_zeros names is exactly 0, and the entries with a scale are the predicted ones;
  entry by entry e = max_i |x_i - r_i| / S_i in units of u = 2^-24 for g_tex, g_pos and the w column of g_pos on a row of its own:
                 e <= 8 * e32 + 4, e32 the same measure of the float32 evaluation of the statement by torch on the CPU.  S is the scale
                 CARRIED through the three stages (render_ref's docstring); g_pos and its w column are held a second time, under the
                 same bar, to the last stage's OWN scale (rows g_pos/own, g_pos.w/own), which is smaller, hence stricter;
  bit for bit    a texel entry with exactly one term, of a covered pixel, equals the float32 product dy_c * w_k, w_k in the kernel's
                 expression order -- on every case, `magnified/C1/wrap` has thousands.  (k_render_bwd forms tu = (u q0 + v q1) + w q2 with
                 w = (1 - u) - v: the expression interpolate_ref.float32_in_kernel_order evaluates.)
Cases: objective_ref's thirteen settled non-mip cases and three cut from them -- C = 2 (the forward takes any C: nothing to refuse), a
1 x 1 and a 1 x 24 texture under 'wrap' --, each with a dense and a sparse upstream gradient, `islands/clamp` and `islands/zero` also with
one that is zero on every covered pixel.  Twins on `soup/C3/clamp` and `islands/zero`: only pos / only tex requiring a gradient, and the
C entry called directly with tri_uv given, on zeroed buffers and on buffers that hold values (the kernel adds: they join the statement
as one more term).  The fit path: a default FitConfig with blur_sigma > 0 calls ops.render_textured once per loss_and_backward and
leaves finite gradients.  Each test prints "RENDER case output calls e_gpu e32 bound" (pytest -s).  tests/test_render_ref.py shows on
the CPU that the statement equals float64 autograd through the oracle, that every case reaches its path and that wrong restatements
miss these bars.

Measured on an MI355X (units of u; the larger of a variant's two calls; the order of the atomics moves the last digits from run to run;
the whole file, 37 tests with the building of the cases and their references on the CPU, ran in 7.1 s).  Every precondition held, every
predicted zero was exact, and every one-term texel entry (last column; the 9315 and 868 of `magnified/C1/wrap` among them) was
bit-identical to dy_c * w_k in both calls.  The 58 rows of the twins (only pos, only tex, tri_uv given, tri_uv given on preloaded
buffers) stayed within 0.12 of their bounds, the largest 4.96 u against 43.65 (`soup/C3/clamp` sparse, preloaded, g_pos/own).  The
fit step called ops.render_textured once and left finite gradients.  No bug was found.

  case-upstream              g_tex           g_pos           g_pos.w         g_pos/own       g_pos.w/own     bounds (8 e32 + 4)                one-term
                             e_gpu / e32     e_gpu / e32     e_gpu / e32     e_gpu / e32     e_gpu / e32
  magnified/C1/wrap-dense    6.110 / 6.110   0.002 / 0.002   0.001 / 0.001   2.824 / 2.824   1.229 / 1.229   52.88  4.01  4.01  26.59  13.83   9315
  magnified/C1/wrap-sparse   2.216 / 2.216   0.004 / 0.004   0.004 / 0.004   12.125 / 12.125 5.054 / 5.010   21.73  4.03  4.03  101.00  44.08  868
  soup/C1/wrap/seam-dense    0.567 / 0.567   0.002 / 0.002   0.001 / 0.001   4.354 / 4.354   1.823 / 1.823   8.53  4.02  4.01  38.83  18.58    1
  soup/C1/wrap/seam-sparse   1.892 / 1.892   0.003 / 0.003   0.003 / 0.003   4.469 / 4.469   2.141 / 2.177   19.14  4.03  4.02  39.76  21.42   42
  soup/C3/clamp-dense        1.469 / 1.469   0.020 / 0.020   0.007 / 0.007   0.797 / 0.813   0.568 / 0.545   15.75  4.16  4.05  10.50  8.36    12
  soup/C3/clamp-sparse       2.054 / 2.054   0.022 / 0.022   0.015 / 0.015   4.956 / 4.956   3.466 / 3.466   20.43  4.18  4.12  43.65  31.73   146
  soup/C4/zero-dense         0.948 / 0.948   0.017 / 0.017   0.016 / 0.016   1.879 / 1.879   1.665 / 1.665   11.58  4.13  4.13  19.03  17.32   0
  soup/C4/zero-sparse        1.721 / 1.721   0.010 / 0.010   0.006 / 0.006   2.349 / 2.349   1.967 / 1.967   17.77  4.08  4.04  22.79  19.74   99
  mesh/B3-dense              0.204 / 0.151   0.000 / 0.000   0.000 / 0.000   0.035 / 0.035   0.032 / 0.032   5.21  4.00  4.00  4.28  4.25      0
  mesh/B3-sparse             0.218 / 0.168   0.000 / 0.000   0.000 / 0.000   0.114 / 0.114   0.113 / 0.113   5.35  4.00  4.00  4.91  4.90      0
  confetti-dense             0.308 / 0.297   0.025 / 0.025   0.017 / 0.017   1.411 / 1.411   1.129 / 1.155   6.38  4.20  4.14  15.29  13.24    0
  confetti-sparse            0.947 / 0.947   0.026 / 0.026   0.021 / 0.021   4.574 / 4.574   3.257 / 3.257   11.58  4.21  4.17  40.59  30.06   4
  islands/wrap-dense         0.524 / 0.524   0.000 / 0.000   0.000 / 0.000   0.398 / 0.385   0.296 / 0.310   8.19  4.00  4.00  7.08  6.48      1
  islands/wrap-sparse        0.621 / 0.621   0.001 / 0.001   0.001 / 0.001   1.014 / 1.014   0.702 / 0.702   8.97  4.01  4.01  12.12  9.61     2
  islands/clamp-dense        0.786 / 0.784   0.000 / 0.000   0.000 / 0.000   0.110 / 0.110   0.092 / 0.092   10.27  4.00  4.00  4.88  4.74     12
  islands/clamp-sparse       0.810 / 0.810   0.000 / 0.000   0.000 / 0.000   0.263 / 0.246   0.161 / 0.157   10.48  4.00  4.00  5.97  5.25     15
  islands/zero-dense         1.212 / 1.212   0.000 / 0.000   0.000 / 0.000   0.200 / 0.211   0.201 / 0.196   13.69  4.00  4.00  5.69  5.57     0
  islands/zero-sparse        1.119 / 1.119   0.001 / 0.001   0.000 / 0.000   0.761 / 0.761   0.225 / 0.261   12.95  4.01  4.00  10.09  6.08    10
  borders-dense              1.531 / 1.531   0.001 / 0.001   0.000 / 0.000   1.227 / 1.227   0.363 / 0.363   16.24  4.01  4.00  13.82  6.90    21
  borders-sparse             1.858 / 1.858   0.005 / 0.005   0.004 / 0.004   3.688 / 3.688   1.204 / 1.204   18.87  4.04  4.03  33.50  13.63   295
  tiny/1x1-dense             0.369 / 0.369   0.000 / 0.000   0.000 / 0.000   0.217 / 0.217   0.000 / 0.000   6.95  4.00  4.00  5.74  4.00      12
  tiny/1x1-sparse            0.390 / 0.390   0.001 / 0.001   0.000 / 0.000   0.571 / 0.571   0.000 / 0.000   7.12  4.01  4.00  8.57  4.00      12
  tiny/1x2-dense             0.605 / 0.605   0.001 / 0.001   0.000 / 0.000   0.883 / 0.883   0.280 / 0.280   8.84  4.01  4.00  11.06  6.24     4
  tiny/1x2-sparse            0.588 / 0.588   0.001 / 0.001   0.000 / 0.000   0.824 / 0.824   0.376 / 0.376   8.70  4.01  4.00  10.59  7.01     4
  tiny/2x1-dense             0.582 / 0.582   0.000 / 0.000   0.000 / 0.000   0.350 / 0.350   0.350 / 0.350   8.66  4.00  4.00  6.80  6.80      4
  tiny/2x1-sparse            0.612 / 0.612   0.000 / 0.000   0.000 / 0.000   0.323 / 0.323   0.323 / 0.323   8.89  4.00  4.00  6.59  6.59      4
  C2/clamp-dense             1.466 / 1.466   0.050 / 0.050   0.004 / 0.004   0.476 / 0.476   0.329 / 0.329   15.73  4.40  4.03  7.81  6.63     8
  C2/clamp-sparse            2.019 / 2.019   0.016 / 0.016   0.008 / 0.008   2.286 / 2.286   1.206 / 1.206   20.16  4.13  4.06  22.28  13.65   47
  tex1x1/wrap-dense          0.020 / 0.057   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   4.46  4.00  4.00  4.00  4.00      0
  tex1x1/wrap-sparse         0.046 / 0.018   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   4.14  4.00  4.00  4.00  4.00      0
  tex1xW/wrap-dense          0.088 / 0.091   0.005 / 0.005   0.001 / 0.002   0.414 / 0.414   0.182 / 0.182   4.73  4.04  4.02  7.31  5.46      0
  tex1xW/wrap-sparse         0.290 / 0.283   0.004 / 0.004   0.003 / 0.003   0.349 / 0.349   0.233 / 0.233   6.27  4.03  4.02  6.79  5.87      0
  islands/clamp-off-geometry 0.388 / 0.293   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   6.35  4.00  4.00  4.00  4.00      0
  islands/zero-off-geometry  0.233 / 0.140   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   0.000 / 0.000   5.12  4.00  4.00  4.00  4.00      0
g_pos and g_pos.w are measured against the CARRIED scale, which is hundreds to thousands of times the error of a float32 evaluation: those
rows see a wrong term or factor (tests/test_render_ref.py: the mutants miss them by 1700 to 8000 u), not a lost bit.  g_pos/own and
g_pos.w/own are the same entries against the last stage's own scale, where the float32 evaluation stands at 0.03 to 12 u."""
import ctypes

import pytest
import torch

import render_ref as R

pytestmark = pytest.mark.gpu


def _call(dr, inp, dy, want=('pos', 'tex')):
    dev = 'cuda'
    ctx = dr.RasterizeGLContext(device=dev)
    pos, tex = inp['pos'].to(dev).requires_grad_('pos' in want), inp['tex'].to(dev).requires_grad_('tex' in want)
    colour, rast = dr.render_textured(ctx, pos, inp['tri'].to(dev), inp['uv'].to(dev), inp['uv_tri'].to(dev), tex, inp['res'],
                                      boundary_mode=inp['boundary'])
    colour.backward(dy.to(dev))
    torch.cuda.synchronize()
    got = {'colour': colour.detach().cpu(), 'rast': rast.cpu()}
    if 'pos' in want:
        got['g_pos'] = pos.grad.cpu()
    else:
        assert pos.grad is None
    if 'tex' in want:
        got['g_tex'] = tex.grad.cpu()
    else:
        assert tex.grad is None
    return got


def _direct(dr, inp, dy, pre=None):
    """fpcdr_render_bwd itself, with tri_uv given (the autograd path hands None) -> g_pos, g_tex; pre: what the buffers hold on entry."""
    from fpc_diffrend_amd import _lib
    dev = 'cuda'
    t = {k: inp[k].to(dev).contiguous() for k in ('pos', 'tri', 'uv', 'uv_tri', 'tex', 'rast')}
    tri_uv = t['uv'][t['uv_tri'].long()].contiguous()
    g_pos = torch.zeros_like(t['pos']) if pre is None else pre['g_pos'].to(dev).contiguous()
    g_tex = torch.zeros_like(t['tex']) if pre is None else pre['g_tex'].to(dev).contiguous()
    d = dy.to(dev).contiguous()
    (B, V, _), (H, W), (Ht, Wt, C) = t['pos'].shape, inp['res'], t['tex'].shape
    p = _lib.RenderBwd(pos=dr._ptr(t['pos']), tri=dr._ptr(t['tri']), uv=dr._ptr(t['uv']), uv_tri=dr._ptr(t['uv_tri']), tex=dr._ptr(t['tex']),
                       rast=dr._ptr(t['rast']), dy=dr._ptr(d), B=B, V=V, T=t['tri'].shape[0], H=H, W=W, Vt=t['uv'].shape[0], Ht=Ht, Wt=Wt, C=C,
                       boundary_mode=_lib.BOUNDARY[inp['boundary']], grad_pos=dr._ptr(g_pos), grad_tex=dr._ptr(g_tex), tri_uv=dr._ptr(tri_uv))
    _lib.call("fpcdr_render_bwd", ctypes.byref(p), dr._stream())
    torch.cuda.synchronize()
    return {'g_pos': g_pos.cpu(), 'g_tex': g_tex.cpu()}


def _preconditions(dr, inp, got):
    dev = 'cuda'
    assert torch.equal(got['rast'][..., 3], inp['ids'].float()), (inp['name'], 'ids')
    assert torch.equal(got['rast'][..., :3], inp['rast'][..., :3]), (inp['name'], 'u, v, z/w are not float32_in_kernel_order')
    ctx = dr.RasterizeGLContext(device=dev)
    rast, _ = dr.rasterize(ctx, inp['pos'].to(dev), inp['tri'].to(dev), inp['res'])
    texc, _ = dr.interpolate(inp['uv'].to(dev)[None], rast, inp['uv_tri'].to(dev))
    col = dr.texture(inp['tex'].to(dev)[None], texc, filter_mode='linear', boundary_mode=inp['boundary'])
    assert torch.equal(got['rast'], rast.cpu()), (inp['name'], 'rast is not the operator\'s')
    assert torch.equal(got['colour'], col.cpu()), (inp['name'], 'colour is not the operators\'')


def _hold(name, kind, inp, dy, got, tag='', calls=1, pre=None):
    ref, r32 = R.reference(inp, dy), R.reference(inp, dy, torch.float32)
    k32 = R.kernel_order(inp, dy) if pre is None else None
    if pre is not None:
        ref, r32 = R.preloaded(ref, r32, pre)
    for k in R.OUTPUTS:
        if k in got:
            for (row, e, _), (_, e32, _) in zip(R.measure_rows(got[k], ref, k), R.measure_rows(r32[k][0], ref, k)):
                print(f"RENDER {name}-{kind}{tag} {row} {calls} {e:.3f} {e32:.3f} {R.bound(e32):.2f}")
    assert R.failures(inp, dy, ref, r32, got, k32, pre=pre) == [], (name, kind, tag)
    return 0 if k32 is None else k32['entry'].numel()


@pytest.mark.parametrize("name,kind", R.VARIANTS, ids=R.VARIANT_IDS)
def test_render_backward_entry_by_entry(name, kind, oracle_ops):
    import fpc_diffrend_amd.ops as dr
    inp = R.inputs(name, oracle_ops)
    dy = R.upstream(inp, kind)
    for call in (1, 2):
        got = _call(dr, inp, dy)
        if call == 1:
            _preconditions(dr, inp, got)
        n = _hold(name, kind, inp, dy, got, '', call)
    print(f"RENDER {name}-{kind} one-term texel entries held bit for bit: {n}")
    if name == 'magnified/C1/wrap':
        assert n >= (5000 if kind == 'dense' else 500)


@pytest.mark.parametrize("name", ['soup/C3/clamp', 'islands/zero'])
def test_twins_meet_the_same_bars(name, oracle_ops):
    import fpc_diffrend_amd.ops as dr
    inp = R.inputs(name, oracle_ops)
    for kind in ('dense', 'sparse'):
        dy = R.upstream(inp, kind)
        for want in (('pos',), ('tex',)):      # grad_tex null; grad_pos null: the kernel returns after the scatter
            _hold(name, kind, inp, dy, _call(dr, inp, dy, want=want), '/only-' + want[0])
        _hold(name, kind, inp, dy, _direct(dr, inp, dy), '/tri_uv')
        # the kernel adds: half of the entries with a term hold a value of their own size on entry
        r32 = R.reference(inp, dy, torch.float32)
        gen = torch.Generator().manual_seed(11)
        pre = {k: (torch.randn(r32[k][0].shape, generator=gen) * (torch.rand(r32[k][0].shape, generator=gen) < 0.5) * r32[k][0].abs()).float()
               for k in R.OUTPUTS}
        assert all(int((p != 0).sum()) > 10 for p in pre.values())
        _hold(name, kind, inp, dy, _direct(dr, inp, dy, pre), '/tri_uv,preloaded', pre=pre)


def test_a_default_blurred_fit_step_runs_the_fused_render_pair(monkeypatch):
    """A default FitConfig with blur_sigma > 0 (fused_render is on by default) at 64 x 64 on two views renders through
    ops.render_textured, so its parameter gradients come through k_render_bwd."""
    from fpc_diffrend_amd import fit, scene
    calls = []
    real = fit.dr.render_textured

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(fit.dr, 'render_textured', counting)
    sc = scene.make_scene(resolution=(64, 64), n_frames=2)
    cfg = fit.FitConfig(blur_sigma=3.0, blur_kernel_size=15, cam_idxs=(0, 4))
    assert cfg.fused_render is True and cfg.weighted_one_pass is False
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.7)
    loss = ft.loss_and_backward(slice(0, 2))
    torch.cuda.synchronize()
    assert len(calls) == 1 and bool(torch.isfinite(loss))
    grads = [p.grad for p in ft.params if p.grad is not None]
    assert len(grads) >= 6 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert float(ft.tex_opt.grad.abs().max()) > 0 and sum(float(g.abs().max()) > 0 for g in grads) >= 6

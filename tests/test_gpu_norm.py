"""GPU: the locally normalised pixel loss (csrc/norm.hip, fpcdr_norm_loss) stage by stage and entry by entry against float64
(tests/norm_ref.py), and the switch that lets a Fitter use it.

Conventions of tests/test_gpu_blur.py: the error of an output x with float64 reference r is e = max_i |x_i - r_i| / S_i in units of u =
2^-24; entries with S_i = 0 must be exactly 0 and their number the one predicted (uncovered pixels x C for the gradient).  Every output
is held to the long-sum bar e <= 8 * e32 + 4, e32 the error of float32 torch on the CPU for the same statement against the same
reference.  Each stage is judged on the float32 planes it read, the ones the kernels themselves wrote:
    the four statistics planes (mu_a, m_a, mu_t, m_t)     on the inputs; S_i = the blur of the absolute values
    d, P, q, p                                            on the kernel's statistics planes; S_i the first-order rounding scale
                                                          norm_ref.pointwise carries down from them (the cancellation of m - mu^2 is in it)
    the sum                                               on the kernel's d
    the gradient                                          on the kernel's (P, q) and p; S_i carried through the two adjoints and the combine
Every line below is printed by a test as "NORM case name e_gpu e32 bound" (pytest -s).

Measured on an MI355X (units of u; the largest over the cases of a row -- the twenty shapes, each with the default and with a larger
n_total --; the last column is the case of the row that came closest to its own bound):

  output   cases  max e_gpu  max e32   closest to its bound (e_gpu / bound)
  mu_a        40       7.88     7.88   2.96 / 20.4   (1,5,5,1) k9
  m_a         40       9.14     9.14   2.93 / 17.4   (1,4,10,1) k5
  mu_t        40       8.98     8.98   4.09 / 30.5   (1,24,40,1) k9, the flat case
  m_t         40       6.85     7.28   3.31 / 26.6   (1,6,255,1) k7
  d           40       0.38     0.38   0.38 / 6.9    (1,8,300,3) k15
  P           40       0.35     0.41   0.35 / 6.8    (2,37,70,1) k31
  q           40       0.42     0.43   0.42 / 7.2    (1,300,9,1) k17
  p           40       0.40     0.40   0.39 / 6.9    (1,300,9,1) k17
  sum         40       1.02     1.59   1.02 / 12.2   (1,5,9,2) k5
  grad        40       3.70     3.16   2.17 / 15.5   (1,300,9,1) k17, the larger n_total
  largest radius (12 x 9, r = 8, flat taps): grad 0.75 / 10.0
  flat case: max |d| where the whole window is flat 0 (bound 5.5e-5); m_a - mu_a^2 there 6.1e-4 (float32 rounding of 2025, against eps^2 = 4)
  Fitter: loss 0.34073326 against torch's 0.34073326; parameter gradients against autograd through the same operators, relative L2
          4.2e-07 (per_frame_q) .. 1.2e-06 (tex_opt), bound 1e-4
  exposure: loss 0.00050 at d = 0, 0.13844 / 0.13905 at -1 / +1, 0.27312 / 0.27420 at -2 / +2; gradient along the axis -0.454, +0.469,
          -0.344, +0.365 there (the oracle's float32 numbers of tests/test_norm_ref.py to every digit shown)
The planes and the gradient are bit-identical from run to run, the sum moves in its last bits with the order of the atomics.  The whole
file runs in 8 s there, 5 s of them the first Fitter test (the process's first Fitter).
"""
import ctypes

import pytest
import torch

import blur_ref as B
import fitstep_ref as R
import norm_ref as N

pytestmark = pytest.mark.gpu

ALL_SHAPES = N.ALL_SHAPES + [N.FLAT_SHAPE]
STAT_NAMES = ('mu_a', 'm_a', 'mu_t', 'm_t')

_cache = {}


def _case(shape):
    """Inputs, taps and the float64 / float32 statistics of a shape, computed once and shared (nobody writes to them)."""
    if shape not in _cache:
        Bn, H, W, C, k, sigma = shape
        colour, cover, ref = N.flat_inputs() if shape == N.FLAT_SHAPE else N.inputs(Bn, H, W, C)
        g = N.taps(k, sigma)
        _cache[shape] = dict(colour=colour, cover=cover, ref=ref, g=g, stats=N.stats(colour, cover, ref, g),
                             stats32=N.stats(colour, cover, ref, g, dtype=torch.float32)[0])
    return _cache[shape]


def _gpu(c):
    rast = torch.zeros(c['colour'].shape[:3] + (4,), device='cuda')
    rast[..., 3] = c['cover'].cuda()
    return c['colour'].cuda(), rast, c['ref'].cuda()


def long_sum(case, name, x, ref, x32, zeros=0):
    r, S = ref
    e, nz = R.measure(x, r, S)
    e32, _ = R.measure(x32, r, S)
    print(f"NORM {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={8 * e32 + 4:.1f}")
    assert nz == zeros, (case, name, nz, zeros)
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_norm_loss_stages_against_float64(shape):
    import fpc_diffrend_amd.ops as dr
    c = _case(shape)
    Bn, H, W, C, k, sigma = shape
    case = f"norm({Bn},{H},{W},{C})k{k}" + ("flat" if shape == N.FLAT_SHAPE else "")
    cg, rast, rg = _gpu(c)
    col, cov, ref, g = c['colour'], c['cover'], c['ref'], c['g']
    uncovered = int((cov <= 0).sum())
    for n_total in (None, 3 * col.numel() + 1):
        gs = 1.0 / (n_total or col.numel())
        s, grad, pl = dr.norm_loss_call(cg, rast, rg, g, gs, eps=N.EPS)
        tag = case + ('' if n_total is None else '/n_total')
        st = pl['stats'].cpu()
        assert all(bool(torch.isfinite(t).all()) for t in (st, pl['d'], pl['pq'], pl['p'], grad))
        for i, name in enumerate(STAT_NAMES):
            long_sum(tag, name, st[..., i], (c['stats'][0][..., i], c['stats'][1][..., i]), c['stats32'][..., i])
        pw = N.pointwise(col, cov, ref, st, N.EPS)
        pw32 = N.pointwise(col, cov, ref, st, N.EPS, dtype=torch.float32)
        pq, p, d = pl['pq'].cpu(), pl['p'].cpu(), pl['d'].cpu()
        for name, x in (('d', d), ('P', pq[..., 0]), ('q', pq[..., 1]), ('p', p)):
            long_sum(tag, name, x, pw[name], pw32[name][0])
        d64 = d.double()
        long_sum(tag, 'sum', s.reshape(()), ((d64 * d64).sum(), (d64 * d64).sum()), (d * d).sum())
        long_sum(tag, 'grad', grad, N.gradient(col, cov, pq, p, g, n_total), N.gradient(col, cov, pq, p, g, n_total, dtype=torch.float32)[0],
                 zeros=C * uncovered)
        unc = (cov <= 0)[..., None].expand_as(d)
        assert bool((grad.cpu()[unc] == 0).all())
    if shape == N.FLAT_SHAPE:
        # where the whole window lies in the flat half, a and t are constants: x - mu is what the two k-term sums and the float32 taps'
        # own sum lose, at most (2 k + 2) u |x| per normalised value, over s >= eps
        flat = d[:, :, : W // 2 - (k - 1) // 2]
        bound = 2 * (2 * k + 2) * R.U * 46.0 / N.EPS
        print(f"NORM {case} flat half: max |d| = {float(flat.abs().max()):.3e} bound {bound:.3e}; "
              f"v_a in [{float((st[..., 1] - st[..., 0] ** 2)[:, :, : W // 2 - (k - 1) // 2].min()):.3e}, "
              f"{float((st[..., 1] - st[..., 0] ** 2)[:, :, : W // 2 - (k - 1) // 2].max()):.3e}]")
        assert float(flat.abs().max()) <= bound
    # a second identical call, and the value-only call (grad_color NULL: three of the five passes), bit for bit
    s2, grad2, pl2 = dr.norm_loss_call(cg, rast, rg, g, gs, eps=N.EPS)
    assert torch.equal(grad2, grad) and all(torch.equal(pl2[n], pl[n]) for n in ('stats', 'd', 'pq', 'p'))
    s3, grad3, pl3 = dr.norm_loss_call(cg, rast, rg, g, gs, eps=N.EPS, want_grad=False)
    assert grad3 is None and set(pl3) == {'stats', 'd'} and torch.equal(pl3['stats'], pl['stats']) and torch.equal(pl3['d'], pl['d'])
    assert abs(float(s3) - float(s)) <= 1e-12 * float(s)


def test_images_are_independent():
    """Nothing crosses an image boundary of the flat buffers: other inputs for image 0 leave image 1's planes and gradient bit-identical."""
    import fpc_diffrend_amd.ops as dr
    shape = (2, 37, 70, 1, 31, 2.0)
    c = _case(shape)
    cg, rast, rg = _gpu(c)
    gs = 1.0 / c['colour'].numel()
    _, grad, pl = dr.norm_loss_call(cg, rast, rg, c['g'], gs)
    colour2, cover2, ref2 = N.inputs(*shape[:4], seed=11)
    cg2, rast2, rg2 = cg.clone(), rast.clone(), rg.clone()
    cg2[0], rg2[0] = colour2[0].cuda(), ref2[0].cuda()
    rast2[0, ..., 3] = cover2[0].cuda()
    _, grad2, pl2 = dr.norm_loss_call(cg2, rast2, rg2, c['g'], gs)
    assert torch.equal(grad2[1], grad[1]) and all(torch.equal(pl2[n][1], pl[n][1]) for n in ('stats', 'd', 'pq', 'p'))
    assert not torch.equal(pl2['stats'][0], pl['stats'][0]) and not torch.equal(grad2[0], grad[0])


def test_largest_legal_radius_runs_and_bad_arguments_are_rejected_without_a_launch():
    from fpc_diffrend_amd import _lib
    import fpc_diffrend_amd.ops as dr
    Bn, H, W, C = 1, 12, 9, 1
    colour, cover, ref = N.inputs(Bn, H, W, C)
    cg, rast, rg = _gpu(dict(colour=colour, cover=cover, ref=ref))
    acc = torch.zeros(1, dtype=torch.float64, device='cuda')
    f = lambda *s: torch.full(s, -7.0, device='cuda')
    tmp, stats, d, pq, p, grad = f(Bn, H, W, C, 4), f(Bn, H, W, C, 4), f(Bn, H, W, C), f(Bn, H, W, C, 2), f(Bn, H, W, C), f(Bn, H, W, C)

    def params(radius, eps=2.0, **over):
        kw = dict(color=_ptr(cg), rast=_ptr(rast), ref=_ptr(rg), B=Bn, H=H, W=W, C=C, bg=B.BACKGROUND, color_scale=255.0, grad_scale=1.0,
                  eps=eps, radius=radius, tmp=_ptr(tmp), stats=_ptr(stats), d=_ptr(d), pq=_ptr(pq), p=_ptr(p), loss_sum=_ptr(acc),
                  grad_color=_ptr(grad))
        kw.update(over)
        q = _lib.NormLoss(**kw)
        for t in range(min(2 * radius + 1, 64) if radius > 0 else 0):
            q.taps[t] = 1.0 / (2 * radius + 1)
        return q

    bad = [params(min(H, W)), params(32), params(0), params(-1), params(2, eps=0.0), params(2, eps=-1.0), params(2, eps=float('nan')),
           params(2, eps=float('inf')), params(2, stats=None), params(2, d=None), params(2, pq=None), params(2, C=5), params(2, W=0)]
    for q in bad:
        with pytest.raises(RuntimeError):
            _lib.call("fpcdr_norm_loss", ctypes.byref(q), _stream())
    torch.cuda.synchronize()
    assert float(acc) == 0.0 and all(bool((t == -7.0).all()) for t in (tmp, stats, d, pq, p, grad))        # nothing ran
    _lib.call("fpcdr_norm_loss", ctypes.byref(params(min(H, W) - 1)), _stream())                            # the largest legal radius does
    torch.cuda.synchronize()
    assert float(acc) > 0.0 and all(bool(torch.isfinite(t).all()) and not bool((t == -7.0).any()) for t in (stats, d, pq, p, grad))
    # and it is the statement's: the whole image in every window, every entry folding at both ends
    g = torch.full((2 * (min(H, W) - 1) + 1,), 1.0 / (2 * (min(H, W) - 1) + 1))
    long_sum('largest radius', 'grad', grad, N.gradient(colour, cover, pq.cpu(), p.cpu(), g, 1), N.gradient(colour, cover, pq.cpu(), p.cpu(), g, 1,
                                                                                                  dtype=torch.float32)[0],
             zeros=C * int((cover <= 0).sum()))
    for kw in (dict(sigma=2.0, kernel_size=8), dict(sigma=2.0, kernel_size=65), dict(sigma=2.0, kernel_size=2 * min(H, W) + 1),
               dict(sigma=0.0, kernel_size=5), dict(sigma=None, kernel_size=5), dict(taps=torch.ones(4) / 4),
               dict(taps=torch.ones(2 * min(H, W) + 1)), dict(sigma=2.0, kernel_size=5, eps=0.0), dict(sigma=2.0, kernel_size=5, eps=float('nan'))):
        with pytest.raises(ValueError):
            dr.normalised_pixel_loss(cg, rast, rg, **kw)
    with pytest.raises(ValueError):
        dr.normalised_pixel_loss(colour, rast, rg, sigma=2.0, kernel_size=5)            # a CPU tensor


def test_ops_normalised_pixel_loss_value_and_backward():
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd import fit
    shape = (2, 37, 70, 1, 31, 2.0)
    c = _case(shape)
    cg, rast, rg = _gpu(c)
    for n_total in (None, 5 * c['colour'].numel()):
        n = n_total or c['colour'].numel()
        s, grad, _ = dr.norm_loss_call(cg, rast, rg, c['g'], 1.0 / n, eps=1.5)
        x = cg.clone().requires_grad_(True)
        loss = dr.normalised_pixel_loss(x, rast, rg, sigma=2.0, kernel_size=31, eps=1.5, n_total=n_total)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert float(loss.detach()) == float((s[0] / n).to(torch.float32))
        (0.5 * loss).backward()
        assert torch.equal(x.grad, 0.5 * grad)
        y = cg.clone().requires_grad_(True)
        dr.normalised_pixel_loss(y, rast, rg, taps=c['g'], eps=1.5, n_total=n_total).backward()      # taps= overrides sigma and kernel_size
        assert torch.equal(y.grad, grad)
        s4, grad4 = fit.pixel_loss_normalised(cg, rast, rg, c['g'], 1.5, n_total)
        assert torch.equal(grad4, grad) and abs(float(s4) - float(s)) <= 1e-12 * float(s)
    # eps is not decoration: another eps, another value
    l15, l40 = (float(dr.normalised_pixel_loss(cg, rast, rg, taps=c['g'], eps=e)) for e in (1.5, 4.0))
    assert abs(l40 - l15) > 1e-3 * l15


def test_fitter_normalised_iterations_then_the_one_pass_objective():
    """A Fitter with norm_sigma > 0: loss and parameter gradients of a normalised iteration equal those autograd gives through the same GPU
    operators with a torch-made loss (norm_ref.loss_plain: F.pad(reflect) + conv2d, float32 on the GPU), within the project's 1e-4
    relative L2; from iteration norm_iters on the step is the one-pass objective's; a resumed checkpoint lands on the right side.  (Measured values: the module docstring.)"""
    from fpc_diffrend_amd import fit, scene
    sc = scene.make_scene(resolution=(96, 96), n_frames=2)
    kw = dict(weight_laplacian=0, max_iter=4, cam_idxs=(0, 4))
    cfg = fit.FitConfig(norm_sigma=3, norm_kernel_size=15, norm_iters=2, **kw)
    fr = slice(0, 2)
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.7)
    loss = ft.loss_and_backward(fr)
    # the same chain by hand on a Fitter WITHOUT the switch (same state, same operators), the loss a plain torch expression
    ft0 = fit.Fitter(sc, fit.FitConfig(**kw), device='cuda')
    ft0.init_near_truth(0.7)
    assert ft0.norm_taps(0) is None
    vtx = ft0.vertices(fr, validate=False).reshape(2, -1, 3)
    pos_clip = fit.transform_clip_batched(ft0.mvp(fr, None, None, validate=False), vtx)
    colour, rast = fit.render_from_clip(ft0.glctx, pos_clip, ft0.pos_idx, ft0.uv, ft0.uv_idx, ft0.tex_opt, ft0.resolution,
                                        cfg.enable_mip, cfg.max_mip_level, cfg.fused_render)
    ref = ft0.targets.reshape(-1, *ft0.resolution)
    taps = N.taps(15, 3.0)
    assert torch.equal(ft.norm_taps(0), taps)
    loss2 = N.loss_plain(colour, rast[..., 3], ref, taps, eps=cfg.norm_eps)
    loss2.backward()
    loss2 = loss2.detach()
    print(f"NORM fitter loss {float(loss):.8f} torch {float(loss2):.8f}")
    assert abs(float(loss) - float(loss2)) <= 1e-4 * abs(float(loss2))
    seen = 0
    for name, p, p2 in zip(("m1", "m2", "m3", "maps", "maps_intermediate", "t_opt", "q_opt", "per_frame_t", "per_frame_q", "tex_opt"),
                           ft.params, ft0.params):
        assert (p.grad is None) == (p2.grad is None), name
        if p.grad is not None:
            err = R.rel_l2(p.grad, p2.grad)
            print(f"NORM fitter grad {name} rel_l2={err:.2e} bound=1e-4")
            assert float(p2.grad.abs().max()) > 0 and err < 1e-4, (name, err)
            seen += 1
    assert seen >= 6
    # iteration 2 onwards: the one-pass objective, as the Fitter without the switch runs it on the same state
    assert ft.norm_taps(1) is not None and ft.norm_taps(2) is None and ft.blur_taps(0) is None
    ft.iteration = 2
    loss_after = ft.loss_and_backward(fr)
    ft0.iteration = 2
    loss0 = ft0.loss_and_backward(fr)
    assert abs(float(loss_after) - float(loss0)) <= 1e-6 * abs(float(loss0)), (float(loss_after), float(loss0))
    assert abs(float(loss_after) - float(loss)) > 1e-3 * abs(float(loss0))               # (and the normalised value was another one)
    # a checkpoint resumed across the switch continues on the right side: norm_taps is a function of the restored iteration alone
    after, ft.iteration = ft.state_dict(), 1
    before = ft.state_dict()
    assert torch.equal(ft.norm_taps(), taps)
    ft.load_state_dict(after)
    assert ft.iteration == 2 and ft.norm_taps() is None
    ft.load_state_dict(before)
    assert ft.iteration == 1 and torch.equal(ft.norm_taps(), taps)
    for bad, words in ((dict(fused_loss=False), ("norm_sigma", "fused_loss")), (dict(hip_graph=True), ("norm_sigma", "hip_graph"))):
        with pytest.raises(ValueError) as ei:
            fit.Fitter(sc, fit.FitConfig(norm_sigma=3, norm_kernel_size=15, **kw, **bad), device='cuda')
        assert all(w in str(ei.value) for w in words)
    with pytest.raises(ValueError):
        fit.Fitter(sc, fit.FitConfig(norm_sigma=3, norm_kernel_size=15, norm_eps=0.0, **kw), device='cuda')


def test_exposure_gains_do_not_move_the_minimum():
    """The scan of tests/test_norm_ref.py::test_exposure_scan_on_the_oracle through the Fitter: the 128 x 128 scene, cameras (0, 4), the
    8-bit targets of camera 0 replaced by round(0.75 x + 8) and of camera 4 by round(1.25 x - 6), everything at the truth but frame 0
    moved along per_frame_t[0, 0] by d pixels (1 unit = 3.494 px).  The normalised loss has its minimum at d = 0 and its gradient along
    the axis points home at d = +-1, +-2 (two orders of magnitude of margin on the oracle).  (Measured values: the module docstring.)"""
    from fpc_diffrend_amd import fit, scene
    PX = 3.494
    sc = scene.make_scene(resolution=(128, 128), n_frames=1)
    cfg = fit.FitConfig(norm_sigma=3, norm_kernel_size=15, norm_eps=2.0, weight_laplacian=0, max_iter=4, cam_idxs=(0, 4))
    ft = fit.Fitter(sc, cfg, device='cuda')
    x = ft.targets.to(torch.float32)
    ft.targets[:, 0] = torch.round(0.75 * x[:, 0] + 8.0).to(torch.uint8)
    ft.targets[:, 1] = torch.round(1.25 * x[:, 1] - 6.0).clamp(0, 255).to(torch.uint8)
    res = {}
    for d in (0, -1, 1, -2, 2):
        with torch.no_grad():
            ft.init_near_truth(1.0)
            ft.per_frame_q.copy_(torch.tensor(sc.q_gt, device='cuda'))
            ft.per_frame_t[0, 0] += d / PX
        loss = ft.loss_and_backward(slice(0, 1))
        res[d] = (float(loss), float(ft.per_frame_t.grad[0, 0]))
        print(f"NORM exposure d={d:+d} loss {res[d][0]:.5f} gradient {res[d][1]:+.4g}")
    assert all(res[0][0] < res[d][0] for d in (-2, -1, 1, 2))
    assert res[-1][1] < 0 and res[-2][1] < 0 and res[1][1] > 0 and res[2][1] > 0

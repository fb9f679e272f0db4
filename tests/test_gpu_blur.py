"""GPU: the blurred pixel loss (csrc/blur.hip, fpcdr_blur_loss) entry by entry against float64 (tests/blur_ref.py), and the switch
that lets a Fitter use it for the first part of a run.

Conventions of tests/test_gpu_fitstep.py: the error of an output x with float64 reference r is e = max_i |x_i - r_i| / S_i in units
of u = 2^-24, S_i the sum of the absolute values of the terms of entry i; entries with S_i = 0 must be exactly 0 and their number the
one predicted (uncovered pixels x C for the gradient).  Every output is a long sum (up to 63 taps per axis): e <= 8 * e32 + 4, e32 the
error of float32 torch on the CPU for the same sum against the same reference.  Each stage is judged on the float32 input it read: E
on the inputs, the sum and the gradient on the plane E the kernel itself wrote.
Every line below is printed by a test as "BLUR case name e_gpu e32 bound" (pytest -s).

Measured on an MI355X (units of u; the largest over the cases of a row -- the fourteen shapes, each with the default and with a
larger n_total --; the last column is the case of the row that came closest to its own bound).  E and the gradient are bit-identical
from run to run, the sum moves in its last bits with the order of the atomics.  The whole file runs in 6 s there, 3.7 s of them the Fitter
test:

  output                              cases max e_gpu  max e32   closest to its bound (e_gpu / bound)
  E                                      28      1.63     1.38   1.63 / 11.3   (1,6,256,1) k7
  sum                                    28      0.79     2.09   0.39 / 4.2    (1,6,255,1) k7
  grad                                   28      9.82     6.52   9.82 / 45.9   (1,64,33,1) k63
  identity taps: sum                      1      0.07     0.05   0.07 / 4.4
  identity taps: fpcdr_pixel_loss sum     1      0.02     0.05   0.02 / 4.4
  identity taps: grad against fpcdr_pixel_loss's  0.00 (bound 2)
  Fitter: loss 79.968033 against torch's 79.968025; parameter gradients against autograd through the same operators, relative L2
          5.5e-08 (q_opt) .. 2.1e-07 (per_frame_t), bound 1e-4
"""
import ctypes

import pytest
import torch

import blur_ref as B
import fitstep_ref as R

pytestmark = pytest.mark.gpu

# the tile extents of csrc/sep_window.h (ROW_TX x ROW_TY pixels x rows in the row passes, COL_TX x COL_TY flat columns x rows in the
# column passes): one case each with W, and with H, one below, at and one above an extent
ROW_TX, ROW_TY = 256, 4
COL_TX, COL_TY = 64, 64
EXTENT_SHAPES = [(1, 6, ROW_TX - 1, 1, 7, 1.5), (1, 6, ROW_TX, 1, 7, 1.5), (1, 6, ROW_TX + 1, 1, 7, 1.5),
                 (1, COL_TY - 1, COL_TX + 1, 1, 7, 1.5), (1, COL_TY, COL_TX, 1, 7, 1.5), (1, COL_TY + 1, COL_TX - 1, 1, 7, 1.5),
                 (1, ROW_TY + 1, 9, 2, 5, 1.0)]
ALL_SHAPES = B.SHAPES + EXTENT_SHAPES

_cache = {}


def _case(shape):
    """Inputs, taps and the float64 / float32 references of a shape, computed once and shared (nobody writes to them)."""
    if shape not in _cache:
        Bn, H, W, C, k, sigma = shape
        colour, cover, ref = B.inputs(Bn, H, W, C)
        g = B.taps(k, sigma)
        _cache[shape] = dict(colour=colour, cover=cover, ref=ref, g=g, E=B.blurred_residual(colour, cover, ref, g),
                             E32=B.blurred_residual(colour, cover, ref, g, dtype=torch.float32)[0])
    return _cache[shape]


def _gpu(c):
    rast = torch.zeros(c['colour'].shape[:3] + (4,), device='cuda')
    rast[..., 3] = c['cover'].cuda()
    return c['colour'].cuda(), rast, c['ref'].cuda()


def long_sum(case, name, x, ref, x32, zeros=0):
    r, S = ref
    e, nz = R.measure(x, r, S)
    e32, _ = R.measure(x32, r, S)
    print(f"BLUR {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={8 * e32 + 4:.1f}")
    assert nz == zeros, (case, name, nz, zeros)
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_blur_loss_entries_against_float64(shape):
    import fpc_diffrend_amd.ops as dr
    c = _case(shape)
    Bn, H, W, C, k, sigma = shape
    case = f"blur({Bn},{H},{W},{C})k{k}"
    cg, rast, rg = _gpu(c)
    uncovered = int((c['cover'] <= 0).sum())
    for n_total in (None, 3 * c['colour'].numel() + 1):
        gs = 1.0 / (n_total or c['colour'].numel())
        s, grad, E = dr.blur_loss_call(cg, rast, rg, c['g'], gs)
        tag = case + ('' if n_total is None else '/n_total')
        long_sum(tag, 'E', E, c['E'], c['E32'])
        Ec = E.cpu()
        E64 = Ec.double()
        long_sum(tag, 'sum', s.reshape(()), ((E64 * E64).sum(), (E64 * E64).sum()), (Ec * Ec).sum())
        long_sum(tag, 'grad', grad, B.gradient(Ec, c['cover'], c['g'], n_total), B.gradient(Ec, c['cover'], c['g'], n_total, dtype=torch.float32)[0],
                 zeros=C * uncovered)
        unc = (c['cover'] <= 0)[..., None].expand_as(Ec)
        assert bool((grad.cpu()[unc] == 0).all())
    # a second identical call, and the value-only call (grad_color NULL: two of the four passes), bit for bit
    s2, grad2, E2 = dr.blur_loss_call(cg, rast, rg, c['g'], gs)
    assert torch.equal(E2, E) and torch.equal(grad2, grad)
    s3, grad3, E3 = dr.blur_loss_call(cg, rast, rg, c['g'], gs, want_grad=False)
    assert grad3 is None and torch.equal(E3, E)
    assert abs(float(s3) - float(s)) <= 1e-12 * float(s)


def test_images_are_independent():
    """Nothing crosses an image boundary of the flat buffer: other inputs for image 0 leave image 1's E and gradient bit-identical."""
    import fpc_diffrend_amd.ops as dr
    shape = (2, 37, 70, 1, 31, 2.0)
    c = _case(shape)
    cg, rast, rg = _gpu(c)
    gs = 1.0 / c['colour'].numel()
    _, grad, E = dr.blur_loss_call(cg, rast, rg, c['g'], gs)
    colour2, cover2, ref2 = B.inputs(*shape[:4], seed=11)
    cg2, rast2, rg2 = cg.clone(), rast.clone(), rg.clone()
    cg2[0], rg2[0] = colour2[0].cuda(), ref2[0].cuda()
    rast2[0, ..., 3] = cover2[0].cuda()
    _, grad2, E2 = dr.blur_loss_call(cg2, rast2, rg2, c['g'], gs)
    assert torch.equal(E2[1], E[1]) and torch.equal(grad2[1], grad[1])
    assert not torch.equal(E2[0], E[0])


def test_identity_taps_give_the_pixel_loss():
    """Taps (0, 1, 0): E is the residual itself, so value and gradient are those of fpcdr_pixel_loss on the same inputs."""
    from fpc_diffrend_amd import fit
    import fpc_diffrend_amd.ops as dr
    Bn, H, W, C = 2, 37, 53, 3
    colour, cover, ref = B.inputs(Bn, H, W, C, seed=4)
    c = dict(colour=colour, cover=cover, ref=ref)
    cg, rast, rg = _gpu(c)
    s, grad, E = dr.blur_loss_call(cg, rast, rg, torch.tensor([0.0, 1.0, 0.0]), 1.0 / colour.numel())
    s0, grad0 = fit.pixel_loss_fused(cg, rast, rg)
    r64, r32 = R.pixel_loss(colour, cover, ref), R.pixel_loss(colour, cover, ref, dtype=torch.float32)
    e, nz = R.measure(grad, grad0.cpu().double(), r64['grad'][1])
    print(f"BLUR identity grad-vs-pixel_loss e={e:.3f} bound=2.0")
    assert e <= 2.0 and nz == C * int((cover <= 0).sum())
    long_sum('identity', 'sum', s.reshape(()), r64['sum'], r32['sum'][0])
    long_sum('identity', 'pixel_loss sum', s0.reshape(()), r64['sum'], r32['sum'][0])


def test_bad_arguments_are_rejected_without_a_launch():
    from fpc_diffrend_amd import _lib
    import fpc_diffrend_amd.ops as dr
    Bn, H, W, C = 1, 12, 9, 1
    colour, cover, ref = B.inputs(Bn, H, W, C)
    cg, rast, rg = _gpu(dict(colour=colour, cover=cover, ref=ref))
    acc = torch.zeros(1, dtype=torch.float64, device='cuda')
    tmp, blurred, grad = torch.empty_like(cg), torch.full_like(cg, -7.0), torch.full_like(cg, -7.0)

    def params(radius, **over):
        kw = dict(color=_ptr(cg), rast=_ptr(rast), ref=_ptr(rg), B=Bn, H=H, W=W, C=C, bg=B.BACKGROUND, color_scale=255.0,
                  grad_scale=1.0, radius=radius, tmp=_ptr(tmp), blurred=_ptr(blurred), loss_sum=_ptr(acc), grad_color=_ptr(grad))
        kw.update(over)
        p = _lib.BlurLoss(**kw)
        for t in range(min(2 * radius + 1, 64) if radius > 0 else 0):
            p.taps[t] = 1.0 / (2 * radius + 1)
        return p

    bad = [params(32), params(0), params(min(H, W)), params(-1), params(2, tmp=None), params(2, blurred=None), params(2, color=None),
           params(2, rast=None), params(2, ref=None), params(2, loss_sum=None), params(2, C=5), params(2, W=0)]
    for p in bad:                                    # k = 65, k = 1, r = min(H, W), ..., a null plane
        with pytest.raises(RuntimeError):
            _lib.call("fpcdr_blur_loss", ctypes.byref(p), _stream())
    torch.cuda.synchronize()
    assert float(acc) == 0.0 and bool((blurred == -7.0).all()) and bool((grad == -7.0).all())        # nothing ran
    _lib.call("fpcdr_blur_loss", ctypes.byref(params(min(H, W) - 1)), _stream())                      # the largest legal radius does
    torch.cuda.synchronize()
    assert float(acc) > 0.0
    for kw in (dict(sigma=2.0, kernel_size=8), dict(sigma=2.0, kernel_size=65), dict(sigma=2.0, kernel_size=2 * min(H, W) + 1),
               dict(sigma=0.0, kernel_size=5), dict(sigma=None, kernel_size=5), dict(taps=torch.ones(4) / 4),
               dict(taps=torch.ones(2 * min(H, W) + 1))):
        with pytest.raises(ValueError):
            dr.blurred_pixel_loss(cg, rast, rg, **kw)
    with pytest.raises(ValueError):
        dr.blurred_pixel_loss(colour, rast, rg, sigma=2.0, kernel_size=5)            # a CPU tensor


def test_ops_blurred_pixel_loss_value_and_backward():
    import fpc_diffrend_amd.ops as dr
    shape = (2, 37, 70, 1, 31, 2.0)
    c = _case(shape)
    cg, rast, rg = _gpu(c)
    for n_total in (None, 5 * c['colour'].numel()):
        n = n_total or c['colour'].numel()
        s, grad, _ = dr.blur_loss_call(cg, rast, rg, c['g'], 1.0 / n)
        x = cg.clone().requires_grad_(True)
        loss = dr.blurred_pixel_loss(x, rast, rg, sigma=2.0, kernel_size=31, n_total=n_total)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert float(loss.detach()) == float((s[0] / n).to(torch.float32))
        (0.5 * loss).backward()
        assert torch.equal(x.grad, 0.5 * grad)
        y = cg.clone().requires_grad_(True)
        dr.blurred_pixel_loss(y, rast, rg, taps=c['g'], n_total=n_total).backward()      # taps= overrides sigma and kernel_size
        assert torch.equal(y.grad, grad)


def test_fitter_blurred_iterations_then_the_one_pass_objective():
    """A Fitter with blur_sigma > 0: the parameter gradients of a blurred iteration equal those autograd gives through the same GPU
    operators with a torch-made loss (F.pad(reflect) + two conv2d), within the project's 1e-4 relative L2; from iteration blur_iters on
    the step is the one-pass objective's; the options that cannot be combined raise."""
    from fpc_diffrend_amd import fit, scene
    sc = scene.make_scene(resolution=(96, 96), n_frames=2)
    kw = dict(weight_laplacian=0, max_iter=4, cam_idxs=(0, 4))
    cfg = fit.FitConfig(blur_sigma=3, blur_kernel_size=15, blur_iters=2, **kw)
    fr = slice(0, 2)
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.7)
    loss = ft.loss_and_backward(fr)
    # the same chain by hand, with the loss as a plain torch expression
    ft2 = fit.Fitter(sc, cfg, device='cuda')
    ft2.init_near_truth(0.7)
    vtx = ft2.vertices(fr, validate=False).reshape(2, -1, 3)
    pos_clip = fit.transform_clip_batched(ft2.mvp(fr, None, None, validate=False), vtx)
    colour, rast = fit.render_from_clip(ft2.glctx, pos_clip, ft2.pos_idx, ft2.uv, ft2.uv_idx, ft2.tex_opt, ft2.resolution,
                                        cfg.enable_mip, cfg.max_mip_level, cfg.fused_render)
    ref = ft2.targets.reshape(-1, *ft2.resolution)
    taps = B.taps(15, 3.0)
    assert torch.equal(ft.blur_taps(0), taps)
    loss2 = B.loss_plain(colour, rast[..., 3], ref, taps)
    loss2.backward()
    print(f"BLUR fitter loss {float(loss):.6f} torch {float(loss2):.6f}")
    assert abs(float(loss) - float(loss2)) <= 1e-5 * abs(float(loss2))
    seen = 0
    for name, p, p2 in zip(("m1", "m2", "m3", "maps", "maps_intermediate", "t_opt", "q_opt", "per_frame_t", "per_frame_q", "tex_opt"),
                           ft.params, ft2.params):
        assert (p.grad is None) == (p2.grad is None), name
        if p.grad is not None:
            err = R.rel_l2(p.grad, p2.grad)
            print(f"BLUR fitter grad {name} rel_l2={err:.2e} bound=1e-4")
            assert float(p2.grad.abs().max()) > 0 and err < 1e-4, (name, err)
            seen += 1
    assert seen >= 6
    # iteration 2 onwards: the one-pass objective, as a Fitter without the blur runs it on the same state
    assert ft.blur_taps(1) is not None and ft.blur_taps(2) is None
    ft.iteration = 2
    loss_after = ft.loss_and_backward(fr)
    ft0 = fit.Fitter(sc, fit.FitConfig(**kw), device='cuda')
    ft0.init_near_truth(0.7)
    ft0.iteration = 2
    loss0 = ft0.loss_and_backward(fr)
    assert abs(float(loss_after) - float(loss0)) <= 1e-6 * abs(float(loss0)), (float(loss_after), float(loss0))
    assert abs(float(loss_after) - float(loss)) > 1e-3 * abs(float(loss0))               # (and the blurred value was another one)
    ft2.load_state_dict(ft.state_dict())
    assert ft2.iteration == 2 and ft2.blur_taps() is None        # a resumed run continues on the right side of the switch
    for bad, words in ((dict(fused_loss=False), ("blur_sigma", "fused_loss")), (dict(hip_graph=True), ("blur_sigma", "hip_graph"))):
        with pytest.raises(ValueError) as ei:
            fit.Fitter(sc, fit.FitConfig(blur_sigma=3, blur_kernel_size=15, **kw, **bad), device='cuda')
        assert all(w in str(ei.value) for w in words)
    # sigma goes geometrically from blur_sigma to blur_sigma_end over the blurred iterations
    import dataclasses
    ft2.cfg = dataclasses.replace(cfg, blur_sigma=4, blur_sigma_end=1, blur_iters=3)
    assert torch.equal(ft2.blur_taps(0), B.taps(15, 4.0)) and torch.equal(ft2.blur_taps(1), B.taps(15, 2.0))
    assert torch.equal(ft2.blur_taps(2), B.taps(15, 1.0)) and ft2.blur_taps(3) is None

"""GPU: the weighted robust pixel loss (csrc/robust.hip, fpcdr_robust_loss) entry by entry against float64 (tests/robust_ref.py), and
the options that put a Fitter's iterations on it.

Conventions of tests/test_gpu_fitstep.py: the error of an output x with float64 reference r is e = max_i |x_i - r_i| / S_i in units of
u = 2^-24, S_i the scale of entry i; entries with S_i = 0 must be exactly 0 and their number the one predicted (uncovered pixels and
pixels of weight 0 -- a mask byte of 0, a face weight of 0, a saturated capture pixel, an id past the table -- times C).  The gradient
is held to (n + 2) u with n derived in tests/robust_ref.py (L2 8, Charbonnier 15, Geman-McClure 19); both sums are long sums: e <= 8 *
e32 + 4, e32 the error of float32 torch on the CPU for the same sum against the same reference (test_gpu_blur.py's bar, for its reason:
the order of a float32 sum is the kernel's own).  Shapes (robust_ref.SMALL_SHAPES, loop_shape): pixel counts one below, at and one above
a 16-pixel chunk, a wave's trip (256) and a workgroup's trip (1024), C = 1 and 3, B = 2, and a count that gives every lane of the full
grid (6 workgroups a compute unit) two trips and a ragged third.  Every case runs with every buffer at an aligned base and at a base
offset by 1 .. 15 elements, with and without mask, face weights and saturation, w_outside 1, 0.25 and 0, all three kinds, c = 2 and 20.
Every line below is printed by a test as "ROBUST ..." (pytest -s).

Measured on an MI355X at 6ed0942 plus the change that adds this file (units of u; the largest over the cases of a row -- 502 calls: ten
small shapes x the kinds and scales x five option sets x two placements, and the two loop cases); the gradient is bit-identical from
run to run, the sums move in their last bits with the order of the atomics.  The whole file runs in 5.6 s there, 2 s of them the first
Fitter test:

  output                      kind            max e_gpu   bound     where
  grad, small shapes          L2                  2.87      10      (1,3,341,1)
  grad, small shapes          Charbonnier         2.62      17      (1,1,257,1)
  grad, small shapes          Geman-McClure       4.03      21      (1,1,257,1)
  grad, loop shape            Charbonnier         4.36      17      (2,1541,1021,1), 3.1 M pixels, everything on, aligned
  grad, loop shape            Geman-McClure       5.39      21      the same shape, mask, every buffer off its alignment
  sum w rho                   all                 0.29      max e32 0.59; closest to its own bound 0.05 of it
  sum w                       all                 1.60      max e32 21.5; closest to its own bound 0.11 of it
  L2, nothing on: grad against fpcdr_pixel_loss's bit-identical; sum 0.02 (e32 0.12, bound 4.9), fpcdr_pixel_loss's own 0.002
  Fitter, full size: loss 15.441944 against torch's 15.441946; parameter gradients against autograd through the same operators,
          relative L2 2.9e-08 (per_frame_t) .. 1.7e-07 (maps), bound 1e-4
  Fitter, pyramid factor 2: loss 12.698143 against 12.698144; 9.0e-08 (q_opt) .. 5.3e-07 (maps_intermediate), bound 1e-4
"""
import ctypes

import numpy as np
import pytest
import torch

import fitstep_ref as R
import robust_ref as RR

pytestmark = pytest.mark.gpu

_cache = {}


def _inputs(shape):
    if shape not in _cache:
        _cache[shape] = RR.inputs(*shape)
    return _cache[shape]


def _reference(shape, kind, c, opt):
    """The float64 and float32 statements of a case, computed once and shared (nobody writes to them)."""
    key = (shape, kind, c, opt[0])
    if key not in _cache:
        inp = _inputs(shape)
        kw = RR.option_kwargs(inp, opt)
        _cache[key] = (RR.robust_loss(inp['colour'], inp['rast_w'], inp['ref'], kind, c, **kw),
                       RR.robust_loss(inp['colour'], inp['rast_w'], inp['ref'], kind, c, dtype=torch.float32, **kw))
    return _cache[key]


def _at(t, off):
    """t on the GPU as a contiguous view that starts `off` elements into its buffer."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device='cuda')
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off * t.element_size()
    return v


def _gpu(inp, offs=(0, 0, 0, 0, 0)):
    rast = torch.zeros(inp['colour'].shape[:3] + (4,))
    rast[..., 3] = inp['rast_w']
    return dict(colour=_at(inp['colour'], offs[0]), rast=_at(rast, offs[1]), ref=_at(inp['ref'], offs[2]), mask=_at(inp['mask'], offs[3]),
                face_w=_at(inp['face_w'], offs[4]))


def _call(g, kind, c, opt, grad_scale, want_grad=True):
    import fpc_diffrend_amd.ops as dr
    _, use_mask, use_faces, sat, w_out = opt
    return dr.robust_loss_call(g['colour'], g['rast'], g['ref'], kind, c, grad_scale, mask=g['mask'] if use_mask else None,
                               face_weights=g['face_w'] if use_faces else None, weight_outside=w_out, saturation=sat, want_grad=want_grad)


def long_sum(case, name, x, r, S, x32):
    e, _ = R.measure(x, r, S)
    e32, _ = R.measure(x32, r, S)
    print(f"ROBUST {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={8 * e32 + 4:.1f}")
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _check_case(shape, kind, c, opt, offs):
    inp = _inputs(shape)
    C = shape[3]
    r64, r32 = _reference(shape, kind, c, opt)
    g = _gpu(inp, offs)
    gs = 1.0 / inp['colour'].numel()
    sums, grad = _call(g, kind, c, opt, gs)
    case = f"{'x'.join(map(str, shape))} {kind} c={c} {opt[0]} offs={offs}"
    e, nz = R.measure(grad, *r64['grad'])
    bound = RR.N_GRAD[kind] + 2
    print(f"ROBUST {case} grad e_gpu={e:.3f} bound={bound} zeros={nz}")
    assert e <= bound, (case, e)
    assert nz == RR.predicted_zeros(inp['rast_w'], r64['w'], C), case
    for k, name in ((0, 'sum w rho'), (1, 'sum w')):
        long_sum(case, name, sums[k], r64['sums'][0][k], r64['sums'][1][k], r32['sums'][0][k])
    # a second identical call: bit for bit; the value-only call: the same sums up to the order of the atomics
    sums2, grad2 = _call(g, kind, c, opt, gs)
    assert torch.equal(grad2, grad)
    sums3, grad3 = _call(g, kind, c, opt, gs, want_grad=False)
    assert grad3 is None
    for k in (0, 1):
        assert abs(float(sums3[k]) - float(sums[k])) <= 1e-12 * abs(float(sums[k])), (case, k)
    return e


OFFSETS = [(0, 0, 0, 0, 0), (1, 3, 1, 7, 1), (5, 2, 15, 3, 2), (3, 1, 8, 13, 3)]


@pytest.mark.parametrize("shape", RR.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_robust_loss_entries_against_float64(shape):
    worst = {k: 0.0 for k in RR.KINDS}
    i = RR.SMALL_SHAPES.index(shape)
    for kind in RR.KINDS:
        for c in ((None,) if kind == 'l2' else RR.SCALES):
            for j, opt in enumerate(RR.OPTIONS):
                for offs in (OFFSETS[0], OFFSETS[1 + (i + j) % 3]):
                    worst[kind] = max(worst[kind], _check_case(shape, kind, c, opt, offs))
    print(f"ROBUST worst grad {shape} " + " ".join(f"{k}={v:.2f}/{RR.N_GRAD[k] + 2}" for k, v in worst.items()))


def test_every_lane_takes_two_trips_and_a_ragged_third():
    """The grid is sized from the device: the shape is derived from its number of compute units."""
    shape = RR.loop_shape(torch.cuda.get_device_properties(0).multi_processor_count)
    _check_case(shape, 'charbonnier', RR.SCALES[0], RR.OPTIONS[-1], OFFSETS[0])
    _check_case(shape, 'geman_mcclure', RR.SCALES[1], RR.OPTIONS[1], OFFSETS[2])
    _cache.clear()


def test_l2_with_nothing_on_is_the_pixel_loss_bit_for_bit():
    from fpc_diffrend_amd import fit
    shape = (2, 37, 53, 3)
    inp = _inputs(shape)
    g = _gpu(inp)
    n = inp['colour'].numel()
    sums, grad = _call(g, 'l2', None, RR.OPTIONS[0], 1.0 / n)
    s0, grad0 = fit.pixel_loss_fused(g['colour'], g['rast'], g['ref'])
    assert torch.equal(grad, grad0)
    r64 = R.pixel_loss(inp['colour'], inp['rast_w'], inp['ref'])
    r32 = R.pixel_loss(inp['colour'], inp['rast_w'], inp['ref'], dtype=torch.float32)
    long_sum('l2-identity', 'sum', sums[0], r64['sum'][0], r64['sum'][1], r32['sum'][0])
    long_sum('l2-identity', 'pixel_loss sum', s0.reshape(()), r64['sum'][0], r64['sum'][1], r32['sum'][0])
    assert float(sums[1]) == float(n)                       # every weight is 1: the float32 lane sums are exact


def test_an_id_above_the_table_weighs_nothing():
    """A hand-made rast with ids T + 1, T + 2 and one far above: weight 0, gradient exactly 0, the other pixels as the statement."""
    import fpc_diffrend_amd.ops as dr
    Bn, H, W, C, T = 1, 4, 9, 1, 5
    inp = RR.inputs(Bn, H, W, C, seed=9, T=T)
    ids = inp['rast_w'].clone()
    ids[0, 0, :3] = torch.tensor([T + 1.0, T + 2.0, 3.0e9])
    ids[0, 1, 0] = float(T)                                 # the last entry of the table
    g = _gpu(dict(inp, rast_w=ids))
    sums, grad = dr.robust_loss_call(g['colour'], g['rast'], g['ref'], 'charbonnier', 20.0, 1.0, face_weights=g['face_w'])
    ref = RR.robust_loss(inp['colour'], ids, inp['ref'], 'charbonnier', 20.0, n_total=1, face_w=inp['face_w'])
    assert bool((ref['w'][0, 0, :3] == 0).all()) and bool((grad[0, 0, :3] == 0).all())
    assert float(ref['w'][0, 1, 0]) == float(inp['face_w'][T - 1]) and float(grad[0, 1, 0, 0]) != 0.0
    e, nz = R.measure(grad, *ref['grad'])
    assert e <= RR.N_GRAD['charbonnier'] + 2 and nz == RR.predicted_zeros(ids, ref['w'], C)
    assert abs(float(sums[1]) - float(ref['sums'][0][1])) <= 1e-5 * float(ref['sums'][0][1])


def test_images_are_independent():
    shape = (2, 37, 53, 3)
    inp = _inputs(shape)
    g = _gpu(inp)
    gs = 1.0 / inp['colour'].numel()
    _, grad = _call(g, 'geman_mcclure', 20.0, RR.OPTIONS[-1], gs)
    other = RR.inputs(*shape, seed=11)
    g2 = {k: v.clone() for k, v in g.items()}
    rast_o = torch.zeros(shape[:3] + (4,))
    rast_o[..., 3] = other['rast_w']
    g2['colour'][0], g2['ref'][0], g2['mask'][0], g2['rast'][0] = other['colour'][0].cuda(), other['ref'][0].cuda(), other['mask'][0].cuda(), rast_o[0].cuda()
    _, grad2 = _call(g2, 'geman_mcclure', 20.0, RR.OPTIONS[-1], gs)
    assert torch.equal(grad2[1], grad[1]) and not torch.equal(grad2[0], grad[0])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def test_bad_arguments_are_rejected_with_a_message_and_without_a_launch():
    from fpc_diffrend_amd import _lib
    inp = _inputs((1, 16, 16, 1))
    g = _gpu(inp)
    sums = torch.zeros(2, dtype=torch.float64, device='cuda')
    grad = torch.full_like(g['colour'], -7.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def params(**over):
        kw = dict(color=_ptr(g['colour']), rast=_ptr(g['rast']), ref=_ptr(g['ref']), B=1, H=16, W=16, C=1, bg=RR.BACKGROUND, color_scale=255.0,
                  grad_scale=1.0, kind=1, inv_c=0.1, w_outside=1.0, sat=0, mask=_ptr(g['mask']), face_w=_ptr(g['face_w']), T=inp['T'],
                  sums=_ptr(sums), grad_color=_ptr(grad))
        kw.update(over)
        return _lib.RobustLoss(**kw)

    bad = [params(kind=3), params(inv_c=0.0), params(inv_c=float('nan')), params(kind=2, inv_c=float('inf')), params(w_outside=-1.0),
           params(w_outside=float('inf')), params(sat=256), params(sat=-1), params(T=0), params(color=None), params(rast=None),
           params(ref=None), params(sums=None), params(W=0), params(C=0)]
    for i, p in enumerate(bad):
        with pytest.raises(RuntimeError, match="fpcdr_robust_loss"):
            _lib.call("fpcdr_robust_loss", ctypes.byref(p), stream)
    torch.cuda.synchronize()
    assert float(sums.abs().sum()) == 0.0 and bool((grad == -7.0).all())        # nothing ran
    _lib.call("fpcdr_robust_loss", ctypes.byref(params(kind=0, inv_c=0.0)), stream)      # L2 ignores inv_c
    torch.cuda.synchronize()
    assert float(sums[0]) > 0.0 and not bool((grad == -7.0).any())


def test_ops_robust_pixel_loss_value_and_backward():
    import fpc_diffrend_amd.ops as dr
    shape = (2, 37, 53, 3)
    inp = _inputs(shape)
    g = _gpu(inp)
    for n_total in (None, 5 * inp['colour'].numel()):
        n = n_total or inp['colour'].numel()
        sums, grad = dr.robust_loss_call(g['colour'], g['rast'], g['ref'], 'charbonnier', 20.0, 1.0 / n, mask=g['mask'], saturation=RR.SAT)
        x = g['colour'].clone().requires_grad_(True)
        loss = dr.robust_pixel_loss(x, g['rast'], g['ref'], kind='charbonnier', scale=20.0, n_total=n_total, mask=g['mask'], saturation=RR.SAT)
        assert loss.dtype == torch.float32 and loss.dim() == 0
        assert abs(float(loss.detach()) - float((sums[0] / n).to(torch.float32))) <= 1e-6 * float(loss.detach())
        (0.5 * loss).backward()
        assert torch.equal(x.grad, 0.5 * grad)
    with pytest.raises(ValueError):
        dr.robust_pixel_loss(g['colour'], g['rast'], g['ref'], kind='charbonnier')                    # no default scale
    with pytest.raises(ValueError):
        dr.robust_loss_call(g['colour'], g['rast'], g['ref'], 'l2', None, 1.0, mask=g['mask'][:, :5])
    with pytest.raises(ValueError):
        dr.robust_loss_call(g['colour'], g['rast'], g['ref'], 'l2', None, 1.0, face_weights=-g['face_w'] - 1.0)
    with pytest.raises(ValueError):
        dr.robust_loss_call(g['colour'], g['rast'], g['ref'], 'l2', None, 1.0, mask=g['mask'].float())


# ---- the Fitter -------------------------------------------------------------------------------------------------------------------------
PARAMS = ("m1", "m2", "m3", "maps", "maps_intermediate", "t_opt", "q_opt", "per_frame_t", "per_frame_q", "tex_opt")
FIT_KW = dict(weight_laplacian=0, max_iter=4, cam_idxs=(0, 4))


def _masked_scene():
    from fpc_diffrend_amd import scene
    sc = scene.make_scene(resolution=(64, 64), n_frames=2)
    rng = np.random.default_rng(3)
    masks = rng.integers(0, 256, size=(2, len(sc.cams), 64, 64)).astype(np.uint8)
    masks[:, :, 20:30, 20:44] = 0
    masks[:, :, 34:50, 10:50] = 255
    face_w = rng.uniform(0.0, 1.5, size=sc.pos_idx.shape[0]).astype(np.float32)
    face_w[rng.uniform(size=face_w.shape[0]) < 0.2] = 0.0
    return sc, masks, face_w


@pytest.mark.parametrize("pyramid", [(), ((2, 4),)], ids=["full", "factor2"])
def test_fitter_robust_step_against_autograd_through_the_same_operators(pyramid):
    """Measured on an MI355X: printed as "ROBUST fitter ..."; bound 1e-4 relative L2, the project's bar."""
    import dataclasses
    from fpc_diffrend_amd import fit
    sc, masks, face_w = _masked_scene()
    sc = dataclasses.replace(sc, masks=masks)
    cfg = fit.FitConfig(robust='charbonnier', robust_scale=10.0, face_weights=face_w, weight_outside=0.25, saturation=130, pyramid=pyramid, **FIT_KW)
    fr = slice(0, 2)
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.7)
    loss = ft.loss_and_backward(fr)
    s = 2 if pyramid else 1
    assert ft.resolution == (64 // s, 64 // s) and tuple(ft.masks.shape) == (2, 2, 64 // s, 64 // s) and ft.full_masks.shape[-1] == 64
    assert ft._wsum is not None and 0.0 < float(ft._wsum) < 4 * ft.resolution[0] * ft.resolution[1]
    import fpc_diffrend_amd.ops as dr
    if pyramid:
        assert torch.equal(ft.masks, dr.downsample_images(ft.full_masks, 2))
    # the same chain by hand, with the loss as a plain torch expression of the rule in float32
    ft2 = fit.Fitter(sc, cfg, device='cuda')
    ft2.init_near_truth(0.7)
    vtx = ft2.vertices(fr, validate=False).reshape(2, -1, 3)
    pos_clip = fit.transform_clip_batched(ft2.mvp(fr, None, None, validate=False), vtx)
    colour, rast = fit.render_from_clip(ft2.glctx, pos_clip, ft2.pos_idx, ft2.uv, ft2.uv_idx, ft2.tex_opt, ft2.resolution,
                                        ft2.enable_mip, cfg.max_mip_level, cfg.fused_render)
    ref = ft2.targets.reshape(-1, *ft2.resolution)
    w, _ = RR.weights(rast[..., 3], ref, ft2.masks.reshape(-1, *ft2.resolution), torch.from_numpy(face_w), 0.25, 130, dtype=torch.float32)
    loss2 = RR.loss_plain(colour, rast[..., 3], ref, 'charbonnier', 10.0, weight=w.cuda())
    loss2.backward()
    print(f"ROBUST fitter {'factor 2' if pyramid else 'full size'} loss {float(loss):.6f} torch {float(loss2.detach()):.6f}")
    assert abs(float(loss) - float(loss2.detach())) <= 1e-5 * abs(float(loss2.detach()))
    seen = 0
    for name, p, p2 in zip(PARAMS, ft.params, ft2.params):
        assert (p.grad is None) == (p2.grad is None), name
        if p.grad is not None:
            err = R.rel_l2(p.grad, p2.grad)
            print(f"ROBUST fitter {'factor 2' if pyramid else 'full size'} grad {name} rel_l2={err:.2e} bound=1e-4")
            assert float(p2.grad.abs().max()) > 0 and err < 1e-4, (name, err)
            seen += 1
    assert seen >= 6


def test_fitter_robust_iters_then_the_default_path_and_off_means_the_one_pass_objective(monkeypatch):
    import dataclasses
    from fpc_diffrend_amd import fit
    sc, masks, face_w = _masked_scene()
    calls = []
    real = fit.pixel_loss_robust
    monkeypatch.setattr(fit, "pixel_loss_robust", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    fr = slice(0, 2)
    # robust_iters = 1: iteration 0 on the robust term, iteration 1 the step of a default Fitter on the same state
    ft = fit.Fitter(sc, fit.FitConfig(robust='charbonnier', robust_scale=10.0, robust_iters=1, **FIT_KW), device='cuda')
    ft.init_near_truth(0.7)
    assert ft.robust_term(0) == ('charbonnier', 10.0) and ft.robust_term(1) is None
    loss_robust = ft.loss_and_backward(fr)
    assert calls == ['charbonnier'] and ft._wsum is not None
    ft.iteration = 1
    loss_after = ft.loss_and_backward(fr)
    assert calls == ['charbonnier'] and ft._wsum is None
    ft0 = fit.Fitter(sc, fit.FitConfig(**FIT_KW), device='cuda')
    ft0.init_near_truth(0.7)
    ft0.iteration = 1
    loss0 = ft0.loss_and_backward(fr)
    assert calls == ['charbonnier']                                       # a default FitConfig on a scene without masks: the one-pass path
    assert abs(float(loss_after) - float(loss0)) <= 1e-6 * abs(float(loss0)), (float(loss_after), float(loss0))
    assert abs(float(loss_robust) - float(loss0)) > 1e-3 * abs(float(loss0))
    for name, p, p0 in zip(PARAMS, ft.params, ft0.params):
        assert (p.grad is None) == (p0.grad is None), name
        if p.grad is not None:
            assert R.rel_l2(p.grad, p0.grad) < 1e-4, name
    ft0.load_state_dict(ft.state_dict())
    assert ft0.iteration == 1
    # a scene with masks: ignored with use_masks=False, kind 'l2' with them; weights alone are kind 'l2' too
    scm = dataclasses.replace(sc, masks=masks)
    ftm = fit.Fitter(scm, fit.FitConfig(use_masks=False, **FIT_KW), device='cuda')
    ftm.init_near_truth(0.7)
    ftm.loss_and_backward(fr)
    assert calls == ['charbonnier'] and ftm.masks is None
    ftm = fit.Fitter(scm, fit.FitConfig(**FIT_KW), device='cuda')
    ftm.init_near_truth(0.7)
    ftm.loss_and_backward(fr)
    assert calls == ['charbonnier', 'l2'] and ftm.robust_term(10 ** 6) == ('l2', None)
    ftw = fit.Fitter(sc, fit.FitConfig(weight_outside=0.0, **FIT_KW), device='cuda')
    ftw.init_near_truth(0.7)
    ftw.loss_and_backward(fr)
    assert calls == ['charbonnier', 'l2', 'l2']
    # what cannot be combined raises at construction
    for sc_, bad in ((sc, dict(robust='l2', fused_loss=False)), (sc, dict(saturation=140, hip_graph=True)), (scm, dict(hip_graph=True)),
                     (scm, dict(blur_sigma=3.0, blur_kernel_size=15)), (scm, dict(norm_sigma=3.0, norm_kernel_size=15)),
                     (sc, dict(face_weights=face_w[:-1])), (dataclasses.replace(sc, masks=masks[:, :, :32]), dict())):
        with pytest.raises(ValueError):
            fit.Fitter(sc_, fit.FitConfig(**FIT_KW, **bad), device='cuda')
    fit.Fitter(scm, fit.FitConfig(blur_sigma=3.0, blur_kernel_size=15, use_masks=False, **FIT_KW), device='cuda')


def test_step_log_carries_wsum_on_robust_iterations_only(tmp_path):
    import json
    from fpc_diffrend_amd import fit
    sc, _, _ = _masked_scene()
    log = tmp_path / "steps.jsonl"
    cfg = fit.FitConfig(robust='geman_mcclure', robust_scale=10.0, robust_iters=1, weight_outside=1.0, log_interval=1, reg_log_interval=0,
                        log_path=str(log), **FIT_KW)
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.7)
    ft.step()
    ft.step()
    recs = [json.loads(l) for l in log.read_text().splitlines()]
    assert [r["it"] for r in recs] == [0, 1]
    n = 2 * 2 * 64 * 64                                     # every weight is 1: the sum of the weights is the number of entries
    assert recs[0]["wsum"] == float(n) and "wsum" not in recs[1]
    assert all(np.isfinite(r["loss"]) for r in recs)

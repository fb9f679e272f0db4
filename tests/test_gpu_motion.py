"""GPU: the motion term (csrc/mesh_reg.hip k_motion_penalty<1>, <2>, k_penalty_finish; fpcdr_motion_penalty, fit.motion_penalty,
FitConfig.weight_motion / motion_order / motion_scale / motion_vertex_weights) entry by entry against float64 (tests/motion_ref.py),
and inside a Fitter: eager, on a random subset of the frames, under a captured graph, on the second of two ranks.

The convention is tests/test_gpu_rest.py's: the error of an output x with float64 reference r is e = max_i |x_i - r_i| / S_i in units of
u = 2^-24, S_i the sum of the absolute values of the terms of entry i (every subtraction charges the absolute values of its operands:
positions sit at y + 170, so x_{f-1} - 2 x_f + x_{f+1} cancels for real); entries with S_i = 0 have no term, must be exactly 0, and their
number must be the one the frame numbers (and the zero weights) predict.  Every output -- per_f, the value, the gradient -- is a sum or
a chain through a root and a division: e <= 8 * e32 + 4, e32 the error of float32 torch on the CPU for the same expression against the
same reference; beside it the rel-L2 of the same outputs against float64 is held to the project's 1e-4 -- with scales that carry the 170
of the positions it is the figure that would show a lost frame.  Every line is printed as "MOTION case name e_gpu e32 bound" (pytest -s).
The Charbonnier scale of a case is the median |a| of its valid stencils, so both regimes occur.

Measured on an MI355X (units of u; the largest over the 338 cases of a row: 288 of consecutive frames -- V in {1, 3, 255, 256, 257, 514} x
F in {1, 2, 3, 4, 5, 33} x both orders x with / without weights x with / without a scale --, 48 with frame numbers and 2 of 300 frames; the
last column is the case that came closest to its own bound).  The per and value rows read 0.00 because their scales carry the 170 of the
positions squared; the rel-L2 of the same outputs against float64, printed beside them, is at most 1.2e-7 (per), 1.1e-7 (value) and
1.6e-7 (gradient) over all cases, against the bar of 1e-4.  The kernel forms the acceleration from two exact differences, float32 torch
in the order of the rule's text: hence e32 above e_gpu.  The whole file runs in 7 s there:

  output                 cases max e_gpu  max e32   closest to its bound (e_gpu / bound, case)
  per                      338      0.00     0.00   -
  value                    338      0.00     0.00   -
  grad                     338      3.21    11.54   2.15 / 10.7  V255/F4/null/o2/w/c
  grad lazy                338      4.02    10.26   2.15 / 8.0  V255/F4/null/o2/w/c
  grad eager_grad          338      4.02    10.26   2.15 / 8.0  V255/F4/null/o2/w/c
  grad acc                 338      4.02    10.26   2.15 / 8.0  V255/F4/null/o2/w/c

Fitter (cfg1, cameras 0 and 3, five frames, init_near_truth(0.8); W_MOT = 6e6 for order 2 with plain squares, W_MOT_O1 = 2e7 for order 1
with motion_scale = 0.02 and a quarter of the vertices at weight 0: the weights at which the term's parameter gradient has the size of
the pixel term's, 1.07e4 and 9.8e3 against 1.06e4.  They are this large because the pixel term's gradient is mostly the poses', which
the term does not reach, and because 0.8 of a smooth truth accelerates little.  Both loss paths agree to the digits shown; "worst" is
the largest |(g_on - g_off) - g_term| over the parameter tensors in units of its bar, 1e-4 (|g_on| + |g_off|) of that tensor, as a
range over both paths and two runs -- the pixel term's gradient differs in its last bits from run to run):
  case                 |g_on|     |g_off|    |g_term|   worst              l_on      l_off    l_term
  order 2              1.5047e4   1.0563e4   1.0717e4   6.3e-4 .. 8.3e-4   211.995   4.949    207.046
  order 1, c, weights  1.4408e4   1.0563e4   9.7988e3   4.1e-4 .. 1.3e-3   2790.84   4.949    2785.89
  subset [0,3,4], o1   1.0435e5   1.2761e4   1.0357e5   8.6e-4 .. 1.9e-3   7163.79   4.918    7158.87
  subset [2,3,4], o2   2.2679e4   1.2516e4   1.8913e4   1.8e-3             271.595   6.337    265.257
  rank 1 of 2, o2      6.2616e3   6.2175e3   7.4138e2   1.4e-3             5.31538   3.83619  1.47919
Captured steps (W_GRAPH = 1e5, fourteen steps): eager and graphed losses agree to every digit printed, 9.26600838 .. 4.010752
(prior, the whole shard, order 2) and 35.25639343 .. 27.82787 (combined, three random frames of five a step, order 1).
Weight at zero: the launches and everything a step computes before its backward are torch.equal to a Fitter built without the options;
the parameters after three steps are not torch.equal between two Fitters built WITHOUT the options either (the pixel term's backward
sums with float atomics), so the test holds them to that control pair's own standard (see the test).
Behaviour (mode='free', cfg1, six frames, the true offsets plus per-frame vertex noise of sigma 0.02, thirty steps, W_FREE = 1e4): the
RMS acceleration of Fitter.result starts at 0.08561 (the truth's: 0.00258) and ends at 0.07982 with the term off, at 0.05750 with it on.
Only the ordering is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fitstep_ref as R
import motion_ref as M
from helpers import additive, fitter_near_truth

pytestmark = pytest.mark.gpu

GAPS = [0, 1, 2, 4, 5, 6, 7, 9]
FRAME_LISTS = {'gaps': GAPS, 'pair': [5, 6], 'odd': [0, 2, 4], 'far': [10 ** 6 + t for t in GAPS]}


def _report(case, name, e, e32, bound):
    print(f"MOTION {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={bound:.1f}")


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


@functools.lru_cache(maxsize=None)
def _base(V):
    """Rest positions [V,3] float32 at y + 170: cfg1's mesh at V = 514, random points of a head's size otherwise."""
    if V == 514:
        from fpc_diffrend_amd import scene
        pos = torch.tensor(scene.cfg('cfg1', n_frames=3).v_base).reshape(-1, 3).float().clone()
        assert pos.shape[0] == 514
    else:
        pos = 8.0 * torch.randn(V, 3, generator=torch.Generator().manual_seed(100 + V))
    pos[:, 1] += 170.0
    return pos


def _inputs(V, F, seed):
    """F meshes: the base, a smooth motion (a sine of the frame index per vertex) and independent noise of a tenth of its size."""
    g = torch.Generator().manual_seed(seed)
    amp, ph = 0.5 * torch.randn(V, 3, generator=g), 6.28 * torch.rand(V, 1, generator=g)
    f = torch.arange(F, dtype=torch.float32)[:, None, None]
    return (_base(V)[None] + amp[None] * torch.sin(0.7 * f + ph[None]) + 0.05 * torch.randn(F, V, 3, generator=g)).float().contiguous()


def _weights(V, seed):
    w = 2.0 * torch.rand(V, generator=torch.Generator().manual_seed(seed))
    w[1::3] = 0.0                                           # (V = 1 keeps its one vertex, V = 3 loses one)
    return w.float()


def _call(x, ft, w, inv_c, order, weight, acc, grad=True):
    from fpc_diffrend_amd import _lib
    F, V, _ = x.shape
    gx = torch.full_like(x, float('nan')) if grad else None
    per = torch.full((F,), float('nan'), dtype=torch.float32, device='cuda')
    val = torch.full((), float('nan'), dtype=torch.float32, device='cuda')
    _lib.call("fpcdr_motion_penalty", _ptr(x), _ptr(ft), _ptr(w), float(inv_c), order, _ptr(gx), _ptr(acc), _ptr(per), _ptr(val),
              float(weight), F, V, _stream())
    assert bool((acc == 0).all())                          # the call leaves its accumulators zeroed
    return per, val, gx


def _case(V, F, frames, order, use_w, use_c, seed):
    from fpc_diffrend_amd import fit
    frame_t = None if frames is None else FRAME_LISTS[frames]
    assert frame_t is None or len(frame_t) == F
    case = f"V{V}/F{F}/{frames or 'null'}/o{order}" + ('/w' if use_w else '') + ('/c' if use_c else '')
    x = _inputs(V, F, seed)
    w = _weights(V, seed + 1) if use_w else None
    weight, upstream = 7.5, 0.3
    inv_c = 0.0
    if use_c:      # near the median |a| of the valid stencils: both regimes occur
        m = M.stencil_flags(F, frame_t, order)
        if bool(m.any()):
            xx = x.double()
            acc_ = (xx[:-2] - 2 * xx[1:-1] + xx[2:])[m[1:-1]] if order == 2 else (xx[1:] - xx[:-1])[m[:-1]]
            nrm = acc_.norm(dim=2).reshape(-1)
            c = float(nrm.median())
            assert float(nrm.min()) <= c <= float(nrm.max())
        else:
            c = 0.5
        inv_c = fit.motion_inv_scale(c)
    ref, ref32 = M.motion(x, weight, frame_t, order, inv_c, w), M.motion(x, weight, frame_t, order, inv_c, w, dtype=torch.float32)
    zg, zp = ref['zeros']
    zv = 1 if zp == F else 0
    vref = tuple(t.reshape(1) for t in ref['value'])
    xc = x.cuda()
    ftc = None if frame_t is None else torch.tensor(frame_t, dtype=torch.int64, device='cuda')
    wc = None if w is None else w.cuda()
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')

    # (i) fpcdr_motion_penalty into buffers prefilled with NaN: every entry is written; twice on one acc: bit-identical
    per, val, gx = _call(xc, ftc, wc, inv_c, order, weight, acc)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(per).all()) and bool(torch.isfinite(val))
    long_sum(case, 'per', per, ref['per'], ref32['per'][0], zp)
    long_sum(case, 'value', val.reshape(1), vref, ref32['value'][0].reshape(1), zv)
    long_sum(case, 'grad', gx, ref['grad'], ref32['grad'][0], zg)
    if zp < F:
        rl2 = [R.rel_l2(per, ref['per'][0]), R.rel_l2(val, ref['value'][0]), R.rel_l2(gx, ref['grad'][0])]
        print(f"MOTION {case} rel-L2 per={rl2[0]:.2e} value={rl2[1]:.2e} grad={rl2[2]:.2e}")
        assert max(rl2) <= 1e-4, (case, rl2)
    else:          # no valid stencil (or no weight): exactly 0, all of it
        assert float(val) == 0.0 and float(per.abs().max()) == 0.0 and float(gx.abs().max()) == 0.0
    per2, val2, gx2 = _call(xc, ftc, wc, inv_c, order, weight, acc)
    assert torch.equal(per2, per) and torch.equal(val2, val) and torch.equal(gx2, gx), case
    per3, val3, _ = _call(xc, ftc, wc, inv_c, order, weight, acc, grad=False)      # grad_x = NULL
    assert torch.equal(per3, per) and torch.equal(val3, val), case

    # (ii) fit.motion_penalty: lazy, eager with a unit upstream, eager with a factor, on the caller's acc
    scale = None if inv_c == 0.0 else c
    for kw, upv in ((dict(), upstream), (dict(eager_grad=True, unit_upstream=True), 1.0), (dict(eager_grad=True), upstream),
                    (dict(acc=acc), upstream)):
        leaf = x.cuda().requires_grad_(True)
        value = fit.motion_penalty(leaf, weight, frame_ids=ftc, order=order, scale=scale, vertex_weights=wc, **kw)
        (value * upv).backward() if upv != 1.0 else value.backward()
        assert torch.equal(value.detach(), val), (case, kw)                  # the same call
        if upv == 1.0:
            assert torch.equal(leaf.grad, gx), (case, kw)
        else:
            up32 = float(np.float32(upv))
            long_sum(case, 'grad ' + (','.join(kw) or 'lazy'), leaf.grad, (upv * ref['grad'][0], upv * ref['grad'][1]),
                     up32 * ref32['grad'][0], zg)
            assert torch.equal(leaf.grad, gx * torch.tensor(upv, dtype=torch.float32, device='cuda')), (case, kw)
        assert bool((acc == 0).all())
    with torch.no_grad():                                                    # no gradient asked for: value only
        assert torch.equal(fit.motion_penalty(xc, weight, frame_ids=ftc, order=order, scale=scale, vertex_weights=wc), val)


# the workgroup edges (256 lanes: one workgroup, one lane of a second) and cfg1's mesh; every F below, at and above both stencils' widths,
# and 33 frames
@pytest.mark.parametrize("V", [1, 3, 255, 256, 257, 514])
def test_motion_entries_against_float64_consecutive_frames(V):
    for F in (1, 2, 3, 4, 5, 33):
        for order in (1, 2):
            for use_w, use_c in ((False, False), (True, False), (False, True), (True, True)):
                _case(V, F, None, order, use_w, use_c, seed=1000 + 10 * F + V)


@pytest.mark.parametrize("frames", ['gaps', 'pair', 'odd', 'far'])
def test_motion_entries_against_float64_frame_numbers(frames):
    """Gaps in the frame numbers switch stencils off: [0,1,2,4,5,6,7,9] leaves three of order 2 and five of order 1, [5,6] one of order 1
    and none of order 2, [0,2,4] none at all; the same numbers 10^6 later give the same flags (they are int64 on the device)."""
    F = len(FRAME_LISTS[frames])
    for V in (3, 257, 514):
        for order in (1, 2):
            for use_w, use_c in ((False, False), (True, True)):
                _case(V, F, frames, order, use_w, use_c, seed=2000 + V)
    if frames == 'far':      # ... bit for bit what the small numbers give
        x = _inputs(257, F, 7).cuda()
        acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
        outs = [_call(x, torch.tensor(FRAME_LISTS[k], dtype=torch.int64, device='cuda'), None, 2.0, 2, 3.0, acc) for k in ('gaps', 'far')]
        assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_motion_with_more_frames_than_the_finish_kernels_threads():
    _case(3, 300, None, 2, True, True, seed=31)
    FRAME_LISTS['long'] = [t + t // 7 for t in range(300)]      # a gap after every seventh frame
    _case(3, 300, 'long', 1, False, False, seed=32)


def test_a_nan_in_a_frame_no_stencil_reaches_stays_there():
    """[0,1,2,4,5,6,7,9]: the mesh of frame number 9 belongs to no valid stencil; NaN positions there change nothing anywhere else."""
    x = _inputs(70, 8, 5).cuda()
    ft = torch.tensor(GAPS, dtype=torch.int64, device='cuda')
    acc = torch.zeros(9, dtype=torch.float64, device='cuda')
    for order in (1, 2):
        good = _call(x, ft, None, 2.0, order, 1.0, acc)
        bad = x.clone()
        bad[7] = float('nan')
        out = _call(bad, ft, None, 2.0, order, 1.0, acc)
        assert all(torch.equal(a, b) for a, b in zip(good, out)) and float(out[2][7].abs().max()) == 0.0


def test_motion_penalty_checks_its_frame_numbers_on_the_host_unless_told_not_to():
    from fpc_diffrend_amd import fit
    x = _inputs(5, 4, 3).cuda()
    with pytest.raises(ValueError, match="strictly increasing"):
        fit.motion_penalty(x, 1.0, frame_ids=torch.tensor([0, 1, 1, 2], device='cuda'))
    with pytest.raises(ValueError, match="device of verts"):
        fit.motion_penalty(x, 1.0, frame_ids=torch.tensor([0, 1, 2, 3]))
    with pytest.raises(ValueError, match="finite and not negative"):
        fit.motion_penalty(x, 1.0, vertex_weights=torch.tensor([1, 1, -1, 1, 1.0], device='cuda'))
    # validate=False: no read-back; numbers that are not increasing only switch stencils off
    v = fit.motion_penalty(x, 1.0, frame_ids=torch.tensor([0, 1, 1, 2], device='cuda'), order=1, validate=False)
    ref = M.motion(x, 1.0, [0, 1, 1, 2], 1)['value'][0]
    assert abs(float(v) - float(ref)) <= 1e-5 * float(ref)


# ---------------------------------------------------------------------------------------------------------------------
# inside a Fitter
# ---------------------------------------------------------------------------------------------------------------------

# the weight at which the term's parameter gradient is of the size of the pixel term's at init_near_truth(0.8) on five frames of cfg1
# (asserted below: between a tenth and ten times)
W_MOT = 6.0e6
W_MOT_O1 = 2.0e7      # the same for order 1 with a Charbonnier scale of 0.02 and a quarter of the vertices switched off
W_GRAPH = 1.0e5       # the captured steps: a weight at which the term is several times the pixel term's value and the fit still converges
W_FREE, NOISE = 1.0e4, 0.02      # the behaviour test: the weight, and the size of the per-frame vertex noise it starts from


def _fitter(n_frames=5, rank=0, world=1, **kw):
    return fitter_near_truth(n_frames, rank, world, **{'optimize_texture': False, **kw})


_additive = functools.partial(additive, "MOTION")


@pytest.mark.parametrize("path", ['one_pass', 'torch'])
@pytest.mark.parametrize("order,scale,weights", [(2, None, False), (1, 0.02, True)])
def test_fitter_gradient_is_the_pixel_terms_plus_the_motion_term(path, order, scale, weights):
    """g_on - g_off = g_term to the project's float bar (1e-4 of the gradients' size) per parameter tensor, on the one-pass path and the
    torch chain; the term's gradient is of the pixel term's size, so a missing term cannot pass."""
    from fpc_diffrend_amd import fit
    kw = {'one_pass': dict(), 'torch': dict(fused_loss=False)}[path]
    vw = (np.arange(514) % 4 != 0).astype(np.float64) * 1.5 if weights else None
    wm = W_MOT if order == 2 else W_MOT_O1
    ft_on = _fitter(weight_motion=wm, motion_order=order, motion_scale=scale, motion_vertex_weights=vw, **kw)
    ft_off = _fitter(**kw)
    assert len(ft_on._reg_terms) == 1 and ft_off._reg_terms == [] and (ft_on._motion_w is not None) == weights
    vwc = ft_on._motion_w
    _additive(f"{path}/o{order}", ft_on, ft_off, slice(0, 5),
              lambda v: fit.motion_penalty(v, wm, order=order, scale=scale, vertex_weights=vwc))



@pytest.mark.parametrize("order", [1, 2])
def test_fitter_on_a_random_subset_gives_the_term_of_the_drawn_frame_numbers(order):
    """frames_per_step = 3 of five frames: the step hands the drawn, sorted frame numbers to the term, which couples only those that are
    adjacent in the take -- the same term as a direct call on those numbers, and not the term of three consecutive meshes."""
    from fpc_diffrend_amd import fit
    wm = W_MOT if order == 2 else W_MOT_O1
    ft_on, ft_off = _fitter(weight_motion=wm, motion_order=order, frames_per_step=3), _fitter(frames_per_step=3)
    want_gap = order == 1      # order 1: a draw with a gap and a valid stencil ([0,1,3]); order 2: three consecutive frames
    for _ in range(200):
        ids = ft_on.pick_frames()
        t = ids.tolist()
        if bool(M.stencil_flags(3, t, order).any()) and ((t[2] - t[0] > 2) == want_gap):
            break
    else:
        raise AssertionError("no usable draw")
    assert ids.dtype == torch.int64 and ids.is_cuda and t == sorted(t)
    l_term, _ = _additive(f"subset{t}/o{order}", ft_on, ft_off, ids, lambda v: fit.motion_penalty(v, wm, frame_ids=ids, order=order),
                          sized=False)
    assert l_term > 0.0
    if want_gap:
        v = ft_on.vertices(ids).detach().reshape(3, -1, 3)
        assert float(fit.motion_penalty(v, wm, order=order)) > 1.2 * l_term      # (consecutive: both steps count)


@pytest.mark.parametrize("mode,fps", [("prior", 0), ("combined", 3)])
def test_hip_graph_steps_equal_eager_steps_with_the_motion_term(mode, fps):
    """The configuration and tolerances of test_gpu_rest.test_hip_graph_steps_equal_eager_steps_with_the_rest_terms on five frames, with
    the motion term on: no host sync, no per-call fill, and the frame numbers of a random subset are read on the device from the step's
    fixed buffer, so it replays."""
    from fpc_diffrend_amd import fit, scene
    traj = {}
    for graph in (False, True):
        sc = scene.cfg('cfg1', n_frames=5)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=14, cam_idxs=(0, 3), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, mode=mode, frames_per_step=fps,
                            hip_graph=graph, weight_laplacian=20.0, weight_motion=W_GRAPH, motion_order=1 if fps else 2)
        ft = fit.Fitter(sc, cfg, device='cuda')
        if mode == "prior":
            ft.init_near_truth(0.8)
        traj[graph] = [float(ft.step()) for _ in range(14)]
        if graph:
            assert ft._graphs is not None
        assert bool((ft._reg_acc == 0).all())
    a, b = np.asarray(traj[False]), np.asarray(traj[True])
    print(f"MOTION graph/{mode} eager {a[:3]} .. {a[-1]:.6e} graphed {b[:3]} .. {b[-1]:.6e}")
    assert np.isfinite(b).all()
    assert np.allclose(a, b, rtol=2e-3), (a, b)
    assert np.allclose(a[:5], b[:5], rtol=1e-5), (a, b)


def test_second_of_two_ranks_takes_the_term_of_its_own_frames_times_a_half():
    """Fitter(rank=1, world=2) on six frames: the stencils end at the shard's borders -- the term of the frames 3..5 alone, its weight
    carrying the 1 / world."""
    from fpc_diffrend_amd import fit
    ft_on, ft_off = _fitter(6, 1, 2, weight_motion=W_MOT), _fitter(6, 1, 2)
    assert (ft_on.frame_lo, ft_on.frame_hi) == (3, 6)
    l_term, _ = _additive("rank1of2", ft_on, ft_off, slice(3, 6), lambda v: fit.motion_penalty(v, W_MOT / 2), sized=False)
    v = ft_on.vertices(slice(3, 6)).detach().reshape(3, -1, 3)
    ref = M.motion(v, W_MOT / 2, None, 2)['value'][0]
    assert l_term > 0.0 and abs(l_term - float(ref)) <= 1e-4 * float(ref)
    with pytest.raises(ValueError, match="shard"):                            # two frames a rank hold no stencil of order 2
        _fitter(4, 1, 2, weight_motion=W_MOT)
    with pytest.raises(ValueError, match="one number per vertex"):
        _fitter(weight_motion=W_MOT, motion_vertex_weights=[1.0] * 10)


def test_with_the_weight_at_zero_a_step_is_the_step_it_was():
    """weight_motion = 0 with every other option set: no term, no weights on the device, the launches of a Fitter built without the
    options, and its results.  What a step computes before its backward -- the vertices, the eager term, the loss -- is torch.equal.
    The parameters after a step are held torch.equal too WHEREVER THAT CAN HOLD: the pixel term's backward sums with float atomics, so
    two Fitters built from the very same options already differ in the last bits (the control pair below; on the MI355X its parameters
    are not torch.equal either).  The Fitter with the options at 0 is therefore held to the control pair's own distance: bit-equal if
    the controls are, else no further from the first control than 1e-5 of the parameter's size, the bar tests/test_gpu_dist.py sets for
    one process against two."""
    from fpc_diffrend_amd import _lib
    runs = []
    zero = dict(weight_motion=0.0, motion_order=1, motion_scale=0.5, motion_vertex_weights=np.ones(514))
    for kw in (dict(), dict(), zero):
        ft = _fitter(weight_laplacian=20.0, **kw)
        assert len(ft._reg_terms) == 1 and ft._motion_w is None
        v = ft.vertices(slice(0, 5)).detach().reshape(5, -1, 3).clone().requires_grad_(True)
        term = ft._reg_terms[0](v, None)
        term.backward()
        before = [v.detach(), term.detach().clone(), v.grad.clone()]
        _lib.TIMER = _lib.KernelTimer()
        try:
            losses = [torch.as_tensor(ft.step()).detach().clone() for _ in range(3)]
            calls = {k: n for k, (n, _) in _lib.TIMER.summary().items()}
        finally:
            _lib.TIMER = None
        assert "fpcdr_motion_penalty" not in calls
        runs.append((calls, before + losses[:1], losses[1:] + [p.detach().clone() for p in ft.params] + [ft.result.clone()]))
    (c0, d0, r0), (c1, d1, r1), (c2, d2, r2) = runs
    assert c0 == c1 == c2, (c0, c1, c2)                                      # the same launches
    assert all(torch.equal(a, b) for a, b in zip(d0, d2)) and all(torch.equal(a, b) for a, b in zip(d0, d1))
    control_equal = all(torch.equal(a, b) for a, b in zip(r0, r1))
    print(f"MOTION off: two Fitters without the options are torch.equal after three steps: {control_equal}; "
          f"with the options at 0: {all(torch.equal(a, b) for a, b in zip(r0, r2))}")
    for k, (a, b) in enumerate(zip(r0, r2)):
        if control_equal:
            assert torch.equal(a, b), k
        else:
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max())), (k, float((a - b).abs().max()))


def test_motion_term_lowers_the_rms_acceleration_of_a_free_fit():
    """mode='free' on six frames of cfg1 from the true per-frame offsets plus independent vertex noise (sigma = NOISE), thirty steps:
    the RMS acceleration of Fitter.result with the term on is below the one with it off (measured: 0.05750 against 0.07982, from 0.08561;
    the truth's is 0.00258).  Only the ordering is asserted."""
    from fpc_diffrend_amd import fit, scene
    F, steps = 6, 30
    rms = {}
    for wm in (0.0, W_FREE):
        sc = scene.cfg('cfg1', n_frames=F)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=steps, cam_idxs=(0, 3), mode='free', weight_laplacian=0.0, weight_motion=wm, optimize_texture=False)
        ft = fit.Fitter(sc, cfg, device='cuda')
        ft.init_near_truth(1.0)                                               # (the poses; the shape is m3's in this mode)
        truth = torch.tensor(sc.weights_gt) @ torch.tensor(sc.blendshapes).t()                     # [F,3V] offsets from the base mesh
        noise = NOISE * torch.randn(truth.shape, generator=torch.Generator().manual_seed(11))
        with torch.no_grad():
            ft.m3.copy_((truth + noise).t().to('cuda'))
        start = M.rms_acceleration(ft.vertices(slice(0, F)).detach().reshape(F, -1, 3))
        for _ in range(steps):
            ft.step()
        rms[wm] = M.rms_acceleration(ft.result.reshape(F, -1, 3))
        print(f"MOTION behaviour weight_motion={wm:g}: RMS acceleration start {start:.5f} after {steps} steps {rms[wm]:.5f} "
              f"(the truth: {M.rms_acceleration((truth + torch.tensor(sc.v_base)[None]).reshape(F, -1, 3)):.5f})")
    assert rms[W_FREE] < rms[0.0], rms

"""GPU: the landmark term (csrc/landmark.hip k_landmark_points, k_landmark_gather, the shared k_penalty_finish; fpcdr_landmark_penalty,
fit.landmark_penalty, FitConfig.weight_landmark / landmark_scale / landmark_iters / landmark_weights / use_landmarks) entry by entry
against float64 (tests/landmark_ref.py), and inside a Fitter: both loss paths, a random subset of frames with one view, the second of two
ranks, a pyramid level, a captured graph, the log, landmark_iters, landmark_residuals, and what the term is for.

The convention is tests/test_gpu_rest.py's and test_gpu_motion.py's: the error of an output x with float64 reference r is
e = max_i |x_i - r_i| / S_i in units of u = 2^-24, S_i the sum of the absolute values of the terms of entry i (every subtraction charges
the absolute values of its operands: positions sit at y + 170 under the matrices of helpers.scene_mvps, so m . q + m_3 cancels for
real, and u - u* is the difference of two numbers of several hundred pixels; the divisor p.w and the Charbonnier root carry their own
scale to first order, tests/landmark_ref.py); entries with S_i = 0 have no term, must be exactly 0, and their number must be the one the
tables predict.  The bar is e <= 8 * e32 + 4, e32 the error of float32 torch on the CPU for the same expression against the same
reference; beside it the rel-L2 of the same outputs against float64 is held to the project's 1e-4.  Every line is printed as
"LANDMARK case name e_gpu e32 bound" (pytest -s).

Shapes: L in {1, 63, 64, 65, 130} (one lane, the wave's edge, two waves and a lane), Nc in {1, 2, 9}, F in {1, 3}, V in {3, 255, 257,
514} (the gather's workgroup edge; cfg1's mesh), all 120 combinations, each with two of the four variants (with / without landmark
weights, a third of them 0; with / without a Charbonnier scale, the median residual, so both regimes occur) so that every shape sees
both values of both.  The raster is 72 x 96 -- not square, so a swapped pair shows.  A third of the confidences are 0, with NaN for
their positions; two landmarks in three are vertices, pairs of them the same vertex, one in three a point of a face; every seventh
landmark's vertex lies behind image 0.  An image's detections sit 15 px off as a whole plus 5 px of noise each, as those of a misplaced
head do: with residuals of a few pixels on positions of several hundred, float32 itself (torch on the CPU) is at 2e-5 rel-L2.

Measured on an MI355X (units of u; the largest over the 240 cases; the last column is the case that came closest to its own bound).
e_gpu equals e32 to the digits shown: the kernel evaluates the float32 statement's own expression in its order (the library is built
without contraction), and only the sums over the workgroup and over the images are ordered differently.  The per and value rows are
small because their scales carry the squares of positions of several hundred pixels; the rel-L2 of the same outputs against float64,
printed beside them, is at most 6.9e-6 (per), 6.9e-6 (value), 4.7e-6 (residuals), 5.3e-6 (grad_x) and 1.8e-5 (grad_mvp) over all cases,
against the bar of 1e-4.  The whole file runs in 8.4 s there:

  output                 cases max e_gpu  max e32   closest to its bound (e_gpu / bound, case)
  per                      240      0.03     0.03   0.034 / 4.3   F3/Nc2/V514/L1/w
  value                    240      0.03     0.03   0.026 / 4.2   F1/Nc1/V514/L1/c
  res                      240      1.53     1.53   1.529 / 16.2  F3/Nc9/V257/L130
  grad_x                   240      1.29     1.29   1.294 / 14.4  F1/Nc1/V514/L130/w
  grad_mvp                 240      1.03     1.03   1.033 / 12.3  F3/Nc9/V514/L1/w
  grad_q (the scratch)     240      1.38     1.38   1.378 / 15.0  F1/Nc9/V257/L130

Fitter (cfg1's mesh at 128 x 128, cameras 0 and 3, four frames, init_near_truth(0.8), 40 landmarks on every thirteenth vertex from
fit.project_landmarks at the truth; W_LMK = 30 is the weight at which the term's parameter gradient has the size of the pixel term's,
1.33e4 against 1.07e4, measured here.  "alone" is the term's own gradient in units of the bar, 1e-4 (|g_on| + |g_off|), of the tensor it
weighs most in; "worst" the largest |(g_on - g_off) - g_term| over the parameter tensors in units of its bar):
  case                      |g_on|     |g_off|    |g_term|   worst     alone     l_on      l_off     l_term
  one_pass                  2.3271e4   1.0743e4   1.3250e4   8.4e-4    4.3e3     6.90937   4.61409   2.29528
  torch                     2.3271e4   1.0743e4   1.3250e4   9.3e-4    4.3e3     6.90937   4.61409   2.29528
  one_pass, c = 2           2.3138e4   1.0743e4   1.3106e4   6.2e-4    4.2e3     6.89578   4.61409   2.28169
  torch, c = 2              2.3138e4   1.0743e4   1.3106e4   8.9e-4    4.2e3     6.89578   4.61409   2.28169
  subset [2,3,4] x view 0   3.4013e4   1.4662e4   1.9403e4   7.3e-4    4.0e3     9.56465   6.05202   3.51263
  rank 1 of 2               1.5441e4   5.7656e3   9.7231e3   8.3e-4    6.7e3     6.52345   3.97082   2.55263
  pyramid level 2           1.4472e4   1.2570e3   1.3250e4   1.3e-3    9.2e3     6.16855   3.87327   2.29528
At the pyramid level the term's value is the full-size Fitter's to every digit printed (2.295282).  Captured steps (W_GRAPH = 3,
landmark_scale = 3, fourteen steps): eager and graphed losses agree to every digit printed, 5.76806974 .. 2.723817 (prior, the whole
shard) and 42.72597885 .. 26.91824 (combined, three random frames of five and one random view a step).  landmark_iters = 6: eager and
graphed losses 6.90936852 5.22450972 3.79056692 2.63325167 1.87551177 1.62302923 | 1.14071965 1.00853097, equal to every digit.
landmark_residuals at init_near_truth(0.8): mean |residual| 0.266 px (four frames x two views), e_gpu = e32 = 0.60 against a bound of
8.8.  Behaviour (every frame 7 units off along x, lr_t = 0.1, forty steps): the mean live |residual| starts at 24.31 px and ends at
23.24 px with the term off, at 12.74 px with it on.  Only the ordering is asserted.
"""
import contextlib
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import fitstep_ref as R
import landmark_cases as LC
import landmark_ref as LR
from helpers import additive, fitter_grads, fitter_near_truth

pytestmark = pytest.mark.gpu

SHAPES_L, SHAPES_V = (1, 63, 64, 65, 130), (3, 255, 257, 514)
WORST = {}


def _report(case, name, e, e32, bound):
    print(f"LANDMARK {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={bound:.1f}")
    w = WORST.setdefault(name, [0, 0.0, 0.0])
    w[0], w[1], w[2] = w[0] + 1, max(w[1], e), max(w[2], e32)


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


def _call(d, inv_c, weight, acc, grad=True, res=True, scratch=None):
    """fpcdr_landmark_penalty on the device tensors d into buffers prefilled with NaN -> (per, value, grad_x, grad_mvp, res, scratch)."""
    from fpc_diffrend_amd import _lib
    x, mvp, obs = d['x'], d['mvp'], d['obs']
    F, V, _ = x.shape
    N, L, K = mvp.shape[0], obs.shape[1], d['inc'].shape[0]
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device='cuda')
    gx, gm = (nan(F, V, 3), nan(N, 4, 4)) if grad else (None, None)
    if grad and scratch is None:
        scratch = nan(N * L * 3)
    r = nan(N, L, 2) if res else None
    per, val = nan(F), nan()
    _lib.call("fpcdr_landmark_penalty", _ptr(x), _ptr(mvp), _ptr(d['vtx']), _ptr(d['bary']), _ptr(d['w']), _ptr(d['inc']), _ptr(obs), float(inv_c),
              LC.W, LC.H, _ptr(scratch) if grad else None, _ptr(gx), _ptr(gm), _ptr(r), _ptr(acc), _ptr(per), _ptr(val), float(weight), F, N // F, V,
              L, K, _stream())
    assert bool((acc == 0).all())                          # the call leaves its accumulators zeroed
    return per, val, gx, gm, r, scratch


def _res_pair(t, live):
    """Residuals with the entries that are not live set to 0 (they are NaN on both sides; their scale is 0)."""
    return torch.where(live[..., None], t.detach().cpu().double(), torch.zeros((), dtype=torch.float64))


def _case(F, Nc, V, L, use_w, use_c, module=False):
    from fpc_diffrend_amd import fit
    case = f"F{F}/Nc{Nc}/V{V}/L{L}" + ('/w' if use_w else '') + ('/c' if use_c else '')
    cs = LC.case(F, Nc, V, L, 0, use_w, use_c)
    weight, upstream = 7.5, 0.3
    inv_c = fit.landmark_inv_scale(cs['scale'])
    a = (cs['x'], cs['mvp'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], weight, LC.H, LC.W, inv_c)
    ref, ref32 = LR.landmark(*a), LR.landmark(*a, dtype=torch.float32)
    z, live = ref['zeros'], ref['live']
    assert torch.equal(ref32['live'], live)                # (nothing sits at the threshold)
    lms = fit.LandmarkSet(cs['points'], V, cs['faces'], 'cuda')
    assert np.array_equal(lms.vtx.cpu().numpy(), cs['vtx']) and np.array_equal(lms.inc.cpu().numpy(), LR.incidence(cs['vtx'], cs['bary'], V))
    d = dict(x=cs['x'].cuda(), mvp=cs['mvp'].cuda(), obs=cs['obs'].cuda(), vtx=lms.vtx, bary=lms.bary, inc=lms.inc,
             w=None if cs['w'] is None else cs['w'].cuda())
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    vref = tuple(t.reshape(1) for t in ref['value'])

    # (i) the entry into buffers prefilled with NaN: every entry is written; twice on one acc: bit-identical
    per, val, gx, gm, res, gq = _call(d, inv_c, weight, acc)
    assert all(bool(torch.isfinite(t).all()) for t in (per, val, gx, gm, gq))
    assert torch.equal(torch.isnan(res).cpu(), ~live[..., None].expand(-1, -1, 2))          # NaN exactly where the entry is not live
    long_sum(case, 'per', per, ref['per'], ref32['per'][0], z['per'])
    long_sum(case, 'value', val.reshape(1), vref, ref32['value'][0].reshape(1), 1 if z['per'] == F else 0)
    long_sum(case, 'res', _res_pair(res, live), (_res_pair(ref['res'][0], live), ref['res'][1]), _res_pair(ref32['res'][0], live), z['res'])
    long_sum(case, 'grad_x', gx, ref['grad_x'], ref32['grad_x'][0], z['grad_x'])
    long_sum(case, 'grad_mvp', gm, ref['grad_mvp'], ref32['grad_mvp'][0], z['grad_mvp'])
    long_sum(case, 'grad_q', gq.reshape(F * Nc, L, 3), ref['grad_q'], ref32['grad_q'][0], 3 * int((~live).sum()))
    if bool(live.any()):
        rl2 = [R.rel_l2(per, ref['per'][0]), R.rel_l2(val, ref['value'][0]), R.rel_l2(_res_pair(res, live), _res_pair(ref['res'][0], live)),
               R.rel_l2(gx, ref['grad_x'][0]), R.rel_l2(gm, ref['grad_mvp'][0])]
        print(f"LANDMARK {case} rel-L2 per={rl2[0]:.2e} value={rl2[1]:.2e} res={rl2[2]:.2e} grad_x={rl2[3]:.2e} grad_mvp={rl2[4]:.2e}")
        assert max(rl2) <= 1e-4, (case, rl2)
    else:
        assert float(val) == 0.0 and float(per.abs().max()) == 0.0 and float(gx.abs().max()) == 0.0 and float(gm.abs().max()) == 0.0
    again = _call(d, inv_c, weight, acc)
    assert all(torch.equal(torch.nan_to_num(p), torch.nan_to_num(q)) for p, q in zip(again, (per, val, gx, gm, res, gq))), case
    per3, val3, _, _, res3, _ = _call(d, inv_c, weight, acc, grad=False)                    # the value-only call
    assert torch.equal(per3, per) and torch.equal(val3, val) and torch.equal(torch.nan_to_num(res3), torch.nan_to_num(res)), case
    per4, val4, _, _, none, _ = _call(d, inv_c, weight, acc, grad=False, res=False)
    assert none is None and torch.equal(per4, per) and torch.equal(val4, val), case
    if not module:
        return
    # (ii) fit.landmark_penalty: lazy, eager with a unit upstream, eager with a factor, on the caller's acc, scratch and residuals
    own_scratch, own_res = torch.full_like(gq, float('nan')), torch.full_like(res, float('nan'))
    for kw, upv in ((dict(), upstream), (dict(eager_grad=True, unit_upstream=True), 1.0), (dict(eager_grad=True), upstream),
                    (dict(acc=acc, scratch=own_scratch, residuals=own_res), upstream)):
        lx, lm = d['x'].clone().requires_grad_(True), d['mvp'].clone().requires_grad_(True)
        value = fit.landmark_penalty(lx, lm, lms if cs['w'] is None else lms.with_weights(cs['w'].numpy()), d['obs'], weight, (LC.H, LC.W),
                                     scale=cs['scale'], **kw)
        (value * upv).backward() if upv != 1.0 else value.backward()
        assert torch.equal(value.detach(), val), (case, kw)                  # the same call
        up = torch.tensor(upv, dtype=torch.float32, device='cuda')
        assert torch.equal(lx.grad, gx if upv == 1.0 else gx * up) and torch.equal(lm.grad, gm if upv == 1.0 else gm * up), (case, kw)
        assert bool((acc == 0).all())
    assert torch.equal(own_scratch, gq) and torch.equal(torch.nan_to_num(own_res), torch.nan_to_num(res))      # the caller's buffers are the ones used
    lx = d['x'].clone().requires_grad_(True)                                  # one input alone
    fit.landmark_penalty(lx, d['mvp'], lms if cs['w'] is None else lms.with_weights(cs['w'].numpy()), d['obs'], weight, (LC.H, LC.W),
                         scale=cs['scale']).backward()
    assert torch.equal(lx.grad, gx)
    with torch.no_grad():                                                    # no gradient asked for: value only
        assert torch.equal(fit.landmark_penalty(d['x'], d['mvp'], lms if cs['w'] is None else lms.with_weights(cs['w'].numpy()), d['obs'],
                                                weight, (LC.H, LC.W), scale=cs['scale']), val)


@pytest.mark.parametrize("F,Nc", [(1, 1), (1, 2), (1, 9), (3, 1), (3, 2), (3, 9)])
def test_landmark_entries_against_float64(F, Nc):
    k = 0
    for V in SHAPES_V:
        for L in SHAPES_L:
            for use_w, use_c in (((False, False), (True, True)) if k % 2 == 0 else ((True, False), (False, True))):
                _case(F, Nc, V, L, use_w, use_c, module=(L == 65))
            k += 1
    print("LANDMARK maxima so far  " + "  ".join(f"{n}: {c} cases e_gpu {e:.2f} e32 {e32:.2f}" for n, (c, e, e32) in WORST.items()))


def test_a_nan_in_what_nobody_observed_and_a_point_behind_the_camera_change_nothing():
    """The flags are selects: garbage in a dead entry's position, and a live-looking entry whose point is behind the camera, leave every
    output as it is with the entry taken out by its confidence."""
    from fpc_diffrend_amd import fit
    cs = LC.case(3, 2, 257, 65, 0, False, True)
    lms = fit.LandmarkSet(cs['points'], 257, cs['faces'], 'cuda')
    d = dict(x=cs['x'].cuda(), mvp=cs['mvp'].cuda(), obs=cs['obs'].cuda(), vtx=lms.vtx, bary=lms.bary, inc=lms.inc, w=None)
    acc = torch.zeros(4, dtype=torch.float64, device='cuda')
    inv_c = fit.landmark_inv_scale(cs['scale'])
    good = _call(d, inv_c, 2.0, acc)
    dead = d['obs'][..., 2] == 0
    for junk in (float('inf'), 1e30, 0.0):
        o = d['obs'].clone()
        o[..., 0][dead], o[..., 1][dead] = junk, -junk
        out = _call(dict(d, obs=o), inv_c, 2.0, acc)
        assert all(torch.equal(torch.nan_to_num(p), torch.nan_to_num(q)) for p, q in zip(good, out)), junk
    behind = torch.isnan(good[4][..., 0]) & ~dead                            # observed, but not live: the point is behind its camera
    assert int(behind.sum()) > 0
    o = d['obs'].clone()
    o[..., 2][behind] = 0.0
    out = _call(dict(d, obs=o), inv_c, 2.0, acc)
    assert all(torch.equal(torch.nan_to_num(p), torch.nan_to_num(q)) for p, q in zip(good, out))


# ---------------------------------------------------------------------------------------------------------------------
# inside a Fitter
# ---------------------------------------------------------------------------------------------------------------------

# The weight at which the term's parameter gradient is of the size of the pixel term's at init_near_truth(0.8) on four frames of cfg1's
# mesh at 128 x 128 (measured on the MI355X, the module's docstring: 1.33e4 against 1.07e4)
W_LMK = 30.0
W_GRAPH = 3.0        # the captured steps: a weight at which the fit still converges
RES = (128, 128)
N_LMK = 40


@contextlib.contextmanager
def _landmark_scenes(landmarks=True):
    """While it is open scene.cfg('cfg1', n) gives cfg1's scene at 128 x 128 with the poses at identity and, asked for, N_LMK landmarks
    from fit.project_landmarks at its truth: what helpers.fitter_near_truth builds its Fitter on."""
    from fpc_diffrend_amd import fit, scene
    orig = scene.cfg

    def cfg(name, n_frames=None, seed=0):
        assert name == 'cfg1'
        sc = scene.make_scene(scene.MESH_1K, 10, n_frames or 4, RES, (256, 256, 1), seed)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        if landmarks:
            sc.landmark_points = [{'vertex': v} for v in range(0, sc.n_vertices, 13)]
            assert len(sc.landmark_points) == N_LMK
            sc.landmarks = fit.project_landmarks(sc, sc.landmark_points).astype(np.float32)
        return sc

    scene.cfg = cfg
    try:
        yield
    finally:
        scene.cfg = orig


def _fitter(n_frames=4, rank=0, world=1, landmarks=True, **kw):
    with _landmark_scenes(landmarks):
        return fitter_near_truth(n_frames, rank, world, **{'optimize_texture': False, **kw})


def _direct(ft, weight, frames, view_ids=None, **kw):
    """The term of ft's current parameters by a direct call of fit.landmark_penalty on its vertices v (helpers.additive's term_of)."""
    from fpc_diffrend_amd import fit

    def term_of(v):
        obs = ft._take(ft._lmk_obs, 0, ft._target_rows(frames, view_ids))
        return fit.landmark_penalty(v, ft.mvp(frames, view_ids), ft._lmk, obs, weight, ft.full_resolution, scale=ft.cfg.landmark_scale, **kw)
    return term_of


def _alone_ratio(tag, ft_on, g_on, g_off):
    """additive() left the term's own gradient in ft_on: on some parameter tensor it is at least ten times that tensor's bar."""
    ratio = max(float(g.norm()) / (1e-4 * (float(a.norm()) + float(o.norm()))) for g, a, o in zip(fitter_grads(ft_on), g_on, g_off) if float(o.norm()) > 0)
    print(f"LANDMARK fitter/{tag} the term alone is {ratio:.3e} x the bar of the tensor it weighs most in")
    assert ratio >= 10.0, (tag, ratio)


def _additive(tag, ft_on, ft_off, frames, term_of):
    ft_on.loss_and_backward(frames)
    ft_off.loss_and_backward(frames)
    g_on, g_off = fitter_grads(ft_on), fitter_grads(ft_off)
    out = additive("LANDMARK", tag, ft_on, ft_off, frames, term_of, sized=False)
    _alone_ratio(tag, ft_on, g_on, g_off)
    return out


@pytest.mark.parametrize("path", ['one_pass', 'torch'])
@pytest.mark.parametrize("scale", [None, 2.0])
def test_fitter_gradient_is_the_pixel_terms_plus_the_landmark_term(path, scale):
    """g_on - g_off = g_term to the project's float bar (1e-4 of the gradients' size) per parameter tensor, on the one-pass path and the
    torch chain; the term alone is at least ten times the bar of some tensor, so a missing term cannot pass."""
    kw = {'one_pass': dict(), 'torch': dict(fused_loss=False)}[path]
    ft_on, ft_off = _fitter(weight_landmark=W_LMK, landmark_scale=scale, **kw), _fitter(**kw)
    assert ft_on._lmk is not None and ft_on._lmk.n == N_LMK and ft_off._lmk is None and len(ft_on._reg_terms) == len(ft_off._reg_terms) == 0
    assert tuple(ft_on._lmk_obs.shape) == (4 * 2, N_LMK, 3)
    l_term, _ = _additive(f"{path}/c{scale}", ft_on, ft_off, slice(0, 4), _direct(ft_on, W_LMK, slice(0, 4)))
    assert l_term > 0.0


def test_fitter_on_a_random_frame_subset_with_one_view():
    """frames_per_step = 3 of five frames and views_per_step = 1: the step hands the term the rows of the drawn (frame, view) images."""
    ft_on, ft_off = _fitter(5, weight_landmark=W_LMK, frames_per_step=3, views_per_step=1), _fitter(5, frames_per_step=3, views_per_step=1)
    ids, views = ft_on.pick_frames(), ft_on.pick_views()
    assert ids.is_cuda and tuple(ids.shape) == (3,) and tuple(views.shape) == (1,)
    for ft in (ft_on, ft_off):      # (helpers.additive names the frames only: the views ride along)
        ft.loss_and_backward = functools.partial(ft.loss_and_backward, view_ids=views)
    l_term, _ = _additive(f"subset{ids.tolist()}x{views.tolist()}", ft_on, ft_off, ids, _direct(ft_on, W_LMK, ids, views))
    assert l_term > 0.0
    other = (views + 1) % 2                                                    # ... and not the other camera's
    v = ft_on.vertices(ids).detach().reshape(3, -1, 3)
    assert abs(float(_direct(ft_on, W_LMK, ids, other)(v)) - l_term) > 1e-3 * l_term


def test_second_of_two_ranks_takes_the_term_of_its_own_frames_times_a_half():
    ft_on, ft_off = _fitter(6, 1, 2, weight_landmark=W_LMK), _fitter(6, 1, 2)
    assert (ft_on.frame_lo, ft_on.frame_hi) == (3, 6) and tuple(ft_on._lmk_obs.shape) == (3 * 2, N_LMK, 3)
    l_term, _ = _additive("rank1of2", ft_on, ft_off, slice(3, 6), _direct(ft_on, W_LMK / 2, slice(3, 6)))
    v, mvp = ft_on.vertices(slice(3, 6)).detach().reshape(3, -1, 3), ft_on.mvp(slice(3, 6)).detach()
    lm = ft_on._lmk
    ref = LR.landmark(v, mvp, lm.vtx.cpu().numpy(), lm.bary.cpu().numpy(), None, ft_on._lmk_obs, W_LMK / 2, *RES, grads=False)['value'][0]
    assert l_term > 0.0 and abs(l_term - float(ref)) <= 1e-4 * float(ref)


def test_at_a_pyramid_level_the_term_is_the_full_size_term():
    """pyramid=((2, 5),): iteration 0 renders at 64 x 64, and the landmark term is the one of the 128 x 128 captures -- the same value as
    a Fitter without the pyramid has, to 1e-6 relative."""
    ft_p, ft_p_off = _fitter(weight_landmark=W_LMK, pyramid=((2, 5),)), _fitter(pyramid=((2, 5),))
    ft_f = _fitter(weight_landmark=W_LMK)
    l_term, _ = _additive("pyramid/2", ft_p, ft_p_off, slice(0, 4), _direct(ft_p, W_LMK, slice(0, 4)))
    assert ft_p.resolution == (64, 64) and ft_p.full_resolution == RES
    v = ft_f.vertices(slice(0, 4)).detach().reshape(4, -1, 3)
    full = float(_direct(ft_f, W_LMK, slice(0, 4))(v))
    assert ft_f.resolution == RES and abs(l_term - full) <= 1e-6 * full, (l_term, full)


@pytest.mark.parametrize("mode,fps,vps", [("prior", 0, 0), ("combined", 3, 1)])
def test_hip_graph_steps_equal_eager_steps_with_the_landmark_term(mode, fps, vps):
    """The configuration and tolerances of test_gpu_rest.test_hip_graph_steps_equal_eager_steps_with_the_rest_terms on five frames, with
    the landmark term on: no host sync, no per-call fill, and the rows of a random subset come from one index_select on the step's fixed
    index buffers, so it replays."""
    from fpc_diffrend_amd import fit, scene
    traj = {}
    for graph in (False, True):
        with _landmark_scenes():
            sc = scene.cfg('cfg1', n_frames=5)
        cfg = fit.FitConfig(max_iter=14, cam_idxs=(0, 3), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, mode=mode, frames_per_step=fps, views_per_step=vps,
                            hip_graph=graph, weight_laplacian=20.0, weight_landmark=W_GRAPH, landmark_scale=3.0)
        ft = fit.Fitter(sc, cfg, device='cuda')
        if mode == "prior":
            ft.init_near_truth(0.8)
        traj[graph] = [float(ft.step()) for _ in range(14)]
        if graph:
            assert ft._graphs is not None
        assert bool((ft._reg_acc == 0).all())
    a, b = np.asarray(traj[False]), np.asarray(traj[True])
    print(f"LANDMARK graph/{mode} eager {a[:3]} .. {a[-1]:.6e} graphed {b[:3]} .. {b[-1]:.6e}")
    assert np.isfinite(b).all()
    assert np.allclose(a, b, rtol=2e-3), (a, b)
    assert np.allclose(a[:5], b[:5], rtol=1e-5), (a, b)


def _logged(ft, path, steps=1):
    from fpc_diffrend_amd import _lib
    _lib.TIMER = _lib.KernelTimer()
    try:
        for _ in range(steps):
            ft.step()
        calls = {k: n for k, (n, _) in _lib.TIMER.summary().items()}
    finally:
        _lib.TIMER = None
    return calls, [json.loads(line) for line in open(path)]


def test_off_there_is_no_launch_and_the_log_is_the_old_one_and_on_lmk_is_the_direct_call(tmp_path):
    keys, n = {}, 0
    for name, kw, lm in (('none', dict(), False), ('zero', dict(weight_landmark=0.0, landmark_scale=2.0, landmark_iters=3), True),
                         ('unused', dict(weight_landmark=W_LMK, use_landmarks=False), True), ('on', dict(weight_landmark=W_LMK), True)):
        path = str(tmp_path / f"{name}.jsonl")
        ft = _fitter(landmarks=lm, weight_laplacian=20.0, log_interval=1, reg_log_interval=1, log_path=path, **kw)
        calls, recs = _logged(ft, path)
        keys[name] = set(recs[0])
        if name == 'on':
            assert calls.get("fpcdr_landmark_penalty") == 2                    # the step's and the log's
            v = ft.vertices(slice(0, 4)).detach().reshape(4, -1, 3)            # (the log is written after the update)
            want = float(_direct(ft, W_LMK, slice(0, 4))(v))
            assert abs(recs[0]["LMK"] - want) <= 1e-6 * want, (recs[0]["LMK"], want)
        else:
            assert "fpcdr_landmark_penalty" not in calls and ft._lmk is None and ft._lmk_obs is None and ft._lmk_scratch is None, name
        assert bool((ft._reg_acc == 0).all())
    assert keys['none'] == keys['zero'] == keys['unused'] and keys['on'] == keys['none'] | {"LMK"}
    with _landmark_scenes(False), pytest.raises(ValueError, match="Scene with landmarks"):
        fitter_near_truth(4, weight_landmark=1.0)
    with pytest.raises(ValueError, match="one number per landmark"):
        _fitter(weight_landmark=1.0, landmark_weights=[1.0, 2.0])
    ft = _fitter(weight_landmark=1.0, landmark_weights=np.arange(N_LMK) % 2)
    assert ft._lmk.w.tolist() == [float(i % 2) for i in range(N_LMK)]


def test_landmark_iters_switches_the_term_off(tmp_path):
    """landmark_iters = 6: the iterations 0 .. 5 run the term, iteration 6 and 7 do not -- eager by the count of the entry's calls, under a
    captured graph (which is captured anew) by the losses of the eager run, to the tolerance of the captured-steps test: the term is more
    than a fiftieth of the loss, so a graph that kept it would miss."""
    n, losses = 6, {}
    for graph in (False, True):
        path = str(tmp_path / f"iters{graph}.jsonl")
        ft = _fitter(weight_landmark=W_LMK, landmark_iters=n, hip_graph=graph, log_interval=1, reg_log_interval=1, log_path=path)
        assert [ft.landmark_on(i) for i in (0, n - 1, n, n + 1)] == [True, True, False, False]
        if graph:      # (no per-call timing inside a graph)
            for _ in range(n + 2):
                ft.step()
            recs = [json.loads(line) for line in open(path)]
        else:
            for i in range(n + 2):
                calls, recs = _logged(ft, path)
                assert calls.get("fpcdr_landmark_penalty", 0) == (2 if i < n else 0), (i, calls)
        assert ["LMK" in r for r in recs] == [True] * n + [False] * 2
        assert recs[n - 1]["LMK"] > 0.02 * recs[n - 1]["loss"]
        losses[graph] = np.asarray([r["loss"] for r in recs])
    print(f"LANDMARK iters eager {losses[False]} graphed {losses[True]}")
    assert np.allclose(losses[False], losses[True], rtol=2e-3), losses


def test_landmark_residuals_against_the_float64_statement():
    ft = _fitter(weight_landmark=W_LMK)
    lm = ft._lmk
    for frames, views in ((None, None), (torch.tensor([2, 0]), torch.tensor([1]))):
        res = ft.landmark_residuals(frames, views)
        fr = slice(0, 4) if frames is None else frames.cuda()
        vw = None if views is None else views.cuda()
        Fb, Nc = (4, 2) if frames is None else (2, 1)
        assert tuple(res.shape) == (Fb, Nc, N_LMK, 2) and not res.requires_grad
        v, mvp = ft.vertices(fr).detach().reshape(Fb, -1, 3), ft.mvp(fr, vw).detach()
        obs = ft._take(ft._lmk_obs, 0, ft._target_rows(fr, vw))
        a = (v, mvp, lm.vtx.cpu().numpy(), lm.bary.cpu().numpy(), None, obs, 1.0, *RES)
        ref, ref32 = LR.landmark(*a, grads=False), LR.landmark(*a, dtype=torch.float32, grads=False)
        live = ref['live']
        assert bool(live.all()) and not bool(torch.isnan(res).any())
        long_sum(f"residuals/{Fb}x{Nc}", 'res', res.reshape(Fb * Nc, N_LMK, 2), ref['res'], ref32['res'][0], 0)
        print(f"LANDMARK residuals/{Fb}x{Nc} mean |residual| {LR.mean_live_residual(res):.4f} px")
    assert bool((ft._reg_acc == 0).all())
    with pytest.raises(ValueError, match="weight_landmark"):
        _fitter().landmark_residuals()


def test_landmark_term_brings_a_misplaced_head_home():
    """Every frame's translation 7 units off along x, so the render sits about 25 px from the captures (3.494 px a unit at 128 x 128), forty
    steps with lr_t = 0.1: the mean live |residual| ends lower with the term on than with it off, and lower than it began.  Only the
    ordering is asserted; the numbers measured on the MI355X are in the module's docstring."""
    end = {}
    for w in (0.0, W_LMK):
        ft = _fitter(weight_landmark=w, lr_t=0.1) if w else _fitter(lr_t=0.1)
        with torch.no_grad():
            ft.per_frame_t[:, 0] += 7.0
        probe = ft if w else None
        if probe is None:      # (the residuals of the Fitter without the term: through one with the term, on the same parameters)
            probe = _fitter(weight_landmark=W_LMK, lr_t=0.1)

        def residual():
            if probe is not ft:
                with torch.no_grad():
                    for p, q in zip(probe.params, ft.params):
                        p.copy_(q)
            return LR.mean_live_residual(probe.landmark_residuals())

        start = residual()
        for _ in range(40):
            ft.step()
        end[w] = residual()
        print(f"LANDMARK behaviour weight_landmark={w:g}: mean live |residual| start {start:.3f} px after 40 steps {end[w]:.3f} px")
    assert end[W_LMK] < end[0.0] and end[W_LMK] < start, (end, start)

"""GPU: the table of the step's prior terms (Fitter._reg_terms: rest Laplacian, stretch, bend, motion, texture prior) with all five on
together, at the smallest shape that holds them: four frames of cfg1, cameras (0, 3), 128 x 128, the weights of the four files that test
the terms one by one.

  (a) the table has five entries in the order above: each, called as (vtx, ids), gives the public function's value on the same input
  (b) g_on - g_off per parameter tensor = the gradients of the five public functions, on the one-pass path and on fused_loss=False
  (c) the same for Fitter(rank=1, world=2) on six frames, every weight halved in the direct calls
  (d) the log record of iteration 0: its key set, and STR BND MOT TEXS TEXA against the public functions at the full weight
  (e) the shared accumulator is all zero after a step and after the log

Bars.  (b), (c): helpers.additive's, 1e-4 (|g_on| + |g_off|) per tensor and 1e-4 on the values; a term left out would miss it: each of
the five alone holds, on some parameter tensor, at least ten times that tensor's bar (asserted).  (a), (d): 1e-6 relative -- the same
kernel on the same input, where only the order of the float64 atomic adds can differ, at most one float32 ulp (6e-8) after the final
rounding; a texture part is logged as weight * part with the weight a double where the direct call rounds the weight to float32 first
and the product once more: two further roundings of 6e-8 each."""
import json

import pytest
import torch

from helpers import additive, fitter_grads, fitter_near_truth
from test_gpu_bend import W_BND
from test_gpu_motion import W_MOT
from test_gpu_rest import W_LAP, W_STR
from test_gpu_tex_prior import SCALE, W_A, W_S, _anchor_of

pytestmark = pytest.mark.gpu

ALL_ON = dict(laplacian_relative=True, weight_laplacian=W_LAP, weight_stretch=W_STR, weight_bend=W_BND, weight_motion=W_MOT, motion_order=2,
              weight_tex_smooth=W_S, tex_smooth_scale=SCALE, tex_smooth_weights='chart', weight_tex_anchor=W_A)
NAMES = ['laplacian', 'stretch', 'bend', 'motion', 'texture']


def _fitter(n_frames=4, rank=0, world=1, on=True, **kw):
    ft = fitter_near_truth(n_frames, rank, world, **{'resolution': (128, 128), **(ALL_ON if on else {}), **kw})
    if on:      # (an anchor that differs from the start texture: at the start itself the hold and its gradient are 0)
        ft.set_texture_anchor(*_anchor_of(ft))
    return ft


def _direct(ft, share=1.0):
    """The five public functions on ft's tables at share * the configured weights: name -> (v -> scalar)."""
    from fpc_diffrend_amd import fit
    s = share
    tex = dict(smooth_weights=ft._tex_smooth_w, scale=SCALE), dict(anchor=ft._tex_anchor, anchor_weights=ft._tex_anchor_w)
    return {'laplacian': lambda v: fit.laplacian_penalty(v, ft.topo, W_LAP * s, rest=ft.rest),
            'stretch': lambda v: fit.stretch_penalty(v, ft.topo, W_STR * s, rest=ft.rest),
            'bend': lambda v: fit.bend_penalty(v, ft.topo, W_BND * s, rest=ft.rest),
            'motion': lambda v: fit.motion_penalty(v, W_MOT * s, order=2),
            'texture': lambda v: fit.texture_prior(ft.tex_opt, W_S * s, W_A * s, **tex[0], **tex[1]),
            'TEXS': lambda v: fit.texture_prior(ft.tex_opt, W_S * s, 0.0, **tex[0]),
            'TEXA': lambda v: fit.texture_prior(ft.tex_opt, 0.0, W_A * s, **tex[1])}


def _close(got, want, what):
    print(f"PRIORS {what}: {got:.9e} against {want:.9e}")
    assert want > 0.0 and abs(got - want) <= 1e-6 * want, (what, got, want)


def _check_additive(tag, ft_on, ft_off, frames, share=1.0):
    direct = _direct(ft_on, share)
    additive("PRIORS", tag, ft_on, ft_off, frames, lambda v: sum(direct[name](v) for name in NAMES), sized=False)
    g_off, g_sum = fitter_grads(ft_off), fitter_grads(ft_on)      # (ft_on holds the gradient of the five direct calls now)
    Fb = ft_on._n(frames)
    for name in NAMES:      # a term left out could not pass: alone it is ten times the bar of some tensor
        ft_on.optimizer.zero_grad(set_to_none=True)
        direct[name](ft_on.vertices(frames).reshape(Fb, -1, 3)).backward()
        ratio = max(float(g.norm()) / (1e-4 * (float((o + t).norm()) + float(o.norm())))
                    for g, o, t in zip(fitter_grads(ft_on), g_off, g_sum) if float(o.norm()) > 0)
        print(f"PRIORS fitter/{tag} {name} alone is {ratio:.3e} x the bar of the tensor it weighs most in")
        assert ratio >= 10.0, (tag, name, ratio)


@pytest.fixture(scope="module")
def ft_all(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("priors") / "log.jsonl")
    return _fitter(log_interval=1, reg_log_interval=1, log_path=path)


def test_the_table_holds_the_five_terms_in_their_order(ft_all):
    ft = ft_all
    assert len(ft._reg_terms) == 5
    v = ft.vertices(slice(0, 4)).detach().reshape(4, -1, 3)
    direct = _direct(ft)
    want = [float(direct[name](v)) for name in NAMES]
    assert all(abs(a - b) > 1e-3 * max(a, b) for k, a in enumerate(want) for b in want[:k]), want      # (so that the order shows)
    for k, name in enumerate(NAMES):
        _close(float(ft._reg_terms[k](v, None)), want[k], f"entry {k} = {name}")
        assert bool((ft._reg_acc == 0).all())


@pytest.mark.parametrize("path", ['one_pass', 'torch'])
def test_gradient_with_all_five_on_is_the_pixel_terms_plus_the_five_functions(path):
    kw = {'one_pass': dict(), 'torch': dict(fused_loss=False)}[path]
    ft_on, ft_off = _fitter(**kw), _fitter(on=False, **kw)
    assert ft_off._reg_terms == [] and ft_off.rest is None and not ft_off._tex_prior_on
    _check_additive(path, ft_on, ft_off, slice(0, 4))


def test_second_of_two_ranks_takes_half_of_every_term_on_its_own_frames():
    ft_on, ft_off = _fitter(6, 1, 2), _fitter(6, 1, 2, on=False)
    assert (ft_on.frame_lo, ft_on.frame_hi) == (3, 6)
    _check_additive("rank1of2", ft_on, ft_off, slice(3, 6), share=0.5)


def test_log_record_of_iteration_0_states_the_terms_at_their_full_weight(ft_all):
    ft, frames = ft_all, slice(0, 4)
    assert ft.iteration == 0
    ft._log_step(frames, torch.zeros((), device='cuda'))
    assert bool((ft._reg_acc == 0).all())
    rec = json.loads(open(ft.cfg.log_path).read().splitlines()[-1])
    assert set(rec) == {"it", "frames", "loss", "lr", "MEL", "LAP", "STR", "BND", "MNC", "MOT", "TEXS", "TEXA"}, sorted(rec)
    assert rec["it"] == 0
    v = ft.vertices(frames).detach().reshape(4, -1, 3)
    direct = _direct(ft)
    with torch.no_grad():
        for key, name in (("STR", 'stretch'), ("BND", 'bend'), ("MOT", 'motion'), ("TEXS", 'TEXS'), ("TEXA", 'TEXA')):
            _close(rec[key], float(direct[name](v)), f"logged {key}")
    ft.step()
    assert bool((ft._reg_acc == 0).all())

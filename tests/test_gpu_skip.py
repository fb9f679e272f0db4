"""GPU: a fit step whose pixel objective ran out of record slots is SKIPPED ON THE DEVICE (include/fpcdr.h ABI v11:
fpcdr_objective_params.skip_out -> dist.GradBucket.flag -> fpcdr_adam_params.skip_flag / skipped): parameters and Adam moments stay as
they were, nothing raises, the run continues, and what follows is the run that never drew the skipped iteration (reference
fit.py:610-613 except for that iteration).  The shortage is forced through the launch-hint record of the batch shape."""
import math

import numpy as np
import pytest
import torch

from adam_ref import AdamRef
from helpers import rel_l2

pytestmark = pytest.mark.gpu

RENORM = (6, 8)      # q_opt, per_frame_q: the reference's whole-tensor division (fit.py:616-618)


def _onepass_hints(dr):
    return dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]


def _make(targets=None, **kw):
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg1', n_frames=2)
    sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
    # max_iter = 40: LambdaLR's lr_ramp^(i / max_iter) falls by 12 % per step -- a skipped step that left the schedule one step ahead
    # would show at once
    hp = dict(max_iter=40, cam_idxs=(0, 3, 6), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, weight_laplacian=40.0, init_texture='truth')
    hp.update(kw)
    cfg = fit.FitConfig(**hp)
    ft = fit.Fitter(sc, cfg, device='cuda', targets=targets)
    ft.init_near_truth(0.8)
    return ft


def _snapshot(ft):
    state = [p.detach().clone() for p in ft.params]
    for p in ft.params:
        st = ft.optimizer.state.get(p, {})
        if 'exp_avg' in st:
            state += [st['exp_avg'].clone(), st['exp_avg_sq'].clone()]
    return state


def _close(ft_a, ft_b, steps_apart=1):
    """Two Fitters that took the same step from the same state: equal up to the order of the float atomics inside a step -- every entry
    of every tensor to 1e-5, except that Adam turns a texel gradient that cancels to ~0 with no history into a step of the learning
    rate whose sign is that order's: the texture and its moments may hold a vanishing share of such entries."""
    sa, sb = _snapshot(ft_a), _snapshot(ft_b)
    assert len(sa) == len(sb)
    n_par = len(ft_a.params)
    tex_like = {i for i, t in enumerate(sa) if t.shape == ft_a.tex_opt.shape}
    for i, (a, b) in enumerate(zip(sa, sb)):
        d = (a - b).abs()
        tol = 1e-5 * max(1.0, float(b.abs().max())) if i < n_par else 1e-4 * max(float(b.abs().max()), 1e-30)
        if i in tex_like:
            assert float((d > tol).float().mean()) <= 2e-4 and float(d.max()) <= 2.0 * 2.5e-3 * steps_apart, (i, float(d.max()))
        else:
            assert float(d.max()) <= tol, (i, tuple(a.shape), float(d.max()), tol)


def test_short_record_pool_skips_the_update_on_the_device_and_the_run_continues(tmp_path, monkeypatch):
    import fpc_diffrend_amd.ops as dr
    dr.clear_hints()
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)       # compact records for this small batch too
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)
    k = 3
    ft = _make()
    for _ in range(k):
        assert math.isfinite(float(ft.step()))
    ft.save_checkpoint(str(tmp_path / "before.pt"))      # the state in front of iteration k
    before = _snapshot(ft)
    h = _onepass_hints(dr)
    h.poll()
    need = h.sil_bins
    assert need > 1
    h.slots, h.frozen = 1, True                          # iteration k: a pool that cannot hold the batch
    bad = ft.step()
    h.frozen = False
    assert math.isnan(float(bad))                        # the call says so in its value ...
    assert ft.skipped_steps == 1                         # ... the update kernel counted the skip ...
    for a, b in zip(_snapshot(ft), before):
        assert torch.equal(a, b)                         # ... and touched neither parameters nor moments (nor the quaternion division)
    # the run continues without an exception; the next call is sized from the demand the short call counted
    assert math.isfinite(float(ft.step()))
    h.poll()
    assert h.skipped_calls == 1 and h.overflowed is None and h.slots >= need
    # ... as the run that never drew the skipped iteration: a second Fitter resumes from the state in front of iteration k and takes
    # its step k with host counters and a schedule that never saw the skipped one -- the same update (the kernel re-forms the bias
    # corrections for step - skipped and the learning rate of one schedule step earlier, in double).  max_iter = 40 puts 12 % between two
    # consecutive learning rates and Adam's first bias corrections differ by 20 % from step to step: an update formed for the wrong
    # step would be off by 1e-3, not 1e-5
    plain = _make(targets=ft.targets)
    plain.load_checkpoint(str(tmp_path / "before.pt"))
    for a, b in zip(_snapshot(plain), before):
        assert torch.equal(a, b)
    plain.step()
    assert plain.skipped_steps == 0
    _close(ft, plain)
    ft.step()
    plain.step()
    _close(ft, plain, steps_apart=2)
    assert ft.skipped_steps == 1 and ft.iteration == plain.iteration + 1
    dr.clear_hints()


def test_skip_counter_survives_a_checkpoint(tmp_path, monkeypatch):
    import fpc_diffrend_amd.ops as dr
    dr.clear_hints()
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)
    a = _make()
    a.step()
    h = _onepass_hints(dr)
    h.poll()
    h.slots, h.frozen = 1, True
    a.step()
    h.frozen = False
    a.step()
    a.save_checkpoint(str(tmp_path / "ck.pt"))
    want = [float(a.step()) for _ in range(3)]
    b = _make(targets=a.targets)
    b.load_checkpoint(str(tmp_path / "ck.pt"))
    assert b.skipped_steps == 1
    got = [float(b.step()) for _ in range(3)]
    assert np.allclose(got, want, rtol=1e-5), (got, want)
    dr.clear_hints()


def test_a_caller_without_skip_out_still_learns_of_the_overflow(monkeypatch):
    """ops.pixel_objective without skip_out= (nobody to skip the update): the short call's value is NaN and the NEXT call on the shape
    raises -- also when another call on the shape finished in between (the device's overflow count is cumulative)."""
    import fpc_diffrend_amd.ops as dr
    from test_gpu_objective import _inputs
    pos, tri, uv, uv_idx, tex, ref = _inputs('soup', 1, (97, 131))
    ctx = dr.RasterizeGLContext(device='cuda')
    res = (97, 131)
    dr.clear_hints()
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)

    def run(**kw):
        p, t = pos.clone().requires_grad_(True), tex.clone().requires_grad_(True)
        loss = dr.pixel_objective(ctx, p, tri, uv, uv_idx, t, ref, res, **kw)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach())

    def enqueue(**kw):      # (no synchronisation: the host runs ahead of the device, as a fit loop does)
        p, t = pos.clone().requires_grad_(True), tex.clone().requires_grad_(True)
        return dr.pixel_objective(ctx, p, tri, uv, uv_idx, t, ref, res, **kw)

    good = run()
    h = _onepass_hints(dr)
    h.poll()
    need = h.sil_bins
    h.slots, h.frozen = 1, True
    assert math.isnan(run())
    h.frozen = False
    with pytest.raises(RuntimeError, match="ran out of record slots"):
        run()
    assert abs(run() - good) <= 1e-6 * abs(good)         # (the shape counts afresh and carries on)
    # the short call followed at once by a good one, nobody polling in between: the device's overflow count is cumulative, so the
    # second call's counters do not wipe it (they did: the flag was overwritten by every call)
    h.poll()
    h.slots, h.frozen = 1, True
    short = enqueue()
    h.frozen, h.slots = False, need + 8
    with pytest.raises(RuntimeError, match="ran out of record slots"):
        later = enqueue()                                # (raises here only if the short call has already landed)
        torch.cuda.synchronize()
        assert math.isnan(float(short)) and abs(float(later) - good) <= 1e-6 * abs(good)
        run()
    assert abs(run() - good) <= 1e-6 * abs(good)
    # with skip_out the same shortage is reported through the flag, in the same call, and nothing raises later
    flag = torch.full((1,), 7.0, device='cuda')
    assert abs(run(skip_out=flag) - good) <= 1e-6 * abs(good) and float(flag) == 0.0
    h.poll()
    h.slots, h.frozen = 1, True
    assert math.isnan(run(skip_out=flag)) and float(flag) == 1.0
    h.frozen = False
    assert abs(run(skip_out=flag) - good) <= 1e-6 * abs(good) and float(flag) == 0.0
    dr.clear_hints()


def _short_step(ft, dr):
    """One step whose pixel objective runs out of record slots: skipped on the device."""
    h = _onepass_hints(dr)
    h.poll()
    h.slots, h.frozen = 1, True
    bad = ft.step()
    h.frozen = False
    assert math.isnan(float(bad))


def _lrs(ft, it, skipped):
    """The group learning rates of iteration `it` in the run that never drew the `skipped` steps before it (reference fit.py:506-507)."""
    cfg = ft.cfg
    return [b * cfg.lr_ramp ** ((it - skipped) / cfg.max_iter) for b in ft.scheduler.base_lrs]


def _checked_step(ft, ref, skipped, tol=2e-6):
    """One step of the Fitter and the float64 reference's update from the gradients that step left on the parameters (the way
    test_optimiser_steps_match_oracle (A) reads them); every parameter must be finite and equal the reference."""
    it = ft.iteration
    for p in ft.params:
        p.grad = None
    loss = float(ft.step())
    assert math.isfinite(loss), (it, loss)
    ref.update([p.grad.detach().clone() if p.grad is not None else None for p in ft.params], _lrs(ft, it, skipped))
    for k, p in enumerate(ft.params):
        assert bool(torch.isfinite(p).all()), f"iteration {it}: parameter {k} has non-finite values"
        e = rel_l2(p, ref.p[k])
        assert e <= tol, (it, k, e)
    return loss


def test_combined_mode_switch_after_a_skip_trains_the_learned_basis_from_its_own_step_count(tmp_path, monkeypatch):
    """Combined mode (cfg5's) switches the learned basis m1 / m2 / m3 on half way (fit.py:603-608): their FIRST update comes after a step
    skipped on the device.  Their own step counts hold no skip, so the update is Adam's first step for them -- the global skip count taken
    off their counters made it a step count of 0 (infinite step size) and the parameters NaN.  After every step that was not skipped the
    parameters equal the float64 reference of the run that never drew the skipped step; a checkpoint written between the skip and the
    switch resumes into the same run."""
    import fpc_diffrend_amd.ops as dr
    dr.clear_hints()
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)
    ft = _make(mode='combined', max_iter=6)        # the learned basis receives its first gradient in iteration 5
    ref = AdamRef(ft.params, renorm=RENORM)
    for _ in range(2):
        _checked_step(ft, ref, 0)
    assert all(p.grad is None for p in ft.params[:3])
    _short_step(ft, dr)                            # iteration 2
    assert ft.skipped_steps == 1
    _checked_step(ft, ref, 1)                      # iteration 3
    ft.save_checkpoint(str(tmp_path / "before_switch.pt"))
    for _ in range(4):                             # iterations 4 .. 7: the switch, the basis's first updates
        _checked_step(ft, ref, 1)
    assert ft.skipped_steps == 1
    assert all(ref.step[k] == 3 for k in range(3)) and all(ref.step[k] == 7 for k in range(3, 10))
    assert [int(ft.optimizer.state[p]['step']) for p in ft.params] == [3] * 3 + [8] * 7
    assert ft.skipped_steps_per_tensor() == [0] * 3 + [1] * 7
    # resumed from the checkpoint between the skip and the switch: the uninterrupted run
    b = _make(targets=ft.targets, mode='combined', max_iter=6)
    b.load_checkpoint(str(tmp_path / "before_switch.pt"))
    assert b.skipped_steps == 1 and b.skipped_steps_per_tensor() == [0] * 3 + [1] * 7
    for _ in range(4):
        assert math.isfinite(float(b.step()))
    assert b.iteration == ft.iteration and b.skipped_steps == 1
    _close(ft, b, steps_apart=4)
    dr.clear_hints()


def test_checkpoint_without_per_tensor_skip_counts_loads_as_before(tmp_path, monkeypatch):
    """A checkpoint written before the per-tensor skip counts (no 'skipped_per_tensor') takes the global count for every tensor with
    optimiser state -- what the update kernel assumed then -- and continues exactly as the same checkpoint with the counts."""
    import fpc_diffrend_amd.ops as dr
    dr.clear_hints()
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)
    a = _make()
    a.step()
    _short_step(a, dr)
    a.step()
    a.save_checkpoint(str(tmp_path / "ck.pt"))
    state = torch.load(str(tmp_path / "ck.pt"), weights_only=False)
    assert state["skipped_steps"] == 1 and state["skipped_per_tensor"] == [0] * 3 + [1] * 7
    del state["skipped_per_tensor"]
    torch.save(state, str(tmp_path / "legacy.pt"))
    new, old = _make(targets=a.targets), _make(targets=a.targets)
    new.load_checkpoint(str(tmp_path / "ck.pt"))
    old.load_checkpoint(str(tmp_path / "legacy.pt"))
    assert old.skipped_steps == 1 and old.skipped_steps_per_tensor() == new.skipped_steps_per_tensor() == [0] * 3 + [1] * 7
    want = [float(new.step()) for _ in range(3)]
    got = [float(old.step()) for _ in range(3)]
    assert np.allclose(got, want, rtol=1e-5), (got, want)
    _close(old, new, steps_apart=3)
    dr.clear_hints()


@pytest.mark.parametrize("kind", ["hip_graph", "torch_adam"])
def test_checkpoint_with_skips_into_an_optimiser_that_cannot_skip(tmp_path, monkeypatch, kind):
    """A checkpoint of a run that skipped a step, loaded into a Fitter whose optimiser has no device skip counter (graph mode's capturable
    GroupedAdam; torch.optim.Adam): the skipped step becomes one never drawn -- each tensor's step count loses its skips, the schedule
    the total -- and the next step equals the float64 reference update of the checkpoint's state with that step's own gradients."""
    import fpc_diffrend_amd.ops as dr
    dr.clear_hints()
    monkeypatch.setattr(dr, "SMALL_BATCH_BINS", 0)
    monkeypatch.setattr(dr, "RECORD_SLOT_MARGIN", 1)
    a = _make()
    a.step()
    _short_step(a, dr)
    a.step()
    a.step()
    a.save_checkpoint(str(tmp_path / "ck.pt"))
    state = torch.load(str(tmp_path / "ck.pt"), weights_only=False)
    per, it = state["skipped_per_tensor"], state["iteration"]
    assert state["skipped_steps"] == 1 and per == [0] * 3 + [1] * 7 and it == 4
    monkeypatch.undo()                             # (the new Fitter runs with the default record pool)
    dr.clear_hints()
    b = _make(targets=a.targets, **(dict(hip_graph=True) if kind == "hip_graph" else dict(grouped_adam=False)))
    b.load_checkpoint(str(tmp_path / "ck.pt"))
    assert b.skipped_steps == 0 and b.scheduler.last_epoch == it - 1
    ref = AdamRef(b.params, renorm=RENORM)
    for k, p in enumerate(b.params):
        st = state["optimizer"]["state"].get(k)
        if st is not None:
            ref.load(k, p, st["exp_avg"], st["exp_avg_sq"], int(st["step"]) - per[k])
            assert int(b.optimizer.state[p]["step"]) == ref.step[k]
    assert all(abs(float(g["lr"]) - lr) <= 1e-12 * lr for g, lr in zip(b.optimizer.param_groups, _lrs(b, it, 1)))
    _checked_step(b, ref, 1)
    assert [int(b.optimizer.state[p]["step"]) for p in b.params[3:]] == ref.step[3:] == [4] * 7
    dr.clear_hints()

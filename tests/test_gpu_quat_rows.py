"""GPU: quaternions normalised one by one ("Quaternion normalisation"; FitConfig.quat_renorm='rows', fit.GroupedAdam(...,
renorm_rows=True), fpcdr_adam_tensor.renorm = 2 in csrc/adam.hip: one lane updates one row of four and divides it by its own norm).

fpcdr_adam_step with renorm = 2 against tests/adam_ref.py's float64 Adam followed by the division of every row by its own norm, after
every step, for the parameter and both moments, to tests/test_gpu_adam.py's bar (rel-L2 1e-6): rows in {1, 9, 63, 64, 65, 257} (a lane,
the wave's edge, the workgroup's edge and past it), with a gradient and division only, beside a plain tensor in the same launch, through
the device-table path too.  renorm = 1 -- the whole-tensor division, quirk Q3 -- stays what it was: on recorded inputs its results equal,
bit for bit, what the library built from the commit before this option gave (tests/golden/adam_renorm_tensor.pt), and they agree with the
unchanged float64 reference.  Two eager Fitter steps under 'rows' with grouped_adam on and off agree to the few ulps a step that
GroupedAdam's docstring promises."""
import os

import pytest
import torch

from adam_ref import AdamRef
from helpers import fitter_near_truth, rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-6
U = 2.0 ** -24
ROWS = (1, 9, 63, 64, 65, 257)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_renorm_tensor.pt")


def _divide_rows(ref, ks):
    for k in ks:
        ref.p[k] = ref.p[k] / ref.p[k].square().sum(dim=1, keepdim=True).sqrt()


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("with_grad", [True, False])
def test_rows_against_float64_adam_and_per_row_division(with_grad, capturable):
    from fpc_diffrend_amd import fit
    gen = torch.Generator().manual_seed(11)
    quats = [(torch.randn(r, 4, generator=gen) * (0.2 + 0.3 * i)).cuda() for i, r in enumerate(ROWS)]
    plain = [torch.randn(1001, generator=gen).cuda(), torch.randn(64, 4, generator=gen).cuda()]
    params = quats + plain
    nq = len(quats)
    lrs = [1e-2 * (0.6 + 0.1 * k) for k in range(len(params))]
    opt = fit.GroupedAdam([{"params": p, "lr": lr} for p, lr in zip(params, lrs)], lr=1e-3, renorm=quats, renorm_rows=True, capturable=capturable)
    if capturable:
        for p in params[nq:] + (quats if with_grad else []):
            p.requires_grad_(True)
    ref = AdamRef(params)
    for it in range(4):
        grads = [(torch.randn(p.shape, generator=gen) * (10.0 ** (k % 4 - 2))) if (with_grad or k >= nq) else None for k, p in enumerate(params)]
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.cuda()
        if capturable:
            opt.prepare()
        opt.step()
        torch.cuda.synchronize()
        ref.update(grads, lrs)
        _divide_rows(ref, range(nq))
        for k, p in enumerate(params):
            assert bool(torch.isfinite(p).all())
            e = rel_l2(p, ref.p[k])
            assert e <= TOL, (it, k, tuple(p.shape), e)
            if grads[k] is not None:
                st = opt.state[p]
                assert int(st['step']) == it + 1
                assert rel_l2(st['exp_avg'], ref.m[k]) <= TOL and rel_l2(st['exp_avg_sq'], ref.v[k]) <= TOL, (it, k)
            else:
                assert 'exp_avg' not in opt.state.get(p, {})
        for q in quats:      # every row is a unit quaternion to 4 u: products and two levels of adds 3 u on the sum of squares, so 1.5 u
            # on the norm, its root 1 u, the quotient 1 u
            assert float((q.detach().double().norm(dim=1) - 1.0).abs().max()) <= 4 * U
    # a tensor that does not hold quaternions is refused
    odd = torch.randn(6, generator=gen).cuda()
    with pytest.raises(AssertionError, match="quaternions"):
        fit.GroupedAdam([{"params": odd, "lr": 1e-3}], renorm=[odd], renorm_rows=True)


def _golden_run(data):
    """The recorded inputs through fit.GroupedAdam(renorm=...) -- the whole-tensor division -- for the recorded number of steps."""
    from fpc_diffrend_amd import fit
    out = []
    for case in data['cases']:
        params = [p.clone().cuda() for p in case['params']]
        opt = fit.GroupedAdam([{"params": p, "lr": lr} for p, lr in zip(params, case['lrs'])], lr=1e-3, renorm=params[:case['n_renorm']])
        for grads in case['grads']:
            for p, g in zip(params, grads):
                p.grad = None if g is None else g.clone().cuda()
            opt.step()
        torch.cuda.synchronize()
        out.append([p.detach().cpu() for p in params])
    return out


def test_whole_tensor_division_is_bit_for_bit_what_it_was():
    data = torch.load(GOLDEN, weights_only=True)
    got = _golden_run(data)
    for case, want, mine in zip(data['cases'], data['results'], got):
        for k, (w, m) in enumerate(zip(want, mine)):
            assert torch.equal(w, m), (case['name'], k)
        # ... and what it was agrees with the unchanged float64 reference
        ref = AdamRef(case['params'], renorm=range(case['n_renorm']))
        for grads in case['grads']:
            ref.update(grads, case['lrs'])
        for k, m in enumerate(mine):
            assert rel_l2(m, ref.p[k]) <= TOL, (case['name'], k)


def test_two_eager_fitter_steps_with_grouped_adam_on_and_off():
    """'rows' in the kernel (grouped_adam) and in the torch branch of Fitter._update: the same parameters to 4 ulps of the tensor's
    largest entry a step (the update is the same formula in another order, the norm one more rounding), every quaternion a unit
    quaternion, and not what 'tensor' leaves."""
    gen = torch.Generator().manual_seed(5)
    q0 = torch.randn(4, 4, generator=gen)
    q0 = (q0 / q0.norm(dim=1, keepdim=True)).cuda()
    fts = {}
    for grouped in (True, False):
        ft = fitter_near_truth(4, quat_renorm='rows', grouped_adam=grouped, lr_q=1e-3)
        with torch.no_grad():
            ft.per_frame_q.copy_(q0)
        for _ in range(2):
            ft.step()
        fts[grouped] = ft
        for q in (ft.per_frame_q, ft.q_opt):
            assert float((q.detach().double().norm(dim=1) - 1.0).abs().max()) <= 4 * U
        assert float((ft.per_frame_q.detach() - q0).abs().max()) > 0.0       # (the step moved them)
    assert fts[True]._grouped and not fts[False]._grouped and fts[True].cfg.quat_renorm == 'rows'
    assert fts[True].state_dict()['config']['quat_renorm'] == 'rows'
    for k, (a, b) in enumerate(zip(fts[True].params, fts[False].params)):
        a, b = a.detach().double(), b.detach().double()
        err, bar = float((a - b).abs().max()), 2 * 4 * U * float(a.abs().max())
        print(f"QUATROWS fitter tensor {k} {tuple(a.shape)} max |on - off| = {err:.3e} bar {bar:.3e}")
        assert err <= bar, (k, err, bar)
    ft = fitter_near_truth(4, lr_q=1e-3)                                      # 'tensor': every row comes out at 1 / sqrt(F)
    ft.step()
    assert abs(float(ft.per_frame_q.detach().double().norm()) - 1.0) <= 4 * U

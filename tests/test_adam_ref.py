"""CPU: the float64 yardstick of the optimiser tests (tests/adam_ref.py) is torch.optim.Adam's update -- checked against torch.optim.Adam
itself in float64, with per-group learning rates, a schedule, tensors that start late or miss steps and the whole-tensor division."""
import torch

from adam_ref import AdamRef


def test_float64_reference_equals_torch_adam():
    g = torch.Generator().manual_seed(11)
    shapes = [(7, 3), (5,), (9, 4), (1,)]
    lrs = [1e-2, 3e-3, 2e-2, 5e-3]
    start = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    ref = AdamRef(start, renorm=(2,))
    b = [t.clone().requires_grad_(True) for t in start]
    opt = torch.optim.Adam([{"params": p, "lr": lr} for p, lr in zip(b, lrs)], lr=1e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: 0.7 ** x)
    for it in range(7):
        grads = []
        for k, p in enumerate(b):
            none = (k == 1 and it < 3) or (k == 2 and it in (1, 4)) or (k == 3 and it == 5)
            gr = None if none else torch.randn(p.shape, generator=g, dtype=torch.float64) * 10.0 ** (k - 1)
            if gr is not None and k == 0:
                gr[2] = 0.0                                   # a row without coverage
            p.grad = gr
            grads.append(gr)
        ref.update(grads, [lr * 0.7 ** it for lr in lrs])
        opt.step()
        with torch.no_grad():
            b[2] /= torch.sum(b[2] ** 2) ** 0.5
        sched.step()
        for k, p in enumerate(b):
            assert torch.allclose(ref.p[k], p.detach(), rtol=1e-13, atol=1e-15), (it, k)
            st = opt.state.get(p, {})
            assert ref.step[k] == (int(st['step']) if 'step' in st else 0), (it, k)
            if 'exp_avg' in st:
                assert torch.allclose(ref.m[k], st['exp_avg'], rtol=1e-13, atol=1e-18)
                assert torch.allclose(ref.v[k], st['exp_avg_sq'], rtol=1e-13, atol=1e-18)
    assert ref.step == [7, 4, 5, 6]

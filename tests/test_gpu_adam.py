"""GPU: fpcdr_adam_step (fit.GroupedAdam, include/fpcdr.h) against the float64 restatement of torch.optim.Adam in tests/adam_ref.py,
after every step, for every parameter and both moments: the sizes and alignments that pick the kernel's float4 loop, its scalar loop and
its grid-stride passes; a full table of sixteen tensors; the whole-tensor quaternion division; tensors that start late or miss steps;
the device-table (capturable, HIP-graph) path; and steps skipped on the device (ABI v11 skip_flag / skipped, v12 skipped_per_tensor).

Learning rates near 1e-2 on O(1) parameters and gradient scales from 1e-3 to 1e2: Adam's first bias corrections differ by 20-90 % from
one step count to the next, so an update formed for the wrong step count misses the 1e-6 bar by orders of magnitude.  There are no float
atomics in the kernel: every result is deterministic."""
import ctypes

import pytest
import torch

from adam_ref import AdamRef
from helpers import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-6
SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2)
GRID_PASS = 1024 * 256 * 4      # floats one pass of the capped grid covers on the float4 path


def _grad(shape, gen, k):
    """Tensor k's gradient: seeded normal values at one of six scales, exactly zero on every seventh element from the fourth on
    (uncovered texels)."""
    g = torch.randn(shape, generator=gen) * SCALES[k % len(SCALES)]
    g.view(-1)[3::7] = 0.0
    return g


def _params(shapes, gen):
    return [torch.randn(s, generator=gen).cuda() for s in shapes]


def _snapshot(opt, params):
    """Every parameter, and the two moments of every tensor that has optimiser state (None for one that has none yet)."""
    out = [p.detach().clone() for p in params]
    for p in params:
        st = opt.state.get(p, {})
        out.append((st['exp_avg'].clone(), st['exp_avg_sq'].clone()) if 'exp_avg' in st else None)
    return out


def _unchanged(before, after):
    """A skipped step: parameters and moments bit for bit as they were -- a tensor whose first gradient came in that step has its state
    created (the host counted the step) with both moments still zero."""
    assert len(before) == len(after)
    for a, b in zip(after, before):
        if torch.is_tensor(b):
            if not torch.equal(a, b):
                return False
        elif b is not None:
            if not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])):
                return False
        elif a is not None and (a[0].any() or a[1].any()):
            return False
    return True


def _check(opt, params, ref, it, extra_steps=None):
    """Every parameter and both moments against the reference; the host's step counters against the reference's (plus the skipped steps
    the host counted for that tensor)."""
    for k, p in enumerate(params):
        assert bool(torch.isfinite(p).all()), f"step {it}: tensor {k} (n = {p.numel()}) has non-finite values"
        e = rel_l2(p, ref.p[k])
        assert e <= TOL, (it, k, p.numel(), e)
        st = opt.state.get(p, {})
        if ref.step[k] == 0 and not (extra_steps and extra_steps[k]):
            assert 'exp_avg' not in st or (not st['exp_avg'].any() and not st['exp_avg_sq'].any()), (it, k)
            continue
        assert int(st['step']) == ref.step[k] + (extra_steps[k] if extra_steps else 0), (it, k, int(st['step']), ref.step[k])
        for name, mine, want in (('exp_avg', st['exp_avg'], ref.m[k]), ('exp_avg_sq', st['exp_avg_sq'], ref.v[k])):
            assert bool(torch.isfinite(mine).all()), f"step {it}: {name} of tensor {k} has non-finite values"
            e = rel_l2(mine, want)
            assert e <= TOL, (it, k, name, e)


def _drive(params, lrs, steps, has_grad, renorm=(), skips=(), gain=1.25, seed=0, place=None):
    """Run `steps` steps of a GroupedAdam over `params` (learning rates `lrs`, schedule lr * (1 / gain)^i) beside the reference.
    has_grad(k, it): whether tensor k receives a gradient in step it.  skips: the steps whose device skip_flag is set (the optimiser
    then runs with enable_skips(gain)); the reference never draws them and takes the schedule of the run without them.
    place(k, g): the device tensor that becomes tensor k's .grad (default: a plain copy)."""
    from fpc_diffrend_amd import fit
    gen = torch.Generator().manual_seed(1000 + seed)
    opt = fit.GroupedAdam([{"params": p, "lr": lr} for p, lr in zip(params, lrs)], lr=1e-3, renorm=[params[k] for k in renorm])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: (1.0 / gain) ** x)
    ref = AdamRef(params, renorm=renorm)
    flag = None
    if skips:
        opt.enable_skips(lr_skip_gain=gain)
        flag = torch.zeros(1, dtype=torch.float32, device='cuda')
        opt.skip_flag = flag
    extra = [0] * len(params)      # skipped steps in which the host counted a step for the tensor
    n_skipped = 0
    for it in range(steps):
        grads = [_grad(p.shape, gen, k) if has_grad(k, it) else None for k, p in enumerate(params)]
        for k, (p, g) in enumerate(zip(params, grads)):
            p.grad = None if g is None else (place(k, g) if place is not None else g.cuda())
        skip = it in skips
        if flag is not None:
            flag.fill_(1.0 if skip else 0.0)
        before = _snapshot(opt, params) if skip else None
        opt.step()
        sched.step()
        if skip:
            n_skipped += 1
            for k, g in enumerate(grads):
                extra[k] += g is not None
            assert _unchanged(before, _snapshot(opt, params)), f"skipped step {it} changed state"
            assert int(opt.skipped) == n_skipped
            continue
        ref.update(grads, [lr * (1.0 / gain) ** (it - n_skipped) for lr in lrs])
        _check(opt, params, ref, it, extra)
    return opt, ref, extra


SIZES = (1, 3, 4, 1001, GRID_PASS, GRID_PASS + 1, GRID_PASS + 4, 3 * 1024 * 1024)


def test_sizes_float4_scalar_and_grid_stride_paths():
    """n % 4 == 0 with aligned pointers: the float4 loop; otherwise the scalar loop.  The grid is capped at 1 024 blocks x 256 threads:
    2^20 floats is exactly one pass of the float4 loop, 2^20 + 4 a second pass for one float4, 2^20 + 1 and 3 x 2^20 (a three-channel
    1024^2 texture) several passes of their loops."""
    gen = torch.Generator().manual_seed(1)
    params = _params([(n,) for n in SIZES], gen)
    lrs = [1e-2 * (0.6 + 0.1 * k) for k in range(len(params))]
    _drive(params, lrs, 4, lambda k, it: True)


def test_misaligned_parameter_and_gradient_take_the_scalar_path():
    """A parameter, and separately a gradient, that is a contiguous view 4 bytes into a larger buffer: n % 4 == 0 but not 16-byte
    aligned, so the tensor must run on the scalar loop -- once with a small tensor, once over several grid passes."""
    gen = torch.Generator().manual_seed(2)
    sizes = (4096, GRID_PASS + 4, 4096, GRID_PASS + 4, 4096)
    bases = [torch.randn(n + 1, generator=gen).cuda() for n in sizes]
    params = [bases[0][1:], bases[1][1:], bases[2][:-1], bases[3][:-1], bases[4][:-1]]
    assert all(p.is_contiguous() for p in params)
    assert params[0].data_ptr() % 16 == 4 and params[1].data_ptr() % 16 == 4 and params[2].data_ptr() % 16 == 0
    mis_grad = {2, 3}
    grad_bufs = {}

    def place(k, g):
        if k not in mis_grad:
            return g.cuda()
        buf = torch.empty(g.numel() + 1, dtype=torch.float32, device='cuda')
        buf[1:] = g.cuda()
        grad_bufs[k] = buf        # (kept alive until the launch has run)
        v = buf[1:]
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    lrs = [1e-2, 8e-3, 1.2e-2, 9e-3, 1.1e-2]
    _drive(params, lrs, 4, lambda k, it: True, place=place)


def test_sixteen_tensors_in_one_launch_and_a_seventeenth_is_refused():
    from fpc_diffrend_amd import _lib, fit
    assert _lib.ADAM_MAX_TENSORS == 16
    gen = torch.Generator().manual_seed(3)
    sizes = [1, 2, 3, 4, 5, 7, 8, 36, 64, 100, 255, 256, 1001, 1024, 4000, 65537]
    params = _params([(n,) for n in sizes], gen)
    lrs = [1e-2 * (0.5 + 0.07 * k) for k in range(16)]
    has = lambda k, it: not (k % 5 == 1 and it == 1) and not (k == 13 and it == 0)
    _drive(params, lrs, 4, has, renorm=(7, 13))
    extra = torch.zeros(4).cuda()
    with pytest.raises(AssertionError, match="more parameter tensors"):
        fit.GroupedAdam([{"params": p, "lr": 1e-2} for p in params + [extra]])
    P = _lib.AdamParams()
    P.n_tensors = _lib.ADAM_MAX_TENSORS + 1
    with pytest.raises(RuntimeError, match="too many tensors"):
        _lib.call("fpcdr_adam_step", ctypes.byref(P), fit._stream())


def test_quaternion_tensors_divided_by_their_whole_norm_with_and_without_a_gradient():
    """The renorm block walks the tensor in steps of 256 threads: 36 floats (the camera quaternions), 1 024 (per-frame quaternions of
    256 frames) and 4 000 (not a multiple of 256), each also in steps where it has no gradient and is only divided."""
    gen = torch.Generator().manual_seed(4)
    params = _params([(9, 4), (256, 4), (1000, 4), (777,)], gen)
    has = lambda k, it: not ((k == 0 and it in (1, 2)) or (k == 1 and it == 0) or (k == 2 and it in (2, 4)))
    _drive(params, [1e-2, 2e-2, 5e-3, 1e-2], 6, has, renorm=(0, 1, 2))


def test_late_starters_count_their_own_steps():
    gen = torch.Generator().manual_seed(5)
    params = _params([(300, 3), (1001,), (64, 64), (5, 4), (9, 4)], gen)
    starts = (0, 2, 3, 1, 4)
    gaps = {(0, 3), (3, 4), (3, 5), (2, 6)}
    has = lambda k, it: it >= starts[k] and (k, it) not in gaps
    opt, ref, _ = _drive(params, [1e-2, 3e-3, 2e-2, 1e-2, 7e-3], 8, has, renorm=(4,))
    assert ref.step == [7, 6, 4, 5, 4]
    assert [int(opt.state[p]['step']) for p in params] == ref.step


def test_capturable_device_table_eager_and_replayed_in_a_graph():
    """GroupedAdam(capturable=True): per-tensor (step_size, bc2_sqrt) from the device table prepare() writes.  Two eager steps, then one
    step() captured in a HIP graph and replayed with prepare() and fresh gradients (copied into the captured buffers) in front of each
    replay; a quaternion tensor that is not trainable is only divided."""
    from fpc_diffrend_amd import fit
    gen = torch.Generator().manual_seed(6)
    params = _params([(1001,), (4096,), (9, 4), (256, 4), (3,)], gen)
    trainable = [True, True, True, False, True]
    for p, t in zip(params, trainable):
        p.requires_grad_(t)
    lrs = [1e-2, 5e-3, 2e-2, 1e-2, 8e-3]
    opt = fit.GroupedAdam([{"params": p, "lr": lr} for p, lr in zip(params, lrs)], lr=1e-3, renorm=(params[2], params[3]),
                          capturable=True)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda x: 0.8 ** x)
    ref = AdamRef(params, renorm=(2, 3))
    bufs = [torch.zeros_like(p) if t else None for p, t in zip(params, trainable)]
    for p, b in zip(params, bufs):
        p.grad = b
    graph = None
    for it in range(6):
        grads = [_grad(p.shape, gen, k) if t else None for k, (p, t) in enumerate(zip(params, trainable))]
        for b, g in zip(bufs, grads):
            if b is not None:
                b.copy_(g)
        if it == 2:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()              # (captured, not run)
        opt.prepare()
        if graph is None:
            opt.step()
        else:
            graph.replay()
        sched.step()
        ref.update(grads, [lr * 0.8 ** it for lr in lrs])
        _check(opt, params, ref, it)
    assert [int(opt.state[p]['step']) for p, t in zip(params, trainable) if t] == [6, 6, 6, 6]


# skip schedules: a skip on the very first step, two consecutive ones and a later one; and one without a first-step skip.  `starts`:
# the first gradient of the late starters -- after one, three (first schedule) or one, two, four skips (second) -- and, last, one whose
# first gradient comes IN a skipped step (the host counts that step for it, so must the kernel)
SKIP_CASES = {"first_pair_later": dict(skips=(0, 3, 4, 9), starts=(1, 5, 3)),
              "spread": dict(skips=(2, 4, 7, 8), starts=(3, 5, 9, 4))}


@pytest.mark.parametrize("case", sorted(SKIP_CASES))
def test_skipped_steps_touch_nothing_and_the_rest_is_the_run_that_never_drew_them(case):
    """enable_skips(lr_skip_gain = g) with a schedule that falls by 1/g per step, skip_flag set by hand on chosen steps.  A skipped step
    leaves every parameter and moment as it was (the quaternion division included); every other step is the update of the run that
    never drew the skipped ones -- for tensors that had a gradient in the skipped steps, tensors that had none, and tensors whose FIRST
    gradient comes only after one or more skips (the learned basis of the combined mode, switched on half way)."""
    skips, starts = SKIP_CASES[case]["skips"], SKIP_CASES[case]["starts"]
    gen = torch.Generator().manual_seed(7)
    fixed = [(1001,), (4096,), (300, 3), (9, 4), (256, 4)]
    params = _params(fixed + [(777,)] * len(starts), gen)
    n_fixed = len(fixed)

    def has(k, it):
        if k == 2:
            return it not in skips                  # no gradient in any skipped step
        if k == 4:
            return it % 2 == 0                      # a quaternion tensor that is only divided in odd steps
        if k >= n_fixed:
            return it >= starts[k - n_fixed]
        return True                                 # a gradient in every step, the skipped ones included

    lrs = [1e-2 * (0.6 + 0.1 * k) for k in range(len(params))]
    opt, ref, extra = _drive(params, lrs, 12, has, renorm=(3, 4), skips=skips, gain=1.3, seed=7)
    assert int(opt.skipped) == len(skips)
    assert all(ref.step[k] >= 1 for k in range(len(params)))
    rows = opt.skipped_per_tensor.cpu().tolist()
    assert rows[:len(params)] == extra and not any(rows[len(params):]), (rows, extra)

"""HIP-event times of the motion term (csrc/mesh_reg.hip, k_motion_penalty) at F = 32 meshes of two sizes -- V = 514 (cfg1's mesh) and
V = 15002 (the UV sphere scripts/time_bend.py uses) --, the variants taking turns in one process:

  fpcdr_motion_penalty order 2              value and gradient: the stencil kernel and the finish kernel
  fpcdr_motion_penalty order 2, Charbonnier the same with a scale (one square root and two divisions a stencil)
  fpcdr_motion_penalty order 2, value only  grad_x = NULL
  fpcdr_motion_penalty order 1              the two-frame stencil
  torch order 2 fwd + bwd                   weight / F * sum_f mean_v |x_{f-1} - 2 x_f + x_{f+1}|^2 and its autograd backward on the same
                                            tensors on the GPU: the yardstick
  torch order 2 Charbonnier fwd + bwd       the same through 2 c^2 (sqrt(1 + s / c^2) - 1)

Before timing, every call is held against torch's expression: the value, and the gradient's relative L2.

Algorithmic bytes of the full call: every position read once (12 F V) and every gradient entry written once (12 F V); that a position is
read by the lanes of up to five frames is cache traffic.

With --step: a cfg3 step (bench.py's flagship configuration) with weight_motion = 0 and with the term on, taking turns, host clock around
`steps` steps that end in a synchronise.  A commit whose FitConfig has no such option (the parent) gets the "off" figure alone: run the
script there too, in turns with this one, to compare the step with the term off against it.

    python scripts/time_motion.py [--commit NAME] [--seconds S] [--step]
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 32


def time_turns(variants, seconds, calls=20):
    import numpy as np
    import torch
    for _, fn in variants:                  # warm-up: code objects, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    turns = {name: [] for name, _ in variants}
    t0 = time.perf_counter()
    while min(sum(v) * calls for v in turns.values()) < seconds * 1e3 or len(turns[variants[0][0]]) < 10:
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            turns[name].append(e0.elapsed_time(e1) / calls)
        if time.perf_counter() - t0 > 60:
            break
    med = {}
    for name, _ in variants:
        t = np.sort(np.asarray(turns[name])) * 1e3
        med[name] = float(np.median(t))
        print(f"  {name:44s} median {med[name]:8.2f} us a call (min {t[0]:.2f}, max {t[-1]:.2f}, {t.size} turns of {calls} calls)", flush=True)
    return med


def calls_at(V, base, seconds):
    import torch
    from fpc_diffrend_amd import _lib, fit
    g = torch.Generator().manual_seed(0)
    amp, ph = 0.5 * torch.randn(V, 3, generator=g), 6.28 * torch.rand(V, 1, generator=g)
    f = torch.arange(F, dtype=torch.float32)[:, None, None]
    x = (base[None] + amp[None] * torch.sin(0.7 * f + ph[None]) + 0.05 * torch.randn(F, V, 3, generator=g)).float().cuda().contiguous()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gx = torch.empty_like(x)
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    per, out = torch.empty(F, dtype=torch.float32, device='cuda'), torch.empty((), dtype=torch.float32, device='cuda')
    w, c = 7.5, 0.3
    inv_c = fit.motion_inv_scale(c)

    def call(order, ic, grad=True):
        _lib.call("fpcdr_motion_penalty", p(x), None, None, ic, order, p(gx) if grad else None, p(acc), p(per), p(out), w, F, V, st())

    leaf = x.clone().requires_grad_(True)

    def torch_term(order, scale):
        a = leaf[:-2] - 2.0 * leaf[1:-1] + leaf[2:] if order == 2 else leaf[1:] - leaf[:-1]
        s = (a * a).sum(dim=2)
        rho = s if scale is None else 2.0 * scale * scale * (torch.sqrt(1.0 + s / (scale * scale)) - 1.0)
        return (w / F) * rho.mean(dim=1).sum()

    def torch_run(order, scale):
        leaf.grad = None
        torch_term(order, scale).backward()

    # faster and different is not faster
    for order, ic, scale in ((2, 0.0, None), (2, inv_c, c), (1, 0.0, None)):
        call(order, ic)
        torch_run(order, scale)
        tv = float(torch_term(order, scale).detach())
        rel = float((gx - leaf.grad).norm() / leaf.grad.norm())
        print(f"  V = {V}: order {order}{'' if scale is None else ' c = %g' % scale}: call {float(out):.6f} torch {tv:.6f}, gradient rel-L2 "
              f"against torch's {rel:.2e}", flush=True)
        assert abs(float(out) - tv) <= 1e-4 * abs(tv) and rel < 1e-4
    variants = [("fpcdr_motion_penalty order 2", lambda: call(2, 0.0)),
                ("fpcdr_motion_penalty order 2, Charbonnier", lambda: call(2, inv_c)),
                ("fpcdr_motion_penalty order 2, value only", lambda: call(2, 0.0, False)),
                ("fpcdr_motion_penalty order 1", lambda: call(1, 0.0)),
                ("torch order 2 fwd + bwd", lambda: torch_run(2, None)),
                ("torch order 2 Charbonnier fwd + bwd", lambda: torch_run(2, c))]
    med = time_turns(variants, seconds)
    nbytes = 24.0 * F * V
    t = med["fpcdr_motion_penalty order 2"]
    print(f"  V = {V}: fpcdr_motion_penalty / torch: {t / med['torch order 2 fwd + bwd']:.4f} (L2), "
          f"{med['fpcdr_motion_penalty order 2, Charbonnier'] / med['torch order 2 Charbonnier fwd + bwd']:.4f} (Charbonnier); "
          f"{nbytes / 1e6:.2f} MB algorithmic -> {nbytes / (t * 1e-6) / 1e9:.0f} GB/s", flush=True)


def step_times(seconds, steps=20):
    """A cfg3 step with the term off and on, taking turns; a FitConfig without the option (the parent commit) times "off" alone."""
    import dataclasses
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, scene
    import bench
    sc = scene.cfg('cfg3')
    has = 'weight_motion' in {f.name for f in dataclasses.fields(fit.FitConfig)}
    fitters, targets = {}, None
    for name, kw in (("off", {}),) + ((("on", dict(weight_motion=1.0e4)),) if has else ()):
        cfg = dataclasses.replace(bench.workload_config('cfg3')[0], **kw)      # (the bench's own configuration of the workload)
        fitters[name] = fit.Fitter(sc, cfg, device='cuda', targets=targets)
        targets = fitters[name].targets                                          # (rendered once)
        for _ in range(5):
            fitters[name].step()
    torch.cuda.synchronize()
    turns = {name: [] for name in fitters}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < max(seconds, 1.0) * 6 or len(turns["off"]) < 5:
        for name, ft in fitters.items():
            torch.cuda.synchronize()
            a = time.perf_counter()
            for _ in range(steps):
                ft.step()
            torch.cuda.synchronize()
            turns[name].append((time.perf_counter() - a) / steps * 1e3)
        if time.perf_counter() - t0 > 120:
            break
    for name in fitters:
        t = np.sort(np.asarray(turns[name]))
        print(f"  cfg3 step, weight_motion {name:3s}: median {np.median(t):.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns of {steps} steps; "
              f"{sc.n_frames} frames, {sc.n_vertices} vertices)", flush=True)


def main(commit, seconds, step):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"commit {commit}; F = {F} meshes", flush=True)
    if step:
        return step_times(seconds)
    import fitstep_ref
    from fpc_diffrend_amd import scene
    base = torch.tensor(scene.cfg('cfg1', n_frames=3).v_base).reshape(-1, 3).float().clone()
    base[:, 1] += 170.0
    calls_at(int(base.shape[0]), base, seconds)
    _, V, pos = fitstep_ref.uv_sphere()
    pos = pos.clone().float()
    pos[:, 1] += 170.0
    calls_at(V, pos, seconds)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")), "--step" in sys.argv)

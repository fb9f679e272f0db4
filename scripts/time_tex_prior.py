"""HIP-event times of the texture prior (csrc/tex_prior.hip, k_tex_prior) at three textures -- 1024 x 1024 x 1 (the reference's), 2048 x
2048 x 3 and 4096 x 4096 x 1 --, the variants taking turns in one process:

  fpcdr_tex_prior                         value and gradient, an anchor and both maps: the kernel and the finish kernel
  fpcdr_tex_prior Charbonnier             the same with a scale (one square root and two divisions a pair)
  fpcdr_tex_prior value only              grad_tex = NULL
  fpcdr_tex_prior smoothness, no maps     no anchor, no maps: the texture read, the gradient written
  torch fwd + bwd                         tests/tex_prior_ref.tex_prior_plain in float32 and its autograd backward on the same tensors on
                                          the GPU: the yardstick
  torch Charbonnier fwd + bwd             the same through 2 c^2 (sqrt(1 + s / c^2) - 1)

Before timing, every call is held against torch's expression: the value, and the gradient's relative L2.

Algorithmic bytes of the full call: the texture, the anchor and the two maps read once, the gradient written once, (3 C + 2) * 4 bytes a
texel; that a texel is read by the threads of its four neighbours is cache traffic.  The floor is those bytes at FLOOR_TBS, the rate the
project's streaming kernels reach (the robust loss's, profiles/pixel_terms_ab.txt).

With --step: a cfg3 step (bench.py's flagship configuration) with both weights 0 and with the term on, taking turns, host clock around
`steps` steps that end in a synchronise.  A commit whose FitConfig has no such option (the parent) gets the "off" figure alone.

    python scripts/time_tex_prior.py [--commit NAME] [--seconds S] [--step]
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1024, 1024, 1), (2048, 2048, 3), (4096, 4096, 1)]
FLOOR_TBS = 4.7


def time_turns(variants, seconds, calls=10):
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
        print(f"  {name:40s} median {med[name]:9.2f} us a call (min {t[0]:.2f}, max {t[-1]:.2f}, {t.size} turns of {calls} calls)", flush=True)
    return med


def calls_at(Ht, Wt, C, seconds):
    import torch
    import tex_prior_ref as T
    from fpc_diffrend_amd import _lib, fit
    g = torch.Generator().manual_seed(0)
    y, x = torch.meshgrid(torch.arange(Ht, dtype=torch.float32), torch.arange(Wt, dtype=torch.float32), indexing='ij')
    t = (0.5 + 0.2 * torch.sin(0.03 * x) * torch.cos(0.02 * y))[..., None] + 0.02 * torch.randn(Ht, Wt, C, generator=g)
    t = t.clamp(0, 1).float().cuda().contiguous()
    a = (t * 0.9 + 0.03).contiguous()
    sw = (0.1 + 1.9 * torch.rand(Ht, Wt, generator=g)).cuda()
    aw = (0.1 + 1.9 * torch.rand(Ht, Wt, generator=g)).cuda()
    sw[Ht // 2], aw[:, Wt // 3] = 0.0, 0.0
    p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gt = torch.empty_like(t)
    acc = torch.zeros(2, dtype=torch.float64, device='cuda')
    part, out = torch.empty(2, dtype=torch.float32, device='cuda'), torch.empty((), dtype=torch.float32, device='cuda')
    ws, wa, c = 7.5, 2.25, 0.03
    inv_c = fit.tex_prior_inv_scale(c)

    def call(ic, grad=True, full=True):
        _lib.call("fpcdr_tex_prior", p(t), p(a) if full else None, p(sw) if full else None, p(aw) if full else None, ic, ws, wa,
                  p(gt) if grad else None, p(acc), p(part), p(out), Ht, Wt, C, st())

    leaf = t.clone().requires_grad_(True)

    def torch_run(scale, full=True):
        leaf.grad = None
        v = T.tex_prior_plain(leaf, ws, wa, a if full else None, sw if full else None, aw if full else None, scale)
        v.backward()
        return v

    # faster and different is not faster
    for ic, scale, full in ((0.0, None, True), (inv_c, c, True), (0.0, None, False)):
        call(ic, full=full)
        tv = float(torch_run(scale, full).detach())
        rel = float((gt - leaf.grad).norm() / leaf.grad.norm())
        print(f"  {Ht}x{Wt}x{C}{'' if scale is None else ' c = %g' % scale}{'' if full else ' smoothness alone'}: call {float(out):.6f} "
              f"torch {tv:.6f}, gradient rel-L2 against torch's {rel:.2e}", flush=True)
        assert abs(float(out) - tv) <= 1e-4 * abs(tv) and rel < 1e-4
    variants = [("fpcdr_tex_prior", lambda: call(0.0)),
                ("fpcdr_tex_prior Charbonnier", lambda: call(inv_c)),
                ("fpcdr_tex_prior value only", lambda: call(0.0, False)),
                ("fpcdr_tex_prior smoothness, no maps", lambda: call(0.0, True, False)),
                ("torch fwd + bwd", lambda: torch_run(None)),
                ("torch Charbonnier fwd + bwd", lambda: torch_run(c))]
    med = time_turns(variants, seconds)
    nbytes = (3 * C + 2) * 4.0 * Ht * Wt
    tk = med["fpcdr_tex_prior"]
    print(f"  {Ht}x{Wt}x{C}: fpcdr_tex_prior / torch: {tk / med['torch fwd + bwd']:.4f} (L2), "
          f"{med['fpcdr_tex_prior Charbonnier'] / med['torch Charbonnier fwd + bwd']:.4f} (Charbonnier); {nbytes / 1e6:.1f} MB algorithmic -> "
          f"{nbytes / (tk * 1e-6) / 1e12:.2f} TB/s; floor at {FLOOR_TBS} TB/s: {nbytes / (FLOOR_TBS * 1e12) * 1e6:.1f} us", flush=True)


def step_times(seconds, steps=20):
    """A cfg3 step with the term off and on, taking turns; a FitConfig without the option (the parent commit) times "off" alone."""
    import dataclasses
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, scene
    import bench
    sc = scene.cfg('cfg3')
    has = 'weight_tex_smooth' in {f.name for f in dataclasses.fields(fit.FitConfig)}
    on = dict(weight_tex_smooth=1.0e2, tex_smooth_scale=0.05, tex_smooth_weights='chart', weight_tex_anchor=1.0e2)
    fitters, targets = {}, None
    for name, kw in (("off", {}),) + ((("on", on),) if has else ()):
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
        print(f"  cfg3 step, texture prior {name:3s}: median {np.median(t):.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns of {steps} "
              f"steps; {sc.n_frames} frames, texture {tuple(sc.texture.shape)})", flush=True)


def main(commit, seconds, step):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"commit {commit}", flush=True)
    if step:
        return step_times(seconds)
    for Ht, Wt, C in SHAPES:
        calls_at(Ht, Wt, C, seconds)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")), "--step" in sys.argv)

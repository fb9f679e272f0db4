"""The fit step's host path, run to run and tree to tree: a script that is copied into two checkouts and imports the package of the tree
it lies in, one fresh process per run.

    python scripts/fit_terms_traj.py OUT.pt [--config NAME] [--graph] [--steps N] [--sync]
    python scripts/fit_terms_traj.py --compare A.pt B.pt [--spread A2.pt A3.pt ...]
    python scripts/fit_terms_traj.py --planes OUT.pt
    python scripts/fit_terms_traj.py --compare-planes A.pt B.pt
    python scripts/fit_terms_traj.py --time
    python scripts/fit_terms_traj.py --enqueue [priors | default]

The first form runs a smoke-sized Fitter for N (20) steps and saves the per-step losses and the final parameters.  --config shape (the
default): cfg1, 4 frames, cameras 0 and 3, seed 0, with laplacian_relative, weight_stretch and weight_bend on, eager or under the captured
HIP graph.  --config default | unfused | blur | norm | robust: the pixel terms, on two frames of 64 x 64 and cameras 0 and 4 (robust: with
masks and face weights); these also save the C-ABI calls of three steps by name and count (_lib.KernelTimer) and the device launches of
one step (the torch profiler).  --config robust1p | mip | compact: what the one-pass objective runs beyond default -- robust with
weighted_one_pass, enable_mip, and the default with ops.SMALL_BATCH_BINS = 0 and ops.RECORD_SLOT_MARGIN = 1, so that the count-only call and
compact records run at this small shape; --graph captures these and default too.  --sync waits for the device after every step and notes,
for every fpcdr_objective_fwd / fpcdr_objective_weighted_fwd call of the process, what the host path handed it (count_only, rec_slots, the
three caps, counts_seq, whether counts_out is set, the element counts of rec / color / grad_aa), the N steps' skip flags and the count of
skipped steps: --compare holds them equal item for item.  --config priors: the step's five prior terms together (rest Laplacian, stretch, bend, motion of order 2,
texture smoothness on the chart with a scale and a hold to an anchor, at the weights of tests/test_gpu_prior_terms.py) on four frames of
cfg1 at 128 x 128, cameras 0 and 3, eager or with --graph; it saves the calls and launches as well, and the log records of the
iterations 0 and 10.  The second form prints the largest relative difference of the losses and of the parameters (L2) between A
and B, beside the largest among A and further runs of A's tree (--spread), and fails if B is further from A than those runs are from each
other (the objective's float atomics make two runs of one tree differ), if the recorded calls or launches differ, or if the log
records differ in their keys or, by more than A's runs among themselves and 1e-6, in a value.

--planes saves the sums and the gradient planes of fit.pixel_loss_fused / _blurred / _normalised / _robust at one small shape each, with
and without n_total; --compare-planes holds the planes of B to torch.equal with A's and the float64 sums, which pass through atomics, to
1e-12 relative.  --time prints the median step time of the unfused, blur, norm and robust configurations at cfg3's shape.  --enqueue
prints the median host time to enqueue a step of the priors configuration at one image a step (frames_per_step 3, views_per_step 1), the
launch-bound shape, or (default) of the default one-pass step on cfg1 at frames_per_step 1, views_per_step 1: 200 steps after 3, no
synchronisation inside the loop."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIXEL_CONFIGS = {'default': {}, 'unfused': dict(fused_objective=False), 'blur': dict(blur_sigma=3.0, blur_kernel_size=15),
                 'norm': dict(norm_sigma=3.0, norm_kernel_size=15), 'robust': dict(robust='charbonnier', robust_scale=10.0, weight_outside=0.25),
                 'robust1p': dict(robust='charbonnier', robust_scale=10.0, weight_outside=0.25, weighted_one_pass=True),
                 'mip': dict(enable_mip=True), 'compact': {}}
OBJECTIVE_CALLS = ('fpcdr_objective_fwd', 'fpcdr_objective_weighted_fwd')

PRIORS = dict(laplacian_relative=True, weight_laplacian=1.0e8, weight_stretch=2.5e7, weight_bend=1.0e9, weight_motion=6.0e6, motion_order=2,
              weight_tex_smooth=3.0e4, tex_smooth_scale=0.1, tex_smooth_weights='chart', weight_tex_anchor=1.0e5)


def _priors_fitter(**kw):
    """A Fitter with the five prior terms on (PRIORS) on four frames of cfg1, and an anchor that differs from the start texture."""
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg1', n_frames=4)
    sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
    cfg = fit.FitConfig(cam_idxs=(0, 3), resolution=(128, 128), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, seed=0, **PRIORS, **kw)
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.8)
    ft.set_texture_anchor((ft.tex_opt.detach() * 0.9 + 0.03).contiguous())
    return ft


def _pixel_fitter(name, sc, **kw):
    """A Fitter of PIXEL_CONFIGS[name] on the scene; 'robust' gets seeded masks and face weights."""
    import dataclasses
    import numpy as np
    from fpc_diffrend_amd import fit
    kw = dict(PIXEL_CONFIGS[name], **kw)
    if name == 'compact':      # the count-only call and compact records at this small shape, as tests/test_gpu_skip.py has them
        from fpc_diffrend_amd import ops
        ops.SMALL_BATCH_BINS, ops.RECORD_SLOT_MARGIN = 0, 1
    if name in ('robust', 'robust1p'):
        rng = np.random.default_rng(3)
        sc = dataclasses.replace(sc, masks=rng.integers(0, 256, size=(sc.n_frames, len(sc.cams)) + tuple(sc.resolution), dtype=np.uint8))
        kw['face_weights'] = rng.uniform(0.0, 1.5, size=sc.pos_idx.shape[0]).astype(np.float32)
    ft = fit.Fitter(sc, fit.FitConfig(**kw), device='cuda')
    ft.init_near_truth(0.8)
    return ft


def _note_objective_calls(calls):
    """Append to `calls` what every one-pass objective call of this process is handed by its host path: the launch caps, the counters'
    hand-over, count_only, rec_slots and the element counts of the record pool's three tensors.  Wraps _lib.call and torch.empty in THIS
    process (the package has no hook for it, and the parent's has none either): the pool's tensors are found again by their pointers."""
    import torch
    from fpc_diffrend_amd import _lib
    sizes, call, empty = {}, _lib.call, torch.empty

    def noting_empty(*args, **kw):
        t = empty(*args, **kw)
        if t.is_cuda:
            sizes[t.data_ptr()] = t.numel()
        return t

    def noting_call(name, *args, **kw):
        if name in OBJECTIVE_CALLS:
            p = args[0]._obj      # (ctypes.byref(struct))
            p = getattr(p, 'base', p)
            calls.append(dict(name=name, count_only=p.count_only, rec_slots=p.rec_slots, cap_bins=p.cap_bins, cap_occ=p.cap_occ, cap_def=p.cap_def,
                              counts_seq=p.counts_seq, counts_out=bool(p.counts_out), rec=sizes.get(p.rec), color=sizes.get(p.color),
                              grad_aa=sizes.get(p.grad_aa)))
            sizes.clear()
        return call(name, *args, **kw)

    _lib.call, torch.empty = noting_call, noting_empty


def run(out, config, graph, steps, sync=False):
    sys.path.insert(0, ROOT)
    import torch
    from fpc_diffrend_amd import _lib, fit, scene
    assert torch.cuda.is_available(), "needs the GPU"
    rec = {}
    if sync:      # what the host path decides for every objective call of this process, the first call on the shape included
        rec['decisions'], rec['skip_out'] = [], []
        _note_objective_calls(rec['decisions'])
    if config == 'shape':
        sc = scene.cfg('cfg1', n_frames=4)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=steps, cam_idxs=(0, 3), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, hip_graph=graph, seed=0,
                            weight_laplacian=20.0, laplacian_relative=True, weight_stretch=2.0e3, weight_bend=2.0e4)
        ft = fit.Fitter(sc, cfg, device='cuda')
        ft.init_near_truth(0.8)
    else:
        if config == 'priors':
            make = lambda **kw: _priors_fitter(max_iter=steps, hip_graph=graph, **kw)
        else:
            sc = scene.make_scene(resolution=(64, 64), n_frames=2)
            make = lambda **kw: _pixel_fitter(config, sc, max_iter=steps, cam_idxs=(0, 4), seed=0, **(dict(hip_graph=True) if graph else {}), **kw)
        ft = make()
        assert fit.Fitter.GRAPH_WARMUP == 3      # (--graph: the three timed steps are the eager ones in front of the capture)
        _lib.TIMER = _lib.KernelTimer()
        try:
            for _ in range(3):
                ft.step()
                if sync:
                    torch.cuda.synchronize()
            rec['calls'] = {k: n for k, (n, _) in _lib.TIMER.summary().items()}
        finally:
            _lib.TIMER = None
        if graph:
            ft.step()      # (the capture: the step profiled below is a replay)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            ft.step()
            torch.cuda.synchronize()
        rec['launches'] = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
        ft = make(**(dict(log_interval=10, reg_log_interval=10, log_path=out + ".log") if config == 'priors' else {}))
    losses = []
    for _ in range(steps):
        losses.append(float(ft.step()))
        if sync:
            torch.cuda.synchronize()      # (nothing is left to timing: poll() sees every call that was enqueued)
            rec['skip_out'].append(None if getattr(ft, '_skip_cur', None) is None else float(ft._skip_cur.reshape(-1)[0]))
    torch.cuda.synchronize()
    rec['skipped_steps'] = ft.skipped_steps
    if config == 'priors':
        import json
        rec['log'] = [json.loads(line) for line in open(out + ".log")]
        os.remove(out + ".log")
    torch.save(dict(rec, losses=losses, params=[p.detach().cpu() for p in ft.params]), out)
    print(f"{os.path.dirname(fit.__file__)}: config={config} graph={graph}, {steps} steps, loss {losses[0]:.6e} -> {losses[-1]:.6e}, "
          f"calls {rec.get('calls')}, launches of a step {rec.get('launches')}, {len(rec.get('decisions', []))} objective calls noted, "
          f"skipped steps {rec['skipped_steps']} -> {out}")


def compare(a_path, b_path, spread_paths):
    import torch

    def dist(x, y):
        dl = max(abs(p - q) / abs(p) for p, q in zip(x['losses'], y['losses']))
        dp = max(float((p.double() - q.double()).norm() / max(float(p.double().norm()), 1e-30)) for p, q in zip(x['params'], y['params']))
        return dl, dp

    import itertools
    a, b = torch.load(a_path), torch.load(b_path)
    dl, dp = dist(a, b)
    line = f"{a_path} vs {b_path}: losses {dl:.3e}, parameters {dp:.3e}"
    ok = True
    if spread_paths:
        runs = [a] + [torch.load(path) for path in spread_paths]
        pairs = [dist(x, y) for x, y in itertools.combinations(runs, 2)]
        sl, sp = max(p[0] for p in pairs), max(p[1] for p in pairs)
        line += f"; among {len(runs)} runs of A's tree: losses {sl:.3e}, parameters {sp:.3e}"
        ok = dl <= sl and dp <= sp
    if 'calls' in a:
        same = a['calls'] == b.get('calls') and a['launches'] == b.get('launches')
        line += f"; C-ABI calls of three steps {sum(a['calls'].values())} in {len(a['calls'])} names, launches of a step {a['launches']}: " + \
            ("the same" if same else f"DIFFERENT ({b.get('calls')}, {b.get('launches')})")
        ok = ok and same
    if 'decisions' in a:      # (--sync runs) item for item; the skip flags and the count of skipped steps are integers
        da, db = a['decisions'], b.get('decisions', [])
        first = next((i for i, (x, y) in enumerate(zip(da, db)) if x != y), None if len(da) == len(db) else min(len(da), len(db)))
        same = first is None and a['skip_out'] == b.get('skip_out') and a['skipped_steps'] == b.get('skipped_steps')
        n = lambda key, value: sum(1 for d in da if d[key] == value)
        line += f"; {len(da)} objective calls ({n('count_only', 1)} count-only, {sum(1 for d in da if d['rec_slots'] > 0)} compact, " \
                f"{n('counts_out', True)} reporting), skip flags set {sum(1 for v in a['skip_out'] if v)}, skipped steps {a['skipped_steps']}: " + \
                ("the same" if same else f"DIFFERENT (first at call {first}: {da[first] if first is not None and first < len(da) else None} / "
                                         f"{db[first] if first is not None and first < len(db) else None}; {b.get('skip_out')}, {b.get('skipped_steps')})")
        ok = ok and same
    if 'log' in a:
        timing = ("frames_per_s",)
        gap = lambda x, y: max((abs(r[k] - s[k]) / max(abs(r[k]), 1e-30) for r, s in zip(x['log'], y['log']) for k in r
                                if k not in timing and not isinstance(r[k], list)), default=0.0)
        keys = [list(r) for r in a['log']] == [list(r) for r in b['log']]
        dv, sv = gap(a, b), max([gap(a, x) for x in runs[1:]] if spread_paths else [0.0])
        line += f"; {len(a['log'])} log records, keys {'the same' if keys else 'DIFFERENT'} ({' '.join(a['log'][0])}), values differ by " \
                f"{dv:.3e} (A's runs: {sv:.3e})"
        ok = ok and keys and dv <= max(sv, 1e-6)
    print(line + ("" if ok else "   OUTSIDE"))
    return 0 if ok else 1


def planes(out):
    """The four pixel-loss wrappers of fit.py on seeded tensors, one small shape each with a ragged tail, with and without n_total."""
    sys.path.insert(0, ROOT)
    import torch
    from fpc_diffrend_amd import fit, ops
    g = torch.Generator().manual_seed(0)
    T = 40
    taps = ops.gaussian_taps(7, 1.5)
    calls = {'fused': ((1, 5, 67, 3), lambda t, n: fit.pixel_loss_fused(*t[:3], n)),
             'blurred': ((2, 37, 70, 1), lambda t, n: fit.pixel_loss_blurred(*t[:3], taps, n)),
             'normalised': ((1, 33, 65, 3), lambda t, n: fit.pixel_loss_normalised(*t[:3], taps, 1.5, n)),
             'robust': ((2, 19, 131, 1), lambda t, n: fit.pixel_loss_robust(*t[:3], 'geman_mcclure', 12.0, n, mask=t[3], face_weights=t[4],
                                                                           weight_outside=0.5, saturation=130))}
    rec = {}
    for name, ((B, H, W, C), call) in calls.items():
        colour = torch.rand(B, H, W, C, generator=g).cuda()
        rast = torch.zeros(B, H, W, 4)
        rast[..., 3] = torch.randint(1, T + 1, (B, H, W), generator=g).float() * (torch.rand(B, H, W, generator=g) > 0.4)
        ref = torch.randint(0, 141, (B, H, W), generator=g, dtype=torch.uint8).cuda()
        mask = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8).cuda()
        t = (colour, rast.cuda(), ref, mask, (torch.rand(T, generator=g) * 1.5).cuda())
        for n in (None, 3 * colour.numel() + 1):
            sums, grad = call(t, n)
            rec[f"{name} n_total={n}"] = (sums.cpu(), grad.cpu())
    torch.save(rec, out)
    print(f"{os.path.dirname(fit.__file__)}: {len(rec)} (sums, gradient plane) pairs -> {out}")


def compare_planes(a_path, b_path):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert list(a) == list(b)
    bad = 0
    for key in a:
        (sa, ga), (sb, gb) = a[key], b[key]
        ds = float(((sa - sb).abs() / sa.abs()).max())
        ok = torch.equal(ga, gb) and float(ga.abs().max()) > 0 and ds <= 1e-12
        bad += not ok
        print(f"{key:34s} gradient plane {tuple(ga.shape)} torch.equal: {torch.equal(ga, gb)}; sums differ by {ds:.1e} relative{'' if ok else '   FAIL'}")
    return 1 if bad else 0


def step_times(steps=8):
    """Milliseconds of a whole Fitter step at cfg3's shape per pixel-term configuration: host clock around step() + synchronise, the
    median of `steps` after 3 warm-up steps."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg3')
    for name in ('unfused', 'blur', 'norm', 'robust'):
        ft = _pixel_fitter(name, sc)
        for _ in range(3):
            ft.step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            ft.step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"STEP_MS {name} {float(np.median(ts)):.3f}   ({os.path.dirname(fit.__file__)})", flush=True)
        del ft
        torch.cuda.empty_cache()


def enqueue_time(config='priors', steps=200):
    """Milliseconds of host time to enqueue one step at one image a step: the median over `steps` steps.  config priors: the priors
    configuration, three frames and one view a step; default: the default one-pass step on cfg1, one frame and one view a step."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, scene
    if config == 'priors':
        ft = _priors_fitter(max_iter=80000, frames_per_step=3, views_per_step=1)
    else:
        assert config == 'default', config
        ft = fit.Fitter(scene.cfg('cfg1', n_frames=4), fit.FitConfig(max_iter=80000, frames_per_step=1, views_per_step=1, seed=0), device='cuda')
        ft.init_near_truth(0.8)
    for _ in range(3):
        ft.step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        ft.step()
        ts.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    print(f"ENQUEUE_MS {config} {float(np.median(ts)):.4f}   (min {min(ts):.4f}, {steps} steps; {os.path.dirname(fit.__file__)})", flush=True)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index("--spread") + 1:] if "--spread" in sys.argv else []))
    if sys.argv[1] == "--compare-planes":
        sys.exit(compare_planes(sys.argv[2], sys.argv[3]))
    if sys.argv[1] == "--planes":
        planes(sys.argv[2])
    elif sys.argv[1] == "--time":
        step_times()
    elif sys.argv[1] == "--enqueue":
        enqueue_time(sys.argv[2] if len(sys.argv) > 2 else 'priors')
    else:
        run(sys.argv[1], arg("--config", "shape"), "--graph" in sys.argv, int(arg("--steps", "20")), "--sync" in sys.argv)

"""HIP-event times of the resolution pyramid (csrc/downsample.hip, DESIGN.md 3 "Downsample rule") -> profiles/pyramid_time.txt:
fpcdr_downsample_u8 at s = 2, 4, 8 on the cfg3 batch (288 images of 1080 x 1920 from scene.cfg('cfg3')) and on one image of 1600 x 1200
(scene.cfg('ref'), one frame, one camera), with the bytes it moves per second (every source byte read once, every output byte written
once), beside the yardstick: the same result through torch -- avg_pool2d on a float copy, the conversions to float and back to 8 bit
included --, in the same process, the variants taking turns.  For s = 2, 4, 8 the float path is exact, and the two results are compared
with torch.equal first.  The cfg3 case then times a whole Fitter.step() at factors 1 (the default path of the same build), 2 and 4 with
pyramid_mip on, three Fitters on the same targets taking turns: a turn is STEPS_PER_TURN steps enqueued back to back between two events,
as a fit runs them (one step between two synchronisations shows the host's ~3 ms of enqueueing, not the kernels).  Steady state: every
variant is warmed up first; medians with minimum and maximum.  No speed is a pass condition.

    python scripts/time_pyramid.py [--out FILE]      every case in a process of its own, each under `timeout`; stops at the first failure
    python scripts/time_pyramid.py --case cfg3       one case in this process (cfg3 | single)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"cfg3": ("cfg3", 32, tuple(range(9))), "single": ("ref", 1, (0,))}
LIMIT = {"cfg3": 540, "single": 240}      # seconds a case may take (cfg3: 288 reference images are rendered first)
FACTORS = (2, 4, 8)
STEPS_PER_TURN = 10


def launcher(out_path):
    text = []
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(LIMIT[case]), sys.executable, os.path.abspath(__file__), "--case", case]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        text.append(p.stdout)
        if p.returncode != 0:
            print(f"case {case}: exit status {p.returncode}; stopping", flush=True)
            return p.returncode
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("".join(text))
    return 0


def take_turns(variants, seconds, cap):
    """Every variant in turn, each call between two HIP events, until each has `seconds` of timed calls (at least 30 turns, at most
    `cap` seconds of wall time).  Returns {name: sorted times in ms}."""
    import numpy as np
    import torch
    turns = {name: [] for name, _ in variants}
    t0 = time.perf_counter()
    while len(turns[variants[0][0]]) < 30 or min(sum(v) for v in turns.values()) < seconds * 1e3:
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            turns[name].append(e0.elapsed_time(e1))
        if time.perf_counter() - t0 > cap and len(turns[variants[0][0]]) >= 30:
            break
    return {name: np.sort(np.asarray(t)) for name, t in turns.items()}


def run(case, seconds=1.0):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import torch.nn.functional as F
    from fpc_diffrend_amd import fit, ops as dr, scene
    assert torch.cuda.is_available(), "needs the GPU"
    name, n_frames, cams = CASES[case]
    sc = scene.cfg(name, n_frames=n_frames)
    kw = dict(max_iter=80000, cam_idxs=cams)
    ft = fit.Fitter(sc, fit.FitConfig(**kw), device="cuda")
    H, W = ft.resolution
    src = ft.targets.reshape(-1, H, W)
    N = src.shape[0]
    px = N * H * W
    outs = {s: torch.empty(N, H // s, W // s, dtype=torch.uint8, device="cuda") for s in FACTORS}

    def kernel(s):
        def fn():
            dr._lib.call("fpcdr_downsample_u8", dr._ptr(src), dr._ptr(outs[s]), N, H, W, s, dr._stream())
        return fn

    def yardstick(s):
        def fn():
            return torch.floor(F.avg_pool2d(src[:, None].to(torch.float32), s) + 0.5).to(torch.uint8)[:, 0]
        return fn

    variants = []
    for s in FACTORS:
        variants += [(f"fpcdr_downsample_u8, s = {s}", kernel(s)), (f"avg_pool2d on a float copy, s = {s} (yardstick)", yardstick(s))]
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for s in FACTORS:      # faster and different is not faster
        kernel(s)()
        assert torch.equal(outs[s], yardstick(s)()), s
    print(f"{case}: {N} x {H} x {W} ({px / 1e6:.1f} Mpx) uint8; the kernel's result equals the yardstick's at s = 2, 4, 8 (torch.equal)", flush=True)
    turns = take_turns(variants, seconds, cap=40)
    med = {}
    for vname, _ in variants:
        t = turns[vname]
        med[vname] = float(np.median(t))
        extra = ""
        if vname.startswith("fpcdr_downsample_u8"):
            s = int(vname.rsplit("=", 1)[1])
            moved = px * (1.0 + 1.0 / (s * s))
            extra = f"  {moved / 1e6:.1f} MB = {moved / (med[vname] * 1e-3) / 1e12:.2f} TB/s"
        print(f"  {vname:48s} median {med[vname]:.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns){extra}", flush=True)
    for s in FACTORS:
        a, b = f"fpcdr_downsample_u8, s = {s}", f"avg_pool2d on a float copy, s = {s} (yardstick)"
        print(f"  s = {s}: {med[b] / med[a]:.2f} x the speed of the yardstick", flush=True)
    if case != "cfg3":
        return
    # ---- a whole step at factors 1, 2, 4: three Fitters on the same targets, the same start ----
    del outs
    fitters = {1: ft}
    for s in (2, 4):
        fitters[s] = fit.Fitter(sc, fit.FitConfig(pyramid=((s, 10 ** 9),), pyramid_mip=True, **kw), device="cuda", targets=ft.targets)
    for f in fitters.values():
        f.init_near_truth(0.8)

    def ten(f):
        def fn():
            for _ in range(STEPS_PER_TURN):
                f.step()
        return fn

    steps = [(f"Fitter.step(), factor {s}" + (" (default path)" if s == 1 else ", pyramid_mip"), ten(f)) for s, f in fitters.items()]
    for _, fn in steps:
        fn()
    torch.cuda.synchronize()
    turns = take_turns(steps, seconds, cap=40)
    base = None
    for vname, _ in steps:
        t = turns[vname] / STEPS_PER_TURN
        m = float(np.median(t))
        base = m if base is None else base
        print(f"  {vname:48s} median {m:.4f} ms a step (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns of {STEPS_PER_TURN} steps)  "
              f"{m / base:.2f} x the factor-1 step", flush=True)
    assert all(f.skipped_steps == 0 for f in fitters.values())


if __name__ == "__main__":
    if "--case" in sys.argv:
        run(sys.argv[sys.argv.index("--case") + 1])
    else:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "pyramid_time.txt")
        sys.exit(launcher(out))

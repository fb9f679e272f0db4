"""What the weighted one-pass objective (FitConfig.weighted_one_pass; DESIGN.md 3, "Weighted objective rule") buys: milliseconds of a
whole Fitter step at cfg3's shape (32 frames x 9 cameras of 1080 x 1920, 30 k triangles) for three weighted configurations -- a mask
only (kind 'l2'), Charbonnier c = 10 with a mask, Charbonnier with a mask and face weights -- each on the operator path and on the
weighted one-pass call, beside the plain one-pass step, ALL IN ONE PROCESS, the variants taking turns: host clock around step() +
synchronise, median after warm-up rounds.  Before timing, the weighted one-pass step's loss is held against its operator-path step's on
the same state (1e-5 relative): faster and different is not faster.

  --parent DIR   also the plain one-pass step of another build of the package (the parent commit's, exported and built under DIR), in a
                 process of its own
  --bench        instead: bench.py --gpus 1 --steps 50 --warmup 5 of this build and of --parent DIR, three runs each, taking turns

    python scripts/weighted_objective_time.py [--commit NAME] [--rounds N] [--parent DIR] [--bench]
"""
import dataclasses
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 10.0


def _time_turns(fitters, rounds, warmup=3):
    """name -> sorted milliseconds per step: every Fitter one step a round, the rounds after `warmup` counted."""
    import numpy as np
    import torch
    ts = {name: [] for name, _ in fitters}
    for r in range(warmup + rounds):
        for name, ft in fitters:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ft.step()
            torch.cuda.synchronize()
            if r >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    return {k: np.sort(np.asarray(v)) for k, v in ts.items()}


def plain_only(rounds):
    """The child of --parent: the plain one-pass step of the package on sys.path."""
    import numpy as np
    from fpc_diffrend_amd import fit, scene
    ft = fit.Fitter(scene.cfg('cfg3'), fit.FitConfig(), device='cuda')
    ft.init_near_truth(0.8)
    t = _time_turns([("plain", ft)], rounds)["plain"]
    print(f"PLAIN_STEP {float(np.median(t)):.3f} {t[0]:.3f} {t[-1]:.3f}", flush=True)


def _child(parent, args, timeout=900):
    env = dict(os.environ, PYTHONPATH=os.path.abspath(parent))
    env.pop("FPCDR_LIB_PATH", None)
    return subprocess.run([sys.executable] + args, env=env, cwd=os.path.abspath(parent), check=True, stdout=subprocess.PIPE,
                          timeout=timeout).stdout.decode()


def main(commit, rounds, parent):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, scene
    assert torch.cuda.is_available(), "needs the GPU"
    sc = scene.cfg('cfg3')
    rng = np.random.default_rng(0)
    shape = (sc.n_frames, len(sc.cams)) + tuple(sc.resolution)
    # a mask as a matting network leaves it: 8 x 8 blocks of one value, a tenth of them 0, half of them 255
    blocks = rng.integers(0, 256, size=shape[:2] + (shape[2] // 8, shape[3] // 8), dtype=np.uint8)
    pick = rng.uniform(size=blocks.shape)
    blocks[pick < 0.1] = 0
    blocks[pick > 0.5] = 255
    masked = dataclasses.replace(sc, masks=np.ascontiguousarray(blocks.repeat(8, axis=2).repeat(8, axis=3)))
    face_w = rng.uniform(0.0, 1.5, size=sc.pos_idx.shape[0]).astype(np.float32)
    face_w[rng.uniform(size=face_w.shape[0]) < 0.2] = 0.0
    configs = [("mask only (kind l2)", {}), ("Charbonnier c=10 + mask", dict(robust='charbonnier', robust_scale=SCALE)),
               ("Charbonnier c=10 + mask + face weights", dict(robust='charbonnier', robust_scale=SCALE, face_weights=face_w))]

    def make(s, **kw):
        ft = fit.Fitter(s, fit.FitConfig(**kw), device='cuda')
        ft.init_near_truth(0.8)
        return ft

    print(f"commit {commit}; a whole Fitter step at cfg3's shape (32 frames x 9 cameras x 1080 x 1920, 30 k triangles), host clock around "
          f"step() + synchronise, one process, the variants taking turns, median of {rounds} rounds after 3 warm-up rounds:", flush=True)
    fitters = [("plain one-pass objective (default, no weights)", make(sc))]
    for name, kw in configs:
        op, wo = make(masked, **kw), make(masked, weighted_one_pass=True, **kw)
        fr = slice(0, sc.n_frames)
        a, b = float(op.loss_and_backward(fr)), float(wo.loss_and_backward(fr))
        gop, gwo = [p.grad for p in op.params if p.grad is not None], [p.grad for p in wo.params if p.grad is not None]
        rel = max(float((x - y).norm() / y.norm()) for x, y in zip(gwo, gop) if float(y.norm()) > 0)
        print(f"  {name}: loss {b:.6f} on the weighted one-pass call, {a:.6f} on the operator path; parameter gradients rel-L2 at most {rel:.2e}; "
              f"wsum {float(wo._wsum):.1f} / {float(op._wsum):.1f}", flush=True)
        assert abs(a - b) <= 1e-5 * abs(a) and rel < 1e-4
        fitters += [(f"{name}: operator path", op), (f"{name}: weighted one-pass", wo)]
    ts = _time_turns(fitters, rounds)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    for name, _ in fitters:
        print(f"  {med[name]:8.3f} ms (min {ts[name][0]:.3f}, max {ts[name][-1]:.3f})  {name}", flush=True)
    plain = med[fitters[0][0]]
    for name, _ in configs:
        o, w = med[f"{name}: operator path"], med[f"{name}: weighted one-pass"]
        print(f"  {name}: weighted one-pass {w:.3f} ms = operator path / {o / w:.2f} = plain one-pass x {w / plain:.3f}"
              f"{'' if w < o else '   NOT FASTER THAN ITS OPERATOR PATH'}", flush=True)
    if parent:
        out = _child(parent, [os.path.abspath(__file__), "--plain-only", "--rounds", str(rounds)])
        m, lo, hi = (float(v) for v in out.split("PLAIN_STEP")[1].split()[:3])
        print(f"  {m:8.3f} ms (min {lo:.3f}, max {hi:.3f})  plain one-pass objective, the parent build (a process of its own)", flush=True)


def bench(commit, parent):
    """bench.py's frames/s on the default path, this build and the parent build taking turns, three runs each."""
    runs = {"this build": [], "parent build": []}
    for _ in range(3):
        for name, root in (("this build", ROOT), ("parent build", os.path.abspath(parent))):
            out = _child(root, [os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5"])
            line = [l for l in out.splitlines() if l.startswith("{")][-1]
            runs[name].append(float(json.loads(line)["value"]))
            print(f"BENCH {name} {runs[name][-1]:.1f}", flush=True)
    print(f"commit {commit}; bench.py --gpus 1 --steps 50 --warmup 5 (cfg3, the default one-pass path), this build and the parent build taking "
          "turns, frames/s:")
    for name, v in runs.items():
        print(f"  {name:12s} " + " ".join(f"{x:.1f}" for x in v))
    a, b = runs["this build"], runs["parent build"]
    print(f"  the ranges {'overlap' if max(a) >= min(b) and max(b) >= min(a) else 'DO NOT OVERLAP'}")


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    n = int(arg("--rounds", "8"))
    if "--plain-only" in sys.argv:
        plain_only(n)
    elif "--bench" in sys.argv:
        bench(arg("--commit", "(not named)"), arg("--parent", ""))
    else:
        main(arg("--commit", "(not named)"), n, arg("--parent", ""))

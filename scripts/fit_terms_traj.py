"""The fit step's host path with all three shape terms on, run to run and tree to tree.

    python scripts/fit_terms_traj.py OUT.pt [--graph] [--steps N]       one fresh process per run; imports the package of the tree it lies in
    python scripts/fit_terms_traj.py --compare A.pt B.pt [--spread A2.pt A3.pt ...]

The first form runs a smoke-sized Fitter (cfg1, 4 frames, cameras 0 and 3, seed 0) with laplacian_relative, weight_stretch and weight_bend
on for N (20) steps, eager or under the captured HIP graph, and saves the per-step losses and the final parameters.  The second form
prints the largest relative difference of the losses and of the parameters (L2) between A and B, beside the largest among A and further
runs of A's tree (--spread), and fails if B is further from A than those runs are from each other (the objective's float atomics make
two runs of one tree differ)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(out, graph, steps):
    sys.path.insert(0, ROOT)
    import torch
    from fpc_diffrend_amd import fit, scene
    assert torch.cuda.is_available(), "needs the GPU"
    sc = scene.cfg('cfg1', n_frames=4)
    sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
    cfg = fit.FitConfig(max_iter=steps, cam_idxs=(0, 3), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, hip_graph=graph, seed=0,
                        weight_laplacian=20.0, laplacian_relative=True, weight_stretch=2.0e3, weight_bend=2.0e4)
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.8)
    losses = [float(ft.step()) for _ in range(steps)]
    torch.cuda.synchronize()
    torch.save({'losses': losses, 'params': [p.detach().cpu() for p in ft.params]}, out)
    print(f"{os.path.dirname(fit.__file__)}: graph={graph}, {steps} steps, loss {losses[0]:.6e} -> {losses[-1]:.6e} -> {out}")


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
    print(line + ("" if ok else "   OUTSIDE"))
    return 0 if ok else 1


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index("--spread") + 1:] if "--spread" in sys.argv else []))
    run(sys.argv[1], "--graph" in sys.argv, int(arg("--steps", "20")))

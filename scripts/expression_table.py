"""The README's expression table: float64 on the CPU (tests/expr_ref.py, the statement of DESIGN.md 3, "Expression solve rule").

The 1K mesh (514 vertices) at 256 x 256 with Kb Gaussian-bump blendshapes (scene.make_blendshapes), the pose at the truth, seeded dense
truth weights in [-3, 5], the start at neutral.  Landmarks on every thirteenth vertex (L = 40) or every fourth (L = 129), cameras 0 and 4
(Nc = 2) or all nine.  Rows: a well-determined case (Kb = 10 and 24 against 160 equations), a large one that the data still determine
(Kb = 150, L = 129, Nc = 9) and an under-determined one (Kb = 150 against 160 equations of rank at most 120: 40 points x 3
coordinates); each without and with a ridge, without and with one pixel of detection noise.  Columns: the mean reprojection error and
the largest vertex error against the truth mesh, before -> after 20 trials (weights kept in float64, to show what the iteration
reaches; the rule rounds them to float32).  ONE scene: what landmarks determine and what they do not, not a promise about real takes.

    python scripts/expression_table.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (256, 256)
RIDGE = 0.01
TRIALS = 20
CASES = [(10, 13, (0, 4)), (24, 13, (0, 4)), (150, 4, tuple(range(9))), (150, 13, (0, 4))]      # (Kb, every n-th vertex, cameras)


def rows():
    """[(Kb, L, Nc, ridge, noise px, residual before, after, vertex error before, after)]."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import expr_ref as ER
    import landmark_ref as LR
    from helpers import scene_mvps
    from fpc_diffrend_amd import scene
    out = []
    for Kb, every, cams in CASES:
        sc = scene.make_scene(scene.MESH_1K, Kb, 1, RES, (256, 256, 1), 0)
        H, W = RES
        V = sc.n_vertices
        points = [{'vertex': v} for v in range(0, V, every)]
        L, Nc = len(points), len(cams)
        vtx, bary, _ = LR.tables(points, V, sc.pos_idx)
        sc.q_gt[0], sc.t_gt[0] = (0.0, 0.0, 0.0, 1.0), 0.0
        mvp = scene_mvps(sc, cams, [0]).double()
        B = torch.tensor(sc.blendshapes).double()
        g = torch.Generator().manual_seed(100 + Kb)
        w_true = 8.0 * torch.rand(1, Kb, generator=g, dtype=torch.float64) - 3.0
        base = torch.tensor(sc.v_base).double().reshape(1, -1)
        x0, x_true = base.reshape(1, V, 3), (base + w_true @ B.t()).reshape(1, V, 3)
        w0 = torch.zeros(1, Kb, dtype=torch.float64)
        clean = torch.zeros(Nc, L, 3, dtype=torch.float64)
        clean[..., 2] = 1.0
        at = ER.normal(x_true, mvp, B, vtx, bary, None, clean, w0, w0, H, W)
        assert bool(at['live'].all())
        clean[..., :2] = at['res'][0]
        jitter = torch.randn(Nc, L, 2, generator=g, dtype=torch.float64)
        for noise in (0.0, 1.0):
            obs = clean.clone()
            obs[..., :2] += noise * jitter
            a = (x0, mvp, B, vtx, bary, None, obs)
            for ridge in (0.0, RIDGE):
                w, info, _ = ER.solve(*a, w0, H, W, ridge=ridge, iters=TRIALS, round32=False)
                x = (base + w.double() @ B.t()).reshape(1, V, 3)
                out.append((Kb, L, Nc, ridge, noise, ER.mean_residual(*a, w0, w0, H, W), ER.mean_residual(*a, w, w0, H, W),
                            float((x0 - x_true).abs().max()), float((x - x_true).abs().max())))
    return out


def fmt(v):
    return f"{v:.2f}" if v >= 0.01 else f"{v:.1e}"


if __name__ == "__main__":
    print("| Kb | L | Nc | ridge | noise, px | mean residual, px | max vertex error, units |")
    print("|---|---|---|---|---|---|---|")
    for Kb, L, Nc, ridge, noise, r0, r1, e0, e1 in rows():
        print(f"| {Kb} | {L} | {Nc} | {ridge:g} | {noise:g} | {fmt(r0)} → {fmt(r1)} | {fmt(e0)} → {fmt(e1)} |", flush=True)

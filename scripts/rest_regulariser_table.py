"""The table of README.md ("Regularising against the base mesh"): what the reference's shape terms measure on the cfg1 mesh at the base
mesh and on its ground-truth frames, and what the same terms measure against the base mesh's own differentials, edge lengths and dihedral angles.
float64 on the CPU, with the statements the tests use (tests/fitstep_ref.py, tests/rest_ref.py, tests/bend_ref.py); needs no GPU.

    python scripts/rest_regulariser_table.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT = 5000.0          # FitConfig.weight_laplacian's default
N_FRAMES = 3


def bend_rows():
    """The bending rows of the table as numbers: the plain normal-consistency term (no rest table) and the Bend rule against the base
    mesh's own angles, per unit weight, on the cfg1 base mesh and its ground-truth frames."""
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import math
    import torch
    import bend_ref as B
    from fpc_diffrend_amd import scene
    sc = scene.cfg('cfg1', n_frames=N_FRAMES)
    V = sc.n_vertices
    base = torch.tensor(sc.v_base, dtype=torch.float64).reshape(1, V, 3)
    truth = (base.reshape(1, -1) + torch.tensor(sc.weights_gt[:N_FRAMES], dtype=torch.float64)
             @ torch.tensor(sc.blendshapes, dtype=torch.float64).t()).reshape(N_FRAMES, V, 3)
    hv, sigma = B.hinges(sc.pos_idx)
    cs = B.rest_cs(base, hv, sigma)
    plain = B.bend(base, hv, sigma, None, 1.0)
    c, s, _, _ = B.angles(base, hv, sigma)
    theta = torch.atan2(s.v, c.v).abs() * (180.0 / math.pi)
    return {'vertices': V, 'hinges': int(hv.shape[0]), 'inconsistent': int((sigma < 0).sum()),
            'plain_base': float(plain['value'][0]), 'plain_grad_max': float(plain['grad'][0].abs().max()),
            'plain_grad_rms': float((plain['grad'][0] ** 2).mean().sqrt()),
            'angle_mean_deg': float(theta.mean()), 'angle_max_deg': float(theta.max()),
            'plain_truth': [float(B.bend(truth[i:i + 1], hv, sigma, None, 1.0)['value'][0]) for i in range(N_FRAMES)],
            'rest_truth': [float(B.bend(truth[i:i + 1], hv, sigma, cs, 1.0)['value'][0]) for i in range(N_FRAMES)]}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import fitstep_ref as R
    import rest_ref as S
    from fpc_diffrend_amd import scene
    sc = scene.cfg('cfg1', n_frames=N_FRAMES)
    V = sc.n_vertices
    base = torch.tensor(sc.v_base, dtype=torch.float64).reshape(1, V, 3)
    truth = (base.reshape(1, -1) + torch.tensor(sc.weights_gt[:N_FRAMES], dtype=torch.float64)
             @ torch.tensor(sc.blendshapes, dtype=torch.float64).t()).reshape(N_FRAMES, V, 3)
    fl = R.FaceLaplacian(sc.pos_idx, V)
    nbr = S.ring_table(sc.pos_idx, V)
    edges = S.edge_list(nbr)
    elen = lambda x: (x[:, edges[:, 0]] - x[:, edges[:, 1]]).norm(dim=2)
    print(f"cfg1 mesh: {V} vertices, {edges.shape[0]} edges, mean edge length {float(elen(base).mean()):.2f}")
    lap_base = fl.apply(base)[0]
    per, value = R.penalty_value(lap_base, WEIGHT)
    grad = R.penalty_grad(lap_base, per, fl, WEIGHT)[0]
    print(f"Laplacian term at the base mesh (weight {WEIGHT:g}): {float(value):.1f}")
    print(f"its gradient at the base mesh: up to {float(grad.abs().max()):.1f} per coordinate (rms {float((grad ** 2).mean().sqrt()):.2f})")
    print(f"mesh_edge_loss(., 0.1) at the base mesh: {float(S.stretch(base, nbr, None, 1.0, 0.1)['value'][0]):.2f}")
    per_plain = fl.apply(truth)[0].norm(dim=2).mean(dim=1)
    per_rest = S.rest_differentials(fl, truth, lap_base[0])[0].norm(dim=2).mean(dim=1)
    print(f"mean ||L x|| on the {N_FRAMES} ground-truth frames: " + ", ".join(f"{float(p):.3f}" for p in per_plain)
          + f" (mean {float(per_plain.mean()):.3f})")
    print("the same against the base mesh's differentials, mean ||L x - L x_base||: " + ", ".join(f"{float(p):.3f}" for p in per_rest))
    err = ((elen(truth) - elen(base)) ** 2).mean()
    print(f"rest-length edge error mean (|e| - |e_base|)^2 on those frames: {float(err):.1e}")
    st = S.rest_penalty(fl, base, lap_base[0], WEIGHT)
    print(f"rest Laplacian term and the largest entry of its gradient at the base mesh: {float(st['value'][0]):g}, {float(st['grad'][0].abs().max()):g}")
    b = bend_rows()
    print(f"hinges: {b['hinges']} ({b['inconsistent']} inconsistently oriented)")
    print(f"mesh_normal_consistency at the base mesh: {b['plain_base']:.6f}")
    print(f"its gradient at the base mesh, per unit weight: up to {b['plain_grad_max']:.1e} per coordinate (rms {b['plain_grad_rms']:.1e})")
    print(f"dihedral angles of the base mesh: mean absolute {b['angle_mean_deg']:.1f} deg, largest {b['angle_max_deg']:.1f} deg")
    print(f"plain term on the {N_FRAMES} ground-truth frames: " + ", ".join(f"{v:.6f}" for v in b['plain_truth']))
    print("the same measured from the base mesh's own angles (Bend rule): " + ", ".join(f"{v:.1e}" for v in b['rest_truth']))


if __name__ == "__main__":
    main()

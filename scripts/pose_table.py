"""The README's pose table: float64 on the CPU (tests/pose_ref.py, the statement of DESIGN.md 3, "Pose solve rule").

cfg1's mesh at 128 x 128, cameras 0 and 4, 40 landmarks on every thirteenth vertex projected without noise; the truth is turned 25
degrees about (0.3, 0.9, 0.2) and moved by (6, -3, 4), the start is the identity.  Rows: the mean reprojection error at the start; after
the damped Gauss-Newton solve of the rule (poses kept in float64, to show what the iteration reaches; the rule rounds them to float32);
the solved pose after ONE whole-tensor division of per_frame_q (quirk Q3) in a take of F = 2 / 4 / 16 frames, where rigid() applies
q / sqrt(F) as it stands; the translation solved alone.  ONE scene: the reason for the design, not a promise about real takes.

    python scripts/pose_table.py
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMS = (0, 4)
TRIALS = 12


def rows():
    """[(label, mean live |residual| in px)]."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import landmark_ref as LR
    import pose_ref as PR
    from helpers import scene_cameras
    from fpc_diffrend_amd import scene
    sc = scene.make_scene(scene.MESH_1K, 10, 1, (128, 128), (256, 256, 1), 0)
    H, W = sc.resolution
    proj, base = scene_cameras(sc, CAMS)
    x = torch.tensor(sc.v_base).reshape(1, -1, 3).float()
    points = [{'vertex': v} for v in range(0, sc.n_vertices, 13)]
    vtx, bary, _ = LR.tables(points, sc.n_vertices, sc.pos_idx)
    axis = np.array([0.3, 0.9, 0.2]) / np.linalg.norm([0.3, 0.9, 0.2])
    h = math.radians(25.0) / 2
    q_true = torch.tensor(np.concatenate([math.sin(h) * axis, [math.cos(h)]]))[None]
    t_true = torch.tensor([[6.0, -3.0, 4.0]], dtype=torch.float64)
    obs = torch.zeros(len(CAMS), len(points), 3, dtype=torch.float64)
    obs[..., 2] = 1.0
    at = PR.normal(x, proj, base, vtx, bary, None, obs, q_true, t_true, H, W)
    assert bool(at['live'].all())
    obs[..., :2] = at['res'][0]
    a = (x, proj, base, vtx, bary, None, obs)
    q0, t0 = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64)
    mean = lambda q, t: PR.mean_residual(*a, q, t, H, W)

    def mean_with(Rm, t):      # the rotation as a matrix: what rigid() makes of a quaternion that is NOT a unit quaternion
        y = PR.normal(*a, q0, t0, H, W)['y'][0]                                         # [Nc,L,3]
        z = y @ Rm.T + t[0]
        p = torch.einsum('crk,clk->clr', proj.double()[:, :, :3], z) + proj.double()[:, None, :, 3]
        u = (p[..., 0] / p[..., 3] * 0.5 + 0.5) * W - 0.5
        v = (p[..., 1] / p[..., 3] * 0.5 + 0.5) * H - 0.5
        return float(torch.stack([u - obs[..., 0], v - obs[..., 1]], dim=-1).norm(dim=-1).mean())

    out = [("start", mean(q0, t0))]
    q, t, info, trace = PR.solve(*a, q0, t0, H, W, iters=TRIALS, round32=False)
    out.append((f"damped Gauss–Newton on the landmark rule, {TRIALS} trials", mean(q, t)))
    Rm = torch.stack([torch.stack([c.v.reshape(()) for c in row]) for row in PR.rotation([PR.SV(q[0, i]) for i in range(4)])])
    assert abs(mean_with(Rm, t) - mean(q, t)) <= 1e-9
    after = [mean_with(torch.eye(3, dtype=torch.float64) + (Rm - torch.eye(3, dtype=torch.float64)) / F, t) for F in (2, 4, 16)]
    out.append(("the same pose after ONE whole-tensor renormalisation, F = 2 / 4 / 16", after))
    qt, tt, _, _ = PR.solve(*a, q0, t0, H, W, iters=TRIALS, rotate=False, round32=False)
    out.append(("translation solved alone, rotation left at the identity", mean(qt, tt)))
    return out


def fmt(v):
    if isinstance(v, list):
        return " / ".join(f"{x:.1f}" for x in v) + " px"
    return f"{v:.1f} px" if v >= 0.05 else f"{v:.0e} px".replace("e-", "e-")


if __name__ == "__main__":
    print("| state | mean reprojection error |")
    print("|---|---|")
    for label, v in rows():
        print(f"| {label} | {fmt(v)} |")

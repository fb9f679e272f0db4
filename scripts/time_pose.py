"""HIP-event times of the pose solve (csrc/landmark_pose.hip, fpcdr_landmark_pose) at F in {32, 1024} frames x 9 views, L = 68 landmarks
on cfg3's 15002-vertex mesh, 20 trials, the variants taking turns in one process:

  fpcdr_landmark_pose F = ..., 20 trials    every frame's truth 25 degrees / 8 units from the identity start; the start pose is copied back
                                            in front of every call (two small device copies, inside the timed region)
  fpcdr_landmark_pose F = ..., iters = 0    one pass: cost and normal equations at the start pose

Before timing, the solved poses are held against the observations: the mean live |residual| must end below 0.01 px.  Recorded, not
gated: the call runs once per fit and the commit before it has nothing to compare it with.

    python scripts/time_pose.py [--commit NAME] [--seconds S]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC, L, ITERS = 9, 68, 20
H, W = 1080, 1920


def calls(seconds):
    import numpy as np
    import torch
    import pose_cases as PC
    import pose_ref as PR
    from time_landmark import _points
    from time_motion import time_turns
    from helpers import scene_cameras
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg3')
    V = sc.n_vertices
    points = _points(sc)
    lms = fit.LandmarkSet(points, V, sc.pos_idx, 'cuda')
    vtx, bary = lms.vtx.cpu().numpy(), lms.bary.cpu().numpy()
    proj, base = scene_cameras(sc, list(range(NC)))
    g = torch.Generator().manual_seed(0)
    variants = []
    for F in (32, 1024):
        x = (torch.tensor(sc.v_base).reshape(1, V, 3) + 0.05 * torch.randn(F, V, 3, generator=g)).float().contiguous()
        poses = [PC.pose_of(25.0, 8.0, f) for f in range(F)]
        q_true, t_true = torch.tensor(np.stack([p[0] for p in poses])), torch.tensor(np.stack([p[1] for p in poses]))
        obs = torch.zeros(F * NC, L, 3, dtype=torch.float64)
        obs[..., 2] = 1.0
        at = PR.normal(x, proj, base, vtx, bary, None, obs, q_true, t_true, H, W)
        obs = torch.cat([torch.nan_to_num(at['res']).reshape(F * NC, L, 2), at['live'].reshape(F * NC, L, 1).double()], dim=-1).float()
        xd, pd, bd, od = x.cuda(), proj.cuda(), base.cuda(), obs.cuda().contiguous()
        q0 = torch.zeros(F, 4, device='cuda')
        q0[:, 3] = 1.0
        t0 = torch.zeros(F, 3, device='cuda')
        q, t = q0.clone(), t0.clone()

        def call(iters, xd=xd, pd=pd, bd=bd, od=od, q=q, t=t, q0=q0, t0=t0):
            q.copy_(q0)
            t.copy_(t0)
            return fit.solve_pose(xd, pd, bd, lms, od, q, t, (H, W), iters=iters)

        info = call(ITERS).cpu()
        end = PR.mean_residual(x, proj, base, vtx, bary, None, obs, q.cpu(), t.cpu(), H, W)
        print(f"  F = {F}: {int(at['live'].sum())} of {at['live'].numel()} entries live; accepted trials {int(info[:, 3].min())} .. "
              f"{int(info[:, 3].max())}; mean live |residual| after the solve {end:.2e} px", flush=True)
        assert end < 1e-2
        variants += [(f"fpcdr_landmark_pose F = {F}, {ITERS} trials", lambda call=call: call(ITERS)),
                     (f"fpcdr_landmark_pose F = {F}, iters = 0", lambda call=call: call(0))]
    time_turns(variants, seconds)


def main(commit, seconds):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"commit {commit}; {NC} views, L = {L}, {ITERS} trials", flush=True)
    calls(seconds)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")))

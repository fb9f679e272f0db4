"""HIP-event times of the expression solve (csrc/landmark_expr.hip, fpcdr_landmark_expr) at F in {32, 1024} frames, 20 trials, in two
shapes -- cfg3's: Kb = 150 blend weights, L = 68 landmarks, Nc = 9 views on the 15002-vertex mesh; cfg1's: Kb = 10, L = 40, Nc = 2 on the
514-vertex mesh --, and cfg3's with a quarter of the landmarks (L = 17: the assembly of H scales with L, the factorisation does not, so the
two times split a trial between them), the variants taking turns in one process:

  fpcdr_landmark_expr    every frame's truth weights dense in [-3, 5], the start at neutral; the start weights are copied back in front
                         of every call (one small device copy, inside the timed region)
  fpcdr_landmark_pose    the pose solve at the same F, L, Nc (scripts/time_pose.py's call), for scale
  torch, float32         the same rule as batched float32 torch on the GPU: a host loop over the trials, per trial the projection, the
                         Jacobian [F, 2 Nc L, Kb], H by one batched product, torch.linalg.cholesky_ex and cholesky_solve, the accept /
                         reject by torch.where (left out when this torch build has no batched Cholesky on the device)

Before timing, the solved weights are held against the observations: the mean live |residual| must end below 0.01 px.  Recorded, not
gated: the call runs once per fit and the commit before it has nothing to compare it with.

    python scripts/time_expr.py [--commit NAME] [--seconds S]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 20
SHAPES = [("cfg3", 150, 68, 9, (1080, 1920)), ("cfg3", 150, 17, 9, (1080, 1920)), ("cfg1", 10, 40, 2, (256, 256))]


def _project(x, mvp, vtx, bary, Nc):
    """(u, v, w) in NDC terms of every landmark, in x's dtype: x [F,V,3], mvp [F Nc,4,4] -> p [F,Nc,L,4] (rows x, y, z, w)."""
    import torch
    q = sum(bary[k][None, :, None] * x[:, vtx[k]] for k in range(3))                                    # [F,L,3]
    m = mvp.reshape(x.shape[0], Nc, 4, 4)
    return torch.einsum('fcrk,flk->fclr', m[..., :3], q) + m[:, :, None, :, 3]


def _torch_solver(x, mvp, A, vtx, bary, obs, Nc, H, W, iters):
    """The rule in batched float32 torch (L2, no ridge, every entry live): -> a function of the start weights."""
    import torch
    F, L, Kb = x.shape[0], obs.shape[1], A.shape[2]
    p0 = sum(bary[k][None, :, None] * x[:, vtx[k]] for k in range(3))                                   # [F,L,3]
    m = mvp.reshape(F, Nc, 4, 4)
    us = obs.reshape(F, Nc, L, 3)

    def sums(dw):
        q = p0 + torch.einsum('lak,fk->fla', A, dw)
        p = torch.einsum('fcrk,flk->fclr', m[..., :3], q) + m[:, :, None, :, 3]
        nx, ny, pw = p[..., 0] / p[..., 3], p[..., 1] / p[..., 3], p[..., 3]
        ru, rv = (nx * 0.5 + 0.5) * W - 0.5 - us[..., 0], (ny * 0.5 + 0.5) * H - 0.5 - us[..., 1]
        gu = (0.5 * W / pw)[..., None] * (m[:, :, None, 0, :3] - nx[..., None] * m[:, :, None, 3, :3])
        gv = (0.5 * H / pw)[..., None] * (m[:, :, None, 1, :3] - ny[..., None] * m[:, :, None, 3, :3])
        J = torch.cat([torch.einsum('fcla,lak->fclk', gu, A), torch.einsum('fcla,lak->fclk', gv, A)], dim=1).reshape(F, -1, Kb)
        r = torch.cat([ru, rv], dim=1).reshape(F, -1)
        return torch.bmm(J.transpose(1, 2), J), torch.bmm(J.transpose(1, 2), r[..., None]), (r * r).sum(dim=1)

    def solve(w0):
        w = w0.clone()
        Hm, g, E = sums(w - w0)
        lam = torch.full((F, 1, 1), 1e-3, device=x.device)
        eye = torch.eye(Kb, device=x.device)[None]
        for _ in range(iters):
            M = Hm + lam * eye * Hm
            Lc, bad = torch.linalg.cholesky_ex(M)
            wn = w - torch.cholesky_solve(g, Lc)[..., 0]
            H2, g2, E2 = sums(wn - w0)
            keep = (bad == 0) & (E2 < E)
            k1, k2 = keep[:, None], keep[:, None, None]
            w, Hm, g, E = torch.where(k1, wn, w), torch.where(k2, H2, Hm), torch.where(k2, g2, g), torch.where(keep, E2, E)
            lam = torch.where(k2, (lam / 10).clamp(min=1e-9), (lam * 10).clamp(max=1e9))
        return w

    return solve


def calls(seconds):
    import torch
    from time_landmark import _points
    from time_motion import time_turns
    from helpers import scene_cameras, scene_mvps
    from fpc_diffrend_amd import fit, scene
    for name, Kb, L, Nc, (H, W) in SHAPES:
        sc = scene.cfg(name, n_frames=1)
        V = sc.n_vertices
        points = _points(sc)[:L] if name == "cfg3" else [{'vertex': v} for v in range(0, V, 13)]
        assert len(points) == L and sc.blendshapes.shape[1] == Kb
        lms = fit.LandmarkSet(points, V, sc.pos_idx, 'cuda')
        vtx, bary = lms.vtx.long(), lms.bary
        sc.q_gt[0], sc.t_gt[0] = (0.0, 0.0, 0.0, 1.0), 0.0
        mvp1 = scene_mvps(sc, list(range(Nc)), [0]).cuda()
        proj, base = (t.cuda() for t in scene_cameras(sc, list(range(Nc))))
        B = torch.tensor(sc.blendshapes).float().cuda().contiguous()
        A = (sum(bary[k][:, None, None] * B.reshape(V, 3, Kb)[vtx[k]] for k in range(3))).contiguous()     # [L,3,Kb]
        g = torch.Generator().manual_seed(0)
        variants = []
        for F in (32, 1024):
            w_true = (8.0 * torch.rand(F, Kb, generator=g, dtype=torch.float64) - 3.0).cuda()
            x = torch.tensor(sc.v_base).float().cuda().reshape(1, V, 3).expand(F, V, 3).contiguous()
            mvp = mvp1.repeat(F, 1, 1).contiguous()
            x_true = (torch.tensor(sc.v_base).double().cuda()[None] + w_true @ B.double().t()).reshape(F, V, 3)
            p = _project(x_true, mvp.double(), vtx, bary.double(), Nc)
            assert bool((p[..., 3] > 1e-6).all())
            obs = torch.stack([(p[..., 0] / p[..., 3] * 0.5 + 0.5) * W - 0.5, (p[..., 1] / p[..., 3] * 0.5 + 0.5) * H - 0.5, torch.ones_like(p[..., 0])],
                              dim=-1).reshape(F * Nc, L, 3).float().contiguous()
            del x_true, p
            w0 = torch.zeros(F, Kb, device='cuda')
            w = w0.clone()

            def expr(iters=ITERS, x=x, mvp=mvp, obs=obs, w=w, w0=w0):
                w.copy_(w0)
                return fit.solve_expression(x, mvp, B, lms, obs, w, (H, W), iters=iters)

            info = expr().cpu()
            res = torch.full((F * Nc, L, 2), float('nan'), device='cuda')
            xs = (x.reshape(F, -1) + w @ B.t()).reshape(F, V, 3).contiguous()
            fit.landmark_penalty(xs, mvp, lms, obs, 1.0, (H, W), residuals=res)
            end = float(res.double().norm(dim=-1).mean())
            print(f"  {name} F = {F}: accepted trials {int(info[:, 3].min())} .. {int(info[:, 3].max())}; mean |residual| after the solve {end:.2e} px; "
                  f"largest weight error {float((w.double() - w_true).abs().max()):.2e}", flush=True)
            assert end < 1e-2 or 3 * L < Kb      # (the quarter shape is under-determined: timed, not held)
            del xs, res
            q0 = torch.zeros(F, 4, device='cuda')
            q0[:, 3] = 1.0
            t0, q, t = torch.zeros(F, 3, device='cuda'), q0.clone(), torch.zeros(F, 3, device='cuda')

            def pose(x=x, obs=obs, q=q, t=t, q0=q0, t0=t0):
                q.copy_(q0)
                t.copy_(t0)
                return fit.solve_pose(x, proj, base, lms, obs, q, t, (H, W), iters=ITERS)

            tag = f"{name} Kb = {Kb}, L = {L}, Nc = {Nc}, F = {F}"
            variants += [(f"fpcdr_landmark_expr {tag}", expr), (f"fpcdr_landmark_expr iters = 0 {tag}", lambda expr=expr: expr(0)),
                         (f"fpcdr_landmark_pose {tag}", pose)]
            try:
                solver = _torch_solver(x, mvp, A, vtx, bary, obs, Nc, H, W, ITERS)
                wt = solver(w0)
                torch.cuda.synchronize()
                print(f"  {name} F = {F}: torch float32 ends {float((wt - w).abs().max()):.2e} from the kernel's weights", flush=True)
                variants.append((f"torch float32, batched {tag}", lambda solver=solver, w0=w0: solver(w0)))
            except RuntimeError as e:
                print(f"  {name} F = {F}: no batched float32 torch variant on this build ({str(e).splitlines()[0][:100]})", flush=True)
        time_turns(variants, seconds, calls=2)


def main(commit, seconds):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"commit {commit}; {ITERS} trials", flush=True)
    calls(seconds)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")))

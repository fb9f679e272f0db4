"""Seeded inputs of the expression solve's tests (tests/test_expr_ref.py on the CPU, tests/test_gpu_expr.py on the GPU).

normal_case: the inputs of landmark_cases.case on cfg1's 514-vertex mesh -- meshes, landmark tables, weights, observations with a third
not observed and NaN for their positions, points behind image 0 -- plus a seeded dense blend basis [3V,Kb] and input weights [F,Kb].

solve_case: cfg1's base mesh and a Gaussian-bump blend basis of Kb shapes (scene.make_blendshapes), three frames under the Scene's own
truth poses on a 128 x 128 raster, each frame with its own dense truth weights; the observations are the float64 projection at that
truth, for the robust variant plus 1 px of noise with every sixth detection 30 px off and a Charbonnier scale of 2 px.  The solve starts
at neutral.  Frame 1 keeps two live entries, which no solve may touch; blendshape DEAD is zero at every landmark's corners and starts
at 0.25: without a ridge no solve may touch it either."""
import functools

import numpy as np
import torch

import expr_ref as ER
import landmark_cases as LC
from helpers import scene_mvps

H, W = 128, 128                 # the raster of solve_case (normal_case keeps landmark_cases' 72 x 96)
V = 514
DEAD = 7
DEAD_START = 0.25
CAMS = {1: (4,), 2: (0, 3), 9: tuple(range(9))}


@functools.lru_cache(maxsize=None)
def normal_case(F, Nc, L, Kb, use_w=False, use_c=False):
    cs = LC.case(F, Nc, V, L, 0, use_w, use_c)
    g = torch.Generator().manual_seed(900 + 13 * Kb + L)
    basis = (0.5 * torch.randn(3 * V, Kb, generator=g)).float().contiguous()
    w_in = (0.3 * torch.randn(F, Kb, generator=g)).float().contiguous()
    return dict(cs, basis=basis, w_in=w_in)


@functools.lru_cache(maxsize=None)
def _scene(Kb):
    from fpc_diffrend_amd import scene
    return scene.make_scene(scene.MESH_1K, Kb, 3, (256, 256), (256, 256, 1), 0)


@functools.lru_cache(maxsize=None)
def solve_case(L, Nc, Kb=10, robust=False, F=3, seed=0):
    """-> dict: x [F,V,3] (the meshes at w_in), mvp [F Nc,4,4], basis [3V,Kb], points, faces, vtx, bary, w (None), obs [F Nc,L,3], w_in
    [F,Kb], w_true [F,Kb] float64, x_true [F,V,3] float64, scale (None or 2.0), still (the frame with two live entries), dead."""
    sc = _scene(Kb)
    g = torch.Generator().manual_seed(8000 + 100 * seed + 10 * L + Nc + 7 * Kb + (500 if robust else 0))
    base = torch.tensor(sc.v_base).reshape(-1, 3).float()
    assert base.shape[0] == V
    faces = np.asarray(sc.pos_idx)
    points = LC.points_of(V, L, faces, seed + 11 * L + V)
    vtx, bary, _ = LC.LR.tables(points, V, faces)
    basis = torch.tensor(sc.blendshapes).float().clone().reshape(V, 3, Kb)
    dead = min(DEAD, Kb - 1)
    basis[torch.as_tensor(np.unique(np.asarray(vtx))), :, dead] = 0.0      # no landmark touches this blendshape
    basis = basis.reshape(3 * V, Kb).contiguous()
    mvp = scene_mvps(sc, CAMS[Nc], list(range(F))).contiguous()
    w_true = 8.0 * torch.rand(F, Kb, generator=g, dtype=torch.float64) - 3.0         # (a bump of weight 1 moves a landmark by a tenth of a pixel here)
    w_in = torch.zeros(F, Kb)
    w_in[:, dead] = DEAD_START
    x = (base.reshape(1, -1) + w_in @ basis.t()).reshape(F, V, 3).contiguous()
    x_true = (base.double().reshape(1, -1) + w_true @ basis.double().t()).reshape(F, V, 3)
    zero_obs = torch.zeros(F * Nc, L, 3, dtype=torch.float64)
    zero_obs[..., 2] = 1.0
    zw = torch.zeros(F, Kb, dtype=torch.float64)
    at = ER.normal(x_true, mvp, basis, vtx, bary, None, zero_obs, zw, zw, H, W)
    assert bool(at['live'].all())                                                    # (the truth has every point in front of its camera)
    obs = torch.zeros(F, Nc, L, 3, dtype=torch.float64)
    obs[..., :2] = at['res']
    obs[..., 2] = 1.0
    scale = None
    if robust:
        obs[..., :2] += torch.randn(F, Nc, L, 2, generator=g, dtype=torch.float64)
        off = torch.zeros(F, Nc * L, dtype=torch.bool)
        off[:, ::6] = True
        ang = 6.283185307179586 * torch.rand(F, Nc, L, generator=g, dtype=torch.float64)
        obs[..., :2] += torch.where(off.reshape(F, Nc, L)[..., None], 30.0 * torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1), torch.zeros(()).double())
        scale = 2.0
    still = 1
    flat = obs[still].reshape(-1, 3)
    flat[2:, 2] = 0.0                                                                # two live entries: the frame must come back as it went in
    flat[2:, :2] = float('nan')
    return dict(x=x, mvp=mvp, basis=basis, points=points, faces=faces, vtx=vtx, bary=bary, w=None,
                obs=obs.reshape(F * Nc, L, 3).float().contiguous(), w_in=w_in.contiguous(), w_true=w_true, x_true=x_true, scale=scale, still=still,
                dead=dead)


RIDGE = 0.05                    # the positive ridge of the cases, px^2 per unit weight^2
SHAPES = [(24, 2, 10), (64, 1, 10), (130, 9, 10), (64, 2, 40)]      # (L, Nc, Kb): both sizes of the kernel by L and by Kb
SOLVE_CASES = [(L, Nc, Kb, robust, ridge) for L, Nc, Kb in SHAPES for robust in (False, True) for ridge in (0.0, RIDGE)]
# the headline shape's Kb and a landmark count beyond one pass of the lanes: the trial loop with more than 64 columns (the second
# stride of the assembly's rows, of the damping and of the trailing update) and with two landmarks a lane
SOLVE_CASES += [(130, 2, 150, False, 0.0), (130, 2, 150, True, RIDGE), (300, 1, 10, False, 0.0), (300, 1, 10, True, RIDGE)]


RES_ROUNDINGS = 21 + 2          # the float32 roundings that reach a residual r_u, plus 2 (fitstep_ref's rules; counted in tests/test_gpu_expr.py)


def cost_floor(r, w):
    """Per frame, the cost that float32 cannot tell from 0, from expr_ref.normal's float64 sums r at the weights w, in two parts.
    The weights: the cost of weights 4 u of their scale max(1, |w|) away, delta^T diag(H) delta -- trial weights are rounded to float32
    in BOTH statements, so a cost below this is the rounding of the weights, not a value (pose_cases.cost_floor's counterpart).  The
    evaluation: the kernel forms every residual in float32, within RES_ROUNDINGS u of the residual's scale S (the pixel coordinate's
    and the detection's magnitudes: |u - u*| is 1e-5 px at a solution and S is a hundred pixels), so a cost below
    sum omega kappa ((n u S_u)^2 + (n u S_v)^2) over the live entries is the rounding of its own residuals.  The float64 statement
    evaluates in float64 and has only the first part; neither part comes from what the kernel returns."""
    Kb = w.shape[1]
    idx = torch.arange(Kb)
    diag = r['H'][0][:, idx * (idx + 1) // 2 + idx]                                   # [F,Kb]
    ws = torch.clamp(w.detach().double().abs(), min=1.0)
    of_weights = (diag * (4 * 2.0 ** -24 * ws) ** 2).sum(dim=1)
    F = w.shape[0]
    of_evaluation = (r['wk'][..., None] * (RES_ROUNDINGS * 2.0 ** -24 * r['resS']) ** 2).reshape(F, -1).sum(dim=1)
    return of_weights + of_evaluation


def weight_floor(w):
    """4 u of the weights' scale max(1, |w|_inf): the distance of two float32 tables that agree to the last places."""
    return 4 * 2.0 ** -24 * max(1.0, float(w.detach().abs().max()))

"""Seeded inputs of the pose solve's tests (tests/test_pose_ref.py on the CPU, tests/test_gpu_pose.py on the GPU).

normal_case: the inputs of landmark_cases.case -- meshes, landmark tables, weights, observations with a third not observed and NaN for
their positions, points behind image 0 -- under the same cameras split into proj and base, at the Scene's truth pose with the
quaternion scaled off the unit sphere (the rule normalises it).

solve_case: cfg1's base mesh, three frames, each with its own truth pose `deg` degrees and `units` units from the identity the solve
starts at; the observations are the float64 projection at that truth, for the robust variant plus 1 px of noise with every sixth
detection 30 px off and a Charbonnier scale of 2 px; frame 1 keeps two live entries, which no solve may touch."""
import functools
import math

import numpy as np
import torch

import landmark_cases as LC
import pose_ref as PR
from helpers import scene_cameras

H, W = LC.H, LC.W
CAMS = {1: (4,), 2: (0, 3), 9: tuple(range(9))}
OFFSETS = ((25.0, 8.0), (40.0, 11.0))


@functools.lru_cache(maxsize=None)
def cameras(Nc):
    """(proj [Nc,4,4], base [Nc,4,4]) float32 of landmark_cases' cameras: base = MV_c . T(0,170,0), the cameras' own poses at identity."""
    proj, base = scene_cameras(LC._scene(), CAMS[Nc])
    return proj.contiguous(), base.contiguous()


@functools.lru_cache(maxsize=None)
def normal_case(F, Nc, V, L, use_w=False, use_c=False):
    cs = LC.case(F, Nc, V, L, 0, use_w, use_c)
    sc = LC._scene()
    proj, base = cameras(Nc)
    q = torch.tensor(np.asarray(sc.q_gt[:F], dtype=np.float32)) * torch.tensor([0.7, 1.0, 1.9][:F])[:, None]
    t = torch.tensor(np.asarray(sc.t_gt[:F], dtype=np.float32))
    return dict(cs, proj=proj, base=base, q=q.contiguous(), t=t.contiguous())


def pose_of(deg, units, seed):
    """A unit quaternion (XYZW) turned deg degrees about a seeded axis and a translation of `units` units in a seeded direction, float64."""
    rng = np.random.default_rng(seed)
    axis, d = rng.normal(size=3), rng.normal(size=3)
    axis, d = axis / np.linalg.norm(axis), d / np.linalg.norm(d)
    h = math.radians(deg) / 2.0
    return np.concatenate([math.sin(h) * axis, [math.cos(h)]]), units * d


@functools.lru_cache(maxsize=None)
def solve_case(L, Nc, offset=0, robust=False, F=3, seed=0):
    """-> dict: x [F,V,3], proj, base, points, faces, vtx, bary, w (None), obs [F Nc,L,3], q / t (the start: identity), q_true / t_true
    (float64), scale (None or 2.0), still (the frame with two live entries)."""
    deg, units = OFFSETS[offset]
    sc = LC._scene()
    g = torch.Generator().manual_seed(7000 + 100 * seed + 10 * L + Nc + 1000 * offset + (500 if robust else 0))
    base_mesh = torch.tensor(sc.v_base).reshape(-1, 3).float()
    V = base_mesh.shape[0]
    x = (base_mesh[None] + 0.2 * torch.randn(F, V, 3, generator=g)).float().contiguous()
    faces = np.asarray(sc.pos_idx)
    points = LC.points_of(V, L, faces, seed + 11 * L + V)
    vtx, bary, _ = LC.LR.tables(points, V, faces)
    proj, base = cameras(Nc)
    poses = [pose_of(deg, units, 31 * f + L + Nc + seed) for f in range(F)]
    q_true, t_true = torch.tensor(np.stack([p[0] for p in poses])), torch.tensor(np.stack([p[1] for p in poses]))
    zero_obs = torch.zeros(F * Nc, L, 3, dtype=torch.float64)
    zero_obs[..., 2] = 1.0
    at = PR.normal(x, proj, base, vtx, bary, None, zero_obs, q_true, t_true, H, W)
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
    q = torch.zeros(F, 4)
    q[:, 3] = 1.0
    return dict(x=x, proj=proj, base=base, points=points, faces=faces, vtx=vtx, bary=bary, w=None,
                obs=obs.reshape(F * Nc, L, 3).float().contiguous(), q=q, t=torch.zeros(F, 3), q_true=q_true, t_true=t_true, scale=scale,
                still=still)


SOLVE_CASES = [(L, Nc, offset, robust) for L in (6, 64, 130) for Nc in (1, 2, 9) for offset in (0, 1) for robust in (False, True)]


def pose_distance(q, t, q_ref, t_ref):
    """(max over the frames of min |q -+ q_ref|_inf, max |t - t_ref|_inf): q and -q are the same rotation."""
    q, t, q_ref, t_ref = (v.detach().cpu().double() for v in (q, t, q_ref, t_ref))
    dq = torch.minimum((q - q_ref).abs().amax(dim=1), (q + q_ref).abs().amax(dim=1))
    return float(dq.max()), float((t - t_ref).abs().max())


def cost_floor(r, t):
    """Per frame, the cost of a pose 4 u of its scale away (1 for the rotation, max(|t|, |y|) for the translation) from pose_ref.normal's
    sums r at the poses (., t): delta^T diag(A) delta.  Trial poses are rounded to float32 in BOTH statements, so a cost below this is the
    rounding of the pose, not a value: a change of E down there says nothing, and a float64 E_out down there is 0 as far as the
    reference can tell."""
    diag = torch.stack([r['A'][0][:, k] for k, (i, j) in enumerate(PR.TRI) if i == j], dim=1)      # [F,6]
    ts = max(float(t.abs().max()), float(r['y'].abs().max()))
    s = torch.tensor([1.0, 1.0, 1.0, ts, ts, ts], dtype=torch.float64)
    return (diag.double() * (4 * 2.0 ** -24 * s) ** 2).sum(dim=1)

"""Seeded inputs of the landmark term's tests (tests/test_landmark_ref.py on the CPU, tests/test_gpu_landmark.py on the GPU): meshes at
y + 170 under the matrices of helpers.scene_mvps, landmarks as vertices and as points of faces, some of them sharing a vertex, some
behind a camera, a third of the confidences (and, asked for, of the landmark weights) at 0."""
import functools

import numpy as np
import torch

import landmark_ref as LR
from helpers import scene_mvps

H, W = 72, 96      # the raster of the observations: not square, so that a swapped pair shows


@functools.lru_cache(maxsize=None)
def _scene():
    from fpc_diffrend_amd import scene
    return scene.cfg('cfg1', n_frames=3)


@functools.lru_cache(maxsize=None)
def _mvps(F, Nc):
    cams = {1: (4,), 2: (0, 3), 9: tuple(range(9))}[Nc]
    return scene_mvps(_scene(), cams, list(range(F))).contiguous()


def points_of(V, L, faces, seed):
    """L points over a mesh of V vertices: two in three at a vertex, one in three inside a face; neighbours in the list share vertices."""
    rng = np.random.default_rng(seed)
    pts = []
    for l in range(L):
        if l % 3 == 2:
            b = rng.uniform(0.1, 1.0, size=3)
            b /= b.sum()
            p = {'face': int(rng.integers(0, len(faces))), 'bary': tuple(float(v) for v in b)}
        else:      # (l and l + 1 of a pair name the same vertex)
            p = {'vertex': int(rng.integers(0, V)) if l % 3 == 0 or not pts else pts[-1]['vertex']}
        pts.append(p)
    return pts


@functools.lru_cache(maxsize=None)
def case(F, Nc, V, L, seed=0, use_w=False, use_c=False, lift=170.0, noise=5.0, shift=15.0, far=600.0):
    """-> dict: x [F,V,3] float32 at y + 170, mvp [F Nc,4,4], points, faces, vtx, bary, w (or None), obs [F Nc,L,3], scale (or None)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + L)
    sc = _scene()
    if V == 514:
        base = torch.tensor(sc.v_base).reshape(-1, 3).float().clone()
        faces = np.asarray(sc.pos_idx)
    else:
        base = 8.0 * torch.randn(V, 3, generator=g)
        faces = np.stack([np.random.default_rng(seed + V).permutation(V)[:3] for _ in range(max(V // 2, 1))])
    base[:, 1] += lift
    x = (base[None] + 0.3 * torch.randn(F, V, 3, generator=g)).float().contiguous()
    mvp = _mvps(F, Nc)
    points = points_of(V, L, faces, seed + 11 * L + V)
    vtx, bary, w = LR.tables(points, V, faces)
    # some points behind the camera: every seventh landmark's first vertex is mirrored through the plane p.w = 0 of image 0
    # (where that leaves the vertex within 20 units of another image's plane it stays where it was: 1 / p.w^2 is no test of a kernel)
    a, d = mvp[0, 3, :3].double(), float(mvp[0, 3, 3])
    rows = mvp[:, 3, :].double().reshape(F, Nc, 4)
    for l in range(3, L, 7):
        v = int(vtx[0, l])
        pw = x[:, v].double() @ a + d
        moved = x[:, v].double() - 2.0 * pw[:, None] * a[None] / float(a @ a)
        if float(((rows[..., :3] * moved[:, None]).sum(-1) + rows[..., 3]).abs().min()) > 20.0:
            x[:, v] = moved.float()
    wv = None
    if use_w:
        wv = (0.25 + 1.5 * torch.rand(L, generator=g)).float()
        wv[1::3] = 0.0
    # observations: the float64 projection plus a few pixels of noise; a third not observed (their positions are NaN: never read)
    zero_obs = torch.zeros(F * Nc, L, 3)
    zero_obs[..., 2] = 1.0
    ref = LR.landmark(x, mvp, vtx, bary, None, zero_obs, 1.0, H, W, grads=False)
    pw = LR._project(x.double(), mvp.double(), vtx, torch.as_tensor(bary).double(), Nc)[2][2]
    near = pw.abs() <= 5.0                 # (a face's point between a moved vertex and one that stayed: switched off below, not observed)
    proj = torch.nan_to_num(ref['res'][0], nan=0.0)                                  # (u, v) where the point is in front
    obs = torch.zeros(F * Nc, L, 3)
    # (an image's detections sit `shift` pixels off as a whole, as those of a misplaced head do, plus a few pixels of noise each)
    ang = 6.283185307179586 * torch.rand(F * Nc, 1, generator=g, dtype=torch.float64)
    obs[..., :2] = proj + shift * torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1) + noise * torch.randn(F * Nc, L, 2, generator=g, dtype=torch.float64)
    obs[..., 2] = 0.2 + 0.8 * torch.rand(F * Nc, L, generator=g)
    dead = torch.rand(F * Nc, L, generator=g) < 1.0 / 3.0
    dead.reshape(-1)[0] = False
    dead |= near
    dead |= (proj.abs() > far).any(dim=-1)      # (a moved vertex seen by another camera lands tens of thousands of pixels off: no detector reports that)
    obs[..., 2][dead] = 0.0
    obs[..., 0][dead] = float('nan')
    obs[..., 1][dead] = float('nan')
    obs = obs.float().contiguous()
    scale = None
    if use_c:      # the median |residual| of the live entries: both regimes occur
        r = LR.landmark(x, mvp, vtx, bary, wv, obs, 1.0, H, W, grads=False)['res'][0]
        live = ~torch.isnan(r[..., 0])
        scale = float(r[live].norm(dim=1).median()) if bool(live.any()) else 2.0
    return dict(x=x, mvp=mvp, points=points, faces=faces, vtx=vtx, bary=bary, w=wv, obs=obs, scale=scale)

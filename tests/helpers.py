"""Shared builders for the parity tests (seeded synthetic inputs; nothing reads /root/reference)."""
import os

import numpy as np
import torch

from fpc_diffrend_amd import camera, scene


def lib_loaded():
    """(the _lib module, the loaded product library), both libraries built first when one is missing."""
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.TWOCALL_LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def rel_l2(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def scene_mvps(sc, cam_ids, frames=None):
    """mvp [len(frames)*len(cam_ids),4,4] float32 for the ground-truth pose of `frames` (frame-major)."""
    out = []
    T = camera.translate(0.0, 170.0, 0.0)
    frames = [None] if frames is None else frames
    for f in frames:
        for c in cam_ids:
            cam = sc.cams[c]
            P = camera.intrinsic_to_projection(cam['intr'])
            MV = camera.extrinsic_to_modelview(cam['rot'], cam['trans_calib'])
            m = MV @ T
            if f is not None:
                R = camera.unitquat_to_rotmat(torch.tensor(sc.q_gt[f])).numpy()
                Rt = np.eye(4, dtype=np.float32)
                Rt[:3, :3] = R
                Rt[:3, 3] = sc.t_gt[f]
                m = Rt @ m
            out.append((P @ m).astype(np.float32))
    return torch.tensor(np.stack(out))


def scene_cameras(sc, cam_ids):
    """(proj [Nc,4,4], t_mv [Nc,4,4]) float32 of the scene's cameras, made as scene_mvps makes them (translation 170 included)."""
    T = camera.translate(0.0, 170.0, 0.0)
    proj = [camera.intrinsic_to_projection(sc.cams[c]['intr']) for c in cam_ids]
    mv = [(camera.extrinsic_to_modelview(sc.cams[c]['rot'], sc.cams[c]['trans_calib']) @ T).astype(np.float32) for c in cam_ids]
    return torch.tensor(np.stack(proj)), torch.tensor(np.stack(mv))


def clip_positions(sc, cam_ids, frames=None, jitter=0.0, seed=0):
    """pos_clip [B,V,4] for the base mesh (+ blendshape ground truth per frame)."""
    mvps = scene_mvps(sc, cam_ids, frames)
    V = sc.n_vertices
    if frames is None:
        verts = torch.tensor(sc.v_base.reshape(1, V, 3))
    else:
        vb = torch.tensor(sc.v_base)
        Bm = torch.tensor(sc.blendshapes)
        w = torch.tensor(sc.weights_gt[frames])
        verts = (vb[None] + w @ Bm.t()).reshape(len(frames), V, 3)
    if jitter:
        g = torch.Generator().manual_seed(seed)
        verts = verts + jitter * torch.randn(verts.shape, generator=g)
    return camera.transform_clip(mvps, verts), mvps


def random_soup(B, T, seed, spread=1.2, size=0.5, wmin=0.5, wmax=3.0):
    """Random triangle soup in clip space, many overlaps, mixed facing, some off-screen; V = 3T."""
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(B, T, 1, 2, generator=g) * 2 - 1) * spread
    xy = c + (torch.rand(B, T, 3, 2, generator=g) * 2 - 1) * size
    z = (torch.rand(B, T, 3, 1, generator=g) * 2 - 1) * 0.9
    w = torch.rand(B, T, 3, 1, generator=g) * (wmax - wmin) + wmin
    pos = torch.cat([xy * w, z * w, w], dim=-1).reshape(B, T * 3, 4).contiguous()
    tri = torch.arange(T * 3, dtype=torch.int32).reshape(T, 3)
    return pos, tri


def decode_aa_flags(flags, B, H, W):
    """The antialias flag planes of include/fpcdr.h (uint64 words [2][B][H][ceil(W/64)], bit x % 64 of word x // 64; plane 0:
    pair (p, p+x) blended, plane 1: pair (p, p+y)) -> [B,H,W] uint8 with bit 0 / bit 1, the oracle's form."""
    Wq = (W + 63) // 64
    words = flags.detach().cpu().reshape(2, B, H, Wq)
    shifts = torch.arange(64, dtype=torch.int64)
    bits = ((words[..., None] >> shifts) & 1).reshape(2, B, H, Wq * 64)[..., :W].to(torch.uint8)
    return bits[0] | (bits[1] << 1)


def near_crossing_soup(B, T, seed, frac=0.4):
    """Triangles in front of a perspective-like camera, a share of them with one or two vertices pushed through the near plane
    (z + w < 0, mostly w < 0 as well): clip-space z = a * w_eye + b with the near plane at w = 1."""
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(B, T, 1, 3, generator=g) * 2 - 1) * torch.tensor([1.5, 1.5, 0.0]) + torch.tensor([0.0, 0.0, 4.0])
    v = c + (torch.rand(B, T, 3, 3, generator=g) * 2 - 1) * torch.tensor([0.9, 0.9, 1.2])       # eye space, depth along +z
    push = torch.rand(B, T, 3, generator=g) < frac * 0.6
    push[:, ::3] = False                                                                  # a third of the triangles untouched
    v[..., 2] = torch.where(push, -torch.rand(B, T, 3, generator=g) * 3.0 + 0.5, v[..., 2])     # depth in (-2.5, 0.5): behind / near
    n, f = 1.0, 20.0
    w = v[..., 2:3]
    z = (f + n) / (f - n) * w - 2 * f * n / (f - n)
    pos = torch.cat([v[..., :2] * 1.2, z, w], dim=-1).reshape(B, T * 3, 4).contiguous()
    tri = torch.arange(T * 3, dtype=torch.int32).reshape(T, 3)
    return pos, tri


def decode_id_planes(idp, B, H, W):
    """The id planes of fpcdr_objective_fwd (include/fpcdr.h: 1024 uint32 per 32 x 32 bin, bins in (image, bin row, bin column) order,
    pixel (y & 31) * 32 + (x & 31) inside, value (triangle + 1) | silhouette bits << 24) -> triangle + 1 as [B,H,W] int32 (0 = empty)."""
    OY, OX = (H + 31) // 32, (W + 31) // 32
    v = idp.detach().cpu().contiguous().view(torch.int32).reshape(B, OY, OX, 32, 32) & 0xffffff
    return v.permute(0, 1, 3, 2, 4).reshape(B, OY * 32, OX * 32)[:, :H, :W].contiguous()


def comparison_pair(i, height=1600, width=1200):
    """Image pair i of the re-render comparison fixture (tests/golden/make_golden.py::rerender_golden and
    tests/test_next_rows.py regenerate the same 120 pairs from this formula): two smooth 8-bit images of the reference's
    1600 x 1200 shape (comparisons.py:10) that differ by a slow pattern depending on i -- low entropy, so the PNG / TIFF
    files the generator writes are small."""
    y = np.arange(height, dtype=np.int64)[:, None]
    x = np.arange(width, dtype=np.int64)[None, :]
    ref = ((y // 8) * 3 + (x // 16) * 5 + 7 * i) % 200
    img = (ref + ((y // 64 + x // 32 + i) % 9) * ((y // 32 + i) % 3) - ((x // 128 + 2 * i) % 5)).clip(0, 255)
    return img.astype(np.uint8), ref.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# a Fitter near the truth and the additive check of the terms in front of the pixel objective (tests/test_gpu_rest.py, _bend.py,
# _motion.py, _tex_prior.py, _prior_terms.py)
# ---------------------------------------------------------------------------------------------------------------------

def fitter_near_truth(n_frames, rank=0, world=1, **kw):
    """A Fitter on n_frames of cfg1 with the poses at identity, cameras (0, 3), the plain Laplacian off, at init_near_truth(0.8); kw
    overrides any FitConfig field."""
    from fpc_diffrend_amd import fit
    sc = scene.cfg('cfg1', n_frames=n_frames)
    sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
    base = dict(max_iter=100, cam_idxs=(0, 3), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, weight_laplacian=0.0)
    base.update(kw)
    ft = fit.Fitter(sc, fit.FitConfig(**base), device='cuda', rank=rank, world=world)
    ft.init_near_truth(0.8)
    return ft


def fitter_grads(ft):
    """The gradient of every parameter tensor of a Fitter as a flat float64 vector (zeros where there is none)."""
    return [(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1).double() for p in ft.params]


def flat_grads(ft):
    return torch.cat(fitter_grads(ft))


def additive(log, tag, ft_on, ft_off, frames, term_of, sized=True):
    """g_on - g_off = g_term per parameter tensor, and the same for the loss values; -> (l_term, |g_term|).  term_of(v): the terms that
    ft_on runs and ft_off does not, from direct calls on ft_on's vertices v [Fb,V,3] (and on its other parameters, where a term reads
    them).  log: the tag of the printed line."""
    l_on, l_off = float(ft_on.loss_and_backward(frames)), float(ft_off.loss_and_backward(frames))
    assert bool((ft_on._reg_acc == 0).all())
    g_on, g_off = fitter_grads(ft_on), fitter_grads(ft_off)
    ft_on.optimizer.zero_grad(set_to_none=True)
    Fb = ft_on._n(frames)
    term = term_of(ft_on.vertices(frames).reshape(Fb, -1, 3))
    term.backward()
    g_term, l_term = fitter_grads(ft_on), float(term.detach())
    cat = lambda g: torch.cat(g)
    n_on, n_off, n_term = float(cat(g_on).norm()), float(cat(g_off).norm()), float(cat(g_term).norm())
    worst = 0.0
    for k, (a, b, t) in enumerate(zip(g_on, g_off, g_term)):
        err, bar = float(((a - b) - t).norm()), 1e-4 * (float(a.norm()) + float(b.norm()))
        worst = max(worst, err / bar if bar > 0 else (0.0 if err == 0 else float('inf')))
        assert err <= bar, (tag, k, err, bar)
    print(f"{log} fitter/{tag} |g_on|={n_on:.4e} |g_off|={n_off:.4e} |g_term|={n_term:.4e} worst err/bar={worst:.3e} "
          f"l_on={l_on:.6e} l_off={l_off:.6e} l_term={l_term:.6e}")
    if sized:
        assert 0.1 * n_off <= n_term <= 10.0 * n_off, (tag, n_term, n_off)
    assert abs((l_on - l_off) - l_term) <= 1e-4 * (abs(l_on) + abs(l_off))
    return l_term, n_term

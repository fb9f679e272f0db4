"""float64 statement on the CPU of the landmark term ("Landmark rule"; csrc/landmark.hip k_landmark_points, k_landmark_gather):
the yardstick of tests/test_gpu_landmark.py, itself checked on the CPU by tests/test_landmark_ref.py.  Nothing here imports
fpc_diffrend_amd.

The convention is tests/motion_ref.py's: every function evaluates in `dtype` (float64 by default; float32 gives "the same formula in
float32 by torch", in the order the kernel evaluates it) and returns (value, S) pairs, S the same formula with every input replaced by its
absolute value and every subtraction by an addition.  Every subtraction contributes the absolute values of its OPERANDS: positions sit at
y + 170 and the matrices carry the translation that takes it out again, so m . q + m_3 cancels for real, and the cancellation is charged
to the scale, not to the kernel.  Two divisors are themselves such sums and carry their own scale to first order, because a quotient's
error has a term from its divisor: p.w (S(a / p.w) = S(a) / |p.w| + |a| S(p.w) / p.w^2), and the Charbonnier root h, whose argument is
the square of a cancelling difference (S(1 / h) = ic^2 (|r_u| S(r_u) + |r_v| S(r_v)) / h^3).  The divisor 1 + h of the value enters with
its actual value, as motion_ref.py's does: the value's scale carries S(r)^2, far above it."""
import numpy as np
import torch

from fitstep_ref import _c

W_MIN = 1e-6      # a point counts when p.w > W_MIN


def tables(points, n_vertices, faces):
    """The Landmark rule's mesh side as a plain loop: (vtx [3,L] int64, bary [3,L] float32, w [L] float32) numpy."""
    faces = np.asarray(faces).reshape(-1, 3)
    L = len(points)
    vtx, bary, w = np.zeros((3, L), np.int64), np.zeros((3, L), np.float32), np.ones(L, np.float32)
    for l, p in enumerate(points):
        if 'vertex' in p:
            for k in range(3):
                vtx[k, l] = p['vertex']
            bary[0, l] = 1.0
        else:
            for k in range(3):
                vtx[k, l] = faces[p['face'], k]
                bary[k, l] = np.float32(np.float64(p['bary'][k]))
        w[l] = np.float32(p.get('weight', 1.0))
    assert vtx.min() >= 0 and vtx.max() < n_vertices
    return vtx, bary, w


def incidence(vtx, bary, n_vertices):
    """lm_inc [K,V] int32 as a plain loop: per vertex the corners 3 l + k whose weight is not 0, ascending, pads -1; K >= 1."""
    slots = [[] for _ in range(n_vertices)]
    for l in range(vtx.shape[1]):
        for k in range(3):
            if bary[k, l] != 0:
                slots[int(vtx[k, l])].append(3 * l + k)
    K = max(1, max(len(s) for s in slots))
    inc = np.full((K, n_vertices), -1, dtype=np.int32)
    for v, s in enumerate(slots):
        for j, e in enumerate(s):
            inc[j, v] = e
    return inc


def _project(xx, mm, vtx, b, Nc):
    """q [N,L,3], (px, py, pw) [N,L] and their scales, in the kernel's order of operations."""
    xn = xx.repeat_interleave(Nc, dim=0)                                             # [N,V,3]
    c = [xn[:, torch.as_tensor(np.asarray(vtx[k], dtype=np.int64))] for k in range(3)]      # corners [N,L,3]
    bb = [b[k][None, :, None] for k in range(3)]
    q = (bb[0] * c[0] + bb[1] * c[1]) + bb[2] * c[2]
    qS = (bb[0].abs() * c[0].abs() + bb[1].abs() * c[1].abs()) + bb[2].abs() * c[2].abs()
    p, pS = [], []
    for j in (0, 1, 3):
        m = mm[:, j, :]                                                              # [N,4]
        p.append(((m[:, None, 0] * q[..., 0] + m[:, None, 1] * q[..., 1]) + m[:, None, 2] * q[..., 2]) + m[:, None, 3])
        a = m.abs()
        pS.append(((a[:, None, 0] * qS[..., 0] + a[:, None, 1] * qS[..., 1]) + a[:, None, 2] * qS[..., 2]) + a[:, None, 3])
    return q, qS, p, pS


def landmark(x, mvp, vtx, bary, w, obs, weight, H, W, inv_c=0.0, dtype=torch.float64, grads=True):
    """x [F,V,3], mvp [F Nc,4,4], vtx / bary [3,L], w [L] or None, obs [F Nc,L,3] = (u*, v*, kappa); inv_c = 1 / c as the float32 the
    kernel is handed (0: L2).
      q = sum_k bary_k x[vtx_k],  p = mvp (q, 1),  u = (p.x / p.w 0.5 + 0.5) W - 0.5,  v likewise with H,  live = kappa > 0, omega > 0, p.w > 1e-6
      s = (u - u*)^2 + (v - v*)^2,  rho(s) = s | 2 c^2 (sqrt(1 + s / c^2) - 1),  per_f = sum_c sum_l omega kappa rho / (Nc L),
      value = weight / F sum_f per_f, and the closed-form gradients of the rule.
    -> dict 'per', 'value', 'grad_x', 'grad_mvp' of (value, S); 'res' = (residuals [N,L,2] with NaN where not live, S); 'live' [N,L];
    'zeros': the number of entries without any term of per, grad_x, grad_mvp, as plain loops over the tables predict them."""
    xx, mm, oo = _c(x, dtype), _c(mvp, dtype), _c(obs, dtype)
    F, V = xx.shape[0], xx.shape[1]
    N, L = oo.shape[0], oo.shape[1]
    Nc = N // F
    assert N == F * Nc and mm.shape == (N, 4, 4)
    b = torch.as_tensor(np.asarray(bary, dtype=np.float32)).to(dtype)
    om = torch.ones(L, dtype=dtype) if w is None else _c(torch.as_tensor(w), dtype)
    ic = float(np.float32(inv_c))
    q, qS, (px, py, pw), (pSx, pSy, pSw) = _project(xx, mm, vtx, b, Nc)
    us, vs, kap = oo[..., 0], oo[..., 1], oo[..., 2]
    live = (kap > 0) & (om[None] > 0) & (pw > W_MIN)
    sw = torch.where(live, pw, torch.ones_like(pw))
    hw, hh = 0.5 * W, 0.5 * H
    ru = ((px / sw * 0.5 + 0.5) * (2.0 * hw) - 0.5) - us
    rv = ((py / sw * 0.5 + 0.5) * (2.0 * hh) - 0.5) - vs
    rw = pSw / sw                                                                    # the relative scale of the divisor p.w (>= 1)
    ruS = (((pSx / sw + px.abs() / sw * rw) * 0.5 + 0.5) * (2.0 * hw) + 0.5) + us.abs()
    rvS = (((pSy / sw + py.abs() / sw * rw) * 0.5 + 0.5) * (2.0 * hh) + 0.5) + vs.abs()
    s, sS = ru * ru + rv * rv, ruS * ruS + rvS * rvS
    if ic > 0.0:
        zu, zv = ru * ic, rv * ic
        h = torch.sqrt(1.0 + (zu * zu + zv * zv))
        rho, d, rhoS = (2.0 * s) / (1.0 + h), 1.0 / h, (2.0 * sS) / (1.0 + h)      # (the form without the cancellation; equal to the rule's)
        dS = (ic * ic) * (ru.abs() * ruS + rv.abs() * rvS) / (h * h * h)
    else:
        rho, d, rhoS, dS = s, torch.ones_like(s), sS, torch.zeros_like(s)
    wk = om[None] * kap
    zero = torch.zeros_like(s)
    e, eS = torch.where(live, wk * rho, zero), torch.where(live, wk * rhoS, zero)
    per, perS = e.reshape(F, -1).sum(1) / (Nc * L), eS.reshape(F, -1).sum(1) / (Nc * L)
    wf = float(weight) / F
    nan = torch.full_like(s, float('nan'))
    res = torch.stack([torch.where(live, ru, nan), torch.where(live, rv, nan)], dim=-1)
    resS = torch.stack([torch.where(live, ruS, zero), torch.where(live, rvS, zero)], dim=-1)
    out = {'per': (per, perS), 'value': (wf * per.sum(), abs(wf) * perS.sum()), 'res': (res, resS), 'live': live}
    # what the tables predict: entries that no live term reaches
    lv = live.reshape(F, Nc, L).any(dim=1).numpy()                                   # [F,L]
    reach = np.zeros((F, V), dtype=bool)
    bn = np.asarray(bary)
    for k in range(3):
        on = bn[k] != 0
        for f in range(F):
            reach[f, np.asarray(vtx[k])[on & lv[f]]] = True
    img = live.any(dim=1)
    out['zeros'] = {'per': int((~live.reshape(F, -1).any(dim=1)).sum()), 'grad_x': 3 * int((~reach).sum()),
                    'grad_mvp': 16 * int((~img).sum()) + 4 * int(img.sum()), 'res': 2 * int((~live).sum())}
    if not grads:
        return out
    coef = dtype_scalar(float(weight), dtype) / dtype_scalar(float(F) * float(Nc) * float(L), dtype)
    k2 = (coef * wk) * (d * 2.0)
    gu, gv = k2 * ru, k2 * rv
    k2S = (coef * wk).abs() * (dS * 2.0)
    guS, gvS = k2.abs() * ruS + k2S * ru.abs(), k2.abs() * rvS + k2S * rv.abs()
    ax, ay, axS, ayS = gu * hw, gv * hh, guS * hw, gvS * hh
    gp = [torch.where(live, ax / sw, zero), torch.where(live, ay / sw, zero), torch.where(live, -((ax * px + ay * py) / (sw * sw)), zero)]
    gpS = [torch.where(live, axS / sw + ax.abs() / sw * rw, zero), torch.where(live, ayS / sw + ay.abs() / sw * rw, zero),
           torch.where(live, (axS * pSx + ayS * pSy) / (sw * sw) + ((ax * px).abs() + (ay * py).abs()) / (sw * sw) * (2.0 * rw), zero)]
    q1 = torch.cat([q, torch.ones_like(q[..., :1])], dim=-1)
    q1S = torch.cat([qS, torch.ones_like(q[..., :1])], dim=-1)
    gm, gmS = torch.zeros(N, 4, 4, dtype=dtype), torch.zeros(N, 4, 4, dtype=dtype)
    for r, j in enumerate((0, 1, 3)):
        gm[:, j, :] = (gp[r][..., None] * q1).sum(dim=1)
        gmS[:, j, :] = (gpS[r][..., None] * q1S).sum(dim=1)
    m0, m1, m3 = mm[:, None, 0, :3], mm[:, None, 1, :3], mm[:, None, 3, :3]
    gq = torch.where(live[..., None], (m0 * gp[0][..., None] + m1 * gp[1][..., None]) + m3 * gp[2][..., None], zero[..., None])
    gqS = (m0.abs() * gpS[0][..., None] + m1.abs() * gpS[1][..., None]) + m3.abs() * gpS[2][..., None]
    gx, gxS = torch.zeros(F, V, 3, dtype=dtype), torch.zeros(F, V, 3, dtype=dtype)
    tq, tqS = gq.reshape(F, Nc, L, 3), gqS.reshape(F, Nc, L, 3)
    t, tS = tq[:, 0].clone(), tqS[:, 0].clone()                                      # the gather's order: images ascending, then the corners
    for c in range(1, Nc):
        t += tq[:, c]
        tS += tqS[:, c]
    for k in range(3):      # (a corner of weight 0 adds 0 to the value and to the scale)
        idx = torch.as_tensor(np.asarray(vtx[k], dtype=np.int64))
        gx.index_add_(1, idx, b[k][None, :, None] * t)
        gxS.index_add_(1, idx, b[k].abs()[None, :, None] * tS)
    out['grad_x'], out['grad_mvp'], out['grad_q'] = (gx, gxS), (gm, gmS), (gq, gqS)
    return out


def dtype_scalar(v, dtype):
    return torch.tensor(v, dtype=dtype)


def landmark_plain(x, mvp, vtx, bary, w, obs, weight, H, W, c=None):
    """The whole term as one differentiable torch expression (for torch.autograd), straight from the rule's text: the projection by
    posw @ mtx.T, the Charbonnier value in its textbook form 2 c^2 (sqrt(1 + s / c^2) - 1)."""
    F, N, L = x.shape[0], obs.shape[0], obs.shape[1]
    Nc = N // F
    b = torch.as_tensor(np.asarray(bary, dtype=np.float32)).to(x.dtype)
    om = torch.ones(L, dtype=x.dtype) if w is None else torch.as_tensor(w).to(x.dtype)
    q = sum(b[k][None, :, None] * x[:, torch.as_tensor(np.asarray(vtx[k], dtype=np.int64))] for k in range(3))     # [F,L,3]
    qw = torch.cat([q, torch.ones_like(q[..., :1])], dim=-1).repeat_interleave(Nc, dim=0)
    p = torch.matmul(qw, mvp.transpose(1, 2))                                         # [N,L,4]
    kap = obs[..., 2]
    live = (kap > 0) & (om[None] > 0) & (p[..., 3] > W_MIN)
    pw = torch.where(live, p[..., 3], torch.ones_like(kap))
    u = (p[..., 0] / pw * 0.5 + 0.5) * W - 0.5
    v = (p[..., 1] / pw * 0.5 + 0.5) * H - 0.5
    us, vs = (torch.where(live, obs[..., i], torch.zeros_like(kap)) for i in (0, 1))      # (what is not live is not read)
    s = (u - us) ** 2 + (v - vs) ** 2
    rho = s if c is None else 2.0 * c * c * (torch.sqrt(1.0 + s / (c * c)) - 1.0)
    e = torch.where(live, om[None] * kap * rho, torch.zeros_like(s))
    return (weight / F) * (e.reshape(F, -1).sum(dim=1) / (Nc * L)).sum()


def mean_live_residual(res):
    """The mean |residual| (pixels) over the live entries of res [...,2] (NaN where not live)."""
    r = _c(res, torch.float64).reshape(-1, 2)
    ok = ~torch.isnan(r[:, 0])
    return float(r[ok].norm(dim=1).mean())

"""Statement on the CPU of the per-frame blend-weight solve ("Expression solve rule"; csrc/landmark_expr.hip
k_landmark_expr): the yardstick of tests/test_gpu_expr.py, itself checked on the CPU by tests/test_expr_ref.py.  Nothing here imports
fpc_diffrend_amd.

The rule is stated twice by ONE text, as tests/pose_ref.py states the pose solve: `dtype` float64 is the rule in float64 throughout;
float32 is the kernel's own precision and order -- the landmark basis A, the point, an entry and the per-landmark sums S_l, s_l over the
cameras in float32, operation for operation and vectorised over the entries, then H, g, the cost C, the Cholesky factorisation and both
substitutions in float64 in the kernel's order.  Every sum of a pass comes as a (value, S) pair, S the same formula over absolute
values (pose_ref.SV's algebra), so that an error can be read in units of 2^-24 of the entry's own scale."""
import math

import numpy as np
import torch

from fitstep_ref import _c
from pose_ref import SV, W_MIN, _ksum, _sqrt

S_TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]      # the six entries of a landmark's block S_l, in the kernel's order


def n_packed(Kb):
    return Kb * (Kb + 1) // 2


def basis_rows(B, vtx, bary, dtype):
    """A [L,3,Kb] as SV: A[l,a,k] = (bary_0 B[3 vtx_0 + a, k] + bary_1 B[3 vtx_1 + a, k]) + bary_2 B[3 vtx_2 + a, k]."""
    Bm = _c(B, dtype)
    Bm = Bm.reshape(-1, 3, Bm.shape[1])
    br = torch.as_tensor(np.asarray(bary, dtype=np.float32)).to(dtype)
    rows = [SV(Bm[torch.as_tensor(np.asarray(vtx[k], dtype=np.int64))]) for k in range(3)]             # [L,3,Kb]
    b = [SV(br[k][:, None, None]) for k in range(3)]
    return (b[0] * rows[0] + b[1] * rows[1]) + b[2] * rows[2]


def normal(x, mvp, basis, vtx, bary, w, obs, wts, w_in, H, W, inv_c=0.0, dtype=torch.float64):
    """One pass at the weights wts [F,Kb] for the meshes x [F,V,3] AT the weights w_in [F,Kb]: mvp [F Nc,4,4], basis [3V,Kb], vtx / bary
    [3,L], w [L] or None, obs [F Nc,L,3]; inv_c = 1 / c as the float32 the kernel is handed (0: L2).
      q = sum_k bary_k x[vtx_k] + A (wts - w_in),  p = mvp (q, 1),  u, v, live, r, rho, d as the Landmark rule;
      g_u = (W / 2) / pw (M_x - (px / pw) M_w),  g_v alike;  w_e = omega kappa d;  per landmark over the cameras ascending
      S_l = sum w_e (g_u g_u^T + g_v g_v^T),  s_l = sum w_e (g_u r_u + g_v r_v);  then in float64 over l ascending
      H = sum_l A_l^T S_l A_l (packed lower triangle, row-major),  g = sum_l A_l^T s_l;  E = sum omega kappa rho over the live entries.
    -> dict 'H' [F,NT], 'g' [F,Kb], 'E' [F] of (value, S) -- H and g float64 --; 'n' [F]; 'live' [F,Nc,L]; 'res' [F,Nc,L,2] (NaN where
    not live), 'resS' its scale (0 where not live), 'wk' [F,Nc,L] = omega kappa (0 where not live); 'Sl' [F,L,6], 'sl' [F,L,3] of (value, S); 'A' [L,3,Kb] (value); 'G' [F,Nc,L,2,3] = (g_u, g_v)."""
    xx, mm, oo = _c(x, dtype), _c(mvp, dtype), _c(obs, dtype)
    wt, wi = _c(wts, dtype), _c(w_in, dtype)
    F, Kb = wt.shape
    N, L = oo.shape[0], oo.shape[1]
    Nc = N // F
    assert N == F * Nc and mm.shape == (N, 4, 4) and wi.shape == (F, Kb)
    oo, mm = oo.reshape(F, Nc, L, 3), mm.reshape(F, Nc, 4, 4)
    br = torch.as_tensor(np.asarray(bary, dtype=np.float32)).to(dtype)
    om = torch.ones(L, dtype=dtype) if w is None else _c(torch.as_tensor(w), dtype)
    ic = float(np.float32(inv_c))
    A = basis_rows(basis, vtx, bary, dtype)
    dw = wt - wi                                                                                       # [F,Kb]
    dv, dS = torch.zeros(F, L, 3, dtype=dtype), torch.zeros(F, L, 3, dtype=dtype)
    for k in range(Kb):      # A_l (w' - w_in), k ascending
        dv = dv + A.v[None, :, :, k] * dw[:, None, None, k]
        dS = dS + A.s[None, :, :, k] * dw[:, None, None, k].abs()
    corner = [xx[:, torch.as_tensor(np.asarray(vtx[k], dtype=np.int64))] for k in range(3)]            # [F,L,3]
    sv = lambda v: SV(v)
    p = [(sv(br[0][None, None, :]) * sv(corner[0][..., i][:, None]) + sv(br[1][None, None, :]) * sv(corner[1][..., i][:, None]))
         + sv(br[2][None, None, :]) * sv(corner[2][..., i][:, None]) for i in range(3)]                # [F,1,L]
    q = [p[i] + SV(dv[..., i][:, None], dS[..., i][:, None]) for i in range(3)]
    Mm = lambda r, k: sv(mm[:, :, r, k][:, :, None])                                                   # [F,Nc,1]
    px, py, pw = (((Mm(r, 0) * q[0] + Mm(r, 1) * q[1]) + Mm(r, 2) * q[2]) + Mm(r, 3) for r in (0, 1, 3))
    us, vs, kap = oo[..., 0], oo[..., 1], oo[..., 2]
    live = (kap > 0) & (om[None, None] > 0) & (pw.v > W_MIN)
    one, zero = torch.ones_like(pw.v), torch.zeros_like(pw.v)
    sw = SV(torch.where(live, pw.v, one), torch.where(live, pw.s, one))
    hw, hh = 0.5 * W, 0.5 * H
    nx, ny = px / sw, py / sw
    us0, vs0 = torch.where(live, us, zero), torch.where(live, vs, zero)                                # (what is not live is not read)
    ru = ((nx * 0.5 + 0.5) * (2.0 * hw) - 0.5) - sv(us0)
    rv = ((ny * 0.5 + 0.5) * (2.0 * hh) - 0.5) - sv(vs0)
    s = ru * ru + rv * rv
    if ic > 0.0:
        zu, zv = ru.v * ic, rv.v * ic
        h = _sqrt(1.0 + (zu * zu + zv * zv))
        rho = SV((2.0 * s.v) / (1.0 + h), (2.0 * s.s) / (1.0 + h))
        d = SV(1.0 / h, 1.0 / h + (ic * ic) * (ru.v.abs() * ru.s + rv.v.abs() * rv.s) / (h * h * h))
    else:
        rho, d = s, SV(torch.ones_like(s.v))
    wk = sv(om[None, None] * kap)
    we = wk * d
    ku, kv = sv(torch.as_tensor(hw, dtype=dtype)) / sw, sv(torch.as_tensor(hh, dtype=dtype)) / sw
    gu = [ku * (Mm(0, i) - nx * Mm(3, i)) for i in range(3)]
    gv = [kv * (Mm(1, i) - ny * Mm(3, i)) for i in range(3)]

    def over_cameras(term):      # [F,Nc,L] -> [F,L], the cameras ascending
        v, S = torch.where(live, term.v, zero), torch.where(live, term.s, zero)
        av, aS = v[:, 0].clone(), S[:, 0].clone()
        for c in range(1, Nc):
            av, aS = av + v[:, c], aS + S[:, c]
        return av, aS

    Sl = [over_cameras(we * (gu[i] * gu[j] + gv[i] * gv[j])) for i, j in S_TRI]
    sl = [over_cameras(we * (gu[i] * ru + gv[i] * rv)) for i in range(3)]
    el = over_cameras(wk * rho)
    E = (_ksum(el[0]), el[1].sum(dim=1))
    # ---- float64 from here on, in both statements ----
    Av, As = A.v.double(), A.s.double()                                                                # [L,3,Kb]
    full = {(i, j): k for k, (i, j) in enumerate(S_TRI)}
    full.update({(j, i): k for (i, j), k in list(full.items())})
    Hv, Hs = torch.zeros(F, Kb, Kb, dtype=torch.float64), torch.zeros(F, Kb, Kb, dtype=torch.float64)
    gvv, gss = torch.zeros(F, Kb, dtype=torch.float64), torch.zeros(F, Kb, dtype=torch.float64)
    for l in range(L):
        for (val, a, out, gout) in ((0, Av, Hv, gvv), (1, As, Hs, gss)):
            Sm = [[Sl[full[(r, c)]][val][:, l].double() for c in range(3)] for r in range(3)]          # [F] each
            al = a[l]                                                                                  # [3,Kb]
            u = [(Sm[r][0][:, None] * al[0][None] + Sm[r][1][:, None] * al[1][None]) + Sm[r][2][:, None] * al[2][None] for r in range(3)]  # [F,Kb]: S_l a_i
            out += (u[0][:, :, None] * al[0][None, None] + u[1][:, :, None] * al[1][None, None]) + u[2][:, :, None] * al[2][None, None]
            sm = [sl[r][val][:, l].double() for r in range(3)]
            gout += (al[0][None] * sm[0][:, None] + al[1][None] * sm[1][:, None]) + al[2][None] * sm[2][:, None]
    ti = torch.tril_indices(Kb, Kb)                                                                    # row-major: (i, k <= i) at i (i + 1) / 2 + k
    nan = torch.full_like(zero, float('nan'))
    return {'H': (Hv[:, ti[0], ti[1]], Hs[:, ti[0], ti[1]]), 'g': (gvv, gss), 'E': E, 'n': live.reshape(F, -1).sum(dim=1), 'live': live,
            'res': torch.stack([torch.where(live, ru.v, nan), torch.where(live, rv.v, nan)], dim=-1),
            'resS': torch.stack([torch.where(live, ru.s, zero), torch.where(live, rv.s, zero)], dim=-1), 'wk': torch.where(live, wk.v, zero),
            'Sl': (torch.stack([v for v, _ in Sl], dim=-1), torch.stack([S for _, S in Sl], dim=-1)),
            'sl': (torch.stack([v for v, _ in sl], dim=-1), torch.stack([S for _, S in sl], dim=-1)), 'A': A.v,
            'G': torch.stack([torch.stack([c.v.expand(F, Nc, L) for c in gu], dim=-1), torch.stack([c.v.expand(F, Nc, L) for c in gv], dim=-1)], dim=-2)}


def ridge_scale(ridge, Nc, L):
    """rs = gamma Nc L in float64, gamma as the float32 the kernel is handed."""
    return (float(np.float32(ridge)) * float(Nc)) * float(L)


def cost(E, rs, w):
    """C = E + rs sum_k w_k^2 in float64, k ascending; E a float, w [Kb] (float32 or float64)."""
    s = 0.0
    for v in np.asarray(w, dtype=np.float64):
        s = s + v * v
    return float(E) + rs * s


def residuals_plain(wts, w_in, pts, A, mvp, obs, H, W):
    """(u - u*, v - v*) [Nc,L,2] of ONE frame as a differentiable torch expression of its weights, straight from the rule's text (for
    torch.autograd): pts [L,3] the landmark points at w_in, A [L,3,Kb], mvp [Nc,4,4], obs [Nc,L,3]."""
    q = pts + torch.einsum('lak,k->la', A, wts - w_in)
    p = torch.einsum('crk,lk->clr', mvp[:, :, :3], q) + mvp[:, None, :, 3]
    u = (p[..., 0] / p[..., 3] * 0.5 + 0.5) * W - 0.5
    v = (p[..., 1] / p[..., 3] * 0.5 + 0.5) * H - 0.5
    return torch.stack([u - obs[..., 0], v - obs[..., 1]], dim=-1)


def trial(Hp, g, lam, rs, w, round32=True):
    """One damped step in float64 from the packed H [NT] and g [Kb] at the weights w [Kb] -> w' (rounded to float32), or None for a
    rejected trial (a pivot that is not positive, a step that is not finite).  M = H + rs I, damped M + lam diag M, right-hand side
    -(g + rs w); a weight with M_kk == 0 keeps its row and column at the identity and its right-hand side at 0.  Right-looking
    Cholesky: column j is finished, then every remaining entry takes its one update; L y = rhs by columns (ascending j), L^T delta = y
    by columns (descending j).  numpy's elementwise float64 operations are the kernel's, one rounding each."""
    Kb = int(g.shape[0])
    w64 = np.asarray(w, dtype=np.float64)
    M = np.zeros((Kb, Kb), dtype=np.float64)
    M[np.tril_indices(Kb)] = np.asarray(Hp, dtype=np.float64)
    M = M + np.tril(M, -1).T
    idx = np.arange(Kb)
    m = M[idx, idx] + rs
    dead = m == 0.0
    M[idx, idx] = m + lam * m
    M[dead, :] = 0.0
    M[:, dead] = 0.0
    M[dead, dead] = 1.0
    rhs = np.where(dead, 0.0, -(np.asarray(g, dtype=np.float64) + rs * w64))
    diag = np.zeros(Kb)
    for j in range(Kb):
        dj = M[j, j]
        if not dj > 0.0:
            return None
        r = math.sqrt(dj)
        diag[j] = r
        M[j + 1:, j] = M[j + 1:, j] / r
        col = M[j + 1:, j]
        M[j + 1:, j + 1:] = M[j + 1:, j + 1:] - col[:, None] * col[None, :]
    y = np.zeros(Kb)
    for j in range(Kb):
        y[j] = rhs[j] / diag[j]
        rhs[j + 1:] = rhs[j + 1:] - M[j + 1:, j] * y[j]
    delta = np.zeros(Kb)
    for j in range(Kb - 1, -1, -1):
        delta[j] = y[j] / diag[j]
        y[:j] = y[:j] - M[j, :j] * delta[j]
    if not np.isfinite(delta).all():
        return None
    out = w64 + delta
    return out.astype(np.float32) if round32 else out


def solve(x, mvp, basis, vtx, bary, w, obs, w_in, H, W, inv_c=0.0, ridge=0.0, iters=20, lambda0=1e-3, dtype=torch.float64, round32=True):
    """The solver loop of the rule on every frame, from the weights w_in [F,Kb] at which the meshes x stand: -> (weights [F,Kb] float32,
    info [F,4] float64 = (C at the input, C at the returned weights, live entries there, accepted trials), trace: per frame the list of
    trials (C before, C of the trial or None, live before, live of the trial, accepted))."""
    wt = torch.float32 if round32 else torch.float64
    w0 = _c(w_in, wt).clone()
    w_out = w0.clone()
    F, Kb = w0.shape
    Nc, L = mvp.shape[0] // F, obs.shape[1]
    rs = ridge_scale(ridge, Nc, L)
    info, trace = torch.zeros(F, 4, dtype=torch.float64), []
    for f in range(F):
        def sums(wf):
            r = normal(x[f:f + 1], mvp[f * Nc:(f + 1) * Nc], basis, vtx, bary, w, obs[f * Nc:(f + 1) * Nc], wf[None], w0[f:f + 1], H, W, inv_c, dtype)
            return r['H'][0][0].numpy(), r['g'][0][0].numpy(), cost(r['E'][0][0].item(), rs, wf.numpy()), int(r['n'][0])
        wf = w0[f].clone()
        Hp, g, C, n = sums(wf)
        info[f, 0], lam, accepted, tr = C, float(np.float32(lambda0)), 0, []
        for _ in range(iters if n >= 3 else 0):
            new = trial(Hp, g, lam, rs, wf.numpy(), round32)
            if new is None:
                tr.append((C, None, n, None, False))
                lam = min(lam * 10.0, 1e9)
                continue
            wn = torch.from_numpy(new)
            H2, g2, C2, n2 = sums(wn)
            keep = n2 >= n and C2 < C
            tr.append((C, C2, n, n2, keep))
            if keep:
                wf, Hp, g, C, n, accepted = wn, H2, g2, C2, n2, accepted + 1
                lam = max(lam / 10.0, 1e-9)
            else:
                lam = min(lam * 10.0, 1e9)
        if accepted:
            w_out[f] = wf
        info[f, 1], info[f, 2], info[f, 3] = C, n, accepted
        trace.append(tr)
    return w_out, info, trace


def mean_residual(x, mvp, basis, vtx, bary, w, obs, wts, w_in, H, W):
    """The mean live |residual| in pixels at the weights wts, float64."""
    r = normal(x, mvp, basis, vtx, bary, w, obs, wts, w_in, H, W)['res'].reshape(-1, 2)
    ok = ~torch.isnan(r[:, 0])
    return float(r[ok].norm(dim=1).mean())

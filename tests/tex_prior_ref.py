"""float64 statement on the CPU of the texture prior ("Texture prior rule"; csrc/tex_prior.hip k_tex_prior): the yardstick
of tests/test_gpu_tex_prior.py, itself checked on the CPU by tests/test_tex_prior_ref.py.  Nothing here imports fpc_diffrend_amd.

The convention is tests/fitstep_ref.py's and tests/motion_ref.py's: every function evaluates in `dtype` (float64 by default; float32
gives "the same formula in float32 by torch") and returns (value, S) pairs, S the same formula with every input replaced by its absolute
value and every subtraction by an addition: t_p - t_q gives |t_p| + |t_q| -- neighbouring texels are close, so the differences cancel
for real, and the cancellation is charged to the scale, not to the kernel."""
import numpy as np
import torch

from fitstep_ref import _c


def pair_weights(Ht, Wt, smooth_w, dtype=torch.float64):
    """(m_h [Ht,Wt-1], m_v [Ht-1,Wt]): the weight min(w_p, w_q) of every horizontal pair (i,j)-(i,j+1) and vertical pair (i,j)-(i+1,j);
    smooth_w None: 1.  There is no pair across the border."""
    w = torch.ones(Ht, Wt, dtype=dtype) if smooth_w is None else _c(smooth_w, dtype)
    assert tuple(w.shape) == (Ht, Wt)
    return torch.minimum(w[:, :-1], w[:, 1:]), torch.minimum(w[:-1], w[1:])


def term_flags(Ht, Wt, w_smooth, w_anchor, has_anchor, smooth_w=None, anchor_w=None):
    """From the weights alone: (texel [Ht,Wt] bool: the texel's gradient has a term, smooth: part[0] has one, anchor: part[1] has one)."""
    mh, mv = pair_weights(Ht, Wt, smooth_w)
    ts = torch.zeros(Ht, Wt, dtype=torch.bool)
    ts[:, :-1] |= mh > 0; ts[:, 1:] |= mh > 0
    ts[:-1] |= mv > 0; ts[1:] |= mv > 0
    ta = torch.zeros(Ht, Wt, dtype=torch.bool)
    if has_anchor:
        ta = torch.ones(Ht, Wt, dtype=torch.bool) if anchor_w is None else _c(anchor_w, torch.float64) > 0
    texel = (ts if w_smooth > 0 else torch.zeros_like(ts)) | (ta if w_anchor > 0 else torch.zeros_like(ta))
    return texel, bool(ts.any()), bool(ta.any())


def tex_prior(t, w_smooth, w_anchor, anchor=None, smooth_w=None, anchor_w=None, inv_c=0.0, dtype=torch.float64):
    """t, anchor [Ht,Wt,C]; smooth_w, anchor_w [Ht,Wt] or None (1); inv_c = 1 / c as the float32 the kernel is handed (0: L2).
      s_pq = |t_p - t_q|^2,  rho(s) = s | 2 s / (1 + sqrt(1 + s / c^2)),  rho' = 1 | 1 / sqrt(1 + s / c^2),  m_pq = min(w_p, w_q)
      part = (sum_pairs m rho, sum_p wa_p |t_p - a_p|^2) / (Ht Wt),   value = w_smooth part[0] + w_anchor part[1]
      grad_p = 2 / (Ht Wt) [ w_smooth sum_q m_pq rho' (t_p - t_q) + w_anchor wa_p (t_p - a_p) ]
    A weight of 0 is a select: the pair or texel contributes exactly 0 whatever the texels hold.
    -> dict 'part' [2], 'value' [1], 'grad' [Ht,Wt,C] of (value, S), and 'zeros': the number of entries of (grad, part, value) without a
    term, from the weights alone (term_flags)."""
    tt = _c(t, dtype)
    Ht, Wt, C = tt.shape
    n = float(Ht * Wt)
    ic = float(np.float32(inv_c))
    mh, mv = pair_weights(Ht, Wt, smooth_w, dtype)
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    g, gS = z(Ht, Wt, C), z(Ht, Wt, C)
    smooth, smoothS = z(()), z(())
    for axis, m in ((1, mh), (0, mv)):
        p, q = (tt[:, :-1], tt[:, 1:]) if axis == 1 else (tt[:-1], tt[1:])
        d, dS = p - q, p.abs() + q.abs()
        s, sS = (d * d).sum(dim=2), (dS * dS).sum(dim=2)
        if ic > 0.0:
            h = torch.sqrt(1.0 + s * (ic * ic))
            rho, rhoS, dr = 2.0 * s / (1.0 + h), 2.0 * sS / (1.0 + h), 1.0 / h       # (the form without the cancellation; equal to the rule's)
        else:
            rho, rhoS, dr = s, sS, torch.ones_like(s)
        live = m > 0
        smooth = smooth + torch.where(live, m * rho, torch.zeros_like(s)).sum()
        smoothS = smoothS + torch.where(live, m * rhoS, torch.zeros_like(s)).sum()
        b = torch.where(live[..., None], (m * dr)[..., None] * d, torch.zeros_like(d))
        bS = torch.where(live[..., None], (m * dr)[..., None] * dS, torch.zeros_like(d))
        if axis == 1:
            g[:, :-1] += b; g[:, 1:] -= b; gS[:, :-1] += bS; gS[:, 1:] += bS
        else:
            g[:-1] += b; g[1:] -= b; gS[:-1] += bS; gS[1:] += bS
    cs, ca = 2.0 * float(w_smooth) / n, 2.0 * float(w_anchor) / n
    g, gS = cs * g, cs * gS
    anch, anchS = z(()), z(())
    if anchor is not None:
        aa = _c(anchor, dtype)
        wa = torch.ones(Ht, Wt, dtype=dtype) if anchor_w is None else _c(anchor_w, dtype)
        e, eS = tt - aa, tt.abs() + aa.abs()
        live = wa > 0
        anch = torch.where(live, wa * (e * e).sum(dim=2), z(Ht, Wt)).sum()
        anchS = torch.where(live, wa * (eS * eS).sum(dim=2), z(Ht, Wt)).sum()
        g = g + ca * torch.where(live[..., None], wa[..., None] * e, torch.zeros_like(e))
        gS = gS + ca * torch.where(live[..., None], wa[..., None] * eS, torch.zeros_like(e))
    part, partS = torch.stack([smooth, anch]) / n, torch.stack([smoothS, anchS]) / n
    value = float(w_smooth) * part[0] + float(w_anchor) * part[1]
    valueS = float(w_smooth) * partS[0] + float(w_anchor) * partS[1]
    texel, any_s, any_a = term_flags(Ht, Wt, w_smooth, w_anchor, anchor is not None, smooth_w, anchor_w)
    zeros = (int((~texel).sum()) * C, int(not any_s) + int(not any_a), int(not ((any_s and w_smooth > 0) or (any_a and w_anchor > 0))))
    return {'part': (part, partS), 'value': (value.reshape(1), valueS.reshape(1)), 'grad': (g, gS), 'zeros': zeros}


def tex_prior_plain(t, w_smooth, w_anchor, anchor=None, smooth_w=None, anchor_w=None, c=None):
    """The whole term as one differentiable torch expression (for torch.autograd, and in float32 on a GPU the yardstick of the timing),
    straight from the rule's text: the Charbonnier value in its textbook form 2 c^2 (sqrt(1 + s / c^2) - 1), the weights as factors."""
    Ht, Wt, _ = t.shape
    rho = (lambda s: s) if c is None else (lambda s: 2.0 * c * c * (torch.sqrt(1.0 + s / (c * c)) - 1.0))
    sh, sv = ((t[:, :-1] - t[:, 1:]) ** 2).sum(dim=2), ((t[:-1] - t[1:]) ** 2).sum(dim=2)
    if smooth_w is None:
        smooth = rho(sh).sum() + rho(sv).sum()
    else:
        w = smooth_w.to(t.dtype)
        smooth = (torch.minimum(w[:, :-1], w[:, 1:]) * rho(sh)).sum() + (torch.minimum(w[:-1], w[1:]) * rho(sv)).sum()
    value = w_smooth * smooth / (Ht * Wt)
    if anchor is not None:
        e = ((t - anchor.to(t.dtype)) ** 2).sum(dim=2)
        value = value + w_anchor * (e if anchor_w is None else anchor_w.to(t.dtype) * e).sum() / (Ht * Wt)
    return value


def neighbour_msd(t, texels):
    """The mean squared difference between neighbouring texels of t [Ht,Wt,C] over the pairs whose two ends are both in `texels`
    [Ht,Wt] bool (float64)."""
    tt, k = _c(t, torch.float64), _c(texels, torch.bool)
    sh, sv = ((tt[:, :-1] - tt[:, 1:]) ** 2).sum(dim=2), ((tt[:-1] - tt[1:]) ** 2).sum(dim=2)
    kh, kv = k[:, :-1] & k[:, 1:], k[:-1] & k[1:]
    return float((sh[kh].sum() + sv[kv].sum()) / max(int(kh.sum()) + int(kv.sum()), 1))


def dilate3(cover):
    """numpy: the 3 x 3 maximum of a [Ht,Wt] bool map, no wrap at the border."""
    c = np.asarray(cover, dtype=bool)
    p = np.pad(c, 1)
    out = np.zeros_like(c)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + c.shape[0], dx:dx + c.shape[1]]
    return out

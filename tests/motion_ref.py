"""float64 statement on the CPU of the motion term ("Motion rule"; csrc/mesh_reg.hip k_motion_penalty): the yardstick of
tests/test_gpu_motion.py, itself checked on the CPU by tests/test_motion_ref.py.  Nothing here imports fpc_diffrend_amd.

The convention is tests/fitstep_ref.py's and tests/rest_ref.py's: every function evaluates in `dtype` (float64 by default; float32 gives
"the same formula in float32 by torch") and returns (value, S) pairs, S the same formula with every input replaced by its absolute value
and every subtraction by an addition.  Every subtraction contributes the absolute values of its OPERANDS: x_{f-1} - 2 x_f + x_{f+1}
gives |x_{f-1}| + 2 |x_f| + |x_{f+1}| -- positions sit at y + 170, so the differences cancel for real, and the cancellation is charged
to the scale, not to the kernel."""
import numpy as np
import torch

from fitstep_ref import _c


def stencil_flags(F, frame_t, order):
    """m [F] bool: the stencil of frame f is valid.  frame_t: a sequence / tensor of F frame numbers, or None (consecutive)."""
    t = torch.arange(F, dtype=torch.int64) if frame_t is None else torch.as_tensor(frame_t, dtype=torch.int64).reshape(-1).cpu()
    assert t.numel() == F
    m = torch.zeros(F, dtype=torch.bool)
    if F >= 2:
        step = (t[1:] - t[:-1]) == 1                      # [F-1]: the frames f and f + 1 are one frame number apart
        if order == 1:
            m[:-1] = step
        elif F >= 3:
            m[1:-1] = step[:-1] & step[1:]
    return m


def zero_entries(F, V, frame_t, order):
    """The number of entries of the gradient [F,V,3] (with all vertex weights > 0) and of per [F] that no valid stencil reaches."""
    m = stencil_flags(F, frame_t, order)
    reach = torch.zeros(F, dtype=torch.bool)
    for f in torch.nonzero(m).reshape(-1).tolist():
        reach[f] = True
        if order == 2:
            reach[f - 1] = reach[f + 1] = True
        else:
            reach[f + 1] = True
    return int((~reach).sum()) * V * 3, int((~m).sum())


def motion(x, weight, frame_t=None, order=2, inv_c=0.0, vertex_w=None, dtype=torch.float64):
    """x [F,V,3]; inv_c = 1 / c as the float32 the kernel is handed (0: L2); vertex_w [V] or None.
      a_f = x_{f-1} - 2 x_f + x_{f+1} (order 2) | x_{f+1} - x_f (order 1),  s = |a|^2,  rho(s) = s | 2 c^2 (sqrt(1 + s / c^2) - 1),
      per_f = m_f / V sum_v w_v rho,  value = weight / F sum_f per_f,
      grad_f = 2 weight / (F V) (b_{f-1} - 2 b_f + b_{f+1}) | (b_{f-1} - b_f),  b = m w rho'(s) a,  rho' = 1 | 1 / sqrt(1 + s / c^2).
    -> dict 'per', 'value', 'grad' of (value, S), and 'zeros': (gradient entries without a term, per entries without a term)."""
    assert order in (1, 2)
    xx = _c(x, dtype)
    F, V = xx.shape[0], xx.shape[1]
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    w = torch.ones(V, dtype=dtype) if vertex_w is None else _c(vertex_w, dtype)
    m = stencil_flags(F, frame_t, order)
    ic = float(np.float32(inv_c))
    a, aS = z(F, V, 3), z(F, V, 3)                                          # the stencil centred on (order 1: starting at) frame f
    if order == 2 and F >= 3:
        a[1:-1] = xx[:-2] - 2.0 * xx[1:-1] + xx[2:]
        aS[1:-1] = xx[:-2].abs() + 2.0 * xx[1:-1].abs() + xx[2:].abs()
    elif order == 1 and F >= 2:
        a[:-1] = xx[1:] - xx[:-1]
        aS[:-1] = xx[1:].abs() + xx[:-1].abs()
    mm = m.to(dtype)[:, None]
    s, sS = (a * a).sum(dim=2), (aS * aS).sum(dim=2)                        # [F,V]
    if ic > 0.0:
        h = torch.sqrt(1.0 + s * (ic * ic))
        rho, d = 2.0 * s / (1.0 + h), 1.0 / h                               # (the form without the cancellation; equal to the rule's)
        rhoS = 2.0 * sS / (1.0 + h)
    else:
        rho, d, rhoS = s, torch.ones_like(s), sS
    per, perS = mm[:, 0] * (w[None] * rho).sum(dim=1) / V, mm[:, 0] * (w[None] * rhoS).sum(dim=1) / V
    q = mm * w[None] * d                                                    # [F,V]: m w rho'
    b, bS = q[..., None] * a, q[..., None] * aS
    g, gS = z(F, V, 3), z(F, V, 3)
    if order == 2:
        g -= 2.0 * b; gS += 2.0 * bS
        g[:-1] += b[1:]; gS[:-1] += bS[1:]
        g[1:] += b[:-1]; gS[1:] += bS[:-1]
    else:
        g -= b; gS += bS
        g[1:] += b[:-1]; gS[1:] += bS[:-1]
    c = 2.0 * float(weight) / (F * V)
    wf = float(weight) / F
    res = {'per': (per, perS), 'value': (wf * per.sum(), abs(wf) * perS.sum()), 'grad': (c * g, abs(c) * gS)}
    if vertex_w is None:
        res['zeros'] = zero_entries(F, V, frame_t, order)
    else:      # a vertex of weight 0 has no term either
        nz = int((w == 0).sum())
        zg, zp = zero_entries(F, V, frame_t, order)
        res['zeros'] = (zg + (F * V * 3 - zg) // V * nz, zp if nz < V else F)
    return res


def motion_plain(x, weight, frame_t=None, order=2, c=None, vertex_w=None):
    """The whole term as one differentiable torch expression (for torch.autograd), straight from the rule's text: the Charbonnier value
    in its textbook form 2 c^2 (sqrt(1 + s / c^2) - 1)."""
    F, V = x.shape[0], x.shape[1]
    m = stencil_flags(F, frame_t, order).to(x.dtype)
    if F < order + 1:
        return x.sum() * 0.0
    if order == 2:
        a, mk = x[:-2] - 2.0 * x[1:-1] + x[2:], m[1:-1]
    else:
        a, mk = x[1:] - x[:-1], m[:-1]
    s = (a * a).sum(dim=2)
    rho = s if c is None else 2.0 * c * c * (torch.sqrt(1.0 + s / (c * c)) - 1.0)
    if vertex_w is not None:
        rho = rho * vertex_w[None].to(x.dtype)
    return (weight / F) * (mk * rho.sum(dim=1) / V).sum()


def rms_acceleration(x):
    """sqrt(mean over frames 1 .. F - 2, vertices of |x_{f-1} - 2 x_f + x_{f+1}|^2) of x [F,V,3]."""
    xx = _c(x, torch.float64)
    a = xx[:-2] - 2.0 * xx[1:-1] + xx[2:]
    return float(torch.sqrt((a * a).sum(dim=2).mean()))

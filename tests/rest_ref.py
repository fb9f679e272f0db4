"""float64 statements on the CPU of the two rest-shape regularisers ("Rest Laplacian rule" and "Stretch rule";
csrc/mesh_reg.hip k_lap_penalty_fwd<true>, k_stretch_penalty): the yardstick of tests/test_gpu_rest.py, itself checked on the CPU by
tests/test_rest_ref.py.  Nothing here imports fpc_diffrend_amd.

The convention is tests/fitstep_ref.py's: every function evaluates in `dtype` (float64 by default; float32 gives "the same formula in
float32 by torch") and returns (value, S) pairs, S the same formula with every input replaced by its absolute value and every
subtraction by an addition.  Every subtraction contributes the absolute values of its OPERANDS: `len - l` gives len + l, `x_n - x_v`
gives |x_n| + |x_v| -- the cancellation of two nearly equal numbers (an edge at its rest length, two vertices 170 units from the
origin) is charged to the scale, not to the kernel."""
import numpy as np
import torch

from fitstep_ref import _c


def ring_table(faces, n_vertices):
    """The padded one-ring table of a triangle list as MeshTopology lays it out: nbr [V,Dmax] int64 (pads = V), rings filled in the
    order of the sorted unique edges."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    e = np.unique(np.sort(e, axis=1), axis=0)
    deg = np.bincount(e.reshape(-1), minlength=n_vertices)
    nbr = np.full((n_vertices, max(int(deg.max()) if deg.size else 0, 1)), n_vertices, dtype=np.int64)
    fill = np.zeros(n_vertices, dtype=np.int64)
    for a, b in e:
        nbr[a, fill[a]] = b; fill[a] += 1
        nbr[b, fill[b]] = a; fill[b] += 1
    return torch.from_numpy(nbr)


def rest_lengths(nbr, x_rest):
    """rest_len [V,D] float32 (vertex-major here; the kernel's table is its transpose): the float32 rest positions, the norm in float64,
    one rounding; pads 0.  -> (rest_len, number of edges)."""
    x = x_rest.detach().to('cpu', torch.float32).reshape(-1, 3).double()
    V = x.shape[0]
    real = nbr < V
    d = x[torch.where(real, nbr, torch.zeros_like(nbr))] - x[:, None]
    length = torch.where(real, d.norm(dim=2), torch.zeros((), dtype=torch.float64))
    return length.float(), int(real.sum()) // 2


# ---------------------------------------------------------------------------------------------------------------------
# rest Laplacian: d = L x - r on a GIVEN r (the float32 table the kernel read)
# ---------------------------------------------------------------------------------------------------------------------

def rest_differentials(fl, x, rest_lap, dtype=torch.float64):
    """d_{f,v} = (L x_f)_v - r_v for x [F,V,3], r [V,3] -> (value, S);  fl a fitstep_ref.FaceLaplacian."""
    lx, S = fl.apply(x, dtype=dtype)
    r = _c(rest_lap, dtype)[None]
    return lx - r, S + r.abs()


def rest_penalty_plain(x, Ldense, rest_lap, weight):
    """The whole term as one differentiable torch expression (for torch.autograd)."""
    d = torch.matmul(Ldense[None], x) - rest_lap[None]
    per = d.norm(dim=2).mean(dim=1)
    return (weight / x.shape[0]) * (per ** 2).sum()


def rest_penalty(fl, x, rest_lap, weight, dtype=torch.float64):
    """per_f = mean_v ||d_{f,v}||, value = weight / F sum_f per_f^2 and d value / d x = L^T y (fitstep_ref.penalty_grad with d as its lap)
    -> dict of (value, S); per and value are sums of positive terms: their scales are themselves."""
    import fitstep_ref as R
    d, _ = rest_differentials(fl, x, rest_lap, dtype)
    per, val = R.penalty_value(d, weight, dtype)
    g, gS = R.penalty_grad(d, per, fl, weight, 1.0, dtype)
    return {'per': (per, per), 'value': (val, val), 'grad': (g, gS)}


# ---------------------------------------------------------------------------------------------------------------------
# stretch
# ---------------------------------------------------------------------------------------------------------------------

def stretch(x, nbr, rest_len, weight, target=0.0, dtype=torch.float64):
    """x [F,V,3], nbr [V,D] (pads = V), rest_len [V,D] or None (then the constant target).
      s = |x_n - x_v| - l,  per_f = 1 / (2 E) sum_v sum_d s^2,  value = weight / F sum_f per_f,
      grad_v = 2 weight / (F E) sum_d (s / len) (x_v - x_n)   (a slot with len = 0 contributes 0);  E = 0: everything 0.
    -> dict 'per', 'value', 'grad' of (value, S)."""
    xx = _c(x, dtype)
    F, V = xx.shape[0], xx.shape[1]
    vs, ds = torch.nonzero(nbr < V, as_tuple=True)                        # the real slots, one entry per (vertex, slot): 2 E of them
    E = vs.numel() // 2
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    if E == 0:
        return {'per': (z(F), z(F)), 'value': (z(()), z(())), 'grad': (z(F, V, 3), z(F, V, 3))}
    ns = nbr[vs, ds]
    xn, xv = xx[:, ns], xx[:, vs]                                         # [F,2E,3]
    e, eS = xn - xv, xn.abs() + xv.abs()
    ln, lnS = e.norm(dim=2), eS.norm(dim=2)                               # [F,2E]
    l = _c(rest_len, dtype)[vs, ds][None] if rest_len is not None else torch.full((), float(np.float32(target)), dtype=dtype)
    s, sS = ln - l, lnS + l.abs()
    per, perS = (s * s).sum(dim=1) / (2.0 * E), (sS * sS).sum(dim=1) / (2.0 * E)
    ok = ln > 0
    safe = torch.where(ok, ln, torch.ones_like(ln))
    q, qS = torch.where(ok, s / safe, z(())), torch.where(ok, sS / safe, z(()))
    c = 2.0 * float(weight) / (F * E)
    g = c * z(F, V, 3).index_add_(1, vs, q[..., None] * (xv - xn))
    gS = abs(c) * z(F, V, 3).index_add_(1, vs, qS[..., None] * eS)
    w = float(weight) / F
    return {'per': (per, perS), 'value': (w * per.sum(), abs(w) * perS.sum()), 'grad': (g, gS)}


def stretch_plain(x, edges, rest_edge_len, weight, target=0.0):
    """The term over the EDGE LIST as one differentiable torch expression: weight / F sum_f mean_edges (|e| - l)^2."""
    d = x[:, edges[:, 0]] - x[:, edges[:, 1]]
    l = rest_edge_len[None] if rest_edge_len is not None else target
    return (weight / x.shape[0]) * ((d.norm(dim=2) - l) ** 2).mean(dim=1).sum()


def edge_list(nbr):
    """[E,2] (a < b) of a ring table."""
    V = nbr.shape[0]
    a = torch.arange(V)[:, None].expand_as(nbr)
    m = (nbr < V) & (a < nbr)
    return torch.stack([a[m], nbr[m]], dim=1)

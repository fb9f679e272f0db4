"""float64 statement on the CPU of the bending term ("Bend rule"; csrc/mesh_reg.hip k_bend_*): the yardstick of
tests/test_gpu_bend.py, itself checked on the CPU by tests/test_bend_ref.py.  Nothing here imports fpc_diffrend_amd.

The convention is tests/rest_ref.py's: every function evaluates in `dtype` (float64 by default; float32 gives "the same formula in
float32 by torch") and returns (value, S) pairs.  S is carried by the rules of tests/rasterize_ref.py (class Q: an input x has S = |x|,
a sum or a difference adds the scales -- every subtraction charges the absolute values of its OPERANDS --, a product is S_a |b| + |a| S_b,
a quotient S_a / |d| + |a / d| S_d / |d|) and tests/norm_ref.py's root, S_x / (2 sqrt x) + sqrt x.  The constant 1 of `1 - cos` and
`1 + cos` has the scale 1, so a degenerate hinge (t = 1 by the rule) has S_t = 1; its gradient has no term: S = 0, exactly 0.
Positions sit 170 units from the origin and an edge is a fraction of a unit long, so S_e / |e| is in the hundreds and the scaled errors
of everything behind the normals are small numbers; the tests hold the relative L2 beside them."""
import numpy as np
import torch

from fitstep_ref import _c
from rasterize_ref import Q


# ---------------------------------------------------------------------------------------------------------------------
# tables, from the faces alone (a dictionary over the directed face edges; MeshTopology sorts keys with numpy)
# ---------------------------------------------------------------------------------------------------------------------

def hinges(faces):
    """-> (hv [H,4] int64: p0, p1, q0, q1;  sigma [H] of +1 / -1).  A hinge is an undirected edge with exactly two faces, in the order of
    (lower vertex, higher vertex); f0 is the lower face index, p0 -> p1 the direction f0 runs through the edge, q0 / q1 the third vertex
    of f0 / f1, sigma = +1 where f1 runs p1 -> p0."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    at = {}
    for fi, tri in enumerate(f.tolist()):
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            at.setdefault((min(a, b), max(a, b)), []).append((fi, k))
    hv, sigma = [], []
    for key in sorted(at):
        if len(at[key]) != 2:
            continue
        (fa, ka), (fb, kb) = sorted(at[key])
        ta, tb = f[fa].tolist(), f[fb].tolist()
        p0, p1, q0 = ta[ka], ta[(ka + 1) % 3], ta[(ka + 2) % 3]
        sigma.append(1 if tb[kb] == p1 else -1)
        hv.append([p0, p1, q0, tb[(kb + 2) % 3]])
    return torch.tensor(hv, dtype=torch.long).reshape(-1, 4), torch.tensor(sigma, dtype=torch.long).reshape(-1)


def hinge_faces(faces):
    """[H,2] the two faces of every hinge (f0 < f1), in the order of hinges()."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    at = {}
    for fi, tri in enumerate(f.tolist()):
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            at.setdefault((min(a, b), max(a, b)), []).append(fi)
    return torch.tensor([sorted(at[k]) for k in sorted(at) if len(at[k]) == 2], dtype=torch.long).reshape(-1, 2)


def packed(hv, sigma):
    """hinge_vtx [4,H] int32 as the kernel reads it: role-major, -1 - q1 where sigma = -1."""
    out = hv.t().clone()
    out[3] = torch.where(sigma < 0, -1 - out[3], out[3])
    return out.to(torch.int32).contiguous()


def incidence(hv, n_vertices):
    """hinge_inc as a list per vertex of its corners 4 h + role, ascending."""
    inc = [[] for _ in range(n_vertices)]
    for h, row in enumerate(hv.tolist()):
        for role, v in enumerate(row):
            inc[v].append(4 * h + role)
    return inc


def small_meshes(gen):
    """name -> (faces, V, positions [V,3] float32): one triangle (no hinge), two triangles oriented consistently and not (sigma = +1, -1),
    a "book" of three faces on the edge (0, 1) -- not a hinge -- with one ordinary hinge on (1, 2), and the fans, the grid (boundary
    edges) and the mesh with an isolated vertex of fitstep_ref.lap_meshes."""
    import fitstep_ref as R
    quad = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.3, 1.0, 0.2], [0.5, -1.0, 0.4]])
    out = {'triangle': (np.asarray([[0, 1, 2]], dtype=np.int32), 3, quad[:3].clone()),
           'two_pos': (np.asarray([[0, 1, 2], [1, 0, 3]], dtype=np.int32), 4, quad.clone()),
           'two_neg': (np.asarray([[0, 1, 2], [0, 1, 3]], dtype=np.int32), 4, quad.clone()),
           'book': (np.asarray([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5]], dtype=np.int32), 6,
                    torch.cat([quad, torch.tensor([[0.4, 0.2, 1.0], [1.4, 0.9, -0.3]])]))}
    lap = R.lap_meshes(gen)
    for name in ('fan8', 'fan73', 'fan256', 'grid', 'isolated'):
        out[name] = lap[name][:3]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------

def _inp(x):
    return Q(x, x.abs())


def _sub(a, b):
    return tuple(p - q for p, q in zip(a, b))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sqrt(x):
    r = x.v.sqrt()
    return Q(r, x.S / (2.0 * r) + r)


def _where(m, a, b):
    return Q(torch.where(m, a.v, b.v), torch.where(m, a.S, b.S))


def angles(x, hv, sigma, dtype=torch.float64):
    """(c, s, live, parts): cos and sin of the signed dihedral angle of every hinge of x [F,V,3] as Q [F,H]; live = the hinge is not
    degenerate (|e|^2, |n0|^2 and |n1|^2 all > 0); a degenerate hinge has c = s = 0 without a scale."""
    xx = _c(x, dtype)
    P = [tuple(_inp(xx[:, hv[:, r], k]) for k in range(3)) for r in range(4)]
    p0, p1, q0, q1 = P
    sg = sigma.to(dtype)[None]
    e = _sub(p1, p0)
    n0 = _cross(e, _sub(q0, p0))
    n1 = tuple(t * sg for t in _cross(_sub(q1, p0), e))
    e2, m0, m1 = _dot(e, e), _dot(n0, n0), _dot(n1, n1)
    live = (e2.v > 0) & (m0.v > 0) & (m1.v > 0)
    one, zero = Q(torch.ones_like(e2.v), torch.zeros_like(e2.v)), Q(torch.zeros_like(e2.v), torch.zeros_like(e2.v))
    e2, m0, m1 = (_where(live, t, one) for t in (e2, m0, m1))
    L, l0, l1 = _sqrt(e2), _sqrt(m0), _sqrt(m1)
    u0, u1, eh = tuple(t / l0 for t in n0), tuple(t / l1 for t in n1), tuple(t / L for t in e)
    c = _where(live, _dot(u0, u1), zero)
    s = _where(live, _dot(_cross(u0, u1), eh), zero)
    return c, s, live, dict(P=P, e=e, n0=n0, n1=n1, m0=m0, m1=m1, L=L)


def rest_cs(x_rest, hv, sigma, rounded=True):
    """[2,H] float32: (cos, sin) of the rest angles in float64 from the float32 rest positions, rounded once; (1, 0) for a hinge
    degenerate at rest.  rounded=False: from x_rest as it is, left in float64 (the statement's own table, for its exact zero)."""
    x = x_rest.detach().to('cpu', torch.float32 if rounded else torch.float64).reshape(1, -1, 3)
    c, s, live, _ = angles(x, hv, sigma)
    c, s = torch.where(live, c.v, torch.ones_like(c.v)), torch.where(live, s.v, torch.zeros_like(s.v))
    out = torch.stack([c[0], s[0]])
    return out.float() if rounded else out


def bend(x, hv, sigma, cs, weight, dtype=torch.float64):
    """x [F,V,3], (hv, sigma) from hinges(), cs [2,H] float32 or None ((1, 0): the plain term), weight.
    -> dict 'per' [F], 'value' [], 'hinge_grad' [F,H,4,3], 'grad' [F,V,3] of (value, S); 'cosd' [F,H] and 'live' [F,H] without a scale."""
    xx = _c(x, dtype)
    F, V, H = xx.shape[0], xx.shape[1], hv.shape[0]
    z = lambda *s: torch.zeros(*s, dtype=dtype)
    if H == 0:
        return {'per': (z(F), z(F)), 'value': (z(()), z(())), 'hinge_grad': (z(F, 0, 4, 3), z(F, 0, 4, 3)), 'grad': (z(F, V, 3), z(F, V, 3)),
                'cosd': z(F, 0), 'live': torch.zeros(F, 0, dtype=torch.bool)}
    c, s, live, g = angles(xx, hv, sigma, dtype)
    if cs is None:
        cr, sr = Q(torch.ones(1, H, dtype=dtype), torch.ones(1, H, dtype=dtype)), Q(z(1, H), z(1, H))
    else:
        cr, sr = _inp(_c(cs[0], dtype)[None]), _inp(_c(cs[1], dtype)[None])
    cd, sd = c * cr + s * sr, s * cr - c * sr
    one = Q(torch.ones_like(cd.v), torch.ones_like(cd.v))
    t = _where(cd.v > 0, (sd * sd) / (one + cd), one - cd)
    per = (t.v.sum(dim=1) / H, t.S.sum(dim=1) / H)
    w = float(weight) / F
    # the gradient: d t / d theta = sin delta, d theta / d corner by the rule's four expressions
    coef = float(weight) / (F * H)
    k = sd * coef
    p0, p1, q0, q1 = g['P']
    e, L = g['e'], g['L']
    a0, a1 = tuple(n / g['m0'] for n in g['n0']), tuple((n * sigma.to(dtype)[None]) / g['m1'] for n in g['n1'])      # a1 = sigma n1 / |n1|^2
    w00, w01 = _dot(_sub(q0, p1), e) / L, _dot(_sub(q1, p1), e) / L
    w10, w11 = _dot(_sub(p0, q0), e) / L, _dot(_sub(p0, q1), e) / L
    corners = [tuple(-((w00 * a + w01 * b) * k) for a, b in zip(a0, a1)), tuple(-((w10 * a + w11 * b) * k) for a, b in zip(a0, a1)),
               tuple(-((L * a) * k) for a in a0), tuple(-((L * b) * k) for b in a1)]
    lv = live[..., None, None]
    hg = torch.where(lv, torch.stack([torch.stack([q.v for q in cn], dim=-1) for cn in corners], dim=2), z(()))
    hgS = torch.where(lv, torch.stack([torch.stack([q.S for q in cn], dim=-1) for cn in corners], dim=2), z(()))
    gx, gxS = z(F, V, 3), z(F, V, 3)
    for r in range(4):
        gx.index_add_(1, hv[:, r], hg[:, :, r])
        gxS.index_add_(1, hv[:, r], hgS[:, :, r])
    return {'per': per, 'value': (w * per[0].sum(), abs(w) * per[1].sum()), 'hinge_grad': (hg, hgS), 'grad': (gx, gxS),
            'cosd': cd.v, 'live': live.expand(F, H)}


def bend_plain(x, hv, sigma, cs, weight):
    """The term as one plain differentiable torch expression (for torch.autograd): weight / F sum_f mean_h (1 - cos(theta - theta_rest)),
    no stable form, no degenerate branch."""
    p0, p1, q0, q1 = (x[:, hv[:, r]] for r in range(4))
    e = p1 - p0
    n0 = torch.cross(e, q0 - p0, dim=-1)
    n1 = sigma.to(x.dtype)[None, :, None] * torch.cross(q1 - p0, e, dim=-1)
    u0, u1, eh = (t / t.norm(dim=-1, keepdim=True) for t in (n0, n1, e))
    c, s = (u0 * u1).sum(-1), (torch.cross(u0, u1, dim=-1) * eh).sum(-1)
    if cs is None:
        cd = c
    else:
        cd = c * cs[0].to(x.dtype)[None] + s * cs[1].to(x.dtype)[None]
    return (weight / x.shape[0]) * (1.0 - cd).mean(dim=1).sum()

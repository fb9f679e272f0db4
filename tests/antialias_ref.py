"""float64 restatement on the CPU of the antialias operator (csrc/antialias.hip over aa_pairs.h and sil_bits.h; DESIGN.md "Antialias
rules"), forward and backward, without autograd: the yardstick of tests/test_gpu_antialias.py, itself checked on the CPU by
tests/test_antialias_ref.py.  Nothing here imports fpc_diffrend_amd or oracle.

decisions() makes every discrete choice in float32, one rounded operation each, in the kernels' order: the three silhouette bits per
(image, triangle) as sil_bits_of does (uncentred coordinates x hw, y hh, w; so and sp strictly of one sign), pair_select (an empty pixel
gives the other's triangle, else strict z1 < z0 gives the second's, a tie the first's; an id outside 1..T gives none), and per edge of
the chosen triangle edge_eval: orient (|Ld| >= |Lo| for x pairs, > for y pairs), the half-open extent (ya < 0) != (yb < 0), nz, 0 <= t <= 1
and far = t >= 1/2; then the two flag planes as FPCDR_AA_ROW_WORDS lays them out (bit x % 64 of word x / 64; plane 0: pair (p, p + x)).

antialias() evaluates the values ON those decisions in `dtype` (float64 by default; float32 gives "the same formula in float32 by torch",
the yardstick e32).  With P the pixel of the analysed triangle, Q its partner, s = +1 if Q lies in the + direction, (fxp, fyp) the centre of
P relative to the image's, a and b the ends of edge e:
    q_a = (x_a hw - fxp w_a, y_a hh - fyp w_a)            Lx = qay wb - wa qby,  Ly = wa qbx - qax wb,  Lz = qax qby - qay qbx
    t = -Lz / (s Ld)         Ld = Lx (x pair) or Ly        amt = t - 1/2 (far: receiver r = Q, other o = P) or 1/2 - t (r = P, o = Q)
    out[r]    += amt (c[o] - c[r])
    g_color[r] -= amt dy[r],   g_color[o] += amt dy[r]     (on top of g_color = dy)
    G = boost sum_c dy[r]_c (c[P]_c - c[Q]_c),  gLz = -G / (s Ld),  gLd = -G t / Ld, chained through the three determinants to
    (g_qax, g_qay, g_wa), (g_qbx, ...) and to pos:  x += g_qax hw,  y += g_qay hh,  w += g_wa - fxp g_qax - fyp g_qay,  z never.
g_pos is per image for pos [B,V,4] and summed over the batch for pos [V,4] (range mode).  For every output it returns (value, S): S is the
first-order rounding scale of rasterize_ref.py's docstring (class Q), carried from the inputs down through q, the determinants, t, amt and
the blend, so the cancellation in t lives in S.  S = 0 marks an entry without any term: a pixel of `out` that receives no blend is `color`
bit for bit, an entry of g_color outside every blended pair is dy bit for bit, the z column of g_pos and the rows of vertices of no active
edge are exactly 0 (measure_through; predicted_equal counts them from the decisions, never from values).

float32_in_kernel_order() gives the same outputs in float32 in the kernels' order: acc = c[me], then the visits R, U, L, D with the edges
0, 1, 2 of each (k_aa_fwd); go = dy[me], then own-x, own-y, left, down (k_aa_bwd_fix); the per-pair terms of g_pos with G accumulated
from 0 channel by channel, G *= boost, and the three atomics per vertex summed by index_add_.  The library is built with
-ffp-contract=off and IEEE division, so out and g_color must equal it bit for bit, and g_pos where every entry has one term.

decision_margin(): float64 and float32 must make the same choices or they differ by a whole blend, so for every candidate pair each edge
that carries a silhouette bit is either active with every one of orient, ya, yb, t, 1 - t and t - 1/2 more than GATE_MARGIN u of its own
scale on its side, or has one of them as far on the other side; so and sp of every triangle a pair analyses and z1 - z0 likewise.  The
constructions move what is closer than SETTLE_MARGIN (_settle); `ties` is dyadic instead and both precisions agree exactly.

dispatch() restates the host code's choices in integers; topology() the edge rule with a dict; CASES / case_inputs the GPU cases."""
import functools

import numpy as np
import torch

from fitstep_ref import U, measure, rel_l2      # noqa: F401  (re-exported: the conventions of the fit step's yardstick)
from interpolate_ref import BIN, hint_off_pixels, make_hint      # noqa: F401
from rasterize_ref import GATE_MARGIN, SETTLE_MARGIN, Q, _clip, _randn_away, _soup_geometry, _where

AROWS = 8             # rows per wave of k_aa_fwd
MUTANT = None         # set by test_antialias_ref.py only: a deliberately wrong restatement (see there)

OUTPUTS = ('out', 'g_color', 'g_pos')


def _q(x):
    return Q(x, x.abs())


def _coef(x):
    return Q(x, torch.zeros_like(x))


def _stack(qs):
    return Q(torch.stack([q.v for q in qs], 1), torch.stack([q.S for q in qs], 1))


# ---------------------------------------------------------------------------------------------------------------------
# topology, dispatch
# ---------------------------------------------------------------------------------------------------------------------

def topology(tri):
    """adj [T,3] int32: per undirected edge the count of triangles and the sum of the vertices opposite; entry (t, e) is for the edge
    opposite corner e: -1 with a count of 1, sum - own with 2, -2 with more."""
    t = tri.detach().cpu().tolist()
    edges = {}
    for v in t:
        for e in range(3):
            key = (min(v[(e + 1) % 3], v[(e + 2) % 3]), max(v[(e + 1) % 3], v[(e + 2) % 3]))
            c, s = edges.get(key, (0, 0))
            edges[key] = (c + 1, s + v[e])
    adj = []
    for v in t:
        row = []
        for e in range(3):
            c, s = edges[(min(v[(e + 1) % 3], v[(e + 2) % 3]), max(v[(e + 1) % 3], v[(e + 2) % 3]))]
            row.append(-1 if c == 1 else (s - v[e] if c == 2 else -2))
        adj.append(row)
    return torch.tensor(adj, dtype=torch.int32).reshape(-1, 3)


def topo_capacity(T):
    cap = 64
    while cap < 6 * T:
        cap *= 2
    return cap


def dispatch(C, W, hint, pointers=(), nfl=None):
    """What fpcdr_antialias_fwd and fpcdr_antialias_bwd launch.  pointers: (color, out, dy, grad_color) addresses, None or missing =
    16-byte aligned; nfl = B H W C.  -> dict fwd, fill (k_aa_fill_bin1 runs), clear (how the flag planes are zeroed), copy (the pieces
    of the bulk copy g_color = dy), bwd."""
    p = list(pointers) + [None] * (4 - len(pointers))
    ok = lambda *ps: all(q is None or q % 16 == 0 for q in ps)
    tmpl = C if C in (1, 3, 4) else 0
    res = dict(fwd=f'k_aa_fwd<{tmpl}>', fill=bool(hint) and C == 1 and W % 4 == 0 and ok(p[0], p[1]),
               clear='memset' if hint else 'lane 0', bwd=f'k_aa_bwd_fix<{tmpl}>')
    if nfl is not None:
        if ok(p[2], p[3]):
            n4 = nfl // 4
            res['copy'] = tuple(k for k, on in (('f4 unrolled', n4 >= 512), ('f4 tail', n4 % 512 != 0), ('remainder', nfl % 4 != 0)) if on)
        else:
            res['copy'] = ('memcpy',)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------------------------------------------------

def _pos3(pos, B):
    p = pos.detach().cpu()
    return p[None].expand(B, -1, -1) if p.dim() == 2 else p


def _sil(pos3, tri, adj, H, W, dtype):
    """sil_bits_of for every (image, triangle) in dtype -> bits [B,T] int64, margin [B,T]: the smallest |so|, |sp| over the edges with a
    neighbour in units of u of its scale (inf without one)."""
    hw, hh = 0.5 * W, 0.5 * H
    B, V = pos3.shape[0], pos3.shape[1]
    p = pos3.to(dtype)
    vi, ad = tri.detach().cpu().long(), adj.detach().cpu().long()
    qx, qy, qw = _q(p[..., 0]) * hw, _q(p[..., 1]) * hh, _q(p[..., 3])
    at = lambda q, idx: Q(q.v[:, idx], q.S[:, idx])
    bits = torch.zeros(B, vi.shape[0], dtype=torch.int64)
    margin = torch.full((B, vi.shape[0]), float('inf'), dtype=torch.float64)
    for e in range(3):
        a, b = vi[:, (e + 1) % 3], vi[:, (e + 2) % 3]
        Lx = at(qy, a) * at(qw, b) - at(qw, a) * at(qy, b)
        Ly = at(qw, a) * at(qx, b) - at(qx, a) * at(qw, b)
        Lz = at(qx, a) * at(qy, b) - at(qy, a) * at(qx, b)
        o, n = vi[:, e], ad[:, e].clamp(0, V - 1)
        so = Lx * at(qx, o) + Ly * at(qy, o) + Lz * at(qw, o)
        sp = Lx * at(qx, n) + Ly * at(qy, n) + Lz * at(qw, n)
        valid = ((ad[:, e] >= 0) & (ad[:, e] < V))[None]
        same = ((so.v > 0) & (sp.v > 0)) | ((so.v < 0) & (sp.v < 0))
        if MUTANT == 'silhouette_ignores_neighbour':
            same = torch.ones_like(same)
        bits |= ((ad[:, e] == -1)[None] | (valid & same)).long() << e
        m = torch.minimum(so.v.abs() / (U * so.S), sp.v.abs() / (U * sp.S)).double()
        margin = torch.minimum(margin, torch.where(valid.expand(B, -1), torch.nan_to_num(m, nan=0.0), torch.full_like(m, float('inf'))))
    return bits, margin


class _Pairs:
    """The candidate pairs of a rast: ids differ, pair_select gives a triangle, and it owns a silhouette bit.  x pairs first."""

    def __init__(self, rast, T, bits):
        r = rast.detach().cpu()
        B, H, W, _ = r.shape
        ids, z = r[..., 3].to(torch.int64), r[..., 2]
        cols = {k: [] for k in ('b', 'x0', 'y0', 'd', 'use1', 'tau', 'zm')}
        self.analysed = torch.zeros(B, T, dtype=torch.bool)      # triangles pair_select hands to the silhouette test
        self.n_id_pairs = 0
        for d in (0, 1):
            sl0, sl1 = ((slice(None), slice(None), slice(0, W - 1)), (slice(None), slice(None), slice(1, W))) if d == 0 else \
                       ((slice(None), slice(0, H - 1)), (slice(None), slice(1, H)))
            b, y, x = torch.nonzero(ids[sl0] != ids[sl1], as_tuple=True)
            i0, i1, z0, z1 = ids[sl0][b, y, x], ids[sl1][b, y, x], z[sl0][b, y, x], z[sl1][b, y, x]
            nearer = (z1 <= z0) if MUTANT == 'z_tie_to_second' else (z1 < z0)
            use1 = torch.where(i0 == 0, torch.ones_like(nearer), torch.where(i1 == 0, torch.zeros_like(nearer), nearer))
            tau = torch.where(use1, i1, i0) - 1
            ok = (tau >= 0) & (tau < T)
            self.n_id_pairs += int(b.numel())
            self.analysed[b[ok], tau[ok]] = True
            zm = torch.where((i0 > 0) & (i1 > 0) & (z0 != z1), (z1 - z0).abs().double() / (U * (z0.abs() + z1.abs()).double()),
                             torch.full(z0.shape, float('inf'), dtype=torch.float64))
            ok = ok & (bits[b, tau.clamp(0, T - 1)] != 0)
            for k, v in zip(cols, (b, x, y, torch.full_like(b, d), use1, tau, zm)):
                cols[k].append(v[ok])
        for k, v in cols.items():
            setattr(self, k, torch.cat(v))
        self.n = int(self.b.numel())
        self.B, self.H, self.W = B, H, W
        self.x1, self.y1 = self.x0 + (self.d == 0).long(), self.y0 + (self.d == 1).long()
        self.Px, self.Py = torch.where(self.use1, self.x1, self.x0), torch.where(self.use1, self.y1, self.y0)
        self.Qx, self.Qy = torch.where(self.use1, self.x0, self.x1), torch.where(self.use1, self.y0, self.y1)
        flat = lambda x, y: (self.b * H + y) * W + x
        self.p0, self.p1, self.pP, self.pQ = flat(self.x0, self.y0), flat(self.x1, self.y1), flat(self.Px, self.Py), flat(self.Qx, self.Qy)


def _edges(pr, pos3, tri, dtype):
    """edge_eval of the three edges of every pair's triangle in dtype -> dict of Q [n,3] (t, Lx, Ly, Lz, Ld, Lo, ya, yb and the six
    coordinates), va, vb [n,3], s, fxp, fyp [n]."""
    hw, hh = 0.5 * pr.W, 0.5 * pr.H
    if MUTANT == 'hw_hh_swapped':
        hw, hh = hh, hw
    fxp, fyp = _coef(pr.Px.to(dtype) + 0.5 - hw), _coef(pr.Py.to(dtype) + 0.5 - hh)
    vi = tri.detach().cpu().long()[pr.tau]
    p = pos3.to(dtype)
    c = [p[pr.b, vi[:, k]] for k in range(3)]
    s = _coef(torch.where(pr.use1, -1.0, 1.0).to(dtype))
    is_x = pr.d == 0
    keys = ('t', 'Lx', 'Ly', 'Lz', 'Ld', 'Lo', 'ya', 'yb', 'qax', 'qay', 'wa', 'qbx', 'qby', 'wb')
    acc = {k: [] for k in keys}
    for e in range(3):
        ca, cb = c[(e + 1) % 3], c[(e + 2) % 3]
        wa, wb = _q(ca[:, 3]), _q(cb[:, 3])
        qax, qay = _q(ca[:, 0]) * hw - fxp * wa, _q(ca[:, 1]) * hh - fyp * wa
        qbx, qby = _q(cb[:, 0]) * hw - fxp * wb, _q(cb[:, 1]) * hh - fyp * wb
        Lx = qay * wb - wa * qby
        Ly = wa * qbx - qax * wb
        Lz = qax * qby - qay * qbx
        Ld, Lo = _where(is_x, Lx, Ly), _where(is_x, Ly, Lx)
        ya, yb = _where(is_x, qay, qax), _where(is_x, qby, qbx)
        den = _where(Ld.v != 0, Ld if MUTANT == 's_dropped' else s * Ld, 1.0)
        t = (-Lz) / den
        for k, v in zip(keys, (t, Lx, Ly, Lz, Ld, Lo, ya, yb, qax, qay, wa, qbx, qby, wb)):
            acc[k].append(v)
    E = {k: _stack(v) for k, v in acc.items()}
    E.update(va=torch.stack([vi[:, 1], vi[:, 2], vi[:, 0]], 1), vb=torch.stack([vi[:, 2], vi[:, 0], vi[:, 1]], 1), s=s, fxp=fxp, fyp=fyp)
    return E


def _choices(pr, E, bits):
    """The float decisions of edge_eval on an evaluation E -> active [n,3], far [n,3]."""
    is_x = (pr.d == 0)[:, None]
    aLd, aLo = E['Ld'].v.abs(), E['Lo'].v.abs()
    orient = torch.where(is_x, (aLd > aLo) if MUTANT == 'x_orient_strict' else (aLd >= aLo), aLd > aLo)
    extent = (E['ya'].v < 0) != (E['yb'].v < 0)
    if MUTANT == 'closed_extent':
        extent = extent | (E['ya'].v == 0) | (E['yb'].v == 0)
    t = E['t'].v
    has = ((bits[pr.b, pr.tau][:, None] >> torch.arange(3)[None]) & 1).bool()
    active = has & orient & extent & (E['Ld'].v != 0) & (t >= 0) & (t <= 1)
    return active, (t > 0.5) if MUTANT == 'half_is_near' else (t >= 0.5)


class Decisions:
    pass


def decisions(color, rast, pos, tri, adj, dtype=torch.float32):
    """Every discrete choice of a call, in float32 (dtype is for the test that `ties` decides alike in float64).  -> Decisions with
    sil [B,T], pairs (_Pairs), E (the float32 edge evaluation), active / far [n,3], the active (pair, edge) entries ei, ee with their
    receiving and other pixel er, eo (flat indices), flags uint64 [2,B,H,ceil(W/64)]."""
    D = Decisions()
    B, H, W, _ = rast.shape
    D.B, D.H, D.W, D.T = B, H, W, tri.shape[0]
    D.range_mode = pos.dim() == 2
    D.pos3 = _pos3(pos, B)
    D.V = D.pos3.shape[1]
    D.tri = tri.detach().cpu()
    D.sil, D.sil_margin = _sil(D.pos3, tri, adj, H, W, dtype)
    D.pairs = pr = _Pairs(rast, D.T, D.sil)
    D.E = _edges(pr, D.pos3, tri, dtype)
    D.active, D.far = _choices(pr, D.E, D.sil)
    D.ei, D.ee = torch.nonzero(D.active, as_tuple=True)
    far = D.far[D.ei, D.ee]
    D.efar = far
    D.er, D.eo = torch.where(far, pr.pQ[D.ei], pr.pP[D.ei]), torch.where(far, pr.pP[D.ei], pr.pQ[D.ei])
    Wq = (W + 63) // 64
    flags = np.zeros((2, B, H, Wq), dtype=np.uint64)
    hit = D.active.any(1)
    for b, x, y, d in zip(pr.b[hit].tolist(), pr.x0[hit].tolist(), pr.y0[hit].tolist(), pr.d[hit].tolist()):
        flags[d, b, y, x // 64] |= np.uint64(1) << np.uint64(x % 64)
    D.flags = flags
    return D


def edge_margins(D, E64):
    """[n,3] float64: how far, in units of u of its own scale, every edge with a silhouette bit is from changing its outcome (module
    docstring); inf without a bit.  E64: the float64 evaluation of the same pairs."""
    pr = D.pairs
    rel = lambda q: torch.nan_to_num(q.v / (U * q.S), nan=0.0)
    Ld, Lo, t = E64['Ld'], E64['Lo'], E64['t']
    m_orient = torch.nan_to_num((Ld.v.abs() - Lo.v.abs()) / (U * (Ld.S + Lo.S)), nan=0.0)
    ya, yb = rel(E64['ya']), rel(E64['yb'])
    m_extent = torch.minimum(ya.abs(), yb.abs()) * torch.where((ya < 0) != (yb < 0), 1.0, -1.0)
    m_t0, m_t1 = rel(t), torch.nan_to_num((1.0 - t.v) / (U * t.S), nan=0.0)
    conds = torch.stack([m_orient, m_extent, m_t0, m_t1], 0)
    m_far = torch.nan_to_num((t.v - 0.5).abs() / (U * t.S), nan=0.0)
    parallel = (Ld.v == 0) & (Ld.S == 0)
    safe = torch.maximum((-conds).max(0).values, torch.minimum(conds.min(0).values, m_far))
    safe = torch.where(parallel, torch.full_like(safe, float('inf')), safe)
    has = ((D.sil[pr.b, pr.tau][:, None] >> torch.arange(3)[None]) & 1).bool()
    return torch.where(has, safe, torch.full_like(safe, float('inf')))


def decision_margin(r):
    """The smallest margin of a reference r = antialias(...): over the edges of every candidate pair, the silhouette tests of every
    triangle a pair analyses, and z1 - z0 of every pair of two covered pixels."""
    D = r['D']
    m = [float('inf')]
    if D.pairs.n:
        m += [float(edge_margins(D, r['E']).min()), float(D.pairs.zm.min())]
    if bool(D.pairs.analysed.any()):
        m.append(float(D.sil_margin[D.pairs.analysed].min()))
    return min(m)


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------

def _pos_terms(D, E, color, dy, boost, dtype):
    """The six atomics of every active (pair, edge) entry -> (rows of va, rows of vb, [Q x, Q y, Q w] for a, the same for b, keep: the
    entries k_aa_bwd_fix does not leave at G == 0)."""
    pr, i, e = D.pairs, D.ei, D.ee
    C = color.shape[-1]
    hw, hh = 0.5 * D.W, 0.5 * D.H
    col, g = color.detach().cpu().to(dtype).reshape(-1, C), dy.detach().cpu().to(dtype).reshape(-1, C)
    gr, cP, cQ = g[D.er], col[pr.pP[i]], col[pr.pQ[i]]
    G = _coef(torch.zeros(i.numel(), dtype=dtype))
    for c in range(C):
        G = G + _q(gr[:, c]) * (_q(cP[:, c]) - _q(cQ[:, c]))
    G = G * float(boost)
    pick = lambda k: Q(E[k].v[i, e], E[k].S[i, e])
    t, Ld = pick('t'), pick('Ld')
    s = Q(E['s'].v[i], E['s'].S[i])
    qax, qay, wa, qbx, qby, wb = (pick(k) for k in ('qax', 'qay', 'wa', 'qbx', 'qby', 'wb'))
    gLz = (-G) / (s * Ld)
    gLd = ((-G) * t) / Ld
    is_x = pr.d[i] == 0
    zero = _coef(torch.zeros(i.numel(), dtype=dtype))
    gLx, gLy = _where(is_x, gLd, zero), _where(is_x, zero, gLd)
    g_qay = zero + gLx * wb; g_wb = zero + gLx * qay; g_wa = zero - gLx * qby; g_qby = zero - gLx * wa
    g_wa = g_wa + gLy * qbx; g_qbx = zero + gLy * wa; g_qax = zero - gLy * wb; g_wb = g_wb - gLy * qax
    g_qax = g_qax + gLz * qby; g_qby = g_qby + gLz * qax; g_qay = g_qay - gLz * qbx; g_qbx = g_qbx - gLz * qay
    fxp = _coef(pr.Px[i].to(dtype) + 0.5 - hw)
    fyp = _coef(pr.Py[i].to(dtype) + 0.5 - hh)
    if MUTANT == 'w_column_without_fxp_fyp':
        wcol = lambda gw, gx, gy: gw
    else:
        wcol = lambda gw, gx, gy: gw - fxp * gx - fyp * gy
    ta = [g_qax * hw, g_qay * hh, wcol(g_wa, g_qax, g_qay)]
    tb = [g_qbx * hw, g_qby * hh, wcol(g_wb, g_qbx, g_qby)]
    base = torch.zeros_like(pr.b[i]) if D.range_mode else pr.b[i] * D.V
    return base + D.E['va'][i, e], base + D.E['vb'][i, e], ta, tb, G.v != 0


def _scatter_pos(D, terms, pick, dtype):
    rows_a, rows_b, ta, tb, keep = terms
    Gp = torch.zeros((1 if D.range_mode else D.B) * D.V, 4, dtype=dtype)
    for rows, three in ((rows_a, ta), (rows_b, tb)):
        for col, q in zip((0, 1, 3), three):
            Gp[:, col].index_add_(0, rows[keep], pick(q)[keep])
    return Gp.reshape(D.V, 4) if D.range_mode else Gp.reshape(D.B, D.V, 4)


def antialias(color, rast, pos, tri, adj, dy=None, boost=1.0, dtype=torch.float64, D=None):
    """color [B,H,W,C], rast [B,H,W,4], pos [B,V,4] or [V,4], tri [T,3], adj [T,3] (topology), dy = d loss / d out -> dict: 'out' and,
    with dy, 'g_color', 'g_pos': (value, S) in dtype on the float32 decisions D (made here unless handed in); 'D', 'E' (the edge
    evaluation in dtype)."""
    if D is None:
        D = decisions(color, rast, pos, tri, adj)
    pr = D.pairs
    C = color.shape[-1]
    E = _edges(pr, D.pos3, tri, dtype)
    i, e = D.ei, D.ee
    t = Q(E['t'].v[i, e], E['t'].S[i, e])
    amt = _where(D.efar, t - 0.5, 0.5 - t)
    amt = Q(amt.v[:, None], amt.S[:, None])
    col = color.detach().cpu().to(dtype).reshape(-1, C)
    res = {'D': D, 'E': E}

    def gather_form(base, term_r, term_o, touched):
        """base + the terms summed at their pixels -> (value, S) shaped like color; S = 0 away from `touched`."""
        v, S = base.clone(), torch.zeros_like(base)
        S[touched] = base[touched].abs()
        for idx, q, sign in ((D.er, term_r, 1.0), (D.eo, term_o, 1.0)):
            if q is not None:
                v.index_add_(0, idx, sign * q.v)
                S.index_add_(0, idx, q.S)
        return v.reshape(color.shape), S.reshape(color.shape)

    delta = amt * (_q(col[D.eo]) - _q(col[D.er]))
    res['out'] = gather_form(col, delta, None, torch.unique(D.er))
    if dy is None:
        return res
    g = dy.detach().cpu().to(dtype).reshape(-1, C)
    term = amt * _q(g[D.er])
    if MUTANT == 'boost_on_g_color':
        term = term * float(boost)
    res['g_color'] = gather_form(g, -term, -term if MUTANT == 'other_pixel_wrong_sign' else term, torch.unique(torch.cat([D.er, D.eo])))
    terms = _pos_terms(D, E, color, dy, boost, dtype)
    res['g_pos'] = (_scatter_pos(D, terms, lambda q: q.v, dtype), _scatter_pos(D, (*terms[:4], torch.ones_like(terms[4])), lambda q: q.S, dtype))
    return res


def float32_in_kernel_order(color, rast, pos, tri, adj, dy=None, boost=1.0, hint=None):
    """-> dict name -> float32 tensor, every operation rounded on its own in the kernels' order (module docstring).  hint: only for the
    mutant that loses the blends into an empty bin."""
    D = decisions(color, rast, pos, tri, adj)
    pr, E = D.pairs, D.E
    C = color.shape[-1]
    i, e = D.ei, D.ee
    t = E['t'].v[i, e]
    amt = torch.where(D.efar, t - 0.5, 0.5 - t).numpy()
    col = color.detach().cpu().float().reshape(-1, C).numpy()
    er, eo = D.er.numpy(), D.eo.numpy()
    d, first = pr.d[i].numpy(), pr.p0[i].numpy()
    xs, ys = np.arange(D.B * D.H * D.W) % D.W, (np.arange(D.B * D.H * D.W) // D.W) % D.H
    # forward: the receiver visits its pairs in the order R, U (it is the pair's first pixel), L, D (the second), edges 0, 1, 2 within
    out = col.copy()
    rank = np.where(er == first, d, 2 + d)
    drop = np.zeros(len(er), dtype=bool)
    if MUTANT == 'empty_bin_blend_dropped' and hint is not None:
        drop = hint_off_pixels(hint, D.B, D.H, D.W).reshape(-1).numpy()[er]
    for k in np.lexsort((e.numpy(), rank)):
        if not drop[k]:
            out[er[k]] = out[er[k]] + amt[k] * (col[eo[k]] - col[er[k]])
    res = {'out': torch.from_numpy(out).reshape(color.shape), 'D': D}
    if dy is None:
        return res
    g = dy.detach().cpu().float().reshape(-1, C).numpy()
    go = g.copy()
    # backward: both pixels of a blended pair visit it -- own-x, own-y (first pixel), left, down (second)
    px = np.concatenate([first, pr.p1[i].numpy()])
    rk = np.concatenate([d, 2 + d])
    kk = np.concatenate([np.arange(len(er))] * 2)
    keep = np.ones(len(px), dtype=bool)
    if MUTANT == 'left_partner_lost_at_lane_0':
        keep &= ~((rk == 2) & (xs[px] % 64 == 0))
    if MUTANT == 'down_partner_lost_at_row_8k':
        keep &= ~((rk == 3) & (ys[px] % AROWS == 0))
    scale = np.float32(boost) if MUTANT == 'boost_on_g_color' else np.float32(1.0)
    for j in np.lexsort((np.concatenate([e.numpy()] * 2), rk)):
        if not keep[j]:
            continue
        k, me = kk[j], px[j]
        if er[k] == me or MUTANT == 'other_pixel_wrong_sign':
            go[me] = go[me] - scale * amt[k] * g[er[k]]
        else:
            go[me] = go[me] + scale * amt[k] * g[er[k]]
    if MUTANT == 'remainder_of_g_color_unwritten' and go.size % 4:
        go.reshape(-1)[go.size - go.size % 4:] = 0.0
    res['g_color'] = torch.from_numpy(go).reshape(color.shape)
    terms = _pos_terms(D, E, color, dy, boost, torch.float32)
    gp = _scatter_pos(D, terms, lambda q: q.v, torch.float32)
    res['g_pos'] = gp
    return res


def predicted_equal(D, C, dy=None):
    """name -> the number of entries without any term, from the decisions and the pattern of zeroed gradients alone: out: C per pixel that
    receives no blend; g_color: the entries outside every blended pair, and those of a pair where neither dy there nor the receiver's
    dy is nonzero; g_pos: the z column, and x, y, w of the vertices of no active edge whose receiver has a gradient."""
    P = D.B * D.H * D.W
    z = {'out': C * (P - int(torch.unique(D.er).numel()))}
    if dy is None:
        return z
    live = dy.detach().cpu().reshape(P, C) != 0
    has = torch.zeros(P, C, dtype=torch.bool)
    touched = torch.unique(torch.cat([D.er, D.eo]))
    has[touched] = live[touched]
    has.index_put_((torch.cat([D.er, D.eo]),), torch.cat([live[D.er], live[D.er]]), accumulate=True)
    z['g_color'] = P * C - int(has.sum())
    on = live[D.er].any(1)
    rows = torch.cat([D.E['va'][D.ei, D.ee][on], D.E['vb'][D.ei, D.ee][on]]) + (0 if D.range_mode else torch.cat([D.pairs.b[D.ei][on]] * 2) * D.V)
    nv = (1 if D.range_mode else D.B) * D.V
    z['g_pos'] = nv + 3 * (nv - int(torch.unique(rows).numel()))
    return z


def measure_through(x, r, S, base):
    """measure() for an output that is `base` wherever it has no term: the entries with S = 0 must equal base bit for bit (asserted),
    the others are measured -> (e in units of u, number of entries with S = 0)."""
    x, base = x.detach().cpu(), base.detach().cpu()
    z = S == 0
    assert torch.equal(x[z], base[z].to(x.dtype)), "an entry without any term is not its input bit for bit"
    return measure(torch.where(z, torch.zeros_like(x), x), torch.where(z, torch.zeros_like(r), r), S)


def failures(inp, ref, r32, k32, got, report=None):
    """What of `got` (name -> tensor) misses a bar of tests/test_gpu_antialias.py -> list.  ref, r32: antialias() in float64 and float32;
    k32: float32_in_kernel_order.  report(name, e, e32, bound) is called for every measured output."""
    bad = []
    D = ref['D']
    zeros = predicted_equal(D, inp['color'].shape[-1], inp['dy'])
    base = {'out': inp['color'], 'g_color': inp['dy'], 'g_pos': torch.zeros_like(ref['g_pos'][0]) if 'g_pos' in ref else None}
    for k in OUTPUTS:
        if k not in got:
            continue
        x = got[k].detach().cpu()
        r, S = ref[k]
        try:
            e, nz = measure_through(x, r, S, base[k])
        except AssertionError:
            bad.append((k, 'a term where there is none'))
            continue
        e32, _ = measure_through(r32[k][0], r, S, base[k])
        if report is not None:
            report(k, e, e32, 8 * e32 + 4)
        if nz != zeros[k]:
            bad.append((k, 'count of entries without a term', nz, zeros[k]))
        if not e <= 8 * e32 + 4:
            bad.append((k, 'bound', round(e, 2), round(8 * e32 + 4, 2)))
        if (k != 'g_pos' or inp.get('one_term')) and not torch.equal(x, k32[k]):
            differ = x != k32[k]
            bad.append((k, 'not bit-identical to float32_in_kernel_order', int(differ.sum()), differ.nonzero()[:3].tolist()))
        if k == 'out' and inp.get('dyadic') and not torch.equal(x.double(), r):
            bad.append((k, 'not equal to float64 on dyadic inputs'))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_antialias.py
# ---------------------------------------------------------------------------------------------------------------------

def _scan(X, zw, tri, H, W, subsets=None):
    """A tiny scanline: pixel centres strictly inside a triangle, z/w affine in the image, the smaller wins, ties to the lower index.
    X [B,V,2] pixel coordinates float64, zw [B,V] -> rast [B,H,W,4] float32 = (0, 0, z/w, id)."""
    B = X.shape[0]
    ids = torch.zeros(B, H, W, dtype=torch.int64)
    depth = torch.full((B, H, W), float('inf'), dtype=torch.float64)
    for b in range(B):
        for t, (i, j, k) in enumerate(tri.tolist()):
            if subsets is not None and t not in subsets[b]:
                continue
            (x0, y0), (x1, y1), (x2, y2) = X[b, i].tolist(), X[b, j].tolist(), X[b, k].tolist()
            area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            lo_x, hi_x = max(int(min(x0, x1, x2)) - 1, 0), min(int(max(x0, x1, x2)) + 2, W)
            lo_y, hi_y = max(int(min(y0, y1, y2)) - 1, 0), min(int(max(y0, y1, y2)) + 2, H)
            if area == 0 or lo_x >= hi_x or lo_y >= hi_y:
                continue
            cy, cx = torch.meshgrid(torch.arange(lo_y, hi_y, dtype=torch.float64) + 0.5, torch.arange(lo_x, hi_x, dtype=torch.float64) + 0.5, indexing='ij')
            l0 = ((x1 - cx) * (y2 - cy) - (y1 - cy) * (x2 - cx)) / area
            l1 = ((x2 - cx) * (y0 - cy) - (y2 - cy) * (x0 - cx)) / area
            l2 = 1.0 - l0 - l1
            z = l0 * float(zw[b, i]) + l1 * float(zw[b, j]) + l2 * float(zw[b, k])
            sub = (b, slice(lo_y, hi_y), slice(lo_x, hi_x))
            win = (l0 > 0) & (l1 > 0) & (l2 > 0) & (z < depth[sub])
            depth[sub] = torch.where(win, z, depth[sub])
            ids[sub] = torch.where(win, torch.full_like(ids[sub], t + 1), ids[sub])
    rast = torch.zeros(B, H, W, 4)
    rast[..., 2] = torch.where(ids > 0, depth, torch.zeros_like(depth)).float()
    rast[..., 3] = ids.float()
    return rast


def _unsafe_rows(D, E64):
    """The rows of pos3.reshape(-1, 4) (vertices per image) of every triangle with a decision closer than SETTLE_MARGIN."""
    pr = D.pairs
    bad_pair = (edge_margins(D, E64) <= SETTLE_MARGIN).any(1) | (pr.zm <= SETTLE_MARGIN)
    bt = torch.stack([pr.b[bad_pair], pr.tau[bad_pair]], 1)
    sb, st = torch.nonzero(D.pairs.analysed & (D.sil_margin <= SETTLE_MARGIN), as_tuple=True)
    bt = torch.cat([bt, torch.stack([sb, st], 1)])
    if bt.numel() == 0:
        return bt.reshape(-1)
    vi = D.tri.long()[bt[:, 1]]
    return torch.unique((bt[:, :1] * D.V + vi).reshape(-1))


def _settle(X, zw, w, tri, H, W, gen, range_mode=False, subsets=None, rounds=200):
    """Move (by up to 0.05 pixel a round) the vertices of every triangle with a decision too close, until none is.
    X [B,V,2] float64 -> (pos, rast)."""
    adj = topology(tri)
    B = 2 if range_mode else X.shape[0]
    for _ in range(rounds):
        pos = _clip(X, torch.zeros_like(w), w, H, W)
        rast = _scan(X.expand(B, -1, -1), zw.expand(B, -1), tri, H, W, subsets)
        pos_in = pos[0] if range_mode else pos
        D = decisions(None, rast, pos_in, tri, adj)
        rows = _unsafe_rows(D, _edges(D.pairs, D.pos3, tri, torch.float64))
        if rows.numel() == 0:
            return pos_in, rast
        if range_mode:
            rows = torch.unique(rows % D.V)
        X.reshape(-1, 2)[rows] += (torch.rand(rows.numel(), 2, generator=gen, dtype=torch.float64) - 0.5) * 0.1
    raise AssertionError("the construction does not settle")


def _soup(B, H, W, n_tri, size_px, seed, range_mode=False):
    gen = torch.Generator().manual_seed(seed)
    X, z, w, tri = _soup_geometry(1 if range_mode else B, n_tri, gen, H, W, size_px)
    subsets = [set(range(n_tri)), set(range(n_tri // 2, n_tri))] if range_mode else None      # (the second image draws half of them)
    pos, rast = _settle(X, z, w, tri, H, W, gen, range_mode, subsets)
    return pos, tri, rast


def _octahedron():
    """A subdivided octahedron: 18 vertices, 32 triangles, closed (every edge has two triangles)."""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    mid, tri = {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            p = np.array(v[a], dtype=np.float64) + np.array(v[b], dtype=np.float64)
            v.append(tuple(p / np.linalg.norm(p)))
            mid[key] = len(v) - 1
        return mid[key]

    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        tri += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return torch.tensor(v, dtype=torch.float64), torch.tensor(tri, dtype=torch.int32)


def _mesh(H, W, seed):
    """Three poses of the octahedron mesh under perspective: X, z/w and w per image."""
    gen = torch.Generator().manual_seed(seed)
    v, tri = _octahedron()
    Xs, zs, ws = [], [], []
    for b in range(3):
        Rm, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
        p = v @ Rm.T * torch.tensor([1.0, 0.8, 1.2], dtype=torch.float64)
        w = 3.0 + p[:, 2]
        Xs.append(torch.stack([W / 2 + 1.3 * (b - 1) + 48.0 * p[:, 0] / w, H / 2 - 0.7 * b + 48.0 * p[:, 1] / w], 1))
        zs.append(p[:, 2] / 4.0)
        ws.append(w)
    X, z, w = torch.stack(Xs), torch.stack(zs), torch.stack(ws)
    pos, rast = _settle(X, z, w, tri, H, W, gen)
    return pos, tri, rast


def _hand(tris, H, W, gen, ghosts=0):
    """Unshared triangles at given pixel coordinates [(x, y) x 3, ...], w in [0.5, 3].  The last `ghosts` of them are in tri and pos
    but not in rast; a second rast that shows them too is returned after it."""
    X = torch.tensor(tris, dtype=torch.float64).reshape(1, -1, 2)
    n = X.shape[1] // 3
    w = torch.rand(1, 3 * n, generator=gen, dtype=torch.float64) * 2.5 + 0.5
    z = torch.rand(1, 3 * n, generator=gen, dtype=torch.float64) * 1.8 - 0.9
    tri = torch.arange(3 * n, dtype=torch.int32).reshape(n, 3)
    pos, rast = _settle(X, z, w, tri, H, W, gen, subsets=[set(range(n - ghosts))])
    return (pos, tri, rast) + ((_scan(X, z, tri, H, W),) if ghosts else ())


# hinted cases: triangles A, B in bin (0, 0) and D in bin (1, 1); the bins between them are empty and receive across the boundaries
HINT_TRIS = [[(12.0, 14.0), (32.2, 3.3), (32.25, 26.6)],        # A: right edge at x ~ 32.2: pixel 31 | 32, receiver in bin (0, 1), its column 0
             [(5.0, 29.0), (6.3, 32.2), (27.6, 32.25)],         # B: top edge at y ~ 32.2: row 31 | 32, receiver in bin (1, 0), its row 0
             [(31.8, 31.75), (55.0, 31.8), (31.75, 52.0)],      # D: bottom edge y ~ 31.8 and left edge x ~ 31.8: receivers in row 31 of bin (0, 1)
             [(40.0, 40.0), (52.3, 44.1), (43.2, 49.4)],        #    and column 31 of bin (1, 0); and a triangle on top of D
             [(95.2, 3.1), (103.0, 20.4), (95.6, 44.7)]]        # a ghost: not in rast; the planted twin shows it in the bins the hint switches off
WIDE_TRIS = [[(240.3, 1.2), (256.2, 0.4), (256.25, 8.7)],       # right edge at x ~ 256.2: pair 255 | 256 (bit 63 of word 3, partner in word 4)
             [(257.8, 0.3), (262.0, 4.4), (257.75, 8.8)],       # left edge at x ~ 257.8: pair 257 | 258 in the partial last word
             [(60.2, 2.1), (64.3, 0.2), (64.2, 8.9)], [(100.0, 1.0), (130.0, 4.0), (110.0, 8.0)], [(1.2, 0.3), (9.1, 3.3), (0.4, 8.8)]]


def _ties():
    """(1, 32, 32), C = 1, every coordinate dyadic, rast written by hand: see the list in test_antialias_ref.py."""
    H = W = 32
    tris, wv = [], []

    def add(a, b, c, w=1.0):
        tris.append([a, b, c])
        wv.append(w)
        return len(tris)          # the id

    ids, zz = torch.zeros(H, W), torch.zeros(H, W)

    def put(x, y, i, z=0.25):
        ids[y, x], zz[y, x] = float(i), z

    put(4, 4, add((4.5, 2), (4.5, 6), (2.5, 2)))                  # t = 0 to the right; to the left two edges of the triangle are active
    put(9, 4, add((10, 2), (10, 6), (8, 2), 2.0))                 # t = 1/2: far, the empty pixel receives 0
    put(14, 4, add((15.5, 2), (15.5, 6), (13.5, 2)))              # t = 1
    put(22, 3, add((20.25, 2), (24.25, 6), (24.25, 2), 2.0))      # a 45-degree edge: the x pair takes it, the y pair refuses
    i = add((5, 12.5), (5, 16.5), (3, 12.5))                      # ends of the edge x = 5 exactly on the axes of rows 12 and 16
    put(4, 12, i)
    put(4, 16, i)
    put(10, 12, add((11.25, 10), (11.25, 14), (9.25, 10)), 0.5)   # equal z/w: the first pixel's triangle is analysed
    put(11, 12, add((10.75, 10), (10.75, 14), (12.75, 10)), 0.5)
    put(19, 14, add((20.25, 12), (20.25, 16), (18.25, 12)))       # the empty pixel (20, 14) receives from all four of its pairs
    put(21, 14, add((20.75, 12), (20.75, 16), (22.75, 12)))
    put(20, 13, add((18, 14.25), (22, 14.25), (18, 12.25), 2.0))
    put(20, 15, add((18, 14.75), (22, 14.75), (18, 16.75)))
    put(25, 12, add((26.25, 10), (26.25, 14), (24.25, 10)), 0.5)  # beside an id of T + 1 that is nearer: nothing is analysed
    n_single = len(tris)
    V = 3 * n_single
    X = [p for t in tris for p in t]
    w = [wv[k] for k in range(n_single) for _ in range(3)]
    tri = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(n_single)]
    # a quad split along its 45-degree diagonal: the diagonal is interior; and the same folded, where it is a silhouette
    X += [(4.25, 22), (8.25, 22), (8.25, 26), (4.25, 26)]
    tri += [[V, V + 1, V + 2], [V, V + 2, V + 3]]
    put(6, 23, len(tri) - 1)
    put(5, 23, len(tri))
    X += [(12.25, 22), (16.25, 22), (16.25, 26), (16.25, 24)]
    tri += [[V + 4, V + 5, V + 6], [V + 4, V + 6, V + 7]]
    put(14, 23, len(tri) - 1)
    w += [1.0] * 8
    T = len(tri)
    put(26, 12, T + 1, 0.125)
    X, w = torch.tensor(X, dtype=torch.float64)[None], torch.tensor(w, dtype=torch.float64)[None]
    pos = _clip(X, torch.zeros_like(w), w, H, W)
    rast = torch.zeros(1, H, W, 4)
    rast[0, ..., 2], rast[0, ..., 3] = zz, ids
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    color = (((7 * x + 13 * y) % 29 + 1).float() / 8.0)[None, ..., None]
    dy = ((((3 * x + 5 * y) % 11) - 5).float() / 4.0)
    dy = torch.where(dy == 0, torch.ones_like(dy), dy)[None, ..., None]
    return pos, torch.tensor(tri, dtype=torch.int32), rast, color.contiguous(), dy.contiguous()


def _case(name, why, geom, C, **kw):
    return dict(dict(name=name, why=why, geom=geom, C=C, boost=1.0, hint=False, empty=False, color_off=False, dy='aligned', one_term=False), **kw)


def _cases():
    out = []
    c = lambda *a, **kw: out.append(_case(*a, **kw))
    c('ties', 't = 0, 1/2, 1, a 45-degree edge, ends on the axis, equal z/w, four pairs into one pixel, the quad and its fold', 'ties', 1)
    for C in (1, 3, 4, 2, 5):
        c(f'soup/C{C}', 'two images of open triangles: word, wave and workgroup boundaries, the image border', 'soup', C)
    c('soup/one-term', 'dy at one receiving pixel per triangle: one term per entry of g_pos', 'soup', 3, one_term=True)
    c('mesh/B3', 'a closed mesh in three poses: silhouette bits per image, an odd batch for k_sil', 'mesh', 3)
    c('wide', 'five flag words, the last of three pixels; W % 4 != 0', 'wide', 3)
    c('range', 'pos [V,4] under two images: g_pos is the sum over the images', 'range', 3)
    c('boost', 'pos_gradient_boost = 3', 'soup', 3, boost=3.0)
    for W in (100, 102):
        for C, off in ((1, False), (1, True), (3, False)):
            if W == 102 and (C != 1 or off):
                continue
            for empty in (False, True):
                nm = f"hint/W{W}/C{C}{'+8B' if off else ''}{'/empty' if empty else ''}"
                c(nm, 'receivers in empty bins that face an occupied one; bins the hint switches off', f'hint{W}', C, hint=True, empty=empty, color_off=off)
    c('copy/105', '(1, 5, 7, 3): 26 float4 in the tail loop and one float left', 'copy105', 3)
    c('copy/2211', '(1, 33, 67, 1): one unrolled piece, a tail and three floats left', 'copy2211', 1)
    c('copy/4096', '(1, 32, 64, 2): two unrolled pieces and nothing else', 'copy4096', 2)
    c('copy/dy+8B', 'dy starts 8 bytes into a buffer: hipMemcpyAsync', 'copy2211', 1, dy='offset')
    c('copy/dy-stride0', 'the expanded scalar of out.sum().backward()', 'copy105', 3, dy='stride0')
    c('tiny/1x2', '(1, 1, 2, 1): two floats, no float4 at all', 'tiny12', 1)
    c('tiny/1x1', '(1, 1, 1, 3): one pixel, no pair', 'tiny11', 3)
    c('tiny/2x1', '(1, 2, 1, 1): one y pair', 'tiny21', 1)
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
SHAPES = {'ties': (1, 32, 32), 'soup': (2, 40, 72), 'mesh': (3, 48, 48), 'wide': (1, 9, 259), 'range': (2, 40, 72), 'hint100': (1, 70, 100),
          'hint102': (1, 70, 102), 'copy105': (1, 5, 7), 'copy2211': (1, 33, 67), 'copy4096': (1, 32, 64), 'tiny12': (1, 1, 2),
          'tiny11': (1, 1, 1), 'tiny21': (1, 2, 1)}
SOUP_SEED, MESH_SEED, RANGE_SEED = 11, 5, 7


@functools.lru_cache(maxsize=None)
def _geometry(geom):
    """-> (pos, tri, rast) of a geometry; ties also colour and dy.  Cached: treat as read-only."""
    B, H, W = SHAPES[geom]
    gen = torch.Generator().manual_seed(100 + sum(ord(ch) for ch in geom))
    if geom == 'ties':
        return _ties()
    if geom == 'soup':
        return _soup(B, H, W, 70, 9.0, SOUP_SEED)
    if geom == 'range':
        return _soup(B, H, W, 70, 9.0, RANGE_SEED, range_mode=True)
    if geom == 'mesh':
        return _mesh(H, W, MESH_SEED)
    if geom == 'wide':
        return _hand(WIDE_TRIS, H, W, gen)
    if geom.startswith('hint'):
        return _hand(HINT_TRIS, H, W, gen, ghosts=1)
    if geom == 'copy105':
        return _hand([[(1.2, 0.3), (5.6, 2.2), (2.1, 4.7)]], H, W, gen)
    if geom.startswith('copy'):
        return _soup(B, H, W, max(4, H * W // 60), 5.0, 3)
    tiny = {'tiny12': [(0.2, -1.0), (1.2, 0.4), (0.1, 2.0)], 'tiny11': [(-1.0, -1.0), (3.0, -1.0), (0.0, 3.0)], 'tiny21': [(-1.0, 0.1), (2.0, 0.2), (0.4, 1.2)]}
    return _hand([tiny[geom]], H, W, gen)


def plane1_off_pixels(hint, B, H, W):
    """[B,H,W] bool: the pixels of the bins whose plane 1 is off -- the bin and its eight neighbours are empty."""
    return hint_off_pixels(hint[1:2], B, H, W)


def plant_off_bins(rast, hint, rast_ghost):
    """rast with the covered pixels of rast_ghost (a triangle that rast does not show, with blended pairs of its own) in every bin
    whose plane 1 is off."""
    B, H, W, _ = rast.shape
    off = plane1_off_pixels(hint, B, H, W)
    r = rast.clone()
    r[off] = rast_ghost[off]
    return r


@functools.lru_cache(maxsize=None)
def _inputs_cached(name):
    c = CASES[CASE_IDS.index(name)]
    g = _geometry(c['geom'])
    pos, tri, rast = g[:3]
    B, H, W, _ = rast.shape
    C = c['C']
    gen = torch.Generator().manual_seed(9000 + sum(ord(ch) for ch in ('soup/C3' if name == 'boost' else name)))      # (boost: soup/C3's inputs)
    if c['geom'] == 'ties':
        color, dy = g[3], g[4]
    else:
        color, dy = _randn_away((B, H, W, C), gen), _randn_away((B, H, W, C), gen)
    if c['dy'] == 'stride0':
        dy = torch.ones(B, H, W, C)
    inp = dict(name=name, color=color, rast=rast, pos=pos, tri=tri, adj=topology(tri), dy=dy, boost=c['boost'], hint=None, empty_color=None,
               one_term=c['one_term'], dyadic=c['geom'] == 'ties')
    if c['hint']:
        inp['hint'] = make_hint(rast)
        inp['rast_planted'] = plant_off_bins(rast, inp['hint'], g[3])
        if c['empty']:
            inp['empty_color'] = torch.tensor([0.1875, -0.75, 1.5][:C])
            color[plane1_off_pixels(inp['hint'], B, H, W)] = inp['empty_color']
    if c['one_term']:
        # dy at one pixel per (image, triangle): the receiver of one of its active entries that receives nothing else
        D = decisions(color, rast, pos, tri, inp['adj'])
        count = torch.bincount(D.er, minlength=B * H * W)
        keep = torch.zeros(B * H * W, dtype=torch.bool)
        seen = set()
        for k in range(D.ei.numel()):
            key = (int(D.pairs.b[D.ei[k]]), int(D.pairs.tau[D.ei[k]]))
            if key not in seen and count[D.er[k]] == 1:
                seen.add(key)
                keep[D.er[k]] = True
        inp['dy'] = torch.where(keep.reshape(B, H, W, 1), dy, torch.zeros_like(dy))
        inp['n_one_term'] = len(seen)
    return inp


def case_inputs(name):
    """The float32 inputs of a case: dict with color, rast, pos ([B,V,4], or [V,4] in `range`), tri, adj (topology(tri)), dy, boost,
    hint / empty_color (hinted cases), one_term, dyadic.  Cached: treat as read-only."""
    return _inputs_cached(name)


@functools.lru_cache(maxsize=None)
def _reference_cached(name, dtype):
    i = _inputs_cached(name)
    return antialias(i['color'], i['rast'], i['pos'], i['tri'], i['adj'], i['dy'], i['boost'], dtype=dtype)


def reference(inp, dtype=torch.float64):
    """antialias() on a case's inputs.  Cached: treat as read-only."""
    return _reference_cached(inp['name'], dtype)


def kernel_order(inp, hint=None):
    return float32_in_kernel_order(inp['color'], inp['rast'], inp['pos'], inp['tri'], inp['adj'], inp['dy'], inp['boost'], hint=hint)


TOPOLOGY_CASES = {
    'T1': [[0, 1, 2]],
    'three on an edge': [[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 3, 4]],
    'a triangle twice': [[0, 1, 2], [0, 1, 2], [3, 4, 5]],
    'same opposite vertex': [[0, 1, 2], [1, 0, 2], [3, 4, 5]],
}


def topology_tri(name):
    """[T,3] int32 of a topology case: the hand-written ones, or 'strip/T': a triangle strip of T triangles (6 T just below and above a
    power of two at 10 | 11 and 170 | 171), or 'strip/T/permuted'."""
    if name in TOPOLOGY_CASES:
        return torch.tensor(TOPOLOGY_CASES[name], dtype=torch.int32)
    parts = name.split('/')
    T = int(parts[1])
    tri = torch.tensor([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2] for k in range(T)], dtype=torch.int32)
    if len(parts) > 2:
        tri = tri[torch.randperm(T, generator=torch.Generator().manual_seed(T))]
    return tri


TOPOLOGY_IDS = list(TOPOLOGY_CASES) + ['strip/10', 'strip/11', 'strip/170', 'strip/171', 'strip/171/permuted']

"""float64 restatement on the CPU of the float side of the rasterize operator (csrc/rasterize.hip: k_bins over shade_pixel, k_grad over
shade_pixel_bwd of csrc/raster_math.h), forward and backward, without autograd: the yardstick of tests/test_gpu_rasterize.py, itself
checked on the CPU by tests/test_rasterize_ref.py.  Nothing here imports fpc_diffrend_amd or oracle.

Visibility is not restated (the triangle ids are pinned bit-exact elsewhere): every function takes ids [B,H,W] (triangle + 1, 0 = empty).

rasterize() takes the float32 inputs the kernels read and evaluates in `dtype` (float64 by default; float32 gives "the same formula in
float32 by torch", the yardstick e32) the formula of shade_pixel, and with go = d loss / d rast (only .x and .y count: z/w receives and
gives no gradient, the id has none) and go_db = d loss / d rast_db the nine components of shade_pixel_bwd per pixel, summed per vertex with
index_add_ -- per image for pos [B,V,4], over the batch for pos [V,4] (range mode).  For every output it returns (value, S).

S is a first-order bound of the entry's rounding error in units of u = 2^-24, carried along with every value (class Q) from the inputs down:
    an input x (a coordinate of pos, an entry of go or go_db)     S = |x|
    a + b, a - b                                                   S_a + S_b
    a b                                                            S_a |b| + |a| S_b
    a / d                                                          S_a / |d| + |a / d| S_d / |d|
    a value clamped to a constant, a branch not taken              the constant's magnitude (0 for the closed gate of a clamp)
    g_pos                                                          the sum of S over the contributing pixels
The pixel's own constants fx = (2 px + 1) / W - 1, fy, sx = 2 / W, sy are coefficients without a scale: P_kx = |x_k| + |fx w_k| is the scale
of p_kx = x_k - fx w_k, A0 = P1x |p2y| + |p1x| P2y + P1y |p2x| + |p1y| P2x that of a0, At = A0 + A1 + A2, S_u = A0 / |at| + |b0| At / |at|
(iw = 1 / at has S = |iw| At / |at|, and b0 = a0 iw the product rule).  What float32 loses in fx itself (1.5 u absolute at most) is therefore
part of e32, which is measured and not derived.  An entry with S = 0 has no term and must be exactly 0: uncovered pixels, a barycentric the
clamp puts at 0, vertices that only show in pixels without a gradient or that no visible triangle names, the z column of g_pos
(predicted_zeros counts them from the pattern of ids, gates and zeroed gradients).

float32_in_kernel_order() is the same sequence of operations on float32 tensors, one rounded operation each, in the order of shade_pixel
and shade_pixel_bwd: at = (a0 + a1) + a2, iw = 1 / at, b0 = a0 * iw, z/w = ((a0 z0 + a1 z1) + a2 z2) / ((a0 w0 + a1 w1) + a2 w2) clamped,
dudx = ((da0x - b0 datx) * iw) * sx, the clamp, sc = 1 / (uc + vc) only where that sum exceeds 1, and the backward's accumulators in program
order.  The library is built with -ffp-contract=off and IEEE division, so the kernels must equal it bit for bit.

gate_margin(): float64 and float32 must take the same clamp and renormalise branches or their gradients differ by a whole term, so for
every covered pixel with a gradient |b0|, |b1|, |1 - b0|, |1 - b1| and |1 - b0 - b1| each exceed GATE_MARGIN u times their own scale; the
constructions below move or redraw what shows a pixel closer than SETTLE_MARGIN until no pixel needs to be left out.

CASES / case_inputs: the geometry and upstream gradients of every GPU case; ids come from the function handed in (oracle.ops)."""
import functools

import torch

from fitstep_ref import U, measure, rel_l2      # noqa: F401  (re-exported: the conventions of the fit step's yardstick)

BIN = 32              # FPCDR_OCC_BIN: k_bins and k_grad work on 32 x 32-pixel bins
VT_SLOTS = 256        # FPCDR_VT_SLOTS: the vertices the LDS table of a k_grad workgroup holds before vtable_add goes to global atomics
GATE_MARGIN = 64.0
SETTLE_MARGIN = 72.0     # what the constructions hold themselves to: an eighth above the margin the tests assert

MUTANT = None         # set by test_rasterize_ref.py only: a deliberately wrong restatement (see there)


class Q:
    """A value and its scale S (module docstring).  Values see exactly the operations written, one torch operation each."""
    __slots__ = ('v', 'S')

    def __init__(self, v, S):
        self.v, self.S = v, S

    @staticmethod
    def of(x):
        return x if isinstance(x, Q) else Q(x, torch.zeros_like(x) if torch.is_tensor(x) else 0.0)

    def __add__(a, b):
        b = Q.of(b)
        return Q(a.v + b.v, a.S + b.S)

    def __sub__(a, b):
        b = Q.of(b)
        return Q(a.v - b.v, a.S + b.S)

    def __rsub__(a, b):
        b = Q.of(b)
        return Q(b.v - a.v, a.S + b.S)

    def __neg__(a):
        return Q(-a.v, a.S)

    def __mul__(a, b):
        b = Q.of(b)
        return Q(a.v * b.v, a.S * abs(b.v) + abs(a.v) * b.S)

    def __truediv__(a, b):
        b = Q.of(b)
        q = a.v / b.v
        return Q(q, a.S / abs(b.v) + abs(q) * b.S / abs(b.v))

    def __rtruediv__(a, b):
        return Q.of(b) / a


def _inp(x):
    return Q(x, x.abs())


def _where(c, a, b):
    a, b = Q.of(a), Q.of(b)
    full = lambda x: x if torch.is_tensor(x) and x.shape == c.shape else torch.zeros(c.shape, dtype=a.v.dtype) + x
    return Q(torch.where(c, full(a.v), full(b.v)), torch.where(c, full(a.S), full(b.S)))


def _clamp(a, lo, hi):
    v = a.v.clamp(lo, hi)
    return Q(v, torch.where(v == a.v, a.S, v.abs()))


class _Pixels:
    """The covered pixels of ids, the vertices they gather and shade_pixel on them, in dtype."""

    def __init__(self, pos, tri, ids, resolution, dtype):
        H, W = int(resolution[0]), int(resolution[1])
        ids = ids.detach().cpu().long()
        B = ids.shape[0]
        assert tuple(ids.shape) == (B, H, W)
        self.B, self.H, self.W, self.dtype = B, H, W, dtype
        self.range_mode = pos.dim() == 2
        self.V = pos.shape[-2]
        self.bi, self.yy, self.xx = torch.nonzero(ids > 0, as_tuple=True)
        self.n = self.bi.numel()
        self.t = ids[self.bi, self.yy, self.xx] - 1
        self.vi = tri.detach().cpu().long()[self.t]                                            # [n,3]
        p = pos.detach().to('cpu', dtype).reshape(-1, 4)
        self.rows = [self.vi[:, k] + (0 if self.range_mode else self.bi * self.V) for k in range(3)]     # rows of pos.reshape(-1, 4)
        v = [p[r] for r in self.rows]
        x0, y0, z0, w0 = (_inp(v[0][:, c]) for c in range(4))
        x1, y1, z1, w1 = (_inp(v[1][:, c]) for c in range(4))
        x2, y2, z2, w2 = (_inp(v[2][:, c]) for c in range(4))
        coeff = lambda x: Q(x, torch.zeros_like(x))
        one = torch.ones(self.n, dtype=dtype)
        fx = coeff((2.0 * self.xx.to(dtype) + 1.0) / W - 1.0)
        fy = coeff((2.0 * self.yy.to(dtype) + 1.0) / (W if MUTANT == 'fy_formed_with_W' else H) - 1.0)
        sx, sy = coeff(2.0 * one / W), coeff(2.0 * one / H)
        if MUTANT == 'sx_sy_swapped':
            sx, sy = sy, sx
        p0x, p0y = x0 - fx * w0, y0 - fy * w0
        p1x, p1y = x1 - fx * w1, y1 - fy * w1
        p2x, p2y = x2 - fx * w2, y2 - fy * w2
        a0 = p1x * p2y - p1y * p2x
        a1 = p2x * p0y - p2y * p0x
        a2 = p0x * p1y - p0y * p1x
        at = a0 + a1 + a2
        iw = 1.0 / at
        b0 = a0 / at if MUTANT == 'b0_by_division' else a0 * iw
        b1 = a1 / at if MUTANT == 'b0_by_division' else a1 * iw
        zw = _clamp((a0 * z0 + a1 * z1 + a2 * z2) / (a0 * w0 + a1 * w1 + a2 * w2), -1.0, 1.0)
        da0x, da0y = w2 * p1y - w1 * p2y, w1 * p2x - w2 * p1x
        da1x, da1y = w0 * p2y - w2 * p0y, w2 * p0x - w0 * p2x
        da2x, da2y = w1 * p0y - w0 * p1y, w0 * p1x - w1 * p0x
        datx, daty = da0x + da1x + da2x, da0y + da1y + da2y
        self.db = [(da0x - b0 * datx) * iw * sx, (da0y - b0 * daty) * iw * sy, (da1x - b1 * datx) * iw * sx, (da1y - b1 * daty) * iw * sy]
        uc, vc = _clamp(b0, 0.0, 1.0), _clamp(b1, 0.0, 1.0)
        sum_ = uc + vc
        ren = sum_.v > 1.0
        sc = _where(ren, 1.0 / sum_, 1.0)
        self.uvz = [uc * sc, vc if MUTANT == 'renormalise_u_only' else vc * sc, zw]
        keep = dict(fx=fx, fy=fy, sx=sx, sy=sy, w=(w0, w1, w2), p=(p0x, p0y, p1x, p1y, p2x, p2y), a0=a0, a1=a1, iw=iw, b0=b0, b1=b1, uc=uc,
                    vc=vc, sum=sum_, ren=ren, da=(da0x, da0y, da1x, da1y, da2x, da2y), datx=datx, daty=daty)
        self.__dict__.update(keep)

    def image(self, qs):
        """[n] values of the covered pixels, one per channel, in images of zeros -> (value, S) [B,H,W,len(qs)]."""
        out = []
        for pick in (lambda q: q.v, lambda q: q.S):
            img = torch.zeros(self.B, self.H, self.W, len(qs), dtype=self.dtype)
            img[self.bi, self.yy, self.xx] = torch.stack([pick(q) + torch.zeros(self.n, dtype=self.dtype) for q in qs], 1)
            out.append(img)
        return tuple(out)

    def gates(self):
        """The five quantities whose sign decides a branch: b0, b1 (clamp below), 1 - b0, 1 - b1 (clamp above), 1 - b0 - b1 (renormalise)."""
        return [self.b0, self.b1, 1.0 - self.b0, 1.0 - self.b1, 1.0 - self.b0 - self.b1]

    def backward(self, g, gd):
        """shade_pixel_bwd: g [n,2] = d loss / d (u, v), gd [n,4] = d loss / d rast_db or None (HAS_DDB false) -> the nine components
        (vertex 0: x, y, w; vertex 1; vertex 2) as Q."""
        w0, w1, w2 = self.w
        p0x, p0y, p1x, p1y, p2x, p2y = self.p
        fx, fy, sx, sy, a0, a1, iw, b0, b1, uc, vc = self.fx, self.fy, self.sx, self.sy, self.a0, self.a1, self.iw, self.b0, self.b1, self.uc, self.vc
        gx, gy = _inp(g[:, 0]), _inp(g[:, 1])
        s = 1.0 / self.sum
        dot = (uc * gx + vc * gy) * s * s
        if MUTANT == 'renormalise_backward_without_dot':
            dot = dot * 0.0
        guc, gvc = _where(self.ren, gx * s - dot, gx), _where(self.ren, gy * s - dot, gy)
        open0, open1 = (b0.v >= 0.0) & (b0.v <= 1.0), (b1.v >= 0.0) & (b1.v <= 1.0)
        if MUTANT == 'clamp_gate_ignored':
            open0, open1 = torch.ones_like(open0), torch.ones_like(open1)
        gb0, gb1 = _where(open0, guc, 0.0), _where(open1, gvc, 0.0)
        zero = Q(torch.zeros(self.n, dtype=self.dtype), torch.zeros(self.n, dtype=self.dtype))
        ga0 = ga1 = ga2 = giw = gp0x = gp0y = gp1x = gp1y = gp2x = gp2y = gw0 = gw1 = gw2 = zero
        if gd is not None:
            da0x, da0y, da1x, da1y, da2x, da2y = self.da
            datx, daty = self.datx, self.daty
            hx0, hy0, hx1, hy1 = _inp(gd[:, 0]) * sx, _inp(gd[:, 1]) * sy, _inp(gd[:, 2]) * sx, _inp(gd[:, 3]) * sy
            n0x, n0y = da0x - b0 * datx, da0y - b0 * daty
            n1x, n1y = da1x - b1 * datx, da1y - b1 * daty
            giw = giw + (hx0 * n0x + hy0 * n0y + hx1 * n1x + hy1 * n1y)
            gn0x, gn0y, gn1x, gn1y = hx0 * iw, hy0 * iw, hx1 * iw, hy1 * iw
            gb0 = gb0 - (gn0x * datx + gn0y * daty)
            gb1 = gb1 - (gn1x * datx + gn1y * daty)
            gdatx, gdaty = -(gn0x * b0 + gn1x * b1), -(gn0y * b0 + gn1y * b1)
            gda0x, gda0y = gn0x + gdatx, gn0y + gdaty
            gda1x, gda1y = gn1x + gdatx, gn1y + gdaty
            gda2x, gda2y = gdatx, gdaty
            gw2 = gw2 + gda0x * p1y; gp1y = gp1y + gda0x * w2; gw1 = gw1 - gda0x * p2y; gp2y = gp2y - gda0x * w1
            gw1 = gw1 + gda0y * p2x; gp2x = gp2x + gda0y * w1; gw2 = gw2 - gda0y * p1x; gp1x = gp1x - gda0y * w2
            gw0 = gw0 + gda1x * p2y; gp2y = gp2y + gda1x * w0; gw2 = gw2 - gda1x * p0y; gp0y = gp0y - gda1x * w2
            gw2 = gw2 + gda1y * p0x; gp0x = gp0x + gda1y * w2; gw0 = gw0 - gda1y * p2x; gp2x = gp2x - gda1y * w0
            gw1 = gw1 + gda2x * p0y; gp0y = gp0y + gda2x * w1; gw0 = gw0 - gda2x * p1y; gp1y = gp1y - gda2x * w0
            gw0 = gw0 + gda2y * p1x; gp1x = gp1x + gda2y * w0; gw1 = gw1 - gda2y * p0x; gp0x = gp0x - gda2y * w1
        ga0, ga1 = ga0 + gb0 * iw, ga1 + gb1 * iw
        giw = giw + (gb0 * a0 + gb1 * a1)
        gat = -giw * iw * iw
        ga0, ga1, ga2 = ga0 + gat, ga1 + gat, ga2 + gat
        gp1x = gp1x + ga0 * p2y; gp2y = gp2y + ga0 * p1x; gp1y = gp1y - ga0 * p2x; gp2x = gp2x - ga0 * p1y
        gp2x = gp2x + ga1 * p0y; gp0y = gp0y + ga1 * p2x; gp2y = gp2y - ga1 * p0x; gp0x = gp0x - ga1 * p2y
        gp0x = gp0x + ga2 * p1y; gp1y = gp1y + ga2 * p0x; gp0y = gp0y - ga2 * p1x; gp1x = gp1x - ga2 * p0y
        if MUTANT == 'w_column_without_fx_fy':
            return [gp0x, gp0y, gw0, gp1x, gp1y, gw1, gp2x, gp2y, gw2]
        return [gp0x, gp0y, gw0 - fx * gp0x - fy * gp0y, gp1x, gp1y, gw1 - fx * gp1x - fy * gp1y, gp2x, gp2y, gw2 - fx * gp2x - fy * gp2y]


def _upstream(px, go, go_db, grad_db):
    """-> (g [n,2], gd [n,4] or None, with [n] bool: the pixels shade_pixel_bwd runs for -- k_grad skips a pixel whose six are all 0)."""
    g = go.detach().to('cpu', px.dtype)[px.bi, px.yy, px.xx][:, :2]
    gd = go_db.detach().to('cpu', px.dtype)[px.bi, px.yy, px.xx] if (grad_db and go_db is not None) else None
    if MUTANT == 'rast_db_chained_without_grad_db' and go_db is not None:
        gd = go_db.detach().to('cpu', px.dtype)[px.bi, px.yy, px.xx]
    with_g = (g != 0).any(1) if gd is None else ((g != 0).any(1) | (gd != 0).any(1))
    return g, gd, with_g


def _scatter(px, nine, pick, with_g):
    """sum the nine components per vertex: columns x, y, w of [B,V,4] (pos [B,V,4]) or of [V,4] (range mode: over the batch)."""
    Bp = 1 if px.range_mode else px.B
    G = torch.zeros(Bp * px.V, 4, dtype=px.dtype)
    sel = with_g.clone()
    if MUTANT == 'one_pixel_dropped':
        live = torch.nonzero(sel, as_tuple=True)[0]
        sel[live[live.numel() // 2]] = False
    if MUTANT == 'range_gradient_not_summed' and px.range_mode:
        sel &= px.bi == 0
    for k in range(3):
        for c, col in enumerate((0, 1, 3)):
            G[:, col].index_add_(0, px.rows[k][sel], pick(nine[3 * k + c])[sel])
    return G.reshape(px.V, 4) if px.range_mode else G.reshape(px.B, px.V, 4)


def rasterize(pos, tri, ids, resolution, go=None, go_db=None, grad_db=True, dtype=torch.float64):
    """pos [B,V,4] or [V,4] (range mode) float32, tri [T,3], ids [B,H,W], go [B,H,W,4] = d loss / d rast, go_db [B,H,W,4] = d loss / d rast_db
    or None -> dict: 'rast' (value, S) [B,H,W,3] = (u, v, z/w), 'rast_db' (value, S) [B,H,W,4], with go 'g_pos' (value, S) shaped like pos
    and 'nine' (value, S) [B,H,W,9], the per-pixel output of shade_pixel_bwd; 'px': the covered pixels (_Pixels), 'with_g': which of
    them carry a gradient."""
    px = _Pixels(pos, tri, ids, resolution, dtype)
    res = {'px': px, 'rast': px.image(px.uvz), 'rast_db': px.image(px.db)}
    if go is None:
        return res
    g, gd, with_g = _upstream(px, go, go_db, grad_db)
    nine = px.backward(g, gd)
    res['with_g'] = with_g
    res['nine'] = px.image(nine)
    res['g_pos'] = (_scatter(px, nine, lambda q: q.v, with_g), _scatter(px, nine, lambda q: q.S, with_g))
    return res


def float32_in_kernel_order(pos, tri, ids, resolution, go=None, go_db=None, grad_db=True):
    """-> dict name -> float32 tensor: 'rast' [B,H,W,3], 'rast_db' [B,H,W,4] and with go 'nine' [B,H,W,9] (zero where k_grad skips the
    pixel), every operation rounded on its own in the order of shade_pixel and shade_pixel_bwd (module docstring), and 'g_pos one term':
    the nine components put at their vertices, which is all of g_pos where every vertex has one contributing pixel."""
    r = rasterize(pos, tri, ids, resolution, go, go_db, grad_db, dtype=torch.float32)
    out = {'rast': r['rast'][0], 'rast_db': r['rast_db'][0]}
    if go is not None:
        px, with_g = r['px'], r['with_g']
        nine = r['nine'][0].clone()
        nine[px.bi[~with_g], px.yy[~with_g], px.xx[~with_g]] = 0.0
        out['nine'] = nine
        out['g_pos one term'] = r['g_pos'][0]
        out['px'] = px
    return out


def gate_margin(r):
    """min over the covered pixels with a gradient (all covered pixels without go) and the five gate quantities of |q| / (u S_q), float64."""
    px = r['px']
    sel = r['with_g'] if 'with_g' in r else torch.ones(px.n, dtype=torch.bool)
    if not bool(sel.any()):
        return float('inf')
    return min(float((q.v.abs() / (U * q.S))[sel].min()) for q in px.gates())


def corner_pixels(px):
    """[n] bool: the pixels whose centre lies beyond a vertex, outside both edges that meet there: b0 >= 1 with b1 <= 0, b1 >= 1 with
    b0 <= 0, or both <= 0 (vertex 2).  There the clamps alone make (u, v) = (1, 0), (0, 1) or (0, 0), exactly."""
    b0, b1 = px.b0.v, px.b1.v
    return ((b0 >= 1) & (b1 <= 0)) | ((b1 >= 1) & (b0 <= 0)) | ((b0 <= 0) & (b1 <= 0))


def unsafe_pixels(r):
    """[n] bool: the covered pixels with a gate quantity within SETTLE_MARGIN u of its scale from 0 (what a construction moves away)."""
    px = r['px']
    bad = torch.zeros(px.n, dtype=torch.bool)
    for q in px.gates():
        bad |= q.v.abs() <= SETTLE_MARGIN * U * q.S
    return bad


def predicted_zeros(inp, grad_db=True, output_db=True):
    """name -> the number of entries without any term, from the pattern of ids, float64 gates and zeroed gradients, never from values:
    rast: three per uncovered pixel, and a barycentric whose clamp stands at 0; rast_db: four per uncovered pixel; g_pos: the z column, and
    x, y, w of every vertex no pixel with a term shows."""
    r = rasterize(inp['pos'], inp['tri'], inp['ids'], inp['res'])
    px = r['px']
    B, H, W = px.B, px.H, px.W
    z = {'rast': 3 * (B * H * W - px.n) + int((px.b0.v <= 0).sum()) + int((px.b1.v <= 0).sum()), 'rast_db': 4 * (B * H * W - px.n)}
    g = inp['go'][px.bi, px.yy, px.xx][:, :2] != 0
    either = g.any(1)
    has_u, has_v = torch.where(px.ren, either, g[:, 0]), torch.where(px.ren, either, g[:, 1])
    open0, open1 = (px.b0.v >= 0) & (px.b0.v <= 1), (px.b1.v >= 0) & (px.b1.v <= 1)
    term = (open0 & has_u) | (open1 & has_v)
    if grad_db and output_db and inp['go_db'] is not None:
        term |= (inp['go_db'][px.bi, px.yy, px.xx] != 0).any(1)
    shown = torch.zeros((1 if px.range_mode else B) * px.V, dtype=torch.int64)
    for k in range(3):
        shown.index_add_(0, px.rows[k][term], torch.ones(int(term.sum()), dtype=torch.int64))
    z['g_pos'] = shown.numel() + 3 * int((shown == 0).sum())
    return z


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_rasterize.py
# ---------------------------------------------------------------------------------------------------------------------

def _clip(X, z, w, H, W):
    """pixel coordinates X [...,2] (pixel (px, py) has its centre at (px + 0.5, py + 0.5)), z/w and w -> float32 clip-space pos [...,4]."""
    ndc = torch.stack([2.0 * X[..., 0] / W - 1.0, 2.0 * X[..., 1] / H - 1.0, z], -1)
    return torch.cat([ndc * w[..., None], w[..., None]], -1).float().contiguous()


def _randn_away(shape, gen):
    """randn with every magnitude raised by 0.1: no entry near 0."""
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    return torch.where(x < 0, x - 0.1, x + 0.1).float()


def _settle(X, z, w, tri, res, ids_of, gen, rounds=200):
    """Move (by up to 0.05 pixel a round) the vertices of every triangle that shows a pixel too close to a gate, until gate_margin
    holds for every covered pixel.  X [B,V,2] or [V,2] float64 -> (pos, ids)."""
    H, W = res
    for _ in range(rounds):
        pos = _clip(X, z, w, H, W)
        ids = ids_of(pos)
        r = rasterize(pos, tri, ids, res)
        bad = unsafe_pixels(r)
        if not bool(bad.any()):
            return pos, ids
        px = r['px']
        rows = torch.unique(torch.cat([px.rows[k][bad] for k in range(3)]))
        Xf = X.reshape(-1, 2)
        Xf[rows] += (torch.rand(rows.numel(), 2, generator=gen, dtype=torch.float64) - 0.5) * 0.1
    raise AssertionError("the construction does not settle")


LATTICE_SEED, SOUP_SEED, CONFETTI_SEED, GRID_SEED, BIG_SEED, RANGE_SEED = 12, 2, 3, 4, 5, 6
LATTICE_RES, BIG_RES, RES = (70, 100), (64, 96), (70, 100)
NUDGE = (0.35 / 256, 0.45 / 256)      # pixels


def _lattice_cell(cx, cy, gen):
    lx, ly = int(torch.randint(3, 12, (1,), generator=gen)), int(torch.randint(3, 11, (1,), generator=gen))
    ox, oy, s = (int(torch.randint(0, 2, (1,), generator=gen)) * 2 - 1 for _ in range(3))
    ax = 12 * cx + (0 if ox > 0 else 11) + 0.5
    ay = 11 * cy + (0 if oy > 0 else 10) + 0.5
    corners = torch.tensor([[ax, ay], [ax + ox * lx, ay], [ax, ay + oy * ly]], dtype=torch.float64)
    m = NUDGE[0] + torch.rand(3, 2, generator=gen, dtype=torch.float64) * (NUDGE[1] - NUDGE[0])
    corners = corners + s * m * torch.tensor([ox, oy], dtype=torch.float64)
    return (corners[torch.randperm(3, generator=gen)], torch.rand(3, generator=gen, dtype=torch.float64) * 1.8 - 0.9,
            torch.rand(3, generator=gen, dtype=torch.float64) * 2.0 + 0.5)


def _lattice(ids_of):
    """48 unshared right triangles, one per 12 x 11-pixel cell of an 8 x 6 grid (the bin column x >= 96 stays empty), legs of 3 to 11 (x)
    and 3 to 10 (y) pixels along the axes, mirrored at random, every vertex on a pixel centre and then nudged by NUDGE pixels per axis --
    all three of a triangle into it (s = +1: the centres along its legs lie outside in float arithmetic, those along the hypotenuse
    inside) or out of it (s = -1: the reverse).  Coverage is decided on positions snapped to 1/256 pixel, where the nudge is gone and the
    fill rule alone decides, so the covered ones among these centres have a float barycentric below 0 or a sum above 1.  The vertex order
    of every triangle is permuted at random, which spreads them over b0, b1 and the sum.  w in [0.5, 2.5].  A cell that shows a pixel
    too close to a gate is drawn again: towards the image's border that is a covered pixel at vertex 0 or 1, where 1 - b0 is a nudge
    over a leg and its scale that of b0 = 1."""
    H, W = LATTICE_RES
    gen = torch.Generator().manual_seed(LATTICE_SEED)
    cells = [_lattice_cell(i % 8, i // 8, gen) for i in range(48)]
    tri = torch.arange(3 * 48, dtype=torch.int32).reshape(48, 3)
    for _ in range(200):
        pos = _clip(torch.cat([c[0] for c in cells])[None], torch.cat([c[1] for c in cells])[None], torch.cat([c[2] for c in cells])[None], H, W)
        ids = ids_of(pos, tri)
        r = rasterize(pos, tri, ids, (H, W))
        redo = torch.unique(r['px'].t[unsafe_pixels(r)]).tolist()
        if not redo:
            return pos, tri, ids, (H, W), None
        for i in redo:
            cells[i] = _lattice_cell(i % 8, i // 8, gen)
    raise AssertionError("the construction does not settle")


def _soup_geometry(B, T, gen, H, W, size_px):
    X = torch.stack([torch.rand(B, T, 1, generator=gen, dtype=torch.float64) * (W + 20) - 10,
                     torch.rand(B, T, 1, generator=gen, dtype=torch.float64) * (H + 20) - 10], -1)
    X = X + (torch.rand(B, T, 3, 2, generator=gen, dtype=torch.float64) * 2 - 1) * size_px
    z = torch.rand(B, T * 3, generator=gen, dtype=torch.float64) * 1.8 - 0.9
    w = torch.rand(B, T * 3, generator=gen, dtype=torch.float64) * 2.5 + 0.5
    return X.reshape(B, T * 3, 2), z, w, torch.arange(T * 3, dtype=torch.int32).reshape(T, 3)


def _soup(ids_of):
    """Two images of 400 overlapping unshared triangles of up to 25 pixels, mixed facing, some off screen: W % 32 and H % 32 are not 0."""
    H, W = RES
    gen = torch.Generator().manual_seed(SOUP_SEED)
    X, z, w, tri = _soup_geometry(2, 400, gen, H, W, 12.0)
    pos, ids = _settle(X, z, w, tri, (H, W), lambda p: ids_of(p, tri), gen)
    return pos, tri, ids, (H, W), None


def _confetti(ids_of):
    """3000 unshared triangles of up to 6 pixels in one image: hundreds of distinct vertices under every 32 x 32 bin."""
    H, W = RES
    gen = torch.Generator().manual_seed(CONFETTI_SEED)
    X, z, w, tri = _soup_geometry(1, 3000, gen, H, W, 3.0)
    pos, ids = _settle(X, z, w, tri, (H, W), lambda p: ids_of(p, tri), gen)
    return pos, tri, ids, (H, W), None


GRID_NX, GRID_NY = 9, 7


def _grid(ids_of):
    """A 9 x 7-vertex mesh over two images, every quad split along the same diagonal (an inner vertex is named by six triangles), the
    vertices jittered by up to 1.5 pixels, w rising across the mesh (perspective): the mesh spans every bin of the image."""
    H, W = RES
    gen = torch.Generator().manual_seed(GRID_SEED)
    B = 2
    gy, gx = torch.meshgrid(torch.arange(GRID_NY, dtype=torch.float64), torch.arange(GRID_NX, dtype=torch.float64), indexing='ij')
    base = torch.stack([4.0 + gx * (W - 8.0) / (GRID_NX - 1), 4.0 + gy * (H - 8.0) / (GRID_NY - 1)], -1).reshape(-1, 2)
    X = base[None] + (torch.rand(B, base.shape[0], 2, generator=gen, dtype=torch.float64) * 2 - 1) * 1.5
    w = 0.8 + 1.5 * (gx / (GRID_NX - 1)).reshape(-1)[None] * torch.tensor([[1.0], [0.4]], dtype=torch.float64) \
        + 0.3 * torch.rand(B, base.shape[0], generator=gen, dtype=torch.float64)
    z = torch.rand(B, base.shape[0], generator=gen, dtype=torch.float64) * 1.0 - 0.5
    quads = [(y * GRID_NX + x) for y in range(GRID_NY - 1) for x in range(GRID_NX - 1)]
    tri = torch.tensor([t for q in quads for t in ((q, q + 1, q + GRID_NX + 1), (q, q + GRID_NX + 1, q + GRID_NX))], dtype=torch.int32)
    pos, ids = _settle(X, z, w, tri, (H, W), lambda p: ids_of(p, tri), gen)
    return pos, tri, ids, (H, W), None


def _big(ids_of):
    """Two triangles over four vertices far outside a 64 x 96 frame, different w at every vertex: the tile path of the raster; every
    wave pass of k_grad is one run of 64 equal keys, and thousands of pixels sum into one vertex."""
    H, W = BIG_RES
    gen = torch.Generator().manual_seed(BIG_SEED)
    X = torch.tensor([[-40.3, -31.7], [150.9, -22.4], [139.2, 101.6], [-28.8, 90.1]], dtype=torch.float64)[None]
    w = torch.tensor([[0.7, 1.9, 1.2, 2.4]], dtype=torch.float64)
    z = torch.tensor([[-0.5, 0.3, 0.6, -0.2]], dtype=torch.float64)
    tri = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    pos, ids = _settle(X, z, w, tri, (H, W), lambda p: ids_of(p, tri), gen)
    return pos, tri, ids, (H, W), None


def _range(ids_of_ranges):
    """Range mode: one vertex array [V,4] of 400 unshared triangles, four images that draw the slices (first, count) of
    tests/test_gpu_parity.py::test_range_mode_matches_oracle, its empty one among them."""
    H, W = RES
    gen = torch.Generator().manual_seed(RANGE_SEED)
    T = 400
    X, z, w, tri = _soup_geometry(1, T, gen, H, W, 12.0)
    ranges = torch.tensor([[0, T], [T // 3, T // 2], [5, 0], [T - 40, 40]], dtype=torch.int32)
    pos, ids = _settle(X[0], z[0], w[0], tri, (H, W), lambda p: ids_of_ranges(p, tri, ranges), gen)
    return pos, tri, ids, (H, W), ranges


def _dense(B, H, W, gen):
    return _randn_away((B, H, W, 4), gen), _randn_away((B, H, W, 4), gen)


def _one_per_triangle(pos, tri, ids, res, gen):
    """go and go_db nonzero at exactly one pixel of each visible triangle: the one whose smallest barycentric (of three) is lowest,
    which is a pixel outside the float triangle wherever the triangle has one."""
    r = rasterize(pos, tri, ids, res)
    px = r['px']
    low = torch.minimum(torch.minimum(px.b0.v, px.b1.v), 1.0 - px.b0.v - px.b1.v)
    key = px.bi * tri.shape[0] + px.t
    B, (H, W) = ids.shape[0], res
    go, go_db = torch.zeros(B, H, W, 4), torch.zeros(B, H, W, 4)
    for k in torch.unique(key).tolist():
        cand = torch.nonzero(key == k, as_tuple=True)[0]
        i = cand[torch.argmin(low[cand])]
        go[px.bi[i], px.yy[i], px.xx[i]] = _randn_away((4,), gen)
        go_db[px.bi[i], px.yy[i], px.xx[i]] = _randn_away((4,), gen)
    return go, go_db


SPARSE_OFF_BINS = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 1, 3), (1, 2, 0), (1, 0, 3)]      # (image, bin row, bin column)
SPARSE_ROW_DB_ONLY, SPARSE_ROW_ZW_ONLY = (1, 40), (1, 41)                                            # (image, pixel row)


def _sparse(B, H, W, gen):
    """go and go_db zero on whole bins (the `any` exit of k_grad) and on 30 % of the pixels elsewhere (the per-pixel skip); one row
    with d loss / du = d loss / dv = 0 but go_db != 0; one row where go is nonzero only in .z and .w, which gives no gradient."""
    go, go_db = _dense(B, H, W, gen)
    off = torch.rand(B, H, W, generator=gen) < 0.3
    for b, by, bx in SPARSE_OFF_BINS:
        off[b, by * BIN:(by + 1) * BIN, bx * BIN:(bx + 1) * BIN] = True
    go[off] = 0.0
    go_db[off] = 0.0
    b, y = SPARSE_ROW_DB_ONLY
    go[b, y, :, :2] = 0.0
    go_db[b, y] = _randn_away((W, 4), gen)
    b, y = SPARSE_ROW_ZW_ONLY
    go[b, y, :, :2] = 0.0
    go[b, y, :, 2:] = _randn_away((W, 2), gen)
    go_db[b, y] = 0.0
    return go, go_db


# name -> (geometry, upstream gradients, what the case is there for)
CASES = {
    'lattice': ('lattice', 'dense', 'clamp gates, renormalise forward and backward, exact corners, empty bins in the hint'),
    'soup': ('soup', 'dense', 'partial bins: out-of-image lanes in the middle of the wave of k_grad'),
    'confetti': ('confetti', 'dense', 'more than 256 distinct vertices in a bin: the global-atomic fallback of vtable_add'),
    'grid': ('grid', 'dense', 'shared vertices: six triangles into one vertex, atomics between workgroups'),
    'big': ('big', 'dense', 'the tile path; runs of 64 equal keys; thousands of pixels into one vertex'),
    'lattice/one-per-triangle': ('lattice', 'one', 'one term per g_pos entry: shade_pixel_bwd bit for bit, clamp and renormalise included'),
    'soup/one-per-triangle': ('soup', 'one', 'the same on two images of a soup'),
    'soup/sparse-gradient': ('soup', 'sparse', 'the `any` exit, the per-pixel skip, rows with only go_db or only .z / .w'),
    'range': ('range', 'dense', 'pos [V,4] with ranges: the gradient summed over the images, an empty range'),
}
# (case, form): every case with and without the rast_db gradient, soup also through a context without rast_db
FORMS = [(name, form) for name in CASES for form in ('grad_db', 'no grad_db')] + [('soup', 'no rast_db')]
FORM_IDS = [f"{n}/{f.replace(' ', '_')}" for n, f in FORMS]

_geometry_cache, _case_cache = {}, {}


def case_inputs(name, oracle_ops):
    """The inputs of a case: dict with pos (float32 [B,V,4], or [V,4] in range mode), tri, ids (from oracle_ops.rasterize_ids /
    rasterize_ids_ranges), res = (H, W), ranges (int32 [B,2] or None), go, go_db [B,H,W,4].  Cached: treat as read-only."""
    if name in _case_cache:
        return _case_cache[name]
    geom, grads, _ = CASES[name]
    if geom not in _geometry_cache:
        res = {'lattice': LATTICE_RES, 'big': BIG_RES}.get(geom, RES)
        if geom == 'range':
            ids_of = lambda p, tri, ranges: oracle_ops.rasterize_ids_ranges(p, tri, res, ranges)
        else:
            ids_of = lambda p, tri: oracle_ops.rasterize_ids(p, tri, res)
        _geometry_cache[geom] = {'lattice': _lattice, 'soup': _soup, 'confetti': _confetti, 'grid': _grid, 'big': _big, 'range': _range}[geom](ids_of)
    pos, tri, ids, res, ranges = _geometry_cache[geom]
    gen = torch.Generator().manual_seed(7000 + sum(ord(ch) for ch in name))
    B, (H, W) = ids.shape[0], res
    go, go_db = {'dense': lambda: _dense(B, H, W, gen), 'one': lambda: _one_per_triangle(pos, tri, ids, res, gen),
                 'sparse': lambda: _sparse(B, H, W, gen)}[grads]()
    _case_cache[name] = dict(name=name, pos=pos, tri=tri, ids=ids, res=res, ranges=ranges, go=go, go_db=go_db)
    return _case_cache[name]


@functools.lru_cache(maxsize=None)
def _reference_cached(name, form, dtype):
    inp = _case_cache[name]
    return rasterize(inp['pos'], inp['tri'], inp['ids'], inp['res'], inp['go'], None if form == 'no rast_db' else inp['go_db'],
                     grad_db=form == 'grad_db', dtype=dtype)


def reference(inp, form, dtype=torch.float64):
    """rasterize() on a case's inputs in one of the three forms ('grad_db', 'no grad_db', 'no rast_db').  Cached: treat as read-only."""
    assert _case_cache.get(inp['name']) is inp
    return _reference_cached(inp['name'], form, dtype)


def kernel_order(inp, form):
    return float32_in_kernel_order(inp['pos'], inp['tri'], inp['ids'], inp['res'], inp['go'], None if form == 'no rast_db' else inp['go_db'],
                                   grad_db=form == 'grad_db')


def bin_vertex_counts(r):
    """(B, bin rows, bin columns) -> the number of distinct vertices the bin's pixels with a gradient name: what a k_grad workgroup
    puts into its table."""
    px = r['px']
    sel = r['with_g']
    out = {}
    key = (px.bi * 1000 + (px.yy // BIN)) * 1000 + px.xx // BIN
    for k in torch.unique(key[sel]).tolist():
        m = sel & (key == k)
        out[(k // 1000000, (k // 1000) % 1000, k % 1000)] = int(torch.unique(torch.cat([px.rows[c][m] for c in range(3)])).numel())
    return out

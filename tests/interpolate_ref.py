"""float64 restatement on the CPU of the interpolate operator (csrc/interpolate.hip), forward and backward, without autograd: the
yardstick of tests/test_gpu_interpolate.py, itself checked on the CPU by tests/test_interpolate_ref.py.  Nothing here imports
fpc_diffrend_amd or oracle.

interpolate() takes the float32 inputs the kernels read and evaluates in `dtype` (float64 by default; float32 gives "the same formula
in float32 by torch", the yardstick e32 of the long sum).  For every output it returns (value, S): S is the entry's formula with every
factor replaced by its absolute value and every subtraction by an addition; an error is measured per entry in units of u = 2^-24
against S (fitstep_ref.measure), and an entry with S = 0 has no term and must be exactly 0.

A pixel is covered iff t = int(rast.w) - 1 lies in [0, T).  With (u, v) = rast.xy, w = 1 - u - v, (i0, i1, i2) = tri[t],
a_c = attr[b or 0, i_c], d = rast_db, kd_j = diff_list[j], g = d loss / d out, (gx_j, gy_j) = d loss / d out_da[2j, 2j + 1]:
    out_k        = u a0_k + v a1_k + w a2_k
    out_da[2j]   = d.x (a0 - a2)[kd_j] + d.z (a1 - a2)[kd_j]          out_da[2j + 1]: d.y, d.w
    g_rast.x     = sum_k g_k (a0_k - a2_k)                            .y: a1;  .z = .w = 0
    g_rast_db.x  = sum_j gx_j (a0 - a2)[kd_j]      .y: gy_j;  .z: gx_j (a1 - a2)[kd_j];  .w: gy_j (a1 - a2)[kd_j]
    g_attr[i0,k] += u g_k + ge0_k,   ge0_k = sum_{j: kd_j = k} (gx_j d.x + gy_j d.y)
    g_attr[i1,k] += v g_k + ge1_k,   ge1_k = sum_{j: kd_j = k} (gx_j d.z + gy_j d.w)
    g_attr[i2,k] += w g_k - ge0_k - ge1_k
summed over every covered pixel (per image with Ba = B, over the batch with Ba = 1).  A repeated index in diff_list gives two pairs in
out_da and sums twice into g_attr.

The module also holds the inputs of every GPU case (CASES, case_inputs) -- rast is synthetic, so ids, barycentrics and empty regions
are under the test's control --, a restatement in integers of the two dispatch conditions of the host code (dispatch), the region
hint of a rast (make_hint, hint_off_pixels, poison_off_bins) and the float32 statement of the four non-atomic outputs with the kernels' order of
operations (float32_in_kernel_order), to which the kernels must be bit-identical."""
import torch

from fitstep_ref import U, measure, rel_l2      # noqa: F401  (re-exported: the conventions of the fit step's yardstick)

# Rounded operations that reach one entry, n (rules of fitstep_ref.py: an input has n = 0; a product n_a + n_b + 1; a sum of k terms
# max n_i + k - 1).  The entry's error is then at most (n + 2) u of S.
# out: w = 1 - u - v is a sum of three terms, 2; the products u a0 and v a1 1, w a2 3; the sum of three 3 + 2 = 5.
N_OUT = 5
# out_da: the difference 1, the product 2, the sum of two 3.
N_OUT_DA = 3
# g_rast.x: the difference 1, the product 2, the sum of A terms 2 + A - 1.
N_G_RAST = lambda A: A + 1
# g_rast_db: the same over the n_diff pairs.
N_G_RAST_DB = lambda n_diff: n_diff + 1

MAX_ATTR = 32       # FPCDR_MAX_ATTR: the most attributes that may carry differentials
BIN = 32            # FPCDR_OCC_BIN
VT, T = 100, 60     # vertices and triangles of every synthetic case

MUTANT = None       # set by test_interpolate_ref.py only: a deliberately wrong restatement (see there)

NON_ATOMIC = ('out', 'out_da', 'g_rast', 'g_rast_db')


def _c(t, dtype):
    return t.detach().to('cpu', dtype)


def diff_indices(diff, A):
    return [] if diff is None else (list(range(A)) if diff == 'all' else [int(k) for k in diff])


class _Pixels:
    """The covered pixels of a rast and what they gather, in dtype."""

    def __init__(self, attr, rast, tri, rast_db, dtype):
        B, H, W, _ = rast.shape
        Ba, Vt, A = attr.shape
        nT = tri.shape[0]
        self.B, self.H, self.W, self.Ba, self.Vt, self.A, self.P = B, H, W, Ba, Vt, A, B * H * W
        r = _c(rast, dtype).reshape(-1, 4)
        tid = rast.detach().cpu().reshape(-1, 4)[:, 3].to(torch.int64) - 1           # (int)r.w - 1: truncation
        if MUTANT == 'accepts_T_plus_1':
            tid = torch.where(tid == nT, torch.full_like(tid, nT - 1), tid)
        self.covered = (tid >= 0) & (tid < nT)
        self.m = torch.nonzero(self.covered, as_tuple=True)[0]
        vi = tri.detach().cpu().long()[tid[self.m]]
        b = self.m // (H * W)
        base = b * Vt if (Ba > 1 and MUTANT != 'no_batch_offset') else torch.zeros_like(b)
        self.rows = [base + vi[:, c] for c in range(3)]                              # rows of attr.reshape(Ba * Vt, A)
        at = _c(attr, dtype).reshape(Ba * Vt, A)
        self.a = [at[i] for i in self.rows]
        self.u, self.v = r[self.m, 0:1], r[self.m, 1:2]
        self.d = _c(rast_db, dtype).reshape(-1, 4)[self.m] if rast_db is not None else None

    def full(self, val, width, dtype):
        """val [n, width] of the covered pixels in an image of zeros [B, H, W, width]."""
        out = torch.zeros(self.P, width, dtype=dtype)
        out[self.m] = val
        return out.reshape(self.B, self.H, self.W, width)


def _scatter(px, contrib, dtype, order):
    """sum the three [n, A] contributions into [Ba, Vt, A].  order None: pixel by pixel as index_add_ does; a permutation of the
    covered pixels: in that order; 'wave64': 64 pixels at a time summed by vertex first, as a wave does before its atomics."""
    G = torch.zeros(px.Ba * px.Vt, px.A, dtype=dtype)
    n = px.m.numel()
    if isinstance(order, str) and order == 'wave64':
        chunk = torch.arange(n) // 64
        nc = int(chunk.max()) + 1 if n else 1
        part = torch.zeros(nc * px.Ba * px.Vt, px.A, dtype=dtype)
        for rows, val in zip(px.rows, contrib):
            part.index_add_(0, chunk * (px.Ba * px.Vt) + rows, val)
        part = part.reshape(nc, px.Ba * px.Vt, px.A)
        for c in range(nc):
            G = G + part[c]
    else:
        sel = slice(None) if order is None else order
        for rows, val in zip(px.rows, contrib):
            G.index_add_(0, rows[sel], val[sel])
    return G.reshape(px.Ba, px.Vt, px.A)


def interpolate(attr, rast, tri, rast_db=None, diff_list=(), go=None, go_da=None, dtype=torch.float64, order=None):
    """attr [Ba,Vt,A], rast [B,H,W,4], tri [T,3] int32, rast_db [B,H,W,4] / None, diff_list: attribute indices, go [B,H,W,A],
    go_da [B,H,W,2 n_diff] -> dict name -> (value, S) for out, out_da (n_diff > 0), and with go g_rast, g_rast_db (n_diff > 0),
    g_attr; 'covered': [B,H,W] bool.  order: the order of the g_attr sum (_scatter)."""
    diff_list = list(diff_list)
    if MUTANT == 'sorted_diff':
        diff_list = sorted(diff_list)
    nd = len(diff_list)
    px = _Pixels(attr, rast, tri, rast_db if nd else None, dtype)
    A, P = px.A, px.P
    a0, a1, a2 = px.a
    u, v = px.u, px.v
    w = 1.0 - u - v
    ua, va, wa = u.abs(), v.abs(), 1.0 + u.abs() + v.abs()
    res = {'covered': px.covered.reshape(px.B, px.H, px.W)}
    res['out'] = (px.full(u * a0 + v * a1 + w * a2, A, dtype), px.full(ua * a0.abs() + va * a1.abs() + wa * a2.abs(), A, dtype))
    e0, e1 = a0 - a2, a1 - a2
    e0a, e1a = a0.abs() + a2.abs(), a1.abs() + a2.abs()
    if nd:
        d, da = px.d, px.d.abs()
        val, S = [], []
        for kd in diff_list:
            val += [d[:, 0] * e0[:, kd] + d[:, 2] * e1[:, kd], d[:, 1] * e0[:, kd] + d[:, 3] * e1[:, kd]]
            S += [da[:, 0] * e0a[:, kd] + da[:, 2] * e1a[:, kd], da[:, 1] * e0a[:, kd] + da[:, 3] * e1a[:, kd]]
        res['out_da'] = (px.full(torch.stack(val, 1), 2 * nd, dtype), px.full(torch.stack(S, 1), 2 * nd, dtype))
    if go is None:
        return res
    g = _c(go, dtype).reshape(P, A)[px.m]
    ga = g.abs()
    zero = torch.zeros(px.m.numel(), dtype=dtype)
    res['g_rast'] = (px.full(torch.stack([(g * e0).sum(1), (g * e1).sum(1), zero, zero], 1), 4, dtype),
                     px.full(torch.stack([(ga * e0a).sum(1), (ga * e1a).sum(1), zero, zero], 1), 4, dtype))
    ge0, ge1, ge0a, ge1a = (torch.zeros(px.m.numel(), A, dtype=dtype) for _ in range(4))
    if nd:
        gd = _c(go_da, dtype).reshape(P, 2 * nd)[px.m]
        gda = gd.abs()
        gx, gy, gxa, gya = gd[:, 0::2], gd[:, 1::2], gda[:, 0::2], gda[:, 1::2]
        sel0, sel1, sel0a, sel1a = e0[:, diff_list], e1[:, diff_list], e0a[:, diff_list], e1a[:, diff_list]
        res['g_rast_db'] = (px.full(torch.stack([(gx * sel0).sum(1), (gy * sel0).sum(1), (gx * sel1).sum(1), (gy * sel1).sum(1)], 1), 4, dtype),
                            px.full(torch.stack([(gxa * sel0a).sum(1), (gya * sel0a).sum(1), (gxa * sel1a).sum(1), (gya * sel1a).sum(1)], 1), 4, dtype))
        seen = set()
        for j, kd in enumerate(diff_list):
            if MUTANT == 'repeat_counts_once' and kd in seen:
                continue
            seen.add(kd)
            ge0[:, kd] += gx[:, j] * d[:, 0] + gy[:, j] * d[:, 1]
            ge1[:, kd] += gx[:, j] * d[:, 2] + gy[:, j] * d[:, 3]
            ge0a[:, kd] += gxa[:, j] * da[:, 0] + gya[:, j] * da[:, 1]
            ge1a[:, kd] += gxa[:, j] * da[:, 2] + gya[:, j] * da[:, 3]
    c2 = w * g - ge0 if MUTANT == 'vertex2_lacks_ge1' else w * g - ge0 - ge1
    G = _scatter(px, [u * g + ge0, v * g + ge1, c2], dtype, order)
    GS = _scatter(px, [ua * ga + ge0a, va * ga + ge1a, wa * ga + ge0a + ge1a], dtype, None)
    res['g_attr'] = (G, GS)
    return res


def float32_in_kernel_order(attr, rast, tri, rast_db=None, diff_list=(), go=None, go_da=None):
    """The four non-atomic outputs in float32 with the kernels' order of operations, every operation rounded on its own (the library
    is built with -ffp-contract=off): out = (u a0 + v a1) + w a2 with w = (1 - u) - v; out_da = d.x e0 + d.z e1; gu, gv and the four
    components of gdb accumulated from 0, channel by channel.  -> dict name -> float32 tensor."""
    f32 = torch.float32
    diff_list = list(diff_list)
    nd = len(diff_list)
    px = _Pixels(attr, rast, tri, rast_db if nd else None, f32)
    a0, a1, a2 = px.a
    u, v = px.u, px.v
    w = (1.0 - (u + v)) if MUTANT == 'w_as_1_minus_sum' else ((1.0 - u) - v)
    res = {'out': px.full((u * a0 + v * a1) + w * a2, px.A, f32)}
    d = px.d
    if nd:
        val = []
        for kd in diff_list:
            e0, e1 = a0[:, kd] - a2[:, kd], a1[:, kd] - a2[:, kd]
            val += [d[:, 0] * e0 + d[:, 2] * e1, d[:, 1] * e0 + d[:, 3] * e1]
        res['out_da'] = px.full(torch.stack(val, 1), 2 * nd, f32)
    if go is None:
        return res
    n = px.m.numel()
    g = _c(go, f32).reshape(px.P, px.A)[px.m]
    gu, gv = torch.zeros(n), torch.zeros(n)
    for k in range(px.A):
        gu = gu + g[:, k] * (a0[:, k] - a2[:, k])
        gv = gv + g[:, k] * (a1[:, k] - a2[:, k])
    res['g_rast'] = px.full(torch.stack([gu, gv, torch.zeros(n), torch.zeros(n)], 1), 4, f32)
    if nd:
        gd = _c(go_da, f32).reshape(px.P, 2 * nd)[px.m]
        acc = [torch.zeros(n) for _ in range(4)]
        for j, kd in enumerate(diff_list):
            e0, e1 = a0[:, kd] - a2[:, kd], a1[:, kd] - a2[:, kd]
            gx, gy = gd[:, 2 * j], gd[:, 2 * j + 1]
            acc = [acc[0] + gx * e0, acc[1] + gy * e0, acc[2] + gx * e1, acc[3] + gy * e1]
        res['g_rast_db'] = px.full(torch.stack(acc, 1), 4, f32)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the host's dispatch and the region hint, in integers
# ---------------------------------------------------------------------------------------------------------------------

def dispatch(A, n_diff, W, need_attr_grad, pointers=()):
    """The two dispatch conditions of fpcdr_interpolate_fwd and fpcdr_interpolate_bwd -> (forward kernel, backward kernel).
    pointers: (attr, out, dy) addresses, None or missing = 16-byte aligned.  The forward tests attr | out, the backward attr | dy."""
    p = list(pointers) + [None] * (3 - len(pointers))
    ok = lambda *ps: all(q is None or q % 16 == 0 for q in ps)
    shape = A == 2 and n_diff == 0 and W % 4 == 0
    fwd = 'k_interp_fwd_bin2' if (shape and ok(p[0], p[1])) else ('k_interp_fwd<2>' if A == 2 else 'k_interp_fwd<0>')
    if need_attr_grad:
        bwd = 'k_interp_bwd<true>'
    else:
        bwd = 'k_interp_bwd_bin2' if (shape and ok(p[0], p[2])) else 'k_interp_bwd_rows'
    return fwd, bwd


KERNELS = ('k_interp_fwd<0>', 'k_interp_fwd<2>', 'k_interp_fwd_bin2', 'k_interp_bwd<true>', 'k_interp_bwd_rows', 'k_interp_bwd_bin2')


def make_hint(rast, extra_on=()):
    """The region hint of a rast, uint8 [2, B, ceil(H/32), ceil(W/32)] (include/fpcdr.h): plane 0 is 1 wherever a bin holds a pixel
    that is not all zero, plane 1 is plane 0 OR-ed over the 3 x 3 neighbourhood.  extra_on: bins (b, by, bx) switched on although
    they are empty -- a hint is conservative."""
    B, H, W, _ = rast.shape
    OY, OX = (H + BIN - 1) // BIN, (W + BIN - 1) // BIN
    live = (rast.detach().cpu() != 0).any(-1).float()
    pad = torch.zeros(B, OY * BIN, OX * BIN)
    pad[:, :H, :W] = live
    p0 = pad.reshape(B, OY, BIN, OX, BIN).amax(dim=(2, 4))
    for b, by, bx in extra_on:
        p0[b, by, bx] = 1.0
    p1 = torch.nn.functional.max_pool2d(p0[:, None], 3, stride=1, padding=1)[:, 0]
    return torch.stack([p0, p1]).to(torch.uint8).contiguous()


def hint_off_pixels(hint, B, H, W, bins_per_row=None):
    """[B,H,W] bool: the pixels whose bin plane 0 of the hint calls empty, looked up as fpcdr_hint_on does, with
    bins_per_row = ceil(W / 32) bins in a row of the map (a wrong count is a mutant)."""
    OY, OX = (H + BIN - 1) // BIN, (W + BIN - 1) // BIN
    ox = OX if bins_per_row is None else bins_per_row
    flat = hint.reshape(-1)
    b = torch.arange(B)[:, None, None]
    y = torch.arange(H)[None, :, None] >> 5
    x = torch.arange(W)[None, None, :] >> 5
    return flat[((b * OY + y) * ox + x).expand(B, H, W)] == 0


def with_hint(rast, hint, bins_per_row=None):
    """What a hinted kernel computes from: a bin the hint calls empty is not read, it counts as rast = 0."""
    B, H, W, _ = rast.shape
    r = rast.clone()
    r[hint_off_pixels(hint, B, H, W, bins_per_row)] = 0.0
    return r


def poison_off_bins(rast, hint):
    """rast with covered-looking pixels (valid ids, barycentrics, depth) in every bin the hint calls empty.  A hinted kernel does not
    read those bins, so its results are those of `rast`; a kernel that ignored its hint would interpolate there."""
    B, H, W, _ = rast.shape
    off = hint_off_pixels(hint, B, H, W)
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    fake = torch.stack([torch.full((H, W), 0.3), torch.full((H, W), 0.4), torch.full((H, W), 0.5), (1 + (x + 3 * y) % T).float()], -1)
    r = rast.clone()
    r[off] = fake[None].expand(B, H, W, 4)[off]
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_interpolate.py (the CPU file measures float32 torch and the mutants on the same inputs)
# ---------------------------------------------------------------------------------------------------------------------

S_BIN, S_BIN2, S_STREAM, S_HINT = (2, 37, 40), (1, 44, 72), (2, 13, 259), (1, 70, 100)

# per shape: bins (b, by, bx) left without any covered pixel, bins covered in five pixels only, and (hinted shape) the empty bin
# the hint leaves on
LAYOUT = {
    S_BIN: dict(empty=[(0, 0, 0)], sparse=[(1, 0, 0)], extra_on=[]),
    S_BIN2: dict(empty=[], sparse=[(0, 1, 2)], extra_on=[]),
    S_STREAM: dict(empty=[(1, 0, 3)], sparse=[(0, 0, 8)], extra_on=[]),
    S_HINT: dict(empty=[(0, 0, 0), (0, 0, 3), (0, 1, 3), (0, 2, 0), (0, 2, 1), (0, 2, 2), (0, 2, 3)], sparse=[(0, 1, 0)], extra_on=[(0, 0, 0)]),
}


def _case(name, why, img, A, diff=None, BaB=False, attr_grad=True, ids='confetti', misalign=False, hint=False, seed=0):
    return dict(name=name, why=why, img=img, A=A, diff=diff, BaB=BaB, attr_grad=attr_grad, ids=ids, misalign=misalign, hint=hint, seed=seed)


def _cases():
    out = []
    c = lambda *a, **kw: out.append(_case(*a, **kw))
    s = S_BIN
    c('bin/A2/confetti', 'both bin-shaped kernels; an uncovered bin without a hint: the all-empty-wave exit', s, 2, attr_grad=False)
    c('bin/A2/one/BaB', 'the same with an attribute table per image, one triangle everywhere', s, 2, BaB=True, attr_grad=False, ids='one')
    c('bin/A2/runs/attr', 'bin-shaped forward, tiled backward with the scatter', s, 2, ids='runs')
    c('gen/A2+8B', 'attr 8 bytes into a buffer: the generic twins of the bin-shaped pair', s, 2, attr_grad=False, misalign=True)
    c('gen/A2+8B/attr', 'attr 8 bytes into a buffer, with its gradient', s, 2, ids='runs', misalign=True)
    c('gen/A2/all/BaB/attr', 'Ba = B together with differentials, the float4 store of k_interp_fwd<2>', s, 2, diff='all', BaB=True)
    c('gen/A2/all', 'differentials without an attribute gradient', s, 2, diff='all', attr_grad=False, ids='runs')
    c('gen/A1/attr', 'one channel', s, 1)
    c('gen/A1/all', 'one channel with its differential', s, 1, diff='all', attr_grad=False, ids='one')
    c('gen/A3/[2,0]/attr', 'diff_attrs in an order that is not sorted', s, 3, diff=[2, 0], ids='runs')
    c('gen/A3/[2,0,2]/BaB/attr', 'a repeated index: two pairs in out_da, summed twice into g_attr', s, 3, diff=[2, 0, 2], BaB=True)
    c('gen/A3/[2,0,2]', 'a repeated index without an attribute gradient', s, 3, diff=[2, 0, 2], attr_grad=False)
    c('gen/A5/all/one/attr', 'one triangle everywhere: one group of 64 in the wave reduction', s, 5, diff='all', ids='one')
    c('gen/A5', 'five channels, no differentials, no attribute gradient', s, 5, attr_grad=False, ids='runs')
    c('gen/A32/all/attr', 'FPCDR_MAX_ATTR channels, all with differentials: DiffIdx is full', s, 32, diff='all')
    c('gen/A32/all', 'the same without an attribute gradient', s, 32, diff='all', attr_grad=False, ids='runs')
    c('gen/A33/[32,0]/attr', 'more channels than FPCDR_MAX_ATTR, a differential of the last one', s, 33, diff=[32, 0], ids='runs')
    c('gen/A33/[32,0]/BaB', 'the same with a table per image, no attribute gradient', s, 33, diff=[32, 0], BaB=True, attr_grad=False)
    s = S_BIN2
    c('bin44/A2/confetti', 'H % 32 = 12: py0 inside the image, some of its + 8 k rows outside', s, 2, attr_grad=False)
    c('bin44/A2/one/attr', 'bin-shaped forward, tiled backward, one triangle', s, 2, ids='one')
    c('gen44/A2+8B', 'the generic twins at this shape', s, 2, attr_grad=False, misalign=True)
    c('gen44/A3/all/attr', 'three channels with differentials', s, 3, diff='all', ids='runs')
    c('gen44/A5/[2,0]', 'five channels, two differentials, no attribute gradient', s, 5, diff=[2, 0], attr_grad=False)
    s = S_STREAM
    c('stream/A2', 'W % 4 != 0: A = 2 without differentials takes the generic kernels; a second x-block of 3 pixels', s, 2, attr_grad=False)
    c('stream/A2/attr', 'the same with the scatter: 17 tiles of 16 across', s, 2, ids='runs')
    c('stream/A3/[2,0,2]/BaB', 'a repeated index across two x-blocks, a table per image', s, 3, diff=[2, 0, 2], BaB=True, attr_grad=False)
    c('stream/A1/all/attr', 'one channel with its differential', s, 1, diff='all', ids='one')
    c('stream/A32/all', 'FPCDR_MAX_ATTR channels across two x-blocks', s, 32, diff='all', attr_grad=False, ids='runs')
    c('stream/A2/all', 'the float4 store of k_interp_fwd<2> at a width that is no multiple of 4', s, 2, diff='all', attr_grad=False, ids='runs')
    s = S_HINT
    c('hint/bin/A2', 'both bin-shaped kernels with a hint', s, 2, attr_grad=False, hint=True)
    c('hint/bin/A2/attr', 'k_interp_fwd_bin2 and k_interp_bwd<true> with a hint', s, 2, ids='runs', hint=True)
    c('hint/gen/A2+8B', 'k_interp_fwd<2> and k_interp_bwd_rows with a hint', s, 2, attr_grad=False, misalign=True, hint=True)
    c('hint/gen/A3/[2,0,2]/attr', 'k_interp_fwd<0> and k_interp_bwd<true> with a hint', s, 3, diff=[2, 0, 2], hint=True)
    c('hint/gen/A3/all', 'k_interp_fwd<0> and k_interp_bwd_rows with a hint', s, 3, diff='all', attr_grad=False, ids='runs', hint=True)
    c('hint/gen/A2/all/attr', 'k_interp_fwd<2> with differentials and a hint', s, 2, diff='all', ids='one', hint=True)
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]

# what tri holds besides random triangles (indices of vertices / triangles)
V_SHARED, V_REPEATED, V_DEAD, V_UNUSED = 5, 7, 98, 99
T_SHARED, T_REPEATED, T_DEAD, T_ONE, T_EXACT = (0, 1, 2), 3, 4, 10, 20


def make_tri(gen):
    """[T,3] int32 over the vertices 0..97 but for: V_SHARED is corner 0 of triangle 0, corner 1 of triangle 1 and corner 2 of
    triangle 2; triangle 3 names V_REPEATED twice; V_DEAD belongs to triangle T_DEAD alone, whose pixels get no gradient; no triangle
    names V_UNUSED."""
    tri = torch.randint(0, V_DEAD, (T, 3), generator=gen)
    tri[0, 0] = tri[1, 1] = tri[2, 2] = V_SHARED
    tri[T_REPEATED] = torch.tensor([V_REPEATED, V_REPEATED, 9])
    tri[T_DEAD, 0] = V_DEAD
    return tri.to(torch.int32)


def _randn_away(shape, gen):
    """randn with every magnitude raised by 0.1: no entry near 0, none denormal."""
    x = torch.randn(shape, generator=gen, dtype=torch.float64)
    return (torch.where(x < 0, x - 0.1, x + 0.1)).float()


def _ids(kind, B, H, W, gen):
    if kind == 'confetti':
        return torch.randint(1, T + 1, (B, H, W), generator=gen)
    if kind == 'one':
        return torch.full((B, H, W), T_ONE + 1)
    ids = torch.zeros(B, H, W, dtype=torch.int64)       # runs of 3 to 20 pixels along a row
    for b in range(B):
        for y in range(H):
            x = 0
            while x < W:
                n = int(torch.randint(3, 21, (1,), generator=gen))
                ids[b, y, x:x + n] = int(torch.randint(1, T + 1, (1,), generator=gen))
                x += n
    return ids


def case_inputs(case):
    """The float32 inputs of a case: dict with attr, rast, tri, rast_db (None without differentials), diff_list, go, go_da (None),
    exact: the pixels (b, y, x, corner) whose out must equal attribute a_corner bit for bit, hint (hinted cases: uint8 CPU)."""
    c = case
    gen = torch.Generator().manual_seed(2000 + c['seed'] + sum(ord(ch) for ch in c['name']))
    B, H, W = c['img']
    A = c['A']
    lay = LAYOUT[c['img']]
    diff_list = diff_indices(c['diff'], A)
    nd = len(diff_list)
    tri = make_tri(gen)
    attr = _randn_away((B if c['BaB'] else 1, VT, A), gen)
    ids = _ids(c['ids'], B, H, W, gen)
    ids[torch.rand(B, H, W, generator=gen) < 0.1] = 0                    # uncovered pixels inside occupied bins
    uvz = torch.rand(B, H, W, 3, generator=gen, dtype=torch.float64) * 2.0 - 0.5     # full float32 mantissas in [-0.5, 1.5)
    binmask = lambda b, by, bx: (b, slice(by * BIN, min((by + 1) * BIN, H)), slice(bx * BIN, min((bx + 1) * BIN, W)))
    free = torch.ones(B, H, W, dtype=torch.bool)
    for bn in lay['empty'] + lay['sparse']:
        ids[binmask(*bn)] = 0
        uvz[binmask(*bn)] = 0.0
        free[binmask(*bn)] = False
    for b, by, bx in lay['sparse']:         # five covered pixels, on a diagonal
        for k in range(5):
            y, x = min(by * BIN + 1 + 2 * k, H - 1), min(bx * BIN + 2 + k, W - 1)
            ids[b, y, x] = 1 + (7 * k) % T
            uvz[b, y, x] = torch.tensor([0.25, 0.5, 0.1], dtype=torch.float64) + 0.01 * k
    # the deliberate pixels, scattered over the occupied bins: the shared, the repeated and the dead vertex's triangles, the last
    # valid id T and the ids the clamp rejects, three pixels each; then nine pixels at the corners of their triangles
    spots = torch.nonzero(free.reshape(-1), as_tuple=True)[0]
    spots = spots[torch.randperm(spots.numel(), generator=gen)]
    flat_ids, flat_uvz = ids.reshape(-1), uvz.reshape(-1, 3)
    k = 0
    for val in [t + 1 for t in T_SHARED] + [T_REPEATED + 1, T_DEAD + 1, T, T + 1, T + 7, 0]:
        flat_ids[spots[k:k + 3]] = val
        k += 3
    exact = []
    for corner, (eu, ev) in enumerate(((1.0, 0.0), (0.0, 1.0), (0.0, 0.0))):
        for p in spots[k:k + 3].tolist():
            flat_ids[p] = T_EXACT + 1 + corner
            flat_uvz[p, 0], flat_uvz[p, 1] = eu, ev
            exact.append((p // (H * W), (p // W) % H, p % W, corner))
        k += 3
    rast = torch.cat([uvz.float(), ids[..., None].float()], -1)
    rast[..., :3][(ids == 0) & ~free] = 0.0
    go = _randn_away((B, H, W, A), gen)
    go_da = _randn_away((B, H, W, 2 * nd), gen) if nd else None
    dead = ids == T_DEAD + 1
    go[dead] = 0.0
    if nd:
        go_da[dead] = 0.0
    res = dict(attr=attr, rast=rast, tri=tri, rast_db=_randn_away((B, H, W, 4), gen) if nd else None, diff_list=diff_list, go=go,
               go_da=go_da, exact=exact, hint=None)
    if c['hint']:
        res['hint'] = make_hint(rast, lay['extra_on'])
    return res


def reference(inp, dtype=torch.float64, order=None, rast=None):
    return interpolate(inp['attr'], inp['rast'] if rast is None else rast, inp['tri'], inp['rast_db'], inp['diff_list'], inp['go'],
                       inp['go_da'], dtype=dtype, order=order)


def kernel_order(inp, rast=None):
    return float32_in_kernel_order(inp['attr'], inp['rast'] if rast is None else rast, inp['tri'], inp['rast_db'], inp['diff_list'],
                                   inp['go'], inp['go_da'])


def bounds(A, n_diff):
    """name -> n of the short paths (the bound is n + 2); g_attr follows the long-sum rule e <= 8 * e32 + 4."""
    return {'out': N_OUT, 'out_da': N_OUT_DA, 'g_rast': N_G_RAST(A), 'g_rast_db': N_G_RAST_DB(n_diff)}


def predicted_zeros(attr, rast, tri, diff_list, go):
    """name -> the number of entries without any term, counted on the pattern of ids and of zeroed gradients, never on values:
    out, out_da: the uncovered pixels; g_rast: .z and .w everywhere, .x and .y where the pixel is uncovered or has no gradient;
    g_rast_db: the same pixels, all four; g_attr: every channel of the vertices no covered pixel with a gradient shows."""
    B, H, W, _ = rast.shape
    Ba, Vt, A = attr.shape
    nT = tri.shape[0]
    nd = len(diff_list)
    tid = rast.detach().cpu().reshape(-1, 4)[:, 3].to(torch.int64) - 1
    cov = (tid >= 0) & (tid < nT)
    live = cov & (go.detach().cpu().reshape(B * H * W, A) != 0).any(1)
    P = B * H * W
    z = {'out': A * int((~cov).sum()), 'g_rast': 2 * P + 2 * int((~live).sum())}
    if nd:
        z['out_da'] = 2 * nd * int((~cov).sum())
        z['g_rast_db'] = 4 * int((~live).sum())
    m = torch.nonzero(live, as_tuple=True)[0]
    rows = tri.detach().cpu().long()[tid[m]] + ((m // (H * W)) * Vt if Ba > 1 else torch.zeros_like(m))[:, None]
    # corner 0 has the term u g_k unless u is exactly 0 (a deliberate pixel), corner 1 likewise with v, corner 2 always
    # (w is a sum with the term 1); a channel that carries a differential has its term at corners 0 and 1 whatever u and v are
    r = rast.detach().cpu().reshape(-1, 4)[m]
    in_diff = torch.zeros(A, dtype=torch.bool)
    in_diff[list(diff_list)] = True
    shown = torch.zeros(Ba * Vt, A, dtype=torch.int64)
    for corner, coeff in enumerate((r[:, 0] != 0, r[:, 1] != 0, torch.ones(m.numel(), dtype=torch.bool))):
        shown.index_add_(0, rows[:, corner], (coeff[:, None] | in_diff[None]).long())
    z['g_attr'] = int((shown == 0).sum())
    return z

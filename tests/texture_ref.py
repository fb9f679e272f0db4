"""float64 restatement on the CPU of the texture operator (csrc/texture.hip, csrc/texsample.h), forward and backward, without
autograd: the yardstick of tests/test_gpu_texture.py, itself checked on the CPU by tests/test_texture_ref.py.  Nothing here imports
fpc_diffrend_amd or oracle.

texture() takes float32 inputs and evaluates in `dtype` (float64 by default; float32 gives "the same formula in float32 by torch",
the yardstick of the long sums).  For every output it returns (value, S); an error is measured per entry in units of u = 2^-24
against S (fitstep_ref.measure): one lost tap of one pixel shows at its own size, however many entries the tensor has.

The scale S is COORDINATE-AWARE.  The fractions fx, fy come from x = prep(u) * Wt - 0.5, whose absolute rounding error grows with
X_s = Wt * (|u| + |floor u|) + 0.5, the sum of the absolute values of the terms of x, and reaches an entry through its
sensitivity to fx.  So every S here is
    the entry's formula with every texel / gradient replaced by its absolute value and every subtraction by an addition
  + for each computed coordinate (fx, fy, and for the mip filters the level), the coordinate's scale times G, the entry's
    |d / d coordinate| written the same way.
A scale built from the taps alone (sum_k |w_k| |t_k|) is wrong by the factor by which the coordinate error dominates:
test_texture_ref.py measures, for float32 torch on (2, 37, 40), 'wrap', uv in [-2, 3) with full float32 mantissas, 100 u against
the plain scale and 0.28 u against the coordinate-aware one on a 32 x 64 texture, 150 u against 0.53 u on a 30 x 60 one (printed by
test_coordinate_aware_scale_is_the_right_one).  At a power-of-two size the product and the - 0.5 are exact and the error is that
of u - floor(u) for a small negative u; at any other size the product rounds as well.

The level of the mip filters, level = 0.5 log2(l2) + bias, l2 = tr + rt, has the scale
    L_s = |0.5 log2 l2| + |bias| + 0.5 / ln 2 * (tr + rt_s) / l2,    rt_s = (df_a^2 + bq_a^2) / rt,
df_a, bq_a being df and bq with their subtractions added (rt_s / rt is the factor by which a cancellation in rt would amplify); it
is 0 where the level is clamped (the clamp is exact).  It reaches `out` through |c0| + |c1|.  A built chain adds its own
roundings: three adds per level (the * 0.25 is exact); the scale of a level's texel is the box average of |tex|.

The module also holds the inputs of every GPU case (CASES, case_inputs), so that the CPU file measures the float32 evaluation, the
margins and the mutants on the very inputs the GPU file hands to the kernels, and a restatement in integers of how
k_tex_bwd_bin1 shapes its LDS window (window_plan), by which both files show that a case reaches the branch it exists for."""
import math

import numpy as np
import torch

from fitstep_ref import U, measure, rel_l2      # noqa: F401  (re-exported: the conventions of the fit step's yardstick)

# Rounded operations that reach one entry, n (rules of fitstep_ref.py: an input has n = 0; a product n_a + n_b + 1; a sum of k terms
# max n_i + k - 1; a product with a power of two is exact; a square root halves the relative error and adds 1).  The entry's error
# is then at most (n + 2) u of S.  CHAIN = 3 per level of a built chain (three adds) is added by the tests where a chain is built.
# x = prep(u) * Wt - 0.5: the wrap subtraction 1, the product 2, the subtraction 3; fx = x - floor(x): its rounding is at most
#            u |fx| <= 2 u X_s (X_s >= 0.5): 5, in units of X_s.  N_COORD = 5 never exceeds the counts below, which hold for the sum.
N_COORD = 5
# out, nearest: a copy.
N_OUT_NEAREST = 0
# out, linear: t10 - t00 1, * fx 2, + t00 3 (top, bot); bot - top 4, * fy 5, + top 6.
N_OUT_LINEAR = 6
# level: dudx = d * Wt 1, its square 3, A = the sum of two 4, tr and df 5, df^2 11, bq (4) squared 9, the sum of three 13, the root 8,
#            l2 = tr + rt 9, log2 10, + bias 11; fl = level - l0: 12, in units of L_s.
N_LEVEL = 12
# out, linear-mipmap-linear: c0, c1 6, c1 - c0 7, * fl 8, + c0 9; the level's own 12 rules.   linear-mipmap-nearest: 6.
N_OUT_MIP_LINEAR = 12
N_OUT_MIP_NEAREST = 6
# g_uv, linear: t10 - t00 1, 1 - fy 1, their product 3, the sum of two such 4, * g_c 5, the sum over C channels 4 + C, * Wt 5 + C.
N_GUV_LINEAR = lambda C: 5 + C
# g_uv, mip: g_c * (1 - fl) 2, * the bracket (4) 7, over C 6 + C, * w_l 7 + C, the sum of the two levels 8 + C.
N_GUV_MIP = lambda C: 8 + C
# g_bias: c1 - c0 7, * g_c 8, over C channels 7 + C.
N_GBIAS = lambda C: 7 + C
# box filter: three adds, * 0.25 exact.  Its backward alone: 0.25 * g added to a zero: exact.
N_MIP_DOWN = 3
N_MIP_DOWN_BWD = 0
CHAIN = 3

MUTANT = None       # set by test_texture_ref.py only: a deliberately wrong restatement (see there)

TWC = 2048          # cells of k_tex_bwd_bin1's window


def _c(t, dtype):
    return t.detach().to('cpu', dtype)


def _prep(u, boundary):
    """The prepared coordinate and the sum of the absolute values of its terms."""
    if boundary == 'wrap':
        f = torch.floor(u)
        return u - f, u.abs() + f.abs()
    if boundary == 'clamp':
        p = u.clamp(0.0, 1.0)
        return p, p.abs()
    return u, u.abs()


def _idx(i, n, boundary):
    if boundary == 'wrap':
        return torch.remainder(i, n)
    return i.clamp(0, n - 1)


def _inside(i, n, boundary):
    if boundary != 'zero':
        return torch.ones_like(i, dtype=torch.bool)
    return (i >= 0) & (i < n)


class _Sample:
    """One bilinear lookup of P pixels in one level t [N,h,w,C] (tA: the texels' scales): values, scales and what the backward
    needs.  Taps k = 0..3 are (00, 10, 01, 11)."""

    def __init__(self, t, tA, tb, u, v, boundary):
        N, h, w, C = t.shape
        self.shape, self.w, self.h = t.shape, w, h
        pu, Us = _prep(u, boundary)
        pv, Vs = _prep(v, boundary)
        x, y = pu * w - 0.5, pv * h - 0.5
        self.Xs, self.Ys = (Us * w + 0.5)[:, None], (Vs * h + 0.5)[:, None]     # sums of the absolute values of the terms of x, y
        x0f, y0f = torch.floor(x), torch.floor(y)
        fx, fy = (x - x0f)[:, None], (y - y0f)[:, None]
        if MUTANT == 'swap_fx_fy':
            fx, fy = fy, fx
        self.fx, self.fy, self.x, self.y = fx, fy, x, y
        x0, y0 = x0f.long(), y0f.long()
        self.x0, self.y0 = x0, y0
        ix = (_idx(x0, w, boundary), _idx(x0 + 1, w, boundary))
        if MUTANT == 'no_seam_wrap' and boundary == 'wrap':
            ix = (ix[0], (x0 + 1).clamp(0, w - 1))
        iy = (_idx(y0, h, boundary), _idx(y0 + 1, h, boundary))
        vx = (_inside(x0, w, boundary), _inside(x0 + 1, w, boundary))
        vy = (_inside(y0, h, boundary), _inside(y0 + 1, h, boundary))
        self.flat, self.valid, tv, ta = [], [], [], []
        for k in range(4):
            jx, jy = k & 1, k >> 1
            ok = vx[jx] & vy[jy]
            self.flat.append((tb * h + iy[jy]) * w + ix[jx])
            self.valid.append(ok)
            m = ok[:, None].to(t.dtype)
            tv.append(t[tb, iy[jy], ix[jx]] * m)
            ta.append(tA[tb, iy[jy], ix[jx]] * m)
        t00, t10, t01, t11 = tv
        a00, a10, a01, a11 = ta
        top, bot = t00 + (t10 - t00) * fx, t01 + (t11 - t01) * fx
        topA, botA = a00 + (a10 + a00) * fx, a01 + (a11 + a01) * fx
        self.c = top + (bot - top) * fy                                            # [P,C]
        self.dfx = (t10 - t00) * (1.0 - fy) + (t11 - t01) * fy                     # d c / d fx
        self.dfy = bot - top                                                      # d c / d fy
        self.dfxA = (a10 + a00) * (1.0 - fy) + (a11 + a01) * fy
        self.dfyA = botA + topA
        self.T4 = a00 + a10 + a01 + a11                                            # |d dfx / d fy| = |d dfy / d fx|, written with additions
        self.cS = topA + (botA + topA) * fy + self.Xs * self.dfxA + self.Ys * self.dfyA
        self.wk = [(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy]
        dwx, dwy = [1.0 - fy, 1.0 - fy, fy, fy], [1.0 - fx, fx, 1.0 - fx, fx]      # |d w_k / d fx|, |d w_k / d fy|
        self.wkS = [self.wk[k] + self.Xs * dwx[k] + self.Ys * dwy[k] for k in range(4)]
        self.any_valid = self.valid[0] | self.valid[1] | self.valid[2] | self.valid[3]

    def scatter(self, G, GS, T, rows, g, scale, Ls):
        """Add g [P,C] * scale [P,1] * w_k into G (flat [N*h*w, C]) at the taps that exist; GS the scale; T the number of terms."""
        ga = g.abs()
        live = (g != 0) & (scale != 0)
        for k in range(4):
            ok = self.valid[k]
            if MUTANT == 'zero_tap_scatters':
                ok = torch.ones_like(ok)
            m = ok[:, None].to(g.dtype)
            G.index_add_(0, self.flat[k][rows], (g * scale * self.wk[k] * m))
            GS.index_add_(0, self.flat[k][rows], ga * (scale * self.wkS[k] + Ls * self.wk[k]) * m)
            T.index_add_(0, self.flat[k][rows], (live & ok[:, None]).to(torch.int64))


def box_chain(tex, n_levels, dtype=torch.float64):
    """The 2 x 2 box chain of tex [N,Ht,Wt,C], levels 0..n_levels, and the chain of the texels' scales (the box average of |tex|)."""
    box = lambda t: (t[:, 0::2, 0::2] + t[:, 0::2, 1::2] + t[:, 1::2, 0::2] + t[:, 1::2, 1::2]) * 0.25
    chain, chainA = [_c(tex, dtype)], [_c(tex, dtype).abs()]
    for _ in range(n_levels):
        chain.append(box(chain[-1]))
        chainA.append(box(chainA[-1]))
    return chain, chainA


def num_levels(Ht, Wt, max_mip_level=None):
    """Levels below the base of a built chain: it stops when a side would become odd or zero."""
    n = 0
    while (max_mip_level is None or n < max_mip_level) and Ht % 2 == 0 and Wt % 2 == 0 and Ht >= 2 and Wt >= 2:
        Ht, Wt, n = Ht // 2, Wt // 2, n + 1
    return n


def _up(g):
    """The box filter's backward: every coarse entry's quarter to its four fine texels."""
    return 0.25 * g.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def mip_down(src, go=None, dtype=torch.float64):
    """One level of the box chain on its own and its backward -> dict name -> (value, S)."""
    (s, d), (sa, da) = box_chain(src, 1, dtype)
    res = {'out': (d, da)}
    if go is not None:
        g = _c(go, dtype)
        res['g_src'] = (_up(g), _up(g.abs()))
    return res


def level_of_detail(uv_da, bias, Ht, Wt, P, dtype=torch.float64):
    """The raw level [P], its scale L_s and the pieces of its backward."""
    L = {}
    if uv_da is not None:
        d = _c(uv_da, dtype).reshape(-1, 4)
        dudx, dudy, dvdx, dvdy = d[:, 0] * Wt, d[:, 1] * Wt, d[:, 2] * Ht, d[:, 3] * Ht
        A, Bq, Cc = dudx * dudx + dudy * dudy, dudx * dvdx + dudy * dvdy, dvdx * dvdx + dvdy * dvdy
        BqA = (dudx * dvdx).abs() + (dudy * dvdy).abs()
        tr, df = 0.5 * (A + Cc), 0.5 * (A - Cc)
        rt = torch.sqrt(df * df + Bq * Bq + 1e-30)
        rtS = (tr * tr + BqA * BqA + 1e-30) / rt             # df with its subtraction added is tr
        l2 = tr + rt
        raw = 0.5 * torch.log2(l2.clamp(min=1e-30))
        Ls = raw.abs() + (0.5 / math.log(2.0)) * (tr + rtS) / l2
        L.update(d=(dudx, dudy, dvdx, dvdy), df=df, bq=Bq, BqA=BqA, tr=tr, rt=rt, rtS=rtS, l2=l2)
    else:
        raw = torch.zeros(P, dtype=dtype)
        Ls = torch.zeros(P, dtype=dtype)
    if bias is not None:
        b = _c(bias, dtype).reshape(-1)
        raw = raw + b
        Ls = Ls + b.abs()
    L['raw'], L['Ls'] = raw, Ls
    return L


def texture(tex, uv, uv_da=None, bias=None, mips=None, go=None, filter_mode='linear', boundary='wrap', max_mip_level=None,
            dtype=torch.float64):
    """tex [1|B,Ht,Wt,C], uv [B,H,W,2], uv_da [B,H,W,4], bias [B,H,W]; mips: a custom stack (levels 1..n, each keeps its own
    gradient) or None (the chain is built from tex and its gradient collapses into tex); go = d loss / d out.
    -> dict name -> (value, S): 'out', and with go 'g_tex' (and 'g_mip1', ... for a custom stack), 'g_uv', 'g_uv_da', 'g_bias' as far
    as the mode has them; 'terms': name -> the number of terms of every entry of g_tex / g_mip*, counted on the pattern of the taps."""
    B, H, W, _ = uv.shape
    Bt, Ht, Wt, C = tex.shape
    P = B * H * W
    q = _c(uv, dtype).reshape(-1, 2)
    u, v = q[:, 0], q[:, 1]
    tb = torch.arange(B).repeat_interleave(H * W) if Bt > 1 else torch.zeros(P, dtype=torch.long)
    g = _c(go, dtype).reshape(P, C) if go is not None else None
    zero = torch.zeros((), dtype=dtype)
    res, terms = {}, {}
    if boundary == 'clamp' and MUTANT != 'no_clamp_mask':      # inclusive at 0 and 1, as torch.clamp's gradient
        mu = ((u >= 0) & (u <= 1)).to(dtype)
        mv = ((v >= 0) & (v <= 1)).to(dtype)
    else:
        mu = mv = torch.ones(P, dtype=dtype)
    t0 = _c(tex, dtype)

    if filter_mode == 'nearest':
        pu, _ = _prep(u, boundary)
        pv, _ = _prep(v, boundary)
        rx, ry = torch.floor(pu * Wt - 0.5 + 0.5).long(), torch.floor(pv * Ht - 0.5 + 0.5).long()
        ok = (_inside(rx, Wt, boundary) & _inside(ry, Ht, boundary))
        ix, iy = _idx(rx, Wt, boundary), _idx(ry, Ht, boundary)
        val = t0[tb, iy, ix] * ok[:, None].to(dtype)
        res['out'] = (val.reshape(B, H, W, C), val.abs().reshape(B, H, W, C))
        res['pad_all'] = ~ok
        if g is not None:
            flat = (tb * Ht + iy) * Wt + ix
            m = ok[:, None].to(dtype)
            G, GS, T = (torch.zeros(Bt * Ht * Wt, C, dtype=d) for d in (dtype, dtype, torch.int64))
            G.index_add_(0, flat, g * m)
            GS.index_add_(0, flat, g.abs() * m)
            T.index_add_(0, flat, ((g != 0) & ok[:, None]).to(torch.int64))
            res['g_tex'] = (G.reshape(tex.shape), GS.reshape(tex.shape))
            terms['g_tex'] = T.reshape(tex.shape)
            res['g_uv'] = (torch.zeros(B, H, W, 2, dtype=dtype), torch.zeros(B, H, W, 2, dtype=dtype))
        res['terms'] = terms
        return res

    if filter_mode == 'linear':
        s = _Sample(t0, t0.abs(), tb, u, v, boundary)
        res['out'] = (s.c.reshape(B, H, W, C), s.cS.reshape(B, H, W, C))
        res['pad_all'] = ~s.any_valid
        if g is not None:
            G, GS, T = (torch.zeros(Bt * Ht * Wt, C, dtype=d) for d in (dtype, dtype, torch.int64))
            one = torch.ones(P, 1, dtype=dtype)
            s.scatter(G, GS, T, slice(None), g, one, torch.zeros(P, 1, dtype=dtype))
            res['g_tex'] = (G.reshape(tex.shape), GS.reshape(tex.shape))
            terms['g_tex'] = T.reshape(tex.shape)
            ga = g.abs()
            gu, gv = (g * s.dfx).sum(1) * Wt * mu, (g * s.dfy).sum(1) * Ht * mv
            guS, gvS = (ga * (s.dfxA + s.Ys * s.T4)).sum(1) * Wt * mu, (ga * (s.dfyA + s.Xs * s.T4)).sum(1) * Ht * mv
            res['g_uv'] = (torch.stack([gu, gv], 1).reshape(B, H, W, 2), torch.stack([guS, gvS], 1).reshape(B, H, W, 2))
        res['terms'] = terms
        return res

    assert filter_mode in ('linear-mipmap-nearest', 'linear-mipmap-linear'), filter_mode
    trilinear = filter_mode == 'linear-mipmap-linear'
    custom = mips is not None
    if custom:
        ms = list(mips) if max_mip_level is None else list(mips)[:int(max_mip_level)]
        chain = [t0] + [_c(m, dtype) for m in ms]
        chainA = [t.abs() for t in chain]
    else:
        chain, chainA = box_chain(tex, num_levels(Ht, Wt, max_mip_level), dtype)
    nlev = len(chain) - 1
    L = level_of_detail(uv_da, bias, Ht, Wt, P, dtype)
    raw = L['raw']
    passes = (raw >= 0) & (raw <= nlev)                            # the clamp passes gradient only inside [0, n_levels]
    level = raw.clamp(0.0, float(nlev))
    Ls = torch.where(passes, L['Ls'], zero)[:, None]               # a clamped level is exact
    if trilinear:
        l0 = torch.floor(level).long().clamp(max=nlev)
        fl = (level - l0.to(dtype))[:, None]
    else:
        l0 = torch.floor(level + 0.5).long().clamp(max=nlev)
        fl = torch.zeros(P, 1, dtype=dtype)
        Ls = torch.zeros(P, 1, dtype=dtype)                        # the level only selects
    res['l0'], res['raw'], res['passes'], res['n_levels'] = l0, raw, passes, nlev
    res['pad_all'] = torch.zeros(P, dtype=torch.bool)
    out, outS = torch.zeros(P, C, dtype=dtype), torch.zeros(P, C, dtype=dtype)
    acc = [[torch.zeros(t.shape[0] * t.shape[1] * t.shape[2], C, dtype=d) for d in (dtype, dtype, torch.int64)] for t in chain]
    gu, gv, guS, gvS = (torch.zeros(P, dtype=dtype) for _ in range(4))
    gl, glS = torch.zeros(P, dtype=dtype), torch.zeros(P, dtype=dtype)
    for l in range(nlev + 1):
        m = torch.nonzero(l0 == l, as_tuple=True)[0]
        if not m.numel():
            continue
        lu = min(l + 1, nlev)
        s0 = _Sample(chain[l], chainA[l], tb[m], u[m], v[m], boundary)
        s1 = _Sample(chain[lu], chainA[lu], tb[m], u[m], v[m], boundary) if trilinear else None
        f, ls = fl[m], Ls[m]
        # (a clamped level has fl = 0 exactly: the upper level then contributes no term)
        res['pad_all'][m] = ~(s0.any_valid | (s1.any_valid & (f[:, 0] != 0))) if trilinear else ~s0.any_valid
        if trilinear:
            out[m] = s0.c + (s1.c - s0.c) * f
            outS[m] = s0.cS + (s1.cS + s0.cS) * f + ls * (s0.c.abs() + s1.c.abs())
        else:
            out[m], outS[m] = s0.c, s0.cS
        if g is None:
            continue
        gm, ga = g[m], g[m].abs()
        every = slice(None)
        s0.scatter(*acc[l], every, gm, 1.0 - f, ls)
        w0, h0 = s0.w, s0.h
        gu[m] = (gm * (1.0 - f) * s0.dfx).sum(1) * w0
        gv[m] = (gm * (1.0 - f) * s0.dfy).sum(1) * h0
        guS[m] = (ga * ((1.0 - f) * (s0.dfxA + s0.Ys * s0.T4) + ls * s0.dfxA)).sum(1) * w0
        gvS[m] = (ga * ((1.0 - f) * (s0.dfyA + s0.Xs * s0.T4) + ls * s0.dfyA)).sum(1) * h0
        if trilinear:
            s1.scatter(*acc[lu], every, gm, f, ls)
            w1, h1 = (Wt, Ht) if (MUTANT == 'level1_scale' and lu >= 1) else (s1.w, s1.h)
            gu[m] += (gm * f * s1.dfx).sum(1) * w1
            gv[m] += (gm * f * s1.dfy).sum(1) * h1
            guS[m] += (ga * (f * (s1.dfxA + s1.Ys * s1.T4) + ls * s1.dfxA)).sum(1) * s1.w
            gvS[m] += (ga * (f * (s1.dfyA + s1.Xs * s1.T4) + ls * s1.dfyA)).sum(1) * s1.h
            gl[m] = (gm * (s1.c - s0.c)).sum(1)
            glS[m] = (ga * (s1.cS + s0.cS)).sum(1)
    res['out'] = (out.reshape(B, H, W, C), outS.reshape(B, H, W, C))
    res['terms'] = terms
    if g is None:
        return res
    res['g_uv'] = (torch.stack([gu * mu, gv * mv], 1).reshape(B, H, W, 2), torch.stack([guS * mu, gvS * mv], 1).reshape(B, H, W, 2))
    shaped = [[a.reshape(t.shape) for a in ac] for ac, t in zip(acc, chain)]
    if custom:
        for l, (G, GS, T) in enumerate(shaped):
            name = 'g_tex' if l == 0 else f'g_mip{l}'
            res[name], terms[name] = (G, GS), T
    else:       # the built chain: the levels' gradients collapse into tex, coarse to fine
        for l in range(nlev, 0, -1):
            shaped[l - 1][0] = shaped[l - 1][0] + _up(shaped[l][0])
            shaped[l - 1][1] = shaped[l - 1][1] + _up(shaped[l][1])
            shaped[l - 1][2] = shaped[l - 1][2] + shaped[l][2].repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        res['g_tex'], terms['g_tex'] = (shaped[0][0], shaped[0][1]), shaped[0][2]
    glevel = torch.where(passes, gl, zero) if trilinear else torch.zeros(P, dtype=dtype)
    glevelS = torch.where(passes, glS, zero) if trilinear else torch.zeros(P, dtype=dtype)
    if bias is not None:
        res['g_bias'] = (glevel.reshape(B, H, W), glevelS.reshape(B, H, W))
    if uv_da is not None:
        dudx, dudy, dvdx, dvdy = L['d']
        l2, rt = L['l2'], L['rt']
        ln2 = 0.6931471805599453
        both = []
        for scale in (False, True):
            s = 1.0 if scale else -1.0
            f = (lambda t: t.abs()) if scale else (lambda t: t)
            gg = glevelS if scale else glevel
            gl2 = torch.where(l2 >= 1e-30, gg * 0.5 / (l2 * ln2), zero)
            gdf = gl2 * (L['tr'] if scale else L['df']) / rt
            gbq = gl2 * (L['BqA'] if scale else L['bq']) / rt
            gA, gC = 0.5 * gl2 + 0.5 * gdf, 0.5 * gl2 + s * 0.5 * gdf
            rows = [(2.0 * f(dudx) * gA + f(dvdx) * gbq) * Wt, (2.0 * f(dudy) * gA + f(dvdy) * gbq) * Wt,
                    (2.0 * f(dvdx) * gC + f(dudx) * gbq) * Ht, (2.0 * f(dvdy) * gC + f(dudy) * gbq) * Ht]
            both.append(torch.stack(rows, 1))
        # the divisors l2 and rt are computed too: their relative errors are those of (tr + rt_s) / l2 and rt_s / rt
        amp = ((L['tr'] + L['rtS']) / l2 + L['rtS'] / rt - 1.0)[:, None]
        res['g_uv_da'] = (both[0].reshape(B, H, W, 4), (both[1] * amp).reshape(B, H, W, 4))
    return res


def plain_scale_out(tex, uv, boundary='wrap', dtype=torch.float64):
    """sum_k |w_k| |t_k| of a 'linear' lookup: the scale that leaves the coordinates out (only to show that it is wrong)."""
    B, H, W, _ = uv.shape
    q = _c(uv, dtype).reshape(-1, 2)
    tb = torch.arange(B).repeat_interleave(H * W) if tex.shape[0] > 1 else torch.zeros(B * H * W, dtype=torch.long)
    t0 = _c(tex, dtype)
    s = _Sample(t0, t0.abs(), tb, q[:, 0], q[:, 1], boundary)
    return (s.cS - s.Xs * s.dfxA - s.Ys * s.dfyA).reshape(B, H, W, -1)


# ---------------------------------------------------------------------------------------------------------------------
# what the construction predicts to be exactly 0 (counted on patterns, never on the values)
# ---------------------------------------------------------------------------------------------------------------------

def tap_patterns(case, inp):
    """The set of 4-bit masks (bit k: tap k lies inside the texture) the level-0 taps of a case's pixels show."""
    q = inp['uv'].double().reshape(-1, 2)
    t0 = inp['tex'].double()
    s = _Sample(t0, t0.abs(), torch.zeros(q.shape[0], dtype=torch.long), q[:, 0], q[:, 1], case['bd'])
    return set((sum(s.valid[k].long() << k for k in range(4))).tolist())


def predicted_zeros(uv, uv_da, bias, go, filter_mode, boundary, ref):
    """name -> the number of entries without any term.  out: the pixels whose taps all lie in the 'zero' padding.  g_tex / g_mip*: texels no tap of a pixel with a gradient reaches (ref['terms']).
    g_uv: every entry for 'nearest'; else the pixels without a gradient, those whose taps all lie in the 'zero' padding (ref['pad_all'],
    from the taps' index tests), and under 'clamp' the components whose coordinate lies outside [0, 1].  g_bias / g_uv_da: the pixels
    without a gradient or a tap, those whose raw level lies outside [0, n_levels], and every pixel of 'linear-mipmap-nearest'."""
    B, H, W, _ = uv.shape
    z = {k: int((t == 0).sum()) for k, t in ref['terms'].items()}
    z['out'] = int(ref['pad_all'].sum()) * ref['out'][0].shape[-1]          # every tap in the 'zero' padding
    if go is None:
        return z
    if filter_mode == 'nearest':
        z['g_uv'] = 2 * B * H * W
        return z
    none = (go.detach().cpu().reshape(B * H * W, -1) == 0).all(1) | ref['pad_all']
    comp = torch.stack([none, none], 1)
    if boundary == 'clamp':
        q = uv.detach().cpu().reshape(-1, 2)
        comp = comp | ~((q >= 0) & (q <= 1))
    z['g_uv'] = int(comp.sum())
    if filter_mode.startswith('linear-mipmap'):
        nolevel = none | (~ref['passes'] if filter_mode == 'linear-mipmap-linear' else torch.ones_like(none))
        if bias is not None:
            z['g_bias'] = int(nolevel.sum())
        if uv_da is not None:
            z['g_uv_da'] = 4 * int(nolevel.sum())
    return z


# ---------------------------------------------------------------------------------------------------------------------
# how k_tex_bwd_bin1 shapes its window, in integers
# ---------------------------------------------------------------------------------------------------------------------

def window_plan(uv, go, Ht, Wt, boundary):
    """Per 32 x 32 bin of every image, what k_tex_bwd_bin1 does with it: a list of dicts with kind 'exit' (no gradient arrives),
    'none' (only uv == (0,0) pixels: no window), 'fits' (the taps' box fits in TWC cells) or 'centred' (it does not: a window of the
    box's aspect around its centre), stride, rows, the pixels whose taps go into the window / to global atomics / into the
    uv == (0,0) sum, and whether a used window cell lies outside the texture (it is wrapped or clamped at the flush)."""
    B, H, W, _ = uv.shape
    q = uv.detach().cpu().double()
    g = go.detach().cpu().reshape(B, H, W)
    pu, _ = _prep(q[..., 0], boundary)
    pv, _ = _prep(q[..., 1], boundary)
    tx, ty = torch.floor(pu * Wt - 0.5).long(), torch.floor(pv * Ht - 0.5).long()
    origin = (q[..., 0] == 0) & (q[..., 1] == 0)
    plan = []
    for b in range(B):
        for by in range(0, H, 32):
            for bx in range(0, W, 32):
                sl = (b, slice(by, min(by + 32, H)), slice(bx, min(bx + 32, W)))
                live = g[sl] != 0
                e = dict(bin=(b, by // 32, bx // 32), kind='exit', stride=1, rows=1, inside=0, outside=0, origin=0, off_texture=False,
                         pixels=int(live.numel()))
                plan.append(e)
                if not bool(live.any()):
                    continue
                act = live & ~origin[sl]
                e['origin'] = int((live & origin[sl]).sum())
                e['kind'] = 'none'
                if not bool(act.any()):
                    continue
                xs, ys = tx[sl][act], ty[sl][act]
                ox, oy = int(xs.min()), int(ys.min())
                nw, nh = int(xs.max()) - ox + 2, int(ys.max()) - oy + 2
                if nw * nh <= TWC:
                    e['kind'], stride = 'fits', nw
                    rows = TWC // stride
                    oy -= (rows - nh) >> 1
                else:
                    aspect = min(max(float(np.float32(nw) / np.float32(nh)), 1.0 / TWC), float(TWC))
                    e['kind'], stride = 'centred', min(max(int(np.sqrt(np.float32(TWC * aspect))), 2), TWC // 2)
                    rows = TWC // stride
                    ox += (nw - stride) >> 1
                    oy += (nh - rows) >> 1
                lx, ly = xs - ox, ys - oy
                inw = (lx >= 0) & (lx < stride - 1) & (ly >= 0) & (ly < rows - 1)
                e.update(stride=stride, rows=rows, inside=int(inw.sum()), outside=int((~inw).sum()))
                cx, cy = xs[inw], ys[inw]
                e['off_texture'] = bool(((cx < 0) | (cx + 1 >= Wt) | (cy < 0) | (cy + 1 >= Ht)).any())
    return plan


def check_plan(case, plan):
    """The plan of a fast-path case shows the branch the case exists for (case['expect'])."""
    ex = case['expect']
    live = [e for e in plan if e['kind'] not in ('exit', 'none')]
    assert any(e['pixels'] < 1024 for e in plan), "no partial bin"
    if 'kinds' in ex:
        assert {e['kind'] for e in plan} == ex['kinds'], (case['name'], {e['kind'] for e in plan})
    if ex.get('outside') == 0:
        assert all(e['outside'] == 0 for e in plan), case['name']
    if ex.get('some_outside'):
        assert all(e['outside'] > 0 and e['inside'] > 0 for e in live), case['name']
    if 'stride' in ex:
        assert all((e['stride'], e['rows']) == (ex['stride'], ex['rows']) for e in live), case['name']
    if ex.get('off_texture'):
        assert any(e['off_texture'] for e in live), case['name']
    if ex.get('single'):
        assert any(e['inside'] + e['outside'] + e['origin'] == 1 for e in plan), case['name']
    if ex.get('origin'):
        assert any(e['kind'] == 'none' and e['origin'] > 0 for e in plan) and any(e['origin'] > 100 and e['inside'] > 100 for e in live), case['name']
    if 'centred' in ex.get('kinds', ()) and 'fits' in ex['kinds']:      # the seam box that does not fit: every tap of it goes to memory
        assert any(e['kind'] == 'centred' and e['inside'] == 0 for e in plan), case['name']


def takes_fast_path(filter_mode, boundary, C, Bt, W, pointers):
    """The dispatch condition of fpcdr_texture_bwd for k_tex_bwd_bin1 (pointers: uv, dy and grad_uv, or None)."""
    return (filter_mode == 'linear' and C == 1 and Bt == 1 and W % 4 == 0 and boundary != 'zero' and
            all(p is None or p % 16 == 0 for p in pointers))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_texture.py (the CPU file measures float32 torch, the margins and the mutants on the same inputs)
# ---------------------------------------------------------------------------------------------------------------------

def _case(name, why, img=(2, 37, 40), tex=(1, 64, 64, 1), mode='linear', bd='wrap', uv=('affine', 4, 3), go='randn', da=False,
          bias=False, mip='built', mml=None, need=('tex', 'uv'), misalign=False, fwd_only=False, origin=None, expect=None, seed=0):
    return dict(name=name, why=why, img=img, tex=tex, mode=mode, bd=bd, uv=uv, go=go, da=da, bias=bias, mip=mip, mml=mml, need=need,
                misalign=misalign, fwd_only=fwd_only, origin=origin, expect=expect or {}, seed=seed)


def _cases():
    out = []
    for bd in ('wrap', 'clamp'):
        f = lambda name, why, **kw: out.append(_case(f'fast/{name}/{bd}', why, bd=bd, **kw))
        fits = dict(kinds={'fits'}, outside=0)
        f('affine64', 'the box fits; partial bins both ways', expect=fits)
        f('seam32', 'a bin across u = 1 and one across v = 1 whose box fits: cells past the last column at the flush', tex=(1, 32, 32, 1),
          uv=('affine', 20, 12), expect=dict(kinds={'fits'}, outside=0, off_texture=True))
        f('seam128', 'the same map on 128 x 128: under wrap the seam box does not fit', tex=(1, 128, 128, 1), uv=('affine', 110, 100),
          expect=dict(kinds={'fits', 'centred'}) if bd == 'wrap' else dict(kinds={'fits'}))
        f('iid64', 'iid uv: no box fits, centred window and global atomics', uv=('iid', 0.0, 1.0), expect=dict(kinds={'centred'}, some_outside=True))
        f('2x4096', 'aspect clamp: stride 1024, rows 2', tex=(1, 2, 4096, 1), uv=('iid', 0.0, 1.0), expect=dict(kinds={'centred'}, stride=1024, rows=2))
        f('4096x2', 'aspect clamp: stride 2, rows 1024', tex=(1, 4096, 2, 1), uv=('iid', 0.0, 1.0), expect=dict(kinds={'centred'}, stride=2, rows=1024))
        f('1x1', 'one texel: every tap is it', tex=(1, 1, 1, 1), uv=('iid', -1.0, 2.0))
        f('1x8', 'one row', tex=(1, 1, 8, 1), uv=('iid', -1.0, 2.0))
        f('8x1', 'one column', tex=(1, 8, 1, 1), uv=('iid', -1.0, 2.0))
        f('wide', 'uv in [-2, 3): large coordinate terms, masks under clamp', tex=(1, 32, 64, 1), uv=('iid', -2.0, 3.0))
        f('dy_bin_zero', 'no gradient in a whole bin: the early exit', go='bin_zero', expect=dict(kinds={'fits', 'exit'}))
        f('dy_single', 'a gradient at one pixel of a bin: the other lanes of the min-reduction keep the identity', go='single',
          expect=dict(kinds={'fits'}, single=True))
        f('dy_scattered', 'no gradient at scattered pixels', go='scattered', expect=fits)
        f('origin_mixed', 'a bin partly uv == (0,0) with gradient, and a bin that is all (0,0)', origin='mixed',
          expect=dict(kinds={'fits', 'none'}, origin=True))
        f('tex_only', 'only tex requires grad', tex=(1, 32, 32, 1), uv=('affine', 20, 12), need=('tex',))
        f('uv_only', 'only uv requires grad', tex=(1, 32, 32, 1), uv=('affine', 20, 12), need=('uv',))
        f('rows65', 'a third bin row of one row', img=(1, 65, 40), tex=(1, 128, 128, 1), expect=fits)
        g = lambda name, why, **kw: out.append(_case(f'generic/{name}/{bd}', why, bd=bd, **kw))
        g('affine64+8B', 'C = 1 through k_tex_fwd / k_tex_bwd: uv 8 bytes into a buffer', misalign=True)
        g('seam32+8B', 'the same, across the seams', tex=(1, 32, 32, 1), uv=('affine', 20, 12), misalign=True)
        g('iid64+8B', 'the same, iid', uv=('iid', 0.0, 1.0), misalign=True)
    g = lambda name, why, **kw: out.append(_case(f'generic/{name}', why, **kw))
    g('W38', 'W not a multiple of 4', img=(2, 37, 38))
    g('C2', 'two channels', tex=(1, 32, 64, 2), uv=('iid', -2.0, 3.0))
    g('C3', 'three channels, clamp', tex=(1, 32, 64, 3), uv=('iid', -2.0, 3.0), bd='clamp')
    g('C4', 'four channels', tex=(1, 32, 64, 4), uv=('iid', -1.0, 2.0))
    g('Bt2', 'a texture per image', tex=(2, 32, 64, 3), uv=('iid', -1.0, 2.0))
    g('Bt2C1', 'a texture per image, one channel: not the fast pair', tex=(2, 32, 64, 1), uv=('iid', -1.0, 2.0), bd='clamp')
    g('zeroC1', "'zero': uv reaches every side and corner of the padding", tex=(1, 8, 16, 1), uv=('iid', -0.5, 1.5), bd='zero')
    g('zeroC3', "'zero', three channels, a texture per image", tex=(2, 8, 16, 3), uv=('iid', -0.5, 1.5), bd='zero')
    for bd in ('wrap', 'clamp', 'zero'):
        g(f'nearest/{bd}', 'nearest', tex=(2, 8, 16, 3), uv=('iid', -0.5, 1.5), mode='nearest', bd=bd)
    g('fwd260', 'forward only: a second 256-column block, a partial group of 8 rows', img=(1, 9, 260), tex=(1, 32, 64, 2),
      uv=('iid', -1.0, 2.0), fwd_only=True)
    out.append(_case('fast/fwd260', 'forward only through k_tex_fwd_bin1: nine bins of 32 columns, the last partial', img=(1, 9, 260),
                     tex=(1, 32, 64, 1), uv=('iid', -1.0, 2.0), fwd_only=True))
    m = lambda name, why, **kw: out.append(_case(f'mip/{name}', why, **{**dict(tex=(1, 32, 64, 1), uv=('iid', -0.5, 1.5), da=True, bias=True), **kw}))
    for mode in ('linear-mipmap-nearest', 'linear-mipmap-linear'):
        short = mode.split('-')[-1]
        for bd in ('wrap', 'clamp', 'zero'):
            m(f'{short}/{bd}/mml4', '32 x 64, four levels', mode=mode, bd=bd, mml=4)
            m(f'{short}/{bd}/all', '32 x 64 down to 1 x 2', mode=mode, bd=bd)
    tri = 'linear-mipmap-linear'
    m('8x32', 'the chain stops when a side becomes odd: 1 x 4', mode=tri, tex=(1, 8, 32, 1))
    m('da_only', 'uv_da only', mode=tri, tex=(1, 32, 64, 3), bias=False, mml=4)
    m('bias_only', 'mip_level_bias only', mode=tri, tex=(1, 32, 64, 3), da=False, mml=4, bd='clamp')
    m('Bt2C3', 'a texture per image, three channels', mode=tri, tex=(2, 32, 64, 3), mml=4)
    m('construct', 'a texture_construct_mip stack: the gradient still collapses into tex', mode=tri, tex=(1, 32, 64, 3), mip='construct', mml=4)
    m('custom', 'a custom stack: every level keeps its own gradient', mode=tri, tex=(1, 32, 64, 3), mip='custom', mml=4, bd='clamp')
    m('custom_nearest', 'a custom stack under linear-mipmap-nearest, cut by max_mip_level', mode='linear-mipmap-nearest', tex=(2, 32, 64, 1),
      mip='custom', mml=2)
    m('tex_only', 'only tex requires grad', mode=tri, mml=4, need=('tex',))
    m('rest_only', 'uv, uv_da and the bias require grad, tex does not', mode=tri, mml=4, need=('uv', 'da', 'bias'))
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]


def _frac(shape, gen):
    """f in [9/64, 23/64] or [41/64, 55/64]: at least 1/8 from 0, 1/2 and 1 after the float32 rounding of the coordinate."""
    r = torch.rand(shape, generator=gen, dtype=torch.float64)
    half = (torch.rand(shape, generator=gen, dtype=torch.float64) < 0.5).double()
    return 9.0 / 64 + r * (14.0 / 64) + 0.5 * half


def case_inputs(case):
    """The float32 inputs of a case: dict with tex, uv, uv_da, bias, mips (a custom stack), go."""
    c = case
    gen = torch.Generator().manual_seed(1000 + c['seed'] + sum(ord(ch) for ch in c['name']))
    B, H, W = c['img']
    Bt, Ht, Wt, C = c['tex']
    tex = 0.1 + torch.rand(Bt, Ht, Wt, C, generator=gen)
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    if c['uv'][0] == 'affine':          # 1.0 x 1.5 texels per pixel
        kx = (c['uv'][1] + px)[None] + 2 * torch.arange(B)[:, None, None]
        ky = (c['uv'][2] + (3 * py) // 2)[None] + 0 * kx
    else:
        lo, hi = c['uv'][1], c['uv'][2]
        kx = torch.randint(int(math.floor(lo * Wt)), int(math.ceil(hi * Wt)), (B, H, W), generator=gen)
        ky = torch.randint(int(math.floor(lo * Ht)), int(math.ceil(hi * Ht)), (B, H, W), generator=gen)
    uv = torch.stack([(kx + _frac((B, H, W), gen)) / Wt, (ky + _frac((B, H, W), gen)) / Ht], dim=-1).float()
    # the deliberately exact pixels: uv == (0,0); u or v exactly 0 or 1
    uv[B - 1, 0, 0:3] = 0.0
    if c['uv'][0] != 'affine':          # (an affine map keeps its bins' boxes as the case names them)
        uv[0, 5, 0:4, 0] = 0.0
        uv[0, 6, 0:4, 0] = 1.0
        uv[0, 7, 0:4, 1] = 1.0
        uv[0, 8, 0:4, 1] = 0.0
    if c['origin'] == 'mixed':
        uv[0, :32, :32][((py + px) % 2 == 0)[:32, :32]] = 0.0
        uv[0, :32, 32:] = 0.0
    go = torch.randn(B, H, W, C, generator=gen)
    go[torch.rand(B, H, W, generator=gen) < 0.05] = 0.0
    if c['go'] == 'bin_zero':
        go[0, :32, :32] = 0.0
    elif c['go'] == 'single':
        keep = go[B - 1, 13, 21].clone()
        go[B - 1, :32, :32] = 0.0
        go[B - 1, 13, 21] = torch.where(keep == 0, torch.ones_like(keep), keep)
    elif c['go'] == 'scattered':
        go[torch.rand(B, H, W, generator=gen) < 0.3] = 0.0
    res = dict(tex=tex, uv=uv, go=go, uv_da=None, bias=None, mips=None)
    if 'mipmap' in c['mode']:
        nlev = num_levels(Ht, Wt, c['mml'])
        # raw levels j + 0.15 .. j + 0.35, j from -2 to n_levels + 1: every interval, below 0 and above the top, 0.15 from every
        # integer and half-integer
        j = torch.randint(-2, nlev + 2, (B, H, W), generator=gen).double()
        target = j + 0.15 + 0.2 * torch.rand(B, H, W, generator=gen, dtype=torch.float64)
        bias = None
        if c['bias']:
            bias = (torch.rand(B, H, W, generator=gen, dtype=torch.float64) * 2 - 1) if c['da'] else target.clone()
            res['bias'] = bias.float()
        if c['da']:
            # footprints (a, b; c, d) * s in texels with |A - C| >= (A + C) / 4: rt is no cancellation residue
            pat = torch.tensor([[1.0, 0.1, -0.07, 0.5], [0.5, -0.07, 0.1, 1.0]], dtype=torch.float64)
            p = pat[torch.randint(0, 2, (B, H, W), generator=gen)]
            p = p * (torch.randint(0, 2, (B, H, W, 1), generator=gen).double() * 2 - 1)
            A, Bq, Cc = p[..., 0] ** 2 + p[..., 1] ** 2, p[..., 0] * p[..., 2] + p[..., 1] * p[..., 3], p[..., 2] ** 2 + p[..., 3] ** 2
            l2 = 0.5 * (A + Cc) + torch.sqrt((0.5 * (A - Cc)) ** 2 + Bq ** 2)
            want = target - (res['bias'].double() if bias is not None else 0.0)
            s = torch.exp2(want - 0.5 * torch.log2(l2))
            da = p * s[..., None] / torch.tensor([Wt, Wt, Ht, Ht], dtype=torch.float64)
            da[torch.rand(B, H, W, generator=gen) < 0.05] = 0.0             # uv_da == 0: the level clamps to 0, no level gradient
            res['uv_da'] = da.float()
        if c['mip'] == 'custom':
            res['mips'] = [0.1 + torch.rand(Bt, Ht >> l, Wt >> l, C, generator=gen) for l in range(1, nlev + 1)]
    return res


def reference(case, inp, dtype=torch.float64, with_go=True):
    return texture(inp['tex'], inp['uv'], inp['uv_da'], inp['bias'], inp['mips'], inp['go'] if (with_go and not case['fwd_only']) else None,
                   case['mode'], case['bd'], case['mml'], dtype=dtype)


def margins(case, inp):
    """The number of pixels inside a margin, recomputed in float64 from the float32 inputs; every entry must be 0.
      coord:  a tap coordinate x_l (for 'nearest' x + 0.5) closer than (1/8) / 2^l to an integer, at any level l the case has (but for
              the prepared coordinates that are exactly 0 or 1)
      level:  a raw level inside [-1/8, n_levels + 1/8] closer than 1/8 to an integer (-linear) or to a half-integer as well (-nearest)
      rt:     a footprint other than 0 with |A - C| < (A + C) / 4"""
    Bt, Ht, Wt, C = case['tex']
    mip = 'mipmap' in case['mode']
    nlev = (len(inp['mips']) if inp['mips'] is not None else num_levels(Ht, Wt, case['mml'])) if mip else 0
    if inp['mips'] is not None and case['mml'] is not None:
        nlev = min(nlev, case['mml'])
    q = inp['uv'].double().reshape(-1, 2)
    out = dict(coord=0, level=0, rt=0)
    for l in range(nlev + 1):
        for axis, n in ((0, Wt >> l), (1, Ht >> l)):
            p, _ = _prep(q[:, axis], case['bd'])
            x = p * n - 0.5 + (0.5 if case['mode'] == 'nearest' else 0.0)
            exact = (p == 0) | (p == 1)         # a prepared coordinate of exactly 0 or 1 gives the same x in both precisions
            out['coord'] += int((~exact & ((x - torch.round(x)).abs() < 0.125 / 2 ** l)).sum())
    if mip:
        L = level_of_detail(inp['uv_da'], inp['bias'], Ht, Wt, q.shape[0])
        raw = L['raw']
        near = (raw > -0.125) & (raw < nlev + 0.125)
        d = (raw - torch.round(raw)).abs()
        if case['mode'] == 'linear-mipmap-nearest':
            d = torch.minimum(d, (raw - 0.5 - torch.round(raw - 0.5)).abs())
        out['level'] = int((near & (d < 0.125)).sum())
        if inp['uv_da'] is not None:
            live = (inp['uv_da'].reshape(-1, 4) != 0).any(1)
            out['rt'] = int((live & (L['df'].abs() * 2 < L['tr'] * 2 / 4)).sum())
    return out


def bounds(case, ref):
    """name -> n of the short paths of a case (the bound is n + 2); outputs not named here follow the long-sum rule
    e <= 8 * e32 + 4: g_tex and the levels of a custom stack (sums over all pixels that touch a texel, finished by atomics), and
    g_uv_da, whose chain of quotients through the computed l2 and rt has no practical derived count."""
    C = case['tex'][3]
    mode = case['mode']
    if mode == 'nearest':
        return {'out': N_OUT_NEAREST, 'g_uv': 0}
    if mode == 'linear':
        return {'out': N_OUT_LINEAR, 'g_uv': N_GUV_LINEAR(C)}
    chain = 0 if case['mip'] == 'custom' else CHAIN * ref['n_levels']          # the texels of a built level carry 3 roundings a level
    n_out = N_OUT_MIP_LINEAR if mode == 'linear-mipmap-linear' else N_OUT_MIP_NEAREST
    return {'out': n_out + chain, 'g_uv': N_GUV_MIP(C) + chain, 'g_bias': N_GBIAS(C) + chain}

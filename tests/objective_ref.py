"""float64 restatement on the CPU of the one-pass pixel objective (csrc/objective.hip: k_shade_list, k_fix<0>, k_fix<1>,
k_objective_finish; the non-mip call, C in 1, 3, 4, the three boundary modes), value and both gradients, without autograd: the
yardstick of tests/test_gpu_objective_ref.py, itself checked on the CPU by tests/test_objective_ref.py.  Nothing here imports
fpc_diffrend_amd; the triangle ids come from the function handed to case_inputs (oracle.ops), as in rasterize_ref.case_inputs.

The call fuses rasterize -> interpolate -> texture 'linear' -> antialias -> where(covered, ., background) -> mean squared error against
an 8-bit reference.  It is restated the way the kernels decompose it, with every value a rasterize_ref.Q (value and first-order
rounding scale S, carried from the float32 inputs down by the rules of rasterize_ref.py's docstring), so that one text gives the
float64 reference, "the same formula in float32 by torch" (dtype=float32: e32) and the per-entry scale:
    k_shade, every covered pixel   (u, v, z/w) = shade_uvz (rasterize_ref._Pixels); w = 1 - u - v, tu = u q0 + v q1 + w q2;
                                   x = prep(tu) Wt - 0.5, x0 = floor x, fx = x - x0 (_Lookup: make_taps / make_taps_fast);
                                   col = top + (bot - top) fy, top = t00 + (t10 - t00) fx; dd = rf - col cs, d0 = rf - bg cs;
                                   value += dd^2 - d0^2; gq = (-2 cs gs) dd; g_tex[tap k] += gq w_k, w_00 = (1 - fx)(1 - fy), ...;
                                   gtu = (sum_c gq dcol/dfx) Wt mu, (gu, gv) through q0 - q2, q1 - q2, then shade_uv_bwd (_uv_bwd)
    k_fix<0>, a blended pixel r    acc = col_r + sum over its active (pair, edge) entries of amt (col_o - col_r), col of an empty
                                   pixel = the texture at uv = (0, 0); dn = rf - acc cs; value += (dn^2 - d0^2) - (dd^2 - d0^2);
                                   g_aa[r] = (-2 cs gs) dn replaces gq
    k_fix<1>, pixel X of a blend   go = g_aa[X] - sum_{r = X} amt g_aa[r] + sum_{o = X, r covered} amt g_aa[r];
                                   the DIFFERENCE dl = go - gq chained like gq above (shade_pixel_bwd<false> is _uv_bwd again);
                                   d alpha / d pos once per entry with a covered receiver (antialias_ref._pos_terms, boost 1);
                                   esum = sum_{r covered, o empty} amt g_aa[r], scattered by k_objective_finish with the four
                                   weights of uv = (0, 0)
    value                          (the float sums above + C * sum over ALL pixels of (rf - b)^2) / n_total
An entry of g_pos or g_tex is the sum of its terms as the kernels form them and its S the sum of their scales: the plain term and
the difference term of a blended pixel each keep their own (S(dl) = S(go) + S(gq)), so their cancellation never shrinks S.  The
texture coordinate's scale enters through fx and fy, which carry it (texture_ref.py: coordinate-aware).  The colours and g_aa that
antialias_ref._pos_terms is handed count as inputs there (S = |value|): the d alpha / d pos terms have the scale antialias_ref gives
them, which is smaller than one carried through the lookup -- a stricter yardstick, the same for e32 and the GPU.
The value's scale is  [ sum over its terms of (S carried to the term + |dd^2| + |d0^2|) + C * bg_sumsq's ] / n_total: the first part
bounds what the per-pixel operations lose, the second what the float accumulations lose; N_VALUE below counts both.

Every discrete choice is made in float32, one rounded operation each, in the kernels' order (choices()): the clamp and renormalise
gates of the barycentrics, floor(tu) under 'wrap', tu < 0 and tu > 1 under 'clamp' (the clamp itself and the masks mu, mv), the tap
cells floor(prep(t) n - 0.5) and with them zero-mode validity, and through antialias_ref.decisions on the float32 z/w that k_shade
stores the silhouette bits, pair_select, the active edges and t >= 1/2.  Which pixels are deferred (pair_maybe on ids and silhouette
bits) and which are hit follow in integers.  reference() evaluates ON those choices and asserts that the gates rasterize_ref makes
in its own dtype agree.  margins() gives, per covered pixel and per candidate pair, how far every one of them is from flipping, in
units of u of its own scale; the constructions move a triangle and its uv until none is within SETTLE_MARGIN (no pixel left out).

float32_in_kernel_order() is reference(dtype=float32) per pixel -- the text above is written in the kernels' operation order -- and
names the texels that hold exactly ONE term, from a pixel outside every blend: there g_tex must equal gq * w_k bit for bit (one
addend through the window's double, the float cast and an atomic onto 0 is exact).  plan() restates in integers how k_shade places
its texel windows and which tables overflow; predicted_zeros() names the entries without a term.

The MIP call (inp['mip_levels'] = the number of levels below the base; None: the call above) is stated on the same skeleton, for
tests/test_gpu_objective_mip_ref.py and tests/test_objective_mip_ref.py: k_shade_mip_list/_queue, k_fix_mip_list/_queue, the host's
_build_mips / _fold_mip_grads.
    the footprint   da = (db.x e0x + db.z e1x, db.y e0x + db.w e1x, db.x e0y + db.z e1y, db.y e0y + db.w e1y), db the restated rast_db of
                    rasterize_ref._Pixels, e0 = q0 - q2, e1 = q1 - q2 the triangle's uv edges (shade_body)
    the lookup      _MipLookup = mip_lookup_fwd: compute_lod, the clamp to [0, n_levels], l0 = floor, fl, l1 = min(l0 + 1, n_levels), two
                    _Lookup on texture_ref.box_chain (a level's texel has the box average of |tex| as its scale), col = c0 + (c1 - c0) fl
    backward        per level g (1 - fl) and g fl times the four weights into that level's gradient; gtu = gfx0 w0 + gfx1 w1 with mu, mv;
                    gfl = sum_c g_c (c1 - c0) gated by 0 <= raw <= n_levels; gl2 -> gdf, gbq -> gA, gC -> gda; gdb through e0, e1 and
                    shade_pixel_bwd with derivative inputs (_uv_bwd(gd=)); the same chain on a blended pixel's difference dl (k_fix forms
                    tu, tv from the float32 u, v of the record and recomputes da: the same formulas, one rounding of u apart)
    the fold        g_tex = level 0's gradient + the box filter's backward of every coarser level, coarse to fine; S the same fold
    empty pixels    their colour is level 0's bilinear value at uv = (0, 0) (empty_color, written by the rasteriser's list round from tex) and k_objective_finish scatters esum
                    through make_taps(0, 0) into grad_tex: level 0 only.  The oracle agrees: a footprint of 0 clamps at level 0, gate closed.
The level's choices (lo = raw < 0, hi = raw > n_levels and with them the gate, l0) and the tap choices of both levels join choices() /
margins(); the level is measured in texture_ref's L_s plus the footprint's own scale through |d level / d da_k|.  plan()['mipbins'] restates
the prepass (mlb, the extent of the prepared coordinates over the pass-0 rows, the half-period view under wrap), place() for the three
windows of MipWinCaps and the routing of every pixel's two levels into a window or to memory -- it proves reach only, evaluate() never calls it.

The WEIGHTED call (inp['weights'] = dict(kind, c, mask [B,H,W] uint8 or None, face_weights [T] or None, weight_outside, saturation); absent:
the calls above, their code path untouched) is DESIGN.md 3, "Weighted objective rule", on the same skeleton, for
tests/test_gpu_objective_weighted_ref.py and tests/test_objective_weighted_ref.py: k_shade_list_w / k_shade_queue_w, k_fix_list_w / k_fix_queue_w,
rho_psi, mask_weight, face_weight, loss_grad_w and the wsum slots of fpcdr_objective_weighted_fwd (_Weights below).
    the weights     robust_ref.weights' rules: wm = mask byte * float32(1 / 255), 0 where sat > 0 and ref >= sat; a covered pixel has
                    w = wm * face_w[id - 1] (an id past the table weighs 0) and w0 = wm * w_outside; they are coefficients (no scale of their own)
    rho, psi        robust_ref.rho_psi with inv_c = robust_ref.inv_scale(c); S_psi = S_d and S_rho = S_d^2 (robust_ref's docstring: |psi'| <= 1,
                    |rho'| <= 2 |d| <= 2 S_d), then times the weight: a weight of 0 gives the exact 0 with S = 0.  There S_d = ref + |a| is a
                    magnitude; here it is CARRIED from the vertices and is thousands of times |d| on a pixel of an ill-conditioned triangle,
                    where its square says nothing (on `islands/clamp` the value's scale came to 2.5e6 times the value, and a background
                    share weighed by w instead of w0 moved the value by 0.41 u of it).  So S_rho is the smaller of S_d^2 and 2 |d| S_d, the
                    scale the plain statement's product d d carries: never above the rule's, first order where the rule's is not
    k_shade         value += w rho(dd) - w0 rho(d0);  gq = K (w psi(dd))
    k_fix<0>        value += (w rho(dn) - w0 rho(d0)) - (w rho(dd) - w0 rho(d0));  g_aa[r] = K (w psi(dn))
    k_fix<1>        dl = go - K (w psi(rf - cme cs)): the gq above
    value           (the float sums + C * sum over ALL pixels of w0 rho(d0)) / n_total
    wsum            C * sum over all pixels of w0 + C * sum over the covered pixels of (w - w0); S the same sums of w0 and of w + w0
The weights add no float32 decision (mask bytes, captures and ids are integers): choices(), margins() and the settled geometry of the cases are
those of the plain call.  The kernels skip a pixel whose gq is all zero and a difference dl that is all zero, so a pixel has a term when its weight
is positive or when it is the partner of a blend entry whose receiver has one (_structure: `has`); an entry with a weight-0 receiver has no term
at all (g_aa[r] = 0: nothing for d alpha / d pos, nothing for esum)."""
import functools
import math

import numpy as np
import torch

import antialias_ref as AR
import rasterize_ref as RR
import robust_ref as RB
import texture_ref as TR
from fitstep_ref import BACKGROUND, U, bg_sumsq, measure, rel_l2      # noqa: F401  (re-exported)
from rasterize_ref import GATE_MARGIN, SETTLE_MARGIN, Q, _clip, _inp, _where

MUTANT = None          # set by test_objective_ref.py only: a deliberately wrong restatement (see there)

BIN = 32               # OB
OWIN_CELLS = {1: 1216, 3: 1600, 4: 1600}      # owin_cells<CS>()
VT_SLOTS, FVS, FTS, ESLOTS = 256, 64, 128, 32
CS_SCALE = 255.0       # color_scale
PASS0_ROWS = (0, 1, 4, 5, 10, 11, 14, 15)     # rows of a half that its first pass shades: row pairs 0, 2, 5, 7 (0x7520)
OUTPUTS = ('g_tex', 'g_pos')

# Rounded operations on the longest path into the value, in units of the scale above (S carried like the error: a path of n operations
# loses at most (n + 1) u of S to first order).  p = x - fx w 2, a0 4, at 6, iw 7, b0 8, the renormalising sum and quotient 10, u 11;
# w = 1 - u - v 13, its product 14, the two adds of tu 16; prep 17, * Wt 18, - 0.5 19, fx 20; (t10 - t00) fx + t00: 22; bot - top 23,
# * fy 24, + top 25; * cs 26, rf - . 27; dd^2 28, - d0^2 29.  A blended pixel adds: col_o - col_r 26, * amt 27, the quad's two DPP adds
# 29, + col_r 30, dn 32, dn^2 33, - d0^2 34, and the subtraction of the plain term 35.
# Then the float accumulations of a lane -- k_shade: four pixels of C channels, 4 C; k_fix<0>: two per channel and trip, a trip per 16
# deferred pixels of the bin --, the six DPP steps of wave_sum_dpp, and the float cast of the quotient.  The four wave sums of a bin,
# the slots, the background share and the division are double.
N_VALUE_PIXEL, N_VALUE_BLEND = 29, 35
# The mip call's longest path runs through the level's fraction: b0 8 as above; da0x = w2 p1y - w1 p2y 4, datx the sum of three 6, b0 datx 10,
# da0x - . 11, * iw 12, * sx 13 (rast_db); the uv edge e0x 1, db.x e0x 15, the sum of two 16 (da); texture_ref.N_LEVEL = 12 operations from
# da to fl (the device's log2f counted as one of them): 28; c1 - c0 is shorter (26), (c1 - c0) fl 29, + c0 30; * cs 31, rf - . 32, dd^2 33,
# - d0^2 34.  A blended pixel adds the same six as above: 40.
N_VALUE_PIXEL_MIP, N_VALUE_BLEND_MIP = 16 + TR.N_LEVEL + 6, 16 + TR.N_LEVEL + 12


# The bar is (n_value + 2) u of S, as in fitstep_ref.py: n_value + 1 is the first-order bound of a path of n_value operations, and one more u
# stands for the second-order terms (n^2 u^2, far below u at these counts).  It is a worst-case count against a scale summed over thousands
# of pixels, so measured errors are a hundredth of a u: this bar sees a wrong term, a wrong factor or a lost pixel, not a lost bit.
def n_value(C, max_deferred_in_a_bin, mip=False, kind=None):
    """kind: the weighted call's (None: the plain and the mip call)."""
    trips = -(-4 * max_deferred_in_a_bin // 64)
    pixel, blend = (N_VALUE_PIXEL_MIP, N_VALUE_BLEND_MIP) if mip else (N_VALUE_PIXEL, N_VALUE_BLEND)
    if kind is not None:
        assert not mip
        pixel, blend = N_VALUE_PIXEL_W[kind], N_VALUE_BLEND_W[kind]
    return max(pixel + 4 * C, blend + 2 * C * trips) + 6 + 1


# The weighted call.  Where rho's scale is S_d^2 (robust_ref's docstring), not the 2 |d| S_d a product carries, what d has lost counts TWICE:
# |rho'| <= 2 |d| <= 2 S_d for every kind (where it is 2 |d| S_d it counts once: the count below holds for both), and d = dd is 27 operations
# down the path above (dn, of a blended pixel: 32).  Behind d, relative to
# |rho| <= d^2 <= S_d^2 and by robust_ref's rules (a product n_a + n_b + 1, a sum max + 1, a product with 2 exact, d itself counted already):
#     L2              d d 1
#     Charbonnier     z 1, t = z z 3, 1 + t 4, the root 5, 1 + h 6; 2 (d d) 1; the quotient 1 + 6 + 1 = 8
#     Geman-McClure   z 1, t 3, k = 1 + t 4; d d 1; the quotient 1 + 4 + 1 = 6
# then the weight's two operations (wm, wm * face weight) and its product with rho, 3, and the subtraction of w0 rho(d0) (a shorter path), 1:
# 2 * 27 + 4 + rho's.  A blended pixel: 2 * 32 + 4 + rho's, and the subtraction of the plain term, 1.  The accumulations are n_value's.
N_RHO = {'l2': 1, 'charbonnier': 8, 'geman_mcclure': 6}
N_VALUE_PIXEL_W = {k: 2 * 27 + 4 + n for k, n in N_RHO.items()}
N_VALUE_BLEND_W = {k: 2 * 32 + 5 + n for k, n in N_RHO.items()}


def _coef(x):
    return Q(x, torch.zeros_like(x))


def _at(q, idx):
    return Q(q.v[idx], q.S[idx])


def _zeros(n, dtype):
    return Q(torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype))


# ---------------------------------------------------------------------------------------------------------------------
# the texture lookup (behind one class: the mip branch can be stated on the same skeleton)
# ---------------------------------------------------------------------------------------------------------------------

class _Lookup:
    """make_taps / make_taps_fast + load_taps + mask_taps for n pixels at (tu, tv) (Q) in tex [Ht,Wt,C].  ch: the float32 choices
    (a dict this fills when it is empty, and follows otherwise).  Taps k = 0..3 are (00, 10, 01, 11)."""

    def __init__(self, tex, tu, tv, boundary, dtype, ch, tex_S=None):
        """tex_S: the texels' scales (a level of the box chain: the box average of |tex|); None: the texels are inputs, S = |t|."""
        Ht, Wt, C = tex.shape
        make = len(ch) == 0
        self.gates = []      # Q whose value must stay positive for the choice to hold

        def coord(t, n, key):
            one = torch.ones_like(t.v)
            if boundary == 'wrap':
                if make:
                    ch[key + 'fl'] = torch.floor(t.v)
                fl = ch[key + 'fl'].to(dtype)
                p = Q(t.v - fl, t.S + fl.abs())
                self.gates += [p, Q(fl + 1.0 - t.v, p.S)]
            elif boundary == 'clamp':
                if make:
                    ch[key + 'lo'], ch[key + 'hi'] = t.v < 0, t.v > 1
                lo, hi = ch[key + 'lo'], ch[key + 'hi']
                p = _where(lo, _coef(torch.zeros_like(one)), _where(hi, Q(one, one), t))
                self.gates += [Q(torch.where(lo, -t.v, t.v), t.S), Q(torch.where(hi, t.v - 1.0, 1.0 - t.v), t.S + 1.0)]
            else:
                p = t
            x = Q(p.v * float(n) - 0.5, p.S * float(n) + 0.5)
            if make:
                ch[key + 'x0'] = torch.floor(x.v)
            x0f = ch[key + 'x0'].to(dtype)
            f = Q(x.v - x0f, x.S)
            self.gates += [f, Q(x0f + 1.0 - x.v, x.S)]
            inside = ~(ch[key + 'lo'] | ch[key + 'hi']) if boundary == 'clamp' else torch.ones_like(t.v, dtype=torch.bool)
            return f, ch[key + 'x0'].long(), inside

        self.fx, self.x0, in_u = coord(tu, Wt, 'u')
        self.fy, self.y0, in_v = coord(tv, Ht, 'v')
        self.mu, self.mv = in_u.to(dtype), in_v.to(dtype)
        ix = (TR._idx(self.x0, Wt, boundary), TR._idx(self.x0 + 1, Wt, boundary))
        iy = (TR._idx(self.y0, Ht, boundary), TR._idx(self.y0 + 1, Ht, boundary))
        vx = (TR._inside(self.x0, Wt, boundary), TR._inside(self.x0 + 1, Wt, boundary))
        vy = (TR._inside(self.y0, Ht, boundary), TR._inside(self.y0 + 1, Ht, boundary))
        t = tex.detach().to('cpu', dtype)
        tS = t.abs() if tex_S is None else tex_S.detach().to('cpu', dtype)
        self.flat, self.valid, self.t = [], [], []
        for k in range(4):
            jx, jy = k & 1, k >> 1
            ok = vx[jx] & vy[jy]
            self.flat.append(iy[jy] * Wt + ix[jx])
            self.valid.append(ok)
            m = ok.to(dtype)
            self.t.append([Q(t[iy[jy], ix[jx], c] * m, tS[iy[jy], ix[jx], c] * m) for c in range(C)])
        fx, fy = self.fx, self.fy
        self.col = []
        for c in range(C):
            t00, t10, t01, t11 = (self.t[k][c] for k in range(4))
            top = t00 + (t10 - t00) * fx
            bot = t01 + (t11 - t01) * fx
            self.col.append(top + (bot - top) * fy)
        self.wk = [(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy]
        self.Ht, self.Wt, self.C = Ht, Wt, C

    def backward(self, g):
        """g: C Q [n] = d loss / d colour -> (gtu, gtv): d loss / d (tu, tv), masked by mu, mv."""
        fx, fy = self.fx, self.fy
        gfx = gfy = _zeros(fx.v.numel(), fx.v.dtype)
        for c in range(self.C):
            t00, t10, t01, t11 = (self.t[k][c] for k in range(4))
            gfx = gfx + g[c] * ((t10 - t00) * (1.0 - fy) + (t11 - t01) * fy)
            gfy = gfy + g[c] * ((t01 + (t11 - t01) * fx) - (t00 + (t10 - t00) * fx))
        return gfx * float(self.Wt) * self.mu, gfy * float(self.Ht) * self.mv

    def scatter(self, G, GS, g, rows):
        """g_tex[tap k] += g_c * w_k for the pixels `rows`, at the taps that exist."""
        for k in range(4):
            ok = self.valid[k][rows]
            if MUTANT == 'zero_padding_gets_gradient':
                ok = torch.ones_like(ok)
            for c in range(self.C):
                term = _at(g[c], rows) * _at(self.wk[k], rows)
                idx = self.flat[k][rows][ok] * self.C + c
                G.index_add_(0, idx, term.v[ok])
                GS.index_add_(0, idx, term.S[ok])


LN2 = 0.6931471805599453


def _pick(q, m):
    return Q(q.v[m], q.S[m])


def _spread(q, m, n, fill_v=0.0):
    """Q over the pixels m of n -> Q [n] (fill_v with no scale elsewhere)."""
    v, S = torch.full((n,), fill_v, dtype=q.v.dtype), torch.zeros(n, dtype=q.v.dtype)
    v[m], S[m] = q.v, q.S
    return Q(v, S)


class _MipLookup:
    """mip_lookup_fwd / mip_lookup_bwd (csrc/texsample.h; mip_sample_bwd in k_fix is the same formulas) for n pixels at (tu, tv) with the
    footprint da (four Q: dudx, dudy, dvdx, dvdy of the texture coordinate per pixel) in the box chain of tex [Ht,Wt,C], levels 0..n_levels.
    The level's discrete choices (float32, ch['level']): lo = raw < 0 and hi = raw > n_levels (the two clamps, and with them the gate
    raw in [0, n_levels] of the level's gradient), l0 = min(floor(level), n_levels); the tap choices of each level's lookup are those of
    _Lookup on the pixels of that l0 (ch[('a', l)], ch[('b', l)]).
    The raw level carries texture_ref's L_s -- |0.5 log2 l2| + 0.5 / ln 2 (tr + rt_s) / l2, which counts the device's log2f (not correctly
    rounded) as one of the N_LEVEL operations behind it -- plus, to first order, |d level / d da_k| S(da_k): here the footprint is no input."""

    def __init__(self, tex, n_levels, tu, tv, da, boundary, dtype, ch):
        Ht, Wt, C = tex.shape
        n = tu.v.numel()
        self.n, self.C, self.Ht, self.Wt, self.nl, self.dtype = n, C, Ht, Wt, n_levels, dtype
        chain, chainA = TR.box_chain(tex[None], n_levels, dtype)
        self.dims = [(t.shape[1], t.shape[2]) for t in chain]
        # compute_lod
        dudx, dudy, dvdx, dvdy = da[0] * float(Wt), da[1] * float(Wt), da[2] * float(Ht), da[3] * float(Ht)
        if MUTANT == 'level_from_Wt_alone':
            dvdx, dvdy = da[2] * float(Wt), da[3] * float(Wt)
        A, Bq, Cc = dudx * dudx + dudy * dudy, dudx * dvdx + dudy * dvdy, dvdx * dvdx + dvdy * dvdy
        tr, df = (A + Cc) * 0.5, (A - Cc) * 0.5
        arg = df * df + Bq * Bq + 1e-30
        rtv = torch.sqrt(arg.v)
        rt = Q(rtv, arg.S / (2.0 * rtv))
        l2 = tr + rt
        raw_v = 0.5 * torch.log2(l2.v.clamp(min=1e-30))
        self.L = dict(dudx=dudx, dudy=dudy, dvdx=dvdx, dvdy=dvdy, df=df, bq=Bq, rt=rt, l2=l2)
        # L_s of texture_ref.level_of_detail on the values, and the footprint's own scale through |d level / d da_k|
        BqA = (dudx.v * dvdx.v).abs() + (dudy.v * dvdy.v).abs()
        rtS = (tr.v * tr.v + BqA * BqA + 1e-30) / rtv
        Ls = raw_v.abs() + (0.5 / math.log(2.0)) * (tr.v + rtS) / l2.v
        one = Q(torch.ones(n, dtype=dtype), torch.zeros(n, dtype=dtype))
        for k, sens in enumerate(self._footprint_bwd(one, absolute=True)):
            Ls = Ls + sens.v * da[k].S
        raw = Q(raw_v, Ls)
        lev = ch.setdefault('level', {})
        if not lev:
            lev['lo'], lev['hi'] = raw_v < 0, raw_v > float(n_levels)
            level32 = raw_v.clamp(0.0, float(n_levels))
            lev['l0'] = torch.floor(level32).long().clamp(max=n_levels)
        lo, hi, l0 = lev['lo'], lev['hi'], lev['l0']
        self.lo, self.hi, self.l0, self.raw = lo, hi, l0, raw
        self.passes = ~(lo | hi)
        if MUTANT == 'level_gate_ignored':
            self.passes = torch.ones_like(lo)
        zero = _zeros(n, dtype)
        level = _where(lo, zero, _where(hi, Q(torch.full((n,), float(n_levels), dtype=dtype), torch.zeros(n, dtype=dtype)), raw))
        l0f = l0.to(dtype)
        self.fl = fl = Q(level.v - l0f, level.S)
        self.l1 = (l0 + 1).clamp(max=n_levels)
        safe = Q(torch.ones(n, dtype=dtype), torch.zeros(n, dtype=dtype))
        free = self.passes
        # the clamps (raw against 0 and n_levels), floor(level) -- a clamped level is exact and has none
        self.gates = [Q(torch.where(lo, -raw.v, raw.v), raw.S), Q(torch.where(hi, raw.v - float(n_levels), float(n_levels) - raw.v), raw.S),
                      _where(free, fl, safe), _where(free, Q(l0f + 1.0 - level.v, level.S), safe)]
        self.level_gates = list(self.gates)
        if MUTANT == 'fl_and_1_minus_fl_exchanged':
            fl = 1.0 - fl
        # the two bilinear lookups, level by level
        self.groups = []
        mu, mv = torch.ones(n, dtype=dtype), torch.ones(n, dtype=dtype)
        c0 = [zero for _ in range(C)]
        c1 = [zero for _ in range(C)]
        for l in range(n_levels + 1):
            m = torch.nonzero(l0 == l, as_tuple=True)[0]
            if not m.numel():
                continue
            lu = min(l + 1, n_levels)
            tum, tvm = _pick(tu, m), _pick(tv, m)
            a = _Lookup(chain[l][0], tum, tvm, boundary, dtype, ch.setdefault(('a', l), {}), chainA[l][0])
            b = _Lookup(chain[lu][0], tum, tvm, boundary, dtype, ch.setdefault(('b', l), {}), chainA[lu][0])
            self.groups.append((m, l, lu, a, b))
            mu[m], mv[m] = a.mu, a.mv
            for q in a.gates + b.gates:
                self.gates.append(_spread(q, m, n, 1.0))
            for c in range(C):
                c0[c] = c0[c] + _spread(a.col[c], m, n)
                c1[c] = c1[c] + _spread(b.col[c], m, n)
        self.mu, self.mv, self.c0, self.c1, self.fl_used = mu, mv, c0, c1, fl
        self.col = [c0[c] + (c1[c] - c0[c]) * fl for c in range(C)]

    def _footprint_bwd(self, glevel, absolute=False):
        """glevel Q [n] = d loss / d level (already gated) -> d loss / d da, four Q.  absolute: every factor by its absolute value and
        every subtraction an addition (the sensitivities |d level / d da_k| of the level's scale)."""
        L = self.L
        f = (lambda q: Q(q.v.abs(), q.S)) if absolute else (lambda q: q)
        l2, rt = L['l2'], L['rt']
        gl2 = _where(l2.v >= 1e-30, glevel * 0.5 / (l2 * LN2), 0.0)
        gdf, gbq = gl2 * f(L['df']) / rt, gl2 * f(L['bq']) / rt
        gA = gl2 * 0.5 + gdf * 0.5
        gC = gl2 * 0.5 + gdf * 0.5 if absolute else gl2 * 0.5 - gdf * 0.5
        dudx, dudy, dvdx, dvdy = f(L['dudx']), f(L['dudy']), f(L['dvdx']), f(L['dvdy'])
        g_dudx = dudx * 2.0 * gA + dvdx * gbq
        g_dudy = dudy * 2.0 * gA + dvdy * gbq
        g_dvdx = dvdx * 2.0 * gC + dudx * gbq
        g_dvdy = dvdy * 2.0 * gC + dudy * gbq
        Wt, Ht = float(self.Wt), float(self.Ht)
        return [g_dudx * Wt, g_dudy * Wt, g_dvdx * Ht, g_dvdy * Ht]

    def backward(self, g):
        """g: C Q [n] -> (gtu, gtv) masked by mu, mv, and gda (four Q): the gradient of the footprint."""
        n, fl = self.n, self.fl_used
        gtu = gtv = gfl = _zeros(n, self.dtype)
        for m, l, lu, a, b in self.groups:
            flm = _pick(fl, m)
            ga, gb = [_pick(g[c], m) * (1.0 - flm) for c in range(self.C)], [_pick(g[c], m) * flm for c in range(self.C)]
            au, av = a.backward(ga)
            bu, bv = b.backward(gb)
            gtu, gtv = gtu + _spread(au + bu, m, n), gtv + _spread(av + bv, m, n)
        for c in range(self.C):
            gfl = gfl + g[c] * (self.c1[c] - self.c0[c])
        glevel = _where(self.passes, gfl, 0.0)
        gda = self._footprint_bwd(glevel)
        if MUTANT == 'gda_dropped':
            gda = [q * 0.0 for q in gda]
        return gtu, gtv, gda

    def scatter(self, G, GS, g, rows):
        """Per level l, G[l] += (g_c (1 - fl)) w_k at level l0's taps and (g_c fl) w_k at level l1's, for the pixels `rows`."""
        sel = torch.zeros(self.n, dtype=torch.bool)
        sel[rows] = True
        for m, l, lu, a, b in self.groups:
            local = torch.nonzero(sel[m], as_tuple=True)[0]
            if not local.numel():
                continue
            flm = _pick(self.fl_used, m)
            a.scatter(G[l], GS[l], [_pick(g[c], m) * (1.0 - flm) for c in range(self.C)], local)
            b.scatter(G[lu], GS[lu], [_pick(g[c], m) * flm for c in range(self.C)], local)

    def level_reach(self):
        """Per level, [h*w] the number of tap terms from the choices alone (an upper level whose fraction is the exact 0 of a clamp has none)."""
        count = [torch.zeros(h * w, dtype=torch.int64) for h, w in self.dims]
        for m, l, lu, a, b in self.groups:
            live_b = self.passes[m]
            for k in range(4):
                count[l].index_add_(0, a.flat[k][a.valid[k]], torch.ones(int(a.valid[k].sum()), dtype=torch.int64))
                ok = b.valid[k] & live_b
                count[lu].index_add_(0, b.flat[k][ok], torch.ones(int(ok.sum()), dtype=torch.int64))
        return count

    def any_valid(self):
        out = torch.zeros(self.n, dtype=torch.bool)
        for m, l, lu, a, b in self.groups:
            va = a.valid[0] | a.valid[1] | a.valid[2] | a.valid[3]
            vb = (b.valid[0] | b.valid[1] | b.valid[2] | b.valid[3]) & self.passes[m]
            out[m] = va | vb
        return out


def fold_levels(G, scale=False):
    """_fold_mip_grads: the box filter's backward, coarse to fine: every coarse texel's quarter to its four fine ones -> level 0's [h,w,C]."""
    wq = 0.5 if (MUTANT == 'fold_weight_half' and scale is False) else 0.25
    if scale is None:      # (counts of terms: summed as they are)
        wq = 1
    g = G[-1]
    for l in range(len(G) - 1, 0, -1):
        g = G[l - 1] + wq * g.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
    return g


def _uv_bwd(px, gu, gv, gd=None):
    """shade_uv_bwd on the kept values of px (= shade_pixel_bwd<false>, which recomputes the same operations): (gu, gv) Q [n] -> the
    nine components (vertex 0: x, y, w; vertex 1; vertex 2).  gd: four Q = d loss / d rast_db (shade_pixel_bwd<true>, the mip call: the
    statement of rasterize_ref._Pixels.backward on Q inputs)."""
    p0x, p0y, p1x, p1y, p2x, p2y = px.p
    fx, fy, a0, a1, iw, b0, b1, uc, vc = px.fx, px.fy, px.a0, px.a1, px.iw, px.b0, px.b1, px.uc, px.vc
    s = 1.0 / px.sum
    dot = (uc * gu + vc * gv) * s * s
    guc, gvc = _where(px.ren, gu * s - dot, gu), _where(px.ren, gv * s - dot, gv)
    open0, open1 = (b0.v >= 0.0) & (b0.v <= 1.0), (b1.v >= 0.0) & (b1.v <= 1.0)
    gb0, gb1 = _where(open0, guc, 0.0), _where(open1, gvc, 0.0)
    zero = _zeros(px.n, px.dtype)
    if gd is not None:
        w0, w1, w2 = px.w
        sx, sy = px.sx, px.sy
        da0x, da0y, da1x, da1y, da2x, da2y = px.da
        datx, daty = px.datx, px.daty
        gw0 = gw1 = gw2 = gp0x = gp0y = gp1x = gp1y = gp2x = gp2y = zero
        hx0, hy0, hx1, hy1 = gd[0] * sx, gd[1] * sy, gd[2] * sx, gd[3] * sy
        n0x, n0y = da0x - b0 * datx, da0y - b0 * daty
        n1x, n1y = da1x - b1 * datx, da1y - b1 * daty
        giw = hx0 * n0x + hy0 * n0y + hx1 * n1x + hy1 * n1y
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
        ga0, ga1 = gb0 * iw, gb1 * iw
        giw = giw + (gb0 * a0 + gb1 * a1)
        gat = -giw * iw * iw
        ga0, ga1, ga2 = ga0 + gat, ga1 + gat, gat
        gp1x = gp1x + ga0 * p2y; gp2y = gp2y + ga0 * p1x; gp1y = gp1y - ga0 * p2x; gp2x = gp2x - ga0 * p1y
        gp2x = gp2x + ga1 * p0y; gp0y = gp0y + ga1 * p2x; gp2y = gp2y - ga1 * p0x; gp0x = gp0x - ga1 * p2y
        gp0x = gp0x + ga2 * p1y; gp1y = gp1y + ga2 * p0x; gp0y = gp0y - ga2 * p1x; gp1x = gp1x - ga2 * p0y
        return [gp0x, gp0y, gw0 - fx * gp0x - fy * gp0y, gp1x, gp1y, gw1 - fx * gp1x - fy * gp1y, gp2x, gp2y, gw2 - fx * gp2x - fy * gp2y]
    ga0, ga1 = gb0 * iw, gb1 * iw
    giw = gb0 * a0 + gb1 * a1
    gat = -giw * iw * iw
    ga0, ga1, ga2 = ga0 + gat, ga1 + gat, gat
    gp1x = ga0 * p2y; gp2y = ga0 * p1x; gp1y = zero - ga0 * p2x; gp2x = zero - ga0 * p1y
    gp2x = gp2x + ga1 * p0y; gp0y = ga1 * p2x; gp2y = gp2y - ga1 * p0x; gp0x = zero - ga1 * p2y
    gp0x = gp0x + ga2 * p1y; gp1y = gp1y + ga2 * p0x; gp0y = gp0y - ga2 * p1x; gp1x = gp1x - ga2 * p0y
    return [gp0x, gp0y, zero - fx * gp0x - fy * gp0y, gp1x, gp1y, zero - fx * gp1x - fy * gp1y, gp2x, gp2y, zero - fx * gp2x - fy * gp2y]


def _edge_pos_terms(D, E, colP, gaa, dtype):
    """aa_edge_pos_grad for every active (pair, edge) entry, G = sum_c g_aa[receiver]_c (col[P]_c - col[Q]_c) on the colours and gradients
    of THIS call (Q per channel over all pixels; g_aa of an empty pixel is 0: such an entry has no term) -> (rows of va, rows of vb,
    [x, y, w] of a, of b, keep: the entries not left at G == 0).  antialias_ref._pos_terms is this with colour and dy as inputs."""
    pr, i, e = D.pairs, D.ei, D.ee
    hw, hh = 0.5 * D.W, 0.5 * D.H
    G = _zeros(i.numel(), dtype)
    for c in range(len(colP)):
        G = G + _at(gaa[c], D.er) * (_at(colP[c], pr.pP[i]) - _at(colP[c], pr.pQ[i]))
    pick = lambda k: Q(E[k].v[i, e], E[k].S[i, e])
    t, Ld = pick('t'), pick('Ld')
    s = Q(E['s'].v[i], E['s'].S[i])
    qax, qay, wa, qbx, qby, wb = (pick(k) for k in ('qax', 'qay', 'wa', 'qbx', 'qby', 'wb'))
    gLz = (-G) / (s * Ld)
    gLd = ((-G) * t) / Ld
    is_x = pr.d[i] == 0
    zero = _zeros(i.numel(), dtype)
    gLx, gLy = _where(is_x, gLd, zero), _where(is_x, zero, gLd)
    g_qay = zero + gLx * wb; g_wb = zero + gLx * qay; g_wa = zero - gLx * qby; g_qby = zero - gLx * wa
    g_wa = g_wa + gLy * qbx; g_qbx = zero + gLy * wa; g_qax = zero - gLy * wb; g_wb = g_wb - gLy * qax
    g_qax = g_qax + gLz * qby; g_qby = g_qby + gLz * qax; g_qay = g_qay - gLz * qbx; g_qbx = g_qbx - gLz * qay
    fxp, fyp = _coef(pr.Px[i].to(dtype) + 0.5 - hw), _coef(pr.Py[i].to(dtype) + 0.5 - hh)
    if MUTANT == 'w_column_with_fxp_fyp_swapped':
        fxp, fyp = fyp, fxp
    ta = [g_qax * hw, g_qay * hh, g_wa - fxp * g_qax - fyp * g_qay]
    tb = [g_qbx * hw, g_qby * hh, g_wb - fxp * g_qbx - fyp * g_qby]
    base = pr.b[i] * D.V
    return base + D.E['va'][i, e], base + D.E['vb'][i, e], ta, tb, G.v != 0


# ---------------------------------------------------------------------------------------------------------------------
# choices and evaluation
# ---------------------------------------------------------------------------------------------------------------------

def _consts(inp, dtype):
    """The float32 numbers the kernels are handed, as `dtype` tensors: gs = 1 / n_total, K = (-2 cs gs) formed first, bg cs."""
    B, (H, W), C = inp['pos'].shape[0], inp['res'], inp['tex'].shape[2]
    n_total = inp.get('n_total') or B * H * W * C
    gs = np.float32(1.0 / n_total)
    K = (torch.tensor(-2.0 * CS_SCALE, dtype=dtype) * torch.tensor(float(gs), dtype=dtype))
    if MUTANT == 'gq_without_2':
        K = K * 0.5
    bgs = np.float32(np.float32(inp.get('background', BACKGROUND)) * np.float32(CS_SCALE))
    return n_total, K, torch.tensor(float(bgs), dtype=dtype)


class _State:
    pass


class _Weights:
    """The weights of a weighted call per pixel, in `dtype`, by robust_ref.weights (mask_weight, face_weight; k_fix forms them by the same
    expressions): w [P] (covered pixels: wm * face weight; 0 elsewhere), w0 [P] (ALL pixels: wm * w_outside), and rho / psi of a residual Q
    (rho_psi) with the scales of the module docstring."""

    def __init__(self, inp, dtype):
        wt = inp['weights']
        assert inp.get('mip_levels') is None, "the mip call has no weighted form"
        self.kind, self.dtype = wt['kind'], dtype
        assert self.kind in RB.KINDS
        self.inv_c = RB.inv_scale(wt['c']) if self.kind != 'l2' else 0.0
        ids = inp['ids'].detach().cpu().long()
        sat = int(wt.get('saturation', 0))
        if MUTANT == 'saturation_as_greater' and sat > 0:
            sat += 1
        rast_w = ids.float()
        if MUTANT == 'face_weight_of_id':
            rast_w = torch.where(ids > 0, ids + 1, ids).float()
        kw = dict(mask=wt.get('mask'), w_outside=float(wt.get('weight_outside', 1.0)), sat=sat, dtype=dtype)
        w, cov = RB.weights(rast_w, inp['ref_u8'], face_w=wt.get('face_weights'), **kw)
        w0, _ = RB.weights(torch.zeros_like(rast_w), inp['ref_u8'], face_w=None, **kw)
        self.w0 = w0.reshape(-1)
        self.w = torch.where(cov, w, torch.zeros((), dtype=dtype)).reshape(-1)
        if MUTANT == 'w0_for_a_covered_pixel':
            self.w = torch.where(cov.reshape(-1), self.w0, self.w)

    def rho(self, d):
        v = RB.rho_psi(d.v, self.kind, self.inv_c, RB.sqrt_rounded)[0]      # (the device's sqrtf is correctly rounded; torch's float32 root is not)
        if MUTANT == 'charbonnier_rho_without_2' and self.kind == 'charbonnier':
            v = v * 0.5
        return Q(v, torch.minimum(d.S * d.S, 2.0 * d.v.abs() * d.S))      # (module docstring: S_rho)

    def psi(self, d):
        v = d.v if MUTANT == 'psi_without_s' else RB.rho_psi(d.v, self.kind, self.inv_c, RB.sqrt_rounded)[1]
        return Q(v, d.S)


def _tex_coord(px, inp, dtype):
    uvt = inp['uv'].detach().to('cpu', dtype)[inp['uv_tri'].detach().cpu().long()[px.t]]      # [n,3,2]
    q = [[_inp(uvt[:, k, c]) for c in range(2)] for k in range(3)]
    u, v = px.uvz[0], px.uvz[1]
    w = 1.0 - u - v
    if MUTANT == 'tu_summed_in_another_order':
        tu, tv = (u * q[0][0] + w * q[2][0]) + v * q[1][0], (u * q[0][1] + w * q[2][1]) + v * q[1][1]
    else:
        tu, tv = u * q[0][0] + v * q[1][0] + w * q[2][0], u * q[0][1] + v * q[1][1] + w * q[2][1]
    return q, tu, tv


def _forward(inp, dtype, ch):
    """k_shade's per-pixel forward in dtype; ch: dict of the float32 choices (filled when empty)."""
    st = _State()
    H, W = inp['res']
    st.px = px = RR._Pixels(inp['pos'], inp['tri'], inp['ids'], (H, W), dtype)
    st.q, st.tu, st.tv = _tex_coord(px, inp, dtype)
    st.mip = inp.get('mip_levels')
    if st.mip is None:
        st.lk = _Lookup(inp['tex'], st.tu, st.tv, inp['boundary'], dtype, ch.setdefault('taps', {}))
    else:
        # shade_body: da from the barycentrics' screen derivatives (rasterize_ref: rast_db) and the triangle's two uv edges
        q, db = st.q, px.db
        st.e = e0x, e0y, e1x, e1y = q[0][0] - q[2][0], q[0][1] - q[2][1], q[1][0] - q[2][0], q[1][1] - q[2][1]
        st.da = [db[0] * e0x + db[2] * e1x, db[1] * e0x + db[3] * e1x, db[0] * e0y + db[2] * e1y, db[1] * e0y + db[3] * e1y]
        if MUTANT == 'dudy_and_dvdx_swapped_in_da':
            st.da = [st.da[0], st.da[2], st.da[1], st.da[3]]
        st.lk = _MipLookup(inp['tex'], st.mip, st.tu, st.tv, st.da, inp['boundary'], dtype, ch.setdefault('taps', {}))
    zero = _zeros(1, dtype)
    if MUTANT == 'esum_with_wrap_taps_under_clamp' and inp['boundary'] == 'clamp':
        st.lk0 = _Lookup(inp['tex'], zero, zero, 'wrap', dtype, {})
    else:
        st.lk0 = _Lookup(inp['tex'], zero, zero, inp['boundary'], dtype, ch.setdefault('taps0', {}))
    if 'ren' not in ch:
        ch['ren'], ch['open0'], ch['open1'] = px.ren, (px.b0.v >= 0) & (px.b0.v <= 1), (px.b1.v >= 0) & (px.b1.v <= 1)
        ch['lo0'], ch['lo1'] = px.b0.v < 0, px.b1.v < 0
        rast = torch.zeros(px.B, H, W, 4)
        rast[px.bi, px.yy, px.xx, 2] = px.uvz[2].v.float()      # (float64 only on _unsafe's way out of a gate the two dtypes decide differently)
        rast[..., 3] = inp['ids'].float()
        ch['rast'] = rast
        ch['adj'] = AR.topology(inp['tri'])
        ch['D'] = AR.decisions(None, rast, inp['pos'], inp['tri'], ch['adj'])
    else:
        same = torch.equal(px.ren, ch['ren']) and torch.equal((px.b0.v >= 0) & (px.b0.v <= 1), ch['open0']) and \
            torch.equal((px.b1.v >= 0) & (px.b1.v <= 1), ch['open1']) and torch.equal(px.b0.v < 0, ch['lo0']) and torch.equal(px.b1.v < 0, ch['lo1'])
        assert same, "a barycentric gate decides differently in float32: the case is not settled"
    return st


@functools.lru_cache(maxsize=None)
def _choices_cached(name):
    ch = {}
    _forward(_case_cache[name], torch.float32, ch)
    return ch


def choices(inp):
    """Every discrete choice of a call, made in float32 (module docstring) -> dict: ren, open0, open1 (barycentric gates), taps (floor(tu),
    clamp states and tap cells per axis), taps0 (the lookup at uv = (0, 0)), rast (z/w as k_shade stores it, ids), adj, D
    (antialias_ref.decisions).  Cached for a case's inputs: treat as read-only."""
    if _case_cache.get(inp.get('name')) is inp:
        return _choices_cached(inp.get('base', inp['name']))      # (with_weights: the weights add no choice, the case's own serve)
    ch = {}
    _forward(inp, torch.float32, ch)
    return ch


def evaluate(inp, dtype=torch.float64):
    """The statement on the choices of choices(inp) -> dict: 'value' (value, S) scalars, 'g_pos' (value, S) [B,V,4], 'g_tex' (value, S)
    [Ht,Wt,C], and what the tests look at: 'st' (the forward), 'D', 'E', 'hit' / 'hit2' (flat pixel indices of the blended covered pixels /
    of the pixels k_fix<1> visits), 'gq' [n,C] values, 'dd' [n,C] values, 'esum' (C values), 'n_esum' entries, 'terms' per texel.  The weighted call
    (inp['weights']) adds 'wsum' (value, S) and 'w', 'w0' [n], the covered pixels' weights."""
    ch = choices(inp)
    st = _forward(inp, dtype, ch)
    px, lk, lk0, D = st.px, st.lk, st.lk0, ch['D']
    B, (H, W) = px.B, inp['res']
    Ht, Wt, C = inp['tex'].shape
    P, n = B * H * W, px.n
    n_total, K, bgs = _consts(inp, dtype)
    Kq = Q(K, K.abs())
    pix = (px.bi * H + px.yy) * W + px.xx                        # flat pixel index of every covered pixel
    rowof = torch.full((P,), -1, dtype=torch.int64)
    rowof[pix] = torch.arange(n)
    cov = rowof >= 0
    rf_all = inp['ref_u8'].detach().cpu().to(dtype).reshape(-1)
    rf = _inp(rf_all[pix])
    d0 = rf - Q(bgs.expand(n), bgs.abs().expand(n))
    dd = [rf - lk.col[c] * CS_SCALE for c in range(C)]
    wg = _Weights(inp, dtype) if inp.get('weights') is not None else None
    if wg is None:
        gq = [Kq * dd[c] for c in range(C)]
    else:      # the weights of the covered pixels as coefficients; what every covered pixel's background term weighed
        w, w0 = _coef(wg.w[pix]), _coef(wg.w0[pix])
        w0rho = w0 * wg.rho(d0)
        gq = [Kq * (w * wg.psi(dd[c])) for c in range(C)]
    mip = st.mip is not None
    if mip:      # one gradient per level of the chain, folded into level 0's at the end (_fold_mip_grads)
        L_tex = [torch.zeros(h * w * C, dtype=dtype) for h, w in lk.dims]
        LS_tex = [torch.zeros(h * w * C, dtype=dtype) for h, w in lk.dims]
        G_tex, S_tex = L_tex[0], LS_tex[0]
    else:
        G_tex, S_tex = torch.zeros(Ht * Wt * C, dtype=dtype), torch.zeros(Ht * Wt * C, dtype=dtype)
    G_pos, S_pos = torch.zeros(B * px.V, 4, dtype=dtype), torch.zeros(B * px.V, 4, dtype=dtype)
    every = torch.arange(n)

    def chain(g, rows):
        """texture, interpolate and rasterize backward of d loss / d colour g (C Q [n]) for the pixels `rows`."""
        q = st.q
        if mip:
            lk.scatter(L_tex, LS_tex, g, rows)
            gtu, gtv, gda = lk.backward(g)
            e0x, e0y, e1x, e1y = st.e
            gdb = [gda[0] * e0x + gda[2] * e0y, gda[1] * e0x + gda[3] * e0y, gda[0] * e1x + gda[2] * e1y, gda[1] * e1x + gda[3] * e1y]
        else:
            lk.scatter(G_tex, S_tex, g, rows)
            gtu, gtv = lk.backward(g)
            gdb = None
        gu = gtu * (q[0][0] - q[2][0]) + gtv * (q[0][1] - q[2][1])
        gv = gtu * (q[1][0] - q[2][0]) + gtv * (q[1][1] - q[2][1])
        nine = _uv_bwd(px, gu, gv, gdb)
        for k in range(3):
            for c3, colm in enumerate((0, 1, 3)):
                G_pos[:, colm].index_add_(0, px.rows[k][rows], nine[3 * k + c3].v[rows])
                S_pos[:, colm].index_add_(0, px.rows[k][rows], nine[3 * k + c3].S[rows])

    chain(gq, every)                                                            # k_shade: the un-antialiased gradient of every covered pixel

    # ---- k_fix<0>: the blend of every covered receiver ----
    pr = D.pairs
    E = AR._edges(pr, D.pos3, inp['tri'], dtype)
    ei, ee, er, eo = D.ei, D.ee, D.er, D.eo
    t = Q(E['t'].v[ei, ee], E['t'].S[ei, ee])
    amt = _where(D.efar, t - 0.5, 0.5 - t)
    rc = cov[er]                                                                # entries whose receiver is covered: the others change nothing
    colP = []
    for c in range(C):
        v, S = lk0.col[c].v.expand(P).clone(), lk0.col[c].S.expand(P).clone()
        v[pix], S[pix] = lk.col[c].v, lk.col[c].S
        colP.append(Q(v, S))
    hit = torch.unique(er[rc])
    hrow = rowof[hit]
    dn, gaa = [], []
    if wg is not None:
        wh = _at(w, hrow)
        if MUTANT == 'partner_weight_in_k_fix0':      # the weight of (one of) the receiver's partners, an empty one's being its w0
            wp = torch.where(cov, wg.w, wg.w0)
            wp[er[rc]] = torch.where(cov, wg.w, wg.w0)[eo[rc]]
            wh = _coef(wp[hit])
    for c in range(C):
        delta = _at(amt, rc) * (_at(colP[c], eo[rc]) - _at(colP[c], er[rc]))
        av, aS = torch.zeros(P, dtype=dtype), torch.zeros(P, dtype=dtype)
        av.index_add_(0, er[rc], delta.v)
        aS.index_add_(0, er[rc], delta.S)
        acc = Q(av[hit], aS[hit]) + _at(lk.col[c], hrow)
        dn.append(_at(rf, hrow) - acc * CS_SCALE)
        gv_, gS_ = torch.zeros(P, dtype=dtype), torch.zeros(P, dtype=dtype)
        gv_[pix], gS_[pix] = gq[c].v, gq[c].S
        g_hit = Kq * dn[c] if wg is None else Kq * (wh * wg.psi(dn[c]))
        gv_[hit], gS_[hit] = g_hit.v, g_hit.S
        gaa.append(Q(gv_, gS_))

    # ---- k_fix<1>: the difference, d alpha / d pos, the empty pixels' share ----
    both = rc & cov[eo]
    hit2 = torch.unique(torch.cat([er[rc], eo[both]]))
    h2row = rowof[hit2]
    dl, esum = [], []
    for c in range(C):
        term = _at(amt, rc) * _at(gaa[c], er[rc])
        gov, goS = torch.zeros(P, dtype=dtype), torch.zeros(P, dtype=dtype)
        gov.index_add_(0, er[rc], -term.v)
        goS.index_add_(0, er[rc], term.S)
        if MUTANT != 'partner_gradient_dropped':
            o_cov = cov[eo[rc]]
            gov.index_add_(0, eo[rc][o_cov], term.v[o_cov])
            goS.index_add_(0, eo[rc][o_cov], term.S[o_cov])
        go = Q(gov[hit2], goS[hit2]) + _at(gaa[c], hit2)
        d = go - _at(gq[c], h2row)
        if MUTANT == 'unweighted_gq_taken_away_in_k_fix1' and wg is not None:
            d = go - Kq * wg.psi(_at(dd[c], h2row))
        if MUTANT == 'difference_term_sign_flipped':
            d = -d
        if MUTANT == 'difference_term_dropped':
            d = d * 0.0
        full = _zeros(n, dtype)
        full.v[h2row], full.S[h2row] = d.v, d.S
        dl.append(full)
        empty_o = ~cov[eo[rc]]
        esum.append(Q(term.v[empty_o].sum(), term.S[empty_o].sum()))
    n_esum = int((rc & ~cov[eo]).sum())
    chain(dl, h2row)
    if n_esum and MUTANT != 'no_esum_share':
        one = torch.zeros(1, dtype=torch.int64)
        lk0.scatter(G_tex, S_tex, [Q(e.v.reshape(1), e.S.reshape(1)) for e in esum], one)
    col_img = torch.stack([q.v for q in colP], 1)
    rows_a, rows_b, ta, tb, keep = _edge_pos_terms(D, E, colP, gaa, dtype)
    for rows, three in ((rows_a, ta), (rows_b, tb)):
        for colm, q in zip((0, 1, 3), three):
            G_pos[:, colm].index_add_(0, rows[keep], q.v[keep])
            S_pos[:, colm].index_add_(0, rows[rc], q.S[rc])
            if MUTANT == 'd_alpha_counted_by_both_pixels':
                G_pos[:, colm].index_add_(0, rows[keep & both], q.v[keep & both])
    levels = None
    if mip:      # _fold_mip_grads: level 0's gradient plus the box filter's backward of every coarser level; the scales fold alike
        levels = [(g.reshape(h, w, C), s.reshape(h, w, C)) for g, s, (h, w) in zip(L_tex, LS_tex, lk.dims)]
        G_tex, S_tex = fold_levels([g for g, _ in levels]).reshape(-1), fold_levels([s for _, s in levels], scale=True).reshape(-1)
    # ---- the value ----
    tv_, tS_ = torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype)
    d0h = _at(d0, hrow)
    for c in range(C if wg is not None else 0):      # the weighted call: the same two sums, every term with its weight
        rho_dd = wg.rho(dd[c])
        plain = w * rho_dd - w0rho
        tv_ = tv_ + plain.v.sum()
        tS_ = tS_ + (plain.S + (w * rho_dd).v.abs() + w0rho.v.abs()).sum()
        w_h, w0rho_h, rho_ddh, rho_dn = _at(w, hrow), _at(w0rho, hrow), _at(rho_dd, hrow), wg.rho(dn[c])
        corr = (w_h * rho_dn - w0rho_h) - (w_h * rho_ddh - w0rho_h)
        tv_ = tv_ + corr.v.sum()
        tS_ = tS_ + (corr.S + (w_h * rho_dn).v.abs() + (w_h * rho_ddh).v.abs() + 2.0 * w0rho_h.v.abs()).sum()
    for c in range(C if wg is None else 0):
        plain = dd[c] * dd[c] if MUTANT == 'background_share_for_covered_pixels_too' else dd[c] * dd[c] - d0 * d0
        tv_ = tv_ + plain.v.sum()
        tS_ = tS_ + (plain.S + (dd[c].v * dd[c].v).abs() + d0.v * d0.v).sum()
        ddh = _at(dd[c], hrow)
        corr = dn[c] * dn[c] - d0h * d0h
        if MUTANT != 'hit_pixel_added_without_removing_the_plain_term':
            corr = corr - (ddh * ddh - d0h * d0h)
        tv_ = tv_ + corr.v.sum()
        tS_ = tS_ + (corr.S + dn[c].v * dn[c].v + ddh.v * ddh.v + 2.0 * d0h.v * d0h.v).sum()
    b = float(np.float32(float(inp.get('background', BACKGROUND)) * 255.0))      # what reference_background_sumsq hands fpcdr_ref_bg_sumsq
    bg_v, bg_S = bg_sumsq(inp['ref_u8'], b, dtype)
    extra = {}
    if wg is not None:      # fpcdr_ref_bg_wsum: w0 rho(d0) and w0 over ALL pixels; the covered pixels' w - w0 from k_shade's wsum slots
        d0_all = _inp(rf_all) - Q(torch.tensor(b, dtype=dtype).expand(P), torch.tensor(b, dtype=dtype).abs().expand(P))
        w0_bg = wg.w0
        if MUTANT == 'background_share_weighted_by_w':
            w0_bg = torch.where(cov, wg.w, wg.w0)
        share = _coef(w0_bg) * wg.rho(d0_all)
        bg_v, bg_S = share.v.reshape(B, -1).sum(dim=1), share.S.reshape(B, -1).sum(dim=1)      # (per image, as bg_sumsq sums)
        covered = w.v if MUTANT == 'wsum_without_minus_w0' else w.v - w0.v
        extra = {'wsum': (float(C) * wg.w0.sum() + float(C) * covered.sum(), float(C) * wg.w0.sum() + float(C) * (w.v + w0.v).sum()),
                 'w': w.v, 'w0': w0.v}
    value = (tv_ + float(C) * bg_v.sum()) / float(n_total)
    value_S = (tS_ + float(C) * bg_S.sum()) / float(n_total)
    return {**extra, 'value': (value, value_S), 'g_pos': (G_pos.reshape(B, px.V, 4), S_pos.reshape(B, px.V, 4)),
            'g_tex': (G_tex.reshape(Ht, Wt, C), S_tex.reshape(Ht, Wt, C)), 'st': st, 'D': D, 'E': E, 'hit': hit, 'hit2': hit2, 'pix': pix,
            'cov': cov, 'rowof': rowof, 'gq': torch.stack([q.v for q in gq], 1), 'dd': torch.stack([q.v for q in dd], 1),
            'dn': torch.stack([q.v for q in dn], 1) if hit.numel() else torch.zeros(0, C, dtype=dtype), 'n_esum': n_esum, 'col': col_img,
            'bgs': float(bgs), 'b': b, 'n_total': n_total, 'levels': levels}


# ---------------------------------------------------------------------------------------------------------------------
# margins, zeros, the kernel-order statement
# ---------------------------------------------------------------------------------------------------------------------

def _margins_of(st, D, E64):
    m = torch.full((st.px.n,), float('inf'), dtype=torch.float64)
    for q in st.px.gates():
        m = torch.minimum(m, torch.nan_to_num(q.v.abs() / (U * q.S), nan=0.0))
    for q in st.lk.gates:
        m = torch.minimum(m, torch.where(q.S > 0, q.v / (U * q.S), torch.where(q.v > 0, torch.full_like(q.v, float('inf')), torch.zeros_like(q.v))))
    sil = torch.where(D.pairs.analysed, D.sil_margin, torch.full_like(D.sil_margin, float('inf')))
    return {'pixel': m, 'edge': AR.edge_margins(D, E64) if D.pairs.n else torch.zeros(0, 3, dtype=torch.float64), 'sil': sil, 'z': D.pairs.zm}


def margins(inp, r=None):
    """How far every float32 choice is from flipping, in units of u of its own scale, on the float64 evaluation r -> dict:
    'pixel' [n] (barycentric gates, floor(tu), the clamp of tu, the tap cells), 'edge' [pairs,3], 'sil' [B,T] (inf where no pair analyses the
    triangle), 'z' [pairs]."""
    r = r or evaluate(inp)
    return _margins_of(r['st'], r['D'], r['E'])


def decision_margin(inp, r=None):
    return min([float('inf')] + [float(v.min()) for v in margins(inp, r).values() if v.numel()])


def _structure(inp):
    """From the choices alone: reach [Ht*Wt] bool (texels some term reaches), rows [B*V] bool (vertices with a term), the per-texel count of
    plain terms and whether the empty pixels' share exists."""
    ch = choices(inp)
    st = _forward(inp, torch.float32, ch)
    px, lk, lk0, D = st.px, st.lk, st.lk0, ch['D']
    B, (H, W) = px.B, inp['res']
    Ht, Wt, C = inp['tex'].shape
    pix = (px.bi * H + px.yy) * W + px.xx
    cov = torch.zeros(B * H * W, dtype=torch.bool)
    cov[pix] = True
    level_count = None
    rc = cov[D.er]
    has = None
    if inp.get('weights') is not None:
        # the weighted call: entries with a weight-0 receiver have no term, and a pixel has one (`has`) when its weight is positive or it is
        # the partner of an entry that has (module docstring); w > 0 is a matter of integers and of the face weights' zeros
        wpos = _Weights(inp, torch.float32).w > 0
        rc = rc & wpos[D.er]
        has_all = wpos.clone()
        has_all[D.eo[rc & cov[D.eo]]] = True
        has = has_all[pix]
    if st.mip is None:
        count = torch.zeros(Ht * Wt, dtype=torch.int64)
        for k in range(4):
            ok = lk.valid[k] if has is None else lk.valid[k] & has
            count.index_add_(0, lk.flat[k][ok], torch.ones(int(ok.sum()), dtype=torch.int64))
        anyv = lk.valid[0] | lk.valid[1] | lk.valid[2] | lk.valid[3]
    else:      # the taps of every level, folded: a coarse texel's terms reach its four fine ones
        level_count = lk.level_reach()
        count = fold_levels([c.reshape(h, w) for c, (h, w) in zip(level_count, lk.dims)], scale=None).reshape(-1)
        anyv = lk.any_valid()
    n_esum = int((rc & ~cov[D.eo]).sum())
    reach = count > 0
    if n_esum:
        for k in range(4):
            reach[lk0.flat[k][lk0.valid[k]]] = True
    term = (ch['open0'] | ch['open1']) & ((lk.mu != 0) | (lk.mv != 0)) & anyv
    if has is not None:
        term = term & has
    off_centre = (px.fx.v != 0) | (px.fy.v != 0)      # (the w column's term is -fx g_x - fy g_y: none at the image's centre)
    if st.mip is not None:      # the footprint's gradient reaches x, y and w of all three vertices wherever the level's gate is open
        through_level = lk.passes & anyv
        term, off_centre = term | through_level, off_centre | through_level
    rows, rows_w = torch.zeros(B * px.V, dtype=torch.bool), torch.zeros(B * px.V, dtype=torch.bool)
    for k in range(3):
        rows[px.rows[k][term]] = True
        rows_w[px.rows[k][term & off_centre]] = True
    # an edge entry has a term when its receiver is covered and one of its two colours is not the exact 0 of zero-mode padding
    live = torch.full((B * H * W,), bool((lk0.valid[0] | lk0.valid[1] | lk0.valid[2] | lk0.valid[3]).any()))
    live[pix] = anyv
    ent = rc & (live[D.pairs.pP[D.ei]] | live[D.pairs.pQ[D.ei]])
    base = D.pairs.b[D.ei] * D.V
    for r_ in (rows, rows_w):
        r_[(base + D.E['va'][D.ei, D.ee])[ent]] = True
        r_[(base + D.E['vb'][D.ei, D.ee])[ent]] = True
    return dict(reach=reach, rows=rows, rows_w=rows_w, count=count, n_esum=n_esum, cov=cov, pix=pix, st=st, D=D, level_count=level_count, has=has)


def predicted_zeros(inp):
    """The entries without any term, from ids and float32 choices alone, never from values -> dict: 'g_tex' [Ht,Wt,C] bool (texels no tap
    of a covered pixel and no share of the empty pixels reaches), 'g_pos' [B,V,4] bool (the z column; vertices of triangles no pixel shows
    or whose pixels all have both clamp gates closed or mu = mv = 0, and of no active edge with a covered receiver: an image wholly behind
    the camera has every row)."""
    s = _structure(inp)
    Ht, Wt, C = inp['tex'].shape
    B, V = inp['pos'].shape[:2]
    zp = (~s['rows']).reshape(B, V, 1).expand(B, V, 4).clone()
    zp[..., 2] = True
    zp[..., 3] = ~s['rows_w'].reshape(B, V)
    return {'g_tex': (~s['reach']).reshape(Ht, Wt, 1).expand(Ht, Wt, C).clone(), 'g_pos': zp}


def float32_in_kernel_order(inp):
    """The per-pixel float32 statement, one rounding per operation, in the kernels' order -> dict: 'r' (evaluate(inp, float32)), 'texel'
    [m] flat indices of the texels that hold exactly one plain term, of a pixel outside every blend, and no share of the empty pixels, and
    'g_tex' [m,C] the float32 product gq * w_k there; 'gq_w' [n,4,C] all the products.  Cached for a case's inputs: treat as read-only."""
    if _case_cache.get(inp.get('name')) is inp and MUTANT is None:
        return (_kernel_order_cached_weighted if 'base' in inp else _kernel_order_cached)(inp['name'])
    return _kernel_order(inp)


@functools.lru_cache(maxsize=None)
def _kernel_order_cached(name):
    return _kernel_order(_case_cache[name])


@functools.lru_cache(maxsize=4)      # (with_weights: see _reference_cached_weighted)
def _kernel_order_cached_weighted(name):
    return _kernel_order(_case_cache[name])


def _kernel_order(inp):
    r = reference(inp, torch.float32)
    if r['st'].mip is not None:      # (the mip call's one-term texels are held through `mip/magnified/C1/wrap`, on the non-mip statement)
        C = inp['tex'].shape[2]
        return {'r': r, 'texel': torch.zeros(0, dtype=torch.int64), 'g_tex': torch.zeros(0, C), 'gq_w': None}
    s = _structure(inp)
    lk, C = r['st'].lk, inp['tex'].shape[2]
    n = r['st'].px.n
    prod = torch.stack([torch.stack([r['gq'][:, c] * lk.wk[k].v for c in range(C)], 1) for k in range(4)], 1)      # [n,4,C]
    in_blend = torch.zeros(n, dtype=torch.bool)
    in_blend[r['rowof'][r['hit2']]] = True
    single = s['count'] == 1
    if s['n_esum']:
        for k in range(4):
            single[r['st'].lk0.flat[k][r['st'].lk0.valid[k]]] = False
    texel, val = [], []
    for k in range(4):
        ok = lk.valid[k] & single[lk.flat[k]] & ~in_blend
        if s['has'] is not None:      # (the weighted call: the one term is a pixel's that has one -- gq = (-2 cs gs) (w psi) in float32)
            ok = ok & s['has']
        texel.append(lk.flat[k][ok])
        val.append(prod[ok, k])
    return {'r': r, 'texel': torch.cat(texel), 'g_tex': torch.cat(val), 'gq_w': prod}


# ---------------------------------------------------------------------------------------------------------------------
# plan: where k_shade places its windows, which tables overflow
# ---------------------------------------------------------------------------------------------------------------------

def _window(x0, y0, Ht, Wt, cells, boundary):
    """setup_window on the taps (x0, y0) the first pass kept -> dict ox, oy, ows, owr, owrap, centred, fits (None without a tap)."""
    if x0.numel() == 0:
        return None
    xa, xb, ya, yb = int(x0.min()), int(x0.max()), int(y0.min()), int(y0.max())
    centred = False
    if boundary == 'wrap' and (xb - xa >= (Wt >> 1) or yb - ya >= (Ht >> 1)):
        cx, cy = torch.where(x0 >= (Wt >> 1), x0 - Wt, x0), torch.where(y0 >= (Ht >> 1), y0 - Ht, y0)
        xa2, xb2, ya2, yb2 = int(cx.min()), int(cx.max()), int(cy.min()), int(cy.max())
        if xb2 - xa2 < xb - xa:
            xa, xb, centred = xa2, xb2, True
        if yb2 - ya2 < yb - ya:
            ya, yb, centred = ya2, yb2, True
    nw, nh = xb - xa + 2, yb - ya + 2
    sx0, sy0 = xa, ya
    fits = nw * nh <= cells
    if fits:
        stride = nw
        rows = cells // stride
        sy0 -= (rows - nh) >> 1
    else:
        f = np.float32
        aspect = min(max(f(nw) / f(nh), f(1.0) / f(cells)), f(cells))
        stride = min(max(int(np.sqrt(f(f(cells) * aspect))), 2), cells // 2)
        rows = cells // stride
        sx0 += (nw - stride) >> 1
        sy0 += (nh - rows) >> 1
    owrap = sx0 < 0 or sy0 < 0 or sx0 + stride > Wt or sy0 + rows > Ht
    return dict(ox=sx0, oy=sy0, ows=stride, owr=rows, owrap=owrap, centred=centred, fits=fits, box=(nw, nh))


MIP_WIN_CELLS = {1: (2304, 704, 256), 3: (1088, 384, 128), 4: (1088, 384, 128)}      # MipWinCaps<CS>
MIP_PASS0_ROWS = (0, 1, 10, 11, 20, 21, 30, 31)      # shade_row_pair(0, wave): row pairs 0, 5, 10, 15 of the WHOLE bin


def _mip_place(ua, ub, va, vb, wl, hl, cap):
    """place() of shade_body's prepass for one level of wl x hl texels: the window (x, y, stride, rows) and whether it fits."""
    f = np.float32
    big = f(1073741824.0)
    fl_ = lambda t, n: int(min(max(np.floor(f(f(t) * f(n)) - f(0.5)), -big), big))
    xa, ya = fl_(ua, wl) - 1, fl_(va, hl) - 1
    nw, nh = fl_(ub, wl) + 2 - xa + 1, fl_(vb, hl) + 2 - ya + 1
    fits = nw * nh <= cap
    if fits:
        stride = nw
        rows = cap // stride
        ya -= (rows - nh) >> 1
    else:
        aspect = min(max(f(nw) / f(nh), f(1.0) / f(cap)), f(cap))
        stride = min(max(int(np.sqrt(f(f(cap) * aspect))), 2), cap // 2)
        rows = cap // stride
        xa += (nw - stride) >> 1
        ya += (nh - rows) >> 1
    return dict(x=xa, y=ya, s=stride, r=rows, fits=fits, box=(nw, nh))


def _plan_mip_bin(st, m, by, boundary, C):
    """The prepass, place() and the routing of one bin (pixels m of the float32 forward st) -> dict: mlb (None: no pass-0 pixel, no window),
    windows (three dicts or None), wrap (w0wrap, w1wrap, w2wrap), shifted (the half-period view taken for u, for v),
    levels {l: [tap sets into a window, tap sets to memory]} over both levels of every pixel, below_mlb (pixels with l0 < mlb)."""
    px, lk = st.px, st.lk
    f32 = torch.float32
    Ht, Wt, nl = lk.Ht, lk.Wt, lk.nl
    prep = lambda t: t - torch.floor(t) if boundary == 'wrap' else (t.clamp(0.0, 1.0) if boundary == 'clamp' else t)
    pu, pv = prep(st.tu.v.to(f32)), prep(st.tv.v.to(f32))
    zy = px.yy - by * BIN
    p0 = m & torch.isin(zy, torch.tensor(MIP_PASS0_ROWS))
    out = dict(mlb=None, windows=[None, None, None], wrap=[False, False, False], shifted=(False, False), levels={}, below_mlb=0)
    wins = [None, None, None]
    if bool(p0.any()):
        mlb = int(lk.l0[p0].min())
        ua, ub, va, vb = float(pu[p0].min()), float(pu[p0].max()), float(pv[p0].min()), float(pv[p0].max())
        su_, sv_ = False, False
        if boundary == 'wrap':
            half = lambda t: (t + 0.5) - torch.floor(t + 0.5)
            su, sv = half(pu[p0]), half(pv[p0])
            ua2, ub2, va2, vb2 = float(su.min()), float(su.max()), float(sv.min()), float(sv.max())
            f = np.float32
            if f(ub2) - f(ua2) < f(ub) - f(ua):
                ua, ub, su_ = float(f(ua2) - f(0.5)), float(f(ub2) - f(0.5)), True
            if f(vb2) - f(va2) < f(vb) - f(va):
                va, vb, sv_ = float(f(va2) - f(0.5)), float(f(vb2) - f(0.5)), True
        for j in range(3):
            l = mlb + j
            if l <= nl:
                wins[j] = _mip_place(ua, ub, va, vb, Wt >> l, Ht >> l, MIP_WIN_CELLS[C][j])
        wrap = [w is not None and (w['x'] < 0 or w['y'] < 0 or w['x'] + w['s'] > (Wt >> (mlb + j)) or w['y'] + w['r'] > (Ht >> (mlb + j)))
                for j, w in enumerate(wins)]
        out.update(mlb=mlb, windows=wins, wrap=wrap, shifted=(su_, sv_), below_mlb=int((lk.l0[m] < mlb).sum()))
    wc = lambda d, n: torch.where(d < 0, d + n, torch.where(d >= n, d - n, d))
    for which, lev, live in ((0, lk.l0, torch.ones_like(m)), (1, lk.l1, lk.passes)):      # (an upper level with fl = 0 scatters nothing)
        for l in torch.unique(lev[m & live]).tolist():
            sel = m & live & (lev == l)
            inside = torch.zeros_like(sel)
            j = None if out['mlb'] is None else l - out['mlb']
            if j is not None and 0 <= j <= 2 and wins[j] is not None:
                w = wins[j]
                lx = torch.floor(pu * float(Wt >> l) - 0.5).long() - w['x']
                ly = torch.floor(pv * float(Ht >> l) - 0.5).long() - w['y']
                if boundary == 'wrap' and out['wrap'][j]:
                    lx, ly = wc(lx, Wt >> l), wc(ly, Ht >> l)
                inside = sel & (lx >= 0) & (lx < w['s'] - 1) & (ly >= 0) & (ly < w['r'] - 1)
            acc = out['levels'].setdefault(l, [0, 0])
            acc[0] += int(inside.sum())
            acc[1] += int((sel & ~inside).sum())
    return out


def plan(inp):
    """In integers, per occupied bin (b, by, bx) and half, what k_shade and k_fix do with the call -> dict:
    'halves': {(b, by, bx, half): window dict + 'inside' / 'outside' (pixels whose four adds go into the window / to memory)},
    'bins': {(b, by, bx): dict vertices (distinct, of the pixels with a gradient: against VT_SLOTS), deferred, hit, hit_vertices (against FVS),
    hit_texels (against FTS), sil (a silhouette bit in the plane or its apron: the bin takes a record slot)},
    'pairs': blended pairs, 'cross': those across a bin border, 'empty_partner': entries with a covered receiver and an empty partner,
    'image_border': blended pairs with a pixel on the image's border, 'max_deferred': the most deferred pixels of a bin."""
    s = _structure(inp)
    st, D = s['st'], s['D']
    px, lk = st.px, st.lk
    B, (H, W) = px.B, inp['res']
    Ht, Wt, C = inp['tex'].shape
    cells, bd = OWIN_CELLS[C], inp['boundary']
    ids = inp['ids'].detach().cpu().long()
    sil = D.sil                                                        # [B,T]
    silpix = torch.zeros(B, H, W, dtype=torch.int64)
    silpix[px.bi, px.yy, px.xx] = sil[px.bi, px.t]
    code = ids | (silpix << 24)
    # deferred: pair_maybe with an in-image neighbour
    pad = torch.zeros(B, H + 2, W + 2, dtype=torch.int64)
    pad[:, 1:-1, 1:-1] = code
    inimg = torch.zeros(B, H + 2, W + 2, dtype=torch.bool)
    inimg[:, 1:-1, 1:-1] = True
    deferred = torch.zeros(B, H, W, dtype=torch.bool)
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        nb = pad[:, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        ok = inimg[:, 1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        deferred |= ok & (((code ^ nb) & 0xffffff) != 0) & (((code | nb) >> 24) != 0)
    deferred &= ids > 0
    rc = s['cov'][D.er]
    hit2 = torch.zeros(B * H * W, dtype=torch.bool)
    hit2[D.er[rc]] = True
    hit2[D.eo[rc & s['cov'][D.eo]]] = True
    hit2 = hit2.reshape(B, H, W)
    key = (px.bi * 1000 + px.yy // BIN) * 1000 + px.xx // BIN
    halves, bins, mipbins = {}, {}, {}
    is_hit = hit2[px.bi, px.yy, px.xx]
    ent_bin = lambda p: ((p // (H * W)) * 1000 + ((p // W) % H) // BIN) * 1000 + (p % W) // BIN
    for k in torch.unique(key).tolist():
        b, by, bx = k // 1000000, (k // 1000) % 1000, k % 1000
        m = key == k
        if st.mip is not None:
            mipbins[(b, by, bx)] = _plan_mip_bin(st, m, by, bd, C)
        for half in ((0, 1) if st.mip is None else ()):
            zy = px.yy - by * BIN
            mh = m & (zy // 16 == half)
            if not bool(mh.any()):
                continue
            first = mh & torch.isin(zy % 16, torch.tensor(PASS0_ROWS))
            w = _window(lk.x0[first], lk.y0[first], Ht, Wt, cells, bd)
            if w is None:
                w = dict(ox=0, oy=0, ows=1, owr=1, owrap=False, centred=False, fits=True, box=(0, 0))
            lx, ly = lk.x0[mh] - w['ox'], lk.y0[mh] - w['oy']
            if bd == 'wrap' and w['owrap']:
                wc = lambda d, n: torch.where(d < 0, d + n, torch.where(d >= n, d - n, d))
                lx, ly = wc(lx, Wt), wc(ly, Ht)
            inside = (lx >= 0) & (lx < w['ows'] - 1) & (ly >= 0) & (ly < w['owr'] - 1)
            halves[(b, by, bx, half)] = dict(w, inside=int(inside.sum()), outside=int((~inside).sum()))
        y0, x0 = by * BIN, bx * BIN
        apron = code[b, max(y0 - 1, 0):y0 + BIN + 1, max(x0 - 1, 0):x0 + BIN + 1]
        apron = apron.clone()
        # (the four corners of the apron are not loaded)
        sub = torch.zeros_like(apron, dtype=torch.bool)
        ys, xs = max(y0 - 1, 0), max(x0 - 1, 0)
        sub[(y0 - ys):(y0 - ys) + BIN, :] = True
        sub[:, (x0 - xs):(x0 - xs) + BIN] = True
        mhit = m & is_hit
        ent = rc & ((ent_bin(D.pairs.pP[D.ei]) == k) | (ent_bin(D.pairs.pQ[D.ei]) == k))
        ent_first = rc & (ent_bin(torch.where(s['cov'][D.pairs.p0[D.ei]], D.pairs.p0[D.ei], D.pairs.p1[D.ei])) == k)
        hv = torch.cat([px.vi[mhit].reshape(-1), D.E['va'][D.ei, D.ee][ent_first], D.E['vb'][D.ei, D.ee][ent_first]])
        bins[(b, by, bx)] = dict(
            vertices=int(torch.unique(px.vi[m].reshape(-1)).numel()), deferred=int(deferred[b, y0:y0 + BIN, x0:x0 + BIN].sum()),
            hit=int(mhit.sum()), hit_vertices=int(torch.unique(hv).numel()),
            hit_texels=0 if st.mip is not None else int(torch.unique(torch.cat([lk.flat[t][mhit & lk.valid[t]] for t in range(4)])).numel()),
            sil=bool((((apron >> 24) != 0) & sub).any()), entries=int(ent.sum()))
    pr = D.pairs
    blended = D.active.any(1)
    p0, p1 = pr.p0[blended], pr.p1[blended]
    on_border = lambda p: ((p % W) == 0) | ((p % W) == W - 1) | (((p // W) % H) == 0) | (((p // W) % H) == H - 1)
    return dict(halves=halves, bins=bins, mipbins=mipbins, pairs=int(blended.sum()), cross=int((ent_bin(p0) != ent_bin(p1)).sum()),
                cross_x31=int(((pr.x0[blended] % BIN == BIN - 1) & (pr.d[blended] == 0)).sum()),
                cross_y31=int(((pr.y0[blended] % BIN == BIN - 1) & (pr.d[blended] == 1)).sum()),
                empty_partner=s['n_esum'], image_border=int((on_border(p0) | on_border(p1)).sum()),
                max_deferred=max([v['deferred'] for v in bins.values()] + [0]), deferred=int(deferred.sum()), hit=int(hit2.sum()),
                code=code)


def id_planes(inp):
    """The id planes the call leaves (include/fpcdr.h): (triangle + 1) | silhouette bits << 24 per pixel -> [B,H,W] int64."""
    if _case_cache.get(inp.get('name')) is inp and 'base' in inp:      # (with_weights: the planes are the case's own)
        return _id_planes_cached(inp['base'])
    return plan(inp)['code']


@functools.lru_cache(maxsize=None)
def _id_planes_cached(name):
    return plan(_case_cache[name])['code']


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_objective_ref.py
# ---------------------------------------------------------------------------------------------------------------------

def _unsafe(inp, shared=False):
    """-> (rows of pos.reshape(-1, 4), rows of uv) of every triangle with a choice closer than SETTLE_MARGIN.  Unshared triangles move
    whole, with their three texture coordinates.  shared (a mesh): a tap too close to a cell border moves the texture coordinate of ONE
    corner, the one the pixel weighs most, and leaves the geometry -- a vertex re-draws its whole fan."""
    ch = {}
    _forward(inp, torch.float32, ch)
    try:
        st = _forward(inp, torch.float64, ch)
    except AssertionError:      # (a gate that float32 and float64 decide differently: closer than any margin)
        st = _forward(inp, torch.float64, {})
    D = ch['D']
    E64 = AR._edges(D.pairs, D.pos3, inp['tri'], torch.float64)
    px = st.px
    geo, tap = torch.zeros(px.n, dtype=torch.bool), torch.zeros(px.n, dtype=torch.bool)
    for q in px.gates():
        geo |= ~(q.v.abs() > SETTLE_MARGIN * U * q.S)
    for q in st.lk.gates:
        tap |= ~(q.v > SETTLE_MARGIN * U * q.S)
        geo |= SETTLE_MARGIN * U * q.S > 0.25      # (a triangle seen edge-on: a scale no fraction is safe at; the triangle moves)
    if not shared:
        geo |= tap
    rows = torch.unique(torch.cat([px.rows[k][geo] for k in range(3)] + [AR._unsafe_rows(D, E64)]))
    tap &= ~geo
    u, v = px.uvz[0].v[tap], px.uvz[1].v[tap]
    corner = torch.stack([u, v, 1.0 - u - v], 1).argmax(1)
    return rows, torch.unique(torch.cat([inp['uv_tri'].long()[px.t[geo]].reshape(-1), inp['uv_tri'].long()[px.t[tap], corner]]))


def _settle(g, ids_of, gen, rounds=200):
    """Move (by up to 0.05 pixel a round) the vertices of every triangle with a choice too close, and its texture coordinates, until none
    is.  g: dict X [B,V,2], z, w [B,V] float64, uv [Vt,2] float64 (or uv_fn(X, off) with off [T,2], the per-triangle offsets that are
    drawn again instead) and the rest of the inputs -> the inputs."""
    H, W = g['res']
    kept, fewest = None, None
    for _ in range(rounds):
        pos = _clip(g['X'], g['z'], g['w'], H, W)
        uv = g['uv_fn'](g['X'], g['off']) if 'uv_fn' in g else g['uv']
        inp = dict(pos=pos, tri=g['tri'], ids=ids_of(pos, g['tri']), res=g['res'], uv=uv.float().contiguous(), uv_tri=g['uv_tri'], tex=g['tex'],
                   ref_u8=g['ref_u8'], boundary=g['boundary'], mip_levels=g.get('mip_levels'))
        shared = bool(g.get('shared'))
        rows, uvr = _unsafe(inp, shared)
        if rows.numel() == 0 and uvr.numel() == 0:
            return inp
        # (shared vertices: a move that leaves more to move than the state it started from is taken back)
        if shared and fewest is not None and rows.numel() + uvr.numel() > fewest:
            g['X'], g['uv'], g['off'], rows, uvr = kept[0].clone(), None if kept[1] is None else kept[1].clone(), \
                None if kept[2] is None else kept[2].clone(), kept[3], kept[4]
        else:
            fewest = rows.numel() + uvr.numel()
            kept = (g['X'].clone(), None if g.get('uv') is None else g['uv'].clone(), None if g.get('off') is None else g['off'].clone(), rows, uvr)
        if 'shift' in g:      # every image shows the triangles of the first, a whole number of pixels away
            rows = torch.unique(rows % g['X'].shape[1])
            g['X'][0][rows] += (torch.rand(rows.numel(), 2, generator=gen, dtype=torch.float64) - 0.5) * 0.1
            g['X'] = g['X'][:1] + g['shift']
        else:
            g['X'].reshape(-1, 2)[rows] += (torch.rand(rows.numel(), 2, generator=gen, dtype=torch.float64) - 0.5) * 0.1
        if 'uv_fn' in g:
            tr = torch.unique(uvr // 3)
            g['off'][tr] = g['draw_off'](tr.numel())
        else:
            g['uv'][uvr] += (torch.rand(uvr.numel(), 2, generator=gen, dtype=torch.float64) - 0.5) * (0.05 if shared else 0.004)
    raise AssertionError("the construction does not settle")


def _fat_soup(B, T, gen, H, W, size_px):
    """rasterize_ref._soup_geometry with triangles near equilateral (circumradius 0.7 to 1 size_px, corners within 25 degrees of a regular
    triangle's): a sliver's barycentrics -- and with them its texture coordinate -- have a scale of thousands of u, and no fraction is
    64 of those away from a cell border."""
    rnd = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    centre = torch.stack([rnd(B, T, 1) * (W + 10) - 5, rnd(B, T, 1) * (H + 10) - 5], -1)
    ang = rnd(B, T, 1) * 2 * math.pi + torch.arange(3, dtype=torch.float64) * (2 * math.pi / 3) + (rnd(B, T, 3) - 0.5) * (50 * math.pi / 180)
    rad = size_px * (0.7 + 0.3 * rnd(B, T, 3))
    X = centre + torch.stack([rad * torch.cos(ang), rad * torch.sin(ang)], -1)
    z = rnd(B, T * 3) * 1.8 - 0.9
    w = rnd(B, T * 3) * 2.5 + 0.5
    return X.reshape(B, T * 3, 2), z, w, torch.arange(T * 3, dtype=torch.int32).reshape(T, 3)


def _subdivided(v, tri):
    """Every triangle of a mesh on the unit sphere split in four (midpoints pushed back onto the sphere)."""
    v, mid, out = [tuple(p) for p in v.tolist()], {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            p = np.array(v[a]) + np.array(v[b])
            v.append(tuple(p / np.linalg.norm(p)))
            mid[key] = len(v) - 1
        return mid[key]

    for a, b, c in tri.tolist():
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return torch.tensor(v, dtype=torch.float64), torch.tensor(out, dtype=torch.int32)


def _screen_uv(X, Ht, Wt, tpp, origin=(0.0, 0.0)):
    """Texture coordinates affine in the screen position: tpp texels per pixel along both axes."""
    return torch.stack([(X[..., 0] - origin[0]) * tpp / Wt, (X[..., 1] - origin[1]) * tpp / Ht], -1)


ISLANDS = [[(6.3, 5.2), (17.8, 8.1), (9.4, 19.7)], [(40.2, 4.4), (58.9, 12.3), (44.1, 17.6)], [(8.8, 30.3), (21.2, 41.7), (5.1, 40.2)],
           [(36.4, 27.9), (62.3, 33.2), (49.7, 43.1)], [(26.1, 18.2), (32.7, 21.9), (28.3, 27.4)]]
TINY = {'1x1': ((1, 1), [(-1.0, -1.0), (3.0, -1.0), (0.0, 3.0)]), '1x2': ((1, 2), [(0.2, -1.0), (1.2, 0.4), (0.1, 2.0)]),
        '2x1': ((2, 1), [(-1.0, 0.1), (2.0, 0.2), (0.4, 1.2)])}


# right edges between the pixel centres of columns 31 | 32 and 63 | 64 (the one-pixel partial bin column), a bottom edge between rows 31 | 32
BORDER_TRIS = [[(20.0, 9.0), (31.9, 3.2), (31.95, 21.0)], [(52.0, 8.0), (63.9, 2.4), (63.95, 24.0)], [(40.0, 20.0), (58.0, 31.9), (41.0, 31.95)]]


def _case(name, why, geom, C, boundary, tex_hw, res=(45, 70), B=2, **kw):
    return dict(dict(name=name, why=why, geom=geom, C=C, boundary=boundary, tex_hw=tex_hw, res=res, B=B), **kw)


def _cases():
    out = []
    c = lambda *a, **kw: out.append(_case(*a, **kw))
    c('magnified/C1/wrap', 'k_shade_list<1, WRAP>; 3 texels a pixel: one term per texel, the aspect window, taps inside and outside it',
      'soup', 1, 'wrap', (256, 256), n_tri=36, size=14.0, tpp=3.0, affine=True)      # (256: 70 pixels of 3 texels lap a 128-texel row, and
    #                                        the taps {3 p, 3 p + 1} of column p would meet those of column p + 43 at 3 * 43 = 129 = 128 + 1)
    c('soup/C1/wrap/seam', 'a 24 x 16 texture at half a texel a pixel over several periods: the centred view, owrap, many terms per texel',
      'soup', 1, 'wrap', (16, 24), n_tri=60, size=10.0, tpp=0.5)
    c('soup/C3/clamp', 'k_shade_list<3, -1>, 1600 cells; uv beyond [0, 1]: mu / mv = 0', 'soup', 3, 'clamp', (12, 20), n_tri=60, size=10.0, span=1.6)
    c('soup/C4/zero', 'k_shade_list<4, -1>; taps with two, three and four corners in the padding', 'soup', 4, 'zero', (10, 14), n_tri=60, size=10.0, span=1.6)
    c('mesh/B3', 'a closed mesh in three poses, the third behind the camera: shared vertices, folds, bins without a silhouette', 'mesh', 3, 'wrap',
      (4, 4), res=(96, 96), B=3)
    c('confetti', 'over 256 vertices in a bin, over 64 vertices and 128 texels among its blended pixels: all three tables go to memory', 'confetti', 1,
      'wrap', (16, 16), n_tri=700, size=3.2)
    for bd, C in (('wrap', 1), ('clamp', 3), ('zero', 4)):
        c(f'islands/{bd}', 'separated triangles on an empty frame: every blend has an empty partner; uv away from the taps of (0, 0)', 'islands', C, bd,
          (16, 16))
    c('borders', 'blended pairs across columns and rows 31 | 32 and on the image border at 33 x 65 (one-pixel partial bins)', 'soup', 3, 'wrap', (16, 24),
      res=(33, 65), n_tri=24, size=11.0, tpp=0.5, extra=BORDER_TRIS)
    for k in TINY:
        c(f'tiny/{k}', 'an image of one or two pixels', 'tiny', 3 if k == '1x1' else 1, 'wrap', (8, 8), res=TINY[k][0], B=1, tiny=k)
    return out


CASES = _cases()
CASE_IDS = [c['name'] for c in CASES]
_case_cache = {}


# The mip call (enable_mip=True; tests/test_gpu_objective_mip_ref.py).  Levels settle by construction: within a triangle every vertex has the
# same w, so the uv map is affine in the screen and the level ONE number per triangle, log2 of the major axis of its texels per pixel; the
# minor axis is `aniso` of it (df far from 0: rt is well conditioned) and alternates between u and v from triangle to triangle.  Each
# triangle has its own place in the texture (drawn again when a tap is too close to a cell border), so a bin's pass-0 extent covers much of
# the texture.  The second image shows the first one's triangles (3, -2) pixels away, with another depth order.
# pass-0 rows of a bin are 0, 1, 10, 11, 20, 21, 30, 31: a triangle whose pixel centres lie in rows 3 .. 8 of image 0 (1 .. 6 + 2 of image 1's
# shift: rows 5 .. 8 and 3 .. 6) covers none of them
OFF_PASS0_TRIS = [[(8.0, 4.7), (19.0, 5.2), (12.5, 9.2)], [(40.0, 36.8), (52.0, 37.1), (45.0, 41.2)]]
# six large triangles, w varying within each by a factor of 1.12 (a quarter of a level, log2 1.12^2 = 0.33, centred by the construction)
PERSPECTIVE_TRIS = [[(2.0, 2.0), (30.0, 4.0), (12.0, 26.0)], [(34.0, 3.0), (66.0, 6.0), (48.0, 28.0)], [(4.0, 24.0), (26.0, 42.0), (3.0, 43.0)],
                    [(28.0, 22.0), (50.0, 40.0), (26.0, 41.0)], [(52.0, 24.0), (68.0, 43.0), (50.0, 42.0)], [(14.0, 8.0), (44.0, 12.0), (30.0, 34.0)]]


def _mip_cases():
    out = []
    c = lambda *a, **kw: out.append(_case(*a, mip=True, **kw))
    c('mip/mid/C1/wrap/seam', '24 x 16 texels over several periods, levels near 1.5 (three levels: 24 -> 3 is odd): the shifted view, w0wrap / w1wrap',
      'levels', 1, 'wrap', (16, 24), n_tri=60, size=10.0, levels=(1.5, 1.35, 1.65), uv_range=(0.0, 3.0))
    c('mip/mid/C3/clamp', '32 x 32 texels, uv beyond [0, 1]: mu / mv = 0, taps in the padding at both levels; levels near 0.5 and 2.5',
      'levels', 3, 'clamp', (32, 32), n_tri=60, size=10.0, levels=(0.4, 2.6), uv_range=(-0.3, 1.3))
    c('mip/mid/C4/zero', 'the same under zero: taps with corners in the padding at both levels', 'levels', 4, 'zero', (32, 32), n_tri=60, size=10.0,
      levels=(0.4, 2.6), uv_range=(-0.3, 1.3))
    c('mip/span', '64 x 64, the whole chain: levels near 1.5 .. 4.5 in one bin and 0.5 in triangles off the pass-0 rows: levels >= mlb + 3 and < mlb go to memory',
      'levels', 1, 'wrap', (64, 64), n_tri=90, size=8.0, levels=(1.45, 2.55, 3.5, 4.6), uv_range=(0.0, 3.0), extra=OFF_PASS0_TRIS, extra_level=0.5)
    c('mip/top', '16 x 16 with all four levels: one group clamps at the 1 x 1 top (l1 == l0, both taps of an axis on one texel), one sits between 3 and 4, one clamps at level 0',
      'levels', 1, 'wrap', (16, 16), n_tri=60, size=10.0, levels=(5.5, 3.5, -0.6), uv_range=(0.0, 3.0))
    c('mip/no-levels', 'a 15 x 17 texture has no chain: the mip kernels with level 0 alone', 'levels', 3, 'wrap', (15, 17), n_tri=60, size=10.0,
      levels=(0.5, 1.5), uv_range=(0.0, 3.0))
    c('mip/overflow/C3', 'a footprint stretched 4 : 1 at level 0.4: the pass-0 extent does not fit 1088 cells, place() takes its aspect branch', 'levels', 3,
      'wrap', (64, 64), n_tri=60, size=10.0, levels=(0.4,), aniso=0.25, uv_range=(0.0, 1.0))
    c('mip/perspective', 'w varies WITHIN each of six large triangles: the level moves inside one integer interval, the w column gets terms through gdb',
      'perspective', 1, 'wrap', (16, 16), level=1.5)
    c('mip/islands/zero', 'separated triangles on an empty frame: k_fix_mip\'s difference term and the empty share alone near uv = (0, 0)', 'islands', 4,
      'zero', (16, 16), uv_box=(0.55, 0.8))      # (about a texel a pixel: levels below 1, so no tap of level 1 comes near texel (0, 0))
    for k in TINY:
        c(f'mip/tiny/{k}', 'an image of one or two pixels', 'tiny', 3 if k == '1x1' else 1, 'wrap', (8, 8), res=TINY[k][0], B=1, tiny=k)
    return out


MIP_CASES = _mip_cases()
MIP_CASE_IDS = [c['name'] for c in MIP_CASES]


def _geometry(c, gen):
    """-> X [B,V,2], z, w [B,V], tri, uv [Vt,2] float64, uv_tri."""
    (H, W), B, (Ht, Wt) = c['res'], c['B'], c['tex_hw']
    if c['geom'] in ('soup', 'confetti'):
        X, z, w, tri = _fat_soup(B, c['n_tri'], gen, H, W, c['size'])
        if 'extra' in c:      # hand-placed triangles in front of the soup (z/w = -0.95), the same in every image but 0.37 pixel apart
            E = torch.tensor(c['extra'], dtype=torch.float64).reshape(1, -1, 2) + torch.arange(B, dtype=torch.float64).reshape(B, 1, 1) * 0.37
            X, z = torch.cat([X, E], 1), torch.cat([z, torch.full((B, E.shape[1]), -0.95, dtype=torch.float64)], 1)
            w = torch.cat([w, torch.rand(B, E.shape[1], generator=gen, dtype=torch.float64) * 2.5 + 0.5], 1)
            tri = torch.arange(X.shape[1], dtype=torch.int32).reshape(-1, 3)
        if c['geom'] == 'confetti':      # every triangle at its own place in the texture, at about a texel a pixel
            centre = X[0].reshape(-1, 3, 2).mean(1, keepdim=True)
            uv = (torch.rand(c['n_tri'], 1, 2, generator=gen, dtype=torch.float64) + (X[0].reshape(-1, 3, 2) - centre) / Wt).reshape(-1, 2)
        elif 'span' in c:
            uv = torch.stack([X[0, :, 0] / W, X[0, :, 1] / H], -1) * c['span'] - 0.5 * (c['span'] - 1.0)
        elif c.get('affine'):
            # w one per triangle: the interpolation is affine in the screen, the step a whole number of texels a pixel, and the fraction
            # (fx, fy) one per triangle, drawn away from the cell borders -- at 128 texels the coordinate's own scale is thousands of u, and
            # no triangle of random fractions keeps all its pixels 64 of them away from a border
            w = w.reshape(B, -1, 3)[..., :1].expand(-1, -1, 3).reshape(B, -1).contiguous()
            shift = torch.tensor([[3.0, -2.0]], dtype=torch.float64) * torch.arange(B, dtype=torch.float64).reshape(B, 1, 1)
            X = X[:1] + shift
            w[1:] = -w[1:]      # the second image lies behind the camera: every texel under a pixel outside a blend has ONE term
            draw = lambda n: 0.15 + 0.7 * torch.rand(n, 2, generator=gen, dtype=torch.float64)
            fn = lambda X_, off: (_screen_uv(X_[0], Ht, Wt, c['tpp']).reshape(-1, 3, 2) + ((off - c['tpp'] * 0.5 + 0.5) / torch.tensor([Wt, Ht]))[:, None]).reshape(-1, 2)
            return X, z, w, tri, None, tri.clone(), dict(uv_fn=fn, off=draw(c['n_tri']), draw_off=draw, shift=shift)
        else:
            uv = _screen_uv(X[0], Ht, Wt, c['tpp'], origin=(-7.3, -5.1))
        return X, z, w, tri, uv, tri.clone(), {}
    if c['geom'] in ('levels', 'perspective'):
        rnd = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
        if c['geom'] == 'levels':
            X, z, w, tri = _fat_soup(B, c['n_tri'], gen, H, W, c['size'])
            lev = [c['levels'][i % len(c['levels'])] for i in range(c['n_tri'])]
            if 'extra' in c:      # hand-placed triangles in front of the soup (z/w = -0.95), at a level of their own
                E = torch.tensor(c['extra'], dtype=torch.float64).reshape(1, -1, 2).repeat(B, 1, 1)
                X, z = torch.cat([X, E], 1), torch.cat([z, torch.full((B, E.shape[1]), -0.95, dtype=torch.float64)], 1)
                w = torch.cat([w, rnd(B, E.shape[1]) * 2.5 + 0.5], 1)
                lev += [c['extra_level']] * (E.shape[1] // 3)
            w = w.reshape(B, -1, 3)[..., :1].expand(-1, -1, 3).reshape(B, -1).contiguous()      # one w per triangle
        else:
            P = torch.tensor(PERSPECTIVE_TRIS, dtype=torch.float64)
            P = P.mean(1, keepdim=True) + 0.6 * (P - P.mean(1, keepdim=True))      # (over a hundred pixels each; larger ones do not settle: every pixel has 20 choices)
            X = P.reshape(1, -1, 2).repeat(B, 1, 1)
            n = X.shape[1] // 3
            z = rnd(B, 3 * n) * 1.8 - 0.9
            w = ((rnd(1, n, 1) * 2.0 + 0.7) * torch.tensor([1.0, 1.06, 1.12], dtype=torch.float64)).reshape(1, -1).repeat(B, 1)
            lev = [0.0] * n      # (case_inputs centres every triangle's level on c['level'] through `scale`)
        T = X.shape[1] // 3
        tri = torch.arange(3 * T, dtype=torch.int32).reshape(T, 3)
        shift = torch.tensor([[3.0, -2.0]], dtype=torch.float64) * torch.arange(B, dtype=torch.float64).reshape(B, 1, 1)
        X = X[:1] + shift
        major = 2.0 ** torch.tensor(lev, dtype=torch.float64)
        minor = major * c.get('aniso', 0.5)
        even = (torch.arange(T) % 2 == 0)
        tpp = torch.stack([torch.where(even, major, minor), torch.where(even, minor, major)], 1)      # texels a pixel along u, along v
        scale = torch.ones(T, dtype=torch.float64)
        lo, hi = c.get('uv_range', (0.0, 3.0))
        draw = lambda n_: lo + (hi - lo) * rnd(n_, 2)
        size = torch.tensor([Wt, Ht], dtype=torch.float64)

        # (perspective: the screen is turned before it is scaled, so dudy != dvdx -- with both 0 their exchange would change nothing)
        ang = (0.5 + 0.3 * torch.arange(T, dtype=torch.float64)) if c['geom'] == 'perspective' else torch.zeros(T, dtype=torch.float64)
        rot = torch.stack([torch.stack([torch.cos(ang), -torch.sin(ang)], 1), torch.stack([torch.sin(ang), torch.cos(ang)], 1)], 1)      # [T,2,2]

        def fn(X_, off):
            P = X_[0].reshape(-1, 3, 2)
            turned = torch.einsum('tij,tkj->tki', rot, P - P.mean(1, keepdim=True))
            return (turned * (tpp * scale[:, None] / size)[:, None] + off[:, None]).reshape(-1, 2)
        return X, z, w, tri, None, tri.clone(), dict(uv_fn=fn, off=draw(T), draw_off=draw, shift=shift, scale=scale)
    if c['geom'] == 'mesh':
        v, tri = _subdivided(*AR._octahedron())      # 66 vertices, 128 triangles, closed
        Xs, zs, ws = [], [], []
        for b in range(3):
            Rm, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
            p = v @ Rm.T * torch.tensor([1.0, 0.9, 1.1], dtype=torch.float64)
            wv = 3.0 + p[:, 2]
            Xs.append(torch.stack([W / 2 + 1.3 * (b - 1) + 130.0 * p[:, 0] / wv, H / 2 - 0.7 * b + 130.0 * p[:, 1] / wv], 1))
            zs.append(p[:, 2] / 4.0)
            ws.append(wv if b < 2 else -wv)      # the third pose: every w negative, the image shows nothing
        uv = 0.5 + 0.45 * v[:, :2] + 0.1 * v[:, 2:3]
        return torch.stack(Xs), torch.stack(zs), torch.stack(ws), tri, uv, tri.clone(), dict(shared=True)
    tris = ISLANDS if c['geom'] == 'islands' else [TINY[c['tiny']][1]]
    X = torch.tensor(tris, dtype=torch.float64).reshape(1, -1, 2).repeat(B, 1, 1)
    X = X + torch.arange(B, dtype=torch.float64).reshape(B, 1, 1) * 0.37
    n = X.shape[1] // 3
    w = torch.rand(B, 3 * n, generator=gen, dtype=torch.float64) * 2.5 + 0.5
    z = torch.rand(B, 3 * n, generator=gen, dtype=torch.float64) * 1.8 - 0.9
    tri = torch.arange(3 * n, dtype=torch.int32).reshape(n, 3)
    uv_lo, uv_span = c.get('uv_box', (0.3, 0.4))
    uv = uv_lo + uv_span * torch.rand(3 * n, 2, generator=gen, dtype=torch.float64)
    return X, z, w, tri, uv, tri.clone(), {}


def case_inputs(name, oracle_ops):
    """The float32 inputs of a case, settled: dict with pos [B,V,4], tri, ids (oracle_ops.rasterize_ids), res, uv [Vt,2], uv_tri, tex
    [Ht,Wt,C], ref_u8 [B,H,W], boundary.  Cached: treat as read-only."""
    if name in _case_cache:
        return _case_cache[name]
    mip = name in MIP_CASE_IDS
    c = MIP_CASES[MIP_CASE_IDS.index(name)] if mip else CASES[CASE_IDS.index(name)]
    gen = torch.Generator().manual_seed(4000 + sum(ord(ch) for ch in (name if mip else name.split('/')[0])) + 7 * c['C'])
    X, z, w, tri, uv, uv_tri, extra = _geometry(c, gen)
    (H, W), B, (Ht, Wt), C = c['res'], c['B'], c['tex_hw'], c['C']
    tex = (torch.rand(Ht, Wt, C, generator=gen) * 0.5 + 0.01).contiguous()
    ref = torch.randint(1, 141, (B, H, W), generator=gen, dtype=torch.uint8)      # (never 0: a pixel that shows only zero-mode padding has colour 0, and dd = 0 must not occur)
    g = dict(X=X, z=z, w=w, tri=tri, uv=uv, uv_tri=uv_tri, tex=tex, ref_u8=ref, boundary=c['boundary'], res=(H, W), **dict(dict(off=None), **extra))
    ids_of = lambda p, t: oracle_ops.rasterize_ids(p, t, (H, W))
    if mip:
        g['mip_levels'] = TR.num_levels(Ht, Wt, c.get('max_mip_level'))
    if c['geom'] == 'perspective':      # centre every triangle's level on c['level']: the level is log2 of the triangle's uv scale plus a term of its geometry
        pos = _clip(X, z, w, H, W)
        probe = dict(pos=pos, tri=tri, ids=ids_of(pos, tri), res=(H, W), uv=extra['uv_fn'](X, g['off']).float().contiguous(), uv_tri=uv_tri, tex=tex,
                     ref_u8=ref, boundary=c['boundary'], mip_levels=g['mip_levels'])
        ch = {}
        _forward(probe, torch.float32, ch)
        st = _forward(probe, torch.float64, ch)
        for t in range(tri.shape[0]):
            raw = st.lk.raw.v[st.px.t == t]
            extra['scale'][t] *= 2.0 ** (c['level'] - 0.5 * float(raw.min() + raw.max()))
    inp = _settle(g, ids_of, gen)
    if mip:
        inp['max_mip_level'] = c.get('max_mip_level')
    inp['name'] = name
    _case_cache[name] = inp
    return inp


def with_mip(inp, max_mip_level=None):
    """The inputs of a non-mip case for the call with enable_mip=True (a copy under the name 'mip/' + its name, cached like a case)."""
    name = 'mip/' + inp['name']
    if name not in _case_cache:
        Ht, Wt, _ = inp['tex'].shape
        _case_cache[name] = dict(inp, name=name, mip_levels=TR.num_levels(Ht, Wt, max_mip_level), max_mip_level=max_mip_level)
    return _case_cache[name]


# The weighted call (tests/test_gpu_objective_weighted_ref.py): seeded weights on the settled cases above.  The captures lie in 1 .. 140, so a
# saturation level of 100 takes a good share of them.  Every case runs the five kinds and scales under the full option set, and each other
# option set of tests/test_gpu_weighted_objective.py -- (w_outside, sat) = (0.25, 0), (0, 0), (0, 100) with mask and face weights, the mask
# alone, the face weights alone -- under one kind other than L2.
WEIGHTED_CASE_IDS = ['soup/C1/wrap/seam', 'soup/C3/clamp', 'soup/C4/zero', 'islands/wrap', 'islands/clamp', 'borders', 'mesh/B3', 'tiny/1x1',
                     'magnified/C1/wrap']      # (the last for its thousands of one-term texels: the others have none to four)
WEIGHT_SAT = 100
# tag: (kind, c, mask, face weights, w_outside, sat)
WEIGHT_SETS = {
    'l2/all': ('l2', None, True, True, 0.25, WEIGHT_SAT),
    'charbonnier2/all': ('charbonnier', 2.0, True, True, 0.25, WEIGHT_SAT),
    'charbonnier20/all': ('charbonnier', 20.0, True, True, 0.25, WEIGHT_SAT),
    'geman2/all': ('geman_mcclure', 2.0, True, True, 0.25, WEIGHT_SAT),
    'geman20/all': ('geman_mcclure', 20.0, True, True, 0.25, WEIGHT_SAT),
    'charbonnier2/w0.25': ('charbonnier', 2.0, True, True, 0.25, 0),
    'geman20/w0': ('geman_mcclure', 20.0, True, True, 0.0, 0),
    'charbonnier20/w0,sat': ('charbonnier', 20.0, True, True, 0.0, WEIGHT_SAT),
    'geman2/mask': ('geman_mcclure', 2.0, True, False, 1.0, 0),
    'charbonnier2/faces': ('charbonnier', 2.0, False, True, 1.0, 0),
}
WEIGHT_TAGS = list(WEIGHT_SETS)
NEUTRAL = ('l2', None, False, False, 1.0, 0)      # tag 'neutral': the plain objective through the weighted statement


def case_weights(inp):
    """The case's own mask [B,H,W] uint8 -- random bytes with a block of 0 and a block of 255 (at 45 x 70: rows 5 .. 13, columns 8 .. 29 and rows
    20 .. 39, columns 25 .. 59), the bytes 1 and 254 on two covered pixels outside the blocks (an image of one pixel: 254) -- and face weights
    [T] float32: random below 1.5, a fifth of them exactly 0, face 0 at 0 and face 1 at 1.25.  Seeded by the case's name."""
    B, (H, W), T = inp['pos'].shape[0], inp['res'], inp['tri'].shape[0]
    g = torch.Generator().manual_seed(77 + sum(ord(ch) for ch in inp.get('base', inp['name'])))
    mask = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    block = torch.zeros(H, W, dtype=torch.bool)
    mask[:, H * 5 // 45:H * 14 // 45, W * 8 // 70:W * 30 // 70] = 0
    mask[:, H * 20 // 45:H * 40 // 45, W * 25 // 70:W * 60 // 70] = 255
    block[H * 5 // 45:H * 14 // 45, W * 8 // 70:W * 30 // 70] = True
    block[H * 20 // 45:H * 40 // 45, W * 25 // 70:W * 60 // 70] = True
    free = torch.nonzero(((inp['ids'].detach().cpu() > 0) & ~block).reshape(-1), as_tuple=True)[0]
    free = free[torch.randperm(free.numel(), generator=g)][:2]
    for p, byte in zip(free.tolist(), (254, 1)):
        mask.reshape(-1)[p] = byte
    face_w = torch.rand(T, generator=g) * 1.5
    face_w[torch.rand(T, generator=g) < 0.2] = 0.0
    face_w[0] = 0.0
    if T > 1:
        face_w[1] = 1.25
    return dict(mask=mask, face_weights=face_w)


def with_weights(inp, tag):
    """The inputs of a case for the weighted call under WEIGHT_SETS[tag] ('neutral': NEUTRAL), a copy under the name case | tag, cached like a
    case; inp['base'] names the case, whose choices it shares."""
    name = inp['name'] + '|' + tag
    if name not in _case_cache:
        kind, c, use_mask, use_faces, w_out, sat = NEUTRAL if tag == 'neutral' else WEIGHT_SETS[tag]
        cw = case_weights(inp)
        _case_cache[name] = dict(inp, name=name, base=inp['name'], tag=tag, weights=dict(
            kind=kind, c=c, mask=cw['mask'] if use_mask else None, face_weights=cw['face_weights'] if use_faces else None, weight_outside=w_out,
            saturation=sat))
    return _case_cache[name]


@functools.lru_cache(maxsize=None)
def _max_deferred_cached(name):
    return plan(_case_cache[name])['max_deferred']


def value_count(inp):
    """n_value of a call: its channels, the most deferred pixels of a bin (a matter of ids and silhouettes, the same with weights), its form."""
    if _case_cache.get(inp.get('name')) is inp and 'base' in inp:
        most = _max_deferred_cached(inp['base'])
    else:
        most = plan(inp)['max_deferred']
    wt = inp.get('weights')
    return n_value(inp['tex'].shape[2], most, inp.get('mip_levels') is not None, None if wt is None else wt['kind'])


@functools.lru_cache(maxsize=None)
def _reference_cached(name, dtype):
    return evaluate(_case_cache[name], dtype)


@functools.lru_cache(maxsize=8)      # (with_weights: ninety variants of a few cases, each used by one test at a time)
def _reference_cached_weighted(name, dtype):
    return evaluate(_case_cache[name], dtype)


def reference(inp, dtype=torch.float64):
    """evaluate() on a case's inputs.  Cached: treat as read-only."""
    if _case_cache.get(inp.get('name')) is inp and MUTANT is None:
        return (_reference_cached_weighted if 'base' in inp else _reference_cached)(inp['name'], dtype)
    return evaluate(inp, dtype)


def measure_rows(x, ref, name):
    """measure() of output `name` (g_tex, g_pos) -> list of (row name, e in units of u): g_pos has its w column on a row of its own."""
    r, S = ref[name]
    x = x.detach().cpu()
    if name == 'g_tex':
        return [('g_tex', measure(x, r, S)[0])]
    if name == 'wsum':      # (the weighted call's sum of all weights: one number)
        return [('wsum', measure(x.reshape(()), r, S)[0])]
    xyz = [0, 1, 2]
    return [('g_pos', measure(x[..., xyz], r[..., xyz], S[..., xyz])[0]), ('g_pos.w', measure(x[..., 3], r[..., 3], S[..., 3])[0])]


def value_error(x, ref):
    """|x - r| / S of the value in units of u."""
    r, S = ref['value']
    if float(S) == 0.0:      # (a weighted call whose every weight is 0: the value is the exact 0)
        return 0.0 if float(x) == float(r) else float('inf')
    return abs(float(x) - float(r)) / float(S) / U


def failures(inp, ref, r32, got, k32=None):
    """What of `got` (value, g_tex, g_pos, optionally the one-term texels) misses a bar of tests/test_gpu_objective_ref.py -> list.  ref, r32: evaluate() in float64 and float32; k32: float32_in_kernel_order."""
    bad = []
    zeros = predicted_zeros(inp)
    for k in OUTPUTS:
        if not torch.equal(ref[k][1] == 0, zeros[k]):
            bad.append((k, 'the entries without a scale are not the predicted ones'))
        try:
            rows, rows32 = measure_rows(got[k], ref, k), measure_rows(r32[k][0], ref, k)
        except AssertionError:
            bad.append((k, 'a term where there is none'))
            continue
        for (row, e), (_, e32) in zip(rows, rows32):
            if not e <= 8 * e32 + 4:
                bad.append((row, 'bound', round(e, 2), round(8 * e32 + 4, 2)))
    n = value_count(inp)
    if not value_error(got['value'], ref) <= n + 2:
        bad.append(('value', value_error(got['value'], ref), n + 2))
    if 'wsum' in ref:      # the weighted call: the sum of all weights, by the long-sum bar
        try:
            e, e32 = measure_rows(got['wsum'], ref, 'wsum')[0][1], measure_rows(r32['wsum'][0], ref, 'wsum')[0][1]
            if not e <= 8 * e32 + 4:
                bad.append(('wsum', 'bound', round(e, 2), round(8 * e32 + 4, 2)))
        except AssertionError:
            bad.append(('wsum', 'a weight where there is none'))
    if k32 is not None and not torch.equal(got['g_tex'].reshape(-1, inp['tex'].shape[2])[k32['texel']].float(), k32['g_tex']):
        bad.append(('g_tex', 'a one-term texel is not gq * w bit for bit'))
    return bad

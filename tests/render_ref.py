"""float64 statement on the CPU of the backward of the fused render pair (csrc/fused.hip: k_render_bwd behind fpcdr_render_bwd, the
backward of ops.render_textured), without autograd: the yardstick of tests/test_gpu_render.py, itself checked on the CPU by
tests/test_render_ref.py.  Nothing here imports fpc_diffrend_amd; the triangle ids come from the function handed to inputs()
(oracle.ops), as in objective_ref.case_inputs.

The statement COMPOSES the three operator references and restates none of them.  Its inputs are the float32 values k_render_bwd reads:
pos, tri, uv, uv_tri, tex, rast = (u, v, z/w, id) as the forward wrote it and dy = d loss / d colour [B,H,W,C].
    interpolate_ref.interpolate      (tu, tv) = u q0 + v q1 + (1 - u - v) q2 on the covered pixels; an empty pixel has uv = (0, 0)
    texture_ref.texture 'linear'     with go = dy on EVERY pixel: g_tex (an empty pixel scatters to the taps of (0, 0); 'zero' padding
                                     receives nothing) and g_uv = (sum_c dy_c d col_c / d fx Wt mu, ... Ht mv), the clamp masks mu, mv
                                     inclusive at 0 and 1
    interpolate_ref.interpolate      go = g_uv: g_rast = (g_u, g_v, 0, 0) on the covered pixels
    rasterize_ref.rasterize          go = g_rast, no rast_db gradient: g_pos [B,V,4] (shade_pixel_bwd<false> on pos itself, as the kernel)
reference(inp, dy, dtype) returns (value, S) for g_tex and g_pos.

THE SCALE S IS CARRIED through all three stages: every reference returns, per entry, the sum of the absolute values of its terms with
its upstream gradient counted as an input (S = |g|), and every backward stage is linear in that gradient.  So each stage runs twice: on
the upstream VALUE for the value, and on the upstream SCALE (a non-negative tensor in the gradient's place) for the scale.  g_tex has no
stage above it; its S is texture_ref's own, coordinate-aware one with dy as the input.  S(g_pos) is therefore never below the last
stage's own scale (|g| <= S_g entry by entry).  The carried scale is the project's rule and gives the rows `g_pos` and `g_pos.w`; it is
hundreds of times the entries where the channels of d colour / d uv cancel, so the last stage's OWN scale (rasterize_ref's S with
g_rast's value as its input: 'g_pos_own') gives two more rows, `g_pos/own` and `g_pos.w/own`, under the same bar -- smaller, hence
stricter, and with more zeros (an entry whose g_rast is the exact 0 has none).  The forward values (rast, and the texture coordinate
formed from it) enter as the references take them: rast as an input, the coordinate through texture_ref's X_s of |tu| alone, so what
float32 loses forming tu from u, v and the three corners is part of e32, which is measured and not derived (6 u on `magnified/C1/wrap`,
256 texels wide; below 2.1 u elsewhere).

Every discrete choice (the tap cells, floor(tu) under 'wrap', the clamp of tu, the clamp and renormalise gates of the barycentrics) is
made by each evaluation in its own dtype; margins() gives how far each is from flipping in units of u of its own scale.  The cases are
objective_ref's settled non-mip cases -- exactly the inputs this kernel pair takes -- and three derived from them by cutting the texture,
which moves no choice that matters (below), so nothing is settled again.

predicted_zeros() names the entries without a term from ids, tap patterns, gates and the zeros of dy alone, never from values.
kernel_order() names the texel entries that hold exactly ONE term and the float32 product dy_c * w_k there, the weights in the kernel's
expression order ((1 - fx) (1 - fy), fx (1 - fy), (1 - fx) fy, fx fy on the fractions of make_taps at the float32 (tu, tv) of
interpolate_ref.float32_in_kernel_order: k_render_bwd forms w = (1 - u) - v and tu = (u q0 + v q1) + w q2, the same expression)."""
import functools

import torch

import interpolate_ref as IR
import objective_ref as OR
import rasterize_ref as RR
import texture_ref as TR
from fitstep_ref import U, measure      # noqa: F401  (re-exported)
from rasterize_ref import GATE_MARGIN

MUTANT = None          # set by test_render_ref.py only: a deliberately wrong restatement (see there)
OUTPUTS = ('g_tex', 'g_pos')
TILE, WAVE = 16, 8     # k_render_bwd: one workgroup per 16 x 16 pixels, one wave per 8 x 8

# name -> (objective_ref case, what becomes of its texture).  A cut texture keeps the case's settled geometry and coordinates: C = 2 keeps
# every tap cell; an axis of ONE texel has both taps of every cell on that texel, so no choice along it changes a value (margins() leaves
# such an axis out), and the other axis keeps its size and with it its cells.
DERIVED = {
    'C2/clamp': ('soup/C3/clamp', lambda t: t[..., :2], 'two channels: the loops are generic in C'),
    'tex1x1/wrap': ('soup/C1/wrap/seam', lambda t: t[:1, :1], 'a 1 x 1 texture: i10 == i00 == i01 == i11, never the two-texel load'),
    'tex1xW/wrap': ('soup/C1/wrap/seam', lambda t: t[:1], 'a 1 x 24 texture: i01 == i00, the two-texel load of C = 1 except across the seam'),
}
CASE_IDS = list(OR.CASE_IDS) + list(DERIVED)
OFF_GEOMETRY = ('islands/clamp', 'islands/zero')
VARIANTS = [(n, k) for n in CASE_IDS for k in ('dense', 'sparse')] + [(n, 'off-geometry') for n in OFF_GEOMETRY]
VARIANT_IDS = [f"{n}-{k}" for n, k in VARIANTS]

_inputs, _upstream = {}, {}


def inputs(name, oracle_ops):
    """The float32 inputs of a case -> dict: pos [B,V,4], tri, ids, res, uv [Vt,2], uv_tri, tex [Ht,Wt,C], boundary, and rast [B,H,W,4],
    the forward's output in float32 (rasterize_ref.float32_in_kernel_order and the ids).  Cached: treat as read-only."""
    if name not in _inputs:
        base, cut, _ = DERIVED.get(name, (name, lambda t: t, ''))
        src = OR.case_inputs(base, oracle_ops)
        inp = {k: src[k] for k in ('pos', 'tri', 'ids', 'res', 'uv', 'uv_tri', 'boundary')}
        inp['tex'] = cut(src['tex']).contiguous()
        k32 = RR.float32_in_kernel_order(inp['pos'], inp['tri'], inp['ids'], inp['res'])
        inp['rast'] = torch.cat([k32['rast'], inp['ids'].float()[..., None]], -1).contiguous()
        inp['name'] = name
        _inputs[name] = inp
    return _inputs[name]


def upstream(inp, kind):
    """dy [B,H,W,C] float32, seeded by the case and the kind.  dense: randn.  sparse: nine pixels in ten zero, and of the rest a third of
    the channels zero (an image of fewer than ten pixels keeps them all).  off-geometry: zero on every covered pixel, randn elsewhere."""
    key = (inp['name'], kind)
    if key not in _upstream:
        gen = torch.Generator().manual_seed(7000 + sum(ord(c) for c in inp['name']) + 13 * len(kind))
        B, (H, W), C = inp['pos'].shape[0], inp['res'], inp['tex'].shape[2]
        dy = torch.randn(B, H, W, C, generator=gen)
        if kind == 'sparse':
            keep = torch.rand(B, H, W, 1, generator=gen) < (0.1 if B * H * W >= 10 else 2.0)
            chan = torch.rand(B, H, W, C, generator=gen) >= (1.0 / 3.0 if C > 1 else 0.0)
            dy = dy * keep * chan
        elif kind == 'off-geometry':
            dy = dy * (inp['ids'] == 0)[..., None]
        else:
            assert kind == 'dense', kind
        _upstream[key] = dy.contiguous()
    return _upstream[key]


# ---------------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------------

def evaluate(inp, dy, dtype=torch.float64):
    """The composition of the module docstring -> dict: 'g_tex' (value, S) [Ht,Wt,C], 'g_pos' (value, S) [B,V,4], and what the tests look
    at: 'uv' (value, S) [B,H,W,2], 'g_uv' (value, S), 'terms' [Ht,Wt,C] (the number of terms of every texel entry), 'pad_all' [B,H,W] (every
    tap in the 'zero' padding), 'covered' [B,H,W], 'px' (rasterize_ref._Pixels) and 'with_g' (the covered pixels shade_pixel_bwd runs for)."""
    B, (H, W) = inp['pos'].shape[0], inp['res']
    attr, rast, uv_tri = inp['uv'][None], inp['rast'], inp['uv_tri']
    if MUTANT == 'q0_q1_swapped':
        uv_tri = uv_tri[:, [1, 0, 2]].contiguous()
    out = IR.interpolate(attr, rast, uv_tri, dtype=dtype)
    covered = out['covered']
    go = dy
    if MUTANT == 'no_empty_scatter':
        go = dy * covered[..., None]
    TR.MUTANT = {'no_clamp_mask': 'no_clamp_mask', 'zero_padding_gets_gradient': 'zero_tap_scatters'}.get(MUTANT)
    try:
        tx = TR.texture(inp['tex'][None], out['out'][0], go=go, filter_mode='linear', boundary=inp['boundary'], dtype=dtype)
    finally:
        TR.MUTANT = None
    g_uv, g_uvS = tx['g_uv']
    if MUTANT == 'Wt_for_both_axes':
        Ht, Wt = inp['tex'].shape[:2]
        g_uv, g_uvS = g_uv * torch.tensor([1.0, Wt / Ht], dtype=dtype), g_uvS * torch.tensor([1.0, Wt / Ht], dtype=dtype)
    # each backward stage on the upstream value for the value, on the upstream scale for the scale
    g_rast = IR.interpolate(attr, rast, uv_tri, go=g_uv, dtype=dtype)['g_rast'][0]
    g_rastS = IR.interpolate(attr, rast, uv_tri, go=g_uvS, dtype=dtype)['g_rast'][1]
    rz = RR.rasterize(inp['pos'], inp['tri'], inp['ids'], (H, W), go=g_rast, grad_db=False, dtype=dtype)
    g_pos = rz['g_pos'][0]
    g_posS = RR.rasterize(inp['pos'], inp['tri'], inp['ids'], (H, W), go=g_rastS, grad_db=False, dtype=dtype)['g_pos'][1]
    if MUTANT == 'w_column_dropped':
        g_pos = g_pos.clone()
        g_pos[..., 3] = 0.0
    return {'g_tex': (tx['g_tex'][0][0], tx['g_tex'][1][0]), 'g_pos': (g_pos, g_posS), 'g_pos_own': (g_pos, rz['g_pos'][1]), 'uv': out['out'], 'g_uv': (g_uv, g_uvS),
            'terms': tx['terms']['g_tex'][0], 'pad_all': tx['pad_all'].reshape(B, H, W), 'covered': covered, 'px': rz['px'], 'with_g': rz['with_g']}


@functools.lru_cache(maxsize=None)
def _reference_cached(name, kind, dtype):
    inp = _inputs[name]
    return evaluate(inp, _upstream[(name, kind)], dtype)


def reference(inp, dy, dtype=torch.float64):
    """evaluate(); cached where dy is upstream(inp, kind) of a case's inputs: treat as read-only."""
    if MUTANT is None and _inputs.get(inp.get('name')) is inp:
        for kind in ('dense', 'sparse', 'off-geometry'):
            if _upstream.get((inp['name'], kind)) is dy:
                return _reference_cached(inp['name'], kind, dtype)
    return evaluate(inp, dy, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# zeros, margins, the one-term texels
# ---------------------------------------------------------------------------------------------------------------------

def _taps(inp, dtype=torch.float64):
    """texture_ref's lookup of every pixel at the statement's coordinate -> (_Sample over the B*H*W pixels, uv (value, S))."""
    out = IR.interpolate(inp['uv'][None], inp['rast'], inp['uv_tri'], dtype=dtype)['out']
    q = out[0].reshape(-1, 2)
    t0 = inp['tex'].detach().to('cpu', dtype)[None]
    return TR._Sample(t0, t0.abs(), torch.zeros(q.shape[0], dtype=torch.long), q[:, 0], q[:, 1], inp['boundary']), out


def predicted_zeros(inp, dy):
    """The entries without any term, from ids, tap patterns, gates and the zeros of dy alone -> dict of bool tensors: 'g_tex' [Ht,Wt,C]
    (texel entries no tap of a pixel with dy_c != 0 reaches: an empty pixel's taps are those of (0, 0)), 'g_pos' [B,V,4] (the z column; x, y
    of a vertex none of whose visible triangles shows a pixel with a term -- dy not all zero, a tap inside the texture, mu or mv open, a
    clamp gate of the barycentrics open --; w also where such pixels all lie at the image's centre, fx = fy = 0)."""
    s, out = _taps(inp)
    B, (H, W) = inp['pos'].shape[0], inp['res']
    Ht, Wt, C = inp['tex'].shape
    P = B * H * W
    live = dy.reshape(P, C) != 0
    count = torch.zeros(Ht * Wt, C, dtype=torch.int64)
    for k in range(4):
        count.index_add_(0, s.flat[k], (live & s.valid[k][:, None]).long())
    q = out[0].reshape(P, 2)
    inside = (q >= 0) & (q <= 1) if inp['boundary'] == 'clamp' else torch.ones(P, 2, dtype=torch.bool)
    has = live.any(1) & s.any_valid & inside.any(1)
    px = RR._Pixels(inp['pos'], inp['tri'], inp['ids'], (H, W), torch.float64)
    has = has.reshape(B, H, W)[px.bi, px.yy, px.xx]
    term = has & (((px.b0.v >= 0) & (px.b0.v <= 1)) | ((px.b1.v >= 0) & (px.b1.v <= 1)))
    off_centre = (px.fx.v != 0) | (px.fy.v != 0)
    rows, rows_w = torch.zeros(B * px.V, dtype=torch.bool), torch.zeros(B * px.V, dtype=torch.bool)
    for k in range(3):
        rows[px.rows[k][term]] = True
        rows_w[px.rows[k][term & off_centre]] = True
    zp = (~rows).reshape(B, px.V, 1).expand(B, px.V, 4).clone()
    zp[..., 2] = True
    zp[..., 3] = ~rows_w.reshape(B, px.V)
    return {'g_tex': (count == 0).reshape(Ht, Wt, C), 'g_pos': zp}


def margins(inp, dy=None):
    """How far the choices of a float32 and a float64 evaluation are from differing, in units of u of each quantity's own scale -> dict:
    'tap': the smallest, over the covered pixels and the axes of more than one texel, of the distances of x = prep(t) n - 0.5 from the
    texel borders below and above it, of t from its own floor and ceiling under 'wrap', and of t from 0 and 1 under 'clamp' (the clamp and
    the masks mu, mv); 'gate': rasterize_ref.gate_margin over the covered pixels (with dy: over those with a gradient)."""
    s, out = _taps(inp)
    cov = (inp['ids'] > 0).reshape(-1)
    q, qS = out[0].reshape(-1, 2)[cov], out[1].reshape(-1, 2)[cov]
    Ht, Wt, _ = inp['tex'].shape
    worst = float('inf')
    for axis, n in ((0, Wt), (1, Ht)):
        if n == 1 or not bool(cov.any()):
            continue
        t, tS = q[:, axis], qS[:, axis]
        gates = []
        if inp['boundary'] == 'wrap':
            fl = torch.floor(t)
            p, pS = t - fl, tS + fl.abs()
            gates += [(p, pS), (1.0 - p, pS)]
        elif inp['boundary'] == 'clamp':
            gates += [(t.abs(), tS), ((1.0 - t).abs(), tS + 1.0)]
            p = t.clamp(0.0, 1.0)
            pS = torch.where(p == t, tS, p)
        else:
            p, pS = t, tS
        x, xS = p * n - 0.5, pS * n + 0.5
        f = x - torch.floor(x)
        gates += [(f, xS), (1.0 - f, xS)]
        worst = min([worst] + [float((v / (U * S)).min()) for v, S in gates])
    r = reference(inp, dy) if dy is not None else {'px': RR._Pixels(inp['pos'], inp['tri'], inp['ids'], inp['res'], torch.float64)}
    return {'tap': worst, 'gate': RR.gate_margin(r)}


def kernel_order(inp, dy):
    """-> dict: 'entry' [m] flat indices into g_tex.reshape(-1) of the texel entries with exactly ONE term, that of a COVERED pixel, and
    'g_tex' [m] float32 dy_c * w_k there (module docstring; one addend onto 0 through an atomic is exact)."""
    k32 = IR.float32_in_kernel_order(inp['uv'][None], inp['rast'], inp['uv_tri'])['out'].reshape(-1, 2)
    t0 = inp['tex'][None]
    s = TR._Sample(t0, t0.abs(), torch.zeros(k32.shape[0], dtype=torch.long), k32[:, 0], k32[:, 1], inp['boundary'])
    Ht, Wt, C = inp['tex'].shape
    g = dy.reshape(-1, C)
    live = g != 0
    count = torch.zeros(Ht * Wt, C, dtype=torch.int64)
    for k in range(4):
        count.index_add_(0, s.flat[k], (live & s.valid[k][:, None]).long())
    cov = (inp['ids'] > 0).reshape(-1, 1)
    entry, val = [], []
    for k in range(4):
        ok = live & s.valid[k][:, None] & cov & (count[s.flat[k]] == 1)
        idx = (s.flat[k][:, None] * C + torch.arange(C)[None])
        entry.append(idx[ok])
        val.append((g * s.wk[k])[ok])
    return {'entry': torch.cat(entry), 'g_tex': torch.cat(val), 'count': count.reshape(Ht, Wt, C)}


# ---------------------------------------------------------------------------------------------------------------------
# the bars
# ---------------------------------------------------------------------------------------------------------------------

def measure_rows(x, ref, name):
    """measure() of output `name` -> list of (row name, e in units of u, entries measured): g_pos has its w column on a row of its own."""
    r, S = ref[name]
    x = x.detach().cpu()
    if name == 'g_tex':
        return [('g_tex', measure(x, r, S)[0], int((S > 0).sum()))]
    xyz = [0, 1, 2]
    rows = [('g_pos', measure(x[..., xyz], r[..., xyz], S[..., xyz])[0], int((S[..., xyz] > 0).sum())),
            ('g_pos.w', measure(x[..., 3], r[..., 3], S[..., 3])[0], int((S[..., 3] > 0).sum()))]
    So = ref['g_pos_own'][1]      # the last stage's own scale: smaller, the stricter rows
    return rows + [('g_pos/own', measure(x[..., xyz], r[..., xyz], So[..., xyz])[0], int((So[..., xyz] > 0).sum())),
                   ('g_pos.w/own', measure(x[..., 3], r[..., 3], So[..., 3])[0], int((So[..., 3] > 0).sum()))]


def bound(e32):
    return 8 * e32 + 4


def preloaded(ref, r32, pre):
    """The statement for buffers that hold `pre` (dict name -> float32 tensor) on entry -- the kernel ADDS: what was there is one more
    term of every entry, value pre and scale |pre| -> (ref, r32) with the float32 side formed in float32."""
    out, out32 = dict(ref), dict(r32)
    for k, p in pre.items():
        out[k] = (ref[k][0] + p.double(), ref[k][1] + p.double().abs())
        out32[k] = (r32[k][0].float() + p, None)
        if k == 'g_pos':
            out['g_pos_own'] = (out[k][0], ref['g_pos_own'][1] + p.double().abs())
    return out, out32


def failures(inp, dy, ref, r32, got, k32=None, one_term_bar=None, pre=None):
    """What of `got` (g_tex and / or g_pos) misses a bar of tests/test_gpu_render.py -> list.  ref, r32: evaluate() in float64 and float32;
    k32: kernel_order() (the one-term texels bit for bit; one_term_bar = a number of u: within that of the product instead); pre: what the
    buffers held on entry (ref and r32 then come from preloaded())."""
    bad = []
    zeros = predicted_zeros(inp, dy)
    for k in OUTPUTS:
        if k not in got:
            continue
        if pre is not None and k in pre:
            zeros[k] = zeros[k] & (pre[k] == 0)
        if not torch.equal(ref[k][1] == 0, zeros[k]):
            bad.append((k, 'the entries without a scale are not the predicted ones'))
        if not bool((got[k][zeros[k]] == 0).all()):
            bad.append((k, 'a predicted zero is not exactly 0'))
        try:
            rows, rows32 = measure_rows(got[k], ref, k), measure_rows(r32[k][0], ref, k)
        except AssertionError:
            bad.append((k, 'a term where there is none'))
            continue
        for (row, e, _), (_, e32, _) in zip(rows, rows32):
            if not e <= bound(e32):
                bad.append((row, 'bound', round(e, 2), round(bound(e32), 2)))
    if k32 is not None and 'g_tex' in got:
        x = got['g_tex'].reshape(-1)[k32['entry']].float()
        if one_term_bar is None:
            if not torch.equal(x, k32['g_tex']):
                bad.append(('g_tex', 'a one-term texel is not dy * w bit for bit'))
        elif k32['entry'].numel() and not float(((x - k32['g_tex']).abs() / k32['g_tex'].abs()).max()) <= one_term_bar * U:
            bad.append(('g_tex', f'a one-term texel is not within {one_term_bar} u of dy * w'))
    return bad

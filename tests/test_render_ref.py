"""CPU: the float64 yardstick of the fused render pair's backward (tests/render_ref.py) is right, and what tests/test_gpu_render.py
asks of k_render_bwd is reachable and discriminates:
  1. on the inputs and upstream gradients of every GPU case the statement equals float64 torch.autograd through the oracle's
     rasterize -> interpolate -> texture 'linear' (the barycentrics taking the VALUE of the float32 rast the kernel reads and the
     derivative of the float64 chain), to 1e-12 of the entry's scale;
  2. every case keeps its margins (the smallest is printed; the worst over all cases is 335 u on the taps, `soup/C1/wrap/seam`, and 77 u
     on the barycentric gates), reaches the path it is named for, leaves no entry with a scale unmeasured, and the float32 evaluation by
     torch meets every bar the GPU is held to, the one-term texels bit for bit included;
  3. wrong restatements, evaluated in float64, exceed 8 * e32 + 4 on a named case: no empty-pixel scatter, q0 and q1 swapped, the factor
     Wt for both axes, the w column of g_pos dropped, padding receiving gradient under 'zero'.
     Ignoring the clamp masks mu, mv is NOT among them, because it cannot be: beyond [0, 1] the clamp puts both taps of the axis on one
     texel, t10 - t00 is exactly 0 and the unmasked gradient is the same 0 (tests/test_texture_ref.py shows it for the operator).  What
     that restatement changes is the SCALE of those entries, so it is caught where the GPU test asks that the entries with a scale be the
     predicted ones; test_ignoring_the_clamp_mask_changes_no_value states both halves.
Lines "RENDER ..." are printed under pytest -s."""
import functools

import pytest
import torch

import render_ref as R
import texture_ref as TR


@functools.lru_cache(maxsize=None)
def _four(name, kind, oracle_ops):
    inp = R.inputs(name, oracle_ops)
    dy = R.upstream(inp, kind)
    return inp, dy, R.reference(inp, dy), R.reference(inp, dy, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the statement against autograd through the oracle
# ---------------------------------------------------------------------------------------------------------------------

def _oracle(inp, dy, oracle_ops):
    leaf = lambda t: t.detach().double().requires_grad_(True)
    pos, tex = leaf(inp['pos']), leaf(inp['tex'])
    rast, _ = oracle_ops.rasterize(pos, inp['tri'], inp['res'], ids=inp['ids'])
    rast = inp['rast'].double() + (rast - rast.detach())      # the kernel's point of evaluation, the chain's derivative
    uv, _ = oracle_ops.interpolate(inp['uv'].double()[None], rast, inp['uv_tri'])
    col = oracle_ops.texture(tex[None], uv, filter_mode='linear', boundary_mode=inp['boundary'])
    (col * dy.double()).sum().backward()
    return {'g_pos': pos.grad, 'g_tex': tex.grad}


@pytest.mark.parametrize("name,kind", R.VARIANTS, ids=R.VARIANT_IDS)
def test_statement_equals_autograd_through_the_oracle(name, kind, oracle_ops):
    inp, dy, ref, _ = _four(name, kind, oracle_ops)
    got = _oracle(inp, dy, oracle_ops)
    for k in R.OUTPUTS:
        r, S = ref[k]
        assert r.shape == got[k].shape, (name, k)
        assert bool((got[k][S == 0] == 0).all()), (name, k, 'the oracle has a term where the statement has none')
        worst = float(((r - got[k]).abs() / S.clamp(min=1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0
        print(f"RENDER {name} {kind} {k} statement vs float64 autograd: {worst:.2e} of the scale")
        assert worst <= 1e-12, (name, k, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the cases
# ---------------------------------------------------------------------------------------------------------------------

def _wave_tiles(flag, res):
    """[B,H,W] bool -> per 8 x 8 wave tile of k_render_bwd the number of set pixels and of pixels, [B,ty,tx] each."""
    B, (H, W) = flag.shape[0], res
    ty, tx = -(-H // R.WAVE), -(-W // R.WAVE)
    pad = torch.zeros(B, ty * R.WAVE, tx * R.WAVE, 2)
    pad[:, :H, :W, 0], pad[:, :H, :W, 1] = flag.float(), 1.0
    t = pad.reshape(B, ty, R.WAVE, tx, R.WAVE, 2).sum((2, 4))
    return t[..., 0], t[..., 1]


def check_paths(name, kind, inp, dy, ref):
    """The path each case is named for, on the patterns of the float64 evaluation."""
    s, out = R._taps(inp)
    B, (H, W) = inp['pos'].shape[0], inp['res']
    Ht, Wt, C = inp['tex'].shape
    P = B * H * W
    cov = (inp['ids'] > 0).reshape(P)
    live = (dy.reshape(P, C) != 0).any(1)
    count = R.kernel_order(inp, dy)['count']
    q = out[0].reshape(P, 2)
    px, with_g = ref['px'], ref['with_g']
    base = R.DERIVED.get(name, (name,))[0]
    if base == 'soup/C3/clamp' and kind != 'off-geometry':
        for axis in (0, 1):      # mu = 0, mv = 0 on pixels that carry a gradient
            assert int((cov & live & ((q[:, axis] < 0) | (q[:, axis] > 1))).sum()) >= (16 if kind == 'dense' else 2), (name, kind, axis)
        assert C == (2 if name == 'C2/clamp' else 3)
    if name == 'soup/C4/zero':
        invalid = sum((~v).long() for v in s.valid)[cov & live]
        # (validity is a column test AND a row test: exactly one corner outside cannot occur; 0, 2, 3 and 4 do)
        assert set(torch.unique(invalid).tolist()) == {0, 2, 3, 4}
        assert int((ref['pad_all'].reshape(P) & cov & live).sum()) > 0
    if name == 'magnified/C1/wrap' and kind == 'dense':
        # every texel under a covered pixel holds exactly one term, thousands of them -- but for the four taps of (0, 0), where the
        # empty pixels scatter
        assert R.kernel_order(inp, dy)['entry'].numel() >= 5000
        empty_taps = torch.unique(torch.cat([s.flat[k][~cov] for k in range(4)]))
        assert empty_taps.numel() == 4
        for k in range(4):
            f = s.flat[k][cov]
            assert bool(((count[f // Wt, f % Wt, 0] == 1) | torch.isin(f, empty_taps)).all())
    if name == 'soup/C1/wrap/seam' and kind == 'dense':
        assert (Ht, Wt) == (16, 24) and int(count.max()) > 100
    if name == 'mesh/B3':
        assert not bool((inp['ids'][2] != 0).any()) and bool((inp['pos'][2, :, 3] < 0).all())          # the third image: behind the camera
        assert bool(R.predicted_zeros(inp, dy)['g_pos'][2].all()) and bool(live.reshape(B, -1)[2].any())
        assert int(torch.bincount(inp['tri'].long().reshape(-1)).min()) >= 4                              # shared vertices
    if name == 'confetti':
        # a wave's 64 pixels name more different vertices than it has lanes: wave_group_atomic_add's grouping finds few equal keys
        tiles = {}
        for k in range(3):
            for b, y, x, v in zip(px.bi[with_g].tolist(), (px.yy[with_g] // R.WAVE).tolist(), (px.xx[with_g] // R.WAVE).tolist(), px.vi[with_g, k].tolist()):
                tiles.setdefault((b, y, x), set()).add(v)
        most = max(len(v) for v in tiles.values())
        print(f"RENDER {name} {kind} most vertices in a wave's tile {most}")
        assert most >= (64 if kind == 'dense' else 10)
    if name.startswith('islands'):
        n_empty = int((~cov & live).sum())
        assert n_empty >= (1000 if kind != 'sparse' else 100)
        zero = torch.zeros(1, dtype=torch.float64)
        t0 = inp['tex'].double()[None]
        s0 = TR._Sample(t0, t0.abs(), torch.zeros(1, dtype=torch.long), zero, zero, inp['boundary'])
        flat0 = [int(f) for f in s0.flat]
        valid0 = [bool(v) for v in s0.valid]
        if inp['boundary'] == 'clamp':      # all four taps of (0, 0) are the same texel
            assert len(set(flat0)) == 1 and all(valid0)
        if inp['boundary'] == 'zero':       # only one of the four is valid
            assert sum(valid0) == 1
        if inp['boundary'] == 'wrap':
            assert len(set(flat0)) == 4
        for f, ok in zip(flat0, valid0):    # the empty pixels' terms, and no covered pixel's: uv lies away from these taps
            if ok and kind == 'dense':
                assert int(count[f // Wt, f % Wt, 0]) == n_empty * sum(1 for f2, ok2 in zip(flat0, valid0) if ok2 and f2 == f)
        if kind == 'off-geometry':
            assert bool(R.predicted_zeros(inp, dy)['g_pos'].all()) and not bool(with_g.any())
            assert int((~R.predicted_zeros(inp, dy)['g_tex']).sum()) == C * len({f for f, ok in zip(flat0, valid0) if ok})
    if name == 'borders':
        assert inp['res'] == (33, 65) and H % R.TILE and W % R.TILE and H % R.WAVE and W % R.WAVE
        term = torch.zeros(B, H, W, dtype=torch.bool)
        term[px.bi[with_g], px.yy[with_g], px.xx[with_g]] = True
        lv = live.reshape(B, H, W)
        # partial tiles in both directions: the last row and column of tiles hold one pixel row / column, with gradients and with terms
        assert bool(lv[:, 32:].any()) and bool(lv[:, :, 64:].any())
        if kind == 'dense':
            assert bool(term[:, 32:].any()) or bool(term[:, :, 64:].any())
    if name.startswith('tiny'):
        assert H * W <= 2
    if name == 'tex1x1/wrap':
        assert (Ht, Wt, C) == (1, 1, 1) and all(bool((f == 0).all()) for f in s.flat)
        # d colour / d uv is the exact 0 on one texel: no lane has a vertex key, the workgroups leave before wave_group_atomic_add
        assert not bool(with_g.any()) and not bool(ref['g_pos'][0].any()) and bool((ref['g_pos'][1] > 0).any())
    if name == 'tex1xW/wrap':
        assert (Ht, Wt, C) == (1, 24, 1) and bool((s.flat[2] == s.flat[0]).all())
        pair = s.flat[1][cov & live] == s.flat[0][cov & live] + 1      # load_taps: the two-texel load, and the seam that must not take it
        assert bool(pair.any()) and bool((~pair).any())
    if kind == 'sparse' and H * W > 64:
        # a wave with lanes that carry a vertex and lanes that do not: a key of -1 meets wave_group_atomic_add
        term = torch.zeros(B, H, W, dtype=torch.bool)
        term[px.bi[with_g], px.yy[with_g], px.xx[with_g]] = True
        n_term, n_pix = _wave_tiles(term, (H, W))
        assert name == 'tex1x1/wrap' or bool(((n_term > 0) & (n_term < n_pix)).any()), (name, 'no wave mixes keys and -1')
        g = dy.reshape(P, C)
        assert bool((g == 0).all(1).any())                                   # the `any` skip
        if C > 1:
            assert bool(((g == 0).any(1) & (g != 0).any(1)).any())           # the gc != 0 skip


@pytest.mark.parametrize("name,kind", R.VARIANTS, ids=R.VARIANT_IDS)
def test_cases_keep_their_margins_reach_their_paths_and_float32_meets_the_bars(name, kind, oracle_ops):
    inp, dy, ref, r32 = _four(name, kind, oracle_ops)
    m = R.margins(inp, dy)
    k32 = R.kernel_order(inp, dy)
    print(f"RENDER {name} {kind} pixels {ref['px'].n} with a vertex term {int(ref['with_g'].sum())} one-term texel entries {k32['entry'].numel()} "
          f"smallest margin: taps {m['tap']:.0f} u, gates {m['gate']:.0f} u")
    assert m['tap'] >= R.GATE_MARGIN and m['gate'] >= R.GATE_MARGIN, (name, kind, m)
    check_paths(name, kind, inp, dy, ref)
    got = {k: r32[k][0] for k in R.OUTPUTS}
    assert R.failures(inp, dy, ref, r32, got, k32) == []
    zeros = R.predicted_zeros(inp, dy)
    for k in R.OUTPUTS:
        measured = 0
        for row, e32, n in R.measure_rows(r32[k][0], ref, k):
            print(f"RENDER {name} {kind} {row} e32 {e32:.3f} bound {R.bound(e32):.2f} entries {n}")
            measured += 0 if row.endswith('/own') else n
        # vacuity: every entry is either measured against its scale or a predicted zero held exactly; no pixel or entry is masked out
        unmeasured = int((ref[k][1] > 0).sum()) - measured
        assert unmeasured == 0 and measured + int(zeros[k].sum()) == ref[k][0].numel(), (name, kind, k)


# ---------------------------------------------------------------------------------------------------------------------
# 3. wrong restatements miss a bar
# ---------------------------------------------------------------------------------------------------------------------

MUTANTS = {
    'no_empty_scatter': ('islands/wrap', 'dense'),
    'q0_q1_swapped': ('soup/C1/wrap/seam', 'dense'),
    'Wt_for_both_axes': ('soup/C3/clamp', 'dense'),
    'w_column_dropped': ('borders', 'sparse'),
    'zero_padding_gets_gradient': ('soup/C4/zero', 'dense'),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_restatement_misses_a_bar(mutant, oracle_ops, monkeypatch):
    name, kind = MUTANTS[mutant]
    inp, dy, ref, r32 = _four(name, kind, oracle_ops)
    monkeypatch.setattr(R, 'MUTANT', mutant)
    wrong = R.evaluate(inp, dy, torch.float64)
    monkeypatch.setattr(R, 'MUTANT', None)
    missed = R.failures(inp, dy, ref, r32, {k: wrong[k][0] for k in R.OUTPUTS})
    print(f"RENDER mutant {mutant} on {name} {kind}: {missed[:3]}")
    assert any(m[1] == 'bound' for m in missed), (mutant, name, missed)
    if mutant == 'w_column_dropped':      # only the rows of its own see it: x and y are untouched
        assert [m[0] for m in missed] == ['g_pos.w', 'g_pos.w/own'], missed


@pytest.mark.parametrize("name", ['soup/C3/clamp', 'C2/clamp'])
def test_ignoring_the_clamp_mask_changes_no_value(name, oracle_ops, monkeypatch):
    """Module docstring, 3: the unmasked restatement gives the same values entry by entry and other scales, so the bars cannot see it."""
    inp, dy, ref, r32 = _four(name, 'dense', oracle_ops)
    q = ref['uv'][0][ref['covered']]
    assert int(((q < 0) | (q > 1)).sum()) > 50
    monkeypatch.setattr(R, 'MUTANT', 'no_clamp_mask')
    wrong = R.evaluate(inp, dy, torch.float64)
    monkeypatch.setattr(R, 'MUTANT', None)
    for k in R.OUTPUTS:
        assert torch.equal(wrong[k][0], ref[k][0]), (name, k)
    assert torch.equal(wrong['g_tex'][1], ref['g_tex'][1])
    # (the hook is live: pixels beyond [0, 1] now have a scale, and their vertices a larger one)
    assert int((wrong['g_uv'][1] != ref['g_uv'][1]).sum()) > 50
    assert bool((wrong['g_pos'][1] >= ref['g_pos'][1]).all()) and int((wrong['g_pos'][1] > ref['g_pos'][1]).sum()) > 0

"""CPU: the float64 yardstick of the antialias operator (tests/antialias_ref.py) is right, and what tests/test_gpu_antialias.py asks of
the kernels is reachable and discriminates:
  1. on the inputs of every GPU case the statement's `out` and hand-written gradients equal oracle.ops.antialias in float64 under
     torch.autograd to 1e-12 of the entry's scale (an independent derivation of the backward), and topology() equals the oracle's edge table;
  2. every case holds the structural condition that makes it reach its branch (pairs across flag words, waves, workgroups, the image's
     border and bin boundaries; the list of `ties`), no candidate pair lies within GATE_MARGIN u of a float32 decision (`ties` decides
     exactly alike in float32 and float64 instead), float32_in_kernel_order meets every bar the GPU is held to, and dispatch() reaches
     every kernel and path over the cases;
  3. fourteen wrong restatements each miss a bar on a named case.
Lines "AA ..." are printed under pytest -s."""
import functools

import numpy as np
import pytest
import torch

import antialias_ref as R


@functools.lru_cache(maxsize=None)
def _four(name):
    inp = R.case_inputs(name)
    return inp, R.reference(inp), R.reference(inp, torch.float32), R.kernel_order(inp)


def _case(name):
    return R.CASES[R.CASE_IDS.index(name)]


def _pair_index(D, x0, y0, d, b=0):
    pr = D.pairs
    m = torch.nonzero((pr.b == b) & (pr.x0 == x0) & (pr.y0 == y0) & (pr.d == d), as_tuple=True)[0]
    return int(m[0]) if m.numel() else None


def _blended(D):
    """The pairs with an active edge -> (b, x0, y0, d) tensors."""
    pr, hit = D.pairs, D.active.any(1)
    return pr.b[hit], pr.x0[hit], pr.y0[hit], pr.d[hit]


def _pairs_per_receiver(D):
    key = torch.unique(torch.stack([D.er, D.ei], 1), dim=0)
    return torch.bincount(key[:, 0], minlength=D.B * D.H * D.W)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the statement against autograd through the oracle
# ---------------------------------------------------------------------------------------------------------------------

def _oracle(inp, oracle_ops):
    leaf = lambda t: t.detach().double().requires_grad_(True)
    color, pos = leaf(inp['color']), leaf(inp['pos'])
    out = oracle_ops.antialias(color, inp['rast'].double(), pos, inp['tri'], pos_gradient_boost=inp['boost'])
    (out * inp['dy'].double()).sum().backward()
    return {'out': out.detach(), 'g_color': color.grad, 'g_pos': pos.grad if pos.grad is not None else torch.zeros_like(pos)}      # (no pair: no graph)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_statement_equals_autograd_through_the_oracle(name, oracle_ops):
    inp, ref, _, _ = _four(name)
    got = _oracle(inp, oracle_ops)
    base = {'out': inp['color'].double(), 'g_color': inp['dy'].double(), 'g_pos': torch.zeros_like(got['g_pos'])}
    for k in R.OUTPUTS:
        r, S = ref[k]
        assert r.shape == got[k].shape, (name, k)
        assert torch.equal(got[k][S == 0], base[k][S == 0]), (name, k, 'the oracle has a term where the statement has none')
        worst = float(((r - got[k]).abs() / S.clamp(min=1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0
        print(f"AA {name} {k} statement vs float64 autograd: {worst:.2e} of the scale")
        assert worst <= 1e-12, (name, k, worst)
    # the flag planes: the oracle's pair set, laid out in 64-pixel words
    _, flags = oracle_ops.antialias(inp['color'], inp['rast'], inp['pos'], inp['tri'], return_flags=True)
    D = ref['D']
    bits = np.zeros((2, D.B, D.H, D.W), dtype=np.uint8)
    for x in range(D.W):
        bits[..., x] = (D.flags[..., x // 64] >> np.uint64(x % 64)) & np.uint64(1)
    assert torch.equal(torch.from_numpy(bits[0] | (bits[1] << 1)), flags), (name, 'flag planes')
    assert D.flags.shape == (2, D.B, D.H, (D.W + 63) // 64)


@pytest.mark.parametrize("name", R.TOPOLOGY_IDS + ['mesh', 'ties'])
def test_topology_equals_the_oracles_edge_table(name, oracle_ops):
    tri = R._geometry(name)[1] if name in ('mesh', 'ties') else R.topology_tri(name)
    adj = R.topology(tri)
    cnt, oth = oracle_ops.edge_table(tri)
    want = torch.where(cnt == 1, torch.full_like(oth, -1), torch.where(cnt == 2, oth, torch.full_like(oth, -2)))
    assert torch.equal(adj, want.to(torch.int32)), name
    assert int(tri.min()) >= 0


def test_topology_cases_reach_their_branches():
    T = lambda n: R.topology_tri(n).shape[0]
    assert T('T1') == 1 and R.topo_capacity(1) == 64
    assert [R.topo_capacity(t) for t in (10, 11, 170, 171)] == [64, 128, 1024, 2048] and 6 * 10 < 64 < 6 * 11 and 6 * 170 < 1024 < 6 * 171
    assert (R.topology(R.topology_tri('three on an edge'))[:3] == -2).sum() == 3
    assert R.topology(R.topology_tri('a triangle twice'))[0].tolist() == [0, 1, 2]            # (its own corner: sum - own of two equal corners)
    assert R.topology(R.topology_tri('same opposite vertex'))[0].tolist()[2] == 2
    a, p = R.topology_tri('strip/171'), R.topology_tri('strip/171/permuted')
    assert not torch.equal(a, p) and sorted(map(tuple, a.tolist())) == sorted(map(tuple, p.tolist()))
    look = {tuple(t): r for t, r in zip(a.tolist(), R.topology(a).tolist())}
    assert [look[tuple(t)] for t in p.tolist()] == R.topology(p).tolist()
    adj = R.topology(a)
    assert int((adj == -1).sum()) == 171 + 2 and int((adj >= 0).sum()) == 2 * 170


# ---------------------------------------------------------------------------------------------------------------------
# 2. the cases
# ---------------------------------------------------------------------------------------------------------------------

def check_ties(inp, ref):
    D = ref['D']
    pr, E, T = D.pairs, D.E, inp['tri'].shape[0]
    t, act = E['t'].v, D.active
    # float32 and float64 decide alike, and every blend is exact
    D64 = R.decisions(inp['color'], inp['rast'], inp['pos'], inp['tri'], inp['adj'], dtype=torch.float64)
    assert torch.equal(D64.sil, D.sil) and torch.equal(D64.active, act) and torch.equal(D64.far, D.far) and torch.equal(D64.pairs.use1, pr.use1)
    assert torch.equal(t[act].double(), ref['E']['t'].v[act])
    aLd, aLo = E['Ld'].v.abs(), E['Lo'].v.abs()
    extent = (E['ya'].v < 0) != (E['yb'].v < 0)
    rest = (E['Ld'].v != 0) & (t >= 0) & (t <= 1)
    for val in (0.0, 0.5, 1.0):
        assert bool((act & (t == val)).any()), val
    assert bool((act & (t == 0.5) & D.far).any())
    # a 45-degree edge: the x pair takes it, the y pair refuses it with everything else in favour
    i, j = _pair_index(D, 21, 3, 0), _pair_index(D, 22, 3, 1)
    assert bool((act[i] & (aLd[i] == aLo[i])).any()) and bool(((aLd[j] == aLo[j]) & extent[j] & rest[j] & ~act[j]).any())
    # an end of the edge exactly on the axis: counted at one end, not at the other
    i, j = _pair_index(D, 4, 12, 0), _pair_index(D, 4, 16, 0)
    on_axis = (E['ya'].v == 0) | (E['yb'].v == 0)
    assert bool((on_axis[i] & (aLd[i] >= aLo[i]) & rest[i] & ~extent[i]).any()) and bool((on_axis[j] & act[j]).any())
    has = ((D.sil[pr.b, pr.tau][:, None] >> torch.arange(3)[None]) & 1).bool()
    assert bool((has & (E['Ld'].v == 0)).any())                                                  # an edge parallel to the axis
    i = _pair_index(D, 10, 12, 0)
    r = inp['rast'][0]
    assert r[12, 10, 3] > 0 and r[12, 11, 3] > 0 and r[12, 10, 2] == r[12, 11, 2] and not bool(pr.use1[i]) and bool(act[i].any())
    hit = act.any(1)
    ids = r[..., 3]
    id0, id1 = ids[pr.y0, pr.x0], ids[pr.y1, pr.x1]
    assert bool((hit & (id0 == 0)).any()) and bool((hit & (id1 == 0)).any())                    # an empty pixel on either side
    assert int(act.sum(1).max()) >= 2                                                            # two edges of one triangle on one pair
    assert int(_pairs_per_receiver(D)[14 * 32 + 20]) == 4                                        # (20, 14) receives from all four pairs
    assert ids[12, 26] == T + 1 and ids[12, 25] > 0 and r[12, 26, 2] < r[12, 25, 2]              # the nearer id T + 1: no triangle
    assert _pair_index(D, 25, 12, 0) is None and _pair_index(D, 26, 12, 0) is None
    # the quad's diagonal is interior (no bit, no blend although it crosses between the centres); folded it is a silhouette
    adj = inp['adj']
    tq = int(ids[23, 6]) - 1
    assert int((adj[tq] >= 0).sum()) == 1 and int(D.sil[0, tq]) == 7 - (1 << int((adj[tq] >= 0).nonzero()[0])) and int(D.sil[0, tq + 1]) in (3, 5, 6)
    i = _pair_index(D, 5, 23, 0)
    assert i is not None and not bool(act[i].any()) and ids[23, 5] == tq + 2
    tf = int(ids[23, 14]) - 1
    assert int(D.sil[0, tf]) == 7 and int((adj[tf] >= 0).sum()) == 1
    i = _pair_index(D, 13, 23, 0)
    assert bool(act[i, int((adj[tf] >= 0).nonzero()[0])])
    return D.ei.numel()


def check_structure(name, inp, ref):
    """The condition that makes a case reach its branch."""
    c, D = _case(name), ref['D']
    B, H, W = R.SHAPES[c['geom']]
    pr = D.pairs
    assert tuple(inp['rast'].shape) == (B, H, W, 4) and inp['color'].shape[-1] == c['C']
    assert int(inp['tri'].min()) >= 0 and int(inp['tri'].max()) < D.V and bool(torch.isfinite(inp['pos']).all())
    ids = inp['rast'][..., 3]
    assert int(ids.max()) <= D.T + 1 and int(ids.min()) >= 0
    b, x0, y0, d = _blended(D)
    xp, yp = d == 0, d == 1
    if c['geom'] in ('soup', 'range'):
        assert int((xp & (x0 == 63)).sum()) >= 1, 'no blended pair at columns 63 | 64'
        assert int((yp & (y0 == 7)).sum()) >= 1 and int((yp & (y0 == 31)).sum()) >= 1, 'rows 7 | 8 and 31 | 32'
        assert int((y0 == 0).sum()) >= 1 and int(((y0 + yp.long()) == H - 1).sum()) >= 1, 'first and last row'
        assert int((x0 == 0).sum()) >= 1 and int(((x0 + xp.long()) == W - 1).sum()) >= 1, 'first and last column'
        assert int(_pairs_per_receiver(D).max()) >= 2
        i0, i1 = ids[pr.b, pr.y0, pr.x0], ids[pr.b, pr.y1, pr.x1]
        hit = D.active.any(1)
        assert int((hit & (i0 > 0) & (i1 > 0)).sum()) >= 50 and int((hit & ((i0 == 0) | (i1 == 0))).sum()) >= 100
        assert all(int((b == k).sum()) >= 100 for k in range(B))
        assert bool((inp['adj'] == -1).all())
    if c['geom'] == 'range':
        assert inp['pos'].dim() == 2 and D.range_mode and not torch.equal(inp['rast'][0], inp['rast'][1])
    if c['geom'] == 'mesh':
        assert B % 2 == 1 and bool((inp['adj'] >= 0).all())
        assert not torch.equal(D.sil[0], D.sil[1]) and not torch.equal(D.sil[1], D.sil[2]) and not torch.equal(D.sil[0], D.sil[2])
        assert all(0 < int((D.sil[k] != 0).sum()) < D.T for k in range(B)) and all(int((b == k).sum()) >= 20 for k in range(B))
        i0, i1 = ids[pr.b, pr.y0, pr.x0], ids[pr.b, pr.y1, pr.x1]
        assert pr.n_id_pairs > 2 * pr.n and int(((i0 > 0) & (i1 > 0)).sum()) >= 1
    if c['geom'] == 'wide':
        assert D.flags.shape[-1] == 5 and W % 64 == 3 and W % 4 != 0
        assert int((xp & (x0 == 255)).sum()) >= 3 and int((xp & (x0 == 257)).sum()) >= 3 and int((xp & (x0 == 63)).sum()) >= 1
        assert int((yp & (y0 == 7)).sum()) >= 1
    if c['boost'] != 1.0:
        assert inp['boost'] == 3.0 and torch.equal(inp['color'], R.case_inputs('soup/C3')['color']) and torch.equal(inp['dy'], R.case_inputs('soup/C3')['dy'])
    if c['hint']:
        check_hint(inp, D, B, H, W)
    if c['one_term']:
        terms = R._pos_terms(D, D.E, inp['color'], inp['dy'], 1.0, torch.float32)
        rows = torch.cat([terms[0][terms[4]], terms[1][terms[4]]])
        assert rows.numel() >= 100 and torch.unique(rows).numel() == rows.numel() and inp['n_one_term'] == rows.numel() // 2
    if c['geom'] == 'tiny12':
        assert D.ei.numel() == 1 and int(pr.d[0]) == 0
    if c['geom'] == 'tiny21':
        assert D.ei.numel() == 1 and int(pr.d[0]) == 1
    if c['geom'] == 'tiny11':
        assert pr.n == 0 and int(ids[0, 0, 0]) == 1
    if c['geom'].startswith('copy'):
        assert D.ei.numel() >= 3


def check_hint(inp, D, B, H, W):
    """Blended pairs across the boundary between an occupied and an empty bin, the receiver inside the empty one, from all four
    sides; bins whose plane 1 is off, with what the planted twins put there."""
    h = inp['hint']
    assert h.dtype == torch.uint8 and tuple(h.shape) == (2, B, (H + 31) // 32, (W + 31) // 32)
    assert h[0, 0].tolist() == [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]] and h[1, 0].tolist() == [[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]]
    off0 = R.hint_off_pixels(h, B, H, W).reshape(-1)
    rx, ry, ox, oy = D.er % W, (D.er // W) % H, D.eo % W, (D.eo // W) % H
    across = off0[D.er] & ~off0[D.eo]
    sides = {'x = 32 (column 0 of its bin)': (rx == 32) & (ox == 31), 'x = 31 (column 31)': (rx == 31) & (ox == 32),
             'y = 32 (first rows of its bin)': (ry == 32) & (oy == 31), 'y = 31 (last rows)': (ry == 31) & (oy == 32)}
    for side, m in sides.items():
        n = int(torch.unique(D.er[across & m]).numel())
        print(f"AA {inp['name']} receivers in an empty bin at {side}: {n}")
        assert n >= 8, (inp['name'], side, n)
    off1 = R.plane1_off_pixels(h, B, H, W)
    assert int(off1.sum()) == H * (W - 96) and not bool(inp['rast'][off1].any())
    planted = inp['rast_planted']
    differ = (planted != inp['rast']).any(-1)
    assert bool((differ <= off1).all()) and int(differ.sum()) >= 40 and bool((planted[..., 3][differ] == inp['tri'].shape[0]).all())
    Dp = R.decisions(inp['color'], planted, inp['pos'], inp['tri'], inp['adj'])
    assert Dp.ei.numel() > D.ei.numel()                     # (read without the hint, the planted pixels would blend)
    if inp['empty_color'] is not None:
        assert bool((inp['color'][off1] == inp['empty_color']).all())


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_gpu_case_inputs_and_float32(name):
    inp, ref, r32, k32 = _four(name)
    D = ref['D']
    check_structure(name, inp, ref)
    if inp['dyadic']:
        n = check_ties(inp, ref)
        print(f"AA {name}: {n} active edges, every one exact in float32")
    else:
        m = R.decision_margin(ref)
        print(f"AA {name}: {D.pairs.n} candidate pairs of {D.pairs.n_id_pairs}, {D.ei.numel()} active edges, decision margin {m:.1f} u")
        assert m >= R.GATE_MARGIN, (name, m)
    for k in R.OUTPUTS:
        assert bool((ref[k][1][ref[k][0] != {'out': inp['color'], 'g_color': inp['dy'], 'g_pos': torch.zeros_like(ref['g_pos'][0])}[k].double()] > 0).all()), (name, k)
    rep = lambda k, e, e32, bound: print(f"AA {name} {k} kernel-order float32 e={e:.3f} e32={e32:.3f} bound={bound:.1f}")
    bad = R.failures(inp, ref, r32, k32, k32, rep)
    assert not bad, (name, bad)
    assert not R.failures(inp, ref, r32, k32, {k: r32[k][0] for k in ('g_pos',)}), name
    zeros = R.predicted_equal(D, inp['color'].shape[-1], inp['dy'])
    assert zeros['g_pos'] >= D.V


def test_dispatch_reaches_every_kernel_and_path():
    reached = set()
    for c in R.CASES:
        B, H, W = R.SHAPES[c['geom']]
        ptr = (8 if c['color_off'] else 0, 0, 8 if c['dy'] == 'offset' else 0, 0)
        d = R.dispatch(c['C'], W, c['hint'], ptr, B * H * W * c['C'])
        reached |= {d['fwd'], d['bwd'], ('fill', d['fill'], c['hint']), d['clear']} | set(d['copy'])
        if c['color_off']:
            assert not d['fill'] and R.dispatch(c['C'], W, True)['fill']
    print("AA dispatch:", sorted(map(str, reached)))
    want = {f'k_aa_fwd<{k}>' for k in (0, 1, 3, 4)} | {f'k_aa_bwd_fix<{k}>' for k in (0, 1, 3, 4)} | {('fill', True, True), ('fill', False, True),
            ('fill', False, False), 'memset', 'lane 0', 'f4 unrolled', 'f4 tail', 'remainder', 'memcpy'}
    assert want <= reached, want - reached
    assert R.dispatch(3, 7, False, (), 105)['copy'] == ('f4 tail', 'remainder') and R.dispatch(1, 67, False, (), 2211)['copy'] == ('f4 unrolled', 'f4 tail', 'remainder')
    assert R.dispatch(2, 64, False, (), 4096)['copy'] == ('f4 unrolled',) and R.dispatch(1, 2, False, (), 2)['copy'] == ('remainder',)
    assert R.dispatch(1, 102, True)['fill'] is False and R.dispatch(3, 100, True)['fill'] is False and R.dispatch(1, 100, True, (0, 8))['fill'] is False


# ---------------------------------------------------------------------------------------------------------------------
# 3. mutants: wrong restatements must miss a bar on a named case
# ---------------------------------------------------------------------------------------------------------------------

MUTANTS = [
    ('x_orient_strict', ['ties'], '> instead of >= in the x pair orient test'),
    ('closed_extent', ['ties'], 'an end of the edge on the axis counts at both ends'),
    ('half_is_near', ['ties'], 'near instead of far at t = 1/2'),
    ('z_tie_to_second', ['ties'], 'a z tie given to the second pixel'),
    ('s_dropped', ['soup/C3', 'mesh/B3'], 't = -Lz / Ld'),
    ('hw_hh_swapped', ['soup/C3', 'wide'], 'hw and hh swapped'),
    ('silhouette_ignores_neighbour', ['ties', 'mesh/B3'], 'every edge with a neighbour is a silhouette'),
    ('w_column_without_fxp_fyp', ['soup/C3', 'soup/one-term'], 'the w column of g_pos without the fxp and fyp terms'),
    ('left_partner_lost_at_lane_0', ['soup/C1', 'wide'], 'the left partner lost at lane 0 of a flag word'),
    ('down_partner_lost_at_row_8k', ['soup/C2', 'wide'], 'the down partner lost at row 8 k'),
    ('empty_bin_blend_dropped', ['hint/W100/C1', 'hint/W102/C1/empty', 'hint/W100/C3'], 'the blend into an empty bin that faces an occupied one dropped'),
    ('other_pixel_wrong_sign', ['soup/C4', 'tiny/2x1'], "g_color of the 'other' pixel with the wrong sign"),
    ('boost_on_g_color', ['boost'], 'boost applied to g_color'),
    ('remainder_of_g_color_unwritten', ['copy/105', 'copy/2211', 'tiny/1x2'], 'the nfl & 3 floats at the end of g_color left unwritten'),
]


@pytest.mark.parametrize("mutant,names,what", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutants_are_caught(mutant, names, what, monkeypatch):
    for name in names:
        inp, ref, r32, k32 = _four(name)
        monkeypatch.setattr(R, 'MUTANT', mutant)
        got = R.kernel_order(inp, hint=inp['hint'])
        monkeypatch.setattr(R, 'MUTANT', None)
        hit = R.failures(inp, ref, r32, k32, got)
        l2 = max(R.rel_l2(got[k], k32[k]) for k in R.OUTPUTS)
        print(f"AA mutant {mutant} ({what}) on {name}: rel-L2 {l2:.2e}: {[h[:2] for h in hit]}")
        assert hit, (mutant, name)
        assert any(h[1] != 'not bit-identical to float32_in_kernel_order' for h in hit), (mutant, name, 'only the bit-identity sees it')
        assert not R.failures(inp, ref, r32, k32, k32)            # (the unmutated one passes)
    assert len(MUTANTS) >= 10

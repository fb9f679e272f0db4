"""CPU: the float64 yardstick of the one-pass pixel objective's MIP branch (tests/objective_ref.py with mip_levels: k_shade_mip_list/_queue,
k_fix_mip_list/_queue, mip_lookup_fwd/_bwd, _build_mips / _fold_mip_grads) is right, and what tests/test_gpu_objective_mip_ref.py asks of
the kernels is reachable and discriminates:
  1. on the inputs of every GPU case the statement's value and hand-written gradients equal float64 torch.autograd through the oracle's
     rasterize (rast_db) -> interpolate(diff_attrs='all') -> texture('linear-mipmap-linear', max_mip_level) -> antialias and the composite
     with the background, to 1e-12 of the entry's scale (the tolerance of test_objective_ref.py);
  2. every case reaches the path its name promises (objective_ref.plan's restatement of the prepass, place() and the routing, counts
     printed), no float32 choice -- the level's two clamps, floor(level), the tap cells of both levels among them -- lies within
     GATE_MARGIN u of flipping, and the float32 evaluation by torch meets every bar the GPU is held to;
  3. `mip/magnified/C1/wrap`: on the inputs of `magnified/C1/wrap` every level clamps at 0, and the mip statement IS the non-mip one (same
     values, same scales): the GPU file holds that call to the established reference;
  4. six wrong restatements each miss a bar on a named case.  The level's gate is ignored at BOTH ends there: at the top level alone no
     bar can see it (l1 == l0, so c1 - c0 and with it gfl are exactly 0 whatever the gate says); `mip/top` has a group clamped at level 0
     for it.  A seventh -- the blended pixel's tu from a recomputed u in place of the float32 u that k_shade stores in the record -- no bar
     can see either: the statement is evaluated in ONE dtype throughout (the float64 reference
     has no float32 record to read), and the difference between the two is one rounding of u, which every entry's scale S already carries.
     The statement therefore forms the blended pixel's (tu, tv) like k_shade's, as the non-mip statement does.
Lines "OBJMIP ..." are printed under pytest -s."""
import functools

import numpy as np
import pytest
import torch

import objective_ref as R
import texture_ref as TR


@functools.lru_cache(maxsize=None)
def _three(name, oracle_ops):
    inp = R.case_inputs(name, oracle_ops)
    return inp, R.reference(inp), R.reference(inp, torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the statement against autograd through the oracle
# ---------------------------------------------------------------------------------------------------------------------

def _oracle(inp, ref, oracle_ops):
    leaf = lambda t: t.detach().double().requires_grad_(True)
    pos, tex = leaf(inp['pos']), leaf(inp['tex'])
    H, W = inp['res']
    rast, rast_db = oracle_ops.rasterize(pos, inp['tri'], (H, W), ids=inp['ids'])
    uv, uv_da = oracle_ops.interpolate(inp['uv'].double()[None], rast, inp['uv_tri'], rast_db=rast_db, diff_attrs='all')
    col = oracle_ops.texture(tex[None], uv, uv_da, filter_mode='linear-mipmap-linear', boundary_mode=inp['boundary'],
                             max_mip_level=inp['max_mip_level'])
    col = oracle_ops.antialias(col, rast, pos, inp['tri'])
    img = torch.where(rast[..., 3:] > 0, col * 255.0, torch.tensor(ref['bgs'], dtype=torch.float64))
    total = ((inp['ref_u8'].double()[..., None] - img) ** 2).sum()
    (total * float(np.float32(1.0 / ref['n_total']))).backward()      # (the kernels are handed 1 / n_total as a float32 number)
    return {'value': total.detach() / ref['n_total'], 'g_pos': pos.grad, 'g_tex': tex.grad}


@pytest.mark.parametrize("name", R.MIP_CASE_IDS)
def test_statement_equals_autograd_through_the_oracle(name, oracle_ops):
    inp, ref, _ = _three(name, oracle_ops)
    got = _oracle(inp, ref, oracle_ops)
    for k in ('value',) + R.OUTPUTS:
        r, S = ref[k]
        assert r.shape == got[k].shape, (name, k)
        assert bool((got[k][S == 0] == 0).all()), (name, k, 'the oracle has a term where the statement has none')
        worst = float(((r - got[k]).abs() / S.clamp(min=1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0
        print(f"OBJMIP {name} {k} statement vs float64 autograd: {worst:.2e} of the scale")
        assert worst <= 1e-12, (name, k, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the cases
# ---------------------------------------------------------------------------------------------------------------------

def check_plan(name, inp, pl, ref):
    """The path each case exists for, on objective_ref.plan's restatement of the prepass, place() and the routing."""
    mb = pl['mipbins']
    lk = ref['st'].lk
    C, nl = inp['tex'].shape[2], inp['mip_levels']
    raw, frac = lk.raw.v, lk.raw.v - torch.floor(lk.raw.v)
    placed = [v for v in mb.values() if v['mlb'] is not None]
    to_window = lambda v, l: v['levels'].get(l, [0, 0])[0]
    to_memory = lambda v, l: v['levels'].get(l, [0, 0])[1]
    if name.startswith('mip/mid') or name in ('mip/span', 'mip/top', 'mip/no-levels', 'mip/overflow/C3'):
        # one level per triangle, its fraction in [0.2, 0.8] or the level clearly beyond a clamp
        free = lk.passes
        assert bool(((frac[free] > 0.19) & (frac[free] < 0.81)).all()) and bool(((raw[~free] < -0.2) | (raw[~free] > nl + 0.2)).all())
        for t in torch.unique(ref['st'].px.t).tolist():
            r_ = raw[ref['st'].px.t == t]
            assert float(r_.max() - r_.min()) < 1e-6, (name, t)
    if name == 'mip/mid/C1/wrap/seam':
        assert nl == 3 and lk.dims[-1] == (2, 3)
        assert any(v['shifted'][0] or v['shifted'][1] for v in placed) and any(v['wrap'][0] for v in placed) and any(v['wrap'][1] for v in placed)
        assert set(torch.unique(lk.l0).tolist()) == {1}
    if name in ('mip/mid/C3/clamp', 'mip/mid/C4/zero'):
        assert nl == 5 and set(torch.unique(lk.l0).tolist()) == {0, 2}
        if name.endswith('clamp'):
            assert int((lk.mu == 0).sum()) >= 16 and int((lk.mv == 0).sum()) >= 16
        else:      # taps with corners in the padding at the lower and at the upper level
            for which in (3, 4):
                assert any(bool((sum((~v).long() for v in g[which].valid) > 0).any()) for g in lk.groups)
    if name == 'mip/span':
        assert nl == 6 and set(torch.unique(lk.l0).tolist()) == {0, 1, 2, 3, 4}
        wide = [v for v in placed if any(l >= v['mlb'] + 3 and to_memory(v, l) > 0 for l in v['levels'])]
        assert wide, 'no bin whose levels span more than the three windows'
        assert any(all(to_window(v, v['mlb'] + j) > 0 for j in range(3)) for v in wide)
        assert any(v['below_mlb'] > 0 and v['mlb'] >= 1 and to_memory(v, 0) > 0 for v in placed), 'no finest-level pixel off the pass-0 rows'
    if name == 'mip/top':
        assert nl == 4 and lk.dims[-1] == (1, 1) and set(torch.unique(lk.l0).tolist()) == {0, 3, 4} and bool(lk.lo.any())
        assert bool(lk.hi.any()) and bool((lk.l1[lk.hi] == lk.l0[lk.hi]).all()) and bool((lk.l0[lk.hi] == 4).all())
    if name == 'mip/no-levels':
        assert nl == 0 and not bool(lk.passes.any()) and len(lk.dims) == 1
    if name == 'mip/overflow/C3':
        assert R.MIP_WIN_CELLS[C][0] == 1088
        big = [v for v in placed if not v['windows'][0]['fits']]
        assert big and all(v['windows'][0]['box'][0] * v['windows'][0]['box'][1] > 1088 for v in big)
        assert any(to_window(v, 0) > 0 and to_memory(v, 0) > 0 for v in big)
    if name == 'mip/perspective':
        px = ref['st'].px
        for t in torch.unique(px.t).tolist():
            r_ = raw[px.t == t]
            assert 0.05 < float(r_.max() - r_.min()) < 0.4 and 1.0 < float(r_.min()) and float(r_.max()) < 2.0, (name, t, float(r_.min()), float(r_.max()))
        w = inp['pos'][..., 3].reshape(inp['pos'].shape[0], -1, 3)
        assert bool((w.max(-1).values / w.min(-1).values <= 1.3).all()) and bool((w.max(-1).values / w.min(-1).values > 1.05).all())
    if name == 'mip/islands/zero':
        cov, D = ref['cov'], ref['D']
        assert pl['pairs'] > 0 and bool((~(cov[D.er] & cov[D.eo])).all()) and pl['empty_partner'] > 0
        s = R._structure(inp)
        lk0 = ref['st'].lk0
        for k in range(4):      # the taps of (0, 0) hold the empty pixels' share alone
            assert bool((s['count'][lk0.flat[k][lk0.valid[k]]] == 0).all())
    if name.startswith('mip/tiny'):
        assert inp['res'][0] * inp['res'][1] <= 2


@pytest.mark.parametrize("name", R.MIP_CASE_IDS)
def test_cases_reach_their_paths_and_float32_meets_the_bars(name, oracle_ops):
    inp, ref, r32 = _three(name, oracle_ops)
    pl = R.plan(inp)
    m = R.decision_margin(inp, ref)
    lk = ref['st'].lk
    mb = pl['mipbins']
    tot = {}
    for v in mb.values():
        for l, (a, b) in v['levels'].items():
            tot.setdefault(l, [0, 0])
            tot[l][0] += a
            tot[l][1] += b
    print(f"OBJMIP {name} pixels {ref['st'].px.n} levels 0..{inp['mip_levels']} l0 {sorted(torch.unique(lk.l0).tolist())} clamped low {int(lk.lo.sum())} high {int(lk.hi.sum())} "
          f"deferred {pl['deferred']} hit {pl['hit']} pairs {pl['pairs']} empty partners {pl['empty_partner']} bins {len(mb)} "
          f"mlb {sorted(set(v['mlb'] for v in mb.values() if v['mlb'] is not None))} windows that do not fit {sum(not w['fits'] for v in mb.values() for w in v['windows'] if w)} "
          f"w?wrap {[sum(v['wrap'][j] for v in mb.values()) for j in range(3)]} shifted {sum(v['shifted'][0] or v['shifted'][1] for v in mb.values())} "
          f"tap sets per level (window, memory) {dict(sorted(tot.items()))} below mlb {sum(v['below_mlb'] for v in mb.values())} worst margin {m:.0f} u")
    assert m >= R.GATE_MARGIN, (name, m)
    assert bool((r32['dd'] != 0).all()) and bool((ref['dd'] != 0).all()) and bool((r32['dn'] != 0).all())
    check_plan(name, inp, pl, ref)
    got = {'value': r32['value'][0], 'g_tex': r32['g_tex'][0], 'g_pos': r32['g_pos'][0]}
    assert R.failures(inp, ref, r32, got) == []
    for k in R.OUTPUTS:
        for row, e32 in R.measure_rows(r32[k][0], ref, k):
            print(f"OBJMIP {name} {row} e32 {e32:.3f} bound {8 * e32 + 4:.2f}")
    n = R.n_value(inp['tex'].shape[2], pl['max_deferred'], True)
    print(f"OBJMIP {name} value e32 {R.value_error(r32['value'][0], ref):.3f} bound {n + 2}")


def test_the_result_does_not_depend_on_the_plan(oracle_ops, monkeypatch):
    inp, ref, _ = _three('mip/tiny/1x2', oracle_ops)
    monkeypatch.setattr(R, '_plan_mip_bin', None)
    again = R.evaluate(inp)
    for k in ('value',) + R.OUTPUTS:
        assert torch.equal(again[k][0], ref[k][0]) and torch.equal(again[k][1], ref[k][1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the magnified call: every level clamps at 0, and the mip statement is the established one
# ---------------------------------------------------------------------------------------------------------------------

def test_magnified_mip_statement_is_the_non_mip_statement(oracle_ops):
    plain = R.case_inputs('magnified/C1/wrap', oracle_ops)
    inp = R.with_mip(plain, 0)
    assert inp['mip_levels'] == 0 and TR.num_levels(256, 256) == 8
    ref, base = R.reference(inp), R.reference(plain)
    lk = ref['st'].lk
    assert bool(lk.hi.all()) and not bool(lk.passes.any()) and bool((lk.l0 == 0).all()) and bool((lk.fl.v == 0).all()) and bool((lk.fl.S == 0).all())
    assert 1.5 < float(lk.raw.v.min()) and float(lk.raw.v.max()) < 1.7      # 3 texels a pixel: log2 3 = 1.58, far above the clamp at max_mip_level = 0
    raw32 = R.reference(inp, torch.float32)['st'].lk.raw.v
    assert 1.5 < float(raw32.min()) and float(raw32.max()) < 1.7
    # (this footprint is isotropic: df = bq = 0, rt cancels completely and texture_ref's L_s, which divides by rt, has no bound for the level;
    #  the clamp is decided a level and a half away all the same -- rt cannot be off by more than sqrt of its argument's error, 1e-3 of l2 = 9.
    #  Every OTHER choice is the non-mip statement's, held to GATE_MARGIN there.)
    m = R.margins(inp, ref)
    lv = ref['st'].lk
    others = [q for q in lv.gates if not any(q is g for g in lv.level_gates)]
    assert all(bool((q.v > R.GATE_MARGIN * R.U * q.S).all()) for q in others) and min(float(m[k].min()) for k in ('edge', 'sil', 'z')) >= R.GATE_MARGIN
    assert all(bool((g == 0).all()) and bool((s == 0).all()) for g, s in ref['levels'][1:])      # the coarser levels' gradients: no term
    for k in ('value',) + R.OUTPUTS:
        assert torch.equal(ref[k][0], base[k][0]) and torch.equal(ref[k][1], base[k][1]), k
    r32, b32 = R.reference(inp, torch.float32), R.reference(plain, torch.float32)
    for k in ('value',) + R.OUTPUTS:      # float32: (gq * (1 - 0)) * w_k is gq * w_k bit for bit
        assert torch.equal(r32[k][0], b32[k][0]), k
    assert torch.equal(R.predicted_zeros(inp)['g_tex'], R.predicted_zeros(plain)['g_tex'])
    assert torch.equal(R.predicted_zeros(inp)['g_pos'], R.predicted_zeros(plain)['g_pos'])


# ---------------------------------------------------------------------------------------------------------------------
# 4. wrong restatements miss a bar
# ---------------------------------------------------------------------------------------------------------------------

MUTANTS = {
    'gda_dropped': 'mip/perspective',
    'dudy_and_dvdx_swapped_in_da': 'mip/perspective',
    'level_from_Wt_alone': 'mip/mid/C1/wrap/seam',
    'fold_weight_half': 'mip/mid/C3/clamp',
    'fl_and_1_minus_fl_exchanged': 'mip/mid/C4/zero',
    'level_gate_ignored': 'mip/top',
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_restatement_misses_a_bar(mutant, oracle_ops, monkeypatch):
    name = MUTANTS[mutant]
    inp, ref, r32 = _three(name, oracle_ops)
    monkeypatch.setattr(R, 'MUTANT', mutant)
    wrong = R.evaluate(inp, torch.float32)
    monkeypatch.setattr(R, 'MUTANT', None)
    got = {'value': wrong['value'][0], 'g_tex': wrong['g_tex'][0], 'g_pos': wrong['g_pos'][0]}
    missed = R.failures(inp, ref, r32, got)
    print(f"OBJMIP mutant {mutant} on {name}: {missed[:3]}")
    assert missed, (mutant, name)

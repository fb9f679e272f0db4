"""CPU: the float64 statement of the WEIGHTED one-pass objective (tests/objective_ref.py, inp['weights']; DESIGN.md 3, "Weighted objective
rule") is right, and what tests/test_gpu_objective_weighted_ref.py asks of the weighted kernels is reachable and discriminates:
  1. on every weighted case and under every option set of objective_ref.WEIGHT_SETS the statement's value, its hand-written gradients and
     wsum equal float64 torch.autograd through the oracle's rasterize -> interpolate -> texture -> antialias, the composite with the background
     and robust_ref.loss_plain(weight = robust_ref.weights(...)), to 1e-12 of the entry's scale (the figure is printed);
  2. the float32 evaluation by torch meets every bar the GPU is held to, and the weights reach what they exist for (REACH below, conditions on
     ids and weights; what a case cannot reach by its geometry is named in NOT_REACHABLE with the reason, and asserted NOT to occur);
  3. with neutral weights (L2, no mask, no face weights, w_outside = 1, sat = 0) the weighted statement IS the plain one: value, gradients and
     their scales' zeros equal in float64 and bit for bit in float32, and wsum is the number of entries;
  4. ten wrong restatements each miss a bar on a named case.
What no bar can see, and so has no mutant: inside the k_fix<0> line (w rho(dn) - w0 rho(d0)) - (w rho(dd) - w0 rho(d0)) the pair w0 rho(d0) cancels,
so any w0 or any rho(d0) there gives the same value to within a rounding of the sum; the bars on the value see a wrong term, not a lost bit.
Likewise k_shade's - w0 rho(d0) and the background share's + w0 rho(d0) of a covered pixel cancel in the value whatever w0 rho(d0) is, as long as
both use the same: only a share that weighs covered pixels differently (the mutant below) is seen.
Lines "WOBJREF ..." are printed under pytest -s."""
import numpy as np
import pytest
import torch

import objective_ref as R
import robust_ref as RB

TAGS = R.WEIGHT_TAGS


def _three(name, tag, oracle_ops):      # (objective_ref caches a few weighted references at a time: ninety variants are not kept)
    inp = R.with_weights(R.case_inputs(name, oracle_ops), tag)
    return inp, R.reference(inp), R.reference(inp, torch.float32)


def _got(r):
    return {'value': r['value'][0], 'g_tex': r['g_tex'][0], 'g_pos': r['g_pos'][0], 'wsum': r['wsum'][0]}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the statement against autograd through the oracle
# ---------------------------------------------------------------------------------------------------------------------

def _chain(name, oracle_ops):
    """The oracle's four operators on the case in float64, once for all its option sets, the graph kept: (pos, tex, rast, composited image in
    colour units)."""
    inp = R.case_inputs(name, oracle_ops)
    leaf = lambda t: t.detach().double().requires_grad_(True)
    pos, tex = leaf(inp['pos']), leaf(inp['tex'])
    rast, _ = oracle_ops.rasterize(pos, inp['tri'], inp['res'], ids=inp['ids'])
    uv, _ = oracle_ops.interpolate(inp['uv'].double()[None], rast, inp['uv_tri'])
    col = oracle_ops.texture(tex[None], uv, filter_mode='linear', boundary_mode=inp['boundary'])
    col = oracle_ops.antialias(col, rast, pos, inp['tri'])
    # (255 * (45 / 255) is 45 to a rounding of float64; loss_plain's own background is the float32 number, which the kernels are not handed)
    img = torch.where(rast[..., 3:] > 0, col, torch.tensor(45.0 / 255.0, dtype=torch.float64))
    return pos, tex, rast, img


@pytest.mark.parametrize("name", R.WEIGHTED_CASE_IDS)
def test_weighted_statement_equals_autograd_through_the_oracle(name, oracle_ops):
    pos, tex, rast, img = _chain(name, oracle_ops)
    everywhere = torch.ones(rast.shape[:3])
    for tag in TAGS:
        inp, ref, _ = _three(name, tag, oracle_ops)
        assert ref['bgs'] == ref['b'] == 45.0
        wt = inp['weights']
        w64, _ = RB.weights(rast[..., 3], inp['ref_u8'], wt['mask'], wt['face_weights'], wt['weight_outside'], wt['saturation'])
        total = RB.loss_plain(img, everywhere, inp['ref_u8'], wt['kind'], wt['c'], n_total=1, weight=w64)
        gp, gt = torch.autograd.grad(total * float(np.float32(1.0 / ref['n_total'])), (pos, tex), retain_graph=True)
        C = inp['tex'].shape[2]
        got = {'value': total.detach() / ref['n_total'], 'g_pos': gp, 'g_tex': gt, 'wsum': float(C) * w64.sum()}
        for k in ('value', 'wsum') + R.OUTPUTS:
            r, S = ref[k]
            assert r.shape == got[k].shape, (name, tag, k)
            assert bool((got[k][S == 0] == 0).all()), (name, tag, k, 'the oracle has a term where the statement has none')
            worst = float(((r - got[k]).abs() / S.clamp(min=1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0
            print(f"WOBJREF {name} {tag} {k} statement vs float64 autograd: {worst:.2e} of the scale")
            assert worst <= 1e-12, (name, tag, k, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the float32 evaluation meets the bars; the weights reach what they exist for
# ---------------------------------------------------------------------------------------------------------------------

REACH = ('blended pixels of weight 0 and of positive weight',
         'a blend entry of two covered pixels: receiver of weight 0, partner weighted',
         'a blend entry of two covered pixels: receiver weighted, partner of weight 0',
         'a weighted receiver with an empty partner (esum != 0)',
         'texels under pixels of weight 0 only',
         'saturated pixels that are covered',
         'residuals of weighted pixels below, near and above c = 2 and c = 20')
# what a case cannot reach by its geometry: condition -> why.  Asserted not to occur, so that a changed case is noticed.
_ISLANDS = {REACH[1]: 'separated triangles on an empty frame: no blend entry has two covered pixels',
            REACH[2]: 'separated triangles on an empty frame: no blend entry has two covered pixels'}
_ONE_PIXEL = 'one pixel, one triangle (face 0, weight 0), no pair'
_MESH = 'a convex closed mesh: its only silhouette lies against the empty frame, no blend entry has two covered pixels'
NOT_REACHABLE = {
    'islands/wrap': _ISLANDS, 'islands/clamp': _ISLANDS,
    'mesh/B3': {REACH[1]: _MESH, REACH[2]: _MESH, REACH[4]: 'a 4 x 4 texture under thousands of pixels: every texel has hundreds of terms'},
    'tiny/1x1': {c: _ONE_PIXEL for c in REACH[:4] + REACH[5:]},
}


def reach(inp, ref):
    """-> {condition: bool} on a case under the full option set (objective_ref.WEIGHT_SETS['.../all']), from ids, weights and the statement's dd."""
    D, cov, rowof = ref['D'], ref['cov'], ref['rowof']
    P = cov.numel()
    w = torch.zeros(P, dtype=torch.float64)
    w[ref['pix']] = ref['w']
    er, eo = D.er, D.eo
    rc = cov[er]
    both = rc & cov[eo]
    w_hit = w[ref['hit']]
    base = R._case_cache[inp['base']]
    plain_count, count = R._structure(base)['count'], R._structure(inp)['count']
    lk0 = ref['st'].lk0
    under = plain_count > 0
    if int((rc & ~cov[eo]).sum()):      # (the taps of uv = (0, 0) hold the empty pixels' share)
        for k in range(4):
            under[lk0.flat[k][lk0.valid[k]]] = False
    sat = inp['ref_u8'].reshape(-1)[ref['pix']] >= inp['weights']['saturation']
    d = ref['dd'][ref['w'] > 0].abs().reshape(-1)
    spread = all(bool((d < c / 2).any()) and bool(((d >= c / 2) & (d <= 2 * c)).any()) and bool((d > 2 * c).any()) for c in RB.SCALES)
    return {REACH[0]: bool((w_hit == 0).any()) and bool((w_hit > 0).any()),
            REACH[1]: bool((both & (w[er] == 0) & (w[eo] > 0)).any()),
            REACH[2]: bool((both & (w[er] > 0) & (w[eo] == 0)).any()),
            REACH[3]: bool((rc & ~cov[eo] & (w[er] > 0)).any()) and R._structure(inp)['n_esum'] > 0,
            REACH[4]: bool((under & (count == 0)).any()),
            REACH[5]: bool(sat.any()) and bool((~sat).any()),
            REACH[6]: spread}


@pytest.mark.parametrize("name", R.WEIGHTED_CASE_IDS)
def test_float32_meets_the_bars_and_the_weights_reach(name, oracle_ops):
    for tag in TAGS:
        inp, ref, r32 = _three(name, tag, oracle_ops)
        k32 = R.float32_in_kernel_order(inp)
        assert bool((r32['dd'] != 0).all()) and bool((ref['dd'] != 0).all()) and bool((r32['dn'] != 0).all())
        assert R.failures(inp, ref, r32, _got(r32), k32) == [], (name, tag)
        zeros = R.predicted_zeros(inp)
        plain_zeros = R.predicted_zeros(R._case_cache[inp['base']])
        print(f"WOBJREF {name} {tag} weights 0 / covered {int((ref['w'] == 0).sum())} / {ref['w'].numel()}, exact zeros g_tex {int(zeros['g_tex'].sum())} "
              f"(plain {int(plain_zeros['g_tex'].sum())}) g_pos {int(zeros['g_pos'].sum())} (plain {int(plain_zeros['g_pos'].sum())}), "
              f"one-term texels {k32['texel'].numel()}")
        for k in R.OUTPUTS + ('wsum',):
            for row, e32 in R.measure_rows(r32[k][0], ref, k):
                print(f"WOBJREF {name} {tag} {row} e32 {e32:.3f} bound {8 * e32 + 4:.2f}")
        print(f"WOBJREF {name} {tag} value e32 {R.value_error(r32['value'][0], ref):.3f} bound {R.value_count(inp) + 2}")
    inp, ref, _ = _three(name, 'charbonnier20/all', oracle_ops)
    got = reach(inp, ref)
    absent = NOT_REACHABLE.get(name, {})
    for cond in REACH:
        print(f"WOBJREF {name} reach: {cond}: {got[cond]}" + (f" ({absent[cond]})" if cond in absent else ""))
        assert got[cond] == (cond not in absent), (name, cond)
    # the mask's special bytes lie on covered pixels, a fifth of the face weights is 0, some are above 1
    cw = R.case_weights(R._case_cache[inp['base']])
    bytes_ = set(cw['mask'].reshape(-1)[ref['pix']].tolist())
    assert {254} <= bytes_ and (name.startswith('tiny') or {0, 1, 254, 255} <= bytes_), (name, sorted(bytes_)[:4])
    fw = cw['face_weights']
    assert float(fw[0]) == 0.0 and (fw.numel() < 20 or (0.05 < float((fw == 0).float().mean()) < 0.4 and bool((fw > 1).any())))


# ---------------------------------------------------------------------------------------------------------------------
# 3. neutral weights
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", R.WEIGHTED_CASE_IDS)
def test_neutral_weights_are_the_plain_statement(name, oracle_ops):
    base = R.case_inputs(name, oracle_ops)
    inp = R.with_weights(base, 'neutral')
    for dtype in (torch.float64, torch.float32):
        plain, w = R.reference(base, dtype), R.reference(inp, dtype)
        for k in ('value',) + R.OUTPUTS:
            assert torch.equal(w[k][0], plain[k][0]), (name, dtype, k)
            assert torch.equal(w[k][1] == 0, plain[k][1] == 0), (name, dtype, k)
        assert torch.equal(w['gq'], plain['gq'])
        assert float(w['wsum'][0]) == float(base['ref_u8'].numel() * base['tex'].shape[2])
    k_plain, k_w = R.float32_in_kernel_order(base), R.float32_in_kernel_order(inp)
    assert torch.equal(k_plain['texel'], k_w['texel']) and torch.equal(k_plain['g_tex'], k_w['g_tex'])
    for k, z in R.predicted_zeros(base).items():
        assert torch.equal(z, R.predicted_zeros(inp)[k]), (name, k)


# ---------------------------------------------------------------------------------------------------------------------
# 4. wrong restatements miss a bar
# ---------------------------------------------------------------------------------------------------------------------

MUTANTS = {
    'w0_for_a_covered_pixel': ('soup/C3/clamp', 'charbonnier20/all'),
    'face_weight_of_id': ('soup/C4/zero', 'geman20/all'),
    'saturation_as_greater': ('borders', 'charbonnier20/w0,sat'),
    'partner_weight_in_k_fix0': ('soup/C1/wrap/seam', 'geman2/all'),
    'unweighted_gq_taken_away_in_k_fix1': ('soup/C1/wrap/seam', 'l2/all'),
    'psi_without_s': ('islands/wrap', 'charbonnier20/all'),
    'charbonnier_rho_without_2': ('soup/C3/clamp', 'charbonnier2/all'),
    'background_share_weighted_by_w': ('islands/clamp', 'geman20/all'),
    'wsum_without_minus_w0': ('mesh/B3', 'charbonnier2/all'),
    'no_esum_share': ('islands/wrap', 'l2/all'),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_weighted_restatement_misses_a_bar(mutant, oracle_ops, monkeypatch):
    name, tag = MUTANTS[mutant]
    inp, ref, r32 = _three(name, tag, oracle_ops)
    k32 = R.float32_in_kernel_order(inp)
    monkeypatch.setattr(R, 'MUTANT', mutant)
    wrong = R.evaluate(inp, torch.float32)
    monkeypatch.setattr(R, 'MUTANT', None)
    missed = R.failures(inp, ref, r32, _got(wrong), k32)
    print(f"WOBJREF mutant {mutant} on {name} {tag}: {missed[:3]}")
    assert missed, (mutant, name, tag)
    if mutant == 'wsum_without_minus_w0':
        assert [m[0] for m in missed] == ['wsum'], missed
    if mutant == 'saturation_as_greater':      # the captures AT the level: a handful of pixels
        n_at = int((inp['ref_u8'].reshape(-1)[ref['pix']] == inp['weights']['saturation']).sum())
        print(f"WOBJREF mutant {mutant}: {n_at} covered pixels at the saturation level of {ref['w'].numel()}")
        assert 0 < n_at

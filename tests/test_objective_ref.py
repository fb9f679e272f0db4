"""CPU: the float64 yardstick of the one-pass pixel objective (tests/objective_ref.py) is right, and what
tests/test_gpu_objective_ref.py asks of the kernels is reachable and discriminates:
  1. on the inputs of every GPU case the statement's value and hand-written gradients equal float64 torch.autograd through the oracle's
     rasterize -> interpolate -> texture -> antialias and the composite with the background, to 1e-12 of the entry's scale;
  2. every case reaches the path it exists for (objective_ref.plan, counts printed), no float32 choice lies within GATE_MARGIN u of
     flipping, dd = 0 does not occur, and the float32 evaluation by torch meets every bar the GPU is held to;
  3. twelve wrong restatements each miss a bar on a named case.  (Ignoring mu / mv is not among them: beyond [0, 1] the clamp puts both taps
     of the axis on one texel, t10 - t00 is exactly 0 and the masked gradient is 0 either way; the statement keeps the masks as the kernels do.)
Lines "OBJ ..." are printed under pytest -s."""
import functools

import numpy as np
import pytest
import torch

import objective_ref as R
from fitstep_ref import U


@functools.lru_cache(maxsize=None)
def _three(name, oracle_ops):
    inp = R.case_inputs(name, oracle_ops)
    return inp, R.reference(inp), R.reference(inp, torch.float32)


bars_missed = R.failures


# ---------------------------------------------------------------------------------------------------------------------
# 1. the statement against autograd through the oracle
# ---------------------------------------------------------------------------------------------------------------------

def _oracle(inp, ref, oracle_ops):
    leaf = lambda t: t.detach().double().requires_grad_(True)
    pos, tex = leaf(inp['pos']), leaf(inp['tex'])
    H, W = inp['res']
    C = inp['tex'].shape[2]
    rast, _ = oracle_ops.rasterize(pos, inp['tri'], (H, W), ids=inp['ids'])
    uv, _ = oracle_ops.interpolate(inp['uv'].double()[None], rast, inp['uv_tri'])
    col = oracle_ops.texture(tex[None], uv, filter_mode='linear', boundary_mode=inp['boundary'])
    col = oracle_ops.antialias(col, rast, pos, inp['tri'])
    img = torch.where(rast[..., 3:] > 0, col * 255.0, torch.tensor(ref['bgs'], dtype=torch.float64))
    total = ((inp['ref_u8'].double()[..., None] - img) ** 2).sum()
    (total * float(np.float32(1.0 / ref['n_total']))).backward()      # (the kernels are handed 1 / n_total as a float32 number)
    return {'value': total.detach() / ref['n_total'], 'g_pos': pos.grad, 'g_tex': tex.grad}


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_statement_equals_autograd_through_the_oracle(name, oracle_ops):
    inp, ref, _ = _three(name, oracle_ops)
    assert ref['bgs'] == ref['b'] == 45.0      # the covered pixels' d0 and the background share use the same number
    got = _oracle(inp, ref, oracle_ops)
    for k in ('value',) + R.OUTPUTS:
        r, S = ref[k]
        assert r.shape == got[k].shape, (name, k)
        assert bool((got[k][S == 0] == 0).all()), (name, k, 'the oracle has a term where the statement has none')
        worst = float(((r - got[k]).abs() / S.clamp(min=1e-300))[S > 0].max()) if bool((S > 0).any()) else 0.0
        print(f"OBJ {name} {k} statement vs float64 autograd: {worst:.2e} of the scale")
        assert worst <= 1e-12, (name, k, worst)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the cases
# ---------------------------------------------------------------------------------------------------------------------

def check_plan(name, inp, pl, k32):
    """The path each case exists for (the table of the issue), on objective_ref.plan."""
    hv, bins = pl['halves'], pl['bins']
    Ht, Wt, C = inp['tex'].shape
    cells = R.OWIN_CELLS[C]
    ref = R.reference(inp)
    D, lk = ref['D'], ref['st'].lk
    most = lambda key: max(v[key] for v in bins.values())
    if name == 'magnified/C1/wrap':
        big = [v for v in hv.values() if not v['fits']]
        assert C == 1 and cells == 1216 and big and all(v['box'][0] * v['box'][1] > cells for v in big)
        assert any(v['inside'] > 0 and v['outside'] > 0 for v in big)
        assert k32['texel'].numel() >= 1000
        # every texel under a pixel outside every blend has exactly one term
        in_blend = torch.zeros(ref['st'].px.n, dtype=torch.bool)
        in_blend[ref['rowof'][ref['hit2']]] = True
        count = R._structure(inp)['count']
        assert all(bool((count[lk.flat[k][~in_blend]] == 1).all()) for k in range(4))
    if name == 'soup/C1/wrap/seam':
        assert (Ht, Wt) == (16, 24) and Wt & (Wt - 1) != 0      # (24 columns: no power of two)
        assert any(v['centred'] for v in hv.values()) and any(v['owrap'] for v in hv.values())
        assert int(R._structure(inp)['count'].max()) > 100
        assert most('hit_vertices') > R.FVS and most('hit_texels') > R.FTS
    if name == 'soup/C3/clamp':
        assert cells == 1600 and int((lk.mu == 0).sum()) >= 16 and int((lk.mv == 0).sum()) >= 16
        assert most('hit_vertices') > R.FVS
    if name == 'soup/C4/zero':
        invalid = sum((~v).long() for v in lk.valid)
        # (validity is a column test AND a row test: exactly one corner outside cannot occur; 0, 2, 3 and 4 do)
        assert set(torch.unique(invalid).tolist()) == {0, 2, 3, 4}
    if name == 'mesh/B3':
        tri = inp['tri'].long()
        assert int(torch.bincount(tri.reshape(-1)).min()) >= 4 and bool((R.choices(inp)['adj'] >= 0).all())      # shared vertices, closed
        assert bool((D.sil[:2] != 0).any())                          # a closed mesh: every silhouette edge is a fold
        assert any(not v['sil'] and k[0] < 2 for k, v in bins.items())                                 # an interior bin: bin_sil false
        assert not bool((inp['ids'][2] != 0).any()) and bool((inp['pos'][2, :, 3] < 0).all())          # the third image: behind the camera
        assert bool(R.predicted_zeros(inp)['g_pos'][2].all())
    if name == 'confetti':
        full = [k for k, v in bins.items() if v['vertices'] > R.VT_SLOTS and v['hit_vertices'] > R.FVS and v['hit_texels'] > R.FTS]
        assert full, 'no bin overflows all three tables'
    if name.startswith('islands'):
        cov = ref['cov']
        assert pl['pairs'] > 0 and bool((~(cov[D.er] & cov[D.eo])).all()) and pl['empty_partner'] > 0
        s = R._structure(inp)
        lk0 = ref['st'].lk0
        for k in range(4):      # the taps of (0, 0) hold the empty pixels' share alone
            assert bool((s['count'][lk0.flat[k][lk0.valid[k]]] == 0).all())
    if name == 'borders':
        pr, bl = D.pairs, D.active.any(1)
        at = lambda x0, d: int(((pr.d[bl] == d) & ((pr.x0[bl] if d == 0 else pr.y0[bl]) == x0)).sum())
        assert inp['res'] == (33, 65) and at(31, 0) > 0 and at(63, 0) > 0 and at(31, 1) > 0 and pl['image_border'] > 0
        assert most('hit_texels') > R.FTS
    if name.startswith('tiny'):
        assert inp['res'][0] * inp['res'][1] <= 2


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_cases_reach_their_paths_and_float32_meets_the_bars(name, oracle_ops):
    inp, ref, r32 = _three(name, oracle_ops)
    k32 = R.float32_in_kernel_order(inp)
    pl = R.plan(inp)
    m = R.decision_margin(inp, ref)
    fit = [v['fits'] for v in pl['halves'].values()]
    print(f"OBJ {name} pixels {ref['st'].px.n} deferred {pl['deferred']} hit {pl['hit']} pairs {pl['pairs']} across bins {pl['cross']} "
          f"(columns 31|32 {pl['cross_x31']}, rows 31|32 {pl['cross_y31']}) empty partners {pl['empty_partner']} image border {pl['image_border']} "
          f"halves {len(fit)} (fit {sum(fit)}, centred {sum(v['centred'] for v in pl['halves'].values())}, owrap {sum(v['owrap'] for v in pl['halves'].values())}, "
          f"taps inside {sum(v['inside'] for v in pl['halves'].values())} outside {sum(v['outside'] for v in pl['halves'].values())}) "
          f"most vertices in a bin {max(v['vertices'] for v in pl['bins'].values())} / {R.VT_SLOTS}, among hit pixels "
          f"{max(v['hit_vertices'] for v in pl['bins'].values())} / {R.FVS}, texels {max(v['hit_texels'] for v in pl['bins'].values())} / {R.FTS}, "
          f"slot bins {sum(v['sil'] for v in pl['bins'].values())}, one-term texels {k32['texel'].numel()}, worst margin {m:.0f} u")
    assert m >= R.GATE_MARGIN, (name, m)
    assert bool((r32['dd'] != 0).all()) and bool((ref['dd'] != 0).all()) and bool((r32['dn'] != 0).all())
    check_plan(name, inp, pl, k32)
    got = {'value': r32['value'][0], 'g_tex': r32['g_tex'][0], 'g_pos': r32['g_pos'][0]}
    assert bars_missed(inp, ref, r32, got, k32) == []
    for k in R.OUTPUTS:
        for row, e32 in R.measure_rows(r32[k][0], ref, k):
            print(f"OBJ {name} {row} e32 {e32:.3f} bound {8 * e32 + 4:.2f}")
    n = R.n_value(inp['tex'].shape[2], pl['max_deferred'])
    print(f"OBJ {name} value e32 {R.value_error(r32['value'][0], ref):.3f} bound {n + 2}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. wrong restatements miss a bar
# ---------------------------------------------------------------------------------------------------------------------

MUTANTS = {
    'no_esum_share': 'islands/wrap',
    'esum_with_wrap_taps_under_clamp': 'islands/clamp',
    'difference_term_sign_flipped': 'soup/C1/wrap/seam',
    'difference_term_dropped': 'soup/C1/wrap/seam',
    'partner_gradient_dropped': 'soup/C1/wrap/seam',
    'd_alpha_counted_by_both_pixels': 'soup/C1/wrap/seam',
    'zero_padding_gets_gradient': 'soup/C4/zero',
    'w_column_with_fxp_fyp_swapped': 'islands/wrap',
    'gq_without_2': 'tiny/1x1',
    'tu_summed_in_another_order': 'magnified/C1/wrap',
    'background_share_for_covered_pixels_too': 'tiny/1x1',
    'hit_pixel_added_without_removing_the_plain_term': 'soup/C3/clamp',
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_restatement_misses_a_bar(mutant, oracle_ops, monkeypatch):
    name = MUTANTS[mutant]
    inp, ref, r32 = _three(name, oracle_ops)
    k32 = R.float32_in_kernel_order(inp)
    monkeypatch.setattr(R, 'MUTANT', mutant)
    wrong = R.evaluate(inp, torch.float32)
    monkeypatch.setattr(R, 'MUTANT', None)
    got = {'value': wrong['value'][0], 'g_tex': wrong['g_tex'][0], 'g_pos': wrong['g_pos'][0]}
    missed = bars_missed(inp, ref, r32, got, k32)
    print(f"OBJ mutant {mutant} on {name}: {missed[:3]}")
    assert missed, (mutant, name)
    if mutant == 'tu_summed_in_another_order':      # only bit-identity sees the order of a float sum
        assert all(m[1] == 'a one-term texel is not gq * w bit for bit' for m in missed), missed

"""GPU: the WEIGHTED one-pass objective (csrc/objective.hip: k_shade_list_w / k_shade_queue_w, k_fix_list_w / k_fix_queue_w<CS, 0 / 1>, rho_psi,
mask_weight, face_weight, loss_grad_w, the wsum slots of fpcdr_objective_weighted_fwd; DESIGN.md 3, "Weighted objective rule") entry by entry
against float64 (tests/objective_ref.py, inp['weights']), through fpc_diffrend_amd.ops.pixel_objective(robust=, mask=, face_weights=,
weight_outside=, saturation=, wsum_out=, unit_upstream=True, id_plane_out=, aa_flags_out=) and backward(), every call twice, the mask stored one
byte off 16-byte alignment.  The twin of tests/test_gpu_objective_ref.py, whose _call and _hold it uses:
  preconditions  the id planes and the flag planes equal the statement's (torch.equal): the weights change neither;
  zeros          every entry objective_ref.predicted_zeros names is exactly 0 -- a texel or vertex reached through pixels of weight 0 only --
                 and the entries with a scale are the predicted ones;
  entry by entry g_tex, g_pos and the w column of g_pos: e <= 8 * e32 + 4 in units of u = 2^-24, e32 the float32 evaluation of the statement;
  the value      |value - r| / S <= (objective_ref.n_value(kind) + 2) u, a derived operation count per kind;
  wsum           the sum of all weights by the long-sum bar, e <= 8 * e32 + 4;
  bit for bit    a texel with exactly one term, of a weighted pixel outside every blend, equals gq * w_k with gq = (-2 cs gs) (w psi) in the
                 kernel's float32 order: for L2, and for Charbonnier and Geman-McClure as well -- the build's divide and square root are
                 correctly rounded (DESIGN: "IEEE divide and square root"); so is torch's divide on the CPU, and the statement takes its
                 square root from float64 (robust_ref.sqrt_rounded: torch's float32 root is not).
Cases: objective_ref.WEIGHTED_CASE_IDS x objective_ref.WEIGHT_SETS -- the five kinds and scales under mask + face weights + sat = 100 +
w_outside = 0.25, and each other option set of tests/test_gpu_weighted_objective.py under one kind other than L2; `soup/C4/zero` at its full
four channels, and `magnified/C1/wrap` for its thousands of one-term texels (the other cases have none to four).  Twins on
`soup/C1/wrap/seam`, `soup/C4/zero` and `magnified/C1/wrap`: launch hints frozen at (1, 1, 1) (the _queue_w sweeps), record_slots equal to the
call's own demand, _cached_tri_uv patched to None, only pos / only tex requiring a gradient: the same bars, ids and flags, the same bits in
the one-term texels.  With neutral weights the call meets the PLAIN statement's bars.  Every test prints "WOBJREF case output calls e_gpu e32
bound" (pytest -s).  tests/test_objective_weighted_ref.py shows on the CPU that the statement equals float64 autograd through the oracle and
robust_ref.loss_plain, that the weights reach what they exist for and that wrong restatements miss these bars.

Measured on an MI355X (units of u; per case the largest e_gpu and e32 and the least bound over its ten option sets and two calls; the whole
file, 95 tests with the building of the cases and their references on the CPU, ran in 7.6 s, the slowest test in 1.1 s).  Every id plane and
flag plane was equal, every predicted zero exact, and every one-term texel bit-identical to gq * w_k, Charbonnier's and Geman-McClure's
included -- 2703 (the full option set) .. 5827 (the mask alone) a call on `magnified/C1/wrap`, 82 041 over all calls of the file -- once the
statement's float32 square root was the correctly rounded one (robust_ref.sqrt_rounded): with torch's own root on the CPU the first run had
one Charbonnier texel of `soup/C4/zero` 2 units in the last place off, and the device was the one that was right.  Every twin gave its case's
figures to the three digits shown.  No bug was found in the kernels.

  case                g_tex e_gpu / e32   g_pos e_gpu / e32   g_pos.w e_gpu / e32   least bounds (8 e32 + 4)   value e_gpu / e32   least bound   wsum e_gpu / e32   least bound
  soup/C1/wrap/seam   0.027 / 0.027       0.014 / 0.014       0.009 / 0.009         4.01  4.01  4.00           0.000 / 0.000       135           0.596 / 0.697      4.51
  soup/C3/clamp       0.136 / 0.136       0.167 / 0.167       0.075 / 0.075         4.11  4.07  4.03           0.000 / 0.000       247           0.561 / 1.048      4.10
  soup/C4/zero        0.082 / 0.082       0.287 / 0.287       0.227 / 0.227         4.04  4.37  4.34           0.001 / 0.003       303           0.758 / 1.523      5.33
  islands/wrap        0.029 / 0.029       0.006 / 0.006       0.004 / 0.004         4.00  4.00  4.00           0.003 / 0.001       87            0.298 / 2.309      5.80
  islands/clamp       0.065 / 0.065       0.002 / 0.002       0.001 / 0.001         4.00  4.00  4.00           0.001 / 0.001       103           0.511 / 1.200      5.27
  borders             0.112 / 0.112       0.017 / 0.017       0.013 / 0.013         4.05  4.00  4.00           0.000 / 0.000       205           0.386 / 3.271      5.08
  mesh/B3             0.022 / 0.062       0.007 / 0.009       0.006 / 0.006         4.00  4.00  4.00           0.005 / 0.005       115           0.650 / 1.677      5.58
  tiny/1x1            0.000 / 0.000       0.000 / 0.000       0.000 / 0.000         4.00  4.00  4.00           0.003 / 0.000       80            0.005 / 0.005      4.00
  magnified/C1/wrap   0.380 / 0.380       0.019 / 0.019       0.012 / 0.012         4.61  4.01  4.00           0.002 / 0.002       125           0.429 / 1.157      4.07
The gradients' scale is S_psi = S_d (|psi| <= |d|, robust_ref.py), so under a robust kind an entry is a small share of its scale and e_gpu small
with it: these bars see a wrong term, a wrong weight or a lost pixel, and the bit-for-bit bar the rest.  The value's bound is a worst-case
operation count against a scale summed over thousands of pixels (objective_ref.n_value)."""
import pytest
import torch

import objective_ref as R
from test_gpu_objective_ref import _call, _hold

pytestmark = pytest.mark.gpu

TWINS = [('soup/C1/wrap/seam', 'charbonnier20/all'), ('soup/C4/zero', 'geman2/all'), ('magnified/C1/wrap', 'charbonnier2/all')]
# one-term texels at the least (objective_ref.float32_in_kernel_order): the two soups have many terms on every texel, `magnified` exists for them
TWIN_TEXELS = {'soup/C1/wrap/seam': 0, 'soup/C4/zero': 1, 'magnified/C1/wrap': 2000}


def _one_term_texels(name, inp, got, tag, calls):
    """Prints how many one-term texels differ from gq * w_k and by how many units in the last place at most (asserted by _hold)."""
    k32 = R.float32_in_kernel_order(inp)
    C = inp['tex'].shape[2]
    x, r = got['g_tex'].reshape(-1, C)[k32['texel']].float(), k32['g_tex']
    ulp = (x.view(torch.int32).long() - r.view(torch.int32).long()).abs()
    print(f"WOBJREF {name}{tag} one-term texels {calls} {x.shape[0]} texels, {int((ulp != 0).any(1).sum()) if x.numel() else 0} differ, "
          f"{int(ulp.max()) if x.numel() else 0} units in the last place at most")


def _hold_w(name, inp, got, tag, calls=1):
    if 'g_tex' in got:
        _one_term_texels(name, inp, got, tag, calls)
    _hold(name, inp, got, tag, calls, word='WOBJREF')


@pytest.mark.parametrize("tag", R.WEIGHT_TAGS)
@pytest.mark.parametrize("name", R.WEIGHTED_CASE_IDS)
def test_weighted_objective_entry_by_entry(name, tag, oracle_ops):
    import fpc_diffrend_amd.ops as dr
    inp = R.with_weights(R.case_inputs(name, oracle_ops), tag)
    dr.clear_hints()
    for call in (1, 2):
        _hold_w(name, inp, _call(dr, inp), '|' + tag, call)
    dr.clear_hints()


@pytest.mark.parametrize("name", ['soup/C1/wrap/seam', 'soup/C4/zero'])
def test_neutral_weights_meet_the_plain_statement(name, oracle_ops):
    """L2, no mask, no face weights, w_outside = 1, sat = 0 through the weighted kernels: held to the plain statement's own bars (the
    statements are equal: tests/test_objective_weighted_ref.py), one-term texels bit for bit, and wsum is the number of entries."""
    import fpc_diffrend_amd.ops as dr
    base = R.case_inputs(name, oracle_ops)
    inp = R.with_weights(base, 'neutral')
    dr.clear_hints()
    got = _call(dr, inp)
    _hold_w(name, inp, got, '|neutral')
    assert float(got['wsum']) == float(base['ref_u8'].numel() * base['tex'].shape[2])
    plain = dict(got)
    del plain['wsum']
    _hold(name, base, plain, '|neutral against the plain statement', word='WOBJREF')
    dr.clear_hints()


@pytest.mark.parametrize("name,tag", TWINS)
def test_weighted_twins_meet_the_same_bars(name, tag, oracle_ops, monkeypatch):
    import fpc_diffrend_amd.ops as dr
    inp = R.with_weights(R.case_inputs(name, oracle_ops), tag)
    ref, k32 = R.reference(inp), R.float32_in_kernel_order(inp)
    B, (H, W), C = inp['pos'].shape[0], inp['res'], inp['tex'].shape[2]
    n = R.value_count(inp)
    assert k32['texel'].numel() >= TWIN_TEXELS[name], (name, k32['texel'].numel())
    dr.clear_hints()
    base = _call(dr, inp, launch_hints=False, record_slots=0)
    _hold_w(name, inp, base, f'|{tag}/no-hints,by-pixel')

    def same(g, what):
        assert torch.equal(g['ids'], base['ids']) and torch.equal(g['flags'], base['flags']), (name, what)
        assert abs(float(g['value']) - float(base['value'])) <= (n + 2) * R.U * float(ref['value'][1]), (name, what)
        if 'g_tex' in g:      # the one-term texels: the same bits in every twin
            assert torch.equal(g['g_tex'].reshape(-1, C)[k32['texel']], base['g_tex'].reshape(-1, C)[k32['texel']]), (name, what)

    # hints frozen at (1, 1, 1): k_shade_queue_w and k_fix_queue_w<CS, 0 / 1> take every entry of their lists but the first
    dr.clear_hints()
    _call(dr, inp)
    h = dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]
    h.poll()
    h.caps, h.frozen = (1, 1, 1), True
    g = _call(dr, inp)
    _hold_w(name, inp, g, f'|{tag}/sweeps')
    same(g, 'sweeps')
    torch.cuda.synchronize()
    assert int(h.host[0]) > 1 and int(h.host[3]) > 1, (name, 'the sweeps had no work')
    dr.clear_hints()
    # compact records in exactly as many slots as the call asks for
    _call(dr, inp, record_slots=4096)
    h = dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]
    need = int(h.host[1])
    assert sum(v['sil'] for v in R.plan(inp)['bins'].values()) <= need <= B * ((H + 31) // 32) * ((W + 31) // 32)
    dr.clear_hints()
    g = _call(dr, inp, record_slots=need)
    _hold_w(name, inp, g, f'|{tag}/slots={need}')
    same(g, 'slots')
    dr.clear_hints()
    # the generic instantiation k_shade_list_w<CS, -1>: uv through the index buffer
    monkeypatch.setattr(dr, "_cached_tri_uv", lambda uv_, idx_: None)
    g = _call(dr, inp)
    _hold_w(name, inp, g, f'|{tag}/uv_indirect')
    same(g, 'uv_indirect')
    monkeypatch.undo()
    for want in (('pos',), ('tex',)):
        g = _call(dr, inp, want=want)
        _hold_w(name, inp, g, f'|{tag}/only-' + want[0])
        same(g, want[0])
    dr.clear_hints()

"""GPU: the MIP branch of the one-pass pixel objective (csrc/objective.hip: k_shade_mip_list/_queue, k_fix<0>, k_fix_mip_list/_queue,
k_objective_finish; csrc/texsample.h: mip_lookup_fwd/_bwd, mip_sample_bwd; ops._build_mips / _fold_mip_grads) entry by entry against float64
(tests/objective_ref.py with mip_levels), through fpc_diffrend_amd.ops.pixel_objective(enable_mip=True, max_mip_level=, id_plane_out=,
aa_flags_out=, unit_upstream=True) and backward(), every case twice.  The bars are those of tests/test_gpu_objective_ref.py, whose
_call and _hold this file imports:
  preconditions  the id planes equal (oracle id) | silhouette bits << 24 and the flag planes the statement's pair set (torch.equal);
  zeros          every entry objective_ref.predicted_zeros names -- the texels no level's tap reaches after folding among them -- is
                 exactly 0, and the entries with a scale are the predicted ones;
  entry by entry e = max_i |x_i - r_i| / S_i in units of u = 2^-24 for g_tex, g_pos and the w column of g_pos on a row of its own:
                 e <= 8 * e32 + 4, e32 the same measure of the float32 evaluation of the statement by torch on the CPU;
  the value      |value - r| / S <= (objective_ref.n_value(mip) + 2) u, a derived operation count.
`mip/magnified/C1/wrap` is the inputs of `magnified/C1/wrap` with enable_mip=True and max_mip_level=0, held to the NON-mip reference by
the non-mip bars, one-term texels bit for bit included ((gq * (1 - fl)) * w_k with fl = 0).  (With the whole chain these inputs do not
clamp at level 0 -- 3 texels a pixel are level log2 3 = 1.58 --, and their footprint is isotropic, where the level's scale has no bound.
Without a chain every level clamps at 0 from above, and the mip kernels must give the established numbers.)
Twins on `mip/mid/C1/wrap/seam` and `mip/span`: launch hints frozen at (1, 1, 1) (k_shade_mip_queue and k_fix_mip_queue do the work),
record_slots equal to the call's own demand, _cached_tri_uv patched to None (uv_indirect), only pos requiring a gradient (the prepass is
skipped, lv.grad all null), only tex: the same bars, the same ids and flags.  Each test prints "OBJMIP case row calls e_gpu e32 bound"
(pytest -s).  tests/test_objective_mip_ref.py shows on the CPU that the statement equals float64 autograd through the oracle, that every
case reaches its path and that wrong restatements miss these bars.

Measured on an MI355X (units of u; the larger of a case's two calls; the whole file, 15 tests with the building of the cases and their
references on the CPU, ran in 6.6 s).  Every id plane and flag plane was equal and every predicted zero exact; the 6315 one-term texels of
`magnified/C1/wrap` were bit-identical to gq * w_k in both mip calls.  Every twin (no hints and records by pixel, sweeps, slots = 12,
uv_indirect, only pos, only tex) gave its case's figures to the three digits shown.  No bug was found.

  case                    g_tex e_gpu / e32   g_pos e_gpu / e32   g_pos.w e_gpu / e32   bounds (8 e32 + 4)    value e_gpu / e32   bound
  mip/mid/C1/wrap/seam    0.003 / 0.003       0.011 / 0.011       0.008 / 0.008         4.02  4.09  4.06      0.000 / 0.000         97
  mip/mid/C3/clamp        0.024 / 0.018       0.016 / 0.016       0.009 / 0.009         4.14  4.13  4.07      0.000 / 0.000        229
  mip/mid/C4/zero         0.033 / 0.033       0.449 / 0.449       0.123 / 0.123         4.27  7.60  4.98      0.001 / 0.001        265
  mip/span                0.010 / 0.010       0.019 / 0.018       0.010 / 0.009         4.08  4.15  4.07      0.000 / 0.000        115
  mip/top                 0.009 / 0.010       0.034 / 0.034       0.024 / 0.024         4.08  4.27  4.19      0.000 / 0.001        103
  mip/no-levels           0.009 / 0.009       0.011 / 0.011       0.005 / 0.005         4.07  4.09  4.04      0.000 / 0.000        247
  mip/overflow/C3         0.075 / 0.075       0.003 / 0.003       0.001 / 0.001         4.60  4.03  4.01      0.000 / 0.000        229
  mip/perspective         0.007 / 0.007       0.002 / 0.002       0.001 / 0.001         4.05  4.02  4.01      0.005 / 0.005         61
  mip/islands/zero        0.024 / 0.024       0.108 / 0.108       0.106 / 0.092         4.19  4.87  4.73      0.004 / 0.005         81
  mip/tiny/1x1            0.209 / 0.209       0.077 / 0.077       0.000 / 0.000         5.67  4.62  4.00      0.004 / 0.004         55
  mip/tiny/1x2            0.015 / 0.015       0.004 / 0.004       0.003 / 0.003         4.12  4.03  4.02      0.016 / 0.016         51
  mip/tiny/2x1            0.133 / 0.129       0.037 / 0.038       0.037 / 0.039         5.03  4.31  4.31      0.007 / 0.007         51
  magnified/C1/wrap/mip   0.175 / 0.175       0.005 / 0.005       0.003 / 0.003         5.40  4.04  4.02      0.000 / 0.000         90
The value's bound is a worst-case operation count against a scale summed over thousands of pixels (objective_ref.n_value): it sees a wrong
term or factor, not a lost bit."""
import pytest
import torch

import objective_ref as R
from test_gpu_objective_ref import _call, _hold

pytestmark = pytest.mark.gpu


def _mip_call(dr, inp, **kw):
    return _call(dr, inp, enable_mip=True, max_mip_level=inp['max_mip_level'], **kw)


@pytest.mark.parametrize("name", R.MIP_CASE_IDS)
def test_mip_objective_entry_by_entry(name, oracle_ops):
    import fpc_diffrend_amd.ops as dr
    inp = R.case_inputs(name, oracle_ops)
    dr.clear_hints()
    for call in (1, 2):
        _hold(name, inp, _mip_call(dr, inp), '', call, word='OBJMIP')
    dr.clear_hints()


def test_magnified_with_no_chain_meets_the_non_mip_reference(oracle_ops):
    import fpc_diffrend_amd.ops as dr
    name = 'magnified/C1/wrap'
    inp = R.case_inputs(name, oracle_ops)
    assert R.float32_in_kernel_order(inp)['texel'].numel() >= 1000
    dr.clear_hints()
    for call in (1, 2):
        _hold(name, inp, _call(dr, inp, enable_mip=True, max_mip_level=0), '/mip', call, word='OBJMIP')
    dr.clear_hints()


@pytest.mark.parametrize("name", ['mip/mid/C1/wrap/seam', 'mip/span'])
def test_mip_twins_meet_the_same_bars(name, oracle_ops, monkeypatch):
    import fpc_diffrend_amd.ops as dr
    inp = R.case_inputs(name, oracle_ops)
    ref = R.reference(inp)
    B, (H, W) = inp['pos'].shape[0], inp['res']
    n = R.n_value(inp['tex'].shape[2], R.plan(inp)['max_deferred'], True)
    dr.clear_hints()
    base = _mip_call(dr, inp, launch_hints=False, record_slots=0)
    _hold(name, inp, base, '/no-hints,by-pixel', word='OBJMIP')

    def same(g, tag):
        assert torch.equal(g['ids'], base['ids']) and torch.equal(g['flags'], base['flags']), (name, tag)
        assert abs(float(g['value']) - float(base['value'])) <= (n + 2) * R.U * float(ref['value'][1]), (name, tag)

    # hints frozen at (1, 1, 1): every list kernel's strided sweep
    dr.clear_hints()
    _mip_call(dr, inp)
    h = dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]
    h.poll()
    h.caps, h.frozen = (1, 1, 1), True
    g = _mip_call(dr, inp)
    _hold(name, inp, g, '/sweeps', word='OBJMIP')
    same(g, 'sweeps')
    dr.clear_hints()
    # compact records in exactly as many slots as the call asks for
    _mip_call(dr, inp, record_slots=4096)
    h = dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]
    need = int(h.host[1])
    assert sum(v['sil'] for v in R.plan(inp)['bins'].values()) <= need <= B * ((H + 31) // 32) * ((W + 31) // 32)
    dr.clear_hints()
    g = _mip_call(dr, inp, record_slots=need)
    _hold(name, inp, g, f'/slots={need}', word='OBJMIP')
    same(g, 'slots')
    dr.clear_hints()
    # uv through the index buffer
    monkeypatch.setattr(dr, "_cached_tri_uv", lambda uv_, idx_: None)
    g = _mip_call(dr, inp)
    _hold(name, inp, g, '/uv_indirect', word='OBJMIP')
    same(g, 'uv_indirect')
    monkeypatch.undo()
    for want in (('pos',), ('tex',)):
        g = _mip_call(dr, inp, want=want)
        _hold(name, inp, g, '/only-' + want[0], word='OBJMIP')
        same(g, want[0])
    dr.clear_hints()

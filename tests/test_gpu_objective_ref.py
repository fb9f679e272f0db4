"""GPU: the one-pass pixel objective (csrc/objective.hip: k_shade_list, k_fix<0>, k_fix<1>, k_objective_finish) entry by entry against
float64 (tests/objective_ref.py), through fpc_diffrend_amd.ops.pixel_objective(id_plane_out=, aa_flags_out=, unit_upstream=True) and
backward(), every case twice.
  preconditions  the id planes equal (oracle id) | silhouette bits << 24 and the flag planes the statement's pair set (torch.equal);
  zeros          every entry objective_ref.predicted_zeros names is exactly 0, and the entries with a scale are the predicted ones;
  entry by entry e = max_i |x_i - r_i| / S_i in units of u = 2^-24 for g_tex, g_pos and the w column of g_pos on a row of its own:
                 e <= 8 * e32 + 4, e32 the same measure of the float32 evaluation of the statement by torch on the CPU;
  the value      |value - r| / S <= (objective_ref.n_value + 2) u, a derived operation count;
  bit for bit    a texel with exactly one term, of a pixel outside every blend, equals float32_in_kernel_order's gq * w_k.
Twins on `soup/C1/wrap/seam` and `magnified/C1/wrap`: launch hints frozen at (1, 1, 1) (every list kernel's strided sweep), record_slots equal to the call's own demand
against records by pixel, _cached_tri_uv patched to None (uv_indirect), only pos / only tex requiring a gradient: the same bars, the
same ids and flags, the same bits in the one-term texels; `borders` by pixel and with compact records.  Each test prints "OBJ case output calls e_gpu e32 bound" (pytest -s).  tests/test_objective_ref.py shows on the
CPU that the statement equals float64 autograd through the oracle, that every case reaches its path and that wrong restatements
miss these bars.

Measured on an MI355X (units of u; the larger of a case's two calls; the whole file, 16 tests with the building of the cases and their
references on the CPU, ran in 5.0 s).  Every id plane and flag plane was equal and every predicted zero exact; the 6315 one-term texels
of `magnified/C1/wrap` (and the four of each `tiny` image) were bit-identical to gq * w_k in both calls and in every twin.  Every twin
(no hints and records by pixel, sweeps, slots = 12 / 5, uv_indirect, only pos, only tex; `borders` by pixel and with 12 slots) gave its
case's figures to the three digits shown.  No bug was found.

  case                g_tex e_gpu / e32   g_pos e_gpu / e32   g_pos.w e_gpu / e32   bounds (8 e32 + 4)    value e_gpu / e32   bound
  magnified/C1/wrap   0.175 / 0.175       0.005 / 0.005       0.003 / 0.003         5.40  4.04  4.02      0.000 / 0.000        90
  soup/C1/wrap/seam   0.032 / 0.032       0.010 / 0.010       0.007 / 0.007         4.26  4.08  4.06      0.000 / 0.000       100
  soup/C3/clamp       0.113 / 0.113       0.281 / 0.281       0.159 / 0.159         4.90  6.25  5.27      0.000 / 0.000       212
  soup/C4/zero        0.038 / 0.038       0.324 / 0.324       0.201 / 0.201         4.30  6.59  5.61      0.004 / 0.004       268
  mesh/B3             0.012 / 0.167       0.004 / 0.018       0.004 / 0.004         5.34  4.14  4.03      0.004 / 0.007        80
  confetti            0.004 / 0.004       0.037 / 0.037       0.021 / 0.021         4.03  4.30  4.17      0.000 / 0.000       140
  islands/wrap        0.010 / 0.010       0.003 / 0.003       0.003 / 0.003         4.08  4.02  4.02      0.002 / 0.002        52
  islands/clamp       0.027 / 0.029       0.002 / 0.002       0.001 / 0.001         4.23  4.02  4.01      0.002 / 0.002        68
  islands/zero        0.029 / 0.029       0.003 / 0.003       0.001 / 0.001         4.23  4.03  4.01      0.000 / 0.000        76
  borders             0.046 / 0.046       0.006 / 0.006       0.003 / 0.004         4.37  4.05  4.03      0.000 / 0.000       170
  tiny/1x1            0.042 / 0.042       0.006 / 0.006       0.000 / 0.000         4.33  4.05  4.00      0.010 / 0.010        50
  tiny/1x2            0.038 / 0.038       0.013 / 0.013       0.007 / 0.007         4.30  4.11  4.06      0.013 / 0.013        46
  tiny/2x1            0.092 / 0.092       0.009 / 0.009       0.009 / 0.009         4.73  4.07  4.07      0.007 / 0.007        46
The value's bound is a worst-case operation count against a scale summed over thousands of pixels (objective_ref.n_value): it sees a wrong
term or factor, not a lost bit."""
import numpy as np
import pytest
import torch

import objective_ref as R

pytestmark = pytest.mark.gpu


def _call(dr, inp, want=('pos', 'tex'), **kw):
    from fpc_diffrend_amd import _lib
    lib = _lib.load()
    dev = 'cuda'
    B, (H, W) = inp['pos'].shape[0], inp['res']
    ctx = dr.RasterizeGLContext(device=dev)
    pos, tex = inp['pos'].to(dev).requires_grad_('pos' in want), inp['tex'].to(dev).requires_grad_('tex' in want)
    idp = torch.zeros(lib.fpcdr_idplane_bytes(B, H, W), dtype=torch.uint8, device=dev)
    flags = torch.zeros(lib.fpcdr_antialias_flags_bytes(B, H, W) // 8, dtype=torch.int64, device=dev)
    wt, wsum = inp.get('weights'), None
    if wt is not None:      # objective_ref.with_weights: the weighted call, its mask stored one byte off 16-byte alignment
        from test_gpu_robust import _at
        wsum = torch.zeros(1, dtype=torch.float64, device=dev)
        mask = None if wt['mask'] is None else _at(wt['mask'], 1)
        assert mask is None or mask.data_ptr() % 16 == 1
        kw = dict(kw, robust=(wt['kind'], wt['c']), mask=mask, face_weights=None if wt['face_weights'] is None else wt['face_weights'].to(dev),
                  weight_outside=wt['weight_outside'], saturation=wt['saturation'], wsum_out=wsum)
    val = dr.pixel_objective(ctx, pos, inp['tri'].to(dev), inp['uv'].to(dev), inp['uv_tri'].to(dev), tex, inp['ref_u8'].to(dev), (H, W),
                             boundary_mode=inp['boundary'], unit_upstream=True, id_plane_out=idp, aa_flags_out=flags, **kw)
    val.backward()
    torch.cuda.synchronize()
    OY, OX = (H + 31) // 32, (W + 31) // 32
    planes = idp.cpu().view(torch.int32).reshape(B, OY, OX, 32, 32).permute(0, 1, 3, 2, 4).reshape(B, OY * 32, OX * 32)[:, :H, :W].long() & 0xffffffff
    got = {'value': val.detach().cpu(), 'ids': planes, 'flags': flags.cpu()}
    if wsum is not None:
        got['wsum'] = wsum.cpu()[0]
    if 'pos' in want:
        got['g_pos'] = pos.grad.cpu()
    if 'tex' in want:
        got['g_tex'] = tex.grad.cpu()
    return got


def _hold(name, inp, got, tag, calls=1, word='OBJ'):
    ref, r32, k32 = R.reference(inp), R.reference(inp, torch.float32), R.float32_in_kernel_order(inp)
    D = ref['D']
    assert torch.equal(got['ids'], R.id_planes(inp)), (name, tag, 'id planes')
    assert torch.equal(got['flags'].reshape(-1), torch.from_numpy(D.flags.view(np.int64).reshape(-1))), (name, tag, 'flag planes')
    full = dict(got)
    for k in R.OUTPUTS:      # (an output that was not asked for: held as the statement's own)
        full.setdefault(k, ref[k][0].float())
    for k in R.OUTPUTS:
        if k in got:
            for (row, e), (_, e32) in zip(R.measure_rows(got[k], ref, k), R.measure_rows(r32[k][0], ref, k)):
                print(f"{word} {name}{tag} {row} {calls} {e:.3f} {e32:.3f} {8 * e32 + 4:.2f}")
    n = R.value_count(inp)
    print(f"{word} {name}{tag} value {calls} {R.value_error(got['value'], ref):.3f} {R.value_error(r32['value'][0], ref):.3f} {n + 2}")
    if 'wsum' in ref:      # the weighted call: the sum of all weights
        (_, e), (_, e32) = R.measure_rows(got['wsum'], ref, 'wsum')[0], R.measure_rows(r32['wsum'][0], ref, 'wsum')[0]
        print(f"{word} {name}{tag} wsum {calls} {e:.3f} {e32:.3f} {8 * e32 + 4:.2f}")
    assert R.failures(inp, ref, r32, full, k32 if 'g_tex' in got else None) == [], (name, tag)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_objective_entry_by_entry(name, oracle_ops):
    import fpc_diffrend_amd.ops as dr
    inp = R.case_inputs(name, oracle_ops)
    dr.clear_hints()
    for call in (1, 2):
        _hold(name, inp, _call(dr, inp), '', call)
    dr.clear_hints()


@pytest.mark.parametrize("name", ['soup/C1/wrap/seam', 'magnified/C1/wrap'])
def test_twins_meet_the_same_bars(name, oracle_ops, monkeypatch):
    import fpc_diffrend_amd.ops as dr
    inp = R.case_inputs(name, oracle_ops)
    ref, k32 = R.reference(inp), R.float32_in_kernel_order(inp)
    B, (H, W) = inp['pos'].shape[0], inp['res']
    n = R.n_value(inp['tex'].shape[2], R.plan(inp)['max_deferred'])
    dr.clear_hints()
    base = _call(dr, inp, launch_hints=False, record_slots=0)
    _hold(name, inp, base, '/no-hints,by-pixel')

    def same(g, tag):
        assert torch.equal(g['ids'], base['ids']) and torch.equal(g['flags'], base['flags']), (name, tag)
        assert abs(float(g['value']) - float(base['value'])) <= (n + 2) * R.U * float(ref['value'][1]), (name, tag)
        if 'g_tex' in g:      # the one-term texels: the same bits in every twin
            assert torch.equal(g['g_tex'].reshape(-1, 1)[k32['texel']], base['g_tex'].reshape(-1, 1)[k32['texel']]), (name, tag)

    # hints frozen at (1, 1, 1): every list kernel's strided sweep
    dr.clear_hints()
    _call(dr, inp)
    h = dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]
    h.poll()
    h.caps, h.frozen = (1, 1, 1), True
    g = _call(dr, inp)
    _hold(name, inp, g, '/sweeps')
    same(g, 'sweeps')
    dr.clear_hints()
    # compact records in exactly as many slots as the call asks for
    _call(dr, inp, record_slots=4096)
    h = dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')]
    need = int(h.host[1])
    assert sum(v['sil'] for v in R.plan(inp)['bins'].values()) <= need <= B * ((H + 31) // 32) * ((W + 31) // 32)
    dr.clear_hints()
    g = _call(dr, inp, record_slots=need)
    _hold(name, inp, g, f'/slots={need}')
    same(g, 'slots')
    dr.clear_hints()
    # the generic instantiation k_shade_list<1, -1>: uv through the index buffer
    monkeypatch.setattr(dr, "_cached_tri_uv", lambda uv_, idx_: None)
    g = _call(dr, inp)
    _hold(name, inp, g, '/uv_indirect')
    same(g, 'uv_indirect')
    monkeypatch.undo()
    for want in (('pos',), ('tex',)):
        g = _call(dr, inp, want=want)
        _hold(name, inp, g, '/only-' + want[0])
        same(g, want[0])
    dr.clear_hints()


def test_borders_with_compact_records(oracle_ops):
    """`borders`: records by pixel against record_slots equal to the call's own demand -- rix goes through the neighbours' slots across
    columns 31 | 32 and 63 | 64 and rows 31 | 32."""
    import fpc_diffrend_amd.ops as dr
    name = 'borders'
    inp = R.case_inputs(name, oracle_ops)
    dr.clear_hints()
    base = _call(dr, inp, record_slots=0)
    _hold(name, inp, base, '/by-pixel')
    dr.clear_hints()
    _call(dr, inp, record_slots=4096)
    need = int(dr._list_hints[next(k for k in dr._list_hints if k[0] == 'onepass')].host[1])
    dr.clear_hints()
    g = _call(dr, inp, record_slots=need)
    _hold(name, inp, g, f'/slots={need}')
    assert torch.equal(g['ids'], base['ids']) and torch.equal(g['flags'], base['flags'])
    dr.clear_hints()

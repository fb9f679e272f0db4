"""GPU: the float outputs of the rasterize operator (csrc/rasterize.hip: k_bins over shade_pixel, k_grad over shade_pixel_bwd) entry by
entry against float64 (tests/rasterize_ref.py), through fpc_diffrend_amd.ops.rasterize and torch.autograd.

The triangle ids must equal the oracle's (rasterize_ids, rasterize_ids_ranges in range mode); everything else is evaluated on those ids.
Every output x is compared with float64 arithmetic on the float32 inputs the kernel read: e = max_i |x_i - r_i| / S_i in units of
u = 2^-24, S_i the first-order rounding scale of entry i carried from the inputs down (rasterize_ref.py); entries with S_i = 0 have no
term, must be exactly 0, and their number must be the one the construction predicts (uncovered pixels, a barycentric its clamp puts at 0,
vertices nothing with a gradient shows, the z column of g_pos).
  forward (u, v, z/w of rast; rast_db): torch.equal to rasterize_ref.float32_in_kernel_order -- the library is built with
              -ffp-contract=off, and DESIGN.md ("Accuracy bars") states that float outputs are bit-identical to unfused float32
              arithmetic --, AND e <= 8 * e32 + 4, e32 the error of the same formula in float32 by torch on the CPU; a pixel whose centre
              the statement puts beyond a vertex has (u, v) = (1, 0), (0, 1) or (0, 0) exactly;
  backward (g_pos: over every pixel that shows a vertex, summed by a DPP scan, an LDS table in double and float atomics):
              e <= 8 * e32 + 4, e32 from the float32 formula summed with index_add_; in the one-per-triangle cases every entry has one
              term and g_pos must be bit-identical to the float32 statement of shade_pixel_bwd.
Every call is made twice: the forward must be bit-identical between the two, g_pos too where every entry has one term, elsewhere both
must meet the bar (the atomics' order).  The tensor rasterize returns carries a region hint whose plane 0 is at least the coverage's and has
empty bins in `lattice`; the same call under ops.no_region_hints() gives bit-identical rast / rast_db and a g_pos within the same bars
(bit-identical where it has one term).  Each case runs with grad_db=True, with grad_db=False (go_db is handed in and ignored) and, for
`soup`, through a context with output_db=False (rast_db of shape [B,H,W,0], k_bins<false>).  tests/test_rasterize_ref.py shows on the
CPU, for each case, the condition that makes it reach its kernel path, that float32 reaches these bars and that ten wrong restatements
miss them.  Every line below is printed by a test as "RAST case output e_gpu e32 bound" (pytest -s).

Measured on an MI355X (units of u; the largest over the calls of a row, a call being one forward and backward of a case in one of its
forms, hinted or under no_region_hints(), and for g_pos each of the two calls; the last column is the call of the row that came closest
to its own bound).  u, v, z/w and rast_db of every call were bit-identical to float32_in_kernel_order, and so was g_pos in the
one-per-triangle cases, clamp and renormalise branches included: no kernel, flag or host bug was found.  Where e_gpu equals e32 the worst
entry is a vertex one or two pixels show, where the kernel and float32 torch make the same roundings; where thousands of pixels meet in a
vertex (big, grid) the table's sums in double leave the kernel closer to float64 than float32 torch is.  The whole file, 19 case forms,
runs in 4.1 s there (the first case carries 1.2 s of start-up):

  case                      output   calls max e_gpu  max e32   closest to its bound (e_gpu / bound, call)
  lattice                   rast         4     5.838    5.838   5.84 / 50.7  grad_db
  lattice                   rast_db      4     1.801    1.801   1.80 / 18.4  grad_db
  lattice                   g_pos        8     1.128    1.128   1.13 / 13.0  no grad_db
  soup                      rast         6     5.276    5.276   5.28 / 46.2  grad_db
  soup                      rast_db      4     1.376    1.376   1.38 / 15.0  grad_db
  soup                      g_pos       12     1.814    1.814   1.81 / 18.5  no grad_db
  confetti                  rast         4     9.606    9.606   9.61 / 80.9  grad_db
  confetti                  rast_db      4     2.181    2.181   2.18 / 21.4  grad_db
  confetti                  g_pos        8     3.056    3.056   3.06 / 28.4  no grad_db
  grid                      rast         4    12.633   12.633   12.63 / 105.1  grad_db
  grid                      rast_db      4     0.842    0.842   0.84 / 10.7  grad_db
  grid                      g_pos        8     0.020    0.020   0.02 / 4.2  no grad_db
  big                       rast         4     0.792    0.792   0.79 / 10.3  grad_db
  big                       rast_db      4     0.657    0.657   0.66 / 9.3  grad_db
  big                       g_pos        8     0.004    0.057   0.00 / 4.2  grad_db
  lattice/one-per-triangle  rast         4     5.838    5.838   5.84 / 50.7  grad_db
  lattice/one-per-triangle  rast_db      4     1.801    1.801   1.80 / 18.4  grad_db
  lattice/one-per-triangle  g_pos        8     5.078    5.078   5.08 / 44.6  no grad_db
  soup/one-per-triangle     rast         4     5.276    5.276   5.28 / 46.2  grad_db
  soup/one-per-triangle     rast_db      4     1.376    1.376   1.38 / 15.0  grad_db
  soup/one-per-triangle     g_pos        8     1.790    1.790   1.79 / 18.3  no grad_db
  soup/sparse-gradient      rast         4     5.276    5.276   5.28 / 46.2  grad_db
  soup/sparse-gradient      rast_db      4     1.376    1.376   1.38 / 15.0  grad_db
  soup/sparse-gradient      g_pos        8     1.138    1.138   1.14 / 13.1  no grad_db
  range                     rast         4     5.611    5.611   5.61 / 48.9  grad_db
  range                     rast_db      4     2.602    2.602   2.60 / 24.8  grad_db
  range                     g_pos        8     0.468    0.468   0.47 / 7.7  no grad_db
"""
import pytest
import torch

import interpolate_ref as I
import rasterize_ref as R

pytestmark = pytest.mark.gpu

FORWARD = ('rast', 'rast_db')


def _report(case, name, e, e32, bound):
    print(f"RAST {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={bound:.1f}")


def _call(ops, inp, form):
    """ops.rasterize and its backward, twice -> name -> tensor (CPU) of the first call, 'g_pos again' of the second, 'hint' (plane 0 as
    [B, bin rows, bin columns], or None without region hints).  The forward of the two calls must be bit-identical."""
    H, W = inp['res']
    ctx = ops.RasterizeGLContext(output_db=form != 'no rast_db', device='cuda')
    tri, go, go_db = inp['tri'].cuda(), inp['go'].cuda(), inp['go_db'].cuda()
    runs = []
    for _ in range(2):
        pos = inp['pos'].cuda().requires_grad_(True)
        rast, db = ops.rasterize(ctx, pos, tri, (H, W), ranges=inp['ranges'], grad_db=form == 'grad_db')
        B = rast.shape[0]
        assert rast.shape == (B, H, W, 4) and db.shape == (B, H, W, 0 if form == 'no rast_db' else 4)
        h = ops._hint_of(rast, 'rast')
        outs, gos = ([rast], [go]) if form == 'no rast_db' else ([rast, db], [go, go_db])
        g, = torch.autograd.grad(outs, [pos], gos)
        assert g.shape == inp['pos'].shape
        got = {'ids': rast[..., 3].detach().cpu().to(torch.int32), 'rast': rast[..., :3].detach().cpu().contiguous(), 'g_pos': g.cpu(),
               'hint': None if h is None else h[0].cpu().reshape(2, B, (H + 31) // 32, (W + 31) // 32)[0]}
        if form != 'no rast_db':
            got['rast_db'] = db.detach().cpu()
        runs.append(got)
    for k in ('ids',) + FORWARD:
        if k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), ('a second identical call differs', k)
    runs[0]['g_pos again'] = runs[1]['g_pos']
    return runs[0]


def _check(label, inp, form, got, ref, r32, k32, zeros, one_term):
    """The bars of the module docstring on one call's outputs."""
    assert torch.equal(got['ids'], inp['ids'].to(torch.int32)), (label, 'ids differ from the oracle')
    for k in FORWARD:
        if k not in got:
            continue
        x = got[k]
        e, nz = R.measure(x, *ref[k])
        e32, _ = R.measure(r32[k][0], *ref[k])
        _report(label, k, e, e32, 8 * e32 + 4)
        assert nz == zeros[k], (label, k, nz, zeros[k])
        differ = (x != k32[k]) | (torch.isnan(x) != torch.isnan(k32[k]))
        assert torch.equal(x, k32[k]), (label, k, 'not bit-identical to float32_in_kernel_order', int(differ.sum()), differ.nonzero()[:4].tolist())
        assert e <= 8 * e32 + 4, (label, k, e, e32)
    px = k32['px']
    uv = got['rast'][px.bi, px.yy, px.xx][R.corner_pixels(px)]
    assert bool((((uv[:, 0] == 0) | (uv[:, 0] == 1)) & ((uv[:, 1] == 0) | (uv[:, 1] == 1))).all()), (label, 'a corner pixel is not exact')
    r, S = ref['g_pos']
    e32, _ = R.measure(r32['g_pos'][0], r, S)
    for k in ('g_pos', 'g_pos again'):
        e, nz = R.measure(got[k], r, S)
        _report(label, k, e, e32, 8 * e32 + 4)
        assert nz == zeros['g_pos'], (label, k, nz, zeros['g_pos'])
        assert e <= 8 * e32 + 4, (label, k, e, e32)
        if one_term:
            differ = got[k] != k32['g_pos one term']
            assert torch.equal(got[k], k32['g_pos one term']), (label, k, 'not bit-identical to the float32 statement of shade_pixel_bwd',
                                                                int(differ.sum()), differ.nonzero()[:4].tolist())


@pytest.mark.parametrize("name,form", R.FORMS, ids=R.FORM_IDS)
def test_rasterize_entries_against_float64(name, form, oracle_ops):
    from fpc_diffrend_amd import ops
    inp = R.case_inputs(name, oracle_ops)
    ref, r32, k32 = R.reference(inp, form), R.reference(inp, form, torch.float32), R.kernel_order(inp, form)
    zeros = R.predicted_zeros(inp, grad_db=form == 'grad_db', output_db=form != 'no rast_db')
    one_term = R.CASES[name][1] == 'one'
    label = f"{name} ({form})"
    got = _call(ops, inp, form)
    _check(label, inp, form, got, ref, r32, k32, zeros, one_term)
    # the hint rides on the tensor rasterize returned: conservative, and with empty bins where nothing is drawn
    assert got['hint'] is not None, (label, 'rast carries no hint')
    coverage = I.make_hint(torch.cat([got['rast'], got['ids'][..., None].float()], -1))[0]
    assert bool((got['hint'] >= coverage).all()) and bool((got['hint'] <= 1).all()), label
    if R.CASES[name][0] == 'lattice':
        assert int((got['hint'][:, :, 3] == 0).sum()) == 3 and int(got['hint'].sum()) == 9, (label, got['hint'].tolist())
    if name == 'range':
        assert int(got['hint'][2].sum()) == 0, label                  # the empty range
    # the same call without region hints: the dense k_grad
    with ops.no_region_hints():
        dense = _call(ops, inp, form)
    assert dense['hint'] is None
    _check(label + ' (no hints)', inp, form, dense, ref, r32, k32, zeros, one_term)
    for k in FORWARD:
        if k in got:
            assert torch.equal(got[k], dense[k]), (label, k, 'the hint changes a result')

"""GPU: the antialias operator (csrc/antialias.hip over aa_pairs.h and sil_bits.h) entry by entry against float64
(tests/antialias_ref.py), through fpc_diffrend_amd.ops.antialias, or ops._antialias_func.apply where a region hint is supplied, and
ops.antialias_construct_topology_hash against the dict statement of the edge rule (torch.equal).

Every output x is compared with float64 arithmetic on the float32 inputs the kernels read, evaluated on the float32 decisions of
antialias_ref.decisions (no candidate pair of a case lies within 64 u of one; `ties` is dyadic and decides exactly alike):
e = max_i |x_i - r_i| / S_i in units of u = 2^-24, S_i the first-order rounding scale of entry i carried from the inputs down.  An entry
with S_i = 0 has no term: such a pixel of `out` is `color` bit for bit, such an entry of g_color is dy bit for bit, the z column of g_pos
and the rows of vertices of no active edge are exactly 0, and their number must be the one the decisions predict.
  out, g_color (plain stores): torch.equal to antialias_ref.float32_in_kernel_order -- the library is built with -ffp-contract=off, and
              DESIGN.md ("Accuracy bars") states that float outputs are bit-identical to unfused float32 arithmetic --, AND
              e <= 8 * e32 + 4, e32 the error of the same formula in float32 by torch on the CPU; in `ties` out equals float64 itself;
  g_pos (float atomics): e <= 8 * e32 + 4; in `soup/one-term` every entry has one term and g_pos is bit-identical to the statement.
Every call is made twice: out and g_color must be bit-identical between the two, g_pos must meet its bar both times.  Each call asserts
through antialias_ref.dispatch, on the pointers it hands in (dy's as a hook on `out` sees it), the kernels and copy pieces it reaches.
A hinted case is also run without its hint, with a triangle's pixels planted in the bins whose plane 1 is off and, with empty_color,
with NaN colour planted there: out and g_color must come back with the same bits (this is what shows that the hinted branches are
taken); `boost` is also run with boost 1 and must give the same out and g_color.  The flag planes are not exposed: a pair missing from
them shows as an entry of g_color that still equals dy, or as a missing term of g_pos.  tests/test_antialias_ref.py shows on the CPU,
for each case, the structural condition that makes it reach its branch, that float32 reaches these bars, that the statement's backward
equals autograd through the oracle in float64, and that fourteen wrong restatements miss the bars.
Every line below is printed by a test as "AA-ROW case output calls e_gpu e32 closest" (pytest -s).

Measured on an MI355X (units of u; the largest over the calls of a row, a call being one forward and backward of a case or of its
boost-1 / unhinted / planted / NaN-colour twin, and for g_pos each of the two calls; the last column is the call of the row that came
closest to its own bound).  out and g_color of every call were bit-identical to float32_in_kernel_order, out of `ties` to float64
itself, and g_pos of `soup/one-term` to the statement; adj of the nine topology cases equalled the dict statement.  g_pos is finished
by atomics and moves in its last digits from run to run.  One host bug was found and fixed: with B H W C < 4 fpcdr_antialias_bwd
launched k_copy_f4_chunk on a grid of 0 workgroups, and the backward of the three `tiny` cases raised "launch failed: invalid
configuration argument" (seen on the MI355X with the library built from the unfixed source); the launch is now skipped and the
remainder copy carries the floats.  Over the cases dispatch() saw k_aa_fwd<0|1|3|4> and k_aa_bwd_fix<0|1|3|4>, k_aa_fill_bin1 running
and not (with a hint: W % 4 != 0, C = 3, colour 8 bytes off), the flag planes cleared by memset and by lane 0, and the copy as
unrolled pieces, tail loop, remainder and hipMemcpyAsync.  The whole file, 27 cases of the operator and 9 of the topology, ran in
5.8 s there and in 4.2 s on a later visit, next to 4.1 s of test_gpu_rasterize.py and 3.9 s of test_gpu_interpolate.py (the first case takes 1.1 s, start-up
included; the time holds the building of the cases and their references on the CPU):

  case                   output   calls max e_gpu  max e32   closest to its bound (e_gpu / bound, call)
  ties                   out        1    0.000    0.000   0.00 / 4.0  ties
  ties                   g_color    1    0.000    0.000   0.00 / 4.0  ties
  ties                   g_pos      2    0.000    0.000   0.00 / 4.0  ties
  soup/C1                out        1    0.558    0.558   0.56 / 8.5  soup/C1
  soup/C1                g_color    1    0.552    0.552   0.55 / 8.4  soup/C1
  soup/C1                g_pos      2    0.339    0.369   0.34 / 7.0  soup/C1
  soup/C3                out        1    0.584    0.584   0.58 / 8.7  soup/C3
  soup/C3                g_color    1    0.558    0.558   0.56 / 8.5  soup/C3
  soup/C3                g_pos      2    0.376    0.376   0.38 / 7.0  soup/C3
  soup/C4                out        1    0.572    0.572   0.57 / 8.6  soup/C4
  soup/C4                g_color    1    0.583    0.583   0.58 / 8.7  soup/C4
  soup/C4                g_pos      2    0.285    0.285   0.28 / 6.3  soup/C4
  soup/C2                out        1    0.567    0.567   0.57 / 8.5  soup/C2
  soup/C2                g_color    1    0.556    0.556   0.56 / 8.4  soup/C2
  soup/C2                g_pos      2    0.307    0.307   0.31 / 6.5  soup/C2
  soup/C5                out        1    0.563    0.563   0.56 / 8.5  soup/C5
  soup/C5                g_color    1    0.554    0.554   0.55 / 8.4  soup/C5
  soup/C5                g_pos      2    0.369    0.369   0.37 / 6.9  soup/C5
  soup/one-term          out        1    0.568    0.568   0.57 / 8.5  soup/one-term
  soup/one-term          g_color    1    0.558    0.558   0.56 / 8.5  soup/one-term
  soup/one-term          g_pos      2    0.620    0.620   0.62 / 9.0  soup/one-term
  mesh/B3                out        1    0.609    0.609   0.61 / 8.9  mesh/B3
  mesh/B3                g_color    1    0.618    0.618   0.62 / 8.9  mesh/B3
  mesh/B3                g_pos      2    0.166    0.152   0.17 / 5.2  mesh/B3
  wide                   out        1    0.624    0.624   0.62 / 9.0  wide
  wide                   g_color    1    0.586    0.586   0.59 / 8.7  wide
  wide                   g_pos      2    0.233    0.233   0.23 / 5.9  wide
  range                  out        1    0.598    0.598   0.60 / 8.8  range
  range                  g_color    1    0.600    0.600   0.60 / 8.8  range
  range                  g_pos      2    0.178    0.178   0.18 / 5.4  range
  boost                  out        1    0.584    0.584   0.58 / 8.7  boost
  boost                  g_color    1    0.558    0.558   0.56 / 8.5  boost
  boost                  g_pos      2    0.321    0.321   0.32 / 6.6  boost
  hint/W100/C1           out        3    0.532    0.532   0.53 / 8.3  hint/W100/C1
  hint/W100/C1           g_color    3    0.548    0.548   0.55 / 8.4  hint/W100/C1
  hint/W100/C1           g_pos      6    0.241    0.241   0.24 / 5.9  hint/W100/C1
  hint/W100/C1/empty     out        4    0.502    0.502   0.50 / 8.0  hint/W100/C1/empty
  hint/W100/C1/empty     g_color    4    0.551    0.551   0.55 / 8.4  hint/W100/C1/empty
  hint/W100/C1/empty     g_pos      8    0.215    0.226   0.21 / 5.8  hint/W100/C1/empty
  hint/W100/C1+8B        out        3    0.486    0.486   0.49 / 7.9  hint/W100/C1+8B
  hint/W100/C1+8B        g_color    3    0.524    0.524   0.52 / 8.2  hint/W100/C1+8B
  hint/W100/C1+8B        g_pos      6    0.142    0.158   0.14 / 5.3  hint/W100/C1+8B
  hint/W100/C1+8B/empty  out        4    0.529    0.529   0.53 / 8.2  hint/W100/C1+8B/empty
  hint/W100/C1+8B/empty  g_color    4    0.549    0.549   0.55 / 8.4  hint/W100/C1+8B/empty
  hint/W100/C1+8B/empty  g_pos      8    0.146    0.092   0.15 / 4.7  hint/W100/C1+8B/empty
  hint/W100/C3           out        3    0.568    0.568   0.57 / 8.5  hint/W100/C3
  hint/W100/C3           g_color    3    0.570    0.570   0.57 / 8.6  hint/W100/C3
  hint/W100/C3           g_pos      6    0.100    0.177   0.10 / 5.4  hint/W100/C3
  hint/W100/C3/empty     out        4    0.529    0.529   0.53 / 8.2  hint/W100/C3/empty
  hint/W100/C3/empty     g_color    4    0.554    0.554   0.55 / 8.4  hint/W100/C3/empty
  hint/W100/C3/empty     g_pos      8    0.096    0.086   0.10 / 4.7  hint/W100/C3/empty
  hint/W102/C1           out        3    0.570    0.570   0.57 / 8.6  hint/W102/C1
  hint/W102/C1           g_color    3    0.591    0.591   0.59 / 8.7  hint/W102/C1
  hint/W102/C1           g_pos      6    0.124    0.122   0.12 / 5.0  hint/W102/C1
  hint/W102/C1/empty     out        4    0.575    0.575   0.57 / 8.6  hint/W102/C1/empty
  hint/W102/C1/empty     g_color    4    0.578    0.578   0.58 / 8.6  hint/W102/C1/empty
  hint/W102/C1/empty     g_pos      8    0.110    0.198   0.11 / 5.6  hint/W102/C1/empty
  copy/105               out        1    0.523    0.523   0.52 / 8.2  copy/105
  copy/105               g_color    1    0.275    0.275   0.28 / 6.2  copy/105
  copy/105               g_pos      2    0.102    0.137   0.10 / 5.1  copy/105
  copy/2211              out        1    0.391    0.391   0.39 / 7.1  copy/2211
  copy/2211              g_color    1    0.389    0.389   0.39 / 7.1  copy/2211
  copy/2211              g_pos      2    0.243    0.243   0.24 / 5.9  copy/2211
  copy/4096              out        1    0.345    0.345   0.34 / 6.8  copy/4096
  copy/4096              g_color    1    0.348    0.348   0.35 / 6.8  copy/4096
  copy/4096              g_pos      2    0.133    0.133   0.13 / 5.1  copy/4096
  copy/dy+8B             out        1    0.391    0.391   0.39 / 7.1  copy/dy+8B
  copy/dy+8B             g_color    1    0.446    0.446   0.45 / 7.6  copy/dy+8B
  copy/dy+8B             g_pos      2    0.377    0.377   0.38 / 7.0  copy/dy+8B
  copy/dy-stride0        out        1    0.264    0.264   0.26 / 6.1  copy/dy-stride0
  copy/dy-stride0        g_color    1    0.208    0.208   0.21 / 5.7  copy/dy-stride0
  copy/dy-stride0        g_pos      2    0.127    0.127   0.13 / 5.0  copy/dy-stride0
  tiny/1x2               out        1    0.271    0.271   0.27 / 6.2  tiny/1x2
  tiny/1x2               g_color    1    0.234    0.234   0.23 / 5.9  tiny/1x2
  tiny/1x2               g_pos      2    0.177    0.177   0.18 / 5.4  tiny/1x2
  tiny/1x1               out        1    0.000    0.000   0.00 / 4.0  tiny/1x1
  tiny/1x1               g_color    1    0.000    0.000   0.00 / 4.0  tiny/1x1
  tiny/1x1               g_pos      2    0.000    0.000   0.00 / 4.0  tiny/1x1
  tiny/2x1               out        1    0.183    0.183   0.18 / 5.5  tiny/2x1
  tiny/2x1               g_color    1    0.233    0.233   0.23 / 5.9  tiny/2x1
  tiny/2x1               g_pos      2    0.258    0.258   0.26 / 6.1  tiny/2x1
"""
import pytest
import torch

import antialias_ref as R

pytestmark = pytest.mark.gpu

NON_ATOMIC = ('out', 'g_color')


def _offset_view(t, n_floats):
    """A contiguous copy of t that starts n_floats floats into a larger buffer."""
    buf = torch.zeros(t.numel() + n_floats + 4, dtype=t.dtype, device='cuda')
    v = buf[n_floats:n_floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _call(ops, inp, case, hint=None, rast=None, color=None, boost=None, hinted_path=False):
    """One forward and backward, made twice -> (name -> tensor of the first, with 'g_pos again' of the second; dispatch() on the pointers
    handed in).  The first backward is torch.autograd.grad, the second .backward()."""
    C = inp['color'].shape[-1]
    tri, rast = inp['tri'].cuda(), (inp['rast'] if rast is None else rast).cuda()
    boost = inp['boost'] if boost is None else boost
    src = inp['color'] if color is None else color
    empty = inp['empty_color'].cuda() if (inp['empty_color'] is not None and hint is not None) else None
    runs, seen = [], []
    for how in ('grad', 'backward'):
        col = (_offset_view(src, 2) if case['color_off'] else src.cuda()).requires_grad_(True)
        pos = inp['pos'].cuda().requires_grad_(True)
        assert col.is_contiguous() and col.data_ptr() % 16 == (8 if case['color_off'] else 0)
        if hinted_path:
            adj = ops.antialias_construct_topology_hash(tri)
            out = ops._antialias_func.apply(col, rast, pos, tri, adj, boost, hint, empty)
        else:
            out = ops.antialias(col, rast, pos, tri, pos_gradient_boost=boost)
        assert out.shape == col.shape and out.data_ptr() % 16 == 0
        ptr = []
        out.register_hook(lambda g: ptr.append(g.data_ptr() if g.is_contiguous() else 0))      # (what is not contiguous is copied first)
        if case['dy'] == 'stride0':
            loss, dy = out.sum(), None
        else:
            dy = _offset_view(inp['dy'], 2) if case['dy'] == 'offset' else inp['dy'].cuda()
            assert dy.data_ptr() % 16 == (8 if case['dy'] == 'offset' else 0)
        if how == 'grad':
            g = torch.autograd.grad(loss, [col, pos]) if dy is None else torch.autograd.grad(out, [col, pos], dy)
            assert col.grad is None and pos.grad is None
        else:
            loss.backward() if dy is None else out.backward(dy)
            g = [col.grad, pos.grad]
        assert g[1].shape == inp['pos'].shape and len(ptr) == 1
        kernels = R.dispatch(C, rast.shape[2], hint is not None, (col.data_ptr(), out.data_ptr(), ptr[0], None), out.numel())
        seen.append(kernels)
        runs.append({'out': out.detach().clone(), 'g_color': g[0].detach().clone(), 'g_pos': g[1].detach().clone()})
    assert seen[0] == seen[1]
    for k in NON_ATOMIC:
        assert torch.equal(runs[0][k], runs[1][k]), ('a second identical call differs', k)
    runs[0]['g_pos again'] = runs[1]['g_pos']
    return runs[0], seen[0]


class _Rows:
    """The report: per (case, output) the calls' e_gpu, e32 and bounds."""

    def __init__(self, case):
        self.case, self.rows = case, {}

    def check(self, call, inp, got, ref, r32, k32):
        for twice in ('', ' again'):
            x = {k: got[k] for k in NON_ATOMIC} if not twice else {}
            x['g_pos'] = got['g_pos' + twice]
            rep = lambda k, e, e32, bound: self.rows.setdefault(k, []).append((e, e32, bound, call + twice))
            bad = R.failures(inp, ref, r32, k32, {k: v.cpu() for k, v in x.items()}, rep)
            assert not bad, (call + twice, bad)

    def print(self):
        for k, calls in self.rows.items():
            e, e32 = max(c[0] for c in calls), max(c[1] for c in calls)
            close = max(calls, key=lambda c: c[0] / c[2])
            print(f"AA-ROW {self.case:<22} {k:<8} {len(calls):>3} {e:>8.3f} {e32:>8.3f}   {close[0]:.2f} / {close[2]:.1f}  {close[3]}")


def _want(case):
    B, H, W = R.SHAPES[case['geom']]
    return R.dispatch(case['C'], W, case['hint'], (8 if case['color_off'] else 0, 0, 8 if case['dy'] == 'offset' else 0, 0), B * H * W * case['C'])


def _same_non_atomic(name, a, b, what):
    for k in NON_ATOMIC:
        assert torch.equal(a[k], b[k]), (name, k, what)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_antialias_entries_against_float64(name):
    from fpc_diffrend_amd import ops
    case = R.CASES[R.CASE_IDS.index(name)]
    inp = R.case_inputs(name)
    ref, r32, k32 = R.reference(inp), R.reference(inp, torch.float32), R.kernel_order(inp)
    rows = _Rows(name)
    hint = inp['hint'].cuda() if case['hint'] else None
    got, kernels = _call(ops, inp, case, hint, hinted_path=case['hint'])
    assert kernels == _want(case), (name, kernels, _want(case))
    print(f"AA {name} kernels {kernels['fwd']} {'k_aa_fill_bin1 ' if kernels['fill'] else ''}flags cleared by {kernels['clear']}, copy {'+'.join(kernels['copy'])}, "
          f"{kernels['bwd']}{' hinted' if case['hint'] else ''}")
    rows.check(name, inp, got, ref, r32, k32)
    if case['boost'] != 1.0:            # boost scales g_pos alone
        plain, pk = _call(ops, inp, case, boost=1.0)
        assert pk == kernels and not torch.equal(plain['g_pos'], got['g_pos'])
        _same_non_atomic(name, got, plain, 'boost changes out or g_color')
    if case['hint']:
        dense, dk = _call(ops, inp, case, None, hinted_path=True)           # the same call without its hint: the same bits
        assert dk == dict(kernels, fill=False, clear='lane 0')
        rows.check(name + ' (no hint)', inp, dense, ref, r32, k32)
        _same_non_atomic(name, got, dense, 'the hint changes a result')
        # the hinted branches are taken: a triangle's pixels planted in the bins whose plane 1 is off, which a hinted kernel does not read
        planted, pk = _call(ops, inp, case, hint, rast=inp['rast_planted'], hinted_path=True)
        assert pk == kernels
        rows.check(name + ' (off bins planted)', inp, planted, ref, r32, k32)
        _same_non_atomic(name, got, planted, 'an off bin was read')
        if case['empty']:               # ... and its colour is not read either: out there is the constant
            B, H, W = R.SHAPES[case['geom']]
            off = R.plane1_off_pixels(inp['hint'], B, H, W)
            nan = inp['color'].clone()
            nan[off] = float('nan')
            poisoned, pk = _call(ops, inp, case, hint, rast=inp['rast_planted'], color=nan, hinted_path=True)
            assert pk == kernels and bool((poisoned['out'].cpu()[off] == inp['empty_color']).all())
            rows.check(name + ' (NaN colour planted)', inp, poisoned, ref, r32, k32)
            _same_non_atomic(name, got, poisoned, "an off bin's colour was read")
    rows.print()


@pytest.mark.parametrize("name", R.TOPOLOGY_IDS)
def test_topology_equals_the_edge_rule(name):
    from fpc_diffrend_amd import ops
    tri = R.topology_tri(name)
    assert int(tri.min()) >= 0
    adj = ops.antialias_construct_topology_hash(tri.cuda()).cpu()
    assert adj.dtype == torch.int32 and torch.equal(adj, R.topology(tri)), name
    if name.endswith('permuted'):       # the same rows, permuted with the triangles
        base = R.topology_tri(name[:-len('/permuted')])
        look = {tuple(t): r for t, r in zip(base.tolist(), ops.antialias_construct_topology_hash(base.cuda()).cpu().tolist())}
        assert [look[tuple(t)] for t in tri.tolist()] == adj.tolist()
    print(f"AA topology {name}: T = {tri.shape[0]}, capacity {R.topo_capacity(tri.shape[0])}")

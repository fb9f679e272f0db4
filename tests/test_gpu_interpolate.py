"""GPU: the interpolate operator (csrc/interpolate.hip) entry by entry against float64 (tests/interpolate_ref.py), through
fpc_diffrend_amd.ops.interpolate, or ops._interpolate_func.apply where a region hint is supplied.

Every output x is compared with float64 arithmetic on the float32 inputs the kernel read: e = max_i |x_i - r_i| / S_i in units of
u = 2^-24, S_i the sum of the absolute values of the terms of entry i; entries with S_i = 0 have no term, must be exactly 0, and their
number must be the one the construction predicts (uncovered pixels, ids the t >= T clamp rejects, pixels without a gradient, .z and
.w of g_rast, the vertices no triangle names or only pixels without a gradient show).
  short paths (out, out_da, g_rast, g_rast_db): e <= n + 2, n derived in interpolate_ref.py (5, 3, A + 1, n_diff + 1), AND torch.equal
              to interpolate_ref.float32_in_kernel_order: the library is built with -ffp-contract=off, and DESIGN.md ("Accuracy bars")
              states that float outputs are bit-identical to unfused float32 arithmetic;
  long sum (g_attr: over every pixel that shows a vertex, finished by atomics): e <= 8 * e32 + 4, e32 the error of float32 torch on
              the CPU (interpolate_ref.interpolate, dtype=float32) against the same reference.
At (u, v) = (1, 0), (0, 1), (0, 0) out equals the attribute of that corner bit for bit.  Each case asserts through
interpolate_ref.dispatch, on the pointers it hands in, the kernels it reaches; a + 8 B case (attr starts 8 bytes into a buffer) is also
run aligned, a hinted case also without its hint and with covered-looking pixels planted in the bins the hint switches off (a hinted
kernel does not read them: this is what shows that the hinted branch is taken), and the four non-atomic outputs must be bit-identical
between such calls; every call is made twice and they must be bit-identical between the two.  tests/test_interpolate_ref.py shows on
the CPU, for each case, that float32 reaches these bars and that nine wrong restatements miss them.
Every line below is printed by a test as "INTERP case output e_gpu e32 bound" (pytest -s).

Measured on an MI355X (units of u; the largest over the calls of a row, a call being one forward and backward of a case or of its
aligned / unhinted / planted twin; e32 "-": the bound is n + 2, derived, no yardstick is measured; the last column is the call of the
row that came closest to its own bound).  All four non-atomic outputs of every call were bit-identical to float32_in_kernel_order:
no kernel or host bug was found.  g_attr is finished by atomics and its largest error moves between 1.5 and 2.3 u from run to run.  The
whole file, 35 cases of the operator and the public path, runs in 3.9 s there (the first case carries 1.1 s of start-up):

  kernel              output     calls max e_gpu  max e32   closest to its bound (e_gpu / bound, call)
  k_interp_fwd<0>     out           24      2.66        -   2.66 / 7.0  stream/A32/all
  k_interp_fwd<0>     out_da        22      2.44        -   2.44 / 5.0  stream/A32/all
  k_interp_fwd<2>     out           14      2.72        -   2.72 / 7.0  stream/A2/all
  k_interp_fwd<2>     out_da         6      2.15        -   2.15 / 5.0  stream/A2/all
  k_interp_fwd_bin2   out           11      2.41        -   2.41 / 7.0  hint/bin/A2/attr
  k_interp_bwd<true>  g_rast        24      2.39        -   2.23 / 5.0  hint/bin/A2/attr
  k_interp_bwd<true>  g_rast_db     16      2.52        -   2.17 / 5.0  gen/A3/[2,0]/attr
  k_interp_bwd<true>  g_attr        48      1.54     2.75   1.38 / 12.4  gen/A2+8B/attr
  k_interp_bwd_rows   g_rast        19      2.56        -   2.46 / 5.0  hint/gen/A2+8B
  k_interp_bwd_rows   g_rast_db     12      2.43        -   2.31 / 5.0  stream/A2/all
  k_interp_bwd_bin2   g_rast         6      2.13        -   2.13 / 5.0  bin44/A2/confetti
"""
import pytest
import torch

import interpolate_ref as R

pytestmark = pytest.mark.gpu


def _report(case, name, e, e32, bound):
    print(f"INTERP {case} {name} e_gpu={e:.3f} e32={'-' if e32 is None else format(e32, '.3f')} bound={bound:.1f}")


def _offset_view(t, n_floats):
    """A contiguous copy of t that starts n_floats floats into a larger buffer."""
    buf = torch.zeros(t.numel() + n_floats + 4, dtype=t.dtype, device='cuda')
    v = buf[n_floats:n_floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _call(ops, inp, attr_grad, misalign=False, hint=None, public=None):
    """One forward and backward -> (name -> tensor, (forward kernel, backward kernel) by dispatch() on the pointers handed in).
    The first run's backward is torch.autograd.grad; the second goes through .backward() and finds no gradient nobody asked for."""
    dl, nd = inp['diff_list'], len(inp['diff_list'])
    tri, go = inp['tri'].cuda(), inp['go'].cuda()
    go_da = inp['go_da'].cuda() if nd else None
    runs = []
    for how in ('grad', 'backward'):
        attr = (_offset_view(inp['attr'], 2) if misalign else inp['attr'].cuda()).requires_grad_(attr_grad)
        if public is not None:
            rast, db = public
            rast.grad = db.grad = None
        else:
            rast = inp['rast'].cuda().requires_grad_(True)
            db = inp['rast_db'].cuda().requires_grad_(True) if nd else None
        assert attr.is_contiguous() and attr.data_ptr() % 16 == (8 if misalign else 0)
        if hint is not None:
            out, out_da = ops._interpolate_func.apply(attr, rast, tri, db, dl, hint)
        else:
            out, out_da = ops.interpolate(attr, rast, tri, rast_db=db, diff_attrs=dl if nd else None)
        A = attr.shape[2]
        assert out.shape == rast.shape[:3] + (A,) and out_da.shape == rast.shape[:3] + (2 * nd,)
        kernels = R.dispatch(A, nd, rast.shape[2], attr_grad, (attr.data_ptr(), out.data_ptr(), go.data_ptr()))
        outs, gos = ([out, out_da], [go, go_da]) if nd else ([out], [go])
        wrt = [rast] + ([db] if nd else []) + ([attr] if attr_grad else [])
        if how == 'grad':
            g = list(torch.autograd.grad(outs, wrt, gos))
            assert all(t.grad is None for t in wrt)
        else:
            torch.autograd.backward(outs, gos)
            g = [t.grad for t in wrt]
            assert attr_grad or attr.grad is None               # a gradient that was not requested is None
            assert nd or (db is None or db.grad is None)
        got = {'out': out.detach(), 'g_rast': g[0]}
        if nd:
            got.update(out_da=out_da.detach(), g_rast_db=g[1])
        if attr_grad:
            got['g_attr'] = g[-1]
        runs.append({k: v.detach().clone() for k, v in got.items()})
    for k in R.NON_ATOMIC:
        if k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), ('a second identical call differs', k)
    if attr_grad:
        runs[0]['g_attr again'] = runs[1]['g_attr']
    return runs[0], kernels, out


def _check(name, inp, got, ref, r32, k32):
    """The bars of the module docstring on one call's outputs."""
    A, nd = inp['attr'].shape[2], len(inp['diff_list'])
    n = R.bounds(A, nd)
    zeros = R.predicted_zeros(inp['attr'], inp['rast'], inp['tri'], inp['diff_list'], inp['go'])
    assert set(got) - {'g_attr', 'g_attr again'} == set(k32), (name, set(got), set(k32))
    for k in R.NON_ATOMIC:
        if k not in got:
            continue
        x = got[k].cpu()
        e, nz = R.measure(x, *ref[k])
        _report(name, k, e, None, n[k] + 2)
        assert nz == zeros[k], (name, k, nz, zeros[k])
        assert e <= n[k] + 2, (name, k, e)
        differ = (x != k32[k]) | (torch.isnan(x) != torch.isnan(k32[k]))
        assert torch.equal(x, k32[k]), (name, k, 'not bit-identical to float32_in_kernel_order', int(differ.sum()), differ.nonzero()[:4].tolist())
    for k in ('g_attr', 'g_attr again'):
        if k in got:
            r, S = ref['g_attr']
            e, nz = R.measure(got[k], r, S)
            e32, _ = R.measure(r32['g_attr'][0], r, S)
            _report(name, k, e, e32, 8 * e32 + 4)
            assert nz == zeros['g_attr'], (name, k, nz, zeros['g_attr'])
            assert e <= 8 * e32 + 4, (name, k, e, e32)
    at = inp['attr']
    for b, y, x, corner in inp.get('exact', ()):
        t = int(inp['rast'][b, y, x, 3]) - 1
        assert torch.equal(got['out'][b, y, x].cpu(), at[b if at.shape[0] > 1 else 0, int(inp['tri'][t, corner])]), (name, 'exact pixel', b, y, x)


def _same_non_atomic(name, a, b, what):
    for k in R.NON_ATOMIC:
        if k in a:
            assert torch.equal(a[k], b[k]), (name, k, what)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_interpolate_entries_against_float64(name):
    from fpc_diffrend_amd import ops
    case = R.CASES[R.CASE_IDS.index(name)]
    inp = R.case_inputs(case)
    ref, r32, k32 = R.reference(inp), R.reference(inp, torch.float32), R.kernel_order(inp)
    A, nd, W = case['A'], len(inp['diff_list']), case['img'][2]
    want = R.dispatch(A, nd, W, case['attr_grad'], (8,) if case['misalign'] else ())
    hint = inp['hint'].cuda() if case['hint'] else None
    got, kernels, _ = _call(ops, inp, case['attr_grad'], case['misalign'], hint)
    assert kernels == want, (name, kernels, want)
    print(f"INTERP {name} kernels {kernels[0]} {kernels[1]}{' hinted' if case['hint'] else ''}")
    _check(name, inp, got, ref, r32, k32)
    if case['misalign']:            # the aligned twin takes the bin-shaped kernels: the same bits
        twin, tk, _ = _call(ops, inp, case['attr_grad'], False, hint)
        assert tk != kernels and 'bin2' in tk[0] and kernels == ('k_interp_fwd<2>', 'k_interp_bwd<true>' if case['attr_grad'] else 'k_interp_bwd_rows')
        _same_non_atomic(name, got, twin, 'the aligned twin differs')
    if case['hint']:                # the same call without its hint: the same kernels, the same bits
        h = inp['hint']
        assert bool((h[0, :, :, -1] == 0).any()) and bool(((h[0] == 1) & (R.make_hint(inp['rast'])[0] == 0)).any()) and bool(R.make_hint(inp['rast'])[0].any())
        dense, dk, _ = _call(ops, inp, case['attr_grad'], case['misalign'], None)
        assert dk == kernels
        _check(name + ' (no hint)', inp, dense, ref, r32, k32)
        _same_non_atomic(name, got, dense, 'the hint changes a result')
        # the hinted branch is taken: with covered-looking pixels planted in the off bins, which a hinted kernel does not read,
        # the results are still those of the clean rast
        planted, pk, _ = _call(ops, dict(inp, rast=R.poison_off_bins(inp['rast'], h)), case['attr_grad'], case['misalign'], hint)
        assert pk == kernels
        _check(name + ' (off bins planted)', inp, planted, ref, r32, k32)
        _same_non_atomic(name, got, planted, 'an off bin was read')


def test_public_path_carries_the_rasteriser_hint():
    """dr.rasterize of two small triangles at (1, 70, 100), dr.interpolate on that very tensor: the hint is found, has empty bins, and
    rides on with `out`; the results are those of the dense path bit for bit and lie within the bounds of the reference on rast.cpu()."""
    from fpc_diffrend_amd import ops
    H, W = 70, 100
    g = torch.Generator().manual_seed(3)
    px = torch.tensor([[5.3, 8.2], [40.1, 10.4], [20.6, 45.7], [50.2, 20.1], [80.4, 25.3], [60.7, 50.6]])
    pos = torch.stack([2 * px[:, 0] / W - 1, 2 * px[:, 1] / H - 1, torch.zeros(6), torch.ones(6)], 1)[None].cuda()
    tri = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32)
    ctx = ops.RasterizeGLContext(device='cuda')
    rast, db = ops.rasterize(ctx, pos, tri.cuda(), (H, W))
    rast.requires_grad_(True)
    db.requires_grad_(True)
    h = ops._hint_of(rast, 'rast')
    assert h is not None
    hint = h[0].cpu().reshape(2, 1, 3, 4)
    assert int((hint[0] == 0).sum()) >= 6 and int(hint[0].sum()) >= 2 and bool((hint[0] >= R.make_hint(rast)[0]).all())
    inp = dict(attr=R._randn_away((1, 6, 3), g), rast=rast.detach().cpu(), tri=tri, rast_db=db.detach().cpu(), diff_list=[2, 0],
               go=R._randn_away((1, H, W, 3), g), go_da=R._randn_away((1, H, W, 4), g))
    covered = int((inp['rast'][..., 3] > 0).sum())
    assert set(inp['rast'][..., 3].unique().tolist()) == {0.0, 1.0, 2.0} and 500 < covered < 3000
    ref, r32, k32 = R.reference(inp), R.reference(inp, torch.float32), R.kernel_order(inp)
    got, kernels, out = _call(ops, inp, True, public=(rast, db))
    assert kernels == ('k_interp_fwd<0>', 'k_interp_bwd<true>')
    ho = ops._hint_of(out, 'zero')
    assert ho is not None and ho[0] is h[0] and ops._hint_of(rast, 'rast') is not None
    _check('public', inp, got, ref, r32, k32)
    with ops.no_region_hints():
        assert ops._hint_of(rast, 'rast') is None
        dense, dk, out2 = _call(ops, inp, True, public=(rast, db))
    assert dk == kernels and ops._hint_of(out2, 'zero') is None
    _check('public (no hints)', inp, dense, ref, r32, k32)
    _same_non_atomic('public', got, dense, 'the hint changes a result')

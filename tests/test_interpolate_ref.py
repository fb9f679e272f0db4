"""CPU: the float64 yardstick of the interpolate operator (tests/interpolate_ref.py) is right, and what
tests/test_gpu_interpolate.py asks of the kernels is reachable and discriminates:
  1. the reference's values and hand-written gradients equal torch.autograd through oracle.ops.interpolate evaluated in float64 to
     1e-12 of the entry's scale, on random inputs and on the inputs of every GPU case; every nonzero entry has S > 0;
  2. on the inputs of every GPU case float32_in_kernel_order meets every n + 2 bound, a float32 g_attr summed in another order than
     the e32 yardstick (pixels permuted; 64 at a time by vertex first, as a wave does) meets 8 e32 + 4, the entries without a term
     are as many as predicted, the deliberate pixels are there, and every kernel is reached by at least three cases, with and
     without a hint;
  3. nine wrong float32 restatements each exceed a bound, break a zero count or an exact pixel on at least one GPU case.
Lines "INTERP ..." are printed under pytest -s."""
import functools

import pytest
import torch

import interpolate_ref as R


@functools.lru_cache(maxsize=None)
def _four(name):
    case = R.CASES[R.CASE_IDS.index(name)]
    inp = R.case_inputs(case)
    return case, inp, R.reference(inp), R.reference(inp, torch.float32)


def _values(res):
    return {k: v[0] for k, v in res.items() if isinstance(v, tuple)}


def _oracle(inp, dtype):
    """oracle.ops.interpolate and torch.autograd on the inputs of a case, in dtype -> name -> tensor."""
    from oracle import ops
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True) if t is not None else None
    attr, rast, db = leaf(inp['attr']), leaf(inp['rast']), leaf(inp['rast_db'])
    nd = len(inp['diff_list'])
    out, out_da = ops.interpolate(attr, rast, inp['tri'], rast_db=db, diff_attrs=inp['diff_list'] if nd else None)
    loss = (out * inp['go'].to(dtype)).sum()
    if nd:
        loss = loss + (out_da * inp['go_da'].to(dtype)).sum()
    loss.backward()
    res = {'out': out.detach(), 'g_rast': rast.grad, 'g_attr': attr.grad}
    if nd:
        res.update(out_da=out_da.detach(), g_rast_db=db.grad)
    return res


def _assert_equal_to_autograd(name, inp, ref):
    got = _oracle(inp, torch.float64)
    assert set(_values(ref)) == set(got), (name, set(_values(ref)) ^ set(got))
    for k in got:
        r, S = ref[k]
        assert bool((S[r != 0] > 0).all()), (name, k)
        worst = float(((r - got[k]).abs() / S.clamp(min=1e-300)).max())
        assert worst <= 1e-12, (name, k, worst)


@pytest.mark.parametrize("A,diff,Ba", [(1, None, 1), (2, 'all', 2), (3, [2, 0, 2], 1), (5, [4], 2), (7, 'all', 1)])
def test_reference_equals_autograd_through_the_oracle_on_random_inputs(A, diff, Ba):
    g = torch.Generator().manual_seed(A)
    B, H, W, Vt, nT = 2, 7, 9, 12, 8
    dl = R.diff_indices(diff, A)
    rast = torch.cat([torch.rand(B, H, W, 3, generator=g) * 2 - 0.5, torch.randint(0, nT + 3, (B, H, W, 1), generator=g).float()], -1)
    inp = dict(attr=torch.randn(Ba, Vt, A, generator=g), rast=rast, tri=torch.randint(0, Vt, (nT, 3), generator=g).to(torch.int32),
               rast_db=torch.randn(B, H, W, 4, generator=g) if dl else None, diff_list=dl, go=torch.randn(B, H, W, A, generator=g),
               go_da=torch.randn(B, H, W, 2 * len(dl), generator=g) if dl else None)
    assert int((rast[..., 3] > nT).sum()) > 0 and int((rast[..., 3] == 0).sum()) > 0
    _assert_equal_to_autograd(f'random A={A}', inp, R.reference(inp))


def _failures(case, inp, ref, r32, got, exact=True):
    """What of `got` (name -> tensor) misses a check test_gpu_interpolate.py makes: a term where there is none, a zero count, a bound
    (n + 2, or 8 * e32 + 4 with e32 from the unmutated r32), an exact pixel."""
    n = R.bounds(case['A'], len(inp['diff_list']))
    zeros = R.predicted_zeros(inp['attr'], inp['rast'], inp['tri'], inp['diff_list'], inp['go'])
    bad = []
    for k, x in got.items():
        r, S = ref[k]
        if not bool((x[S == 0] == 0).all()):
            bad.append((k, 'a term where there is none'))
            continue
        e, nz = R.measure(x, r, S)
        if nz != zeros[k]:
            bad.append((k, 'zero count', nz, zeros[k]))
        limit = n[k] + 2 if k in n else 8 * R.measure(r32[k][0], r, S)[0] + 4
        if not e <= limit:
            bad.append((k, round(e, 1), round(limit, 1)))
    if exact and 'out' in got:
        at = inp['attr']
        for b, y, x, corner in inp['exact']:
            t = int(inp['rast'][b, y, x, 3]) - 1
            if not torch.equal(got['out'][b, y, x].float(), at[b if at.shape[0] > 1 else 0, int(inp['tri'][t, corner])]):
                bad.append(('out', 'exact pixel', (b, y, x)))
    return bad


def check_hint(case, inp):
    """A hinted case's map: an off bin in the last bin column and in the last bin row, an empty bin left on, occupied bins that hold
    uncovered pixels; and it is conservative: no pixel of an off bin is anything but zero."""
    B, H, W = case['img']
    h, rast = inp['hint'], inp['rast']
    assert h.dtype == torch.uint8 and tuple(h.shape) == (2, B, (H + 31) // 32, (W + 31) // 32)
    p0 = h[0].bool()
    assert bool((~p0[:, :, -1]).any()) and bool((~p0[:, -1, :]).any()), case['name']
    occupied = R.make_hint(rast)[0].bool()
    assert bool((p0 & ~occupied).any()) and bool(occupied.any()) and bool((p0 | ~occupied).all()), case['name']
    assert bool((h[1] >= h[0]).all()) and bool(h[1][0, 2, 3] == 1) and bool(h[0][0, 2, 3] == 0), case['name']   # (the far corner: off, a neighbour on)
    off = R.hint_off_pixels(h, B, H, W)
    assert int(off.sum()) > 0 and bool((rast[off] == 0).all())
    covered = R.reference(inp)['covered']
    for b in range(B):
        for by in range(p0.shape[1]):
            for bx in range(p0.shape[2]):
                if occupied[b, by, bx] and (by, bx) != (1, 0):          # (but for the bin covered in five pixels only)
                    sl = covered[b, by * 32:(by + 1) * 32, bx * 32:(bx + 1) * 32]
                    assert 0 < int((~sl).sum()) < sl.numel() // 2, (case['name'], by, bx)
    assert torch.equal(R.with_hint(rast, h), rast)
    # the poisoned twin (how the GPU file shows that a hinted kernel skips its off bins): covered pixels in every off bin and only there
    bad = R.poison_off_bins(rast, h)
    assert torch.equal(R.with_hint(bad, h), rast) and torch.equal((bad != rast).any(-1), off)
    assert bool(((bad[..., 3] >= 1) & (bad[..., 3] <= R.T))[off].all())


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_gpu_case_inputs_and_float32(name):
    """On the inputs of a GPU case: the reference equals float64 autograd; the deliberate pixels and vertices are there; the
    predicted entries without a term; float32 within the bounds."""
    case, inp, ref, r32 = _four(name)
    B, H, W = case['img']
    A, nd = case['A'], len(inp['diff_list'])
    assert inp['attr'].shape == (B if case['BaB'] else 1, R.VT, A) and inp['tri'].shape == (R.T, 3) and nd <= R.MAX_ATTR
    _assert_equal_to_autograd(name, inp, ref)
    # what the issue asks of the inputs
    tri, rast = inp['tri'].long(), inp['rast']
    ids = rast[..., 3]
    assert bool((ids >= 0).all()) and bool((ids == ids.round()).all()) and int(tri.min()) >= 0 and int(tri.max()) < R.VT
    for val in (0, R.T, R.T + 1, R.T + 7):
        assert int((ids == val).sum()) >= 3, (name, val)
    assert int(ids.max()) == R.T + 7
    assert tri[0, 0] == tri[1, 1] == tri[2, 2] == R.V_SHARED and tri[R.T_REPEATED, 0] == tri[R.T_REPEATED, 1]
    assert int((tri == R.V_UNUSED).sum()) == 0 and (tri == R.V_DEAD).nonzero().tolist() == [[R.T_DEAD, 0]]
    for t in R.T_SHARED + (R.T_REPEATED, R.T_DEAD):
        assert int((ids == t + 1).sum()) >= 3, (name, t)
    assert bool((inp['go'][ids == R.T_DEAD + 1] == 0).all()) and int((inp['go'] == 0).all(-1).sum()) == int((ids == R.T_DEAD + 1).sum())
    uv = rast[..., :2][ref['covered']]
    assert float(uv.min()) < -0.4 and float(uv.max()) > 1.4
    for t in [inp['attr'], inp['go'][ids != R.T_DEAD + 1]] + ([inp['rast_db'], inp['go_da'][ids != R.T_DEAD + 1]] if nd else []):
        assert float(t.abs().min()) >= 0.1
    assert len(inp['exact']) == 9 and {c for *_, c in inp['exact']} == {0, 1, 2}
    lay = R.LAYOUT[case['img']]
    for b, by, bx in lay['empty']:
        assert not bool(rast[b, by * 32:(by + 1) * 32, bx * 32:(bx + 1) * 32].any())
    for b, by, bx in lay['sparse']:
        assert int(ref['covered'][b, by * 32:(by + 1) * 32, bx * 32:(bx + 1) * 32].sum()) == 5
    tile = set(ids[0, 8:16, 32:40].reshape(-1).tolist()) - {0.0}          # an 8 x 8 tile of k_interp_bwd<true>: one wave
    if case['ids'] == 'confetti':       # tens of triangles among its 64 lanes
        assert len(tile) > ids[0, 8:16, 32:40].numel() // 3, (name, len(tile))
    elif case['ids'] == 'one':
        assert float((ids[0, 8:16, 32:40] == R.T_ONE + 1).float().mean()) > 0.7, (name, tile)
    if case['hint']:
        check_hint(case, inp)
    # the zeros the construction predicts: the dead and the unused vertex among them
    zeros = R.predicted_zeros(inp['attr'], rast, inp['tri'], inp['diff_list'], inp['go'])
    G, GS = ref['g_attr']
    assert bool((GS[:, [R.V_DEAD, R.V_UNUSED]] == 0).all()) and bool((GS[:, R.V_SHARED] > 0).all())
    # float32: the kernels' order on the short paths, the long sum in other orders than the yardstick's
    k32 = R.kernel_order(inp)
    assert not _failures(case, inp, ref, r32, k32), (name, _failures(case, inp, ref, r32, k32))
    assert not _failures(case, inp, ref, r32, _values(r32)), name
    n = R.bounds(A, nd)
    for k, x in k32.items():
        e, nz = R.measure(x, *ref[k])
        print(f"INTERP {name} {k} kernel-order float32 e32={e:.3f} bound={n[k] + 2} zeros={nz}")
        assert nz == zeros[k]
    e32, nz = R.measure(r32['g_attr'][0], G, GS)
    assert nz == zeros['g_attr'] and nz >= 2 * A * inp['attr'].shape[0]
    gen = torch.Generator().manual_seed(5)
    perm = torch.randperm(int(ref['covered'].sum()), generator=gen)
    for how, order in (('permuted', perm), ('wave64', 'wave64')):
        x = R.reference(inp, torch.float32, order=order)['g_attr'][0]
        e, _ = R.measure(x, G, GS)
        print(f"INTERP {name} g_attr {how} float32 e={e:.3f} e32={e32:.3f} bound={8 * e32 + 4:.1f} zeros={nz}")
        assert e <= 8 * e32 + 4, (name, how, e, e32)


def test_every_kernel_is_reached_by_three_cases_with_and_without_a_hint():
    """dispatch() on the cases (aligned pointers but for the + 8 B twins, whose attr fails the alignment test alone)."""
    reached = {k: [] for k in R.KERNELS}
    for case in R.CASES:
        nd = len(R.diff_indices(case['diff'], case['A']))
        fwd, bwd = R.dispatch(case['A'], nd, case['img'][2], case['attr_grad'], (8,) if case['misalign'] else ())
        reached[fwd].append(case)
        reached[bwd].append(case)
        if case['misalign']:
            assert R.dispatch(case['A'], nd, case['img'][2], case['attr_grad']) != (fwd, bwd)
            assert fwd == 'k_interp_fwd<2>' and bwd in ('k_interp_bwd_rows', 'k_interp_bwd<true>')
    for k, cs in reached.items():
        print(f"INTERP {k}: {len(cs)} cases")
        assert len(cs) >= 3 and any(c['hint'] for c in cs) and any(not c['hint'] for c in cs), k
    assert 30 <= len(R.CASES) <= 40
    assert {c['img'] for c in R.CASES} == {R.S_BIN, R.S_BIN2, R.S_STREAM, R.S_HINT}
    assert {c['A'] for c in R.CASES} == {1, 2, 3, 5, 32, 33}
    assert R.dispatch(2, 0, 40, False, (0, 0, 8))[1] == 'k_interp_bwd_rows' and R.dispatch(2, 0, 40, False, (0, 8, 0)) == ('k_interp_fwd<2>', 'k_interp_bwd_bin2')


# ---------------------------------------------------------------------------------------------------------------------
# mutants: wrong float32 restatements must miss a check on at least one GPU case
# ---------------------------------------------------------------------------------------------------------------------

def _l2(case_got, r32):
    return max(R.rel_l2(x, r32[k][0]) for k, x in case_got.items() if float(r32[k][0].abs().max()) > 0)


def _report(mutant, name, hit, got, r32):
    print(f"INTERP mutant {mutant} on {name}: rel-L2 {_l2(got, r32):.2e}: {hit[:4]}")


@pytest.mark.parametrize("mutant,names", [
    ('no_batch_offset', ['gen/A2/all/BaB/attr', 'bin/A2/one/BaB']),
    ('sorted_diff', ['gen/A3/[2,0]/attr']),
    ('repeat_counts_once', ['gen/A3/[2,0,2]/BaB/attr']),
    ('accepts_T_plus_1', ['bin/A2/confetti']),
    ('vertex2_lacks_ge1', ['gen/A5/all/one/attr']),
])
def test_mutants_of_the_formula_are_caught(mutant, names, monkeypatch):
    """The attr batch offset ignored under Ba = B; diff_idx taken in sorted order; a repeated diff_idx counted once in g_attr; an id of
    T + 1 accepted as triangle T - 1; vertex 2's gradient without - ge1."""
    caught = []
    for name in names:
        case, inp, ref, r32 = _four(name)
        monkeypatch.setattr(R, 'MUTANT', mutant)
        got = _values(R.reference(inp, torch.float32))
        monkeypatch.setattr(R, 'MUTANT', None)
        hit = _failures(case, inp, ref, r32, got)
        _report(mutant, name, hit, got, r32)
        caught += hit
        assert not _failures(case, inp, ref, r32, _values(r32))      # (the unmutated one passes)
    assert caught, mutant


@pytest.mark.parametrize("name", ['bin/A2/confetti', 'stream/A3/[2,0,2]/BaB'])
def test_mutant_last_rows_not_written_is_caught(name):
    """The last H % 8 rows of the four non-atomic outputs keep what the buffer held (here: zeros)."""
    case, inp, ref, r32 = _four(name)
    H = case['img'][1]
    assert H % 8
    got = {k: x.clone() for k, x in R.kernel_order(inp).items()}
    for x in got.values():
        x[:, H - H % 8:] = 0.0
    hit = _failures(case, inp, ref, r32, got, exact=False)
    _report('rows_unwritten', name, hit, got, r32)
    assert {h[0] for h in hit} == set(got)


@pytest.mark.parametrize("name", [c['name'] for c in R.CASES if c['hint']])
def test_mutant_hint_indexed_with_floor_bins_per_row_is_caught(name):
    """fpcdr_hint_on with W // 32 bins in a row of the map instead of ceil(W / 32): bin (1, 0) reads the byte of bin (0, 3)."""
    case, inp, ref, r32 = _four(name)
    W = case['img'][2]
    bad_rast = R.with_hint(inp['rast'], inp['hint'], W // 32)
    assert not torch.equal(bad_rast, inp['rast'])
    got = _values(R.reference(inp, torch.float32, rast=bad_rast))
    hit = _failures(case, inp, ref, r32, got, exact=False)
    _report('hint_floor_bins', name, hit, got, r32)
    assert {h[0] for h in hit} == set(got)


def test_mutant_w_as_one_minus_the_sum_breaks_bit_identity_not_the_bound(monkeypatch):
    """w = 1 - (u + v) instead of (1 - u) - v: another rounding of the same quantity.  It cannot exceed n + 2 (the count holds for
    any order of a sum) and does not; what catches it is the bit-identity with float32_in_kernel_order, on every case."""
    for name in ('bin/A2/confetti', 'gen/A5/all/one/attr', 'stream/A1/all/attr'):
        case, inp, ref, r32 = _four(name)
        k32 = R.kernel_order(inp)
        monkeypatch.setattr(R, 'MUTANT', 'w_as_1_minus_sum')
        got = R.kernel_order(inp)
        monkeypatch.setattr(R, 'MUTANT', None)
        differ = int((got['out'] != k32['out']).any(-1).sum())
        hit = _failures(case, inp, ref, r32, got)
        e = R.measure(got['out'], *ref['out'])[0]
        print(f"INTERP mutant w_as_1_minus_sum on {name}: rel-L2 {R.rel_l2(got['out'], k32['out']):.2e}: {differ} pixels differ in a bit, "
              f"e={e:.3f} bound={R.N_OUT + 2}: {hit}")
        assert differ > 50 and not hit
        assert all(torch.equal(got[k], k32[k]) for k in got if k != 'out')


@pytest.mark.parametrize("name", ['bin/A2/runs/attr', 'gen/A32/all/attr', 'stream/A2/attr', 'hint/gen/A3/[2,0,2]/attr'])
def test_mutant_one_pixels_contribution_to_g_attr_dropped_is_caught(name):
    case, inp, ref, r32 = _four(name)
    cov = ref['covered'] & (inp['go'] != 0).all(-1) & (inp['rast'][..., 0].abs() > 0.25) & (inp['rast'][..., 1].abs() > 0.25)
    b, y, x = cov.nonzero()[len(cov.nonzero()) // 2].tolist()
    less = dict(inp, go=inp['go'].clone(), go_da=inp['go_da'].clone() if inp['go_da'] is not None else None)
    less['go'][b, y, x] = 0.0
    if less['go_da'] is not None:
        less['go_da'][b, y, x] = 0.0
    got = {'g_attr': R.reference(less, torch.float32)['g_attr'][0]}
    hit = [h for h in _failures(case, inp, ref, r32, got) if h[1] != 'zero count']
    _report('dropped_pixel', name, hit, got, r32)
    assert hit

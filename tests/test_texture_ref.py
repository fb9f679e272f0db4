"""CPU: the float64 yardstick of the texture operator (tests/texture_ref.py) is right, and what tests/test_gpu_texture.py asks of
the kernels is reachable and discriminates:
  1. the reference's values and hand-written gradients equal torch.autograd through oracle.ops.texture evaluated in float64 to
     1e-12 of the entry's scale, in every mode and boundary (the first float64 check the oracle's texture gets), on random inputs and
     on the inputs of every GPU case;
  2. on the inputs of every GPU case no pixel lies inside a margin of a discontinuity, the fast-path cases reach the branch of
     k_tex_bwd_bin1 they are named for, the entries without a term are as many as predicted, and float32 (oracle.ops.texture and
     texture_ref with dtype=float32) meets the bounds: n + 2 on the short paths, below 8 u on the long sums;
  3. seven wrong float32 restatements each exceed a bound on at least one GPU case; an eighth, the clamp mask omitted, is shown to
     be equivalent for finite texels (both taps of a clamped axis read one texel), so no bound can catch it.
Lines "TEXTURE ..." are printed under pytest -s."""
import pytest
import torch

import texture_ref as R


def _oracle(case, inp, dtype, with_go=True):
    """oracle.ops.texture and torch.autograd on the inputs of a case, in dtype -> name -> tensor (names of texture_ref.texture)."""
    from oracle import ops
    leaf = lambda t: t.detach().to(dtype).requires_grad_(True) if t is not None else None
    tex, uv, da, bias = leaf(inp['tex']), leaf(inp['uv']), leaf(inp['uv_da']), leaf(inp['bias'])
    mips = [leaf(m) for m in inp['mips']] if inp['mips'] is not None else None
    kw = dict(filter_mode=case['mode'], boundary_mode=case['bd'])
    if 'mipmap' in case['mode']:
        kw.update(uv_da=da, mip_level_bias=bias, mip=mips, max_mip_level=case['mml'])
    out = ops.texture(tex, uv, **kw)
    res = {'out': out.detach()}
    if with_go and not case['fwd_only']:
        out.backward(inp['go'].to(dtype))
        z = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
        res.update(g_tex=z(tex), g_uv=z(uv))
        if da is not None:
            res['g_uv_da'] = z(da)
        if bias is not None:
            res['g_bias'] = z(bias)
        for l, m in enumerate((mips or [])[:case['mml']] if case['mml'] else (mips or [])):
            res[f'g_mip{l + 1}'] = z(m)
    return res


def _outputs(ref):
    return [k for k, v in ref.items() if isinstance(v, tuple)]


def _assert_equal_to_autograd(case, inp):
    ref = R.reference(case, inp)
    got = _oracle(case, inp, torch.float64)
    assert set(_outputs(ref)) == set(got), (case['name'], set(_outputs(ref)) ^ set(got))
    for k in got:
        r, S = ref[k]
        assert bool((S[r != 0] > 0).all()), (case['name'], k)
        worst = float(((r - got[k]).abs() / S.clamp(min=1e-300)).max())
        assert worst <= 1e-12, (case['name'], k, worst)


@pytest.mark.parametrize("mode", ['nearest', 'linear', 'linear-mipmap-nearest', 'linear-mipmap-linear'])
@pytest.mark.parametrize("bd", ['wrap', 'clamp', 'zero'])
def test_reference_equals_autograd_through_the_oracle_on_random_inputs(mode, bd):
    """Unconstrained uv in [-1, 2) and footprints (a float64 reference and float64 autograd take the same side of every
    discontinuity): Bt in {1, B}, C in {1, 3}, uv_da / bias / both, the built chain with and without max_mip_level, a custom
    stack with and without it."""
    g = torch.Generator().manual_seed(0)
    B, H, W = 2, 7, 9
    mip = 'mipmap' in mode
    for Bt, C in ((1, 1), (2, 3)):
        for da, bias in (((True, False), (False, True), (True, True)) if mip else ((False, False),)):
            for kind, mml in ((('built', None), ('built', 2), ('custom', None), ('custom', 1)) if mip else (('built', None),)):
                case = R._case(f'{mode}/{bd}', '', img=(B, H, W), tex=(Bt, 8, 16, C), mode=mode, bd=bd, mip=kind, mml=mml)
                inp = dict(tex=torch.rand(Bt, 8, 16, C, generator=g) + 0.1, uv=torch.rand(B, H, W, 2, generator=g) * 3 - 1,
                           uv_da=(torch.rand(B, H, W, 4, generator=g) - 0.5) * 0.6 if da else None,
                           bias=torch.rand(B, H, W, generator=g) * 4 - 1 if bias else None, go=torch.randn(B, H, W, C, generator=g),
                           mips=[torch.rand(Bt, 4, 8, C, generator=g), torch.rand(Bt, 2, 4, C, generator=g)] if kind == 'custom' else None)
                _assert_equal_to_autograd(case, inp)


def test_box_chain_equals_autograd_and_stops_at_an_odd_side():
    from oracle import ops
    g = torch.Generator().manual_seed(1)
    for shape in ((2, 6, 10, 3), (1, 2, 2, 1)):
        src, go = torch.randn(shape, generator=g), torch.randn(shape[0], shape[1] // 2, shape[2] // 2, shape[3], generator=g)
        ref = R.mip_down(src, go)
        leaf = src.double().requires_grad_(True)
        lvl = ops.build_mip_chain(leaf, 1)[1]
        lvl.backward(go.double())
        assert torch.allclose(ref['out'][0], lvl.detach(), rtol=1e-14, atol=0) and torch.allclose(ref['g_src'][0], leaf.grad, rtol=1e-14, atol=0)
    assert R.num_levels(32, 64) == 5 and R.num_levels(32, 64, 4) == 4 and R.num_levels(8, 32) == 3 and R.num_levels(6, 10) == 1
    assert [t.shape[1:3] for t in ops.build_mip_chain(torch.zeros(1, 8, 32, 1))] == [t.shape[1:3] for t in R.box_chain(torch.zeros(1, 8, 32, 1), 3)[0]]


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_gpu_case_inputs_and_float32(name):
    """On the inputs of a GPU case: the reference equals float64 autograd; no pixel inside a margin; the branch the case is named
    for; the predicted entries without a term; float32 within the bounds."""
    case = R.CASES[R.CASE_IDS.index(name)]
    inp = R.case_inputs(case)
    m = R.margins(case, inp)
    assert m == dict(coord=0, level=0, rt=0), (name, m)
    _assert_equal_to_autograd(case, inp)
    Bt, Ht, Wt, C = case['tex']
    B, H, W = case['img']
    if name.startswith('fast/'):
        assert R.takes_fast_path(case['mode'], case['bd'], C, Bt, W, ())
        if not case['fwd_only']:
            R.check_plan(case, R.window_plan(inp['uv'], inp['go'], Ht, Wt, case['bd']))
    elif not case['misalign']:
        assert not R.takes_fast_path(case['mode'], case['bd'], C, Bt, W, ())
    # the deliberately exact pixels are there
    q = inp['uv'].reshape(-1, 2)
    assert int(((q[:, 0] == 0) & (q[:, 1] == 0)).sum()) >= 3
    if case['uv'][0] != 'affine':
        assert int((q == 0).sum()) >= 8 and int((q == 1).sum()) >= 8
    if case['bd'] == 'clamp' and ('seam' in name or (case['uv'][0] == 'iid' and case['uv'][1] < 0)):
        assert int(((q < 0) | (q > 1)).sum()) > 50
    if inp['uv_da'] is not None:
        assert int((inp['uv_da'].reshape(-1, 4) == 0).all(1).sum()) > 20
    if case['bd'] == 'zero':      # inside, the four sides (two taps), all of the padding and, on the small texture, the four corners (one tap)
        corners = set() if 'mipmap' in case['mode'] else {0b1000, 0b0100, 0b0010, 0b0001}
        assert R.tap_patterns(case, inp) >= {0b1111, 0b1010, 0b0101, 0b1100, 0b0011, 0} | corners, name
    ref = R.reference(case, inp)
    if 'l0' in ref:      # every level is sampled; some pixels lie below 0 and some above the top
        assert int(torch.bincount(ref['l0'], minlength=ref['n_levels'] + 1).min()) > 50
        assert int((ref['raw'] < -0.125).sum()) > 50 and int((ref['raw'] > ref['n_levels'] + 0.125).sum()) > 50
    zeros = R.predicted_zeros(inp['uv'], inp['uv_da'], inp['bias'], None if case['fwd_only'] else inp['go'], case['mode'], case['bd'], ref)
    bounds = R.bounds(case, ref)
    for who, got in (('oracle32', _oracle(case, inp, torch.float32)), ('ref32', {k: v[0] for k, v in R.reference(case, inp, torch.float32).items() if isinstance(v, tuple)})):
        for k in _outputs(ref):
            e, nz = R.measure(got[k], *ref[k])
            n = bounds.get(k)
            print(f"TEXTURE {name} {k} {who} e32={e:.3f} bound={'8.0 (long sum)' if n is None else n + 2} zeros={nz}")
            assert nz == zeros.get(k, 0), (name, k, who, nz, zeros.get(k, 0))
            assert (e < 8) if n is None else (e <= n + 2), (name, k, who, e)


def test_coordinate_aware_scale_is_the_right_one():
    """float32 (oracle.ops.texture) against float64 on (2, 37, 40), 'wrap', uv in [-2, 3), four draws each of a 32 x 64 and a 30 x 60
    texture, uv with full float32 mantissas (drawn in float64, then rounded): against sum_k |w_k| |t_k| the error is far above the 8 u a six-operation path may have (the rounding of
    x = prep(u) * Wt - 0.5 dominates: at a power-of-two size it comes from u - floor(u) alone, at any other size from the product
    as well); against the coordinate-aware scale it is below 1 u."""
    from oracle import ops
    for shape in ((32, 64), (30, 60)):
        e_plain, e_aware = 0.0, 0.0
        for seed in range(4):
            g = torch.Generator().manual_seed(seed)
            tex, uv = torch.rand(1, *shape, 1, generator=g), (torch.rand(2, 37, 40, 2, generator=g, dtype=torch.float64) * 5 - 2).float()
            r, S = R.texture(tex, uv)['out']
            o32 = ops.texture(tex, uv, filter_mode='linear', boundary_mode='wrap')
            e_plain = max(e_plain, R.measure(o32, r, R.plain_scale_out(tex, uv))[0])
            e_aware = max(e_aware, R.measure(o32, r, S)[0])
        print(f"TEXTURE scale {shape}: float32 against the plain scale {e_plain:.1f} u, against the coordinate-aware scale {e_aware:.2f} u")
        assert e_plain > 3 * (R.N_OUT_LINEAR + 2) and e_aware <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# mutants: wrong float32 restatements must exceed a bound on at least one GPU case
# ---------------------------------------------------------------------------------------------------------------------

def _exceeds(case, ref, r32, got):
    """The outputs of `got` that miss the bound test_gpu_texture.py sets (n + 2, or 8 * e32 + 4 with e32 from the unmutated r32)."""
    bounds = R.bounds(case, ref)
    bad = []
    for k in got:
        r, S = ref[k]
        x = got[k]
        if not bool((x[S == 0] == 0).all()):
            bad.append((k, 'a term where there is none'))
            continue
        e = R.measure(x, r, S)[0]
        n = bounds.get(k)
        limit = n + 2 if n is not None else 8 * R.measure(r32[k][0], r, S)[0] + 4
        if not e <= limit:
            bad.append((k, round(e, 1), round(limit, 1)))
    return bad


def _three(name):
    case = R.CASES[R.CASE_IDS.index(name)]
    inp = R.case_inputs(case)
    return case, inp, R.reference(case, inp), R.reference(case, inp, torch.float32)


@pytest.mark.parametrize("mutant,names", [
    ('swap_fx_fy', ['fast/affine64/wrap']),
    ('no_seam_wrap', ['fast/seam32/wrap']),
    ('level1_scale', ['mip/linear/wrap/mml4']),
    ('zero_tap_scatters', ['generic/zeroC1']),
])
def test_mutants_of_the_formula_are_caught(mutant, names, monkeypatch):
    """fx and fy swapped; x0 + 1 not wrapped at the seam; level-1 g_uv scaled by Wt instead of Wt >> 1; a 'zero'-padding tap that
    scatters."""
    caught = []
    for name in names:
        case, inp, ref, r32 = _three(name)
        monkeypatch.setattr(R, 'MUTANT', mutant)
        bad = R.reference(case, inp, torch.float32)
        monkeypatch.setattr(R, 'MUTANT', None)
        hit = _exceeds(case, ref, r32, {k: v[0] for k, v in bad.items() if isinstance(v, tuple)})
        print(f"TEXTURE mutant {mutant} on {name}: {hit}")
        caught += hit
    assert caught, mutant
    assert not _exceeds(case, ref, r32, {k: v[0] for k, v in r32.items() if isinstance(v, tuple)})      # (the unmutated one passes)


@pytest.mark.parametrize("name", ['fast/seam32/clamp', 'fast/wide/clamp', 'generic/C3', 'mip/linear/clamp/mml4', 'mip/custom'])
def test_mutant_without_the_clamp_mask_is_equivalent_for_finite_texels(name, monkeypatch):
    """The clamp mask omitted CANNOT exceed a bound, and this test says why instead of pretending: a coordinate outside [0, 1] is
    prepared to exactly 0 or 1, so x0 + 1 (or x0) is clamped onto its neighbour, both taps of the axis read the same texel and
    d out / d fx is t - t = 0 whatever the mask says.  The mask decides the result only for a texel that is Inf or NaN.  So the
    unmasked restatement gives the SAME g_uv, entry by entry, on every clamp case with coordinates outside; what the GPU test pins
    is that those entries, whose scale is 0, are exactly 0."""
    case, inp, ref, r32 = _three(name)
    q = inp['uv']
    assert int(((q < 0) | (q > 1)).sum()) > 50
    monkeypatch.setattr(R, 'MUTANT', 'no_clamp_mask')
    bad = R.reference(case, inp, torch.float32)
    monkeypatch.setattr(R, 'MUTANT', None)
    assert torch.equal(bad['g_uv'][0], r32['g_uv'][0])
    assert int((bad['g_uv'][1] != r32['g_uv'][1]).sum()) > 50          # (the hook is live: the scales differ)


def test_mutant_one_tap_dropped_at_one_pixel_is_caught():
    case, inp, ref, r32 = _three('fast/affine64/wrap')
    out = r32['out'][0].clone()
    b, py, px = 1, 20, 17
    Ht, Wt = case['tex'][1], case['tex'][2]
    u, v = (float(t) for t in inp['uv'][b, py, px])
    x, y = (u - int(u // 1)) * Wt - 0.5, (v - int(v // 1)) * Ht - 0.5
    x0, y0 = int(x // 1), int(y // 1)
    drop = (x - x0) * (y - y0) * float(inp['tex'][0, (y0 + 1) % Ht, (x0 + 1) % Wt, 0])      # tap 11
    assert drop > 1e-3
    out[b, py, px, 0] -= drop
    hit = _exceeds(case, ref, r32, {'out': out})
    print(f"TEXTURE mutant dropped_tap: {hit}")
    assert hit


def test_mutant_a_window_shifted_by_one_column_is_caught():
    """The texel gradient of one bin's footprint lands one column to the right."""
    case, inp, ref, r32 = _three('fast/affine64/wrap')
    g = r32['g_tex'][0].clone()
    g[0, 3:40, 5:38] = r32['g_tex'][0][0, 3:40, 4:37]
    hit = _exceeds(case, ref, r32, {'g_tex': g})
    print(f"TEXTURE mutant shifted_window: {hit}")
    assert hit


def test_mutant_the_origin_pixels_share_added_twice_is_caught():
    case, inp, ref, r32 = _three('fast/origin_mixed/wrap')
    origin = (inp['uv'] == 0).all(-1, keepdim=True)
    only = dict(inp, go=inp['go'] * origin)
    twice = r32['g_tex'][0] + R.reference(case, only, torch.float32)['g_tex'][0]
    hit = _exceeds(case, ref, r32, {'g_tex': twice})
    print(f"TEXTURE mutant origin_twice: {hit}")
    assert hit

"""GPU: the texture operator (csrc/texture.hip, csrc/texsample.h) entry by entry against float64 (tests/texture_ref.py), through
fpc_diffrend_amd.ops.texture.

Every output x is compared with float64 arithmetic on the float32 inputs the kernel read: e = max_i |x_i - r_i| / S_i in units of
u = 2^-24, S_i the coordinate-aware scale of entry i (texture_ref.py); entries with S_i = 0 have no term, must be exactly 0, and
their number must be the one the construction predicts (untouched texels, pixels without a gradient, 'zero' padding, masked
components under 'clamp', levels outside [0, n_levels], 'nearest' g_uv).
  short paths (out, g_uv, g_bias): e <= n + 2, n derived in texture_ref.py (bounds());
  long sums (g_tex and the levels of a custom stack: sums over all pixels that touch a texel, finished by atomics; g_uv_da: its
              chain of quotients through the computed l2 and rt has no practical derived count): e <= 8 * e32 + 4, e32 the error of
              float32 torch on the CPU (texture_ref.texture, dtype=float32) against the same reference.
No pixel is masked: the inputs keep every tap coordinate and every level away from its discontinuities, which
tests/test_texture_ref.py asserts on the CPU for each case, together with the branch of k_tex_bwd_bin1 a fast-path case reaches.
Every line below is printed by a test as "TEXTURE case output e_gpu e32 bound" (pytest -s); fast-path cases also print what
k_tex_bwd_bin1 does with each bin.

Measured on an MI355X (units of u; the largest over the cases of a row; e32 "-": the bound is n + 2, derived, no yardstick is
measured; the last column is the case of the row that came closest to its own bound).  g_tex and the levels' gradients are
finished by atomics and move by a few hundredths of u from run to run.  g_mip1..n are the levels of the two custom stacks.  The
whole file, 74 cases of the operator and 2 of the box filter, runs in 5 s there:

  path     output     cases max e_gpu  max e32   closest to its bound (e_gpu / bound, case)
  fast     out           35      0.21        -   0.21 / 8.0  fast/1x8/wrap
  fast     g_tex         32      0.33     0.67   0.33 / 6.7  fast/wide/wrap
  fast     g_uv          32      0.66        -   0.66 / 8.0  fast/4096x2/wrap
  generic  out           18      0.64        -   0.64 / 8.0  generic/zeroC3
  generic  g_tex         17      1.85     2.14   1.59 / 16.4  generic/nearest/zero
  generic  g_uv          17      0.85        -   0.85 / 8.0  generic/zeroC1
  mip      out           21      1.09        -   0.90 / 20.0  mip/nearest/zero/mml4
  mip      g_tex         20      0.44     0.42   0.44 / 5.8  mip/nearest/clamp/mml4
  mip      g_uv          20      1.42        -   1.42 / 26.0  mip/linear/zero/all
  mip      g_uv_da       19      0.19     0.19   0.19 / 5.5  mip/linear/zero/all
  mip      g_bias        19      0.82        -   0.82 / 25.0  mip/linear/zero/all
  mip      g_mip1..n      6      0.52     0.40   0.52 / 5.4  mip/custom
  mip_down out            2      1.96        -   1.96 / 5.0  mip_down(2, 6, 10, 3)
  mip_down g_src          2      0.00        -   0.00 / 2.0  mip_down(2, 6, 10, 3)
"""
import ctypes

import pytest
import torch

import texture_ref as R

pytestmark = pytest.mark.gpu


def _report(case, name, e, e32, bound):
    print(f"TEXTURE {case} {name} e_gpu={e:.3f} e32={'-' if e32 is None else format(e32, '.3f')} bound={bound:.1f}")


def short(case, name, x, ref, n, zeros):
    r, S = ref
    e, nz = R.measure(x, r, S)
    _report(case, name, e, None, n + 2)
    assert nz == zeros, (case, name, nz, zeros)
    assert e <= n + 2, (case, name, e)


def long_sum(case, name, x, ref, x32, zeros):
    r, S = ref
    e, nz = R.measure(x, r, S)
    e32, _ = R.measure(x32, r, S)
    _report(case, name, e, e32, 8 * e32 + 4)
    assert nz == zeros, (case, name, nz, zeros)
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offset_view(t, n_floats):
    """A contiguous copy of t that starts n_floats floats into a larger buffer."""
    buf = torch.zeros(t.numel() + n_floats + 4, dtype=t.dtype, device='cuda')
    v = buf[n_floats:n_floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_texture_entries_against_float64(name):
    from fpc_diffrend_amd import ops
    case = R.CASES[R.CASE_IDS.index(name)]
    inp = R.case_inputs(case)
    ref, ref32 = R.reference(case, inp), R.reference(case, inp, torch.float32)
    Bt, Ht, Wt, C = case['tex']
    B, H, W = case['img']
    mip = 'mipmap' in case['mode']
    need = set(case['need'])
    if mip and need == {'tex', 'uv'}:
        need |= {'da', 'bias', 'mips'}
    dev = lambda t, flag: t.cuda().requires_grad_(flag) if t is not None else None
    tex = dev(inp['tex'], 'tex' in need)
    uv = (_offset_view(inp['uv'], 2) if case['misalign'] else inp['uv'].cuda()).requires_grad_('uv' in need and not case['fwd_only'])
    da, bias = dev(inp['uv_da'], 'da' in need), dev(inp['bias'], 'bias' in need)
    mips = [dev(m, 'mips' in need) for m in inp['mips']] if inp['mips'] is not None else None
    go = inp['go'].cuda()
    assert uv.is_contiguous() and uv.data_ptr() % 16 == (8 if case['misalign'] else 0) and go.data_ptr() % 16 == 0
    # the dispatch condition of fpcdr_texture_bwd: the fast cases satisfy it, the generic twins fail it on the pointer alone
    fast = R.takes_fast_path(case['mode'], case['bd'], C, Bt, W, (uv.data_ptr(), go.data_ptr()))
    assert fast == name.startswith('fast/'), name
    if case['misalign']:
        assert R.takes_fast_path(case['mode'], case['bd'], C, Bt, W, (go.data_ptr(),))
    if fast and not case['fwd_only']:
        plan = R.window_plan(inp['uv'], inp['go'], Ht, Wt, case['bd'])
        R.check_plan(case, plan)
        print(f"TEXTURE {name} bins " + ' '.join(f"{e['kind']}:{e['stride']}x{e['rows']}:in{e['inside']}/out{e['outside']}/origin{e['origin']}" for e in plan))
    kw = dict(filter_mode=case['mode'], boundary_mode=case['bd'])
    if mip:
        stack = ops.texture_construct_mip(tex, max_mip_level=case['mml']) if case['mip'] == 'construct' else mips
        if case['mip'] == 'construct':
            assert len(stack) == ref['n_levels']
        kw.update(uv_da=da, mip_level_bias=bias, mip=stack, max_mip_level=case['mml'])
    zeros = R.predicted_zeros(inp['uv'], inp['uv_da'], inp['bias'], None if case['fwd_only'] else inp['go'], case['mode'], case['bd'], ref)
    n = R.bounds(case, ref)
    if case['fwd_only']:
        with torch.no_grad():
            out = ops.texture(tex, uv, **kw)
        short(name, 'out', out, ref['out'], n['out'], zeros['out'])
        return
    out = ops.texture(tex, uv, **kw)
    out.backward(go)
    short(name, 'out', out, ref['out'], n['out'], zeros['out'])
    got = {'g_tex': tex.grad, 'g_uv': uv.grad, 'g_uv_da': da.grad if da is not None else None, 'g_bias': bias.grad if bias is not None else None}
    for l, m in enumerate(mips or []):
        got[f'g_mip{l + 1}'] = m.grad
    wanted = {'g_tex': 'tex' in need, 'g_uv': 'uv' in need, 'g_uv_da': 'da' in need and da is not None, 'g_bias': 'bias' in need and bias is not None}
    for k, x in got.items():
        if k.startswith('g_mip'):
            if int(k[5:]) > ref['n_levels']:          # a level max_mip_level cuts off is never sampled
                assert x is None or not bool(x.any()), (name, k)
                continue
            wanted[k] = 'mips' in need
        if not wanted[k]:
            assert x is None, (name, k)
            continue
        assert x is not None and x.shape == ref[k][0].shape, (name, k)
        if fast and k == 'g_uv':
            assert x.data_ptr() % 16 == 0
        if k in n:
            short(name, k, x, ref[k], n[k], zeros.get(k, 0))
        else:
            long_sum(name, k, x, ref[k], ref32[k][0], zeros.get(k, 0))


@pytest.mark.parametrize("shape", [(2, 6, 10, 3), (1, 2, 2, 1)])
def test_mip_downsample_and_its_backward_on_their_own(shape):
    """fpcdr_mip_downsample: three adds and an exact quarter; fpcdr_mip_downsample_bwd into a zeroed gradient: exact."""
    from fpc_diffrend_amd import _lib
    g = torch.Generator().manual_seed(11)
    N, h, w, C = shape
    src, go = torch.randn(shape, generator=g), torch.randn(N, h // 2, w // 2, C, generator=g)
    ref = R.mip_down(src, go)
    s, gd = src.cuda(), go.cuda()
    dst, gs = torch.empty_like(gd), torch.zeros_like(s)
    _lib.call("fpcdr_mip_downsample", _ptr(s), _ptr(dst), N, h, w, C, _stream())
    _lib.call("fpcdr_mip_downsample_bwd", _ptr(gd), _ptr(gs), N, h, w, C, _stream())
    short(f"mip_down{shape}", 'out', dst, ref['out'], R.N_MIP_DOWN, 0)
    short(f"mip_down{shape}", 'g_src', gs, ref['g_src'], R.N_MIP_DOWN_BWD, 0)
    _lib.call("fpcdr_mip_downsample_bwd", _ptr(gd), _ptr(gs), N, h, w, C, _stream())        # it ADDS: a second call doubles, exactly
    assert torch.equal(gs.cpu().double(), 2 * ref['g_src'][0].float().double())

"""GPU: the slab form of the blend's weight gradient (csrc/blend.hip: k_blend_bwd_w_slab + k_blend_bwd_w_sum behind fpcdr_blend_bwd_w_ws)
and its fallback, against a float64 einsum.

  grad_w[f][k] += sum_i grad_out[f][i] Bmat[i][k]

Shapes: M in {111, 513, 1539} (not a multiple of 32; two, nine and twenty-five slabs of 64 rows, the last one partial), K in {7, 150, 224, 225}
(one, five and seven column tiles; 224 takes the 32-row chunks; 225 is past LDS_KMAX and must come out of the atomics kernel), F in {1, 5, 32,
33} (33: a second frame tile), all 48 combinations; and (16449, 150, 5): slabs of 128 rows, two chunks each, the last slab one full chunk and
one row.

The error of an entry x with float64 value r is |x - r| / S in units of u = 2^-24, S the sum of the absolute values of the entry's terms, so
that cases of different sizes compare.  The bar is not a number chosen here: E_old is the largest error of the ATOMICS kernel (the entry
fpcdr_blend_bwd_w, unchanged) over all the cases, on the same inputs, and every case of the new entry must stay within 1.5 E_old -- the margin
for a different but fixed order of summation.  (One figure for the kernel, not one per case: a case with K = 7, F = 1 has seven entries, and
the ratio of two maxima over seven entries says nothing about either kernel.)  Every case prints "BLEND_STREAMS case e_new e_old".

The new entry adds into grad_w (checked on a grad_w that holds values on entry), gives the same bits on every call, and is the old entry
when there is no workspace or a pointer is not 16-byte aligned.

The forward (fpcdr_blend_fwd: k_blend_fwd_lds and its fallback, the register kernel k_blend_fwd) is held at the same shapes in the
same way, with and without v_base; its yardstick is the register kernel ("BLEND_STREAMS fwd...").

Measured on an MI355X (units of u): bwd_w E_old = 4.02, largest e_new 4.02 (the K = 225 cases, which ARE the old kernel; the slab
form's error is below the old kernel's in 36 of its 37 cases); fwd E_reg = 4.92, largest e of the entry 4.81.  The file runs in 4 s.
"""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = list(itertools.product((111, 513, 1539), (7, 150, 224, 225), (1, 5, 32, 33))) + [(16449, 150, 5)]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(M, K, F, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 131 * K + F)
    Bm = torch.randn(M, K, generator=g, dtype=torch.float32)
    go = torch.randn(F, M, generator=g, dtype=torch.float32) * torch.rand(F, 1, generator=g)
    return Bm, go


def _reference(Bm, go):
    """float64 value and scale S of every entry of grad_w."""
    B64, g64 = Bm.double(), go.double()
    return torch.einsum('fi,ik->fk', g64, B64), torch.einsum('fi,ik->fk', g64.abs(), B64.abs())


def _err(x, r, S):
    return float(((x.detach().cpu().double() - r).abs() / S).max()) / U


def _workspace(lib, M, K, F):
    n = lib.fpcdr_blend_bwd_w_workspace_bytes(M, K, F)
    assert n % 4 == 0 and n > 0
    # NaN: the kernels must write every word of the workspace that they read
    return torch.full((n // 4,), float('nan'), dtype=torch.float32, device='cuda')


def _old(Bg, gg, init=None):
    from fpc_diffrend_amd import _lib
    (M, K), F = Bg.shape, gg.shape[0]
    gw = torch.zeros(F, K, dtype=torch.float32, device='cuda') if init is None else init.clone()
    _lib.call("fpcdr_blend_bwd_w", _ptr(Bg), _ptr(gg), _ptr(gw), M, K, F, _stream())
    return gw


def _new(Bg, gg, init=None, ws=False):
    from fpc_diffrend_amd import _lib
    lib = _lib.load()
    (M, K), F = Bg.shape, gg.shape[0]
    gw = torch.zeros(F, K, dtype=torch.float32, device='cuda') if init is None else init.clone()
    if ws is False:
        ws = _workspace(lib, M, K, F)
    _lib.call("fpcdr_blend_bwd_w_ws", _ptr(Bg), _ptr(gg), _ptr(gw), _ptr(ws), ws.numel() * 4 if ws is not None else 0, M, K, F, _stream())
    return gw


@pytest.fixture(scope="module")
def measured():
    """(M, K, F) -> (e_new, e_old, new == second call of new), computed once for the module; E_old = max of e_old."""
    res = {}
    for M, K, F in SHAPES:
        Bm, go = _inputs(M, K, F)
        r, S = _reference(Bm, go)
        Bg, gg = Bm.cuda(), go.cuda()
        assert Bg.data_ptr() % 16 == 0 and gg.data_ptr() % 16 == 0
        a, b = _new(Bg, gg), _new(Bg, gg)
        res[(M, K, F)] = (_err(a, r, S), _err(_old(Bg, gg), r, S), torch.equal(a, b))
        print(f"BLEND_STREAMS bwd_w({M},{K},{F}) e_new={res[(M, K, F)][0]:.3f} e_old={res[(M, K, F)][1]:.3f}")
    E_old = max(v[1] for v in res.values())
    print(f"BLEND_STREAMS bwd_w E_old={E_old:.3f} max e_new={max(v[0] for v in res.values()):.3f}")
    return res, E_old


@pytest.mark.parametrize("M,K,F", SHAPES)
def test_slab_weight_gradient_within_the_atomics_kernels_error(measured, M, K, F):
    res, E_old = measured
    e_new, _, same = res[(M, K, F)]
    assert e_new <= 1.5 * E_old, (M, K, F, e_new, E_old)
    if K <= 224:      # (past LDS_KMAX the call IS the atomics kernel, whose last bits depend on the order of arrival)
        assert same, "two calls of fpcdr_blend_bwd_w_ws differ"


# ---------------------------------------------------------------------------------------------------------------------
# forward: k_blend_fwd_lds (one wave per tile) and its fallback, the register kernel k_blend_fwd
# ---------------------------------------------------------------------------------------------------------------------

def _fwd_inputs(M, K, F, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 131 * K + F + 17)
    return (torch.randn(M, generator=g, dtype=torch.float32), torch.randn(M, K, generator=g, dtype=torch.float32),
            torch.randn(F, K, generator=g, dtype=torch.float32))


def _fwd_reference(vb, Bm, w):
    r = torch.einsum('fk,ik->fi', w.double(), Bm.double())
    S = torch.einsum('fk,ik->fi', w.double().abs(), Bm.double().abs())
    return (r + vb.double(), S + vb.double().abs()) if vb is not None else (r, S)


def _offset_view(t):
    """A contiguous copy of t one float into a larger buffer: not 16-byte aligned, so the entry takes the register kernel."""
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device='cuda')
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _fwd(vb, Bg, wg):
    from fpc_diffrend_amd import _lib
    (M, K), F = Bg.shape, wg.shape[0]
    out = torch.full((F, M), float('nan'), dtype=torch.float32, device='cuda')
    _lib.call("fpcdr_blend_fwd", _ptr(vb), _ptr(Bg), _ptr(wg), _ptr(out), M, K, F, _stream())
    return out


@pytest.fixture(scope="module")
def measured_fwd():
    """(M, K, F, with v_base) -> (e of the entry on aligned inputs, e of the register kernel on the same values); E_reg = max of the latter.
    At K <= 224 the first is k_blend_fwd_lds; at 225 both are the register kernel."""
    res = {}
    for (M, K, F), has_vb in itertools.product(SHAPES, (True, False)):
        vb, Bm, w = _fwd_inputs(M, K, F)
        vb = vb if has_vb else None
        r, S = _fwd_reference(vb, Bm, w)
        vg = vb.cuda() if has_vb else None
        e = _err(_fwd(vg, Bm.cuda(), w.cuda()), r, S)
        e_reg = _err(_fwd(vg, _offset_view(Bm), _offset_view(w)), r, S)
        res[(M, K, F, has_vb)] = (e, e_reg)
        print(f"BLEND_STREAMS fwd({M},{K},{F},vb={int(has_vb)}) e_new={e:.3f} e_reg={e_reg:.3f}")
    E_reg = max(v[1] for v in res.values())
    print(f"BLEND_STREAMS fwd E_reg={E_reg:.3f} max e_new={max(v[0] for v in res.values()):.3f}")
    return res, E_reg


@pytest.mark.parametrize("has_vb", [True, False])
@pytest.mark.parametrize("M,K,F", SHAPES)
def test_forward_within_the_register_kernels_error(measured_fwd, M, K, F, has_vb):
    """The forward at the same shapes, with and without a base mesh: the yardstick is the register kernel k_blend_fwd, reached through
    views that are not 16-byte aligned (E_reg: its largest error over all the cases); every case of the entry on aligned inputs
    (k_blend_fwd_lds at K <= 224) stays within 1.5 E_reg."""
    res, E_reg = measured_fwd
    e, _ = res[(M, K, F, has_vb)]
    assert 0.0 < E_reg < 16.0
    assert e <= 1.5 * E_reg, (M, K, F, has_vb, e, E_reg)


def test_the_yardstick_is_a_few_units(measured):
    """The yardstick itself is sane: E_old is a few u (tests/test_gpu_fitstep.py records 1.02 u for g_w), not a figure so wide that
    anything passes under it."""
    _, E_old = measured
    assert 0.0 < E_old < 16.0, E_old


@pytest.mark.parametrize("M,K,F", [(111, 7, 1), (1539, 150, 33), (513, 224, 5), (513, 225, 32), (16449, 150, 5)])
def test_slab_weight_gradient_adds_into_grad_w(measured, M, K, F):
    """grad_w holds values on entry: the call adds its sum to them (one more rounded add per entry: + 1 u of the larger scale)."""
    _, E_old = measured
    Bm, go = _inputs(M, K, F, seed=1)
    r, S = _reference(Bm, go)
    init = torch.randn(F, K, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    gw = _new(Bm.cuda(), go.cuda(), init=init.cuda())
    e = _err(gw, r + init.double(), S + init.double().abs())
    print(f"BLEND_STREAMS bwd_w({M},{K},{F})+init e_new={e:.3f}")
    assert e <= 1.5 * E_old + 1.0, (e, E_old)


def test_fallbacks_are_the_atomics_kernel(measured):
    """No workspace, or grad_out one float into a larger buffer: the old kernel's path, same bar."""
    _, E_old = measured
    M, K, F = 1539, 150, 5
    Bm, go = _inputs(M, K, F, seed=2)
    r, S = _reference(Bm, go)
    Bg = Bm.cuda()
    assert _err(_new(Bg, go.cuda(), ws=None), r, S) <= 1.5 * E_old
    buf = torch.zeros(go.numel() + 8, dtype=torch.float32, device='cuda')
    gv = buf[1:1 + go.numel()].view(F, M)
    gv.copy_(go)
    assert gv.data_ptr() % 16 == 4
    assert _err(_new(Bg, gv), r, S) <= 1.5 * E_old


def test_a_short_workspace_is_refused():
    from fpc_diffrend_amd import _lib
    Bm, go = _inputs(111, 7, 1)
    ws = torch.zeros(4, dtype=torch.float32, device='cuda')
    gw = torch.zeros(1, 7, dtype=torch.float32, device='cuda')
    with pytest.raises(RuntimeError, match="workspace too small"):
        _lib.call("fpcdr_blend_bwd_w_ws", _ptr(Bm.cuda()), _ptr(go.cuda()), _ptr(gw), _ptr(ws), 16, 111, 7, 1, _stream())


def test_autograd_takes_the_slab_form_and_is_reproducible():
    """fit.blend_batched's backward: the same bits twice (the atomics kernel differed in the last bits from run to run)."""
    from fpc_diffrend_amd import fit
    Bm, go = _inputs(1539, 150, 32, seed=3)
    w = torch.randn(32, 150, generator=torch.Generator().manual_seed(9), dtype=torch.float32)
    grads = []
    for _ in range(2):
        wg = w.cuda().requires_grad_(True)
        fit.blend_batched(None, Bm.cuda(), wg).backward(go.cuda())
        grads.append(wg.grad.clone())
    assert torch.equal(grads[0], grads[1])
    r, S = _reference(Bm, go)
    assert _err(grads[0], r, S) < 16.0

"""CPU: the float64 restatement of the locally normalised pixel loss (tests/norm_ref.py) checked against torch itself, the exact
invariance the loss exists for, the host side of the feature (argument checks, FitConfig, the C ABI's new entry) and the exposure scan
on the CPU oracle that is the reason for the design -- no GPU.

The closed-form gradient  grad_a = p - G^T P - a (G^T q)  is the statement tests/test_gpu_norm.py judges the kernels by; here it is
compared with torch.autograd through F.pad(reflect) + conv2d in float64 at every shape the GPU file uses, entry by entry: |g_i -
auto_i| <= 1e-10 S_i, S_i the size of the terms of entry i (|p| + G^T |P| + |a| G^T |q|, times the gain) -- a lost fold or a wrong
factor of one entry shows at that entry's own size."""
import ctypes
import dataclasses
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import blur_ref as B  # noqa: E402
import norm_ref as N  # noqa: E402
from helpers import lib_loaded  # noqa: E402

_ids = lambda s: "x".join(str(v) for v in s[:5])


@pytest.fixture
def exact_operands():
    """The statement with a and a*a unrounded (norm_ref.EXACT_OPERANDS): what autograd can be held against to 1e-10."""
    N.EXACT_OPERANDS = True
    yield
    N.EXACT_OPERANDS = False


def _inputs(shape):
    return N.flat_inputs() if shape == N.FLAT_SHAPE else N.inputs(*shape[:4])


@pytest.mark.parametrize("shape", N.ALL_SHAPES + [N.FLAT_SHAPE], ids=_ids)
def test_closed_form_gradient_equals_autograd(shape, exact_operands):
    Bn, H, W, C, k, sigma = shape
    colour, cover, ref = _inputs(shape)
    g = N.taps(k, sigma)
    res = N.loss_and_gradient(colour, cover, ref, g)
    grad, gS = res['grad']
    assert grad.dtype == torch.float64
    cd = colour.double().requires_grad_(True)
    loss = N.loss_plain(cd, cover, ref, g)
    loss.backward()
    # gradient() scales by the float32 product 255 * float32(1 / n_total) the kernel is handed; the plain expression by 255 / n_total
    gain = float(torch.tensor(np.float32(255.0)) * torch.tensor(np.float32(1.0 / colour.numel())))
    auto = cd.grad * (gain / (255.0 / colour.numel()))
    unc = (cover <= 0)[..., None].expand_as(grad)
    assert bool((grad[unc] == 0).all()) and bool((gS[unc] == 0).all()) and bool((auto[unc] == 0).all()) and bool((gS[~unc] > 0).all())
    err = float(((grad - auto).abs()[~unc] / gS[~unc]).max())
    print(f"NORMREF closed-form-vs-autograd {shape} {err:.2e}")
    assert err <= 1e-10
    assert abs(float(res['loss']) - float(loss.detach())) <= 1e-10 * float(loss.detach())
    for name in ('stats', 'd', 'P', 'q', 'p'):
        v, S = res[name]
        assert bool(torch.isfinite(v).all()) and bool((S >= v.abs() * (1 - 1e-12)).all()), name


def test_closed_form_holds_for_asymmetric_taps(exact_operands):
    """taps= may be anything non-negative: neither adjoint may lean on the symmetry of a Gaussian."""
    colour, cover, ref = N.inputs(1, 9, 12, 2, seed=5)
    g = torch.rand(7, generator=torch.Generator().manual_seed(1))
    g = g / g.sum()
    grad, gS = N.loss_and_gradient(colour, cover, ref, g)['grad']
    cd = colour.double().requires_grad_(True)
    N.loss_plain(cd, cover, ref, g).backward()
    gain = float(torch.tensor(np.float32(255.0)) * torch.tensor(np.float32(1.0 / colour.numel())))
    auto = cd.grad * (gain / (255.0 / colour.numel()))
    cov = gS > 0
    assert float(((grad - auto).abs()[cov] / gS[cov]).max()) <= 1e-10


def test_normalisation_is_exactly_invariant_under_gain_and_offset():
    """n(alpha x + beta; alpha eps) == n(x; eps) for alpha > 0, with taps that sum to 1 (here normalised in float64; the float32 taps do
    to 1 u per axis): the whole point of the loss.  The loss between an image and its own affine copy is then at rounding level."""
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(2, 23, 31, 2, generator=gen, dtype=torch.float64) * 140.0
    x[0, :, :10] = 45.0                                            # a flat region: the clamp's territory
    for k, sigma in ((15, 3.0), (31, 5.0)):
        g = N.taps(k, sigma).double()
        g = g / g.sum()
        n0 = N.normalised(x, g, 2.0)
        assert float(n0.abs().max()) > 1.0
        # (float64 itself cancels in m - mu^2: about 2^-53 (alpha x + beta)^2 / (alpha eps)^2, 1e-14 to 1e-13 for these pairs -- the
        # bound of 1e-12 is the statement's, the pairs are chosen so that float64 can show it)
        for alpha, beta in ((0.75, 8.0), (1.25, -6.0), (2.0, 30.0), (0.5, 20.0)):
            n1 = N.normalised(alpha * x + beta, g, alpha * 2.0)
            err = float((n1 - n0).abs().max())
            print(f"NORMREF invariance k{k} alpha={alpha} beta={beta} max |dn| = {err:.2e}")
            assert err <= 1e-12
            assert float(((n1 - n0) ** 2).mean()) <= 1e-24
        # with eps NOT scaled the copy differs, and a different image differs by order 1
        assert float((N.normalised(0.1 * x, g, 2.0) - n0).abs().max()) > 1e-3


def test_norm_shapes_cover_the_tile_extents():
    assert all(s in N.ALL_SHAPES for s in B.SHAPES) and len(B.SHAPES) == 7
    ws, hs = {s[2] for s in N.ALL_SHAPES if s[3] == 1}, {s[1] for s in N.ALL_SHAPES}
    assert {N.ROW_TX - 1, N.ROW_TX, N.ROW_TX + 1} <= ws and {N.COL_TY - 1, N.COL_TY, N.COL_TY + 1} <= hs
    assert {N.ROW_TY - 1, N.ROW_TY, N.ROW_TY + 1} <= hs
    assert {N.COL_TX // 4 - 1, N.COL_TX // 4, N.COL_TX // 4 + 1} <= ws and {N.COL_TX // 2 - 1, N.COL_TX // 2, N.COL_TX // 2 + 1} <= ws
    assert any(s[3] == 2 for s in N.ALL_SHAPES)
    src = open(os.path.join(ROOT, "fpc_diffrend_amd", "csrc", "sep_window.h")).read()
    assert re.search(rf"ROW_TX = {N.ROW_TX}, ROW_TY = {N.ROW_TY};", src) and re.search(rf"COL_TX = {N.COL_TX}, COL_TY = {N.COL_TY};", src)
    colour, cover, ref = N.flat_inputs()
    W = N.FLAT_SHAPE[2]
    assert bool((cover[:, :, : W // 2] == 0).all()) and bool((ref[:, :, : W // 2] == 45).all()) and bool((cover[:, :, W // 2:] > 0).any())


def test_fitconfig_has_the_norm_fields_off_by_default_and_excludes_the_blur():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert (cfg.norm_sigma, cfg.norm_kernel_size, cfg.norm_eps, cfg.norm_iters) == (0.0, 31, 2.0, 0)
    names = [f.name for f in dataclasses.fields(fit.FitConfig)]
    assert names.index('norm_sigma') > names.index('blur_iters') > names.index('frames_per_step')
    with pytest.raises(ValueError) as ei:
        fit.FitConfig(blur_sigma=3.0, norm_sigma=3.0)
    assert "blur_sigma" in str(ei.value) and "norm_sigma" in str(ei.value)
    fit.FitConfig(blur_sigma=3.0)
    fit.FitConfig(norm_sigma=3.0, norm_kernel_size=15, norm_iters=5)


def test_library_exports_the_norm_entry_with_abi_16_and_the_binding_mirrors_the_header():
    """(size and field offsets of the struct against the C compiler's: test_host_logic.py, for every parameter struct of the header)"""
    _lib, lib = lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert hasattr(lib, "fpcdr_norm_loss") and hasattr(lib, "fpcdr_norm_loss_scratch_bytes")
    assert lib.fpcdr_norm_loss_scratch_bytes(2, 37, 70, 3) == 2 * 37 * 70 * 3 * 4
    assert lib.fpcdr_norm_loss_scratch_bytes(2, 0, 70, 3) == 0
    header = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    assert re.search(r"#define FPCDR_ABI_VERSION 16\b", header)
    assert [f for f, _ in _lib.NormLoss._fields_][:10] == [f for f, _ in _lib.BlurLoss._fields_][:10]      # (the style of the blur's struct)


def test_bad_arguments_give_an_error_code_before_any_launch():
    """eps <= 0, a NaN or infinite eps, a radius outside 1 .. 31 or above min(H, W) - 1, a null or misaligned plane: the entry returns
    its error code from the argument checks, which come before the first HIP call -- so this runs on a machine without a GPU, on host
    memory the entry never touches.  An even kernel cannot be written into the C struct (it takes a radius); ops rejects it, with eps
    and the radius, before it looks at the tensors."""
    _lib, lib = lib_loaded()
    Bn, H, W, C = 1, 12, 9, 1
    n = Bn * H * W * C
    bufs = {name: (ctypes.c_float * (k * n + 4))() for name, k in (('color', 1), ('rast', 4), ('tmp', 4), ('stats', 4), ('d', 1), ('pq', 2),
                                                                  ('p', 1), ('grad_color', 1))}
    ref = (ctypes.c_uint8 * n)()
    acc = ctypes.c_double(0.0)
    al = lambda b: ctypes.c_void_p((ctypes.addressof(b) + 15) & ~15)

    def params(radius, eps=2.0, **over):
        kw = dict(color=al(bufs['color']), rast=al(bufs['rast']), ref=ctypes.cast(ref, ctypes.c_void_p), B=Bn, H=H, W=W, C=C,
                  bg=B.BACKGROUND, color_scale=255.0, grad_scale=1.0, eps=eps, radius=radius, tmp=al(bufs['tmp']), stats=al(bufs['stats']),
                  d=al(bufs['d']), pq=al(bufs['pq']), p=al(bufs['p']), loss_sum=ctypes.cast(ctypes.pointer(acc), ctypes.c_void_p),
                  grad_color=al(bufs['grad_color']))
        kw.update(over)
        return _lib.NormLoss(**kw)

    off = lambda b, k: ctypes.c_void_p(al(b).value + k)
    bad = [params(2, eps=0.0), params(2, eps=-2.0), params(2, eps=float('nan')), params(2, eps=float('inf')), params(2, eps=1e30),
           params(32), params(0), params(-1), params(min(H, W)), params(2, C=5), params(2, W=0), params(2, B=65536),
           params(2, tmp=None), params(2, stats=None), params(2, d=None), params(2, pq=None), params(2, p=None), params(2, color=None),
           params(2, rast=None), params(2, ref=None), params(2, loss_sum=None), params(2, tmp=off(bufs['tmp'], 4)),
           params(2, stats=off(bufs['stats'], 8)), params(2, pq=off(bufs['pq'], 4))]
    for i, p in enumerate(bad):
        assert lib.fpcdr_norm_loss(ctypes.byref(p), None) != 0, i
        assert b"fpcdr_norm_loss" in lib.fpcdr_last_error()
    assert acc.value == 0.0
    import fpc_diffrend_amd.ops as dr
    colour, cover, ref_t = N.inputs(Bn, H, W, C)
    rast = torch.zeros(Bn, H, W, 4)
    for kw in (dict(taps=torch.ones(4) / 4), dict(taps=torch.ones(65) / 65), dict(taps=torch.ones(2 * min(H, W) + 1)),
               dict(taps=torch.tensor([0.5, 0.7, -0.2])), dict(taps=torch.ones(3) / 3, eps=0.0), dict(taps=torch.ones(3) / 3, eps=-1.0),
               dict(taps=torch.ones(3) / 3, eps=float('nan')), dict(taps=torch.ones(3) / 3, eps=float('inf'))):
        with pytest.raises(ValueError, match="taps|kernel|eps"):
            dr.norm_loss_call(colour, rast, ref_t, kw['taps'], 1.0, eps=kw.get('eps', 2.0))
    for kw in (dict(sigma=2.0, kernel_size=8), dict(sigma=0.0, kernel_size=5), dict(sigma=None, kernel_size=5)):
        with pytest.raises(ValueError):
            dr.normalised_pixel_loss(colour, rast, ref_t, **kw)
    with pytest.raises(ValueError, match="GPU tensor"):                      # no CPU fallback
        dr.normalised_pixel_loss(colour, rast, ref_t, sigma=2.0, kernel_size=5)


def test_norm_kernels_have_no_private_segment():
    """the taps are indexed by a runtime radius -- from registers that would be a private segment.  They are read
    uniformly from the kernel arguments; read from the built object (tests/codeobj.py).  LDS: at least four workgroups a CU (160 KiB)."""
    import codeobj
    recs = codeobj.kernels("norm.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = set()
    for name, private, lds in recs:
        if "k_norm_" in name:
            seen.add(name)
            assert private == 0, name
            assert lds <= 160 * 1024 // 4, name
    assert len(seen) == 5, seen              # rows, cols<false>, cols<true>, point, rows_adj


# ---- the exposure scan on the CPU oracle: the reason for the design ---------------------------------------------------------------------
def test_exposure_scan_on_the_oracle(oracle_ops):
    """scene.make_scene(resolution=(128, 128), n_frames=1), cameras (0, 4), everything at the hidden truth; targets the oracle's own
    render, quantised; frame 0 moved along per_frame_t[0, 0] by d full-size pixels (1 unit = 3.494 px); camera 0's target becomes
    round(0.75 x + 8), camera 4's round(1.25 x - 6).  Normalised loss with k = 15, sigma = 3, eps = 2, float32.  Measured here:

        d    L2 equal         L2 gains         normalised equal     normalised gains
       -4    74.429 (g -11.6) 119.855 (g -6.15) 0.41086 (g -0.0479) 0.40909 (g -0.0488)
       -2    43.890 (g -36.3)  89.360 (g -33.8) 0.27423 (g -0.347)  0.27312 (g -0.344)
       -1    22.471 (g -44.1)  67.842 (g -40.6) 0.13884 (g -0.458)  0.13844 (g -0.454)
        0     0.017 (g -0.11)  45.288 (g -2.67) 0.00020 (g -0.0001) 0.00050 (g +0.0004)
       +1    22.549 (g +48.0)  67.974 (g +48.5) 0.13935 (g +0.473)  0.13905 (g +0.469)
       +2    43.920 (g +38.0)  89.443 (g +36.9) 0.27507 (g +0.367)  0.27420 (g +0.365)
       +4    74.528 (g +5.00) 119.984 (g +0.90) 0.41190 (g +0.0774) 0.40998 (g +0.0767)
    (g: the derivative of the value along per_frame_t[0, 0], per unit.)
    """
    from fpc_diffrend_amd import scene
    from oracle import fit as ofit
    PX = 3.494
    sc = scene.make_scene(resolution=(128, 128), n_frames=1)
    g = N.taps(15, 3.0)

    def state(d):
        st = ofit.State(sc, cams=[0, 4])
        with torch.no_grad():
            st.M1.copy_(torch.eye(1))
            st.M2.copy_(torch.tensor(sc.weights_gt).t())
            st.per_frame_t.copy_(torch.tensor(sc.t_gt))
            st.per_frame_q.copy_(torch.tensor(sc.q_gt))
            st.per_frame_t[0, 0] += d / PX
        return st

    with torch.no_grad():
        st = state(0.0)
        pos_clip, _ = ofit.clip_positions(st, torch.arange(1))
        _, image, _ = ofit.forward_from_clip(st, pos_clip, torch.zeros(2, 128, 128, dtype=torch.uint8))
        x = torch.round(image[..., 0] * 255.0)
        equal = x.clamp(0, 255).to(torch.uint8)
        gains = torch.stack([torch.round(0.75 * x[0] + 8.0), torch.round(1.25 * x[1] - 6.0)]).clamp(0, 255).to(torch.uint8)

    def evaluate(d, targets):
        out = []
        for norm in (False, True):
            st = state(d)
            pos_clip, _ = ofit.clip_positions(st, torch.arange(1))
            loss, image, rast = ofit.forward_from_clip(st, pos_clip, targets)
            if norm:
                loss = N.loss_plain(image, rast[..., 3], targets, g, eps=2.0)
            loss.backward()
            out.append((float(loss.detach()), float(st.per_frame_t.grad[0, 0])))
        return out

    table = {}
    for d in (-4, -2, -1, 0, 1, 2, 4):
        (l2e, gl2e), (ne, gne) = evaluate(float(d), equal)
        (l2g, gl2g), (ng, gng) = evaluate(float(d), gains)
        table[d] = dict(l2e=l2e, l2g=l2g, ne=ne, ng=ng, gne=gne, gng=gng)
        print(f"NORMREF scan d={d:+d}  L2 equal {l2e:.3f} (g {gl2e:+.3g})  L2 gains {l2g:.3f} (g {gl2g:+.3g})  "
              f"normalised equal {ne:.5f} (g {gne:+.3g})  normalised gains {ng:.5f} (g {gng:+.3g})")
    for d in (-4, -2, -1, 1, 2, 4):
        assert table[0]['ng'] < table[d]['ng'], d
    for d in (-2, -1):
        assert table[d]['gng'] < 0 and table[d]['gne'] < 0, d
    for d in (1, 2):
        assert table[d]['gng'] > 0 and table[d]['gne'] > 0, d
    for d in (-2, -1, 1, 2):
        assert abs(table[d]['ng'] - table[d]['ne']) < 0.02 * table[d]['ne'], d
    assert table[0]['l2g'] >= 100.0 * table[0]['l2e']

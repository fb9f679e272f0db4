"""CPU: the float64 restatement of the blurred pixel loss (tests/blur_ref.py) checked against torch itself, and the host side of the
feature (ops.gaussian_taps, FitConfig, the C ABI's new entry) -- no GPU.  The fold formula of the reflecting blur's adjoint is the
statement tests/test_gpu_blur.py judges the kernel's gradient by; here it is compared with torch.autograd through F.pad(reflect) +
conv2d at every shape the GPU file uses."""
import dataclasses
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import blur_ref as B  # noqa: E402
import fitstep_ref as R  # noqa: E402
from helpers import lib_loaded  # noqa: E402


@pytest.mark.parametrize("shape", B.SHAPES, ids=lambda s: "x".join(str(v) for v in s[:5]))
def test_fold_formula_gradient_equals_autograd(shape):
    Bn, H, W, C, k, sigma = shape
    colour, cover, ref = B.inputs(Bn, H, W, C)
    g = B.taps(k, sigma)
    E, S = B.blurred_residual(colour, cover, ref, g)
    assert E.dtype == torch.float64 and bool((S >= E.abs()).all())
    grad, gS = B.gradient(E, cover, g)
    cd = colour.double().requires_grad_(True)
    loss = B.loss_plain(cd, cover, ref, g)
    loss.backward()
    # gradient() scales by the float32 1 / n_total the kernel is handed; the plain expression divides by n_total
    gs = float(torch.tensor(1.0 / colour.numel(), dtype=torch.float32))
    auto = cd.grad * (colour.numel() * gs)
    err = float((grad - auto).abs().max() / auto.abs().max())
    print(f"BLURREF fold-vs-autograd {shape} {err:.2e}")
    assert err <= 1e-12
    assert abs(float(B.loss_sum(E, S)[0]) / colour.numel() - float(loss.detach())) <= 1e-12 * float(loss.detach())
    # uncovered entries: no gradient, no scale; covered ones have one
    unc = (cover <= 0)[..., None].expand_as(grad)
    assert bool((grad[unc] == 0).all()) and bool((gS[unc] == 0).all()) and bool((gS[~unc] > 0).all())


def test_fold_formula_holds_for_asymmetric_taps():
    """taps= may be anything: the adjoint must not lean on the symmetry of a Gaussian."""
    colour, cover, ref = B.inputs(1, 9, 12, 2, seed=5)
    g = torch.rand(7, generator=torch.Generator().manual_seed(1))
    E, _ = B.blurred_residual(colour, cover, ref, g)
    grad, _ = B.gradient(E, cover, g)
    cd = colour.double().requires_grad_(True)
    B.loss_plain(cd, cover, ref, g).backward()
    auto = cd.grad * (colour.numel() * float(torch.tensor(1.0 / colour.numel(), dtype=torch.float32)))
    assert float((grad - auto).abs().max() / auto.abs().max()) <= 1e-12


def test_constant_residual_blurs_to_itself_and_taps_are_normalised():
    for k, sigma in [(3, 0.8), (9, 1.5), (31, 5.0), (63, 9.0), (31, 0.1)]:
        g = B.taps(k, sigma)
        assert g.dtype == torch.float32 and g.numel() == k
        assert torch.equal(g, g.flip(0))
        assert abs(float(g.double().sum()) - 1.0) <= R.U
        n = (k - 1) // 2 + 1                                   # the smallest legal extent
        e = torch.full((2, n, n + 3, 2), 37.25, dtype=torch.float64)
        E = B.blurred(e, g)
        assert float((E - 37.25).abs().max()) <= 2 * R.U * 37.25      # (the float32 taps sum to 1 within 1 u, per axis)
    assert B.reflect_index(5, 3).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]


def test_ops_gaussian_taps_equals_the_reference_and_rejects_bad_arguments():
    import fpc_diffrend_amd.ops as dr
    for k, sigma in [(3, 0.8), (9, 1.5), (15, 3.0), (31, 5.0), (31, 2.0), (63, 9.0), (17, 4.0)]:
        t = dr.gaussian_taps(k, sigma)
        assert t.device.type == 'cpu' and t.dtype == torch.float32
        assert torch.equal(t, B.taps(k, sigma))
    for bad in [(30, 2.0), (1, 2.0), (65, 2.0), (31, 0.0), (31, -1.0), (4, 1.0)]:
        with pytest.raises(ValueError):
            dr.gaussian_taps(*bad)


def test_fitconfig_has_the_blur_fields_off_by_default():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert (cfg.blur_sigma, cfg.blur_sigma_end, cfg.blur_kernel_size, cfg.blur_iters) == (0.0, None, 31, 0)
    names = [f.name for f in dataclasses.fields(fit.FitConfig)]
    assert names.index('blur_sigma') > names.index('frames_per_step')      # under the build-side additions


def test_library_exports_the_blur_entry_with_abi_16_and_the_binding_mirrors_the_header():
    """(size and field offsets of the struct against the C compiler's: test_host_logic.py, for every parameter struct of the header)"""
    _lib, lib = lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert hasattr(lib, "fpcdr_blur_loss") and hasattr(lib, "fpcdr_blur_loss_scratch_bytes")
    assert lib.fpcdr_blur_loss_scratch_bytes(2, 37, 70, 3) == 2 * 37 * 70 * 3 * 4
    assert lib.fpcdr_blur_loss_scratch_bytes(0, 37, 70, 3) == 0
    header = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    assert re.search(r"#define FPCDR_ABI_VERSION 16\b", header)


def test_blur_kernels_have_no_private_segment():
    """The taps are indexed by a runtime radius: from registers that would be a private segment.  They are read
    uniformly from the kernel arguments instead; read from the built object (tests/codeobj.py)."""
    import codeobj
    recs = codeobj.kernels("blur.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = 0
    for name, private, lds in recs:
        if re.search(r"k_blur_rows|k_blur_cols", name):
            seen += 1
            assert private == 0, name
            assert lds <= 80 * 1024, name      # two workgroups per CU
    assert seen == 4


def test_gpu_blur_states_the_tile_extents_of_the_source():
    """tests/test_gpu_blur.py builds its EXTENT_SHAPES around a copy of the tile extents (it reads no C): that copy and
    csrc/sep_window.h state the same four numbers."""
    gpu_test = open(os.path.join(HERE, "test_gpu_blur.py")).read()
    m = re.search(r"^ROW_TX, ROW_TY = (\d+), (\d+)\nCOL_TX, COL_TY = (\d+), (\d+)$", gpu_test, re.M)
    assert m, "test_gpu_blur.py no longer states its tile extents in the form this test reads"
    row_tx, row_ty, col_tx, col_ty = m.groups()
    src = open(os.path.join(ROOT, "fpc_diffrend_amd", "csrc", "sep_window.h")).read()
    assert re.search(rf"ROW_TX = {row_tx}, ROW_TY = {row_ty};", src) and re.search(rf"COL_TX = {col_tx}, COL_TY = {col_ty};", src)

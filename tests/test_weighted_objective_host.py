"""CPU: the host side of the weighted one-pass objective ("Weighted objective rule") -- the two new symbols and the new
parameter struct, the function that states which iterations take the weighted one-pass call, the options that keep raising, the
background kernel's private segment, and a float64 numpy statement of the background sums against tests/robust_ref.py."""
import ctypes
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import codeobj
import robust_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fpcdr_objective_weighted_fwd", "fpcdr_ref_bg_wsum")


def test_new_symbols_are_declared_bound_and_exported_and_the_abi_version_stays():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*(fpcdr_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS, name
    assert re.search(r"#define FPCDR_ABI_VERSION 16\b", header) and _lib.ABI_VERSION == 16
    assert int(re.search(r"#define FPCDR_WSUM_SLOTS (\d+)", header).group(1)) == _lib.WSUM_SLOTS
    for path in (_lib.LIB_PATH, _lib.TWOCALL_LIB_PATH):
        lib = ctypes.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), f"{name} not exported by {os.path.basename(path)}"
    lib = _lib.load()      # (binds every symbol with its argument types)
    assert lib.fpcdr_abi_version() == 16
    assert lib.fpcdr_objective_weighted_fwd.argtypes[0]._type_ is _lib.ObjectiveWeighted
    assert len(lib.fpcdr_ref_bg_wsum.argtypes) == 11


def test_weighted_params_have_the_size_and_offsets_of_their_ctypes_mirror():
    """Ask the C compiler, as test_abi_library_exports_every_declared_symbol does for the other structs."""
    from fpc_diffrend_amd import _lib
    cls, name = _lib.ObjectiveWeighted, "fpcdr_objective_weighted_params"
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "sz.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "fpcdr.h"\nint main(void) {\n')
            f.write(f'    printf("size %zu\\n", sizeof({name}));\n    printf("base_size %zu\\n", sizeof(fpcdr_objective_params));\n')
            for field, _ in cls._fields_:
                f.write(f'    printf("{field} %zu\\n", offsetof({name}, {field}));\n')
            f.write("    return 0;\n}\n")
        exe = os.path.join(td, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        sizes = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert ctypes.sizeof(cls) == int(sizes["size"]) and ctypes.sizeof(_lib.Objective) == int(sizes["base_size"])
    assert [f for f, _ in cls._fields_] == ["base", "kind", "inv_c", "w_outside", "sat", "T_weights", "mask", "face_w", "wsum"]
    for field, _ in cls._fields_:
        assert getattr(cls, field).offset == int(sizes[field]), field


FLAGS = ("fused_objective", "fused_render", "fused_loss", "one_pass", "sparse_objective")


def test_which_iterations_take_the_weighted_one_pass_call():
    from fpc_diffrend_amd import fit
    assert fit.FitConfig().weighted_one_pass is False
    robust = dict(robust='charbonnier', robust_scale=10.0)
    # the option grid: the flag, every flag of the one-pass step, the shading, mip at the level, the channels
    for on, mip, shading, channels in itertools.product((False, True), (False, True), ('texture', 'vertex'), (1, 2, 3, 4)):
        for off in (None,) + FLAGS:
            kw = {off: False} if off else {}
            cfg = fit.FitConfig(weighted_one_pass=on, shading=shading, **robust, **kw)
            term = fit.pixel_term(cfg, 0)
            assert term == ('robust', 'charbonnier', 10.0)
            want = on and off is None and not mip and shading == 'texture' and channels in (1, 3, 4)
            assert fit.weighted_one_pass_term(cfg, term, mip, channels) is want, (on, mip, shading, channels, off)
    # the term decides: no term (the plain step), a windowed term, weights alone (kind 'l2')
    cfg = fit.FitConfig(weighted_one_pass=True)
    assert fit.pixel_term(cfg, 0) is None and fit.weighted_one_pass_term(cfg, None, False) is False
    assert fit.weighted_one_pass_term(cfg, fit.pixel_term(cfg, 0, weighted=True), False) is True
    assert fit.pixel_term(cfg, 0, weighted=True) == ('robust', 'l2', None)
    blur = fit.FitConfig(weighted_one_pass=True, blur_sigma=3.0, blur_kernel_size=15)
    assert fit.weighted_one_pass_term(blur, fit.pixel_term(blur, 0), False) is False
    # resuming across robust_iters: a function of the iteration alone
    cfg = fit.FitConfig(weighted_one_pass=True, robust_iters=5, **robust)
    took = [fit.weighted_one_pass_term(cfg, fit.pixel_term(cfg, i), False) for i in range(8)]
    assert took == [True] * 5 + [False] * 3
    resumed = [fit.weighted_one_pass_term(cfg, fit.pixel_term(cfg, i), False) for i in (4, 5, 6)]      # (a run picked up at 4)
    assert resumed == took[4:7]
    # ... and with weights on, the iterations after robust_iters keep the weighted call, with kind 'l2'
    cfg = fit.FitConfig(weighted_one_pass=True, robust_iters=5, weight_outside=0.0, **robust)
    terms = [fit.pixel_term(cfg, i, weighted=True) for i in (4, 5)]
    assert terms == [('robust', 'charbonnier', 10.0), ('robust', 'l2', None)]
    assert all(fit.weighted_one_pass_term(cfg, t, False) for t in terms)
    # a pyramid level under pyramid_mip hands mip=True: the operator path
    assert fit.weighted_one_pass_term(cfg, terms[0], True) is False


def test_hip_graph_with_weights_keeps_raising():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig(weighted_one_pass=True, hip_graph=True, saturation=140)
    with pytest.raises(ValueError, match="hip_graph"):
        fit.check_pixel_terms(cfg)
    with pytest.raises(ValueError, match="hip_graph"):
        fit.check_pixel_terms(fit.FitConfig(weighted_one_pass=True, hip_graph='auto'), has_masks=True)
    fit.check_pixel_terms(fit.FitConfig(weighted_one_pass=True, saturation=140))


def test_pixel_objective_keywords_and_their_defaults():
    """The new keywords are off by default: without them the call is the plain one."""
    import fpc_diffrend_amd.ops as dr
    assert dr.robust_args('charbonnier', 10.0, 0.25, 130) == (1, float(np.float32(0.1)), 0.25, 130)
    import inspect
    sig = inspect.signature(dr.pixel_objective).parameters
    assert [sig[k].default for k in ("robust", "mask", "face_weights", "weight_outside", "saturation", "ref_bg_wsum", "wsum_out")] == \
        [None, None, None, 1.0, 0, None, None]
    assert list(inspect.signature(dr.reference_background_weighted).parameters)[:7] == \
        ["ref_u8", "mask", "kind", "scale", "weight_outside", "saturation", "background"]


def test_background_kernel_has_no_private_segment():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(os.path.join(codeobj.BUILD, "robust.o")):
        _lib.build()
    ks = codeobj.kernels("robust.o")
    if ks is None:
        pytest.skip("no build products or no llvm tools")
    bg = [k for k in ks if "k_robust_bg" in k[0]]
    assert len(bg) == 3, [k[0] for k in ks]
    for name, private, lds in bg:
        assert private == 0 and lds <= 64, (name, private, lds)
    # the weighted instantiations of the objective: present, and without a private segment (test_host_logic holds them by name too)
    ko = codeobj.kernels("objective.o")
    w = [k for k in ko if re.search(r"k_shade_list_w|k_shade_queue_w|k_fix_list_w|k_fix_queue_w", k[0])]
    assert len(w) == 4 + 3 + 6 + 6, [k[0] for k in w]
    for name, private, _ in w:
        assert private == 0, (name, private)


def _bg_numpy(ref, mask, kind, c, w_outside, sat, bg_scaled):
    """The float64 statement of fpcdr_ref_bg_wsum for one image, in numpy: (sum of w0 * rho(ref - bg_scaled), sum of w0)."""
    r = ref.astype(np.float64).reshape(-1)
    wm = np.ones_like(r) if mask is None else mask.astype(np.float64).reshape(-1) * float(np.float32(1.0) / np.float32(255.0))
    if sat > 0:
        wm = np.where(ref.reshape(-1) >= sat, 0.0, wm)
    w0 = wm * float(np.float32(w_outside))
    d = r - bg_scaled
    dd = d * d
    if kind == 'l2':
        rho = dd
    else:
        t = (d * RR.inv_scale(c)) ** 2
        rho = 2.0 * dd / (1.0 + np.sqrt(1.0 + t)) if kind == 'charbonnier' else dd / (1.0 + t)
    return float((w0 * rho).sum()), float(w0.sum())


@pytest.mark.parametrize("kind,c", [('l2', None), ('charbonnier', 2.0), ('charbonnier', 20.0), ('geman_mcclure', 2.0), ('geman_mcclure', 20.0)])
def test_background_sums_in_numpy_agree_with_the_robust_statement_on_an_uncovered_image(kind, c):
    inp = RR.inputs(2, 9, 31, 1, seed=5)
    bgs = float(np.float32(RR.BACKGROUND)) * 255.0
    for use_mask, w_out, sat in ((False, 1.0, 0), (True, 1.0, 0), (True, 0.25, RR.SAT), (False, 0.0, 0), (False, 0.25, 1)):
        for b in range(2):
            ref, mask = inp['ref'][b:b + 1], inp['mask'][b:b + 1] if use_mask else None
            uncovered = torch.zeros(1, 9, 31)
            s = RR.robust_loss(torch.zeros(1, 9, 31, 1), uncovered, ref, kind, c, mask=mask, w_outside=w_out, sat=sat)['sums'][0]
            w, cov = RR.weights(uncovered, ref, mask, None, w_out, sat)
            assert not bool(cov.any())
            plain = RR.loss_plain(torch.zeros(1, 9, 31, 1, dtype=torch.float64), uncovered, ref, kind, c, n_total=1, weight=w)
            got = _bg_numpy(ref.numpy(), None if mask is None else mask.numpy(), kind, c, w_out, sat, bgs)
            assert abs(got[0] - float(s[0])) <= 1e-12 * max(abs(float(s[0])), 1.0), (kind, c, use_mask, w_out, sat)
            assert abs(got[1] - float(s[1])) <= 1e-12 * max(abs(float(s[1])), 1.0)
            assert abs(got[0] - float(plain)) <= 1e-9 * max(abs(float(plain)), 1.0)      # (the textbook form of rho)
            if w_out == 0.0:
                assert got == (0.0, 0.0)

"""CPU: the float64 statement of the texture prior (tests/tex_prior_ref.py; DESIGN.md 3, "Texture prior rule") against torch.autograd of
a plain restatement and against central finite differences, the consequences of the rule (exact zeros, selects, the degenerate shapes,
the L2 limit of the Charbonnier form), the argument errors of FitConfig / fit.texture_prior / fpcdr_tex_prior that need no GPU, and the
private segment of the built kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tex_prior_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1, 1), (1, 5, 1), (5, 1, 1), (3, 7, 3)]


def _tex(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def _map(Ht, Wt, seed):
    """Weights in (0, 2) with zeros: a whole row, a whole column and single texels where the shape has room."""
    w = 0.1 + 1.9 * torch.rand(Ht, Wt, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    if Ht > 2:
        w[1, :] = 0.0
    if Wt > 2:
        w[:, 2] = 0.0
    w.reshape(-1)[::5] = 0.0
    return w


def _variants(shape, seed):
    Ht, Wt, _ = shape
    a = _tex(shape, seed + 1)
    for sw in (None, _map(Ht, Wt, seed + 2)):
        for anchor, aw in ((None, None), (a, None), (a, _map(Ht, Wt, seed + 3))):
            yield sw, anchor, aw


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("scale", [None, 0.3])
def test_statement_equals_autograd_of_the_plain_form(shape, scale):
    t = _tex(shape, 3)
    # (the statement takes inv_c as a float32; the plain form is handed the c that float32 stands for)
    inv_c = 0.0 if scale is None else float(np.float32(1.0 / scale))
    c = None if scale is None else 1.0 / inv_c
    for sw, anchor, aw in _variants(shape, 10):
        leaf = t.clone().requires_grad_(True)
        val = T.tex_prior_plain(leaf, 3.5, 0.75, anchor, sw, aw, c)
        g, = torch.autograd.grad(val, leaf, allow_unused=True) if val.requires_grad else (None,)
        g = torch.zeros_like(t) if g is None else g
        val = val.detach()
        ref = T.tex_prior(t, 3.5, 0.75, anchor, sw, aw, inv_c)
        assert abs(float(ref['value'][0]) - float(val)) <= 1e-13 * max(1.0, abs(float(val)))
        assert float((ref['grad'][0] - g).abs().max()) <= 1e-13 * max(1.0, float(g.abs().max()))
        # the scales dominate the values, and vanish exactly where the weights say there is no term
        assert bool((ref['grad'][1] >= ref['grad'][0].abs() * (1 - 1e-12)).all())
        zg, zp, zv = ref['zeros']
        assert int((ref['grad'][1] == 0).sum()) == zg and int((ref['part'][1] == 0).sum()) == zp and int((ref['value'][1] == 0).sum()) == zv
        assert bool((ref['grad'][0][ref['grad'][1] == 0] == 0).all())


@pytest.mark.parametrize("scale", [None, 0.3])
def test_statement_equals_central_differences(scale):
    shape = (3, 4, 2)
    t = _tex(shape, 4)
    inv_c = 0.0 if scale is None else float(np.float32(1.0 / scale))
    sw, aw, a = _map(3, 4, 5), _map(3, 4, 6), _tex(shape, 7)
    f = lambda x: float(T.tex_prior(x, 2.0, 1.5, a, sw, aw, inv_c)['value'][0])
    g = T.tex_prior(t, 2.0, 1.5, a, sw, aw, inv_c)['grad'][0]
    h = 1e-5
    fd = torch.zeros_like(t)
    for i in range(t.numel()):
        e = torch.zeros(t.numel(), dtype=torch.float64)
        e[i] = h
        e = e.reshape(shape)
        fd.reshape(-1)[i] = (f(t + e) - f(t - e)) / (2 * h)
    assert float((fd - g).abs().max()) <= 1e-7 * max(1.0, float(g.abs().max()))


def test_degenerate_shapes_have_no_pairs_on_the_missing_axis():
    one = T.tex_prior(_tex((1, 1, 3), 1), 2.0, 0.0)
    assert float(one['value'][0]) == 0.0 and float(one['grad'][0].abs().max()) == 0.0 and one['zeros'] == (3, 2, 1)
    t = _tex((1, 5, 1), 2)
    row = T.tex_prior(t, 1.0, 0.0)
    assert abs(float(row['part'][0][0]) - float(((t[0, 1:] - t[0, :-1]) ** 2).sum() / 5)) <= 1e-15
    col = T.tex_prior(t.reshape(5, 1, 1), 1.0, 0.0)
    assert float(col['part'][0][0]) == float(row['part'][0][0])
    assert torch.equal(col['grad'][0].reshape(-1), row['grad'][0].reshape(-1))
    # no pair across the border: the first and last texel of a row have one neighbour each
    ramp = torch.arange(5, dtype=torch.float64).reshape(1, 5, 1)
    g = T.tex_prior(ramp, 1.0, 0.0)['grad'][0].reshape(-1)
    assert g.tolist() == [2.0 / 5 * -1.0, 0.0, 0.0, 0.0, 2.0 / 5 * 1.0]


@pytest.mark.parametrize("scale", [None, 0.3])
def test_zero_weights_are_selects_even_for_a_nan_texel(scale):
    inv_c = 0.0 if scale is None else 1.0 / scale
    shape = (4, 6, 3)
    t, a = _tex(shape, 8), _tex(shape, 9)
    sw, aw = torch.ones(4, 6, dtype=torch.float64), torch.ones(4, 6, dtype=torch.float64)
    sw[2, 3] = aw[2, 3] = 0.0
    good = T.tex_prior(t, 2.0, 1.0, a, sw, aw, inv_c)
    bad = t.clone()
    bad[2, 3] = float('nan')
    out = T.tex_prior(bad, 2.0, 1.0, a, sw, aw, inv_c)
    for k in ('part', 'value', 'grad'):
        assert torch.equal(out[k][0], good[k][0]), k
    assert float(out['grad'][0][2, 3].abs().max()) == 0.0 and good['zeros'] == (3, 0, 0)
    # a pair takes the smaller of its two weights
    sw2 = torch.ones(1, 3, dtype=torch.float64)
    sw2[0, 1] = 0.25
    r = torch.tensor([0.0, 1.0, 3.0], dtype=torch.float64).reshape(1, 3, 1)
    assert abs(float(T.tex_prior(r, 1.0, 0.0, smooth_w=sw2)['part'][0][0]) - 0.25 * (1.0 + 4.0) / 3) <= 1e-15


def test_the_charbonnier_value_tends_to_l2_for_large_scales_and_is_linear_above_the_scale():
    t = _tex((5, 6, 3), 11)
    l2 = T.tex_prior(t, 1.0, 0.0)
    prev = None
    for c in (1.0, 1e2, 1e4):
        ch = T.tex_prior(t, 1.0, 0.0, inv_c=1.0 / c)
        gap = abs(float(ch['value'][0] - l2['value'][0])) / float(l2['value'][0])
        assert float(ch['value'][0]) <= float(l2['value'][0])            # rho(s) <= s
        assert prev is None or gap < prev * 1e-2                          # the gap is s / (4 c^2) to first order
        prev = gap
    assert prev < 1e-7
    step = torch.zeros(1, 2, 1, dtype=torch.float64)
    step[0, 1, 0] = 10.0                                                  # one edge of height 10 at c = 2^-7: rho ~ 2 c |d|
    c = 2.0 ** -7
    assert abs(float(T.tex_prior(step, 1.0, 0.0, inv_c=1.0 / c)['part'][0][0]) * 2 - 2 * c * 10.0) <= 2 * c * c * 1.001


# ---------------------------------------------------------------------------------------------------------------------
# argument errors that need no GPU
# ---------------------------------------------------------------------------------------------------------------------

def test_fitconfig_texture_prior_option_errors():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert cfg.weight_tex_smooth == 0.0 and cfg.weight_tex_anchor == 0.0 and cfg.tex_smooth_scale is None
    assert cfg.tex_smooth_weights is None and cfg.tex_anchor_weights is None
    for name in ("weight_tex_smooth", "weight_tex_anchor"):
        for bad in (-1.0, float('nan'), float('inf'), "x"):
            with pytest.raises(ValueError, match=name):
                fit.FitConfig(**{name: bad})
        with pytest.raises(ValueError, match="optimize_texture"):
            fit.FitConfig(**{name: 1.0}, optimize_texture=False)
        fit.FitConfig(**{name: 1.0})
    for scale in (0.0, -1.0, float('inf'), float('nan'), 1e-60, "x"):
        with pytest.raises(ValueError, match="tex_smooth_scale"):
            fit.FitConfig(tex_smooth_scale=scale)
    fit.FitConfig(weight_tex_smooth=2.0, tex_smooth_scale=0.05, tex_smooth_weights='chart', weight_tex_anchor=1.0)
    fit.FitConfig(optimize_texture=False, tex_smooth_scale=0.05)          # (the term off: nothing is asked of the other options)


def test_texel_weight_maps_are_checked_and_an_image_is_read_as_bytes_over_255(tmp_path):
    from PIL import Image
    from fpc_diffrend_amd import fit
    w = fit.load_texel_weights([[0, 1, 2], [0.5, 0, 3]], 2, 3, 'tex_smooth_weights')
    assert w.dtype == np.float32 and w.tolist() == [[0, 1, 2], [0.5, 0, 3]]
    for bad, why in ((np.ones((3, 2)), "one number per texel"), (np.ones(6), "one number per texel"),
                     ([[0, 1, -2], [0, 0, 0]], "finite and not negative"), ([[0, 1, float('nan')], [0, 0, 0]], "finite and not negative")):
        with pytest.raises(ValueError, match=why):
            fit.load_texel_weights(bad, 2, 3, 'tex_smooth_weights')
    img = np.array([[0, 51, 255], [102, 0, 204]], dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "w.png")
    w = fit.load_texel_weights(str(tmp_path / "w.png"), 2, 3, 'tex_anchor_weights')
    assert np.array_equal(w, (img[::-1].astype(np.float64) / 255.0).astype(np.float32))      # (the image's top row is the texture's last)
    with pytest.raises(ValueError, match="cannot read"):
        fit.load_texel_weights(str(tmp_path / "none.png"), 2, 3, 'tex_anchor_weights')
    with pytest.raises(ValueError, match="one number per texel"):
        fit.load_texel_weights(str(tmp_path / "w.png"), 3, 2, 'tex_anchor_weights')


def test_texture_prior_argument_errors():
    from fpc_diffrend_amd import fit
    t = torch.zeros(4, 5, 3)
    for scale in (0.0, -2.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match="scale"):
            fit.texture_prior(t, 1.0, 0.0, scale=scale)
    for ws, wa in ((-1.0, 0.0), (0.0, -1.0), (float('nan'), 0.0), (0.0, float('inf'))):
        with pytest.raises(ValueError, match="finite and not negative"):
            fit.texture_prior(t, ws, wa)
    for bad in (torch.zeros(4, 5), torch.zeros(4, 5, 5), torch.zeros(4, 5, 3, dtype=torch.float64), torch.zeros(0, 5, 3)):
        with pytest.raises(ValueError, match=r"float32 \[Ht,Wt,C\]"):
            fit.texture_prior(bad, 1.0, 0.0)
    for a in (torch.zeros(4, 5, 1), torch.zeros(4, 5, 3, dtype=torch.float64), [0.0]):
        with pytest.raises(ValueError, match="anchor must be a float32 tensor"):
            fit.texture_prior(t, 1.0, 1.0, anchor=a)
    with pytest.raises(ValueError, match="anchor_weights without an anchor"):
        fit.texture_prior(t, 1.0, 1.0, anchor_weights=torch.ones(4, 5))
    for name in ("smooth_weights", "anchor_weights"):
        for w in (torch.ones(5, 4), torch.ones(4, 5, dtype=torch.float64), np.ones((4, 5), dtype=np.float32)):
            with pytest.raises(ValueError, match=name + " must be a float32 tensor"):
                fit.texture_prior(t, 1.0, 1.0, anchor=t, **{name: w})
        for v in (-1.0, float('nan'), float('inf')):
            w = torch.ones(4, 5)
            w[1, 2] = v
            with pytest.raises(ValueError, match=name + " must be finite and not negative"):
                fit.texture_prior(t, 1.0, 1.0, anchor=t, **{name: w})
    with pytest.raises(RuntimeError, match="GPU only"):                   # valid arguments: no CPU fallback
        fit.texture_prior(t, 1.0, 1.0, anchor=t, smooth_weights=torch.ones(4, 5), anchor_weights=torch.ones(4, 5), scale=0.1)


def _lib_loaded():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def test_the_library_exports_the_entry_and_abi_stays_16():
    _lib, lib = _lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert "fpcdr_tex_prior" in _lib.SYMBOLS and hasattr(lib, "fpcdr_tex_prior")
    assert "int fpcdr_tex_prior(" in open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    if os.path.exists(_lib.TWOCALL_LIB_PATH):
        assert hasattr(ctypes.CDLL(_lib.TWOCALL_LIB_PATH), "fpcdr_tex_prior")
    from fpc_diffrend_amd import fit, ops
    assert callable(ops.tex_prior_call) and callable(fit.texture_prior) and callable(fit.chart_map)


def test_bad_arguments_give_an_error_code_before_any_launch():
    """Nulls, sizes, a channel count outside 1..4, a misaligned acc, weights of an absent anchor, a negative or non-finite inv_c or weight:
    the checks come before the first HIP call, so this runs without a GPU on host memory the entry never touches."""
    _lib, lib = _lib_loaded()
    Ht, Wt, C = 3, 5, 3
    fb = lambda n: (ctypes.c_float * (n + 4))()
    tex, anchor, sw, aw, g, part, out = fb(Ht * Wt * C), fb(Ht * Wt * C), fb(Ht * Wt), fb(Ht * Wt), fb(Ht * Wt * C), fb(2), fb(1)
    acc = (ctypes.c_double * 3)()
    P = lambda b: ctypes.cast(b, ctypes.c_void_p)
    names = ('tex', 'anchor', 'smooth_w', 'anchor_w', 'inv_c', 'w_smooth', 'w_anchor', 'grad_tex', 'acc', 'part', 'out', 'Ht', 'Wt', 'C')

    def args(**over):
        kw = dict(tex=P(tex), anchor=P(anchor), smooth_w=P(sw), anchor_w=P(aw), inv_c=0.0, w_smooth=1.0, w_anchor=1.0, grad_tex=P(g),
                  acc=P(acc), part=P(part), out=P(out), Ht=Ht, Wt=Wt, C=C)
        kw.update(over)
        return [kw[k] for k in names] + [None]

    bad = [dict(tex=None), dict(acc=None), dict(part=None), dict(out=None), dict(acc=ctypes.c_void_p(ctypes.addressof(acc) + 4)),
           dict(Ht=0), dict(Ht=-1), dict(Wt=0), dict(Wt=-3), dict(C=0), dict(C=5), dict(C=-1), dict(Ht=1 << 16, Wt=1 << 16),
           dict(anchor=None), dict(inv_c=-1.0), dict(inv_c=float('inf')), dict(inv_c=float('nan')), dict(w_smooth=-1.0),
           dict(w_smooth=float('nan')), dict(w_anchor=-0.5), dict(w_anchor=float('inf'))]
    for i, over in enumerate(bad):
        assert lib.fpcdr_tex_prior(*args(**over)) != 0, i
        assert b"fpcdr_tex_prior" in lib.fpcdr_last_error()
    assert all(v == 0.0 for v in acc)


def test_tex_prior_kernels_have_no_private_segment():
    """read from the built object (tests/codeobj.py).  A thread's run of four texels, its neighbours and its gradient are
    indexed by compile-time constants only: C in 1..4, each with and without vector loads, and the finish."""
    import codeobj
    recs = codeobj.kernels("tex_prior.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    main = {name: private for name, private, _ in recs if "k_tex_prior" in name and "finish" not in name}
    assert len(main) == 8 and all(p == 0 for p in main.values()), main
    finish = {name: private for name, private, _ in recs if "k_tex_prior_finish" in name}
    assert len(finish) == 1 and all(p == 0 for p in finish.values()), finish

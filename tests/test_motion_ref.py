"""CPU: the float64 statement of the motion term (tests/motion_ref.py; DESIGN.md 3, "Motion rule") against torch.autograd of a plain
restatement and against central finite differences, the consequences of the rule (exact zeros, the invariances, zero weights, the L2
limit of the Charbonnier form), the argument errors of FitConfig / fit.motion_penalty / fpcdr_motion_penalty that need no GPU, and the
private segment of the built kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

import motion_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAME_LISTS = [None, [0, 1, 2, 4, 5, 6, 7, 9], [0, 2, 4], [3], [5, 6], [1000000, 1000001, 1000002, 1000004]]


def _x(F, V, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    x = 0.3 * torch.randn(F, V, 3, generator=g, dtype=torch.float64)
    x[..., 1] += 170.0
    return x.to(dtype)


def _frames(ft):
    return 7 if ft is None else len(ft)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("scale", [None, 0.4])
@pytest.mark.parametrize("ft", FRAME_LISTS)
def test_statement_equals_autograd_of_the_plain_form(order, scale, ft):
    F, V = _frames(ft), 5
    x = _x(F, V, 3).requires_grad_(True)
    w = torch.tensor([1.0, 0.0, 2.5, 0.5, 1.0], dtype=torch.float64)
    for vw in (None, w):
        # (the statement takes inv_c as a float32; the plain form is handed the c that float32 stands for)
        inv_c = 0.0 if scale is None else float(np.float32(1.0 / scale))
        c = None if scale is None else 1.0 / inv_c
        val = M.motion_plain(x, 3.5, ft, order, c, vw)
        g, = torch.autograd.grad(val, x, allow_unused=True)
        g = torch.zeros_like(x) if g is None else g
        val = val.detach()
        ref = M.motion(x.detach(), 3.5, ft, order, inv_c, vw)
        assert abs(float(ref['value'][0]) - float(val)) <= 1e-13 * max(1.0, abs(float(val)))
        assert float((ref['grad'][0] - g).abs().max()) <= 1e-13 * max(1.0, float(g.abs().max()))
        m = M.stencil_flags(F, ft, order)
        assert bool((ref['per'][0][~m] == 0).all())
        # the scales dominate the values, and vanish only where no term is
        assert bool((ref['grad'][1] >= ref['grad'][0].abs() * (1 - 1e-12)).all())
        assert int((ref['grad'][1] == 0).sum()) == ref['zeros'][0] and int((ref['per'][1] == 0).sum()) == ref['zeros'][1]


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("scale", [None, 0.4])
def test_statement_equals_central_differences(order, scale):
    ft = [0, 1, 2, 4, 5, 6, 7, 9]
    F, V = len(ft), 3
    x = _x(F, V, 4)
    inv_c = 0.0 if scale is None else float(np.float32(1.0 / scale))
    w = torch.tensor([1.0, 0.25, 2.0], dtype=torch.float64)
    g = M.motion(x, 2.0, ft, order, inv_c, w)['grad'][0]
    h = 1e-5
    fd = torch.zeros_like(x)
    for i in range(x.numel()):
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[i] = h
        e = e.reshape(x.shape)
        fd.reshape(-1)[i] = (M.motion(x + e, 2.0, ft, order, inv_c, w)['value'][0] - M.motion(x - e, 2.0, ft, order, inv_c, w)['value'][0]) / (2 * h)
    assert float((fd - g).abs().max()) <= 1e-7 * max(1.0, float(g.abs().max()))


@pytest.mark.parametrize("scale", [None, 0.4])
def test_exactly_zero_without_a_valid_stencil(scale):
    inv_c = 0.0 if scale is None else 1.0 / scale
    for ft, F, orders in (([3], 1, (1, 2)), (None, 1, (1, 2)), ([0, 2, 4], 3, (1, 2)), (None, 2, (2,)), ([5, 6], 2, (2,))):
        for order in orders:
            ref = M.motion(_x(F, 4, 5), 3.0, ft, order, inv_c)
            assert float(ref['value'][0]) == 0.0 and float(ref['per'][0].abs().max()) == 0.0 and float(ref['grad'][0].abs().max()) == 0.0
            assert ref['zeros'] == (F * 4 * 3, F)
            assert int((ref['grad'][1] == 0).sum()) == F * 4 * 3
    # ... and order 1 on two adjacent frames is not zero
    assert float(M.motion(_x(2, 4, 5), 3.0, [5, 6], 1, inv_c)['value'][0]) > 0.0


def test_zero_counts_follow_the_frame_numbers():
    # [0,1,2,4,5,6,7,9]: order 2 is valid at the frames 1 (0,1,2), 5 (4,5,6) and 6 (5,6,7): the entry of frame number 9 is reached by none
    assert M.stencil_flags(8, [0, 1, 2, 4, 5, 6, 7, 9], 2).tolist() == [False, True, False, False, True, True, False, False]
    assert M.zero_entries(8, 10, [0, 1, 2, 4, 5, 6, 7, 9], 2) == (1 * 30, 5)
    # order 1: the steps 0-1, 1-2, 4-5, 5-6, 6-7
    assert M.stencil_flags(8, [0, 1, 2, 4, 5, 6, 7, 9], 1).tolist() == [True, True, False, True, True, True, False, False]
    assert M.zero_entries(8, 10, [0, 1, 2, 4, 5, 6, 7, 9], 1) == (1 * 30, 3)
    assert M.zero_entries(5, 2, None, 2) == (0, 2) and M.zero_entries(5, 2, None, 1) == (0, 1)


def test_order_2_ignores_a_constant_velocity_and_order_1_a_constant_offset():
    F, V = 7, 6
    x = _x(F, V, 6)
    u = torch.tensor([0.3, -0.2, 0.11], dtype=torch.float64)
    for inv_c in (0.0, 2.5):
        a = M.motion(x, 2.0, None, 2, inv_c)
        b = M.motion(x + torch.arange(F, dtype=torch.float64)[:, None, None] * u, 2.0, None, 2, inv_c)
        # the accelerations are 1e-1 and differ by the rounding of positions at 170: 1e-14 relative to 170, 1e-12 relative to a
        assert abs(float(a['value'][0] - b['value'][0])) <= 1e-11 * float(a['value'][0])
        assert float((a['grad'][0] - b['grad'][0]).abs().max()) <= 1e-11 * float(a['grad'][0].abs().max())
        a = M.motion(x, 2.0, None, 1, inv_c)
        b = M.motion(x + u, 2.0, None, 1, inv_c)
        assert abs(float(a['value'][0] - b['value'][0])) <= 1e-11 * float(a['value'][0])
        assert float((a['grad'][0] - b['grad'][0]).abs().max()) <= 1e-11 * float(a['grad'][0].abs().max())
        # ... and order 1 does see the velocity
        c = M.motion(x + torch.arange(F, dtype=torch.float64)[:, None, None] * u, 2.0, None, 1, inv_c)
        assert float(c['value'][0]) > 1.05 * float(a['value'][0])


@pytest.mark.parametrize("order", [1, 2])
def test_a_zero_weight_removes_the_vertex(order):
    F, V = 6, 5
    x = _x(F, V, 7)
    w = torch.ones(V, dtype=torch.float64)
    w[2] = 0.0
    full, cut = M.motion(x, 1.0, None, order, 1.5), M.motion(x, 1.0, None, order, 1.5, w)
    keep = [0, 1, 3, 4]
    rest = M.motion(x[:, keep], 1.0, None, order, 1.5)
    assert float(cut['grad'][0][:, 2].abs().max()) == 0.0 and float(cut['grad'][1][:, 2].abs().max()) == 0.0
    assert torch.equal(cut['grad'][0][:, keep], full['grad'][0][:, keep])
    # the value share: the mean is still over all V vertices
    assert abs(float(cut['value'][0]) - float(rest['value'][0]) * len(keep) / V) <= 1e-15 * float(full['value'][0]) * 10
    assert float(cut['value'][0]) < float(full['value'][0])


@pytest.mark.parametrize("order", [1, 2])
def test_the_charbonnier_value_tends_to_l2_for_large_scales(order):
    x = _x(6, 5, 8)
    l2 = M.motion(x, 1.0, None, order, 0.0)
    prev = None
    for c in (1.0, 1e2, 1e4):
        ch = M.motion(x, 1.0, None, order, 1.0 / c)
        gap = abs(float(ch['value'][0] - l2['value'][0])) / float(l2['value'][0])
        assert float(ch['value'][0]) <= float(l2['value'][0])            # rho(s) <= s
        assert prev is None or gap < prev * 1e-2                          # the gap is s / (4 c^2) to first order
        prev = gap
    assert prev < 1e-7
    assert float((ch['grad'][0] - l2['grad'][0]).abs().max()) <= 1e-7 * float(l2['grad'][0].abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# argument errors that need no GPU
# ---------------------------------------------------------------------------------------------------------------------

def test_fitconfig_motion_option_errors():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert cfg.weight_motion == 0.0 and cfg.motion_order == 2 and cfg.motion_scale is None and cfg.motion_vertex_weights is None
    for order in (0, 3, 1.5, True, None):
        with pytest.raises(ValueError, match="motion_order"):
            fit.FitConfig(motion_order=order)
    for scale in (0.0, -1.0, float('inf'), float('nan'), 1e-60):
        with pytest.raises(ValueError, match="motion_scale"):
            fit.FitConfig(motion_scale=scale)
    with pytest.raises(ValueError, match="frames_per_step"):
        fit.FitConfig(weight_motion=1.0, frames_per_step=2)
    with pytest.raises(ValueError, match="frames_per_step"):
        fit.FitConfig(weight_motion=1.0, motion_order=1, frames_per_step=1)
    fit.FitConfig(weight_motion=1.0, frames_per_step=3)
    fit.FitConfig(weight_motion=1.0, motion_order=1, frames_per_step=2)
    fit.FitConfig(frames_per_step=1)                                      # (the term off: the reference's run shape stays legal)


def test_motion_options_of_the_mesh_and_the_shard(tmp_path):
    """What Fitter.__init__ checks before it touches the GPU (fit.motion_options)."""
    from fpc_diffrend_amd import fit
    V = 6
    cfg = fit.FitConfig(weight_motion=2.0, motion_scale=0.5, motion_vertex_weights=[1, 0, 2, 1, 1, 0.5])
    inv_c, w = fit.motion_options(cfg, V, 3)
    assert inv_c == 2.0 and w.dtype == np.float32 and w.tolist() == [1, 0, 2, 1, 1, 0.5]
    assert fit.motion_options(fit.FitConfig(weight_motion=2.0), V, 3) == (0.0, None)
    with pytest.raises(ValueError, match="shard"):
        fit.motion_options(cfg, V, 2)
    fit.motion_options(fit.FitConfig(weight_motion=2.0, motion_order=1), V, 2)
    with pytest.raises(ValueError, match="shard"):
        fit.motion_options(fit.FitConfig(weight_motion=2.0, motion_order=1), V, 1)
    for bad, why in (([1.0] * 5, "one number per vertex"), ([1, 1, 1, 1, 1, -0.5], "finite and not negative"),
                     ([1, 1, 1, 1, 1, float('nan')], "finite and not negative"), (np.ones((6, 1)), "one number per vertex")):
        with pytest.raises(ValueError, match=why):
            fit.motion_options(fit.FitConfig(weight_motion=1.0, motion_vertex_weights=bad), V, 4)
    path = tmp_path / "w.txt"
    path.write_text("\n".join(str(v) for v in (1, 0, 0.25, 3, 1, 1)) + "\n")
    assert fit.motion_options(fit.FitConfig(weight_motion=1.0, motion_vertex_weights=str(path)), V, 4)[1].tolist() == [1, 0, 0.25, 3, 1, 1]
    with pytest.raises(ValueError, match="cannot read"):
        fit.motion_options(fit.FitConfig(weight_motion=1.0, motion_vertex_weights=str(tmp_path / "none.txt")), V, 4)
    # the face weights' loader reads as it did
    with pytest.raises(ValueError, match="FitConfig.face_weights holds one number per face"):
        fit.load_face_weights([1.0, 2.0], 3)


def test_motion_penalty_argument_errors():
    from fpc_diffrend_amd import fit
    x = torch.zeros(4, 5, 3)
    for order in (0, 3, True):
        with pytest.raises(ValueError, match="order"):
            fit.motion_penalty(x, 1.0, order=order)
    for scale in (0.0, -2.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match="scale"):
            fit.motion_penalty(x, 1.0, scale=scale)
    with pytest.raises(ValueError, match=r"float32 \[F,V,3\]"):
        fit.motion_penalty(torch.zeros(4, 5, 2), 1.0)
    for ids in (torch.arange(4, dtype=torch.int32), torch.arange(3), [0, 1, 2, 3], torch.arange(4).reshape(2, 2)):
        with pytest.raises(ValueError, match="int64 tensor"):
            fit.motion_penalty(x, 1.0, frame_ids=ids)
    for ids in ([0, 1, 1, 2], [0, 2, 1, 3], [3, 2, 1, 0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            fit.motion_penalty(x, 1.0, frame_ids=torch.tensor(ids))
    for w in (torch.ones(4), torch.ones(5, dtype=torch.float64), [1.0] * 5):
        with pytest.raises(ValueError, match="vertex_weights must be a float32 tensor"):
            fit.motion_penalty(x, 1.0, vertex_weights=w)
    for w in (torch.tensor([1, 1, -1, 1, 1.0]), torch.tensor([1, 1, float('inf'), 1, 1.0])):
        with pytest.raises(ValueError, match="finite and not negative"):
            fit.motion_penalty(x, 1.0, vertex_weights=w)
    with pytest.raises(RuntimeError, match="GPU only"):                   # valid arguments: no CPU fallback
        fit.motion_penalty(x, 1.0, frame_ids=torch.tensor([0, 1, 2, 4]), scale=0.5, vertex_weights=torch.ones(5))


def _lib_loaded():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def test_the_library_exports_the_entry_and_abi_stays_16():
    _lib, lib = _lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert "fpcdr_motion_penalty" in _lib.SYMBOLS and hasattr(lib, "fpcdr_motion_penalty")
    assert "fpcdr_motion_penalty" in open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    if os.path.exists(_lib.TWOCALL_LIB_PATH):
        assert hasattr(ctypes.CDLL(_lib.TWOCALL_LIB_PATH), "fpcdr_motion_penalty")


def test_bad_arguments_give_an_error_code_before_any_launch():
    """Nulls, sizes, a misaligned acc, an order outside {1, 2}, a negative or non-finite inv_c: the checks come before the first HIP
    call, so this runs without a GPU on host memory the entry never touches."""
    _lib, lib = _lib_loaded()
    F, V = 3, 5
    fb = lambda n: (ctypes.c_float * (n + 4))()
    x, per, out, gx, vw = fb(F * V * 3), fb(F), fb(1), fb(F * V * 3), fb(V)
    ft = (ctypes.c_int64 * F)(0, 1, 2)
    acc = (ctypes.c_double * (F + 2))()
    P = lambda b: ctypes.cast(b, ctypes.c_void_p)

    def args(**over):
        kw = dict(x=P(x), frame_t=P(ft), vertex_w=P(vw), inv_c=0.0, order=2, grad_x=P(gx), acc=P(acc), per=P(per), out=P(out), weight=1.0,
                  F=F, V=V)
        kw.update(over)
        return [kw[k] for k in ('x', 'frame_t', 'vertex_w', 'inv_c', 'order', 'grad_x', 'acc', 'per', 'out', 'weight', 'F', 'V')] + [None]

    bad = [dict(x=None), dict(acc=None), dict(per=None), dict(out=None), dict(acc=ctypes.c_void_p(ctypes.addressof(acc) + 4)),
           dict(F=0), dict(F=-1), dict(F=65536), dict(V=0), dict(V=-3), dict(order=0), dict(order=3), dict(order=-1),
           dict(inv_c=-1.0), dict(inv_c=float('inf')), dict(inv_c=float('nan'))]
    for i, over in enumerate(bad):
        assert lib.fpcdr_motion_penalty(*args(**over)) != 0, i
        assert b"fpcdr_motion_penalty" in lib.fpcdr_last_error()
    assert all(v == 0.0 for v in acc)


def test_motion_kernels_have_no_private_segment():
    """read from the built object (tests/codeobj.py).  The five frames of a lane and its three stencils are indexed by
    compile-time constants only."""
    import codeobj
    recs = codeobj.kernels("mesh_reg.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    motion = {name: private for name, private, _ in recs if "k_motion" in name}
    assert len(motion) == 2 and all(p == 0 for p in motion.values()), motion       # k_motion_penalty<1> and <2>

"""CPU: the statement of the expression solve (tests/expr_ref.py) checked against torch.autograd and the Landmark rule's own statement,
the float64 solver's guarantees on tests/expr_cases.py, the header and the binding, the entry's argument checks on host memory, the
built kernels' private segment and LDS, and FitConfig's new options.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import expr_cases as EC
import expr_ref as ER
import landmark_cases as LC
import landmark_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solve_args(cs, ridge=0.0):
    ic = 0.0 if cs['scale'] is None else 1.0 / cs['scale']
    return (cs['x'], cs['mvp'], cs['basis'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], cs['w_in'], EC.H, EC.W, ic, ridge)


@pytest.mark.parametrize("robust", [False, True])
def test_normal_equations_are_the_jacobian_of_the_residuals(robust):
    """(g_u^T A_l, g_v^T A_l) of expr_ref.normal against torch.autograd.functional.jacobian of the residuals with respect to the weights,
    float64, at weights away from those of the meshes; H and g are its weighted sums, E the robust cost: to 1e-9 relative."""
    cs = EC.solve_case(24, 2, 10, robust)
    g = torch.Generator().manual_seed(5)
    wts = cs['w_in'].double() + 0.7 * torch.randn(3, 10, generator=g, dtype=torch.float64)
    a = _solve_args(cs)
    ref = ER.normal(*a[:7], wts, cs['w_in'], *a[8:11])
    F, Nc, L = ref['live'].shape
    obs, mvp, ic = cs['obs'].double().reshape(F, Nc, L, 3), cs['mvp'].double().reshape(F, Nc, 4, 4), a[10]
    A = ref['A']
    vt, br = torch.as_tensor(np.asarray(cs['vtx'], dtype=np.int64)), torch.as_tensor(cs['bary']).double()
    ti = torch.tril_indices(10, 10)
    for f in range(F):
        live = ref['live'][f]
        pts = sum(br[k][:, None] * cs['x'][f].double()[vt[k]] for k in range(3))
        o = torch.where(live[..., None], obs[f], torch.zeros((), dtype=torch.float64))
        res = lambda w: ER.residuals_plain(w, cs['w_in'][f].double(), pts, A, mvp[f], o, EC.H, EC.W)
        J = torch.autograd.functional.jacobian(res, wts[f])                                            # [Nc,L,2,Kb]
        Jr = torch.einsum('clra,lak->clrk', ref['G'][f], A)
        r0 = res(wts[f])
        if bool(live.any()):
            assert float((J[live] - Jr[live]).abs().max()) <= 1e-9 * float(Jr[live].abs().max())
            assert float((r0[live] - ref['res'][f][live]).abs().max()) <= 1e-9 * float(r0[live].abs().max())
        s = (r0 ** 2).sum(-1)
        d = torch.ones_like(s) if ic == 0.0 else 1.0 / torch.sqrt(1.0 + s * ic * ic)
        rho = s if ic == 0.0 else 2.0 / (ic * ic) * (torch.sqrt(1.0 + s * ic * ic) - 1.0)              # the textbook form
        zero = torch.zeros((), dtype=torch.float64)
        wgt = torch.where(live, obs[f][..., 2] * d, zero)
        Jz, rz = torch.where(live[..., None, None], J, zero), torch.where(live[..., None], r0, zero)
        Hm = torch.einsum('cl,clri,clrj->ij', wgt, Jz, Jz)
        gv = torch.einsum('cl,clri,clr->i', wgt, Jz, rz)
        E = torch.where(live, obs[f][..., 2] * rho, zero).sum()
        Hp = Hm[ti[0], ti[1]]
        assert float((Hp - ref['H'][0][f]).abs().max()) <= 1e-9 * float(Hp.abs().max())
        assert float((gv - ref['g'][0][f]).abs().max()) <= 1e-9 * float(gv.abs().max())
        assert abs(float(E) - float(ref['E'][0][f])) <= 1e-9 * max(float(E), 1e-300)
        assert bool((ref['H'][1][f] >= ref['H'][0][f].abs()).all()) and bool((ref['g'][1][f] >= ref['g'][0][f].abs()).all())
        assert int(ref['n'][f]) == int(live.sum())


@pytest.mark.parametrize("use_w,use_c", [(False, False), (True, True)])
def test_at_the_input_weights_an_entry_is_the_landmark_rules(use_w, use_c):
    """At w' = w_in: E is landmark_ref.landmark's sum (float64, 1e-12), and in float32 -- the kernel's order -- the residuals and the
    live entries are landmark_ref's float32 statement's bit for bit, NaN for NaN."""
    cs = EC.normal_case(3, 2, 64, 23, use_w, use_c)
    ic = 0.0 if cs['scale'] is None else float(np.float32(1.0 / cs['scale']))
    a = (cs['x'], cs['mvp'], cs['basis'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], cs['w_in'], cs['w_in'], LC.H, LC.W, ic)
    for dtype in (torch.float64, torch.float32):
        r = ER.normal(*a, dtype=dtype)
        lr = LR.landmark(cs['x'], cs['mvp'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], 1.0, LC.H, LC.W, ic, dtype=dtype, grads=False)
        F, Nc, L = r['live'].shape
        assert torch.equal(r['live'].reshape(F * Nc, L), lr['live'])
        assert torch.equal(torch.nan_to_num(r['res'].reshape(F * Nc, L, 2), nan=-7.0), torch.nan_to_num(lr['res'][0], nan=-7.0))
        if dtype == torch.float64:
            E = lr['per'][0] * (Nc * L)
            assert float((r['E'][0] - E).abs().max()) <= 1e-12 * float(E.abs().max())


@pytest.mark.parametrize("L,Nc,Kb", EC.SHAPES)
def test_float64_solver_never_raises_the_cost_and_leaves_what_it_must(L, Nc, Kb):
    for robust in (False, True):
        for ridge in (0.0, EC.RIDGE):
            cs = EC.solve_case(L, Nc, Kb, robust)
            a = _solve_args(cs, ridge)
            w, info, trace = ER.solve(*a)
            still, dead = cs['still'], cs['dead']
            assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(info).all())
            assert bool((info[:, 1] <= info[:, 0]).all())
            assert len(trace[still]) == 0 and torch.equal(w[still], cs['w_in'][still]) and float(info[still, 2]) == 2.0
            for f in range(3):
                c = float(info[f, 0])
                for c0, c1, n0, n1, keep in trace[f]:
                    assert c0 == c
                    if keep:
                        assert c1 < c0 and n1 >= n0
                        c = c1
                if f != still:
                    assert float(info[f, 3]) >= 1 and float(info[f, 1]) < float(info[f, 0]) and float(info[f, 2]) == Nc * L
            if ridge == 0.0:      # M_kk == 0: the weight stays bit for bit
                assert torch.equal(w[:, dead], cs['w_in'][:, dead])
            else:                 # ... with a ridge it is pulled towards neutral
                moved = [f for f in range(3) if f != still]
                assert bool((w[moved, dead].abs() < EC.DEAD_START).all())
            if not robust and ridge == 0.0:      # exact data: the truth comes back wherever the landmarks see it
                seen = [k for k in range(Kb) if k != dead]
                x_err = float((cs['x_true'][[0, 2]] - (cs['x'][[0, 2]].double() + ((w[[0, 2]] - cs['w_in'][[0, 2]]).double() @ cs['basis'].double().t()).reshape(2, -1, 3))
                               )[:, np.unique(np.asarray(cs['vtx']))].abs().max())
                print(f"EXPR ref L{L}/Nc{Nc}/Kb{Kb}: cost {info[0, 0]:.3e} -> {info[0, 1]:.3e}, landmark vertex error {x_err:.2e} units, "
                      f"weights off by {float((w[[0, 2]][:, seen].double() - cs['w_true'][[0, 2]][:, seen]).abs().max()):.2e}")
                assert x_err <= 1e-3


def test_a_rejected_trial_and_the_dead_select():
    """expr_ref.trial: a matrix that is not positive definite is a rejected trial; a dead weight's step is exactly 0."""
    Hp = np.array([1.0, 2.0, 1.0])                                                                     # [[1, 2], [2, 1]]
    assert ER.trial(Hp, np.array([1.0, 1.0]), 1e-3, 0.0, np.zeros(2, np.float32)) is None
    Hp = np.array([2.0, 0.0, 0.0])                                                                     # weight 1 untouched by any landmark
    w = np.array([0.5, 0.3], np.float32)
    out = ER.trial(Hp, np.array([1.0, 0.0]), 0.0, 0.0, w)
    assert out[1] == w[1] and abs(out[0] - 0.0) < 1e-7
    assert ER.trial(Hp, np.array([float('nan'), 0.0]), 0.0, 0.0, w) is None


def _lib_loaded():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def test_the_entry_is_declared_bound_and_exported_and_abi_stays_16():
    _lib, lib = _lib_loaded()
    text = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    m = re.search(r"int fpcdr_landmark_expr\((.*?)\);", text, re.S)
    assert m is not None
    n_args = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    assert n_args == len(_lib.SYMBOLS["fpcdr_landmark_expr"][1]) == 24
    assert "size_t fpcdr_landmark_expr_scratch_bytes(int32_t F, int32_t L, int32_t Kb);" in text
    assert "#define FPCDR_ABI_VERSION 16" in text and _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert hasattr(lib, "fpcdr_landmark_expr") and "fpcdr_landmark_expr" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "landmark_expr.hip" in open(os.path.join(ROOT, "fpc_diffrend_amd", "csrc", "Makefile")).read()
    for F, L, Kb in ((1, 1, 1), (32, 68, 150), (1024, 512, 160)):      # the landmark basis, shared by the frames: 3 L Kb floats
        assert lib.fpcdr_landmark_expr_scratch_bytes(F, L, Kb) == 3 * L * Kb * 4
    assert lib.fpcdr_landmark_expr_scratch_bytes(1, 0, 5) == 0
    if os.path.exists(_lib.TWOCALL_LIB_PATH):
        assert hasattr(ctypes.CDLL(_lib.TWOCALL_LIB_PATH), "fpcdr_landmark_expr")


def test_bad_arguments_give_an_error_code_before_any_launch():
    """Nulls, sizes, the two caps, alignment, inv_c / ridge / lambda0 out of range, a negative iters, a missing or short scratch: the
    checks come before the first HIP call, so this runs without a GPU on host memory the entry never touches."""
    _lib, lib = _lib_loaded()
    F, Nc, V, L, Kb = 2, 3, 5, 4, 3
    fb = lambda n: (ctypes.c_float * (n + 4))()
    ib = lambda n: (ctypes.c_int32 * (n + 4))()
    bufs = dict(x=fb(F * V * 3), mvp=fb(F * Nc * 16), basis=fb(3 * V * Kb), lm_vtx=ib(3 * L), lm_bary=fb(3 * L), lm_w=fb(L), obs=fb(F * Nc * L * 3),
                w=fb(F * Kb), info=fb(F * 4), scratch=fb(3 * L * Kb))
    nrm = (ctypes.c_double * (F * (Kb * (Kb + 1) // 2 + Kb + 2) + 2))()
    P = lambda b: ctypes.cast(b, ctypes.c_void_p)
    off = lambda b, n: ctypes.c_void_p(ctypes.addressof(b) + n)
    order = ('x', 'mvp', 'basis', 'lm_vtx', 'lm_bary', 'lm_w', 'obs', 'w', 'inv_c', 'ridge', 'width', 'height', 'iters', 'lambda0', 'info',
             'normal_out', 'scratch', 'scratch_bytes', 'F', 'Nc', 'V', 'L', 'Kb')

    def args(**over):
        kw = {k: P(v) for k, v in bufs.items()}
        kw.update(inv_c=0.0, ridge=0.0, width=8, height=6, iters=3, lambda0=1e-3, normal_out=P(nrm), scratch_bytes=3 * L * Kb * 4, F=F, Nc=Nc, V=V,
                  L=L, Kb=Kb)
        kw.update(over)
        return [kw[k] for k in order] + [None]

    bad = [dict(x=None), dict(mvp=None), dict(basis=None), dict(lm_vtx=None), dict(lm_bary=None), dict(obs=None), dict(w=None), dict(info=None),
           dict(scratch=None), dict(scratch_bytes=3 * L * Kb * 4 - 1), dict(scratch_bytes=0),
           dict(F=0), dict(Nc=0), dict(V=0), dict(L=0), dict(Kb=0), dict(L=-2), dict(Kb=161), dict(L=513), dict(Kb=161, L=513),
           dict(width=0), dict(height=-1), dict(iters=-1), dict(inv_c=-1.0), dict(inv_c=float('inf')), dict(inv_c=float('nan')),
           dict(ridge=-1e-3), dict(ridge=float('inf')), dict(ridge=float('nan')), dict(lambda0=0.0), dict(lambda0=-1.0), dict(lambda0=float('nan')),
           dict(lambda0=float('inf')), dict(x=off(bufs['x'], 2)), dict(w=off(bufs['w'], 1)), dict(lm_vtx=off(bufs['lm_vtx'], 2)),
           dict(info=off(bufs['info'], 3)), dict(scratch=off(bufs['scratch'], 2)), dict(normal_out=off(nrm, 4))]
    for i, over in enumerate(bad):
        assert lib.fpcdr_landmark_expr(*args(**over)) != 0, (i, over)
        assert b"fpcdr_landmark_expr" in lib.fpcdr_last_error()
    assert all(v == 0.0 for v in bufs['w']) and all(v == 0.0 for v in nrm) and all(v == 0.0 for v in bufs['scratch'])


def test_expr_kernels_have_no_private_segment():
    """read from the built object (tests/codeobj.py).  LDS of k_landmark_expr<KB, LB>: the float64 packed triangle
    KB (KB + 1) / 2, four float64 vectors of KB (right-hand side, y, delta, the factor's diagonal), two buffers of LB x 9 float32 (S_l and
    s_l of the best and of the trial weights), four float32 vectors of KB (the best, trial and input weights, the trial's offset), KB
    flags, the eight partials of four waves, (E, n) and one flag: 15 148 bytes for (32, 128) and 148 268 for (160, 512), which the
    compiler lays out in 15 152 and 148 272."""
    import codeobj
    recs = codeobj.kernels("landmark_expr.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    own = {name: (private, lds) for name, private, lds in recs if "k_landmark_expr" in name or "k_expr_basis" in name}
    assert len(own) == 3 and all(p == 0 for p, _ in own.values()), own
    size = lambda KB, LB: 8 * (KB * (KB + 1) // 2) + 4 * 8 * KB + 2 * LB * 9 * 4 + 4 * 4 * KB + 4 * KB + 32 + 8 + 4
    assert (size(32, 128), size(160, 512)) == (15148, 148268)
    lds = sorted(l for _, l in own.values())
    assert lds == [0, 15152, 148272], own
    assert 148272 <= 160 * 1024


def test_the_landmark_entry_is_shared_not_copied():
    csrc = os.path.join(ROOT, "fpc_diffrend_amd", "csrc")
    marks = ("lm_vtx[(size_t)L + l]", "sqrtf(1.0f + (zu * zu")
    text = open(os.path.join(csrc, "landmark_expr.hip")).read()
    assert '#include "landmark_entry.h"' in text and not any(m in text for m in marks)
    assert "landmark_entry(" in text and "landmark_residual(" in text and "landmark_corners(" in text
    header = open(os.path.join(csrc, "landmark_entry.h")).read()
    assert [header.count(m) for m in marks] == [1, 1]


def test_fitconfig_refuses_bad_expression_options():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert (cfg.init_expression, cfg.init_expression_iters, cfg.init_expression_ridge, cfg.init_landmark_rounds) == ('keep', 20, 0.0, 1)
    fit.FitConfig(init_expression='landmarks', init_expression_iters=0, init_expression_ridge=0.5, init_landmark_rounds=3)
    fit.FitConfig(init_expression='landmarks', mode='combined')
    for kw, match in ((dict(init_expression='auto'), "init_expression"), (dict(init_expression=None), "init_expression"),
                      (dict(init_expression_iters=-1), "init_expression_iters"), (dict(init_expression_iters=2.5), "init_expression_iters"),
                      (dict(init_expression_iters=True), "init_expression_iters"), (dict(init_expression_ridge=-0.1), "init_expression_ridge"),
                      (dict(init_expression_ridge=float('nan')), "init_expression_ridge"), (dict(init_expression_ridge=float('inf')), "init_expression_ridge"),
                      (dict(init_landmark_rounds=0), "init_landmark_rounds"), (dict(init_landmark_rounds=1.5), "init_landmark_rounds"),
                      (dict(init_expression='landmarks', mode='free'), "mode='free'")):
        with pytest.raises(ValueError, match=match):
            fit.FitConfig(**kw)
    assert fit.solve_expression is __import__('fpc_diffrend_amd').landmarks.solve_expression and hasattr(fit.Fitter, "solve_expression")


def test_solve_expression_shares_the_entry_checks_and_has_its_own():
    """CPU tensors: every check comes before any launch."""
    from fpc_diffrend_amd import fit
    lms = fit.LandmarkSet([{'vertex': 0}, {'face': 0, 'bary': (0.2, 0.3, 0.5)}], 4, np.array([[0, 1, 2], [2, 1, 3]]), 'cpu')
    ok = dict(verts=torch.zeros(1, 4, 3), mvp=torch.eye(4).reshape(1, 4, 4), basis=torch.zeros(12, 3), lms=lms, obs=torch.zeros(1, 2, 3),
              w=torch.zeros(1, 3), resolution=(8, 8))
    for over, why in ((dict(lms=None), "LandmarkSet"), (dict(verts=torch.zeros(1, 5, 3)), "verts must hold"), (dict(obs=torch.zeros(1, 3, 3)), "obs must be"),
                      (dict(resolution=(0, 8)), "both positive"), (dict(mvp=torch.eye(4)), "mvp must be"), (dict(basis=torch.zeros(11, 3)), "basis must be"),
                      (dict(basis=torch.zeros(12, 161), w=torch.zeros(1, 161)), "at most 160"), (dict(w=torch.zeros(1, 4)), "w must be"),
                      (dict(w=torch.zeros(1, 3).double()), "w must be"), (dict(iters=-1), "iters"), (dict(iters=1.5), "iters"), (dict(damping=0.0), "damping"),
                      (dict(ridge=-1.0), "ridge"), (dict(ridge=float('nan')), "ridge"), (dict(scale=-2.0), "scale"),
                      (dict(normal_out=torch.zeros(1, 11)), "normal_out"), (dict(normal_out=torch.zeros(1, 10, dtype=torch.float64)), "normal_out")):
        with pytest.raises(ValueError, match=why) as e:
            fit.solve_expression(**{**ok, **over})
        assert str(e.value).startswith("solve_expression: ") or "scale" in why, (over, str(e.value))

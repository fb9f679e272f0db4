"""CPU: the float64 statement of the pose solve (tests/pose_ref.py) checked against torch.autograd and against what it is for, the
conditions tests/test_gpu_pose.py puts on its inputs, the header, and FitConfig's new options.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import pose_cases as PC
import pose_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def _args(cs, q=None, t=None):
    ic = 0.0 if cs['scale'] is None else 1.0 / cs['scale']
    return (cs['x'], cs['proj'], cs['base'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], cs['q'] if q is None else q, cs['t'] if t is None else t,
            PC.H, PC.W, ic)


@pytest.mark.parametrize("robust", [False, True])
def test_normal_equations_are_the_jacobian_of_the_residuals(robust):
    """J of pose_ref.normal against torch.autograd.functional.jacobian of the residuals with respect to a left-multiplied rotation
    increment and a translation increment, float64; A and b are its weighted sums."""
    cs = PC.solve_case(64, 2, 0, robust)
    q = torch.tensor(np.stack([PC.pose_of(12.0, 3.0, 5 + f)[0] for f in range(3)])) * 1.3      # (off the unit sphere: the rule normalises)
    t = torch.tensor(np.stack([PC.pose_of(12.0, 3.0, 5 + f)[1] for f in range(3)]))
    a = _args(cs, q, t)
    ref = PR.normal(*a)
    F, Nc, L = ref['live'].shape
    obs = cs['obs'].double().reshape(F, Nc, L, 3)
    ic = a[-1]
    for f in range(F):
        live = ref['live'][f]
        qf = q[f] / q[f].norm()

        def res(delta):
            dq = torch.cat([0.5 * delta[:3], torch.ones(1, dtype=torch.float64)])      # exp(delta / 2) to first order
            qq = torch.stack([dq[3] * qf[0] + dq[0] * qf[3] + dq[1] * qf[2] - dq[2] * qf[1], dq[3] * qf[1] - dq[0] * qf[2] + dq[1] * qf[3] + dq[2] * qf[0],
                              dq[3] * qf[2] + dq[0] * qf[1] - dq[1] * qf[0] + dq[2] * qf[3], dq[3] * qf[3] - dq[0] * qf[0] - dq[1] * qf[1] - dq[2] * qf[2]])
            o = torch.where(live[..., None], obs[f], torch.zeros((), dtype=torch.float64))
            return PR.residuals_plain(qq, t[f] + delta[3:], ref['y'][f], cs['proj'].double(), o, PC.H, PC.W)

        J = torch.autograd.functional.jacobian(res, torch.zeros(6, dtype=torch.float64))       # [Nc,L,2,6]
        r0 = res(torch.zeros(6, dtype=torch.float64))
        Jl, Jr = J[live], ref['J'][f][live]
        assert float((Jl - Jr).abs().max()) <= 1e-9 * float(Jr.abs().max())
        assert float((r0[live] - ref['res'][f][live]).abs().max()) <= 1e-9 * float(r0[live].abs().max())
        s = (r0 ** 2).sum(-1)
        d = torch.ones_like(s) if ic == 0.0 else 1.0 / torch.sqrt(1.0 + s * ic * ic)
        rho = s if ic == 0.0 else 2.0 / (ic * ic) * (torch.sqrt(1.0 + s * ic * ic) - 1.0)      # the textbook form
        w = torch.where(live, obs[f][..., 2] * d, torch.zeros((), dtype=torch.float64))
        Jz = torch.where(live[..., None, None], J, torch.zeros((), dtype=torch.float64))
        rz = torch.where(live[..., None], r0, torch.zeros((), dtype=torch.float64))
        A = torch.einsum('cl,clki,clkj->ij', w, Jz, Jz)
        b = torch.einsum('cl,clki,clk->i', w, Jz, rz)
        E = torch.where(live, obs[f][..., 2] * rho, torch.zeros((), dtype=torch.float64)).sum()
        Ar = torch.stack([A[i, j] for i, j in PR.TRI])
        assert float((Ar - ref['A'][0][f]).abs().max()) <= 1e-9 * float(Ar.abs().max())
        assert float((b - ref['b'][0][f]).abs().max()) <= 1e-9 * float(b.abs().max())
        assert abs(float(E) - float(ref['E'][0][f])) <= 1e-9 * max(float(E), 1e-300)
        assert bool((ref['A'][1][f] >= ref['A'][0][f].abs()).all()) and bool((ref['b'][1][f] >= ref['b'][0][f].abs()).all())
        assert int(ref['n'][f]) == int(live.sum())


def _table_scene(cams, deg, units, n_lmk=40, noise=0.0, outliers=False, seed=0):
    """The README's setup: cfg1's mesh at 128 x 128, `cams`, landmarks on every thirteenth vertex, the truth turned deg degrees about
    (0.3, 0.9, 0.2) and moved `units` units along (6, -3, 4), the start at the identity."""
    import landmark_ref as LR
    from helpers import scene_cameras
    from fpc_diffrend_amd import scene
    sc = scene.make_scene(scene.MESH_1K, 10, 1, (128, 128), (256, 256, 1), 0)
    proj, base = scene_cameras(sc, cams)
    x = torch.tensor(sc.v_base).reshape(1, -1, 3).float()
    points = [{'vertex': v} for v in range(0, sc.n_vertices, 13)][:n_lmk]
    vtx, bary, _ = LR.tables(points, sc.n_vertices, sc.pos_idx)
    axis, d = np.array([0.3, 0.9, 0.2]), np.array([6.0, -3.0, 4.0])
    axis, d = axis / np.linalg.norm(axis), d / np.linalg.norm(d)
    h = math.radians(deg) / 2
    q_true = torch.tensor(np.concatenate([math.sin(h) * axis, [math.cos(h)]]))[None]
    t_true = torch.tensor(units * d)[None]
    L = len(points)
    zero = torch.zeros(len(cams), L, 3, dtype=torch.float64)
    zero[..., 2] = 1.0
    at = PR.normal(x, proj, base, vtx, bary, None, zero, q_true, t_true, 128, 128)
    obs = torch.zeros(len(cams), L, 3, dtype=torch.float64)
    obs[..., :2], obs[..., 2] = at['res'][0], at['live'][0].double()
    obs = torch.nan_to_num(obs)
    g = torch.Generator().manual_seed(seed)
    if noise:
        obs[..., :2] += noise * torch.randn(len(cams), L, 2, generator=g, dtype=torch.float64)
    if outliers:
        obs[:, ::6, 0] += 30.0
    q0 = torch.tensor([[0.0, 0.0, 0.0, 1.0]])
    return (x, proj, base, vtx, bary, None, obs.float(), q0, torch.zeros(1, 3), 128, 128), q_true, t_true


@pytest.mark.parametrize("cams,deg,units", [((0, 4), 25.0, math.sqrt(61.0)), ((4,), 25.0, 8.0), ((0, 4), 60.0, 15.0), (tuple(range(9)), 60.0, 15.0),
                                            (tuple(range(9)), 40.0, 11.0)])
def test_solver_recovers_the_truth(cams, deg, units):
    a, q_true, t_true = _table_scene(cams, deg, units)
    start = PR.mean_residual(*a[:7], a[7], a[8], 128, 128)
    q, t, info, trace = PR.solve(*a)
    end = PR.mean_residual(*a[:7], q, t, 128, 128)
    print(f"POSE ref cams={cams} {deg:g} deg / {units:.2f} units: start {start:.1f} px, after {len(trace[0])} trials "
          f"({int(info[0, 3])} accepted) {end:.2e} px")
    assert start > 50.0 and end < 1e-3
    dq, dt = PC.pose_distance(q, t, q_true.float(), t_true.float())
    assert dq <= 1e-5 and dt <= 1e-3
    assert float(info[0, 2]) == len(cams) * 40


def test_with_noise_and_outliers_a_charbonnier_scale_converges():
    a, q_true, t_true = _table_scene((0, 4), 25.0, 8.0, noise=1.0, outliers=True)
    q, t, info, _ = PR.solve(*a[:11], 1.0 / 2.0)
    dq, dt = PC.pose_distance(q, t, q_true.float(), t_true.float())
    print(f"POSE ref noise + outliers: dq {dq:.2e} dt {dt:.2e} accepted {int(info[0, 3])}")
    assert dq <= 5e-3 and dt <= 1.0


def test_one_camera_far_off_keeps_its_live_count():
    """One camera with the truth 60 degrees / 15 units away: without the guard a trial 'wins' by throwing every point behind the camera,
    where E = 0.  The solver never ends there."""
    a, _, _ = _table_scene((4,), 60.0, 15.0)
    q, t, info, trace = PR.solve(*a)
    n0 = int(PR.normal(*a)['n'][0])
    assert int(info[0, 2]) >= n0 and n0 == 40
    assert float(info[0, 1]) > 0.0 or int(info[0, 2]) == 40
    assert all(n2 is None or n2 >= n or not keep for _, _, n, n2, keep in trace[0])
    r = PR.normal(*a[:7], q, t, 128, 128)
    assert int(r['n'][0]) == 40 and bool(torch.isfinite(r['res']).all())


def test_translation_alone_leaves_the_quaternion():
    a, _, _ = _table_scene((0, 4), 25.0, 8.0)
    q, t, info, _ = PR.solve(*a, rotate=False)
    assert torch.equal(q, a[7]) and float(info[0, 1]) < float(info[0, 0]) and float(info[0, 3]) > 0
    end = PR.mean_residual(*a[:7], q, t, 128, 128)
    assert end < 0.2 * PR.mean_residual(*a[:7], a[7], a[8], 128, 128)


@pytest.mark.parametrize("L,Nc", [(L, Nc) for L in (6, 64, 130) for Nc in (1, 2, 9)])
def test_the_gpu_cases_decide_their_trials_by_a_margin(L, Nc):
    """A condition on the inputs of tests/test_gpu_pose.py: before convergence -- while the cost a trial starts from is more than 1 %
    above the cost the solver ends at, and above the cost of a pose 4 u away -- every trial of the float64 solver changes E by more than
    1e-3 E, so that float32 takes the same branch.  Every moved frame is solved, and the frame with two live entries is not touched."""
    for offset in (0, 1):
        for robust in (False, True):
            cs = PC.solve_case(L, Nc, offset, robust)
            a = _args(cs)
            q, t, info, trace = PR.solve(*a)
            floor = PC.cost_floor(PR.normal(*a[:7], q, t, *a[9:]), t)
            still = cs['still']
            assert len(trace[still]) == 0 and torch.equal(q[still], cs['q'][still]) and float(info[still, 2]) == 2.0
            for f in range(3):
                if f == still:
                    continue
                e_end = float(info[f, 1])
                assert float(info[f, 3]) >= 3 and e_end < 0.5 * float(info[f, 0]), (L, Nc, offset, robust, f, info[f])
                assert float(info[f, 2]) == Nc * L
                for e, e2, n, n2, keep in trace[f]:
                    if e > 1.01 * e_end and e > float(floor[f]):
                        assert e2 is not None and abs(e2 - e) > 1e-3 * e, (L, Nc, offset, robust, f, e, e2)
            ref = PR.mean_residual(*a[:7], q, t, PC.H, PC.W)
            assert math.isfinite(ref)


def test_the_restated_sine_and_cosine_are_the_librarys():
    """pose_ref.sincos -- the kernel's pose_sincos operation for operation -- against math.sin / math.cos: 2^6 roundings of 2^-53 (six
    doublings, each at most doubles the error; 1.1e-15 measured) up to the half angle of a full turn, exact at 0, and a unit vector to 1e-12 however far a wild step goes."""
    assert PR.sincos(0.0) == (0.0, 1.0)
    for h in list(np.linspace(0.0, math.pi, 2001)) + [1e-9, 0.0625, 0.06250000001, 1.0, 2.5]:
        s, c = PR.sincos(float(h))
        assert abs(s - math.sin(h)) <= 64 * 2.0 ** -53 and abs(c - math.cos(h)) <= 64 * 2.0 ** -53, (h, s - math.sin(h), c - math.cos(h))
    for h in (10.0, 1e3, 1e6):
        s, c = PR.sincos(h)
        assert abs(s * s + c * c - 1.0) <= 1e-9 and math.isfinite(s)


def test_header_declares_the_entry_and_the_binding_matches():
    text = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    m = re.search(r"int fpcdr_landmark_pose\((.*?)\);", text, re.S)
    assert m is not None
    n_args = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    from fpc_diffrend_amd import _lib
    assert n_args == len(_lib.SYMBOLS["fpcdr_landmark_pose"][1]) == 22
    assert "#define FPCDR_ABI_VERSION 16" in text and _lib.ABI_VERSION == 16
    assert "landmark_pose.hip" in open(os.path.join(ROOT, "fpc_diffrend_amd", "csrc", "Makefile")).read()


def test_pose_kernel_has_no_private_segment():
    """read from the built object (tests/codeobj.py).  LDS: the 29 partial sums of four waves, the new and the current
    sums, the trial and the best pose, two flags -- 768 bytes, which the compiler lays out in 784."""
    import codeobj
    recs = codeobj.kernels("landmark_pose.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    own = {name: (private, lds) for name, private, lds in recs if "k_landmark_pose" in name}
    assert len(own) == 1 and list(own.values()) == [(0, 784)], own


def test_the_landmark_entry_is_shared_not_copied():
    """One statement of an entry's table read and of its robust pair, in the header that the term and the solve both include."""
    csrc = os.path.join(ROOT, "fpc_diffrend_amd", "csrc")
    marks = ("lm_vtx[(size_t)L + l]", "sqrtf(1.0f + (zu * zu")
    for src in ("landmark.hip", "landmark_pose.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "landmark_entry.h"' in text and not any(m in text for m in marks), src
    header = open(os.path.join(csrc, "landmark_entry.h")).read()
    assert [header.count(m) for m in marks] == [1, 1]
    assert "landmark_entry.h" in open(os.path.join(csrc, "Makefile")).read()


def test_fitconfig_refuses_bad_pose_options():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert (cfg.init_pose, cfg.init_pose_iters, cfg.init_pose_rotation, cfg.quat_renorm) == ('keep', 20, True, 'tensor')
    fit.FitConfig(init_pose='landmarks', quat_renorm='rows', init_pose_iters=0, init_pose_rotation=False)
    for kw, match in ((dict(init_pose='auto'), "init_pose"), (dict(quat_renorm='row'), "quat_renorm"), (dict(quat_renorm=None), "quat_renorm"),
                      (dict(init_pose_iters=-1), "init_pose_iters"), (dict(init_pose_iters=2.5), "init_pose_iters"),
                      (dict(init_pose_iters=True), "init_pose_iters"), (dict(init_pose_rotation=1), "init_pose_rotation")):
        with pytest.raises(ValueError, match=match):
            fit.FitConfig(**kw)
    assert fit.solve_pose is not None and hasattr(fit.Fitter, "align_to_landmarks")

"""GPU: the per-frame pose solve from the landmarks (csrc/landmark_pose.hip k_landmark_pose; fpcdr_landmark_pose, fit.solve_pose,
Fitter.align_to_landmarks, FitConfig.init_pose / quat_renorm) against the float64 statement tests/pose_ref.py: the sums of a pass entry
by entry, the solved poses, and inside a Fitter.

Normal equations (iters = 0, normal_out): the convention is tests/test_gpu_landmark.py's -- the error of an entry in units of u = 2^-24
of its scale S (tests/pose_ref.py's algebra), the bar e <= 8 e32 + 4 with e32 the float32 statement on the CPU against the same float64,
entries without a term exactly 0 and counted.  Inputs: landmark_cases.case under pose_cases.normal_case's cameras and poses, L in {1, 63,
64, 65, 130}, Nc in {1, 2, 9}, F in {1, 3}, V in {3, 257}, with and without weights and a scale, on the 72 x 96 raster.  Every line is
printed as "POSE case name e_gpu e32 bound" (pytest -s).

Solve: pose_cases.solve_case, L in {6, 64, 130}, Nc in {1, 2, 9}, F = 3 with one frame of two live entries, the truth 25 degrees / 8 units
and 40 degrees / 11 units from the identity start, L2 and Charbonnier (c = 2 px, 1 px of noise, every sixth detection 30 px off).  The
distance of the GPU's (q, t) from the float64 solver's is held to 8 x the float32 statement's distance plus 4 u of the scale (1 for q,
max(|t|, |y|) for t): the factor covers another order of summation, the floor the case where float32 lands exactly.  E_out is held to
(1 + 1e-4) x float64's (where that is 0: the float32 statement's).  Exact: E_out <= E_in and the live count not smaller per frame,
|q| = 1 within 2 u, two runs bit-identical, NaN-prefilled neighbours of every output untouched, rotation = 0 leaves q bit-identical, the
frame with two live entries comes back bit for bit.

tests/pose_ref.py in float32 is the kernel operation for operation: an entry in the kernel's order, the sums in the kernel's order
(wave_sum_dpp is a balanced tree over neighbouring lanes), a correctly rounded root, the damping as the float32 the entry is handed, the
6 x 6 factorisation by plain loops in the unrolled code's order, and the sine and cosine of the quaternion update restated from +, -, *
(pose_sincos in the kernel, pose_ref.sincos here: a library's sine differs from another's in the last place, and the 6 x 6 systems, which
carry the lever arm |y| of about 300 units, turn a last place into a float32 ulp of the pose).  Every other float64 operation of the
trial is IEEE's on both sides.  So the float32 statement takes the kernel's branches, and the comparison with float64 measures float32,
not which of two draws of rounding noise first rejects a step.

Measured on an MI355X (the whole file: 93 tests in 13.1 s):

  normal equations   120 cases   max e_gpu A 1.67  b 0.35  E 0.02  (e32 the same; bit-identical to the float32 statement in 120 of 120)
  solved poses       36 cases    (q, t, info) bit-identical to the float32 statement after every number of trials from 1 to 20 in 36 of
                                 36; distance from float64: L2 dq <= 1.8e-7, dt <= 6.1e-5; Charbonnier dq <= 8.2e-5, dt <= 2.4e-2
                                 (L6/Nc1/25deg: six points, one camera, one of them 30 px off; float64 accepts 20 trials there, float32
                                 15); the worst case is 0.125 of its bound, the float32 statement's own distance
  cost, Charbonnier  36 frames   E_out / float64 - 1 between -5.4e-7 and +8.8e-9
  cost, L2           36 frames   float64's E_out is 3.6e-12 .. 1.2e-7, never a literal 0: its trial poses are rounded to float32 as the
                                 kernel's are.  "Is 0" is therefore read as "below pose_cases.cost_floor", the cost of a pose 4 u away
                                 (1.8e-7 .. 1.2e-4 here), and E_out is held against the float32 statement's: equal in 36 of 36.  (E_out
                                 itself is 5 .. 60 times float64's figure: float32 cannot see a cost below its own rounding.)
  Fitter             align 249.9 px -> 1.75e-5 px, the poses the float32 statement's bit for bit (its mean residual in float64: 1.09e-5 px,
                     bound 1.48e-4 px), the same after three steps at the default learning rates; translation alone 249.9 -> 10.5 px;
                     graphed and eager losses equal to every digit printed (1.87597048 12.41031933 6.50502968 3.94877672 3.03876567
                     2.35734463 3.29257059)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fitstep_ref as R
import landmark_ref as LR
import pose_cases as PC
import pose_ref as PR

pytestmark = pytest.mark.gpu

U = R.U
WORST = {}
BITS = [0, 0]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(rows, cols):
    """A NaN-filled buffer [rows + 2, cols] and its inner view [rows, cols]: the rows around an output must stay NaN."""
    buf = torch.full((rows + 2, cols), float('nan'), dtype=torch.float32, device='cuda')
    return buf, buf[1:rows + 1]


def _untouched(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


def _call(d, inv_c, iters, rotation=1, lambda0=1e-3, normal=True):
    """fpcdr_landmark_pose on the device tensors d; q and t are copies inside NaN guards -> (q, t, info, normal_out or None)."""
    from fpc_diffrend_amd import _lib
    F, V = d['x'].shape[0], d['x'].shape[1]
    Nc, L = d['proj'].shape[0], d['obs'].shape[1]
    qb, q = _guarded(F, 4)
    tb, t = _guarded(F, 3)
    ib, info = _guarded(F, 4)
    nb, nrm = _guarded(F, 28) if normal else (None, None)
    q.copy_(d['q'])
    t.copy_(d['t'])
    _lib.call("fpcdr_landmark_pose", _ptr(d['x']), _ptr(d['proj']), _ptr(d['base']), _ptr(d['vtx']), _ptr(d['bary']), _ptr(d['w']), _ptr(d['obs']),
              _ptr(q), _ptr(t), float(inv_c), PC.W, PC.H, int(iters), int(rotation), float(lambda0), _ptr(info), _ptr(nrm), F, Nc, V, L, _stream())
    torch.cuda.synchronize()
    assert all(_untouched(b) for b in (qb, tb, ib) + ((nb,) if normal else ()))
    return q.clone(), t.clone(), info.clone(), (nrm.clone() if normal else None)


def _device(cs):
    from fpc_diffrend_amd import fit
    V = cs['x'].shape[1]
    lms = fit.LandmarkSet(cs['points'], V, cs['faces'], 'cuda')
    assert np.array_equal(lms.vtx.cpu().numpy(), cs['vtx'])
    d = dict(x=cs['x'].cuda(), proj=cs['proj'].cuda(), base=cs['base'].cuda(), obs=cs['obs'].cuda(), q=cs['q'].cuda(), t=cs['t'].cuda(),
             vtx=lms.vtx, bary=lms.bary, w=None if cs['w'] is None else cs['w'].cuda())
    return d, lms


def _report(case, name, e, e32, bound):
    print(f"POSE {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={bound:.1f}")
    w = WORST.setdefault(name, [0, 0.0, 0.0])
    w[0], w[1], w[2] = w[0] + 1, max(w[1], e), max(w[2], e32)


def long_sum(case, name, x, ref, x32):
    r, Sc = ref
    e, nz = R.measure(x, r, Sc)
    e32, nz32 = R.measure(x32, r, Sc)
    _report(case, name, e, e32, 8 * e32 + 4)
    assert nz == nz32 == int((Sc == 0).sum())
    assert e <= 8 * e32 + 4, (case, name, e, e32)
    return nz


def _normal_case(F, Nc, V, L, use_w, use_c):
    from fpc_diffrend_amd import fit
    case = f"F{F}/Nc{Nc}/V{V}/L{L}" + ('/w' if use_w else '') + ('/c' if use_c else '')
    cs = PC.normal_case(F, Nc, V, L, use_w, use_c)
    inv_c = fit.landmark_inv_scale(cs['scale'])
    a = (cs['x'], cs['proj'], cs['base'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], cs['q'], cs['t'], PC.H, PC.W, inv_c)
    ref, ref32 = PR.normal(*a), PR.normal(*a, dtype=torch.float32)
    assert torch.equal(ref['live'], ref32['live'])          # (nothing sits at the threshold)
    d, _ = _device(cs)
    q, t, info, nrm = _call(d, inv_c, 0)
    assert torch.equal(q, d['q']) and torch.equal(t, d['t'])                              # iters = 0 returns only the sums
    assert bool(torch.isfinite(nrm).all()) and bool(torch.isfinite(info).all())
    zeros = long_sum(case, 'A', nrm[:, :21], ref['A'], ref32['A'][0])
    zeros += long_sum(case, 'b', nrm[:, 21:27], ref['b'], ref32['b'][0])
    zeros += long_sum(case, 'E', nrm[:, 27], ref['E'], ref32['E'][0])
    # a frame without a live entry: 28 exact zeros; any other: one, A[t_x, t_y] -- the projections have no skew (P_01 = P_10 = 0) and
    # their row w no x or y (P_30 = P_31 = 0), so d u / d t_y = d v / d t_x = 0 and neither product of the entry has a term
    assert zeros == 28 * int((ref['n'] == 0).sum()) + int((ref['n'] > 0).sum()), (case, zeros, ref['n'])
    assert torch.equal(info[:, 0], nrm[:, 27]) and torch.equal(info[:, 1], nrm[:, 27])
    assert torch.equal(info[:, 2].cpu().long(), ref['n']) and float(info[:, 3].abs().max()) == 0.0
    same = torch.equal(nrm[:, :21].cpu(), ref32['A'][0]) and torch.equal(nrm[:, 21:27].cpu(), ref32['b'][0]) and torch.equal(nrm[:, 27].cpu(), ref32['E'][0])
    BITS[0], BITS[1] = BITS[0] + int(same), BITS[1] + 1      # (information: the float32 statement sums in the kernel's order)
    if not same:
        k = [int((nrm[:, a:b].cpu() != r).sum()) for a, b, r in ((0, 21, ref32['A'][0]), (21, 27, ref32['b'][0]), (27, 28, ref32['E'][0][:, None]))]
        print(f"POSE {case} differs from the float32 statement in {k} entries of A, b, E")
    again = _call(d, inv_c, 0)
    assert torch.equal(again[3], nrm) and torch.equal(again[2], info)
    none = _call(d, inv_c, 0, normal=False)
    assert none[3] is None and torch.equal(none[2], info)


@pytest.mark.parametrize("F,Nc", [(1, 1), (1, 2), (1, 9), (3, 1), (3, 2), (3, 9)])
def test_normal_equations_entry_by_entry_against_float64(F, Nc):
    k = 0
    for V in (3, 257):
        for L in (1, 63, 64, 65, 130):
            for use_w, use_c in (((False, False), (True, True)) if k % 2 == 0 else ((True, False), (False, True))):
                _normal_case(F, Nc, V, L, use_w, use_c)
            k += 1
    print("POSE maxima so far  " + "  ".join(f"{n}: {c} cases e_gpu {e:.2f} e32 {e32:.2f}" for n, (c, e, e32) in WORST.items())
          + f"  bit-identical to the float32 statement: {BITS[0]} of {BITS[1]} cases")


def _case_name(L, Nc, offset, robust):
    return f"L{L}/Nc{Nc}/{PC.OFFSETS[offset][0]:g}deg/" + ('charbonnier' if robust else 'l2')


@functools.lru_cache(maxsize=None)
def _solved(L, Nc, offset, robust):
    """One case solved by the float64 statement, the float32 statement and the kernel (20 trials): computed once, shared, left unchanged."""
    from fpc_diffrend_amd import fit
    cs = PC.solve_case(L, Nc, offset, robust)
    inv_c = fit.landmark_inv_scale(cs['scale'])
    a = (cs['x'], cs['proj'], cs['base'], cs['vtx'], cs['bary'], None, cs['obs'], cs['q'], cs['t'], PC.H, PC.W, inv_c)
    d, lms = _device(cs)
    return dict(cs=cs, inv_c=inv_c, a=a, d=d, lms=lms, f64=PR.solve(*a)[:3], f32=PR.solve(*a, dtype=torch.float32)[:3], gpu=_call(d, inv_c, 20))


@pytest.mark.parametrize("L,Nc", [(L, Nc) for L in (6, 64, 130) for Nc in (1, 2, 9)])
def test_solved_poses_exact_properties(L, Nc):
    from fpc_diffrend_amd import fit
    for offset in (0, 1):
        for robust in (False, True):
            case, r = _case_name(L, Nc, offset, robust), _solved(L, Nc, offset, robust)
            cs, inv_c, a, d, lms = r['cs'], r['inv_c'], r['a'], r['d'], r['lms']
            q, t, info, nrm = r['gpu']
            still, F = cs['still'], 3
            moved = [f for f in range(F) if f != still]
            # exact properties
            assert torch.equal(q[still], d['q'][still]) and torch.equal(t[still], d['t'][still]) and float(info[still, 3]) == 0.0
            assert float(info[still, 2]) == 2.0 and torch.equal(info[still, 0], info[still, 1])
            at_in = _call(d, inv_c, 0)[2]
            assert bool((info[:, 1] <= info[:, 0]).all()) and bool((info[:, 2] >= at_in[:, 2]).all()) and torch.equal(info[:, 0], at_in[:, 0])
            assert bool((info[moved, 3] > 0).all())
            qn = q[moved].double().norm(dim=1)
            assert float((qn - 1.0).abs().max()) <= 2 * U, (case, qn)
            again = _call(d, inv_c, 20)
            assert all(torch.equal(p, r) for p, r in zip(again, (q, t, info, nrm))), case
            q0, t0, info0, _ = _call(d, inv_c, 20, rotation=0)
            assert torch.equal(q0, d['q']) and bool((info0[:, 1] <= info0[:, 0]).all()) and bool((info0[moved, 3] > 0).all())
            assert torch.equal(q0[still], d['q'][still]) and torch.equal(t0[still], d['t'][still])
            # the module's entry: the same call
            qm, tm = d['q'].clone(), d['t'].clone()
            im = fit.solve_pose(d['x'], d['proj'], d['base'], lms, d['obs'], qm, tm, (PC.H, PC.W), scale=cs['scale'])
            assert torch.equal(qm, q) and torch.equal(tm, t) and torch.equal(im, info), case


@pytest.mark.parametrize("L,Nc,offset,robust", PC.SOLVE_CASES)
def test_distance_of_the_solved_pose_from_the_float64_solver(L, Nc, offset, robust):
    """|(q, t) - float64's| <= 8 x the float32 statement's distance + 4 u of the scale (1 for q, max(|t|, |y|) for t)."""
    case, r = _case_name(L, Nc, offset, robust), _solved(L, Nc, offset, robust)
    a = r['a']
    (q64, t64, info64), (q32, t32, info32), (q, t, info, _) = r['f64'], r['f32'], r['gpu']
    ys = float(PR.normal(*a[:7], q64, t64, PC.H, PC.W)['y'].abs().max())
    ts = max(float(t64.abs().max()), ys)
    dq, dt = PC.pose_distance(q, t, q64, t64)
    dq32, dt32 = PC.pose_distance(q32, t32, q64, t64)
    print(f"POSE solve/{case} dq={dq:.3e} dq32={dq32:.3e} bound={8 * dq32 + 4 * U:.3e}  dt={dt:.3e} dt32={dt32:.3e} "
          f"bound={8 * dt32 + 4 * U * ts:.3e}  accepted gpu {info[:, 3].tolist()} f64 {info64[:, 3].tolist()} f32 {info32[:, 3].tolist()}")
    assert dq <= 8 * dq32 + 4 * U and dt <= 8 * dt32 + 4 * U * ts, (case, dq, dq32, dt, dt32)


@pytest.mark.parametrize("L,Nc,offset,robust", PC.SOLVE_CASES)
def test_cost_at_the_solved_pose_against_the_float64_solver(L, Nc, offset, robust):
    """E_out <= (1 + 1e-4) x float64's E_out, the project's relative bar; where that is 0, the float32 statement's value instead.  "Is 0":
    below pose_cases.cost_floor, the cost of a pose 4 u away -- the float64 solver rounds its trial poses to float32 as the kernel does,
    so where the data are exact (the L2 cases) its E_out is the rounding of its own pose (1e-12 .. 1e-7 here), never a literal 0."""
    case, r = _case_name(L, Nc, offset, robust), _solved(L, Nc, offset, robust)
    (q64, t64, info64), info32, info = r['f64'], r['f32'][2], r['gpu'][2]
    floor = PC.cost_floor(PR.normal(*r['a'][:7], q64, t64, *r['a'][9:]), t64)
    for f in range(3):
        if f == r['cs']['still']:
            continue
        e, e64, e32 = float(info[f, 1]), float(info64[f, 1]), float(info32[f, 1])
        zero = e64 <= float(floor[f])
        print(f"POSE cost/{case} frame {f} E_in={float(info[f, 0]):.6e} E_out={e:.6e} float64 {e64:.6e} float32 {e32:.6e} floor {float(floor[f]):.3e} "
              + (f"float64 is 0: E_out / float32 - 1 = {e / e32 - 1:.3e}" if zero else f"E_out / float64 - 1 = {e / e64 - 1:.3e}"))
        assert e <= (1 + 1e-4) * (e32 if zero else e64), (case, f, e, e64, e32)


def test_solve_pose_refuses_what_does_not_fit():
    from fpc_diffrend_amd import fit
    cs = PC.solve_case(6, 2, 0, False)
    d, lms = _device(cs)
    ok = lambda **kw: dict(dict(verts=d['x'], proj=d['proj'], base=d['base'], lms=lms, obs=d['obs'], q=d['q'].clone(), t=d['t'].clone(),
                                resolution=(PC.H, PC.W)), **kw)
    for kw, match in ((dict(q=torch.zeros(3, 4, device='cuda')), "norm of q"), (dict(q=d['q'][:2].clone()), "q must be"),
                      (dict(t=d['t'].double()), "t must be"), (dict(iters=-1), "iters"), (dict(iters=2.5), "iters"), (dict(damping=0.0), "damping"),
                      (dict(scale=-1.0), "scale"), (dict(base=d['base'][:1]), "same cameras"), (dict(obs=d['obs'][:2]), "obs must be"),
                      (dict(normal_out=torch.zeros(3, 27, device='cuda')), "normal_out"), (dict(resolution=(0, 5)), "resolution"),
                      (dict(lms=None), "LandmarkSet")):
        with pytest.raises(ValueError, match=match):
            fit.solve_pose(**ok(**kw))
    assert fit.solve_pose is __import__('fpc_diffrend_amd').landmarks.solve_pose


# ---------------------------------------------------------------------------------------------------------------------
# inside a Fitter
# ---------------------------------------------------------------------------------------------------------------------

RES = (128, 128)
N_LMK = 40


def _scene(n_frames=4):
    """cfg1's scene at 128 x 128 with the truth pose of every frame replaced by one 25 degrees / 8 units from the identity, and N_LMK
    landmarks on every thirteenth vertex from fit.project_landmarks at that truth."""
    from fpc_diffrend_amd import fit, scene
    sc = scene.make_scene(scene.MESH_1K, 10, n_frames, RES, (256, 256, 1), 0)
    for f in range(n_frames):
        q, t = PC.pose_of(25.0, 8.0, 40 + f)
        sc.q_gt[f], sc.t_gt[f] = q.astype(np.float32), t.astype(np.float32)
    sc.landmark_points = [{'vertex': v} for v in range(0, sc.n_vertices, 13)]
    assert len(sc.landmark_points) == N_LMK
    sc.landmarks = fit.project_landmarks(sc, sc.landmark_points).astype(np.float32)
    return sc


@functools.lru_cache(maxsize=None)
def _targets(n_frames=4):
    """The rendered captures of _scene(n_frames), made once and shared (each Fitter would render them anew)."""
    return _fitter(n_frames, _shared=False).targets


def _fitter(n_frames=4, rank=0, world=1, _shared=True, **kw):
    """A Fitter on _scene: cameras 0 and 3, the blend weights at the truth, the pose at the identity, FitConfig's default learning
    rates; kw overrides any FitConfig field."""
    from fpc_diffrend_amd import fit
    sc = _scene(n_frames)
    base = dict(max_iter=100, cam_idxs=(0, 3), weight_laplacian=0.0, optimize_texture=False)
    base.update(kw)
    targets = None
    if _shared:
        lo, hi = rank * n_frames // world, (rank + 1) * n_frames // world
        targets = _targets(n_frames)[lo:hi]
    ft = fit.Fitter(sc, fit.FitConfig(**base), device='cuda', rank=rank, world=world, targets=targets)
    with torch.no_grad():
        ft.maps['local'].copy_(torch.eye(n_frames, device='cuda'))
        ft.maps_intermediate['local'].copy_(torch.tensor(sc.weights_gt, device='cuda').t())
    return ft


def _float32_solver_residual(ft):
    """The mean live |residual| (float64, px) at the poses the float32 CPU statement solves for ft's meshes, cameras and observations."""
    lms, obs, res = ft._landmark_tables("test")
    F = ft.frame_hi - ft.frame_lo
    x = ft.vertices(slice(ft.frame_lo, ft.frame_hi)).detach().reshape(F, -1, 3).cpu()
    q0 = torch.zeros(F, 4)
    q0[:, 3] = 1.0
    a = (x, ft.proj.cpu(), ft.t_mv.cpu(), lms.vtx.cpu().numpy(), lms.bary.cpu().numpy(), None, obs.cpu())      # (the cameras' own poses are at the identity: B_c = MV_c T)
    q32, t32, info32, _ = PR.solve(*a, q0, torch.zeros(F, 3), *res, dtype=torch.float32)
    return PR.mean_residual(*a, q32, t32, *res), (q32, t32, info32)


def test_align_to_landmarks_brings_every_frame_home_and_rows_keep_it_there():
    ft = _fitter(quat_renorm='rows')
    assert ft._lmk is None and ft._lmk_obs is None and not ft.landmark_on()       # weight_landmark = 0: nothing is built before the call
    with pytest.raises(ValueError, match="weight_landmark"):
        ft.landmark_residuals()
    out = ft.align_to_landmarks()
    assert ft._lmk is not None and ft._lmk_scratch is None and not ft.landmark_on()      # ... and the term stays off
    after = LR.mean_live_residual(ft.landmark_residuals())                        # the independent chain: k_mvp_fwd, k_landmark_points
    ref, (q32, t32, info32) = _float32_solver_residual(ft)
    bound = 8 * ref + 4 * U * (RES[0] + RES[1])
    dq, dt = PC.pose_distance(ft.per_frame_q, ft.per_frame_t, q32, t32)
    print(f"POSE fitter align: before {out['before']:.3f} px after {out['after']:.3e} px; landmark_residuals {after:.3e} px; the float32 "
          f"statement's poses {ref:.3e} px, bound {bound:.3e} px; distance from them dq={dq:.3e} dt={dt:.3e}; accepted {out['info'][:, 3].tolist()}")
    assert out['before'] > 50.0 and abs(out['after'] - after) <= 1e-6 * max(after, 1e-3) and tuple(out['info'].shape) == (4, 4)
    assert after <= bound, (after, ref, bound)
    assert all(not st for st in ft.optimizer.state.values())                      # Adam's moments are not touched
    for _ in range(3):
        ft.step()
    later = LR.mean_live_residual(ft.landmark_residuals())
    print(f"POSE fitter align: after three steps at the default learning rates {later:.3e} px (2 x the bound: {2 * bound:.3e} px)")
    assert later <= 2 * bound, (later, bound)


def test_under_tensor_renorm_rotation_is_refused_and_translation_alone_helps():
    ft = _fitter()
    assert ft.cfg.quat_renorm == 'tensor'
    with pytest.raises(ValueError, match="quat_renorm='rows'"):
        ft.align_to_landmarks()
    q0 = ft.per_frame_q.detach().clone()
    out = ft.align_to_landmarks(rotation=False)
    print(f"POSE fitter translation alone: before {out['before']:.3f} px after {out['after']:.3f} px")
    assert out['after'] < out['before'] and torch.equal(ft.per_frame_q.detach(), q0)
    assert LR.mean_live_residual(ft.landmark_residuals()) < out['before']
    with pytest.raises(ValueError, match="iters"):
        ft.align_to_landmarks(rotation=False, iters=-2)
    one = _fitter(1)                                                              # one frame: the whole tensor IS the row
    assert one.align_to_landmarks()['after'] < 1e-2
    from fpc_diffrend_amd import fit, scene
    plain = scene.make_scene(scene.MESH_1K, 10, 2, RES, (256, 256, 1), 0)         # a Scene without landmarks
    with pytest.raises(ValueError, match="Scene with landmarks"):
        fit.Fitter(plain, fit.FitConfig(max_iter=10, cam_idxs=(0, 3), init_pose='landmarks', init_pose_rotation=False), device='cuda')


def test_init_pose_landmarks_is_the_explicit_call():
    from fpc_diffrend_amd import fit
    sc = _scene()
    kw = dict(max_iter=100, cam_idxs=(0, 3), weight_laplacian=0.0, optimize_texture=False, quat_renorm='rows')
    a = fit.Fitter(sc, fit.FitConfig(init_pose='landmarks', init_pose_iters=15, **kw), device='cuda', targets=_targets())
    b = fit.Fitter(sc, fit.FitConfig(**kw), device='cuda', targets=_targets())
    assert float((b.per_frame_t.detach()).abs().max()) == 0.0
    b.align_to_landmarks(iters=15)
    assert all(torch.equal(p.detach(), r.detach()) for p, r in zip(a.params, b.params))
    assert float(a.per_frame_t.detach().abs().max()) > 1.0 and a.state_dict()['config']['init_pose'] == 'landmarks'
    c = fit.Fitter(sc, fit.FitConfig(init_pose='landmarks', init_pose_rotation=False, **dict(kw, quat_renorm='tensor')), device='cuda', targets=_targets())
    assert float(c.per_frame_t.detach().abs().max()) > 1.0 and float((c.per_frame_q.detach()[:, :3]).abs().max()) == 0.0


def test_two_ranks_end_with_identical_tables():
    """Rank 1 of 2 with a reduce that adds the other shard's delta, and rank 0 with rank 1's: the replicated tables are identical, and
    they are the single rank's."""
    whole = _fitter(quat_renorm='rows')
    whole.align_to_landmarks()
    r0, r1 = _fitter(rank=0, world=2, quat_renorm='rows'), _fitter(rank=1, world=2, quat_renorm='rows')
    own = {}

    def keep(rank, other=None):
        def reduce(delta):
            own[rank] = delta.clone()
            return delta if other is None else delta + own[other]
        return reduce

    r0.align_to_landmarks(reduce=keep(0))
    assert float(own[0][2:].abs().max()) == 0.0 and float(own[0][:2].abs().max()) > 0.0      # zero outside the shard
    r1.align_to_landmarks(reduce=keep(1, other=0))
    assert float(own[1][:2].abs().max()) == 0.0
    with torch.no_grad():                                                          # rank 0 receives rank 1's share of the sum
        r0.per_frame_q.add_(own[1][:, :4])
        r0.per_frame_t.add_(own[1][:, 4:])
    for a, b, c in zip(r0.params, r1.params, whole.params):
        assert torch.equal(a.detach(), b.detach()) and torch.equal(a.detach(), c.detach())
    with pytest.raises(IndexError):
        r1.align_to_landmarks(frame_ids=[0])                                       # a frame of the other shard


def test_a_graphed_step_after_the_align_equals_the_eager_one():
    """The solve writes per_frame_q / per_frame_t in place, so a captured graph replays with them; 'rows' is a value of the update
    kernel's renorm field, so it replays too.  The tolerance is the captured-steps tests' (the pixel term's gradient has float atomics)."""
    traj, poses = {}, {}
    for graph in (False, True):
        ft = _fitter(quat_renorm='rows', hip_graph=graph, weight_landmark=3.0, landmark_scale=3.0, lr_t=1e-3, lr_q=1e-3)
        ft.align_to_landmarks(rotation=True, iters=3)                             # (three trials: the steps still have somewhere to go)
        traj[graph] = [float(ft.step()) for _ in range(ft.GRAPH_WARMUP + 4)]
        poses[graph] = torch.cat([ft.per_frame_q.detach(), ft.per_frame_t.detach()], dim=1).cpu()
        if graph:
            assert ft._graphs is not None
        assert float((ft.per_frame_q.detach().double().norm(dim=1) - 1.0).abs().max()) <= 4 * U      # (the update kernel's float32 division)
    a, b = np.asarray(traj[False]), np.asarray(traj[True])
    print(f"POSE fitter graph: eager {a} graphed {b}")
    assert np.isfinite(b).all() and np.allclose(a, b, rtol=1e-5), (a, b)
    assert torch.allclose(poses[False], poses[True], rtol=0, atol=1e-5)

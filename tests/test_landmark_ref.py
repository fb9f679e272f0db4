"""CPU: the float64 statement of the landmark term (tests/landmark_ref.py; DESIGN.md 3, "Landmark rule") against torch.autograd of a plain
restatement, the consequences of the rule (exact zeros where an entry is not live), the host side of the feature -- LandmarkSet's tables
against plain loops, the landmark file's round trip, project_landmarks against helpers.scene_mvps applied by hand, FitConfig, the C entry
and its argument checks, the kernels' private segment, the README's table -- no GPU.

Measured: the closed-form gradients against autograd, the largest |g_i - a_i| over an output relative to its largest entry, over the
cases below: 5.1e-15 (grad_x) and 1.9e-15 (grad_mvp); the bound is 1e-10."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import landmark_cases as LC
import landmark_ref as LR
from helpers import scene_mvps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _ref_and_autograd(cs, weight=3.5):
    inv_c = 0.0 if cs['scale'] is None else float(np.float32(1.0 / cs['scale']))
    c = None if cs['scale'] is None else 1.0 / inv_c      # (the plain form is handed the c that the float32 stands for)
    x, m = cs['x'].double().requires_grad_(True), cs['mvp'].double().requires_grad_(True)
    val = LR.landmark_plain(x, m, cs['vtx'], cs['bary'], cs['w'], cs['obs'].double(), weight, LC.H, LC.W, c)
    gx, gm = torch.autograd.grad(val, (x, m), allow_unused=True)
    gx = torch.zeros_like(x) if gx is None else gx
    gm = torch.zeros_like(m) if gm is None else gm
    return LR.landmark(cs['x'], cs['mvp'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], weight, LC.H, LC.W, inv_c), val.detach(), gx, gm


@pytest.mark.parametrize("use_w,use_c", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("F,Nc,V,L", [(1, 1, 3, 1), (3, 2, 257, 65), (1, 9, 514, 130), (3, 9, 255, 63)])
def test_closed_form_gradients_equal_autograd_of_the_plain_form(F, Nc, V, L, use_w, use_c):
    """Cases with live and dead entries, both rho, landmark weights with zeros, points behind a camera, landmarks that share vertices."""
    cs = LC.case(F, Nc, V, L, 0, use_w, use_c)
    ref, val, gx, gm = _ref_and_autograd(cs)
    live = ref['live']
    if L > 1:
        assert bool(live.any()) and not bool(live.all())
    assert abs(float(ref['value'][0]) - float(val)) <= 1e-10 * max(1.0, abs(float(val)))
    ex = float((ref['grad_x'][0] - gx).abs().max()) / max(float(gx.abs().max()), 1e-300)
    em = float((ref['grad_mvp'][0] - gm).abs().max()) / max(float(gm.abs().max()), 1e-300)
    print(f"LANDMARK ref F{F}/Nc{Nc}/V{V}/L{L} closed form against autograd: grad_x {ex:.2e} grad_mvp {em:.2e}")
    assert ex <= 1e-10 and em <= 1e-10, (ex, em)
    # the scales dominate the values, and vanish exactly where the tables say that no term is
    for k in ('grad_x', 'grad_mvp', 'per'):
        assert bool((ref[k][1] >= ref[k][0].abs() * (1 - 1e-12)).all()), k
        assert int((ref[k][1] == 0).sum()) == ref['zeros'][k], (k, int((ref[k][1] == 0).sum()), ref['zeros'][k])
    assert int(torch.isnan(ref['res'][0]).sum()) == ref['zeros']['res']


def test_entries_that_are_not_live_give_exact_zeros():
    """kappa = 0, omega = 0, p.w <= 1e-6: value, per and every gradient exactly 0; a NaN in what nobody observed changes nothing."""
    cs = LC.case(3, 2, 257, 65, 0, True, True)
    inv_c = float(np.float32(1.0 / cs['scale']))
    full = LR.landmark(cs['x'], cs['mvp'], cs['vtx'], cs['bary'], cs['w'], cs['obs'], 2.0, LC.H, LC.W, inv_c)
    for name, kw in (('kappa', dict(obs=torch.cat([cs['obs'][..., :2], torch.zeros_like(cs['obs'][..., 2:])], dim=-1))),
                     ('omega', dict(w=torch.zeros(65))),
                     ('behind', dict(mvp=cs['mvp'] * torch.tensor([1.0, 1.0, 1.0, -1.0]).reshape(1, 4, 1)))):      # p.w -> -p.w
        a = dict(x=cs['x'], mvp=cs['mvp'], w=cs['w'], obs=cs['obs'])
        a.update(kw)
        r = LR.landmark(a['x'], a['mvp'], cs['vtx'], cs['bary'], a['w'], a['obs'], 2.0, LC.H, LC.W, inv_c)
        if name == 'behind':      # what was in front is behind now, and the other way round: live flips among the observed entries
            seen = (cs['obs'][..., 2] > 0) & (cs['w'][None] > 0)
            assert torch.equal(r['live'], seen & ~full['live'])
            continue
        assert not bool(r['live'].any()), name
        assert float(r['value'][0]) == 0.0 and float(r['per'][0].abs().max()) == 0.0, name
        assert float(r['grad_x'][0].abs().max()) == 0.0 and float(r['grad_mvp'][0].abs().max()) == 0.0, name
        assert bool(torch.isnan(r['res'][0]).all()), name
    # a point exactly at the threshold does not count; just above it, it does
    x = torch.zeros(1, 1, 3, dtype=torch.float64)
    for pw, want in ((1e-6, False), (0.0, False), (-1.0, False), (1.0000001e-6, True)):
        m = torch.eye(4, dtype=torch.float64)[None].clone()
        m[0, 3, 3] = pw
        r = LR.landmark(x, m, np.zeros((3, 1), np.int64), np.array([[1.0], [0.0], [0.0]], np.float32), None,
                        torch.tensor([[[0.5, 0.5, 1.0]]], dtype=torch.float64), 1.0, 4, 4)
        assert bool(r['live'][0, 0]) == want, pw


def test_landmark_set_tables_agree_with_a_plain_loop():
    from fpc_diffrend_amd import fit
    faces = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4], [0, 2, 5]])
    V = 7      # (vertex 6 belongs to no face and to no landmark)
    points = [{'vertex': 2, 'name': 'nose'}, {'face': 1, 'bary': (0.2, 0.3, 0.5), 'weight': 2.5}, {'vertex': 2}, {'vertex': 5, 'weight': 0.0},
              {'face': 0, 'bary': (1 / 3, 1 / 3, 1 / 3)}, {'face': 3, 'bary': (0.0, 1.0, 0.0), 'name': 'on a vertex'}]
    lms = fit.LandmarkSet(points, V, faces, 'cpu')
    vtx, bary, w = LR.tables(points, V, faces)
    inc = LR.incidence(vtx, bary, V)
    assert lms.vtx.dtype == torch.int32 and lms.bary.dtype == torch.float32 and lms.w.dtype == torch.float32 and lms.inc.dtype == torch.int32
    assert np.array_equal(lms.vtx.numpy(), vtx) and np.array_equal(lms.bary.numpy(), bary) and np.array_equal(lms.w.numpy(), w)
    assert np.array_equal(lms.inc.numpy(), inc) and lms.K == inc.shape[0] and lms.n == 6 and lms.n_vertices == V
    # vertex 2: landmarks 0 and 2 (corner 0 each), face 1's corner 0, face 0's corner 2, face 3's corner 1 -> five slots, ascending
    assert inc[:, 2].tolist() == [0, 3, 6, 14, 16] and lms.K == 5
    assert inc[:, 6].tolist() == [-1] * 5 and inc[:, 5].tolist() == [9, -1, -1, -1, -1]      # (a corner of weight 0 has no slot: face 3's corner 2)
    assert lms.names == ['nose', '1', '2', '3', '4', 'on a vertex']
    assert lms.bary[:, 1].tolist() == [float(np.float32(0.2)), float(np.float32(0.3)), 0.5]
    other = lms.with_weights([1, 2, 3, 4, 5, 6])
    assert other.w.tolist() == [1, 2, 3, 4, 5, 6] and other.inc is lms.inc and lms.w.tolist() == [1, 2.5, 1, 0, 1, 1]
    for bad, why in (([{'vertex': 7}], "out of range"), ([{'vertex': -1}], "out of range"), ([{'face': 4, 'bary': (1, 0, 0)}], "out of range"),
                     ([{'face': 0, 'bary': (1, float('nan'), 0)}], "finite"), ([{'face': 0, 'bary': (1, 0)}], "three finite"),
                     ([{'vertex': 1, 'weight': float('inf')}], "finite and not negative"), ([{'vertex': 1, 'weight': -1.0}], "finite and not negative"),
                     ([{'vertex': 1, 'face': 0}], "a point is"), ([{}], "a point is"), ([], "at least one")):
        with pytest.raises(ValueError, match=why):
            fit.LandmarkSet(bad, V, faces, 'cpu')
    with pytest.raises(ValueError, match="one number per landmark"):
        lms.with_weights([1.0, 2.0])


def _scene_with_landmarks(n_frames=3):
    from fpc_diffrend_amd import fit, scene
    sc = scene.cfg('cfg1', n_frames=n_frames)
    sc.landmark_points = [{'vertex': int(v), 'name': f"v{v}"} for v in range(5, 514, 37)] + [{'face': 100, 'bary': [0.5, 0.25, 0.25], 'weight': 2.0}]
    sc.landmarks = fit.project_landmarks(sc, sc.landmark_points).astype(np.float32)
    return sc


def test_landmark_file_round_trip_is_exact(tmp_path):
    """write_take -> from_take: float32 for float32, the row flip included; a null entry and an absent camera come back as kappa = 0."""
    from fpc_diffrend_amd import scene
    sc = _scene_with_landmarks(2)
    cams = [0, 3, 4]
    H, W = 24, 32
    lm = sc.landmarks[:, cams].copy()                             # [2,3,L,3]
    lm[..., :2] += np.float32(0.1)                                # (not on a grid of halves)
    lm[0, 1, 2, 2] = 0.0                                          # one entry not observed
    lm[1, 2, :, 2] = 0.0                                          # a whole image not observed
    lm[..., 2] *= np.float32(0.7)
    images = np.zeros((2, 3, H, W), dtype=np.uint8)
    paths = scene.write_take(sc, str(tmp_path), images, cam_idxs=cams, landmarks=lm)
    path = os.path.join(str(tmp_path), "landmarks.json")
    doc = json.load(open(path))
    names = [f"cam_{sc.cams[c]['cam']}" for c in cams]
    assert sorted(doc["observations"]) == sorted(names) and doc["points"] == sc.landmark_points
    assert doc["observations"][names[1]][0][2] is None
    e = doc["observations"][names[0]][1][3]
    assert e[0] == float(lm[1, 0, 3, 0]) and e[1] == (H - 1) - float(lm[1, 0, 3, 1])      # x right, y DOWN
    back = scene.from_take(*paths, landmarkpath=path)
    assert back.landmark_points == sc.landmark_points and back.landmarks.dtype == np.float32 and back.landmarks.shape == lm.shape
    want = lm.copy()
    want[want[..., 2] == 0] = 0.0                                 # (what nobody observed is not stored)
    order = [sorted(names).index(n) for n in names]              # (from_take sorts the camera directories)
    assert np.array_equal(back.landmarks[:, order], want)
    # an absent camera: kappa = 0 for all of it
    del doc["observations"][names[2]]
    doc["observations"][names[0]][0] = None                        # ... and a frame given as null
    json.dump(doc, open(path, "w"))
    back = scene.from_take(*paths, landmarkpath=path)
    assert float(np.abs(back.landmarks[:, order[2]]).max()) == 0.0 and float(np.abs(back.landmarks[0, order[0]]).max()) == 0.0
    assert np.array_equal(back.landmarks[1, order[0]], want[1, 0])
    assert scene.from_take(*paths).landmarks is None
    doc["observations"][names[0]][1][0] = [1.0, 2.0]
    json.dump(doc, open(path, "w"))
    with pytest.raises(ValueError, match="an entry is"):
        scene.from_take(*paths, landmarkpath=path)


def test_project_landmarks_agrees_with_the_scenes_matrices_applied_by_hand():
    from fpc_diffrend_amd import fit
    sc = _scene_with_landmarks(3)
    cams = (0, 4, 7)
    got = fit.project_landmarks(sc, sc.landmark_points, cams)
    L = len(sc.landmark_points)
    assert got.shape == (3, 3, L, 3) and got.dtype == np.float64 and bool((got[..., 2] == 1.0).all())
    assert np.array_equal(got, fit.project_landmarks(sc, sc.landmark_points)[:, list(cams)])
    H, W = sc.resolution
    mvps = scene_mvps(sc, cams, [0, 1, 2]).double().reshape(3, 3, 4, 4)
    verts = (torch.tensor(sc.v_base).double()[None] + torch.tensor(sc.weights_gt).double() @ torch.tensor(sc.blendshapes).double().t()).reshape(3, -1, 3)
    vtx, bary, _ = LR.tables(sc.landmark_points, sc.n_vertices, sc.pos_idx)
    for f in range(3):
        for j in range(3):
            for l in range(L):
                q = sum(float(bary[k, l]) * verts[f, int(vtx[k, l])] for k in range(3))
                p = mvps[f, j] @ torch.cat([q, torch.ones(1, dtype=torch.float64)])
                u, v = (p[0] / p[3] * 0.5 + 0.5) * W - 0.5, (p[1] / p[3] * 0.5 + 0.5) * H - 0.5
                # (scene_mvps rounds its matrices to float32: 1e-3 of a pixel on a 256-pixel raster)
                assert abs(float(u) - got[f, j, l, 0]) <= 2e-3 and abs(float(v) - got[f, j, l, 1]) <= 2e-3, (f, j, l)
    assert bool(((got[..., 0] > 0) & (got[..., 0] < W) & (got[..., 1] > 0) & (got[..., 1] < H)).mean() > 0.9)      # the head is in view


def test_fitconfig_landmark_options():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert (cfg.weight_landmark, cfg.landmark_scale, cfg.landmark_iters, cfg.landmark_weights, cfg.use_landmarks) == (0.0, None, 0, None, True)
    for w in (-1.0, float('nan'), float('inf'), True, "1"):
        with pytest.raises(ValueError, match="weight_landmark"):
            fit.FitConfig(weight_landmark=w)
    for scale in (0.0, -1.0, float('inf'), float('nan'), 1e-60, True):
        with pytest.raises(ValueError, match="landmark_scale"):
            fit.FitConfig(landmark_scale=scale)
    for n in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="landmark_iters"):
            fit.FitConfig(landmark_iters=n)
    for u in (1, None, "yes"):
        with pytest.raises(ValueError, match="use_landmarks"):
            fit.FitConfig(use_landmarks=u)
    fit.FitConfig(weight_landmark=2.0, landmark_scale=3.0, landmark_iters=10, landmark_weights=[1.0, 2.0], use_landmarks=False)


def test_landmark_penalty_argument_errors():
    from fpc_diffrend_amd import fit
    faces = np.array([[0, 1, 2], [2, 1, 3]])
    lms = fit.LandmarkSet([{'vertex': 0}, {'face': 1, 'bary': (0.2, 0.3, 0.5)}], 5, faces, 'cpu')
    x, mvp, obs = torch.zeros(2, 5, 3), torch.eye(4).repeat(6, 1, 1), torch.zeros(6, 2, 3)
    ok = dict(verts=x, mvp=mvp, lms=lms, obs=obs, weight=1.0, resolution=(8, 8))
    for over, why in ((dict(lms=None), "LandmarkSet"), (dict(verts=torch.zeros(2, 5, 2)), r"float32 \[F,V,3\]"), (dict(verts=torch.zeros(2, 4, 3)), "5 vertices"),
                      (dict(mvp=torch.eye(4).repeat(5, 1, 1)), "mvp must be"), (dict(mvp=torch.eye(4).repeat(6, 1, 1).double()), "mvp must be"),
                      (dict(obs=torch.zeros(6, 3, 3)), "obs must be"), (dict(obs=torch.zeros(6, 2, 3).double()), "obs must be"),
                      (dict(resolution=8), "resolution"), (dict(resolution=(0, 8)), "resolution"), (dict(scale=0.0), "scale"),
                      (dict(scale=float('nan')), "scale"), (dict(residuals=torch.zeros(6, 2, 3)), "residuals must be"),
                      (dict(obs=torch.full((6, 2, 3), -1.0)), "finite and not negative")):
        with pytest.raises(ValueError, match=why):
            fit.landmark_penalty(**{**ok, **over})
    with pytest.raises(RuntimeError, match="GPU only"):                   # valid arguments: no CPU fallback
        fit.landmark_penalty(**ok, scale=2.0)


_SHARED_BAD = [("lms", dict(lms=None), "lms must be a LandmarkSet"), ("verts dtype", dict(verts=torch.zeros(1, 4, 3, dtype=torch.float64)), "verts must be float32"),
               ("verts rank", dict(verts=torch.zeros(4, 3)), "verts must be float32"), ("vertex count", dict(verts=torch.zeros(1, 5, 3)), "4 vertices"),
               ("obs shape", dict(obs=torch.zeros(1, 3, 3)), "obs must be"), ("resolution pair", dict(resolution=8), "resolution must be"),
               ("resolution positive", dict(resolution=(0, 8)), "both positive")]


@pytest.mark.parametrize("entry", ["landmark_penalty", "solve_pose"])
def test_the_shared_argument_checks_speak_in_the_callers_name(entry):
    """What landmark_penalty and solve_pose ask of lms, verts, obs and resolution is one check: each fault raises ValueError, and the
    message starts with the name of the function that was called.  CPU tensors: the checks come before any launch."""
    from fpc_diffrend_amd import fit
    lms = fit.LandmarkSet([{'vertex': 0}, {'face': 0, 'bary': (0.2, 0.3, 0.5)}], 4, np.array([[0, 1, 2], [2, 1, 3]]), 'cpu')
    ok = dict(verts=torch.zeros(1, 4, 3), lms=lms, obs=torch.zeros(1, 2, 3), resolution=(8, 8))
    if entry == "landmark_penalty":
        ok.update(mvp=torch.eye(4).reshape(1, 4, 4), weight=1.0)
    else:
        ok.update(proj=torch.eye(4).reshape(1, 4, 4), base=torch.eye(4).reshape(1, 4, 4), q=torch.tensor([[0.0, 0.0, 0.0, 1.0]]), t=torch.zeros(1, 3))
    for what, over, why in _SHARED_BAD:
        with pytest.raises(ValueError, match=why) as e:
            getattr(fit, entry)(**{**ok, **over})
        assert str(e.value).startswith(entry + ": "), (what, str(e.value))


def _lib_loaded():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def test_the_entry_is_declared_bound_and_exported_and_abi_stays_16():
    _lib, lib = _lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert "fpcdr_landmark_penalty" in _lib.SYMBOLS and hasattr(lib, "fpcdr_landmark_penalty")
    assert len(_lib.SYMBOLS["fpcdr_landmark_penalty"][1]) == 24
    assert "int fpcdr_landmark_penalty(" in open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    assert "fpcdr_landmark_penalty" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if os.path.exists(_lib.TWOCALL_LIB_PATH):
        assert hasattr(ctypes.CDLL(_lib.TWOCALL_LIB_PATH), "fpcdr_landmark_penalty")


def test_bad_arguments_give_an_error_code_before_any_launch():
    """Nulls, sizes, a misaligned acc, a negative or non-finite inv_c, one gradient without the other: the checks come before the first
    HIP call, so this runs without a GPU on host memory the entry never touches."""
    _lib, lib = _lib_loaded()
    F, Nc, V, L, K = 2, 3, 5, 4, 2
    fb = lambda n: (ctypes.c_float * (n + 4))()
    ib = lambda n: (ctypes.c_int32 * (n + 4))()
    bufs = dict(x=fb(F * V * 3), mvp=fb(F * Nc * 16), lm_vtx=ib(3 * L), lm_bary=fb(3 * L), lm_w=fb(L), lm_inc=ib(K * V), obs=fb(F * Nc * L * 3),
                scratch=fb(F * Nc * L * 3), grad_x=fb(F * V * 3), grad_mvp=fb(F * Nc * 16), res_out=fb(F * Nc * L * 2), per=fb(F), out=fb(1))
    acc = (ctypes.c_double * (F + 2))()
    P = lambda b: ctypes.cast(b, ctypes.c_void_p)
    order = ('x', 'mvp', 'lm_vtx', 'lm_bary', 'lm_w', 'lm_inc', 'obs', 'inv_c', 'width', 'height', 'scratch', 'grad_x', 'grad_mvp', 'res_out',
             'acc', 'per', 'out', 'weight', 'F', 'Nc', 'V', 'L', 'K')

    def args(**over):
        kw = {k: P(v) for k, v in bufs.items()}
        kw.update(inv_c=0.0, width=8, height=6, acc=P(acc), weight=1.0, F=F, Nc=Nc, V=V, L=L, K=K)
        kw.update(over)
        return [kw[k] for k in order] + [None]

    bad = [dict(x=None), dict(mvp=None), dict(lm_vtx=None), dict(lm_bary=None), dict(obs=None), dict(acc=None), dict(per=None), dict(out=None),
           dict(acc=ctypes.c_void_p(ctypes.addressof(acc) + 4)), dict(F=0), dict(F=65536), dict(Nc=0), dict(V=0), dict(L=0), dict(K=0), dict(L=-2),
           dict(width=0), dict(height=-1), dict(inv_c=-1.0), dict(inv_c=float('inf')), dict(inv_c=float('nan')),
           dict(grad_x=None), dict(grad_mvp=None), dict(scratch=None), dict(lm_inc=None)]
    for i, over in enumerate(bad):
        assert lib.fpcdr_landmark_penalty(*args(**over)) != 0, i
        assert b"fpcdr_landmark_penalty" in lib.fpcdr_last_error()
    assert all(v == 0.0 for v in acc)


def test_landmark_kernels_have_no_private_segment():
    """read from the built object (tests/codeobj.py).  LDS only for the reductions: the twelve matrix entries of four
    waves and the four value partials in k_landmark_points, none in the gather."""
    import codeobj
    recs = codeobj.kernels("landmark.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    own = {name: (private, lds) for name, private, lds in recs if "k_landmark" in name}
    assert len(own) == 2 and all(p == 0 for p, _ in own.values()), own
    lds = {("points" if "points" in name else "gather"): l for name, (_, l) in own.items()}
    assert lds == {"points": 4 * 12 * 4 + 4 * 8, "gather": 0}, lds
    finish = {name: private for name, private, _ in recs if "k_penalty_finish" in name}      # the finish kernel it shares with the mesh terms
    assert len(finish) == 1 and all(p == 0 for p in finish.values()), finish
    # ... shared, not copied: one definition, in the header both sources include
    csrc = os.path.join(ROOT, "fpc_diffrend_amd", "csrc")
    for src in ("landmark.hip", "mesh_reg.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "penalty_finish.h"' in text and "void block_add_f64(" not in text and "k_penalty_finish(double" not in text, src


def test_the_readmes_table_rows_come_from_the_statement():
    import landmark_table as T
    rows = T.rows()
    assert [r['d'] for r in rows] == [-40, -20, -8, -2, 0, 2, 8, 20, 40]
    readme = open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()
    for r in rows:
        assert T.format_row(r) in readme, T.format_row(r)
    # the landmark term's derivative along the axis has the sign of the offset at every distance, and its value grows with it
    for r in rows:
        assert r['d'] == 0 or np.sign(r['lmk_slope']) == np.sign(r['d']), r
    vals = [r['lmk'] for r in rows]
    assert vals[4] < 1e-6 and vals[:5] == sorted(vals[:5], reverse=True) and vals[4:] == sorted(vals[4:])

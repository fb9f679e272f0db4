"""CPU: the float64 yardstick of the fit step's small kernels (tests/fitstep_ref.py) is right, and the bounds that
tests/test_gpu_fitstep.py asks of the kernels are reachable: each hand-written gradient equals torch.autograd on the plain float64
formula, the Laplacian built from faces equals the dense form, the MVP restatement equals camera.rigid_grad /
camera.unitquat_to_rotmat, and float32 torch on the GPU file's own inputs stays within the derived bound (short paths) or below 8 u
(long sums) of the float64 value, per entry, against the sum of the absolute values of the entry's terms."""
import numpy as np
import pytest
import torch

import fitstep_ref as R

RT = dict(rtol=1e-12, atol=0.0)


def _close(a, b, scale):
    """|a - b| <= 1e-12 * (sum of the absolute values of the terms): rtol = 1e-12 against the scale, which cancellation cannot
    shrink."""
    assert bool(((a - b).abs() <= 1e-12 * scale).all()), float(((a - b).abs() / scale.clamp(min=1e-300)).max())


def test_blend_and_rig_weight_gradients_equal_autograd():
    vb, Bm, w, go = (t.double() for t in R.blend_inputs(97, 13, 5))
    ref = R.blend(vb, Bm, w, go)
    leaves = [t.clone().requires_grad_(True) for t in (vb, Bm, w)]
    out = leaves[0][None] + leaves[2] @ leaves[1].t()
    (out * go).sum().backward()
    assert torch.allclose(ref['out'][0], out.detach(), **RT)
    for name, leaf in zip(('g_vb', 'g_B', 'g_w'), leaves):
        _close(ref[name][0], leaf.grad, ref[name][1])
    for ids in R.rig_ids(32):
        Fb = len(R.rig_columns(ids, 32))
        mi, maps, go = (t.double() for t in R.rig_inputs(17, 32, 32, Fb))
        ref = R.rig_weights(mi, maps, ids, go)
        a, m = mi.clone().requires_grad_(True), maps.clone().requires_grad_(True)
        wv = torch.matmul(a, m[:, ids]).t()
        (wv * go).sum().backward()
        assert torch.allclose(ref['w'][0], wv.detach(), **RT)
        _close(ref['g_mi'][0], a.grad, ref['g_mi'][1])
        _close(ref['g_maps'][0], m.grad, ref['g_maps'][1])
        named = torch.zeros(32, dtype=torch.bool)
        named[R.rig_columns(ids, 32)] = True
        assert bool((ref['g_maps'][1][:, ~named] == 0).all()) and bool((ref['g_maps'][1][:, named] > 0).all())


def test_mvp_restatement_equals_camera_functions_and_autograd():
    from fpc_diffrend_amd import camera
    g = torch.Generator().manual_seed(0)
    for kind in ('randn', 'camera'):
        qc, tc, qf, tf, P, MV, go = (t.double() for t in R.mvp_inputs(5, 3, kind))
        ref = R.mvp_chain(qc, tc, qf, tf, P, MV, go)
        leaves = [t.clone().requires_grad_(True) for t in (qc, tc, qf, tf)]
        rc = camera.rigid_grad(leaves[1], camera.unitquat_to_rotmat(leaves[0]))
        rf = camera.rigid_grad(leaves[3], camera.unitquat_to_rotmat(leaves[2]))
        out = torch.matmul(P[None], torch.matmul(rf[:, None], torch.matmul(rc, MV)[None])).reshape(-1, 4, 4)
        out.backward(go)
        _close(ref['mvp'][0], out.detach(), ref['mvp'][1])
        for name, leaf in zip(('g_q_cam', 'g_t_cam', 'g_q_frame', 'g_t_frame'), leaves):
            _close(ref[name][0], leaf.grad, ref[name][1])
    for name, nf, ncam, nv, fi, vi, cov in R.mvp_index_cases(g):
        Fb, Nc = (len(fi) if fi is not None else nf), (len(vi) if vi is not None else nv)
        qc, tc, qf, tf, P, MV, go = (t.double() for t in R.mvp_inputs(Fb, Nc, 'camera', n_frames=nf, n_cams=ncam, n_views=nv))
        ref = R.mvp_chain(qc, tc, qf, tf, P, MV, go, fi, vi, cov)
        leaves = [t.clone().requires_grad_(True) for t in (qc, tc, qf, tf)]
        R.mvp_chain_plain(*leaves, P, MV, fi, vi, cov).backward(go)
        for key, leaf in zip(('g_q_cam', 'g_t_cam', 'g_q_frame', 'g_t_frame'), leaves):
            _close(ref[key][0], leaf.grad, ref[key][1])
        rows_f = set(fi.tolist()) if fi is not None else set(range(Fb))
        unnamed = [r for r in range(nf) if r not in rows_f]
        assert bool((ref['g_q_frame'][1][unnamed] == 0).all()) and bool((ref['g_q_frame'][1][sorted(rows_f)] > 0).all()), name


def test_clip_gradients_equal_autograd():
    mvp, verts, go = (t.double() for t in R.clip_inputs(2, 3, 41, 'real', zero_images=True))
    ref = R.clip_transform(mvp, verts, go)
    m, x = mvp.clone().requires_grad_(True), verts.clone().requires_grad_(True)
    pw = torch.cat([x, torch.ones(2, 41, 1, dtype=torch.float64)], dim=-1).repeat_interleave(3, dim=0)
    out = torch.matmul(pw, m.transpose(1, 2))
    out.backward(go)
    _close(ref['out'][0], out.detach(), ref['out'][1])
    _close(ref['g_verts'][0], x.grad, ref['g_verts'][1].clamp(min=1e-300))
    _close(ref['g_mvp'][0], m.grad, ref['g_mvp'][1].clamp(min=1e-300))
    # the images without an upstream: view 0 of both frames and all of frame 1
    assert int((ref['g_mvp'][1] == 0).sum()) == 16 * 4 and int((ref['g_verts'][1] == 0).sum()) == 41 * 3


def test_face_laplacian_equals_the_dense_form_and_penalty_gradient_equals_autograd():
    from fpc_diffrend_amd import scene
    sc = scene.cfg('cfg1', n_frames=3)
    V = sc.n_vertices
    fl = R.FaceLaplacian(sc.pos_idx, V)
    # the dense form of test_laplacian_gather_form_matches_dense, in float64
    f = np.asarray(sc.pos_idx, dtype=np.int64)
    e = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0), axis=1), axis=0)
    A = torch.zeros(V, V, dtype=torch.float64)
    A[e[:, 0], e[:, 1]] = 1
    A[e[:, 1], e[:, 0]] = 1
    L = A / A.sum(1, keepdim=True).clamp(min=1) - torch.eye(V, dtype=torch.float64)
    assert torch.allclose(fl.dense(), L, rtol=1e-15, atol=1e-300)
    g = torch.Generator().manual_seed(0)
    x = torch.tensor(sc.v_base).reshape(1, -1, 3).double() + 0.1 * torch.randn(3, V, 3, generator=g, dtype=torch.float64)
    lap, S = fl.apply(x)
    _close(lap, torch.matmul(L[None], x), S)
    lt, St = fl.apply(x, transpose=True)
    _close(lt, torch.matmul(L.t()[None], x), St)
    # the penalty in stages == autograd of the whole expression; also with vertices whose Laplacian is exactly 0 and an isolated one
    meshes = R.lap_meshes(g)
    for name, (faces, Vm, pos, _) in [('cfg1', (sc.pos_idx, V, None, None))] + [(k, meshes[k]) for k in ('grid', 'isolated', 'fan9')]:
        flm = R.FaceLaplacian(faces, Vm)
        xm = x if pos is None else pos.double()[None].repeat(2, 1, 1) * torch.tensor([1.0, 2.0])[:, None, None]
        leaf = xm.clone().requires_grad_(True)
        val = R.penalty_plain(leaf, flm.dense(), 7.5)
        (val * 0.3).backward()
        lapm = torch.matmul(flm.dense()[None], xm)      # (the backward divides by ||lap||: from the very Laplacian autograd sees)
        _close(flm.apply(xm)[0], lapm, flm.apply(xm)[1].clamp(min=1e-300))
        per, value = R.penalty_value(lapm, 7.5)
        val = val.detach()
        assert abs(float(value) - float(val)) <= 1e-12 * abs(float(val))
        assert abs(float(R.penalty_value_from_per(per, 7.5)) - float(val)) <= 1e-12 * abs(float(val))
        gr, Sg = R.penalty_grad(lapm, per, flm, 7.5, upstream=0.3)
        assert bool(torch.isfinite(gr).all())
        _close(gr, leaf.grad, Sg.clamp(min=1e-300))
        if name == 'grid':
            assert int((lapm.norm(dim=2) < 1e-14).sum()) == 2 * 9      # the 3 x 3 interior of both copies: 0 but for 1 / 6
            assert R.closed_ring_zero_count(flm, xm) == 2 * 25          # z = 0 everywhere: no term at all in that component


def test_meshes_have_the_degrees_named():
    g = torch.Generator().manual_seed(1)
    for name, (faces, V, pos, degs) in R.lap_meshes(g).items():
        fl = R.FaceLaplacian(faces, V)
        assert pos.shape == (V, 3)
        for v, d in degs.items():
            assert int(fl.deg[v]) == d, (name, v)
    faces, V, pos = R.uv_sphere()
    fl = R.FaceLaplacian(faces, V)
    assert int((fl.deg == 5).sum()) == 240 and int((fl.deg == 6).sum()) == V - 242      # (the rings next to the poles: 5)
    assert V == 15002 and int(fl.deg[0]) == 120 and int(fl.deg[V - 1]) == 120 and int(np.sort(fl.deg)[-3]) == 6


def test_pixel_loss_gradient_equals_autograd_and_background_sums_agree():
    colour, cover, ref = R.pixel_inputs(2, 9, 11, 3)
    res = R.pixel_loss(colour, cover, ref)
    leaf = colour.double().requires_grad_(True)
    bg = torch.tensor(float(np.float32(R.BACKGROUND)), dtype=torch.float64)
    col = torch.where(cover[..., None] > 0, leaf, bg)
    ssum = ((ref[..., None].double() - col * 255) ** 2).sum()
    (ssum * float(np.float32(1.0 / colour.numel()))).backward()
    ssum = ssum.detach()
    assert abs(float(res['sum'][0]) - float(ssum)) <= 1e-12 * float(ssum)
    _close(res['grad'][0], leaf.grad, res['grad'][1].clamp(min=1e-300))
    assert int((res['grad'][1] == 0).sum()) == 3 * int((cover <= 0).sum())
    img = torch.randint(0, 256, (3, 7, 13), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    exact = R.bg_sumsq_int(img, 45.0)
    v, S = R.bg_sumsq(img, 45.0)
    assert torch.equal(v, exact.double())
    assert float(np.float32(R.BACKGROUND) * np.float32(255.0)) == 45.0      # what ops.reference_background_sumsq hands the kernel
    val, S = R.objective_value(torch.tensor([1.5, 2.5, 3.0], dtype=torch.float64), 4.0, 0.5, 2.0)
    assert val == 4.5 and S == 4.5


# ---------------------------------------------------------------------------------------------------------------------
# float32 torch on the GPU file's inputs: the bounds are reachable
# ---------------------------------------------------------------------------------------------------------------------

def _e32(fn, *args, **kw):
    r64, r32 = fn(*args, **kw), fn(*args, dtype=torch.float32, **kw)
    return {k: R.measure(r32[k][0], r64[k][0], r64[k][1])[0] for k in r64}


@pytest.mark.parametrize("M,K,F", R.BLEND_SHAPES)
def test_float32_blend_meets_the_bounds(M, K, F):
    e = _e32(R.blend, *R.blend_inputs(M, K, F))
    assert e['out'] <= K + 1 + 2 and e['g_B'] <= F + 2 and e['g_vb'] <= F + 2, e
    assert e['g_w'] < 8, e                                  # the long sum (over M)


def test_float32_rig_weights_meet_the_bounds():
    for ids in R.rig_ids(32):
        Fb = len(R.rig_columns(ids, 32))
        e = _e32(R.rig_weights, *R.rig_inputs(150, 32, 32, Fb)[:2], ids, R.rig_inputs(150, 32, 32, Fb)[2])
        assert e['w'] <= 32 + 2 and e['g_mi'] < 8 and e['g_maps'] < 8, e
    ids = torch.arange(130) * 7 % 70
    mi, maps, go = R.rig_inputs(151, 70, 70, 130)
    e = _e32(R.rig_weights, mi, maps, ids, go)
    assert e['w'] <= 70 + 2 and e['g_mi'] < 8 and e['g_maps'] < 8, e


@pytest.mark.parametrize("F,Nc,V", R.CLIP_SHAPES)
@pytest.mark.parametrize("kind,zero_images", [('randn', False), ('real', False), ('randn', True)])
def test_float32_clip_transform_meets_the_bounds(F, Nc, V, kind, zero_images):
    e = _e32(R.clip_transform, *R.clip_inputs(F, Nc, V, kind, zero_images=zero_images))
    assert e['out'] <= 4 + 2 and e['g_verts'] <= 4 * Nc + 2, e
    assert e['g_mvp'] < 8, e


def _cfg1_cameras(t):
    from fpc_diffrend_amd import scene
    from helpers import scene_cameras
    t = list(t)
    t[4], t[5] = scene_cameras(scene.cfg('cfg1', n_frames=2), [i % 9 for i in range(t[4].shape[0])])
    return t


@pytest.mark.parametrize("Fb,Nc", R.MVP_SHAPES)
@pytest.mark.parametrize("kind", ['randn', 'camera', 'cfg1'])
def test_float32_mvp_chain_meets_the_bounds(Fb, Nc, kind):
    t = R.mvp_inputs(Fb, Nc, 'camera' if kind == 'cfg1' else kind)
    qc, tc, qf, tf, P, MV, go = _cfg1_cameras(t) if kind == 'cfg1' else t
    r64 = R.mvp_chain(qc, tc, qf, tf, P, MV, go)
    r32 = R.mvp_chain(qc, tc, qf, tf, P, MV, go, dtype=torch.float32)
    e = {k: R.measure(r32[k][0], r64[k][0], r64[k][1])[0] for k in r64}
    assert e['mvp'] <= R.MVP_N_VALUE + 2, e
    assert e['g_q_cam'] <= R.MVP_N_GRAD + Fb + 2 and e['g_t_cam'] <= R.MVP_N_GRAD + Fb + 2, e
    assert e['g_q_frame'] <= R.MVP_N_GRAD + Nc + 2 and e['g_t_frame'] <= R.MVP_N_GRAD + Nc + 2, e


@pytest.mark.parametrize("kind", ['randn', 'cfg1'])
def test_float32_indexed_mvp_chain_meets_the_bounds(kind):
    for name, nf, ncam, nv, fi, vi, cov in R.mvp_index_cases(torch.Generator().manual_seed(7)):
        Fb, Nc = (len(fi) if fi is not None else nf), (len(vi) if vi is not None else nv)
        t = R.mvp_inputs(Fb, Nc, 'camera' if kind == 'cfg1' else kind, n_frames=nf, n_cams=ncam, n_views=nv)
        qc, tc, qf, tf, P, MV, go = _cfg1_cameras(t) if kind == 'cfg1' else t
        r64 = R.mvp_chain(qc, tc, qf, tf, P, MV, go, fi, vi, cov, Fb, Nc)
        r32 = R.mvp_chain(qc, tc, qf, tf, P, MV, go, fi, vi, cov, Fb, Nc, dtype=torch.float32)
        e = {k: R.measure(r32[k][0], r64[k][0], r64[k][1])[0] for k in r64}
        assert e['mvp'] <= R.MVP_N_VALUE + 2 and max(e.values()) <= R.MVP_N_GRAD + 2 * Fb * Nc + 2, (name, e)


def test_float32_laplacian_and_penalty_meet_the_bounds():
    g = torch.Generator().manual_seed(5)
    meshes = R.lap_meshes(g)
    faces, V, pos = R.uv_sphere()
    meshes['sphere'] = (faces, V, pos, None)
    from fpc_diffrend_amd import scene
    sc = scene.cfg('cfg1', n_frames=1)
    meshes['cfg1'] = (sc.pos_idx, sc.n_vertices, torch.tensor(sc.v_base).reshape(-1, 3), None)
    for name, (faces, V, pos, _) in meshes.items():
        fl = R.FaceLaplacian(faces, V)
        dmax = int(fl.deg.max())
        x = pos[None].repeat(3, 1, 1) + 0.05 * torch.randn(3, V, 3, generator=g) * (name != 'grid')
        lap64, S = fl.apply(x)
        lap32, _ = fl.apply(x, dtype=torch.float32)
        assert R.measure(lap32, lap64, S)[0] <= dmax + 2 + 2, name
        per64, _ = R.penalty_value(lap32, 7.5)
        per32, _ = R.penalty_value(lap32, 7.5, dtype=torch.float32)
        assert R.measure(per32, per64, per64)[0] < 8, name
        g64, Sg = R.penalty_grad(lap32, per32, fl, 7.5, 0.3)
        g32, _ = R.penalty_grad(lap32, per32, fl, 7.5, 0.3, dtype=torch.float32)
        assert R.measure(g32, g64, Sg)[0] <= dmax + R.LAP_N_GRAD + 2, name


@pytest.mark.parametrize("B,H,W,C", [(3, 37, 53, 1), (2, 37, 53, 3)])
def test_float32_pixel_loss_meets_the_bounds(B, H, W, C):
    colour, cover, ref = R.pixel_inputs(B, H, W, C)
    cov = float((cover > 0).float().mean())
    assert 0.3 <= cov <= 0.7
    r64, r32 = R.pixel_loss(colour, cover, ref), R.pixel_loss(colour, cover, ref, dtype=torch.float32)
    assert R.measure(r32['grad'][0], *r64['grad'])[0] <= R.PIXEL_N_GRAD + 2
    assert R.measure(r32['sum'][0], *r64['sum'])[0] < 8
    img = torch.randint(0, 256, (3, 37, 53), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    v64, S = R.bg_sumsq(img, 44.7)
    v32, _ = R.bg_sumsq(img, 44.7, dtype=torch.float32)
    assert R.measure(v32, v64, S)[0] < 8

"""GPU: the bending term (csrc/mesh_reg.hip k_bend_hinges, k_bend_gather, k_penalty_finish; fit.MeshTopology.hinges(), RestShape.bend_cs,
fit.bend_penalty, FitConfig.weight_bend) entry by entry against float64 (tests/bend_ref.py), and inside a Fitter: eager, under a captured
graph, on two ranks.

The convention is tests/test_gpu_rest.py's: the error of an output x with float64 reference r is e = max_i |x_i - r_i| / S_i in units of
u = 2^-24, S_i the first-order scale of entry i (bend_ref's docstring); every output is held to the long-sum bar e <= 8 * e32 + 4, e32 the
error of float32 torch on the CPU on the same statement.  Entries with S_i = 0 have no term, must be exactly 0, and their number must be
the one the case predicts from its topology.  Positions sit at y + 170, so S carries the 170 through `p1 - p0` into everything behind
the normals and the scaled errors are small numbers; the relative L2 against float64, printed beside them and held to the project's
1e-4, is the figure that would show a lost corner.  It is not taken where the reference itself is rounding: with a table at x = x_rest
exactly (sin delta is one float32 rounding from 0; the term is rounding squared there, which the test holds to (2^-20)^2 instead).
Every line is printed as "BEND case name e_gpu e32 bound" / "BEND case rel-L2 ..." (pytest -s).

Measured on an MI355X (units of u; the largest over the cases of a row -- every case runs with and without a rest table; the last but one
column is the case that came closest to its own bound, the last the largest relative L2 against float64 over the cases where it is
taken).  The whole file runs in 17 s there, 9 s of them the two-rank test:

  output       cases max e_gpu  max e32   closest to its bound (e_gpu / bound, case)   max rel-L2 (cases, case)
  hinge_grad      84     0.120    0.120   0.120 / 5.0  fan8/F300/plain                 9.02e-06 (75, sphere/F1)
  grad_x          84     0.018    0.018   0.018 / 4.1  fan8/F300                       5.38e-06 (75, grid/F1/collapsed)
  per             84     0.004    0.002   0.004 / 4.0  grid/F1/coincident/plain        1.85e-06 (75, book/F1)
  value           84     0.004    0.002   0.004 / 4.0  grid/F1/coincident/plain        1.81e-06 (75, book/F1)
Against torch's mesh_normal_consistency on the GPU (30 cases without a table and without a degenerate hinge): value within 1.3e-5
(grid/F1), gradient rel-L2 within 9.6e-6 (fan256/F3).

Fitter (cfg1, cameras 0 and 3, four frames, init_near_truth(0.8), W_BND = 1e9; the three loss paths agree to the digits shown):
  |g_on|     |g_off|    |g_term|   |(g_on - g_off) - g_term|   1e-4 (|g_on| + |g_off|)   l_on      l_off   l_term
  9.4495e4   1.0723e4   9.3885e4   8.2e-3 .. 1.0e-2            10.5                      34283.60  4.779   34278.82
At the base mesh (mode='free', weight 100): logged BND 6.2e-14; largest gradient entry 1.6e-8 against the base mesh's angles, 7.6e-2 for
the plain term at the same weight.
Behaviour (mode='free', 30 steps from the base mesh, weight 1000, mean distance to the ground-truth vertices 0.01401 at the start):
0.02165 with the plain weight_normalconsistency term, 0.01763 with weight_bend, 0.01755 with neither.
"""
import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch

import bend_ref as B
import fitstep_ref as R
from helpers import fitter_near_truth, flat_grads as _flat_grads

pytestmark = pytest.mark.gpu


def _report(case, name, e, e32, bound):
    print(f"BEND {case} {name} e_gpu={e:.3f} e32={e32:.3f} bound={bound:.1f}")


def long_sum(case, name, x, ref, x32, zeros=0):
    r, Sc = ref
    e, nz = R.measure(x, r, Sc)
    e32, _ = R.measure(x32, r, Sc)
    _report(case, name, e, e32, 8 * e32 + 4)
    if isinstance(zeros, tuple):      # (at least: see _bend_case on the rest variant)
        assert nz >= zeros[0], (case, name, nz, zeros)
    else:
        assert nz == zeros, (case, name, nz, zeros)
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _unaligned(n, dtype=torch.float32, fill=None):
    """n elements that start one element past an allocation's base: 4 bytes off every wider alignment."""
    t = torch.empty(n + 1, dtype=dtype, device='cuda')[1:]
    if fill is not None:
        t.fill_(fill)
    return t


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(faces, V, rest positions [V,3] float32 at y + 170, hv, sigma, hinge faces, MeshTopology on the GPU, RestShape), once per mesh."""
    from fpc_diffrend_amd import fit, scene
    if name == 'cfg1':
        sc = scene.cfg('cfg1', n_frames=3)
        faces, V, pos = sc.pos_idx, sc.n_vertices, torch.tensor(sc.v_base).reshape(-1, 3)
    elif name == 'sphere':
        faces, V, pos = R.uv_sphere()
    else:
        faces, V, pos = B.small_meshes(torch.Generator().manual_seed(5))[name]
    rest = pos.clone().float()
    rest[:, 1] += 170.0
    hv, sigma = B.hinges(faces)
    topo = fit.MeshTopology(faces, V, 'cuda')
    return faces, V, rest, hv, sigma, B.hinge_faces(faces), topo, fit.RestShape(topo, rest.cuda())


def _raw_call(x, tabs, cs, weight, acc, grad=True, unaligned=False):
    """fpcdr_bend_penalty on the tables `tabs` = (hinge_vtx, hinge_inc, H, K) -> (per, out, hinge_grad as [F,H,4,3] or None, grad_x or None)."""
    from fpc_diffrend_amd import _lib
    hinge_vtx, hinge_inc, H, K = tabs
    F, V, _ = x.shape
    new = (lambda n: _unaligned(n, fill=float('nan'))) if unaligned else (lambda n: torch.full((n,), float('nan'), device='cuda'))
    hg, gx = (new(max(F * H * 12, 1)), new(F * V * 3)) if grad else (None, None)
    per, out = new(F), new(1)
    if unaligned:      # the inputs too: copies that start 4 bytes into their allocations
        def moved(t):
            if t is None or t.numel() == 0:
                return t
            m = _unaligned(t.numel(), dtype=t.dtype)
            m.copy_(t.reshape(-1))
            return m
        x, hinge_vtx, hinge_inc, cs = moved(x), moved(hinge_vtx), moved(hinge_inc), moved(cs)
    _lib.call("fpcdr_bend_penalty", _ptr(x), _ptr(hinge_vtx) if H else None, _ptr(cs), _ptr(hinge_inc) if grad else None,
              _ptr(hg) if (grad and H) else None, _ptr(gx), _ptr(acc), _ptr(per), _ptr(out), float(weight), F, V, H, K, _stream())
    assert bool((acc == 0).all())                          # the call leaves its accumulators zeroed
    return per, out, (_corners(hg, F, H) if grad else None), (gx.reshape(F, V, 3) if grad else None)


def _corners(buf, F, H):
    """The hinge_grad scratch [F,4,3,H] (role, component, hinge) as [F,H,4,3]."""
    return buf[:F * H * 12].reshape(F, 4, 3, H).permute(0, 3, 1, 2).contiguous()


def _positions(name, F, seed, variant):
    """-> (x [F,V,3] float32, the hinges the variant makes degenerate (predicted from the topology alone))."""
    faces, V, rest, hv, sigma, hf, topo, rs = _mesh(name)
    gen = torch.Generator().manual_seed(seed)
    H = hv.shape[0]
    x = rest[None].repeat(F, 1, 1)
    if variant != 'rest':
        x = x + 0.05 * torch.randn(F, V, 3, generator=gen)
    dead_faces = set()
    fset = [set(t) for t in np.asarray(faces).tolist()]
    if variant == 'coincident':        # the two ends of hinge 0's edge at one point: every face that holds both has no area
        a, b = int(hv[0, 0]), int(hv[0, 1])
        x[:, b] = x[:, a]
        dead_faces = {i for i, s in enumerate(fset) if a in s and b in s}
    elif variant == 'collapsed':       # f0's third vertex onto the line of its edge, EXACTLY: the ends snapped to multiples of 2^-10,
        h = H // 2                     # q0 = p0 + 2 (p1 - p0) is then a float32 and e x (q0 - p0) = e x 2 e = 0 in any precision
        p0, p1, q0 = (int(hv[h, r]) for r in range(3))
        snap = lambda t: (torch.round(t.double() * 1024.0) / 1024.0).float()
        x[:, p0], x[:, p1] = snap(x[:, p0]), snap(x[:, p1])
        x[:, q0] = x[:, p0] + 2.0 * (x[:, p1] - x[:, p0])
        dead_faces = {int(hf[h, 0])}
    elif variant == 'folded':          # f0's third vertex of a few hinges turned 2 rad about the edge
        for h in sorted({H // 3, (2 * H) // 3, H - 1}):
            p0, p1, q0 = (x[:, int(hv[h, r])].double() for r in range(3))
            k = (p1 - p0) / (p1 - p0).norm(dim=1, keepdim=True)
            v = q0 - p0
            turned = v * math.cos(2.0) + torch.cross(k, v, dim=1) * math.sin(2.0) + k * (k * v).sum(1, keepdim=True) * (1.0 - math.cos(2.0))
            x[:, int(hv[h, 2])] = (p0 + turned).float()
    dead = [h for h in range(H) if int(hf[h, 0]) in dead_faces or int(hf[h, 1]) in dead_faces]
    return x, dead


def _bend_case(name, F, seed, variant='noise'):
    from fpc_diffrend_amd import fit
    faces, V, rest, hv, sigma, hf, topo, rs = _mesh(name)
    tabs = topo.hinges()
    H = tabs[2]
    assert H == hv.shape[0] and torch.equal(tabs[0].cpu(), B.packed(hv, sigma))
    cs_cpu = rs.bend_cs.cpu()      # the table the kernel reads; two float64 evaluations may round to neighbouring float32s
    assert cs_cpu.shape == (2, H) and (H == 0 or float((cs_cpu - B.rest_cs(rest, hv, sigma)).abs().max()) <= 2.0 ** -23)
    x, dead = _positions(name, F, seed, variant)
    xc = x.cuda()
    weight, upstream = 7.5, 0.3
    # what the case predicts from its topology: the degenerate hinges, the vertices none of whose corners is at a live hinge
    live_h = torch.ones(H, dtype=torch.bool)
    live_h[dead] = False
    has_term = torch.zeros(V, dtype=torch.bool)
    has_term[hv[live_h].reshape(-1)] = True
    n_bare = int((~has_term).sum())
    flat = name == 'grid' and variant == 'rest'      # z = 0 everywhere: sin theta, its scale and every gradient entry are exactly 0
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    for table in (True, False):
        case = f"{name}/F{F}" + ('' if variant == 'noise' else '/' + variant) + ('' if table else '/plain')
        cs, cs_gpu = (cs_cpu, rs.bend_cs) if table else (None, None)
        ref, ref32 = B.bend(x, hv, sigma, cs, weight), B.bend(x, hv, sigma, cs, weight, dtype=torch.float32)
        # (i) the statement alone: the case reaches what it claims to reach, in float64 and in float32
        for st in (ref, ref32):
            assert int((~st['live']).sum()) == F * len(dead), (case, int((~st['live']).sum()), len(dead))
            assert bool((st['live'] == live_h[None]).all()), case
        if variant in ('coincident', 'collapsed'):
            assert len(dead) >= 1, case
        if variant == 'folded':
            assert bool((ref['cosd'] <= 0).any()) and bool((ref['cosd'] > 0).any()), case
        assert int((ref['grad'][1].abs().sum(dim=2) == 0).sum()) == (F * V if flat else F * n_bare), case      # vertices without a term
        # (ii) the C entry, every buffer at an unaligned base
        per, out, hg, gx = _raw_call(xc, tabs, cs_gpu, weight, acc, unaligned=True)
        z_hg, z_gx = (F * H * 12, F * V * 3) if flat else (F * len(dead) * 12, F * n_bare * 3)
        if variant == 'rest' and not flat:
            # x = rest exactly keeps the rest mesh's exact zeros (cfg1's vertices on its symmetry plane x = 0): entries whose every product
            # has a zero factor have S = 0 beyond the ones the topology predicts.  measure() still holds each of them to exactly 0.
            z_hg, z_gx = (z_hg,), (z_gx,)
        z_val = H == 0 or flat
        long_sum(case, 'hinge_grad', hg, ref['hinge_grad'], ref32['hinge_grad'][0], zeros=z_hg)
        long_sum(case, 'grad_x', gx, ref['grad'], ref32['grad'][0], zeros=z_gx)
        long_sum(case, 'per', per, ref['per'], ref32['per'][0], zeros=F if z_val else 0)
        long_sum(case, 'value', out, tuple(t.reshape(1) for t in ref['value']), ref32['value'][0].reshape(1), zeros=1 if z_val else 0)
        assert int((gx == 0).all(dim=2).sum()) >= F * n_bare
        if H == 0:
            assert float(out) == 0.0 and float(per.abs().max()) == 0.0 and float(gx.abs().max()) == 0.0
        if variant == 'rest' and table:      # rounding squared: sin delta within 2^-20 of 0 (the angle's conditioning at y + 170)
            assert float(per.max()) <= (2.0 ** -20) ** 2, (case, float(per.max()))
        elif H:
            rl = [R.rel_l2(hg, ref['hinge_grad'][0]), R.rel_l2(gx, ref['grad'][0]), R.rel_l2(per, ref['per'][0]), R.rel_l2(out, ref['value'][0])]
            print(f"BEND {case} rel-L2 hinge_grad={rl[0]:.2e} grad_x={rl[1]:.2e} per={rl[2]:.2e} value={rl[3]:.2e}")
            assert max(rl) < 1e-4, (case, rl)
        # (iii) determinism: the gradient buffers bit for bit; a value-only call to one float32 ulp (the double adds may reorder)
        per2, out2, hg2, gx2 = _raw_call(xc, tabs, cs_gpu, weight, acc)
        assert torch.equal(hg2, hg) and torch.equal(gx2, gx), case
        per_v, out_v, _, _ = _raw_call(xc, tabs, cs_gpu, weight, acc, grad=False)
        for a, b in ((per_v, per), (out_v, out), (per2, per), (out2, out)):
            assert bool(((a - b).abs() <= 2.0 ** -23 * b.abs()).all()), case
        # (iv) fit.bend_penalty: lazy, eager with a unit upstream, eager with a factor, on the caller's acc and scratch
        scratch = _unaligned(max(F * H * 12, 1))
        for kw, upv in ((dict(), upstream), (dict(eager_grad=True, unit_upstream=True), 1.0), (dict(eager_grad=True), upstream),
                        (dict(acc=acc, scratch=scratch), upstream)):
            leaf = x.cuda().requires_grad_(True)
            value = fit.bend_penalty(leaf, topo, weight, rest=rs if table else None, **kw)
            (value * upv).backward() if upv != 1.0 else value.backward()
            assert abs(float(value.detach()) - float(out)) <= 2.0 ** -23 * abs(float(out)), (case, kw)
            want = gx if upv == 1.0 else gx * torch.tensor(upv, dtype=torch.float32, device='cuda')
            assert torch.equal(leaf.grad, want), (case, kw)
            assert bool((acc == 0).all())
        assert torch.equal(_corners(scratch, F, H), hg), case
        with torch.no_grad():
            assert abs(float(fit.bend_penalty(xc, topo, weight, rest=rs if table else None)) - float(out)) <= 2.0 ** -23 * abs(float(out))
        # (v) without a table it is weight * mesh_normal_consistency (torch's clamp differs at a degenerate hinge: DESIGN.md 3)
        if not table and not dead and H:
            leaf = x.cuda().requires_grad_(True)
            mnc = weight * fit.mesh_normal_consistency(leaf, topo)
            mnc.backward()
            rv = abs(float(out) - float(mnc)) / max(abs(float(mnc)), 1e-300)
            rg = R.rel_l2(gx, leaf.grad) if float(leaf.grad.abs().max()) > 0 else float(gx.abs().max())
            print(f"BEND {case} against torch's mesh_normal_consistency: value {rv:.2e} grad rel-L2 {rg:.2e}")
            if not (variant == 'rest' and name == 'grid'):
                assert rv < 1e-4 and rg < 1e-4, (case, rv, rg)


@pytest.mark.parametrize("name", ['triangle', 'two_pos', 'two_neg', 'book', 'fan8', 'fan73', 'fan256', 'grid', 'isolated'])
def test_bend_entries_against_float64_small_meshes(name):
    for F in (1, 3):
        _bend_case(name, F, seed=20 + F)


def test_bend_with_more_meshes_than_the_finish_kernels_threads():
    _bend_case('fan8', 300, seed=30)


@pytest.mark.parametrize("name", ['cfg1', 'sphere'])       # the sphere: 15002 vertices, two poles with 240 corners each
def test_bend_entries_against_float64_cfg1_and_sphere(name):
    for F in (1, 3):
        _bend_case(name, F, seed=40 + F)


@pytest.mark.parametrize("variant", ['rest', 'coincident', 'collapsed', 'folded'])
def test_bend_at_the_rest_shape_degenerate_and_folded(variant):
    """x = rest exactly: rounding squared with a table.  Two vertices at one point, a face without area: t = 1, no gradient, nothing
    turns NaN, and the zeros are counted.  Hinges turned 2 rad: the 1 - cos branch runs beside the stable one."""
    for name, F in (('cfg1', 3), ('fan73', 1), ('book', 1), ('isolated', 1), ('grid', 1)):
        if variant == 'folded' and name == 'book':
            continue      # (one hinge: it cannot be on both branches)
        _bend_case(name, F, seed=50, variant=variant)


# ---------------------------------------------------------------------------------------------------------------------
# inside a Fitter
# ---------------------------------------------------------------------------------------------------------------------

# the weight at which the term's parameter gradient is at least a tenth of the pixel term's at init_near_truth(0.8) (asserted below): large
# because the pixel term's gradient is mostly the poses', which the term does not reach, and because 0.8 of the truth bends little
W_BND = 1.0e9


def _fitter(**kw):
    return fitter_near_truth(4, **{'optimize_texture': False, **kw})


def test_fitter_without_the_weight_builds_nothing():
    ft = _fitter()
    assert ft.cfg.weight_bend == 0.0 and ft.rest is None and ft.topo._hinges is None and ft._reg_terms == [] and ft._bnd_scratch is None
    ft.loss_and_backward(slice(0, 4))
    assert ft.rest is None and ft.topo._hinges is None


@pytest.mark.parametrize("path", ['one_pass', 'operator', 'torch'])
def test_fitter_gradient_is_the_pixel_terms_plus_the_op(path):
    """g_on - g_off = g_term to the project's float bar (1e-4 of the gradients' size) on the one-pass path, the operator path and the torch
    chain; the term is at least a tenth of the pixel gradient, so a missing term cannot pass.  The same for the loss values."""
    from fpc_diffrend_amd import fit
    kw = {'one_pass': dict(), 'operator': dict(fused_objective=False), 'torch': dict(fused_loss=False)}[path]
    frames = slice(0, 4)
    ft_on, ft_off = _fitter(weight_bend=W_BND, **kw), _fitter(**kw)
    assert ft_off.rest is None and ft_on.rest is not None and ft_on._bnd_scratch.numel() == 4 * 1536 * 12
    l_on, l_off = float(ft_on.loss_and_backward(frames)), float(ft_off.loss_and_backward(frames))
    assert bool((ft_on._reg_acc == 0).all())
    g_on, g_off = _flat_grads(ft_on), _flat_grads(ft_off)
    ft_on.optimizer.zero_grad(set_to_none=True)
    v = ft_on.vertices(frames).reshape(4, -1, 3)
    term = fit.bend_penalty(v, ft_on.topo, W_BND, rest=ft_on.rest)
    term.backward()
    g_term, l_term = _flat_grads(ft_on), float(term.detach())
    n_on, n_off, n_term = float(g_on.norm()), float(g_off.norm()), float(g_term.norm())
    err = float(((g_on - g_off) - g_term).norm())
    print(f"BEND fitter/{path} |g_on|={n_on:.4e} |g_off|={n_off:.4e} |g_term|={n_term:.4e} err={err:.3e} "
          f"l_on={l_on:.6e} l_off={l_off:.6e} l_term={l_term:.6e}")
    assert n_term >= 0.1 * n_off
    assert err <= 1e-4 * (n_on + n_off)
    assert abs((l_on - l_off) - l_term) <= 1e-4 * (abs(l_on) + abs(l_off))


@pytest.mark.parametrize("mode,fps", [("prior", 0), ("combined", 2)])
def test_hip_graph_steps_equal_eager_steps_with_the_bend_term(mode, fps):
    """The configuration and tolerances of test_gpu_rest.test_hip_graph_steps_equal_eager_steps_with_the_rest_terms, with the bending term
    on: no host sync, no per-call fill or allocation, so it replays."""
    from fpc_diffrend_amd import fit, scene
    traj = {}
    for graph in (False, True):
        sc = scene.cfg('cfg1', n_frames=4)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=14, cam_idxs=(0, 3), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, mode=mode, frames_per_step=fps,
                            hip_graph=graph, weight_laplacian=20.0, weight_bend=2.0e4)
        ft = fit.Fitter(sc, cfg, device='cuda')
        if mode == "prior":
            ft.init_near_truth(0.8)
        traj[graph] = [float(ft.step()) for _ in range(14)]
        if graph:
            assert ft._graphs is not None
        assert bool((ft._reg_acc == 0).all())      # (the one buffer of the Laplacian and the bending term)
    a, b = np.asarray(traj[False]), np.asarray(traj[True])
    assert np.isfinite(b).all()
    assert np.allclose(a, b, rtol=2e-3), (a, b)
    assert np.allclose(a[:5], b[:5], rtol=1e-5), (a, b)


def test_two_rank_fitter_with_the_bend_term_equals_single_process(tmp_path, monkeypatch):
    """tests/test_gpu_dist.py's two-rank run with weight_bend in the place of its weight_meshedge: the term's weight carries the
    1 / world, the replicas stay bit-identical and equal the single process."""
    import test_gpu_dist as D
    assert "weight_meshedge=0.3" in D.CHILD
    monkeypatch.setattr(D, "CHILD", D.CHILD.replace("weight_meshedge=0.3", "weight_bend=2.0e4"))
    steps = 3
    D._run(tmp_path, 2, False, steps)
    D._run(tmp_path, 1, False, steps)
    a, b = (torch.load(tmp_path / f"w2_r{r}.pt") for r in (0, 1))
    one = torch.load(tmp_path / "w1_r0.pt")
    for k, (p, q) in enumerate(zip(a["params"], b["params"])):
        assert torch.equal(p, q), (k, float((p - q).abs().max()))
    assert np.allclose(a["losses"], one["losses"], rtol=1e-5), (a["losses"], one["losses"])
    for k, (p, q) in enumerate(zip(a["params"], one["params"])):
        if k == 9:
            continue        # (the texture: the term does not reach it; test_gpu_dist.py holds it to its own share rule)
        dmax = float((p - q).abs().max())
        assert dmax <= 1e-5 * max(1.0, float(q.abs().max())), (k, tuple(p.shape), dmax)
    assert float((a["result"] - one["result"]).abs().max()) < 1e-4


def test_at_the_base_mesh_the_term_rests_where_the_plain_one_pushes(tmp_path):
    """mode='free' starts at the base mesh.  At iteration 0 the logged BND is below 1e-10 and no entry of the term's gradient reaches
    1e-6, where the plain normal-consistency term at the same weight has entries beyond 1e-4 * weight (float64 on the CPU: up to 3.0e-3
    per unit weight and mesh; four meshes share the weight)."""
    from fpc_diffrend_amd import fit, scene
    weight = 100.0
    sc = scene.cfg('cfg1', n_frames=4)
    sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
    log = tmp_path / "log.jsonl"
    cfg = fit.FitConfig(max_iter=30, cam_idxs=(0, 3), mode='free', weight_laplacian=0.0, weight_bend=weight, log_interval=1,
                        reg_log_interval=1, log_path=str(log))
    ft = fit.Fitter(sc, cfg, device='cuda')
    frames = slice(0, 4)
    v = ft.vertices(frames).detach().reshape(4, -1, 3)
    assert float((v - ft.v_base.reshape(1, -1, 3)).abs().max()) == 0.0
    assert ft.iteration == 0
    ft._log_step(frames, torch.zeros((), device='cuda'))
    rec = json.loads(open(log).read().splitlines()[-1])
    print(f"BEND base mesh: logged {rec}")
    assert rec["it"] == 0 and 0.0 <= rec["BND"] < 1e-10 and rec["MNC"] == 0.0
    leaf = v.clone().requires_grad_(True)
    fit.bend_penalty(leaf, ft.topo, weight, rest=ft.rest).backward()
    g_rest = float(leaf.grad.abs().max())
    leaf = v.clone().requires_grad_(True)
    (weight * fit.mesh_normal_consistency(leaf, ft.topo)).backward()
    g_plain = float(leaf.grad.abs().max())
    print(f"BEND base mesh: largest gradient entry {g_rest:.3e} against the base mesh's angles, {g_plain:.3e} for the plain term")
    assert g_rest < 1e-6
    assert g_plain > 1e-4 * weight


def test_behaviour_of_thirty_free_steps_is_recorded():
    """mode='free' on cfg1, 30 steps from the base mesh, weight 1000: the mean distance to the ground-truth vertices with the plain
    normal-consistency term, with weight_bend, and with neither.  Recorded in the module docstring; only finiteness is asserted."""
    from fpc_diffrend_amd import fit, scene
    dist = {}
    for tag, kw in (('plain', dict(weight_normalconsistency=1000.0)), ('bend', dict(weight_bend=1000.0)), ('neither', dict())):
        sc = scene.cfg('cfg1', n_frames=4)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=30, cam_idxs=(0, 3), mode='free', weight_laplacian=0.0, **kw)
        ft = fit.Fitter(sc, cfg, device='cuda')
        ft.init_near_truth(0.8)
        truth = (torch.tensor(sc.v_base)[None] + torch.tensor(sc.weights_gt) @ torch.tensor(sc.blendshapes).t()).reshape(4, -1, 3).cuda()
        start = float((ft.vertices(slice(0, 4)).detach().reshape(4, -1, 3) - truth).norm(dim=2).mean())
        for _ in range(30):
            ft.step()
        dist[tag] = float((ft.result.reshape(4, -1, 3) - truth).norm(dim=2).mean())
        print(f"BEND behaviour {tag}: mean distance to the truth: start {start:.5f} after 30 steps {dist[tag]:.5f}")
    assert all(math.isfinite(d) for d in dist.values()), dist

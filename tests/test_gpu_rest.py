"""GPU: the rest-shape regularisers (csrc/mesh_reg.hip k_lap_penalty_fwd<true>, k_stretch_penalty, k_penalty_finish; fit.RestShape,
laplacian_penalty(rest=), stretch_penalty, FitConfig.laplacian_relative / weight_stretch) entry by entry against float64
(tests/rest_ref.py, tests/fitstep_ref.py), and inside a Fitter: eager, under a captured graph, on two ranks.

The convention is tests/test_gpu_fitstep.py's: the error of an output x with float64 reference r is e = max_i |x_i - r_i| / S_i in units
of u = 2^-24, S_i the sum of the absolute values of the terms of entry i (every subtraction charges the absolute values of its operands:
positions sit at y + 170, so `x_n - x_v` and `len - l` cancel for real); entries with S_i = 0 have no term, must be exactly 0, and their
number must be the one the mesh predicts.
  short paths: rest_lap = L x_rest (degree + 2 rounded operations, as fitstep's L x) and d = L x - rest_lap (one more subtraction:
               degree + 3) must have e <= n + 2;  the value from per_f: LAP_N_VALUE.
  sums and chains through a root and a division (per_f of both terms, stretch value and gradient): e <= 8 * e32 + 4, e32 the error of
               float32 torch on the CPU for the same expression against the same reference.
  the Laplacian's backward is the existing kernel fed d: fitstep's bound, LAP_N_GRAD + degree.
Every line is printed as "REST case name e_gpu e32 bound" (pytest -s).

Measured on an MI355X (units of u; the largest over the 29 cases of a row -- 58 where a case makes two calls; e32 "-": the bound is
derived, no yardstick is measured; the last column is the case that came closest to its own bound).  The stretch rows are small
because their scales carry the 170 of the positions twice (`x_n - x_v`, then `len - l`); the rel-L2 of the same outputs against float64,
printed beside them and held to the project's 1e-4, is the figure that would show a lost slot.  The whole file runs in 16 s there:

  output                                 cases max e_gpu  max e32   closest to its bound (e_gpu / bound, case)
  rest_lap                                  29      2.67        -   1.28 / 12.0  fan8/F1
  d                                         29      3.48        -   1.32 / 11.0  grid/F3
  per                                       29      1.91     2.25   1.91 / 20.9  fan73/F300
  value                                     29      2.63        -   2.63 / 5.0  isolated/F1/coincident
  lap lazy value                            29      3.38     3.21   3.38 / 7.5  isolated/F1/coincident
  lap lazy grad                             29      4.16        -   2.17 / 20.0  grid/F1
  lap eager_grad,unit_upstream value        29      3.38     3.21   3.38 / 7.5  isolated/F1/coincident
  lap eager_grad,unit_upstream grad         29      4.14        -   2.96 / 20.0  grid/F3
  lap eager_grad value                      29      3.38     3.21   3.38 / 7.5  isolated/F1/coincident
  lap eager_grad grad                       29      5.18        -   3.96 / 23.0  fan8/F3
  lap acc value                             58      3.38     3.21   3.38 / 7.5  isolated/F1/coincident
  lap acc grad                              58      4.16        -   2.17 / 20.0  grid/F1
  smoothing per                             29      2.78     2.25   1.45 / 4.1  sphere/F1
  stretch per                               58      0.00     0.00   0.00 / 4.0  fan8/F1
  stretch value                             58      0.00     0.00   0.00 / 4.0  fan8/F1
  stretch grad                              58      0.01     0.02   0.01 / 4.1  cfg1/F3/coincident/target
  stretch lazy / eager / acc value         116      0.00     0.00   0.00 / 4.0  fan8/F1
  stretch lazy / eager / acc grad          116      0.01     0.01   0.01 / 4.0  cfg1/F3

Fitter (cfg1, cameras 0 and 3, four frames, init_near_truth(0.8), W_LAP = 1e8, W_STR = 2.5e7; both loss paths agree to the digits shown):
  terms    |g_on|     |g_off|    |g_term|   |(g_on - g_off) - g_term|   1e-4 (|g_on| + |g_off|)   l_on     l_off   l_term
  lap      1.1045e4   1.0723e4   2.6472e3   4.9e-4 .. 7.8e-4            2.18                      876.350  4.779   871.570
  stretch  1.4621e4   1.0723e4   9.9397e3   1.7e-3                      2.53                      3312.98  4.779   3308.20
  both     1.6396e4   1.0723e4   1.2404e4   8.7e-4                      2.71                      4184.55  4.779   4179.77
Behaviour (mode='free', weight_laplacian 5000, 30 steps from the base mesh, mean distance to the ground-truth vertices 0.01401 at the
start): 0.02291 with the plain term, 0.01740 against the base mesh's differentials -- where the pixel term alone (weight_laplacian = 0)
ends at 0.01755: what is left of the growth is the pixel term's own first Adam steps, not the regulariser.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fitstep_ref as R
import rest_ref as S
from helpers import fitter_near_truth, flat_grads as _flat_grads

pytestmark = pytest.mark.gpu


def _report(case, name, e, e32, bound):
    print(f"REST {case} {name} e_gpu={e:.3f} e32={'-' if e32 is None else format(e32, '.3f')} bound={bound:.1f}")


def short(case, name, x, ref, n, zeros=0):
    r, Sc = ref
    e, nz = R.measure(x, r, Sc)
    nmax = float(n.max()) if torch.is_tensor(n) else float(n)
    _report(case, name, e, None, nmax + 2)
    assert nz == zeros, (case, name, nz, zeros)
    if torch.is_tensor(n):
        worst, _ = R.measure(x, r, Sc * (n.to(torch.float64) + 2.0))
        assert worst <= 1.0, (case, name, worst)
    assert e <= nmax + 2, (case, name, e)


def long_sum(case, name, x, ref, x32, zeros=0):
    r, Sc = ref
    e, nz = R.measure(x, r, Sc)
    e32, _ = R.measure(x32, r, Sc)
    _report(case, name, e, e32, 8 * e32 + 4)
    assert nz == zeros, (case, name, nz, zeros)
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(faces, V, rest positions [V,3] float32 at y + 170, FaceLaplacian, MeshTopology on the GPU, RestShape), made once per mesh."""
    from fpc_diffrend_amd import fit, scene
    if name == 'cfg1':
        sc = scene.cfg('cfg1', n_frames=3)
        faces, V, pos = sc.pos_idx, sc.n_vertices, torch.tensor(sc.v_base).reshape(-1, 3)
    elif name == 'sphere':
        faces, V, pos = R.uv_sphere()
    else:
        faces, V, pos, _ = R.lap_meshes(torch.Generator().manual_seed(5))[name]
    rest = pos.clone().float()
    rest[:, 1] += 170.0
    fl = R.FaceLaplacian(faces, V)
    topo = fit.MeshTopology(faces, V, 'cuda')
    return faces, V, rest, fl, topo, fit.RestShape(topo, rest.cuda())


def _stretch_call(x, topo, rest_len, target, weight, E, acc, grad=True):
    from fpc_diffrend_amd import _lib
    F, V, _ = x.shape
    gx = torch.full_like(x, float('nan')) if grad else None
    per = torch.empty(F, dtype=torch.float32, device='cuda')
    val = torch.empty((), dtype=torch.float32, device='cuda')
    _lib.call("fpcdr_stretch_penalty", _ptr(x), _ptr(topo.nbr32), _ptr(rest_len), float(target), _ptr(gx), _ptr(acc), _ptr(per), _ptr(val),
              float(weight), F, V, topo.nbr32.shape[0], E, _stream())
    assert bool((acc == 0).all())                          # the call leaves its accumulators zeroed
    return per, val, gx


def _rest_case(name, F, seed, variant='noise'):
    """variant: 'noise' x = rest + 0.05 randn;  'rest' x = rest exactly;  'coincident' two adjacent vertices at one position."""
    from fpc_diffrend_amd import _lib, fit
    faces, V, rest, fl, topo, rs = _mesh(name)
    D = topo.nbr32.shape[0]
    gen = torch.Generator().manual_seed(seed)
    case = f"{name}/F{F}" + ('' if variant == 'noise' else '/' + variant)
    deg = torch.tensor(fl.deg, dtype=torch.float64)[None, :, None].expand(F, V, 3)
    n_isolated = int((fl.deg == 0).sum())
    nbr = topo.nbr.cpu()
    assert rs.n_edges == int(fl.deg.sum()) // 2
    x = rest[None].repeat(F, 1, 1)
    if variant != 'rest':
        x = x + 0.05 * torch.randn(F, V, 3, generator=gen)
    if variant == 'coincident':
        a = int(np.argmax(fl.deg > 0))
        x[:, int(nbr[a, 0])] = x[:, a]
    weight, upstream = 7.5, 0.3
    xc = x.cuda()

    # (i) rest_lap = L x_rest by the term's own device code
    zr = R.closed_ring_zero_count(fl, rest[None])
    assert zr == (V if name == 'grid' else 0)             # the flat grid: z = 0 everywhere; nothing else is zero
    short(case, 'rest_lap', rs.lap[None], fl.apply(rest[None]), deg[:1] + 2, zeros=zr)

    # (ii) fpcdr_laplacian_penalty_rest_fwd: d, per_f, the value from per_f
    d = torch.empty_like(xc)
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    per = torch.empty(F, dtype=torch.float32, device='cuda')
    val = torch.empty((), dtype=torch.float32, device='cuda')
    _lib.call("fpcdr_laplacian_penalty_rest_fwd", _ptr(xc), _ptr(topo.nbr32), _ptr(topo.inv_deg), _ptr(rs.lap), _ptr(d), _ptr(acc), _ptr(per),
              _ptr(val), weight, F, V, D, _stream())
    assert bool((acc == 0).all())
    short(case, 'd', d, S.rest_differentials(fl, x, rs.lap), deg + 3)      # (no entry without a term: |x_v| and |r_v| are in every scale)
    if variant == 'rest':       # the consequence of the rule: exactly 0, every entry, and with it the value
        assert int((d == 0).sum()) == F * V * 3 and float(per.abs().max()) == 0.0 and float(val) == 0.0
    per64, _ = R.penalty_value(d, weight)
    per32, _ = R.penalty_value(d, weight, dtype=torch.float32)
    long_sum(case, 'per', per, (per64, per64), per32, zeros=F if variant == 'rest' else 0)
    v64 = R.penalty_value_from_per(per, weight).reshape(1)
    short(case, 'value', val.reshape(1), (v64, v64), R.LAP_N_VALUE, zeros=1 if variant == 'rest' else 0)

    # (iii) rest_lap = NULL is fpcdr_laplacian_penalty_fwd, bit for bit
    outs = []
    for entry in ("fpcdr_laplacian_penalty_fwd", "fpcdr_laplacian_penalty_rest_fwd"):
        l2, p2, v2 = torch.empty_like(xc), torch.empty_like(per), torch.empty_like(val)
        args = [_ptr(xc), _ptr(topo.nbr32), _ptr(topo.inv_deg)] + ([None] if entry.endswith("rest_fwd") else []) + \
               [_ptr(l2), _ptr(acc), _ptr(p2), _ptr(v2), weight, F, V, D, _stream()]
        _lib.call(entry, *args)
        assert bool((acc == 0).all())
        outs.append((l2, p2, v2))
    assert all(torch.equal(a, b) for a, b in zip(*outs)), case

    # (iv) fit.laplacian_penalty(rest=): the three modes, twice on the caller's acc; the backward is the existing kernel fed d
    gref, g1 = R.penalty_grad(d, per, fl, weight, upstream), R.penalty_grad(d, per, fl, weight, 1.0)
    zg = R.closed_ring_zero_count(fl, d)
    assert zg == (F * V * 3 if variant == 'rest' else 0)
    vref = R.penalty_value(d, weight)[1].reshape(1)
    v32 = R.penalty_value(d, weight, dtype=torch.float32)[1].reshape(1)
    for kw, upv, extra in ((dict(), upstream, 0), (dict(eager_grad=True, unit_upstream=True), 1.0, 0), (dict(eager_grad=True), upstream, 1),
                           (dict(acc=acc), upstream, 0), (dict(acc=acc), upstream, 0)):
        leaf = x.cuda().requires_grad_(True)
        value = fit.laplacian_penalty(leaf, topo, weight, rest=rs, **kw)
        (value * upv).backward() if upv != 1.0 else value.backward()
        tag = 'lap ' + (','.join(kw) if kw else 'lazy')
        long_sum(case, tag + ' value', value.reshape(1), (vref, vref), v32, zeros=1 if variant == 'rest' else 0)
        short(case, tag + ' grad', leaf.grad, g1 if upv == 1.0 else gref, deg + R.LAP_N_GRAD + extra, zeros=zg)
        assert bool((acc == 0).all())
    # ... and mesh_laplacian_smoothing(rest=), the torch path's form of the same per_f
    per_t = fit.mesh_laplacian_smoothing(xc, topo, per_mesh=True, rest=rs)
    long_sum(case, 'smoothing per', per_t, (per64, per64), per32, zeros=F if variant == 'rest' else 0)

    # (v) fpcdr_stretch_penalty: against the table, against a constant, value only; two calls on one acc
    table = rs.len.t().cpu()
    for tname, rl_gpu, rl_cpu, target in (('', rs.len, table, 0.0), ('/target', None, None, 0.1)):
        ref, ref32 = S.stretch(x, nbr, rl_cpu, weight, target), S.stretch(x, nbr, rl_cpu, weight, target, dtype=torch.float32)
        per_s, val_s, gx = _stretch_call(xc, topo, rl_gpu, target, weight, rs.n_edges, acc)
        tag = case + tname
        long_sum(tag, 'stretch per', per_s, ref['per'], ref32['per'][0], zeros=F if rs.n_edges == 0 else 0)
        long_sum(tag, 'stretch value', val_s.reshape(1), tuple(t.reshape(1) for t in ref['value']), ref32['value'][0].reshape(1))
        long_sum(tag, 'stretch grad', gx, ref['grad'], ref32['grad'][0], zeros=3 * F * n_isolated)
        if variant != 'rest' and rs.n_edges:      # beside the scaled errors (whose scales carry the 170): the project's float bar on the values themselves
            rl2 = [R.rel_l2(per_s, ref['per'][0]), R.rel_l2(val_s, ref['value'][0]), R.rel_l2(gx, ref['grad'][0])]
            print(f"REST {tag} stretch rel-L2 per={rl2[0]:.2e} value={rl2[1]:.2e} grad={rl2[2]:.2e}")
            assert max(rl2) < 1e-4, (tag, rl2)
        per_v, val_v, _ = _stretch_call(xc, topo, rl_gpu, target, weight, rs.n_edges, acc, grad=False)      # grad_x = NULL
        assert torch.equal(per_v, per_s) and torch.equal(val_v, val_s), tag
    if variant == 'coincident':
        a = int(np.argmax(fl.deg > 0))
        assert float((x[:, int(nbr[a, 0])] - x[:, a]).abs().max()) == 0.0 and bool(torch.isfinite(gx).all())

    # (vi) fit.stretch_penalty: lazy, eager with a unit upstream, eager with a factor, on the caller's acc
    ref, ref32 = S.stretch(x, nbr, table, weight), S.stretch(x, nbr, table, weight, dtype=torch.float32)
    vref = tuple(t.reshape(1) for t in ref['value'])
    for kw, upv in ((dict(), upstream), (dict(eager_grad=True, unit_upstream=True), 1.0), (dict(eager_grad=True), upstream),
                    (dict(acc=acc), upstream)):
        leaf = x.cuda().requires_grad_(True)
        value = fit.stretch_penalty(leaf, topo, weight, rest=rs, **kw)
        (value * upv).backward() if upv != 1.0 else value.backward()
        tag = 'stretch ' + (','.join(kw) if kw else 'lazy')
        long_sum(case, tag + ' value', value.reshape(1), vref, ref32['value'][0].reshape(1))
        long_sum(case, tag + ' grad', leaf.grad, (upv * ref['grad'][0], upv * ref['grad'][1]), float(np.float32(upv)) * ref32['grad'][0],
                 zeros=3 * F * n_isolated)
        assert bool((acc == 0).all())


# fans with 8 and 9 spokes (the table is 8 slots wide / the hub is the one ring the whole wave finishes), 72 and 73 (one round of 64
# slots / one slot of a second), 200, 255 and 256 (V = 256 and 257: one workgroup / one thread of a second), a vertex without an edge,
# the sheared grid
@pytest.mark.parametrize("name", ['fan8', 'fan9', 'fan72', 'fan73', 'fan200', 'fan255', 'fan256', 'isolated', 'grid'])
def test_rest_terms_entries_against_float64_small_meshes(name):
    for F in (1, 3):
        _rest_case(name, F, seed=20 + F)


def test_rest_terms_with_more_meshes_than_the_finish_kernels_threads():
    _rest_case('fan73', 300, seed=30)


@pytest.mark.parametrize("name", ['cfg1', 'sphere'])       # the sphere: 15002 vertices, two poles of degree 120
def test_rest_terms_entries_against_float64_cfg1_and_sphere(name):
    for F in (1, 3):
        _rest_case(name, F, seed=40 + F)


@pytest.mark.parametrize("variant", ['rest', 'coincident'])
def test_rest_terms_at_the_rest_shape_and_with_an_edge_of_length_zero(variant):
    """x = rest exactly: d, per_f, the value and the Laplacian's gradient are exactly 0 (counted); the stretch term meets its bound like
    any other input (its float32 table is one rounding from sqrtf's length).  Two adjacent vertices coincident: the slot contributes 0
    to the gradient, as torch's norm does, and nothing turns NaN."""
    for name, F in (('cfg1', 3), ('fan73', 1), ('isolated', 1)):
        _rest_case(name, F, seed=50, variant=variant)


def test_stretch_with_no_edge_at_all_is_zero():
    """E = 0 (a table of pads): value 0 and gradient 0, exactly."""
    from fpc_diffrend_amd import fit
    V = 70
    nbr32 = torch.full((1, V), V, dtype=torch.int32, device='cuda')
    x = torch.randn(2, V, 3, device='cuda')
    acc = torch.zeros(3, dtype=torch.float64, device='cuda')
    topo = type('T', (), dict(nbr32=nbr32))
    per, val, gx = _stretch_call(x, topo, None, 0.1, 3.0, 0, acc)
    assert float(val) == 0.0 and float(per.abs().max()) == 0.0 and float(gx.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# inside a Fitter
# ---------------------------------------------------------------------------------------------------------------------

# weights at which each term's parameter gradient is at least a tenth of the pixel term's at init_near_truth(0.8) (asserted below).  They are
# this large because the pixel term's gradient is mostly the poses' (norm 1.07e4 over all parameters), which the terms do not reach, and
# because at 0.8 of the truth the terms are small: per unit weight the rest Laplacian is 8.7e-6 and the stretch term 1.3e-4 (float64)
W_LAP, W_STR = 1.0e8, 2.5e7


def _fitter(**kw):
    return fitter_near_truth(4, **{'optimize_texture': False, **kw})


@pytest.mark.parametrize("terms", ['lap', 'stretch', 'both'])
@pytest.mark.parametrize("fused_loss", [True, False])
def test_fitter_gradient_is_the_pixel_terms_plus_the_two_ops(terms, fused_loss):
    """g_on - g_off = g_term to the project's float bar (1e-4 of the gradients' size), on the fused_loss path and the torch chain; the
    term is at least a tenth of the pixel gradient, so a missing term cannot pass.  The same for the loss values."""
    from fpc_diffrend_amd import fit
    on = dict(weight_laplacian=W_LAP if terms != 'stretch' else 0.0, laplacian_relative=terms != 'stretch',
              weight_stretch=W_STR if terms != 'lap' else 0.0)
    frames = slice(0, 4)
    ft_on, ft_off = _fitter(fused_loss=fused_loss, **on), _fitter(fused_loss=fused_loss)
    assert ft_off.rest is None and ft_on.rest is not None
    l_on, l_off = float(ft_on.loss_and_backward(frames)), float(ft_off.loss_and_backward(frames))
    g_on, g_off = _flat_grads(ft_on), _flat_grads(ft_off)
    ft_on.optimizer.zero_grad(set_to_none=True)
    v = ft_on.vertices(frames).reshape(4, -1, 3)
    term = 0.0
    if terms != 'stretch':
        term = term + fit.laplacian_penalty(v, ft_on.topo, W_LAP, rest=ft_on.rest)
    if terms != 'lap':
        term = term + fit.stretch_penalty(v, ft_on.topo, W_STR, rest=ft_on.rest)
    term.backward()
    g_term, l_term = _flat_grads(ft_on), float(term.detach())
    n_on, n_off, n_term = float(g_on.norm()), float(g_off.norm()), float(g_term.norm())
    err = float(((g_on - g_off) - g_term).norm())
    print(f"REST fitter/{terms}/fused_loss={fused_loss} |g_on|={n_on:.4e} |g_off|={n_off:.4e} |g_term|={n_term:.4e} err={err:.3e} "
          f"l_on={l_on:.6e} l_off={l_off:.6e} l_term={l_term:.6e}")
    assert n_term >= 0.1 * n_off and l_term >= 0.1 * l_off
    assert err <= 1e-4 * (n_on + n_off)
    assert abs((l_on - l_off) - l_term) <= 1e-4 * (abs(l_on) + abs(l_off))


@pytest.mark.parametrize("mode,fps", [("prior", 0), ("combined", 2)])
def test_hip_graph_steps_equal_eager_steps_with_the_rest_terms(mode, fps):
    """The configuration and tolerances of test_gpu_fit.test_hip_graph_steps_equal_eager_steps, with both terms on: no host sync and no
    per-call fill, so they replay."""
    from fpc_diffrend_amd import fit, scene
    traj = {}
    for graph in (False, True):
        sc = scene.cfg('cfg1', n_frames=4)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=14, cam_idxs=(0, 3), lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, mode=mode, frames_per_step=fps,
                            hip_graph=graph, weight_laplacian=20.0, laplacian_relative=True, weight_stretch=5.0)
        ft = fit.Fitter(sc, cfg, device='cuda')
        if mode == "prior":
            ft.init_near_truth(0.8)
        traj[graph] = [float(ft.step()) for _ in range(14)]
        if graph:
            assert ft._graphs is not None
        assert bool((ft._reg_acc == 0).all())      # (the one buffer of the Laplacian and the stretch term)
    a, b = np.asarray(traj[False]), np.asarray(traj[True])
    assert np.isfinite(b).all()
    assert np.allclose(a, b, rtol=2e-3), (a, b)
    assert np.allclose(a[:5], b[:5], rtol=1e-5), (a, b)


def test_two_rank_fitter_with_the_rest_terms_equals_single_process(tmp_path, monkeypatch):
    """tests/test_gpu_dist.py's two-rank run with laplacian_relative and weight_stretch in the place of its weight_meshedge: the terms'
    weights carry the 1 / world, the replicas stay bit-identical and equal the single process."""
    import test_gpu_dist as D
    assert "weight_meshedge=0.3" in D.CHILD
    monkeypatch.setattr(D, "CHILD", D.CHILD.replace("weight_meshedge=0.3", "laplacian_relative=True, weight_stretch=30.0"))
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
            continue        # (the texture: the terms do not reach it; test_gpu_dist.py holds it to its own share rule)
        dmax = float((p - q).abs().max())
        assert dmax <= 1e-5 * max(1.0, float(q.abs().max())), (k, tuple(p.shape), dmax)
    assert float((a["result"] - one["result"]).abs().max()) < 1e-4


def test_relative_laplacian_keeps_the_shape_the_plain_one_smooths_away():
    """mode='free' on cfg1, the default weight_laplacian = 5000, 30 steps from the base mesh: with the plain term the mean distance
    to the ground-truth vertices grows (the term's gradient at the base mesh, up to 9.8 per coordinate, outweighs the pixel term's); against
    the base mesh's own differentials the term starts at exactly 0 and the fit is left to the pixels.  Only the ordering is asserted."""
    from fpc_diffrend_amd import fit, scene
    dist = {}
    for relative in (False, True):
        sc = scene.cfg('cfg1', n_frames=4)
        sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
        cfg = fit.FitConfig(max_iter=30, cam_idxs=(0, 3), mode='free', weight_laplacian=5000.0, laplacian_relative=relative)
        ft = fit.Fitter(sc, cfg, device='cuda')
        ft.init_near_truth(0.8)
        truth = (torch.tensor(sc.v_base)[None] + torch.tensor(sc.weights_gt) @ torch.tensor(sc.blendshapes).t()).reshape(4, -1, 3).cuda()
        start = float((ft.vertices(slice(0, 4)).detach().reshape(4, -1, 3) - truth).norm(dim=2).mean())
        for _ in range(30):
            ft.step()
        dist[relative] = float((ft.result.reshape(4, -1, 3) - truth).norm(dim=2).mean())
        print(f"REST behaviour laplacian_relative={relative} mean distance to the truth: start {start:.5f} after 30 steps {dist[relative]:.5f}")
    assert dist[False] > dist[True], dist

"""CPU: the float64 statement of the bending term (tests/bend_ref.py) against torch.autograd of one plain expression, against
fit.mesh_normal_consistency, its zero at the rest shape, its invariance and its sign; the host side of the feature (MeshTopology.hinges(),
RestShape.bend_cs, FitConfig, the C entry and its argument checks, the kernels' private segment, the README's table) -- no GPU.

Measured: the statement's gradient against autograd, max_i |g_i - a_i| / S_i over all meshes, with and without a table: 1.9e-16 (the
bound is 1e-10; S carries the 170 of the positions, so the same figure relative to the gradient's largest entry is printed beside it:
at most 1.5e-15)."""
import ctypes
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bend_ref as B  # noqa: E402
import fitstep_ref as R  # noqa: E402


def _meshes():
    """Every mesh of tests/test_gpu_bend.py: name -> (faces, V, rest positions [V,3] float32)."""
    out = dict(B.small_meshes(torch.Generator().manual_seed(5)))
    out['sphere'] = R.uv_sphere()
    from fpc_diffrend_amd import scene
    sc = scene.cfg('cfg1', n_frames=3)
    out['cfg1'] = (sc.pos_idx, sc.n_vertices, torch.tensor(sc.v_base).reshape(-1, 3))
    return out


def test_statement_gradient_equals_autograd_of_the_plain_expression():
    g = torch.Generator().manual_seed(12)
    worst, worst_rel = 0.0, 0.0
    for name, (faces, V, rest) in _meshes().items():
        hv, sigma = B.hinges(faces)
        if hv.shape[0] == 0:
            continue
        F, w = 2, 7.5
        rest_y = rest.clone().float()
        rest_y[:, 1] += 170.0
        x = (rest_y[None].repeat(F, 1, 1) + 0.05 * torch.randn(F, V, 3, generator=g)).double()
        for cs in (None, B.rest_cs(rest_y, hv, sigma)):
            leaf = x.clone().requires_grad_(True)
            val = B.bend_plain(leaf, hv, sigma, cs, w)
            val.backward()
            st = B.bend(x, hv, sigma, cs, w)
            assert bool(st['live'].all()), name
            gv, gS = st['grad']
            assert bool((gS >= gv.abs() * (1 - 1e-12)).all()) and float(st['value'][1]) >= float(st['value'][0])
            touched = gS > 0
            e = float(((gv - leaf.grad).abs()[touched] / gS[touched]).max())
            rel = float((gv - leaf.grad).abs().max() / leaf.grad.abs().max())
            print(f"BEND autograd {name} table={cs is not None} e/S={e:.2e} rel={rel:.2e}")
            assert bool((leaf.grad[~touched] == 0).all()), name
            assert e <= 1e-10, (name, e)
            worst, worst_rel = max(worst, e), max(worst_rel, rel)
            # the value: the stable form and the float32 table's norm (c_r^2 + s_r^2 = 1 to 2^-23) are all that separate the two
            assert abs(float(st['value'][0]) - float(val.detach())) <= 2.0 ** -22 * w, name
            # the corners' gradients of one hinge sum to zero (to the rounding their scales describe)
            hg, hgS = st['hinge_grad']
            assert bool((hg.sum(dim=2).abs() <= 1e-12 * hgS.sum(dim=2)).all()), name
    print(f"BEND autograd worst e/S={worst:.2e} rel={worst_rel:.2e}")


def test_without_a_table_the_statement_is_mesh_normal_consistency():
    """1e-12, on a CPU MeshTopology; two_neg has a hinge with sigma = -1, book an edge with three faces, grid and the fans' rims a boundary."""
    from fpc_diffrend_amd import fit
    g = torch.Generator().manual_seed(13)
    seen_neg = False
    for name, (faces, V, rest) in _meshes().items():
        hv, sigma = B.hinges(faces)
        seen_neg = seen_neg or bool((sigma < 0).any())
        topo = fit.MeshTopology(faces, V, 'cpu')
        x = (rest[None].repeat(3, 1, 1) + 0.05 * torch.randn(3, V, 3, generator=g)).double()
        x[..., 1] += 170.0
        want = float(fit.mesh_normal_consistency(x, topo))
        got = float(B.bend(x, hv, sigma, None, 1.0)['value'][0])
        assert abs(got - want) <= 1e-12, (name, got, want)
    assert seen_neg
    hv, sigma = B.hinges(_meshes()['book'][0])
    assert hv.tolist() == [[1, 2, 0, 5]] and sigma.tolist() == [1]
    hv, sigma = B.hinges(_meshes()['two_neg'][0])
    assert hv.tolist() == [[0, 1, 2, 3]] and sigma.tolist() == [-1]


def test_topology_tables_agree_with_the_statements():
    from fpc_diffrend_amd import fit
    for name, (faces, V, rest) in _meshes().items():
        topo = fit.MeshTopology(faces, V, 'cpu')
        assert topo._hinges is None                      # nothing is built for a topology that never asks
        hinge_vtx, hinge_inc, H, K = topo.hinges()
        assert topo.hinges()[0] is hinge_vtx             # cached
        hv, sigma = B.hinges(faces)
        assert H == hv.shape[0] == topo.edge_faces[0].numel(), name
        assert hinge_vtx.dtype == torch.int32 and hinge_vtx.shape == (4, H) and torch.equal(hinge_vtx, B.packed(hv, sigma)), name
        # the hinges are edge_faces', in that order, f0 the lower face index
        ef = torch.stack([torch.minimum(*topo.edge_faces), torch.maximum(*topo.edge_faces)], dim=1)
        assert torch.equal(ef, B.hinge_faces(faces)), name
        want = B.incidence(hv, V)
        assert hinge_inc.dtype == torch.int32 and hinge_inc.shape == (K, V) and K == max(max(len(l) for l in want), 1), name
        inc = hinge_inc.t().tolist()
        for v in range(V):
            n = len(want[v])
            assert inc[v][:n] == want[v] and all(e == -1 for e in inc[v][n:]), (name, v)       # ascending, pads trail
        real = hinge_inc[hinge_inc >= 0]
        assert sorted(real.tolist()) == list(range(4 * H)), name                                 # every corner exactly once
        # the rest angles
        rs = fit.RestShape(topo, rest)
        assert rs._bend_cs is None
        cs = rs.bend_cs
        assert cs.dtype == torch.float32 and cs.shape == (2, H), name
        if H:      # (two float64 evaluations of the same expressions, rounded once each: equal or neighbouring float32s)
            assert float((cs - B.rest_cs(rest, hv, sigma)).abs().max()) <= 2.0 ** -23, name
            assert float(((cs ** 2).sum(dim=0) - 1.0).abs().max()) <= 2.0 ** -22, name
    # a hinge degenerate at rest gets (1, 0)
    faces, V, rest = _meshes()['two_pos']
    flat = rest.clone()
    flat[3] = flat[0] + 2.0 * (flat[1] - flat[0])
    topo = fit.MeshTopology(faces, V, 'cpu')
    assert fit.RestShape(topo, flat).bend_cs.tolist() == [[1.0], [0.0]]
    assert B.rest_cs(flat, *B.hinges(faces)).tolist() == [[1.0], [0.0]]


def test_zero_at_the_rest_shape_and_unchanged_by_a_rigid_motion():
    g = torch.Generator().manual_seed(14)
    for name, (faces, V, rest) in _meshes().items():
        hv, sigma = B.hinges(faces)
        x = rest.double()[None].repeat(2, 1, 1)
        x[..., 1] += 170.0
        st = B.bend(x, hv, sigma, B.rest_cs(x[0], hv, sigma, rounded=False), 3.0)
        assert float(st['value'][0]) < 1e-25 and float(st['grad'][0].abs().max() if V else 0.0) < 1e-25, name
        # a rigid motion (about the mesh's own centre, so that it costs no digits of the edges)
        x = (rest[None] + 0.05 * torch.randn(1, V, 3, generator=g)).double()
        cs = B.rest_cs(rest, hv, sigma)
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        if float(torch.linalg.det(q)) < 0:
            q[:, 0] = -q[:, 0]
        centre = x.mean(dim=1, keepdim=True)
        moved = (x - centre) @ q.t() + centre + torch.randn(3, generator=g, dtype=torch.float64)
        a, b = float(B.bend(x, hv, sigma, cs, 1.0)['value'][0]), float(B.bend(moved, hv, sigma, cs, 1.0)['value'][0])
        assert abs(a - b) <= 1e-12, (name, a, b)


def test_the_term_sees_the_sign_of_the_angle():
    """A hinge folded to -theta_rest costs 1 - cos(2 theta_rest); a (cos - cos_rest)^2 form would cost nothing."""
    faces = np.asarray([[0, 1, 2], [1, 0, 3]], dtype=np.int32)
    hv, sigma = B.hinges(faces)
    for phi in (0.3, 1.2, 2.5):
        rest = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, 1.0, 0.0], [0.5, -math.cos(phi), math.sin(phi)]], dtype=torch.float64)
        cs = B.rest_cs(rest, hv, sigma, rounded=False)
        theta = math.atan2(float(cs[1]), float(cs[0]))
        assert abs(abs(theta) - phi) < 1e-12
        mirrored = rest.clone()
        mirrored[:, 2] = -mirrored[:, 2]
        st = B.bend(mirrored[None], hv, sigma, cs, 1.0)
        assert abs(float(st['value'][0]) - (1.0 - math.cos(2.0 * theta))) < 1e-12
        assert abs(float(st['cosd'][0, 0]) - math.cos(2.0 * theta)) < 1e-12
        assert float(B.bend(rest[None], hv, sigma, cs, 1.0)['value'][0]) == 0.0


def test_fitconfig_and_the_python_entry():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert cfg.weight_bend == 0.0 and 'weight_bend' in [f.name for f in dataclasses.fields(fit.FitConfig)]
    assert (cfg.weight_laplacian, cfg.weight_meshedge, cfg.weight_normalconsistency, cfg.weight_stretch) == (5000.0, 0.0, 0.0, 0.0)
    import inspect
    assert list(inspect.signature(fit.bend_penalty).parameters) == ['verts', 'topo', 'weight', 'rest', 'eager_grad', 'unit_upstream', 'acc',
                                                                    'scratch']
    with pytest.raises(RuntimeError, match="GPU only"):
        topo = fit.MeshTopology(R.fan(8)[0], 9, 'cpu')
        fit.bend_penalty(torch.zeros(1, 9, 3), topo, 1.0)


def _lib_loaded():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def test_both_libraries_export_the_entry_and_abi_stays_16():
    _lib, lib = _lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert "fpcdr_bend_penalty" in _lib.SYMBOLS and hasattr(lib, "fpcdr_bend_penalty")
    assert "int fpcdr_bend_penalty(" in open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    if os.path.exists(_lib.TWOCALL_LIB_PATH):
        assert hasattr(ctypes.CDLL(_lib.TWOCALL_LIB_PATH), "fpcdr_bend_penalty")


def test_bad_arguments_give_an_error_code_before_any_launch():
    """Nulls, sizes out of range, a misaligned acc, grad_x without its tables: the checks come before the first HIP call, so this runs
    without a GPU on host memory the entry never touches."""
    _lib, lib = _lib_loaded()
    F, V, H, K = 2, 5, 3, 4
    fb = lambda n: (ctypes.c_float * (n + 4))()
    x, cs, hg, gx, per, out = fb(F * V * 3), fb(2 * H), fb(F * H * 12), fb(F * V * 3), fb(F), fb(1)
    hv, inc = (ctypes.c_int32 * (4 * H))(), (ctypes.c_int32 * (K * V))()
    acc = (ctypes.c_double * (F + 2))()
    P = lambda b: ctypes.cast(b, ctypes.c_void_p)
    off = lambda b, k: ctypes.c_void_p(ctypes.addressof(b) + k)

    def args(**over):
        kw = dict(x=P(x), hinge_vtx=P(hv), rest_cs=P(cs), hinge_inc=P(inc), hinge_grad=P(hg), grad_x=P(gx), acc=P(acc), per=P(per),
                  out=P(out), weight=1.0, F=F, V=V, H=H, K=K)
        kw.update(over)
        return [kw[k] for k in ('x', 'hinge_vtx', 'rest_cs', 'hinge_inc', 'hinge_grad', 'grad_x', 'acc', 'per', 'out', 'weight', 'F', 'V',
                                'H', 'K')] + [None]

    bad = [dict(x=None), dict(hinge_vtx=None), dict(acc=None), dict(per=None), dict(out=None),
           dict(F=0), dict(F=-1), dict(F=65536), dict(V=0), dict(V=-3), dict(H=-1), dict(K=0), dict(K=-2),
           dict(acc=off(acc, 4)), dict(hinge_inc=None), dict(hinge_grad=None), dict(hinge_inc=None, hinge_grad=None)]
    for i, over in enumerate(bad):
        assert lib.fpcdr_bend_penalty(*args(**over)) != 0, i
        assert b"fpcdr_bend_penalty" in lib.fpcdr_last_error(), i
    assert all(v == 0.0 for v in acc)


def test_bend_kernels_have_no_private_segment():
    """read from the built object (tests/codeobj.py).  The gather keeps a running sum, not an indexed local array."""
    import codeobj
    recs = codeobj.kernels("mesh_reg.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    bend = {name: private for name, private, _ in recs if "k_bend_" in name}
    assert len(bend) == 2 and all(p == 0 for p in bend.values()), bend
    assert all(any(k in name for name in bend) for k in ("k_bend_hinges", "k_bend_gather"))
    finish = {name: private for name, private, _ in recs if "k_penalty_finish" in name}      # the finish kernel it shares with the other terms
    assert len(finish) == 2 and all(p == 0 for p in finish.values()), finish


def test_the_readmes_table_rows_come_from_the_statement():
    import rest_regulariser_table as T
    b = T.bend_rows()
    assert (b['vertices'], b['hinges'], b['inconsistent']) == (514, 1536, 0)
    rows = [f"{b['plain_base']:.6f}", f"{b['plain_grad_max']:.1e}", f"{b['plain_grad_rms']:.1e}", f"{b['angle_mean_deg']:.1f}°",
            f"{b['angle_max_deg']:.1f}°", ", ".join(f"{v:.6f}" for v in b['plain_truth'])]
    assert rows == ["0.009515", "3.0e-03", "1.1e-04", "6.2°", "14.2°", "0.009534, 0.009518, 0.009515"], rows
    assert [f"{v:.1e}" for v in b['rest_truth'][:2]] == ["4.0e-05", "1.4e-05"] and b['rest_truth'][2] < 1e-15
    readme = open(os.path.join(ROOT, "README.md"), encoding="utf-8").read()
    for cell in ("| 0.009515 |", "3.0e-3 per coordinate (rms 1.1e-4)", "| 6.2° |", "| 14.2° |", "| 0.009534, 0.009518, 0.009515 |",
                 "| 4.0e-5, 1.4e-5, 0 |"):
        assert cell in readme, cell

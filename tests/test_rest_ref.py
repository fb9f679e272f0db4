"""CPU: the float64 statements of the rest-shape regularisers (tests/rest_ref.py) against torch.autograd of one plain expression each
and against the oracle's mesh_edge_loss, their exact zero at the rest shape, the host side of the feature (RestShape's tables, FitConfig,
the two new C entries and their argument checks, the kernels' private segment) -- no GPU."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import fitstep_ref as R  # noqa: E402
import rest_ref as S  # noqa: E402


def _meshes():
    g = torch.Generator().manual_seed(11)
    out = {k: (f, V, pos) for k, (f, V, pos, _) in R.lap_meshes(g).items() if k in ('fan9', 'fan73', 'isolated', 'grid')}
    from fpc_diffrend_amd import scene
    sc = scene.cfg('cfg1', n_frames=3)
    out['cfg1'] = (sc.pos_idx, sc.n_vertices, torch.tensor(sc.v_base).reshape(-1, 3))
    return out, g


def _rel(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


def test_statements_equal_autograd_of_a_plain_expression():
    meshes, g = _meshes()
    for name, (faces, V, rest) in meshes.items():
        fl = R.FaceLaplacian(faces, V)
        nbr = S.ring_table(faces, V)
        F, w = 3, 7.5
        x = (rest[None].repeat(F, 1, 1) + 0.05 * torch.randn(F, V, 3, generator=g)).double()
        x[..., 1] += 170.0
        rest_d = rest.double()
        rest_d[:, 1] += 170.0
        # rest Laplacian
        r_lap = fl.apply(rest_d[None])[0][0]
        leaf = x.clone().requires_grad_(True)
        val = S.rest_penalty_plain(leaf, fl.dense(), r_lap, w)
        val.backward()
        st = S.rest_penalty(fl, x, r_lap, w)
        assert abs(float(st['value'][0]) - float(val.detach())) <= 1e-10 * abs(float(val.detach())), name
        assert _rel(st['grad'][0], leaf.grad) <= 1e-10, name
        # stretch, with a table and with the constant target
        rl, E = S.rest_lengths(nbr, rest_d.float())
        edges = S.edge_list(nbr)
        assert E == edges.shape[0]
        el = (rest_d.float().double()[edges[:, 0]] - rest_d.float().double()[edges[:, 1]]).norm(dim=1).float().double()
        for table, target in ((rl, 0.0), (None, 0.1)):
            leaf = x.clone().requires_grad_(True)
            val = S.stretch_plain(leaf, edges, el if table is not None else None, w, float(np.float32(target)))
            val.backward()
            st = S.stretch(x, nbr, table, w, target)
            assert abs(float(st['value'][0]) - float(val.detach())) <= 1e-10 * abs(float(val.detach())), (name, target)
            assert _rel(st['grad'][0], leaf.grad) <= 1e-10, (name, target)
            assert bool((st['grad'][1] >= st['grad'][0].abs() * (1 - 1e-12)).all()) and float(st['value'][1]) >= float(st['value'][0])


def test_constant_target_stretch_is_the_oracles_mesh_edge_loss_on_cfg1():
    from fpc_diffrend_amd import scene
    from oracle import fit as ofit
    sc = scene.cfg('cfg1', n_frames=3)
    V = sc.n_vertices
    verts = (torch.tensor(sc.v_base, dtype=torch.float64)[None]
             + torch.tensor(sc.weights_gt[:3], dtype=torch.float64) @ torch.tensor(sc.blendshapes, dtype=torch.float64).t()).reshape(3, V, 3)
    nbr = S.ring_table(sc.pos_idx, V)
    want = ofit.mesh_edge_loss(verts, torch.tensor(np.asarray(sc.pos_idx)), float(np.float32(0.1)))
    got = S.stretch(verts, nbr, None, 1.0, 0.1)
    assert _rel(got['per'][0], want) <= 1e-12
    assert abs(float(got['value'][0]) - float(want.mean())) <= 1e-12 * float(want.mean())


def test_both_terms_vanish_exactly_at_the_rest_shape():
    """x = x_rest in every frame: d = L x - L x_rest and s = |e| - |e_rest| are differences of equal numbers -- value and gradient are
    exactly 0, not small.  (The stretch table here is the statement's own float64 norm; the float32 table of the kernel is one rounding
    away from it, a relative 2^-24 of an edge.)"""
    meshes, _ = _meshes()
    for name, (faces, V, rest) in meshes.items():
        fl = R.FaceLaplacian(faces, V)
        nbr = S.ring_table(faces, V)
        x = rest.double()[None].repeat(2, 1, 1)
        st = S.rest_penalty(fl, x, fl.apply(x[:1])[0][0], 5000.0)
        assert float(st['value'][0]) == 0.0 and float(st['grad'][0].abs().max()) == 0.0, name
        real = nbr < V
        d = x[0][torch.where(real, nbr, torch.zeros_like(nbr))] - x[0][:, None]
        table = torch.where(real, d.norm(dim=2), torch.zeros((), dtype=torch.float64))
        st = S.stretch(x, nbr, table, 3.0)
        assert float(st['value'][0]) == 0.0 and float(st['grad'][0].abs().max()) == 0.0, name
        rl, _ = S.rest_lengths(nbr, rest)
        st = S.stretch(x, nbr, rl, 3.0)
        assert float(st['per'][0].max()) <= (2.0 ** -24 * float(table.max())) ** 2, name


def test_rest_shape_tables_on_the_host():
    """rest_len is symmetric (both ends of an edge hold the same float32), zero on the pads, aligned with MeshTopology.nbr32, and equal
    to the reference module's; n_edges is the face list's own count."""
    from fpc_diffrend_amd import fit
    meshes, _ = _meshes()
    for name, (faces, V, rest) in meshes.items():
        topo = fit.MeshTopology(faces, V, 'cpu')
        rs = fit.RestShape(topo, rest)
        fl = R.FaceLaplacian(faces, V)
        assert rs.n_edges == int(fl.deg.sum()) // 2 == topo.edges.shape[0], name
        assert rs.lap is None and rs.len.shape == topo.nbr32.shape and rs.len.dtype == torch.float32
        nbr = topo.nbr32.long()                                       # [D,V]
        pad = nbr >= V
        assert bool((rs.len[pad] == 0).all()) and bool((rs.len[~pad] > 0).all()), name
        back = {}
        for d, v in zip(*[t.tolist() for t in torch.nonzero(~pad, as_tuple=True)]):
            back[(v, int(nbr[d, v]))] = float(rs.len[d, v])
        assert all(back[(n, v)] == l for (v, n), l in back.items()), name
        assert torch.equal(topo.nbr, S.ring_table(faces, V))
        assert torch.equal(rs.len.t(), S.rest_lengths(topo.nbr, rest)[0]), name
        tl, ne = fit.rest_edge_lengths(topo.nbr32, rest)
        assert torch.equal(tl, rs.len) and ne == rs.n_edges


def test_fitconfig_has_the_new_fields_off_by_default():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert cfg.laplacian_relative is False and cfg.weight_stretch == 0.0
    names = [f.name for f in dataclasses.fields(fit.FitConfig)]
    assert 'laplacian_relative' in names and 'weight_stretch' in names
    assert (cfg.weight_laplacian, cfg.weight_meshedge, cfg.weight_normalconsistency) == (5000.0, 0.0, 0.0)
    import inspect
    assert inspect.signature(fit.laplacian_penalty).parameters['rest'].default is None
    assert inspect.signature(fit.mesh_laplacian_smoothing).parameters['rest'].default is None
    sp = inspect.signature(fit.stretch_penalty).parameters
    assert list(sp) == ['verts', 'topo', 'weight', 'rest', 'target', 'eager_grad', 'unit_upstream', 'acc']
    with pytest.raises(RuntimeError, match="GPU only"):
        topo = fit.MeshTopology(R.fan(8)[0], 9, 'cpu')
        fit.stretch_penalty(torch.zeros(1, 9, 3), topo, 1.0)


def _lib_loaded():
    from fpc_diffrend_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.load()


def test_both_libraries_export_the_entries_and_abi_stays_16():
    _lib, lib = _lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    for name in ("fpcdr_laplacian_penalty_rest_fwd", "fpcdr_stretch_penalty"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert name in open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    if os.path.exists(_lib.TWOCALL_LIB_PATH):
        tc = ctypes.CDLL(_lib.TWOCALL_LIB_PATH)
        assert hasattr(tc, "fpcdr_laplacian_penalty_rest_fwd") and hasattr(tc, "fpcdr_stretch_penalty")


def test_bad_arguments_give_an_error_code_before_any_launch():
    """Nulls, non-positive and oversize sizes, a misaligned acc, E < 0: the checks come before the first HIP call, so this runs without a
    GPU on host memory the entries never touch."""
    _lib, lib = _lib_loaded()
    F, V, D = 2, 5, 3
    fb = lambda n: (ctypes.c_float * (n + 4))()
    x, inv_deg, rest_lap, lap, per, out, rest_len, gx = fb(F * V * 3), fb(V), fb(V * 3), fb(F * V * 3), fb(F), fb(1), fb(D * V), fb(F * V * 3)
    nbr = (ctypes.c_int32 * (D * V))()
    acc = (ctypes.c_double * (F + 2))()
    P = lambda b: ctypes.cast(b, ctypes.c_void_p)
    off = lambda b, k: ctypes.c_void_p(ctypes.addressof(b) + k)

    def lap_args(**over):
        kw = dict(x=P(x), nbr=P(nbr), inv_deg=P(inv_deg), rest_lap=P(rest_lap), lap=P(lap), acc=P(acc), per=P(per), out=P(out), weight=1.0,
                  F=F, V=V, D=D)
        kw.update(over)
        return [kw[k] for k in ('x', 'nbr', 'inv_deg', 'rest_lap', 'lap', 'acc', 'per', 'out', 'weight', 'F', 'V', 'D')] + [None]

    def str_args(**over):
        kw = dict(x=P(x), nbr=P(nbr), rest_len=P(rest_len), target=0.0, grad_x=P(gx), acc=P(acc), per=P(per), out=P(out), weight=1.0,
                  F=F, V=V, D=D, E=4)
        kw.update(over)
        return [kw[k] for k in ('x', 'nbr', 'rest_len', 'target', 'grad_x', 'acc', 'per', 'out', 'weight', 'F', 'V', 'D', 'E')] + [None]

    sizes = [dict(F=0), dict(F=-1), dict(F=65536), dict(V=0), dict(V=-3), dict(D=0), dict(D=-1)]
    bad_lap = [dict(x=None), dict(nbr=None), dict(inv_deg=None), dict(lap=None), dict(acc=None), dict(per=None), dict(out=None),
               dict(acc=off(acc, 4))] + sizes
    for i, over in enumerate(bad_lap):
        assert lib.fpcdr_laplacian_penalty_rest_fwd(*lap_args(**over)) != 0, i
        assert b"fpcdr_laplacian_penalty_rest_fwd" in lib.fpcdr_last_error()
    bad_str = [dict(x=None), dict(nbr=None), dict(acc=None), dict(per=None), dict(out=None), dict(acc=off(acc, 4)), dict(E=-1)] + sizes
    for i, over in enumerate(bad_str):
        assert lib.fpcdr_stretch_penalty(*str_args(**over)) != 0, i
        assert b"fpcdr_stretch_penalty" in lib.fpcdr_last_error()
    assert all(v == 0.0 for v in acc)


def test_rest_and_stretch_kernels_have_no_private_segment():
    """read from the built object (tests/codeobj.py).  The per-slot terms of the unrolled ring walk are indexed by
    compile-time constants only."""
    import codeobj
    recs = codeobj.kernels("mesh_reg.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    stretch = {name: private for name, private, _ in recs if "k_stretch_" in name}
    assert len(stretch) == 1 and all(p == 0 for p in stretch.values()), stretch       # k_stretch_penalty
    fwd = {name: private for name, private, _ in recs if "k_lap_penalty_fwd" in name}
    assert len(fwd) == 2 and all(p == 0 for p in fwd.values()), fwd       # <false> and <true>
    finish = {name: private for name, private, _ in recs if "k_penalty_finish" in name}      # the finish kernel of all three terms
    assert len(finish) == 2 and all(p == 0 for p in finish.values()), finish       # <false> (stretch, bend) and <true> (Laplacian)

"""Bit-identity of the mesh regularisers, transform_clip and the MVP chain (csrc/mesh_reg.hip, csrc/clip.hip) between two builds of
libfpcdr.so.

    FPCDR_LIB_PATH=/path/to/libfpcdr.so python scripts/mesh_reg_planes.py OUT.pt        one fresh process per library
    python scripts/mesh_reg_planes.py --compare A.pt B.pt [--spread A2.pt A3.pt ...]

The first form calls every entry of the two sources at the shapes of the GPU tests -- the fans, the isolated vertex and the sheared grid of
fitstep_ref.lap_meshes, the cfg1 mesh and the UV sphere at F = 1 and 3, a fan at F = 257 and 300 (more meshes than the finish kernel has
threads); fitstep_ref.CLIP_SHAPES; fitstep_ref.MVP_SHAPES, (1, 1), (2, 2) and fitstep_ref.mvp_index_cases -- and saves every output.
The second form holds B to A.  Outputs that are gathers or whose sums have a fixed order must be torch.equal: the Laplacians, every
grad_x, the bend scratch, the clip positions and vertex gradients, the MVP matrices, and the MVP gradients at (1, 1) and (2, 2).  Outputs
summed by atomics ("loose": per / out of the three penalties, grad_mvp of the clip transform, the MVP gradients at the other shapes) are
held to the spread of A's own library (--spread: further runs of it; without them they are only reported): the order of float atomics is
not controlled, so with the same code B - A is a draw from the distribution A2 - A comes from, and the bound of an output is the largest
difference, in units of the output's largest entry, that any two runs of A's library show in any output of its class (the penalties, the
clip transform, the MVP chain).  Exit status 1 on a difference."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import fitstep_ref as R
    from fpc_diffrend_amd import _lib, fit, scene
    assert torch.cuda.is_available(), "needs the GPU"
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device='cuda')
    res, w = {}, 7.5

    def keep(case, **planes):
        torch.cuda.synchronize()
        for name, t in planes.items():
            res[f"{case}/{name}"] = t.detach().cpu().clone()

    # ---- the regularisers
    meshes = dict(R.lap_meshes(torch.Generator().manual_seed(5)))
    sc = scene.cfg('cfg1', n_frames=3)
    meshes['cfg1'] = (sc.pos_idx, sc.n_vertices, torch.tensor(sc.v_base).reshape(-1, 3), None)
    meshes['sphere'] = (*R.uv_sphere(), None)
    todo = [(name, F) for name in meshes for F in (1, 3)] + [('fan8', 257), ('fan73', 300)]
    made = {}
    for name, F in todo:
        faces, V, pos, _ = meshes[name]
        if name not in made:
            rest = pos.clone().float()
            rest[:, 1] += 170.0
            topo = fit.MeshTopology(faces, V, 'cuda')
            made[name] = (rest, topo, fit.RestShape(topo, rest.cuda()))
        rest, topo, rs = made[name]
        D, E = topo.nbr32.shape[0], rs.n_edges
        hinge_vtx, hinge_inc, H, K = topo.hinges()
        x = (rest[None] + 0.05 * torch.randn(F, V, 3, generator=torch.Generator().manual_seed(F))).cuda()
        acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
        up = torch.full((), 0.7, dtype=torch.float32, device='cuda')
        case = f"{name}/F{F}"
        for mode in (0, 1):
            o = f32(F, V, 3)
            _lib.call("fpcdr_laplacian_gather", p(x), p(topo.nbr32), p(topo.inv_deg), p(o), F, V, D, mode, st())
            keep(case, **{f"gather{mode}": o})
        for form, rest_lap in (('plain', None), ('rest', rs.lap)):
            lap, per, out, gx = f32(F, V, 3), f32(F), f32(()), f32(F, V, 3)
            if rest_lap is None:
                _lib.call("fpcdr_laplacian_penalty_fwd", p(x), p(topo.nbr32), p(topo.inv_deg), p(lap), p(acc), p(per), p(out), w, F, V, D, st())
            else:
                _lib.call("fpcdr_laplacian_penalty_rest_fwd", p(x), p(topo.nbr32), p(topo.inv_deg), p(rest_lap), p(lap), p(acc), p(per), p(out),
                          w, F, V, D, st())
            keep(case, **{f"lap_{form}": lap, f"loose_per_lap_{form}": per, f"loose_out_lap_{form}": out})
            _lib.call("fpcdr_laplacian_penalty_bwd", p(lap), p(topo.nbr32), p(topo.inv_deg), p(per), p(up), p(gx), w, F, V, D, st())
            keep(case, **{f"grad_lap_{form}": gx})
        for form, rest_len, target in (('rest', rs.len, 0.0), ('target', None, 0.1)):
            per, out, gx = f32(F), f32(()), f32(F, V, 3)
            _lib.call("fpcdr_stretch_penalty", p(x), p(topo.nbr32), p(rest_len), target, p(gx), p(acc), p(per), p(out), w, F, V, D, E, st())
            keep(case, **{f"grad_stretch_{form}": gx, f"loose_per_stretch_{form}": per, f"loose_out_stretch_{form}": out})
        for form, cs in (('rest', rs.bend_cs), ('plain', None)):
            per, out, gx, hg = f32(F), f32(()), f32(F, V, 3), torch.zeros(max(F * H * 12, 1), dtype=torch.float32, device='cuda')
            _lib.call("fpcdr_bend_penalty", p(x), p(hinge_vtx), p(cs), p(hinge_inc), p(hg), p(gx), p(acc), p(per), p(out), w, F, V, H, K, st())
            keep(case, **{f"grad_bend_{form}": gx, f"scratch_bend_{form}": hg, f"loose_per_bend_{form}": per, f"loose_out_bend_{form}": out})
        assert bool((acc == 0).all()), case
    # ---- transform_clip
    for F, Nc, V in R.CLIP_SHAPES:
        mvp, verts, go = (t.cuda().contiguous() for t in R.clip_inputs(F, Nc, V, 'randn'))
        out, gv, gm = f32(F * Nc, V, 4), f32(F, V, 3), torch.zeros(F * Nc, 4, 4, dtype=torch.float32, device='cuda')
        _lib.call("fpcdr_transform_clip_fwd", p(mvp), p(verts), p(out), F, Nc, V, st())
        _lib.call("fpcdr_transform_clip_bwd", p(mvp), p(verts), p(go), p(gv), p(gm), F, Nc, V, st())
        gv1, gm1 = f32(F, V, 3), torch.zeros_like(gm)
        _lib.call("fpcdr_transform_clip_bwd", p(mvp), p(verts), p(go), p(gv1), None, F, Nc, V, st())
        _lib.call("fpcdr_transform_clip_bwd", p(mvp), p(verts), p(go), None, p(gm1), F, Nc, V, st())
        keep(f"clip/{F}x{Nc}x{V}", pos=out, grad_verts=gv, grad_verts_alone=gv1, loose_grad_mvp=gm, loose_grad_mvp_alone=gm1)
    # ---- the MVP chain
    cases = [(f"{Fb}x{Nc}", Fb, Nc, Fb, Nc, Nc, None, None, None) for Fb, Nc in [(1, 1), (2, 2)] + R.MVP_SHAPES]
    cases += [(name, len(fi) if fi is not None else nf, len(vi) if vi is not None else nv, nf, ncam, nv, fi, vi, cov)
              for name, nf, ncam, nv, fi, vi, cov in R.mvp_index_cases(torch.Generator().manual_seed(7))]
    for name, Fb, Nc, nf, ncam, nv, fi, vi, cov in cases:
        qc, tc, qf, tf, P, MV, go = (t.cuda().contiguous() for t in R.mvp_inputs(Fb, Nc, 'randn', n_frames=nf, n_cams=ncam, n_views=nv))
        idx = [t.cuda() if t is not None else None for t in (fi, vi, cov)]
        tables = (p(P), p(MV), p(qc), p(tc), p(qf), p(tf))
        exact = 'small' if (Fb, Nc) in ((1, 1), (2, 2)) else 'loose'
        forms = [('indexed', idx)] if name in ('all', 'no_frame_idx', 'no_view_idx', 'no_cam_of_view') else [('plain', None), ('indexed', idx)]
        for form, ix in forms:
            out = f32(Fb * Nc, 4, 4)
            g = [torch.zeros_like(t) for t in (qc, tc, qf, tf)]
            if ix is None:
                _lib.call("fpcdr_mvp_fwd", *tables, p(out), Fb, Nc, st())
                _lib.call("fpcdr_mvp_bwd", *tables, p(go), *(p(t) for t in g), Fb, Nc, st())
            else:
                _lib.call("fpcdr_mvp_fwd_indexed", *tables, *(p(t) for t in ix), p(out), Fb, Nc, st())
                _lib.call("fpcdr_mvp_bwd_indexed", *tables, *(p(t) for t in ix), p(go), *(p(t) for t in g), Fb, Nc, st())
            keep(f"mvp/{name}/{form}", mvp=out, **{f"{exact}_g{i}": t for i, t in enumerate(g)})
    torch.save(res, out_path)
    print(f"{_lib.LIB_PATH}: {len(res)} outputs -> {out_path}")


def compare(a_path, b_path, spread_paths):
    import itertools
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert list(a) == list(b), "the two files hold different outputs"
    # the largest difference of two tensors in units of the larger one's largest entry
    diff = lambda x, y: float((x.double() - y.double()).abs().max() / max(float(x.abs().max()), float(y.abs().max()), 1e-300)) if x.numel() else 0.0
    cls = lambda key: key.split('/')[0] if key.split('/')[0] in ('clip', 'mvp') else 'penalties'
    # the spread of A's library: per class of outputs, the largest difference any two of its runs show in any output of the class
    runs = [a] + [torch.load(path) for path in spread_paths]
    spread = {}
    for x, y in itertools.combinations(runs, 2):
        for key in a:
            if key.rsplit('/', 1)[1].startswith('loose_'):
                spread[cls(key)] = max(spread.get(cls(key), 0.0), diff(x[key], y[key]))
    exact = loose = loose_same = 0
    bad, worst = [], {}
    for key, x in a.items():
        y = b[key]
        if key.rsplit('/', 1)[1].startswith('loose_'):
            loose += 1
            loose_same += int(torch.equal(x, y))
            d = diff(x, y)
            worst[cls(key)] = max(worst.get(cls(key), 0.0), d)
            if spread_paths and d > spread[cls(key)]:
                bad.append((key, f"differs by {d:.3e} of its largest entry, the {len(runs)} runs of A's library by {spread[cls(key)]:.3e} at the most"))
        else:
            exact += 1
            if not torch.equal(x, y):
                bad.append((key, f"{int((x != y).sum())} elements differ"))
    fmt = lambda d: ", ".join(f"{k} {v:.3e}" for k, v in sorted(d.items()))
    print(f"{a_path} vs {b_path}: {exact} exact outputs, {loose} loose outputs ({loose_same} of them equal to the bit); largest relative "
          f"difference by class: {fmt(worst)}" + (f"; among {len(runs)} runs of A's library: {fmt(spread)}" if spread_paths else "")
          + f"; {len(bad)} fail")
    for item in bad:
        print("  DIFFERENT", *item)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index("--spread") + 1:] if "--spread" in sys.argv else []))
    run(sys.argv[1])

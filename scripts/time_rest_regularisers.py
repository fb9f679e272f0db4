"""HIP-event times of the rest-shape regularisers (csrc/mesh_reg.hip) at F = 32 meshes of the 15002-vertex UV sphere (two poles of degree 120),
the variants taking turns in one process:

  fpcdr_laplacian_penalty_fwd           the existing forward (gather + norms, then the finish kernel)
  fpcdr_laplacian_penalty_rest_fwd      the same against a rest shape: one more 12-byte read per vertex
  fpcdr_stretch_penalty                 value and gradient from one call (ring walk, then the finish kernel)
  torch mesh_edge_loss fwd + bwd        fit.mesh_edge_loss(x, topo, 0.1) and its autograd backward on the same tensors: the yardstick

Before timing, the stretch call's value and gradient are held against torch's for the same expression.

Algorithmic bytes per mesh of the stretch call: the positions once (12 V) and the gradient once (12 V), and per real slot the neighbour
index (4), its rest length (4) and a gathered position (12, from cache: every vertex is the neighbour of deg others): 24 V + 40 E.

    python scripts/time_rest_regularisers.py [--commit NAME] [--seconds S]
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 32


def main(commit, seconds):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import fitstep_ref
    from fpc_diffrend_amd import _lib, fit
    assert torch.cuda.is_available(), "needs the GPU"
    faces, V, pos = fitstep_ref.uv_sphere()
    rest = pos.clone()
    rest[:, 1] += 170.0
    topo = fit.MeshTopology(faces, V, 'cuda')
    rs = fit.RestShape(topo, rest.cuda())
    D, E = topo.nbr32.shape[0], rs.n_edges
    x = (rest[None] + 0.05 * torch.randn(F, V, 3, generator=torch.Generator().manual_seed(0))).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lap, gx = torch.empty_like(x), torch.empty_like(x)
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    per, out = torch.empty(F, dtype=torch.float32, device='cuda'), torch.empty((), dtype=torch.float32, device='cuda')
    w = 7.5

    def lap_plain():
        _lib.call("fpcdr_laplacian_penalty_fwd", p(x), p(topo.nbr32), p(topo.inv_deg), p(lap), p(acc), p(per), p(out), w, F, V, D, st())

    def lap_rest():
        _lib.call("fpcdr_laplacian_penalty_rest_fwd", p(x), p(topo.nbr32), p(topo.inv_deg), p(rs.lap), p(lap), p(acc), p(per), p(out), w,
                  F, V, D, st())

    def stretch():
        _lib.call("fpcdr_stretch_penalty", p(x), p(topo.nbr32), p(rs.len), 0.0, p(gx), p(acc), p(per), p(out), w, F, V, D, E, st())

    leaf = x.clone().requires_grad_(True)

    def torch_edge():
        leaf.grad = None
        (w * fit.mesh_edge_loss(leaf, topo, 0.1)).backward()

    # faster and different is not faster: the constant-target form against torch's expression, value and gradient
    _lib.call("fpcdr_stretch_penalty", p(x), p(topo.nbr32), None, 0.1, p(gx), p(acc), p(per), p(out), w, F, V, D, E, st())
    torch_edge()
    tv = float(w * fit.mesh_edge_loss(x, topo, 0.1))
    rel = float((gx - leaf.grad).norm() / leaf.grad.norm())
    print(f"commit {commit}; F = {F} meshes of V = {V}, D = {D}, E = {E}; stretch(target 0.1) {float(out):.6f} torch {tv:.6f}, gradient rel-L2 "
          f"against torch's {rel:.2e}", flush=True)
    assert abs(float(out) - tv) <= 1e-4 * abs(tv) and rel < 1e-4
    variants = [("fpcdr_laplacian_penalty_fwd", lap_plain), ("fpcdr_laplacian_penalty_rest_fwd", lap_rest),
                ("fpcdr_stretch_penalty", stretch), ("torch mesh_edge_loss fwd + bwd", torch_edge)]
    for _, fn in variants:                  # warm-up: code objects, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    calls = 20
    turns = {name: [] for name, _ in variants}
    t0 = time.perf_counter()
    while min(sum(v) * calls for v in turns.values()) < seconds * 1e3 or len(turns[variants[0][0]]) < 10:
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            turns[name].append(e0.elapsed_time(e1) / calls)
        if time.perf_counter() - t0 > 90:
            break
    med = {}
    for name, _ in variants:
        t = np.sort(np.asarray(turns[name])) * 1e3
        med[name] = float(np.median(t))
        print(f"  {name:36s} median {med[name]:8.2f} us a call (min {t[0]:.2f}, max {t[-1]:.2f}, {t.size} turns of {calls} calls)", flush=True)
    print(f"  rest forward / plain forward: {med['fpcdr_laplacian_penalty_rest_fwd'] / med['fpcdr_laplacian_penalty_fwd']:.3f}", flush=True)
    ratio = med['fpcdr_stretch_penalty'] / med['torch mesh_edge_loss fwd + bwd']
    gbs = F * (24.0 * V + 40.0 * E) / (med['fpcdr_stretch_penalty'] * 1e-6) / 1e9
    print(f"  fpcdr_stretch_penalty / torch: {ratio:.3f}; {F * (24 * V + 40 * E) / 1e6:.1f} MB algorithmic -> {gbs:.0f} GB/s", flush=True)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")))

"""HIP-event times of the bending term (csrc/mesh_reg.hip) at F = 32 meshes of the 15002-vertex UV sphere (45000 hinges, two poles with 240
hinge corners each), the variants taking turns in one process:

  fpcdr_bend_penalty                        value and gradient: the hinge pass, the per-vertex gather, the finish kernel
  fpcdr_bend_penalty, value only            grad_x = NULL: the hinge pass without its stores, the finish kernel
  torch mesh_normal_consistency fwd + bwd   fit.mesh_normal_consistency(x, topo) and its autograd backward on the same tensors: the yardstick
  (--alt-lib PATH)                          the same call from a second build of the library, e.g. one compiled with
                                            -DFPCDR_BEND_COMPONENT_MAJOR=0: the other layout of the hinge_grad scratch

Before timing, the call without a rest table is held against torch's expression: the value, and the gradient's relative L2.

Algorithmic bytes per mesh of the full call: per hinge its four indices (16), its rest angle (8), four gathered positions (48, from cache:
a vertex is a corner of ~12 hinges) and twelve floats of corner gradients written (48) and read back by the gather (48, with 4 bytes of
incidence each corner: 16); per vertex the gradient (12): 184 H + 12 V.

    python scripts/time_bend.py [--commit NAME] [--seconds S] [--alt-lib PATH]
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 32


def main(commit, seconds, alt_lib):
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
    hinge_vtx, hinge_inc, H, K = topo.hinges()
    cs = rs.bend_cs
    x = (rest[None] + 0.05 * torch.randn(F, V, 3, generator=torch.Generator().manual_seed(0))).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gx, hg = torch.empty_like(x), torch.empty(F * H * 12, dtype=torch.float32, device='cuda')
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    per, out = torch.empty(F, dtype=torch.float32, device='cuda'), torch.empty((), dtype=torch.float32, device='cuda')
    w = 7.5

    def bend():
        _lib.call("fpcdr_bend_penalty", p(x), p(hinge_vtx), p(cs), p(hinge_inc), p(hg), p(gx), p(acc), p(per), p(out), w, F, V, H, K, st())

    def bend_value():
        _lib.call("fpcdr_bend_penalty", p(x), p(hinge_vtx), p(cs), None, None, None, p(acc), p(per), p(out), w, F, V, H, K, st())

    leaf = x.clone().requires_grad_(True)

    def torch_mnc():
        leaf.grad = None
        (w * fit.mesh_normal_consistency(leaf, topo)).backward()

    # faster and different is not faster: without a table the call is torch's expression, value and gradient
    _lib.call("fpcdr_bend_penalty", p(x), p(hinge_vtx), None, p(hinge_inc), p(hg), p(gx), p(acc), p(per), p(out), w, F, V, H, K, st())
    torch_mnc()
    tv = float(w * fit.mesh_normal_consistency(x, topo))
    rel = float((gx - leaf.grad).norm() / leaf.grad.norm())
    print(f"commit {commit}; F = {F} meshes of V = {V}, H = {H}, K = {K}; bend(no table) {float(out):.6f} torch {tv:.6f}, gradient rel-L2 "
          f"against torch's {rel:.2e}", flush=True)
    assert abs(float(out) - tv) <= 1e-4 * abs(tv) and rel < 1e-4
    plain_gx = gx.clone()
    variants = [("fpcdr_bend_penalty", bend), ("fpcdr_bend_penalty, value only", bend_value),
                ("torch mesh_normal_consistency fwd + bwd", torch_mnc)]
    if alt_lib:
        alt = ctypes.CDLL(alt_lib)
        alt.fpcdr_bend_penalty.restype, alt.fpcdr_bend_penalty.argtypes = _lib.SYMBOLS["fpcdr_bend_penalty"]
        gx2 = torch.empty_like(gx)

        def bend_alt(table=cs):
            rc = alt.fpcdr_bend_penalty(p(x), p(hinge_vtx), p(table), p(hinge_inc), p(hg), p(gx2), p(acc), p(per), p(out), w, F, V, H, K, st())
            assert rc == 0

        bend_alt(None)      # (the gather sums the same numbers in the same order: the layout changes no bit of grad_x)
        assert torch.equal(gx2, plain_gx), "the second library gives another gradient"
        variants.append((f"fpcdr_bend_penalty of {os.path.basename(alt_lib)}", bend_alt))
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
        print(f"  {name:44s} median {med[name]:8.2f} us a call (min {t[0]:.2f}, max {t[-1]:.2f}, {t.size} turns of {calls} calls)", flush=True)
    ratio = med['fpcdr_bend_penalty'] / med['torch mesh_normal_consistency fwd + bwd']
    nbytes = F * (184.0 * H + 12.0 * V)
    print(f"  fpcdr_bend_penalty / torch: {ratio:.4f}; {nbytes / 1e6:.1f} MB algorithmic -> {nbytes / (med['fpcdr_bend_penalty'] * 1e-6) / 1e9:.0f} GB/s",
          flush=True)
    if alt_lib:
        print(f"  second library / this one: {med[variants[-1][0]] / med['fpcdr_bend_penalty']:.3f}", flush=True)
    assert ratio < 1.0, "the call must be faster than the torch expression"


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")), arg("--alt-lib", None))

"""HIP-event times of the landmark term (csrc/landmark.hip) at cfg3's shape -- F = 32 frames x 9 views, the 15002-vertex mesh, L = 68
landmarks --, the variants taking turns in one process:

  fpcdr_landmark_penalty                   value and both gradients: the pass over the landmarks, the gather over all V, the finish
  fpcdr_landmark_penalty, Charbonnier      the same with a scale
  fpcdr_landmark_penalty, value only       grad_x = grad_mvp = NULL: the pass over the landmarks and the finish
  fpcdr_motion_penalty order 2             at the same F, V on the same build: the yardstick -- both write one dense [F,V,3] gradient
                                           from one gather

Before timing, the call is held against the float64 statement (tests/landmark_ref.py): the value, and both gradients' relative L2.

Algorithmic bytes of the full call: the dense gradient written once (12 F V) and the first row of the incidence table read once per frame
(4 F V); the landmarks' own traffic (F Nc L entries of a few dozen bytes) is three orders of magnitude below it.

With --step: a cfg3 step (bench.py's flagship configuration) with weight_landmark = 0 and with the term on, taking turns, host clock
around `steps` steps that end in a synchronise.  A commit whose FitConfig has no such option (the parent) gets the "off" figure alone: run
the script there too, in turns with this one, to compare the step with the term off against it.

--step --frozen: the same with every learning rate at 0: the geometry stays what it was, so the difference is the term's own cost.

    python scripts/time_landmark.py [--commit NAME] [--seconds S] [--step [--frozen]]
"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, NC, L = 32, 9, 68
H, W = 1080, 1920


def _points(sc):
    """68 points of the mesh: two in three at a vertex, one in three inside a face, spread over the mesh."""
    V, T = sc.n_vertices, sc.pos_idx.shape[0]
    return [({'face': (l * 7919) % T, 'bary': (0.5, 0.3, 0.2)} if l % 3 == 2 else {'vertex': (l * 104729) % V}) for l in range(L)]


def calls(seconds):
    import numpy as np
    import torch
    import landmark_ref as LR
    from time_motion import time_turns
    from fpc_diffrend_amd import _lib, fit, scene
    from helpers import scene_mvps
    sc = scene.cfg('cfg3')
    V = sc.n_vertices
    points = _points(sc)
    lms = fit.LandmarkSet(points, V, sc.pos_idx, 'cuda')
    g = torch.Generator().manual_seed(0)
    truth = (torch.tensor(sc.v_base)[None] + torch.tensor(sc.weights_gt) @ torch.tensor(sc.blendshapes).t()).reshape(F, V, 3)
    x = (truth + 0.05 * torch.randn(F, V, 3, generator=g)).float().contiguous()
    mvp = scene_mvps(sc, list(range(NC)), list(range(F))).contiguous()
    obs = torch.tensor(fit.project_landmarks(sc, points)).reshape(F * NC, L, 3).float()
    obs[..., :2] += 4.0 * torch.randn(F * NC, L, 2, generator=g)
    obs[..., 2] = torch.where(torch.rand(F * NC, L, generator=g) < 0.2, torch.zeros(()), 0.2 + 0.8 * torch.rand(F * NC, L, generator=g))
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    xd, md, od = x.cuda(), mvp.cuda(), obs.cuda().contiguous()
    gx, gm, gmo = torch.empty_like(xd), torch.empty_like(md), torch.empty_like(xd)
    scratch = torch.empty(F * NC * L * 3, dtype=torch.float32, device='cuda')
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    per, out = torch.empty(F, dtype=torch.float32, device='cuda'), torch.empty((), dtype=torch.float32, device='cuda')
    w, c = 7.5, 4.0
    inv_c = fit.landmark_inv_scale(c)

    def call(ic, grad=True):
        _lib.call("fpcdr_landmark_penalty", p(xd), p(md), p(lms.vtx), p(lms.bary), p(lms.w), p(lms.inc), p(od), ic, W, H,
                  p(scratch) if grad else None, p(gx) if grad else None, p(gm) if grad else None, None, p(acc), p(per), p(out), w, F, NC, V, L,
                  lms.K, st())

    def motion():
        _lib.call("fpcdr_motion_penalty", p(xd), None, None, 0.0, 2, p(gmo), p(acc), p(per), p(out), w, F, V, st())

    # faster and different is not faster
    vtx, bary = lms.vtx.cpu().numpy(), lms.bary.cpu().numpy()
    for ic in (0.0, inv_c):
        call(ic)
        ref = LR.landmark(x, mvp, vtx, bary, None, obs, w, H, W, ic)
        rx = float((gx.cpu().double() - ref['grad_x'][0]).norm() / ref['grad_x'][0].norm())
        rm = float((gm.cpu().double() - ref['grad_mvp'][0]).norm() / ref['grad_mvp'][0].norm())
        print(f"  inv_c = {ic:g}: call {float(out):.6f} float64 {float(ref['value'][0]):.6f}, rel-L2 grad_x {rx:.2e} grad_mvp {rm:.2e}; "
              f"{int(ref['live'].sum())} of {ref['live'].numel()} entries live, K = {lms.K}", flush=True)
        assert abs(float(out) - float(ref['value'][0])) <= 1e-4 * float(ref['value'][0]) and rx < 1e-4 and rm < 1e-4
    variants = [("fpcdr_landmark_penalty", lambda: call(0.0)),
                ("fpcdr_landmark_penalty, Charbonnier", lambda: call(inv_c)),
                ("fpcdr_landmark_penalty, value only", lambda: call(0.0, False)),
                ("fpcdr_motion_penalty order 2", motion)]
    med = time_turns(variants, seconds)
    t, tm = med["fpcdr_landmark_penalty"], med["fpcdr_motion_penalty order 2"]
    nbytes = 16.0 * F * V
    print(f"  fpcdr_landmark_penalty / fpcdr_motion_penalty: {t / tm:.3f}; value only {med['fpcdr_landmark_penalty, value only']:.2f} us "
          f"(the pass over the landmarks and the finish), so the gather is {t - med['fpcdr_landmark_penalty, value only']:.2f} us: "
          f"{nbytes / 1e6:.2f} MB algorithmic -> {nbytes / ((t - med['fpcdr_landmark_penalty, value only']) * 1e-6) / 1e9:.0f} GB/s", flush=True)
    if t > 2.0 * tm:
        print("  more than twice the motion term's: the time goes where the line above says (value only = landmarks pass + finish; the rest = "
              "the gather)", flush=True)


def step_times(seconds, steps=20, frozen=False):
    """A cfg3 step with the term off and on, taking turns; a FitConfig without the option (the parent commit) times "off" alone.
    frozen: every learning rate 0, so that both Fitters keep rendering the geometry they started with -- the time of the pixel kernels
    follows the geometry, and a fit that the landmarks pull elsewhere than the pixels do is a different workload after a few hundred steps."""
    import dataclasses
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, scene
    import bench
    sc = scene.cfg('cfg3')
    has = 'weight_landmark' in {f.name for f in dataclasses.fields(fit.FitConfig)}
    if has:
        sc.landmark_points = _points(sc)
        sc.landmarks = fit.project_landmarks(sc, sc.landmark_points).astype(np.float32)
    fitters, targets = {}, None
    for name, kw in (("off", {}),) + ((("on", dict(weight_landmark=1.0)),) if has else ()):
        if frozen:
            kw = dict(kw, lr_base=0.0, lr_t=0.0, lr_q=0.0)
        cfg = dataclasses.replace(bench.workload_config('cfg3')[0], **kw)      # (the bench's own configuration of the workload)
        fitters[name] = fit.Fitter(sc, cfg, device='cuda', targets=targets)
        targets = fitters[name].targets                                          # (rendered once)
        for _ in range(5):
            fitters[name].step()
    torch.cuda.synchronize()
    turns = {name: [] for name in fitters}
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < max(seconds, 1.0) * 6 or len(turns["off"]) < 5:
        for name, ft in fitters.items():
            torch.cuda.synchronize()
            a = time.perf_counter()
            for _ in range(steps):
                ft.step()
            torch.cuda.synchronize()
            turns[name].append((time.perf_counter() - a) / steps * 1e3)
        if time.perf_counter() - t0 > 120:
            break
    for name in fitters:
        t = np.sort(np.asarray(turns[name]))
        print(f"  cfg3 step{', learning rates 0' if frozen else ''}, weight_landmark {name:3s}: median {np.median(t):.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns of {steps} steps; "
              f"{sc.n_frames} frames, {sc.n_vertices} vertices)", flush=True)


def main(commit, seconds, step, frozen=False):
    root = os.environ.get("FPCDR_TIME_ROOT", ROOT)      # (another build of the package: its tree in front of this one)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, root)
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"commit {commit}; F = {F} frames x {NC} views, L = {L}", flush=True)
    if step:
        return step_times(seconds, frozen=frozen)
    calls(seconds)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")), "--step" in sys.argv, "--frozen" in sys.argv)

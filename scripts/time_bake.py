"""HIP-event times of the texture bake (csrc/bake.hip, DESIGN.md 3 "Bake rule") -> profiles/bake_time.txt: fpcdr_bake_accumulate_u8 on a
whole batch, fpcdr_bake_resolve, one pass of fpcdr_bake_dilate and the whole Fitter.bake_texture, at the cfg3 batch (288 images of
1080 x 1920 from scene.cfg('cfg3'), a 1024 x 1024 texture) and at one image of 1600 x 1200 (scene.cfg('ref'), one frame, one camera),
beside the yardstick: the same two sums as two backward calls of ops.texture on the same coordinates (gradient = the capture as float
on covered pixels, gradient = 1 on covered pixels), with the conversions they need, in the same process, the variants taking turns.
Steady state: every variant is warmed up first; medians with minimum and maximum.

The inputs are the rasteriser's own output for the scene at the Fitter's start parameters, so coverage and the texel footprint are those
of a real bake.  Algorithmic bytes of the accumulate kernel per pixel: rast.w (4) for every pixel, texc (8) and the capture (1) for a
covered one; atomics: two per tap of non-zero weight.  The bake runs once per fit: no speed is a pass condition.

    python scripts/time_bake.py [--out FILE]      every case in a process of its own, each under `timeout`; stops at the first failure
    python scripts/time_bake.py --case cfg3       one case in this process (cfg3 | single)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"cfg3": ("cfg3", 32, tuple(range(9))), "single": ("ref", 1, (0,))}
LIMIT = {"cfg3": 540, "single": 240}      # seconds a case may take (cfg3: 288 reference images are rendered first)


def launcher(out_path):
    text = []
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(LIMIT[case]), sys.executable, os.path.abspath(__file__), "--case", case]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        text.append(p.stdout)
        if p.returncode != 0:
            print(f"case {case}: exit status {p.returncode}; stopping", flush=True)
            return p.returncode
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("".join(text))
    return 0


def run(case, seconds=1.0):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from fpc_diffrend_amd import fit, ops as dr, scene
    assert torch.cuda.is_available(), "needs the GPU"
    name, n_frames, cams = CASES[case]
    sc = scene.cfg(name, n_frames=n_frames)
    ft = fit.Fitter(sc, fit.FitConfig(max_iter=80000, cam_idxs=cams, init_texture="random"), device="cuda")
    H, W = ft.resolution
    Ht, Wt, _ = ft.tex_opt.shape
    # the batch's rast / texc, as bake_texture forms them
    glctx = dr.RasterizeGLContext(output_db=False, device="cuda")
    rasts, texcs = [], []
    with torch.no_grad():
        for lo in range(0, n_frames, 4):
            ids = torch.arange(lo, min(lo + 4, n_frames), device="cuda")
            pos_clip = fit.transform_clip_batched(ft.mvp(ids), ft.vertices(ids).reshape(len(ids), -1, 3))
            rast, _ = dr.rasterize(glctx, pos_clip, ft.pos_idx, resolution=(H, W))
            texc, _ = dr.interpolate(ft.uv[None], rast, ft.uv_idx)
            rasts.append(rast)
            texcs.append(texc)
    rast, texc = torch.cat(rasts), torch.cat(texcs)
    del rasts, texcs
    ref = ft.targets.reshape(-1, H, W)
    N = rast.shape[0]
    px = N * H * W
    cov = rast[..., 3] > 0
    n_cov = int(cov.sum())
    # taps of non-zero weight among the covered pixels (the rule's float32 arithmetic, 'wrap')
    uv = texc[cov]
    n_taps = 0
    fr = []
    for axis, n in ((0, Wt), (1, Ht)):
        p = uv[:, axis] - torch.floor(uv[:, axis])
        x = p * float(n) - 0.5
        a = torch.floor((x - torch.floor(x)) * 256.0)
        fr.append(((a < 256).long(), (a > 0).long()))          # (first tap of the axis has weight, second has)
    n_taps = int((fr[0][0] * fr[1][0] + fr[0][1] * fr[1][0] + fr[0][0] * fr[1][1] + fr[0][1] * fr[1][1]).sum())
    del uv, fr
    bpp = 4.0 + 9.0 * n_cov / px

    acc = torch.zeros(Ht, Wt, 2, dtype=torch.int64, device="cuda")
    plane = torch.empty(Ht, Wt, device="cuda")
    mask = torch.empty(Ht, Wt, dtype=torch.bool, device="cuda")
    plane2, mask2 = torch.empty_like(plane), torch.empty_like(mask)
    tex = torch.zeros(1, Ht, Wt, 1, device="cuda", requires_grad=True)
    out = dr.texture(tex, texc, filter_mode="linear")          # (the forward is not part of the yardstick: its graph is kept)

    def accumulate():
        acc.zero_()
        dr.bake_accumulate(texc, rast, ref, acc)

    def resolve():
        dr._lib.call("fpcdr_bake_resolve", dr._ptr(acc), dr._ptr(plane), dr._ptr(mask), Ht, Wt, 255.0, 1, dr._stream())

    def dilate():
        dr._lib.call("fpcdr_bake_dilate", dr._ptr(plane), dr._ptr(mask), dr._ptr(plane2), dr._ptr(mask2), Ht, Wt, dr._stream())

    def yardstick():
        c = rast[..., 3:] > 0
        g_num = torch.where(c, ref[..., None].to(torch.float32), 0.0)
        num, = torch.autograd.grad(out, tex, g_num, retain_graph=True)
        den, = torch.autograd.grad(out, tex, c.to(torch.float32), retain_graph=True)
        return num, den

    def whole():
        ft.bake_texture(assign=False)

    variants = [("fpcdr_bake_accumulate_u8 (+ zero fill)", accumulate), ("two ops.texture backward calls (yardstick)", yardstick),
                ("fpcdr_bake_resolve", resolve), ("fpcdr_bake_dilate, one pass", dilate), ("Fitter.bake_texture, whole", whole)]
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    # faster and different is not faster: the integer sums against the float ones
    accumulate()
    num, den = yardstick()
    a = acc.to(torch.float64)
    e_num = float((a[..., 0] / 65536.0 - num[0, :, :, 0].double()).abs().max() / num.abs().max())
    e_den = float((a[..., 1] / 65536.0 - den[0, :, :, 0].double()).abs().max() / den.abs().max())
    print(f"{case}: {N} x {H} x {W} ({px / 1e6:.1f} Mpx), texture {Ht} x {Wt}, coverage {100.0 * n_cov / px:.1f} %, {n_taps / max(n_cov, 1):.2f} "
          f"taps of non-zero weight a covered pixel; largest |num / 65536 - yardstick| {e_num:.2e} of the largest sum, den {e_den:.2e}", flush=True)
    assert e_num < 2.0 / 256 and e_den < 2.0 / 256
    turns = {name: [] for name, _ in variants}
    t0 = time.perf_counter()
    while len(turns[variants[0][0]]) < 30 or (min(sum(v) for v in turns.values()) < seconds * 1e3 and time.perf_counter() - t0 < 8):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            turns[name].append(e0.elapsed_time(e1))
        if time.perf_counter() - t0 > 25:
            break
    med = {}
    for name, _ in variants:
        t = np.sort(np.asarray(turns[name]))
        med[name] = float(np.median(t))
        extra = ""
        if name.startswith("fpcdr_bake_accumulate"):
            extra = (f"  {bpp:.2f} B/px = {bpp * px / (med[name] * 1e-3) / 1e12:.2f} TB/s; {2 * n_taps / 1e6:.1f} M atomics = "
                     f"{2 * n_taps / (med[name] * 1e-3) / 1e9:.2f} G atomics/s")
        print(f"  {name:44s} median {med[name]:.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns){extra}", flush=True)
    a, b = variants[0][0], variants[1][0]
    print(f"  accumulate: {med[b] / med[a]:.2f} x the speed of the yardstick", flush=True)


if __name__ == "__main__":
    if "--case" in sys.argv:
        run(sys.argv[sys.argv.index("--case") + 1])
    else:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "bake_time.txt")
        sys.exit(launcher(out))

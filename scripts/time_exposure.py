"""HIP-event times of the exposure equalisation (csrc/exposure.hip, DESIGN.md 3 "Exposure rule") -> profiles/exposure_time.txt, at 18 and
288 images of 1080 x 1920 (scene.cfg('cfg3'), 2 and 32 frames x 9 cameras), the variants of a case taking turns in one process:

  fpcdr_exposure_sums against fpcdr_robust_loss without gradient on the same tensors -- the project's streaming yardstick over the
      same planes: colour (4 C), rast (16) and the capture (1 byte a pixel);
  fpcdr_apply_lut_u8 against the torch gather lut[cam][img.long()] written back, and against its floor of 2 bytes a pixel;
  the whole Fitter.equalise_exposure() -- fit and a table applied -- against Fitter.bake_texture().

The inputs are the Fitter's own render at its start parameters (Fitter.render_full), so coverage is that of a real call.  Steady state:
every variant is warmed up first; medians with minimum and maximum.  The equalisation runs once or twice per fit: no speed is a pass
condition.  Equality of what is timed: the sums against tests/exposure_ref.py on the first image, the apply against the gather.

    python scripts/time_exposure.py [--out FILE]      every case in a process of its own, each under `timeout`; stops at the first failure
    python scripts/time_exposure.py --case 18         one case in this process (18 | 288)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"18": 2, "288": 32}          # frames of cfg3, nine cameras each
LIMIT = {"18": 300, "288": 560}       # seconds a case may take (288 reference images are rendered first)


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
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import exposure_ref as R
    from fpc_diffrend_amd import exposure, fit, ops as dr, scene
    assert torch.cuda.is_available(), "needs the GPU"
    n_frames = CASES[case]
    sc = scene.cfg('cfg3', n_frames=n_frames)
    ft = fit.Fitter(sc, fit.FitConfig(max_iter=80000, cam_idxs=tuple(range(9))), device="cuda")
    H, W = ft.full_resolution
    Nc = len(ft.cam_idxs)
    glctx = dr.RasterizeGLContext(output_db=False, device="cuda")
    cols, rasts = [], []
    with torch.no_grad():
        for lo in range(0, n_frames, 4):
            c, r = ft.render_full(glctx, torch.arange(lo, min(lo + 4, n_frames), device="cuda"))
            cols.append(c.contiguous())
            rasts.append(r)
    colour, rast = torch.cat(cols), torch.cat(rasts)
    del cols, rasts
    ref = ft.full_targets.reshape(-1, H, W)
    N, C = colour.shape[0], colour.shape[3]
    px = N * H * W
    plane_bytes = px * (4 * C + 16 + 1)
    sums = torch.zeros(N, 6, dtype=torch.int64, device="cuda")
    images = ref.clone()
    lut = torch.from_numpy(np.stack([np.roll(np.arange(256, dtype=np.uint8), c + 1) for c in range(Nc)])).cuda()
    cams = (torch.arange(N, device="cuda") % Nc).to(torch.int32)
    swap = np.tile((np.arange(256) ^ 1).astype(np.uint8), (Nc, 1))      # an involution: two applications give the captures back

    def exposure_sums():
        dr.exposure_sums(colour, rast, ref, sums=sums)

    def robust():
        dr.robust_loss_call(colour, rast, ref, 'l2', None, 1.0, want_grad=False)

    def apply_lut():
        dr._lib.call("fpcdr_apply_lut_u8", dr._ptr(images), dr._ptr(lut), dr._ptr(cams), Nc, N, H * W, dr._stream())

    def gather():
        images.copy_(lut[cams.long()[:, None, None], images.long()])

    def whole():
        ft.equalise_exposure(apply=False)
        ft._apply_exposure(swap)

    def bake():
        ft.bake_texture(assign=False)

    variants = [("fpcdr_exposure_sums", exposure_sums), ("fpcdr_robust_loss, no gradient (yardstick)", robust),
                ("fpcdr_apply_lut_u8", apply_lut), ("torch gather lut[cam][img.long()] (yardstick)", gather),
                ("Fitter.equalise_exposure, whole (fit + a table applied)", whole), ("Fitter.bake_texture, whole (yardstick)", bake)]
    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    # equality of what is timed
    sums.zero_()
    exposure_sums()
    want = R.sums(colour[:1].cpu().numpy(), rast[:1].cpu().numpy(), ref[:1].cpu().numpy())
    assert np.array_equal(sums[:1].cpu().numpy(), want), "the sums differ from the statement"
    n_counted = int(sums[:, 0].sum()) // C
    a, b = ref.clone(), ref.clone()
    dr.apply_lut_u8(a, lut, cams)
    b.copy_(lut[cams.long()[:, None, None], b.long()])
    assert torch.equal(a, b), "the apply differs from the gather"
    del a, b
    cov = float((rast[..., 3] > 0).float().mean())
    print(f"case {case}: {N} x {H} x {W} x {C} ({px / 1e6:.1f} Mpx), coverage {100.0 * cov:.1f} %, counted pixels {100.0 * n_counted / px:.1f} %; "
          f"sums equal the statement on image 0, the apply equals the gather", flush=True)
    turns = {name: [] for name, _ in variants}
    t0 = time.perf_counter()
    while len(turns[variants[0][0]]) < 20 or (min(sum(v) for v in turns.values()) < seconds * 1e3 and time.perf_counter() - t0 < 20):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            turns[name].append(e0.elapsed_time(e1))
        if time.perf_counter() - t0 > 60:
            break
    med = {}
    for name, _ in variants:
        t = np.sort(np.asarray(turns[name]))
        med[name] = float(np.median(t))
        print(f"  {name:58s} median {med[name]:9.3f} ms  (min {t[0]:.3f}, max {t[-1]:.3f}, {len(t)} turns)", flush=True)
    s, y = med["fpcdr_exposure_sums"], med["fpcdr_robust_loss, no gradient (yardstick)"]
    print(f"  planes colour + rast + capture = {4 * C + 16 + 1} B/px: exposure_sums {plane_bytes / s / 1e9:.2f} TB/s, robust_loss "
          f"{plane_bytes / y / 1e9:.2f} TB/s; ratio of times sums / yardstick {s / y:.2f}")
    s, y = med["fpcdr_apply_lut_u8"], med["torch gather lut[cam][img.long()] (yardstick)"]
    print(f"  apply: 2 B/px = {2 * px / 1e9:.3f} GB: {2 * px / s / 1e9:.2f} TB/s; ratio of times apply / gather {s / y:.3f}")
    s, y = med["Fitter.equalise_exposure, whole (fit + a table applied)"], med["Fitter.bake_texture, whole (yardstick)"]
    print(f"  whole: equalise_exposure / bake_texture {s / y:.2f}", flush=True)


if __name__ == "__main__":
    if "--case" in sys.argv:
        run(sys.argv[sys.argv.index("--case") + 1])
    else:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "exposure_time.txt")
        sys.exit(launcher(out))

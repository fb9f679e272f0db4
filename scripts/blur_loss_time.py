"""HIP-event time of fpcdr_blur_loss (the blurred pixel loss, csrc/blur.hip), with and without the gradient, on a batch of 32 images of
1080 x 1920 and on one image of 1600 x 1200 (one channel, the default 31-tap kernel, sigma 5), beside the yardstick: the same loss as a
torch expression (F.pad(reflect) + two conv2d, tests/blur_ref.py's loss_plain) with its autograd backward, on the same GPU in the same
run, the variants taking turns.

Algorithmic bytes per pixel of a call with C channels: the row pass reads colour (4 C), the coverage record (16) and the capture (1) and
writes a plane (4 C); the column pass reads and writes a plane (8 C): 16 C + 17 for the value; the two adjoint passes read and write a
plane each and the last one reads the coverage again: 32 C + 33 with the gradient.

    python scripts/blur_loss_time.py                  every case in a process of its own, each under `timeout`; stops at the first failure
    python scripts/blur_loss_time.py --case batch     one case in this process (batch | single)
    python scripts/blur_loss_time.py --case batch --kernel    a few calls only (the run to put under rocprofv3 --kernel-trace --stats)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"batch": (32, 1080, 1920, 1), "single": (1, 1600, 1200, 1)}
KERNEL_SIZE, SIGMA = 31, 5.0
HBM_PEAK = 8.0e12        # bytes/s, MI355X spec
LIMIT = {"batch": 420, "single": 240}      # seconds a case may take (torch's first convolutions look for their algorithm)


def launcher(extra):
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(LIMIT[case]), sys.executable, os.path.abspath(__file__), "--case", case] + extra
        rc = subprocess.call(cmd)
        if rc != 0:
            print(f"case {case}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


def run(case, kernel_only, seconds=1.0):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import blur_ref
    from fpc_diffrend_amd import ops as dr
    assert torch.cuda.is_available(), "needs the GPU"
    B, H, W, C = CASES[case]
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    colour = torch.rand(B, H, W, C, generator=g).cuda()
    rast = torch.zeros(B, H, W, 4, device='cuda')
    rast[..., 3] = (torch.rand(B, H, W, generator=g) > 0.4).float().cuda() * 7
    ref = torch.randint(0, 141, (B, H, W), generator=g, dtype=torch.uint8).cuda()
    taps = dr.gaussian_taps(KERNEL_SIZE, SIGMA)
    gs = 1.0 / colour.numel()
    cover = rast[..., 3]

    def torch_value():
        with torch.no_grad():
            return blur_ref.loss_plain(colour, cover, ref, taps)

    def torch_grad():
        x = colour.detach().requires_grad_(True)
        blur_ref.loss_plain(x, cover, ref, taps).backward()
        return x.grad

    variants = [("fpcdr_blur_loss value", 16.0 * C + 17.0, lambda: dr.blur_loss_call(colour, rast, ref, taps, gs, want_grad=False)),
                ("fpcdr_blur_loss value+grad", 32.0 * C + 33.0, lambda: dr.blur_loss_call(colour, rast, ref, taps, gs)),
                ("torch value (yardstick)", 16.0 * C + 17.0, torch_value),
                ("torch value+grad (yardstick)", 32.0 * C + 33.0, torch_grad)]
    for _, _, fn in variants:                  # warm-up: code objects, allocator, torch's choice of convolution
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # faster and different is not faster: the two agree at this size
    s, grad, _ = dr.blur_loss_call(colour, rast, ref, taps, gs)
    tg = torch_grad()
    tv = float(torch_value())
    rel = float((grad - tg).norm() / tg.norm())
    print(f"{case}: {B} x {H} x {W} x {C} ({px / 1e6:.1f} Mpx), {KERNEL_SIZE} taps, sigma {SIGMA}; loss {float(s) * gs:.6f} torch {tv:.6f}; "
          f"gradient rel-L2 against torch's {rel:.2e}", flush=True)
    assert abs(float(s) * gs - tv) <= 1e-4 * abs(tv) and rel < 1e-4
    if kernel_only:
        return
    calls = 10 if case == "single" else 2
    turns = {name: [] for name, _, _ in variants}
    t0 = time.perf_counter()
    while min(sum(v) for v in turns.values()) < seconds * 1e3 or len(turns[variants[0][0]]) < 10:
        for name, _, fn in variants:
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
    for name, bpp, _ in variants:
        t = np.sort(np.asarray(turns[name]))
        med[name] = float(np.median(t))
        rate = bpp * px / (med[name] * 1e-3)
        print(f"  {name:30s} {bpp:5.1f} B/px  median {med[name]:.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f}, {t.size} turns of {calls} calls)  "
              f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.1f} % of 8 TB/s", flush=True)
    for a, b in (("fpcdr_blur_loss value", "torch value (yardstick)"), ("fpcdr_blur_loss value+grad", "torch value+grad (yardstick)")):
        print(f"  {a}: {med[b] / med[a]:.2f} x the speed of the yardstick", flush=True)


if __name__ == "__main__":
    if "--case" in sys.argv:
        run(sys.argv[sys.argv.index("--case") + 1], "--kernel" in sys.argv)
    else:
        sys.exit(launcher([a for a in sys.argv[1:] if a == "--kernel"]))

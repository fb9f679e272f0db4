"""HIP-event time of fpcdr_norm_loss (the locally normalised pixel loss, csrc/norm.hip), value only and value with gradient, on a batch of
32 images of 1080 x 1920 (one channel, 31 taps, sigma 5, eps 2), beside fpcdr_blur_loss at the same shape in the same process, the four
variants taking turns.  Before timing, value and gradient are held against the torch statement of the rule (tests/norm_ref.py's
loss_plain) on a crop of the batch.

Algorithmic bytes per pixel of a call with C channels: rows read colour (4 C), the coverage record (16) and the capture (1) and write
four row sums (16 C); columns read and write that plane (32 C); the pointwise pass reads the statistics (16 C) and the inputs again
(4 C + 17) and writes d (4 C): 76 C + 34 for the value.  With the gradient the pointwise pass also writes (P, q) and p (12 C), the column
adjoint reads and writes (P, q) (16 C), the row adjoint reads it, p, colour and the coverage (16 C + 16) and writes the gradient (4 C):
124 C + 50.

    python scripts/norm_loss_time.py [--commit NAME] [--seconds S]
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (32, 1080, 1920, 1)
KERNEL_SIZE, SIGMA, EPS = 31, 5.0, 2.0
HBM_PEAK = 8.0e12        # bytes/s, MI355X spec


def main(commit, seconds):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import norm_ref
    from fpc_diffrend_amd import ops as dr
    assert torch.cuda.is_available(), "needs the GPU"
    B, H, W, C = SHAPE
    px = B * H * W
    g = torch.Generator().manual_seed(0)
    colour = torch.rand(B, H, W, C, generator=g).cuda()
    rast = torch.zeros(B, H, W, 4, device='cuda')
    rast[..., 3] = (torch.rand(B, H, W, generator=g) > 0.4).float().cuda() * 7
    ref = torch.randint(0, 141, (B, H, W), generator=g, dtype=torch.uint8).cuda()
    taps = dr.gaussian_taps(KERNEL_SIZE, SIGMA)
    gs = 1.0 / colour.numel()
    # faster and different is not faster: one image of the batch, cropped, against the torch statement
    cc, cr, cf = colour[:1, :270, :480].contiguous(), rast[:1, :270, :480].contiguous(), ref[:1, :270, :480].contiguous()
    s, grad, _ = dr.norm_loss_call(cc, cr, cf, taps, 1.0 / cc.numel(), EPS)
    x = cc.clone().requires_grad_(True)
    tv = norm_ref.loss_plain(x, cr[..., 3], cf, taps, EPS)
    tv.backward()
    rel = float((grad - x.grad).norm() / x.grad.norm())
    print(f"commit {commit}; {B} x {H} x {W} x {C} ({px / 1e6:.1f} Mpx), {KERNEL_SIZE} taps, sigma {SIGMA}, eps {EPS}; on a 270 x 480 crop: loss "
          f"{float(s) / cc.numel():.6f} torch {float(tv):.6f}, gradient rel-L2 against torch's {rel:.2e}", flush=True)
    assert abs(float(s) / cc.numel() - float(tv)) <= 1e-4 * abs(float(tv)) and rel < 1e-4
    variants = [("fpcdr_norm_loss value", 76.0 * C + 34.0, lambda: dr.norm_loss_call(colour, rast, ref, taps, gs, EPS, want_grad=False)),
                ("fpcdr_norm_loss value+grad", 124.0 * C + 50.0, lambda: dr.norm_loss_call(colour, rast, ref, taps, gs, EPS)),
                ("fpcdr_blur_loss value", 16.0 * C + 17.0, lambda: dr.blur_loss_call(colour, rast, ref, taps, gs, want_grad=False)),
                ("fpcdr_blur_loss value+grad", 32.0 * C + 33.0, lambda: dr.blur_loss_call(colour, rast, ref, taps, gs))]
    for _, _, fn in variants:                  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    calls = 2
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
    for kind in ("value", "value+grad"):
        print(f"  fpcdr_norm_loss {kind}: {med['fpcdr_norm_loss ' + kind] / med['fpcdr_blur_loss ' + kind]:.2f} x the time of fpcdr_blur_loss {kind}",
              flush=True)


if __name__ == "__main__":
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    main(arg("--commit", "(not named)"), float(arg("--seconds", "1.0")))

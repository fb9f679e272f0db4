"""HIP-event time of fpcdr_undistort_u8 at cfg3's target size (288 images of 1080 x 1920, 597 Mpx), warmed, over at least a second of
calls; and the wall time of scene.from_take(undistort=True) beside undistort=False on the same take (disk, decode, PCIe round trip).

    python scripts/time_undistort.py              both parts
    python scripts/time_undistort.py --kernel     the kernel loop only (the run to put under rocprofv3 --kernel-trace --stats)
"""
import ctypes, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from fpc_diffrend_amd import _lib, scene

HBM_PEAK = 8.0e12        # bytes/s, MI355X spec (6.3e12 achievable with a float4 copy)
FP64_PEAK = 78.6e12      # vector double-precision FLOP/s, MI355X spec (an FMA = 2; the rule is unfused: half of it at best)


def kernel_time(seconds=1.0):
    N, H, W, Nc = 288, 1080, 1920, 9
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.uint8).cuda()
    dst = torch.empty_like(src)
    rows = [[9600.0 + 10 * c, 9590.0 + 10 * c, W / 2 + 3.7, H / 2 - 3.8, -0.35, 0.9, 1e-3, -7e-4, -2.0] for c in range(Nc)]
    table = torch.tensor(rows, dtype=torch.float64).cuda()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda: _lib.call("fpcdr_undistort_u8", P(src), P(dst), P(table), N, H, W, Nc, 140, 1, st)
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    times, t0 = [], time.perf_counter()
    while time.perf_counter() - t0 < seconds or len(times) < 10:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    med, px = times[len(times) // 2], N * H * W
    rate = 2 * px / (med * 1e-3)
    # per pixel, unfused: 17 multiplies + 22 adds / subtracts + 3 floors of the rule; not counted: its one division (the row's y is
    # shared; ~10 instructions), four u8 -> f64 conversions, the address arithmetic
    flops = 42 * px / (med * 1e-3)
    print(f"fpcdr_undistort_u8 {N} x {H} x {W} ({px / 1e6:.0f} Mpx): median {med:.3f} ms, min {times[0]:.3f}, max {times[-1]:.3f} over {len(times)} calls")
    print(f"  {px / (med * 1e-3) / 1e9:.1f} Gpx/s; algorithmic 2 B/px = {rate / 1e12:.3f} TB/s = {100 * rate / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    print(f"  42 double operations per pixel = {flops / 1e12:.2f} TFLOP/s of unfused f64 = {100 * flops / (FP64_PEAK / 2):.1f} % of the {FP64_PEAK / 2e12:.1f} TFLOP/s "
          f"the vector unit gives without FMA")


def take_time(frames=4, resolution=(1200, 1600)):
    sc = scene.make_scene(mesh=(8, 4), K=2, n_frames=frames, resolution=resolution, texshape=(8, 8, 1))
    rng = np.random.default_rng(0)
    H, W = resolution
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    base = (70 + 60 * np.sin(yy / 37.0) * np.cos(xx / 53.0))
    images = np.stack([np.stack([np.clip(base + rng.normal(0, 6, size=(H, W)), 0, 255).astype(np.uint8) for _ in range(9)]) for _ in range(frames)])
    dist = np.tile(np.array([-0.35, 0.9, 1e-3, -7e-4, -2.0]), (9, 1))
    with tempfile.TemporaryDirectory() as td:
        b, bl, cal, imdir = scene.write_take(sc, td, images, distortion=dist)
        scene.from_take(b, bl, cal, imdir, undistort=True)       # (library load, first launch)
        t = {}
        for und in (False, True, False, True):
            t0 = time.perf_counter()
            take = scene.from_take(b, bl, cal, imdir, undistort=und)
            t.setdefault(und, []).append(time.perf_counter() - t0)
    n = frames * 9
    print(f"from_take, {n} TIFFs of {H} x {W} ({n * H * W / 1e6:.0f} Mpx): undistort=False {min(t[False]):.3f} s, undistort=True {min(t[True]):.3f} s "
          f"(+{1e3 * (min(t[True]) - min(t[False])) / n:.2f} ms per image: upload, kernel, download)")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU"
    kernel_time()
    if "--kernel" not in sys.argv:
        take_time()

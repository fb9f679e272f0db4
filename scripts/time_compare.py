"""HIP-event time of fpcdr_compare_u8 on 108 images of 1600 x 1200 (12 frames x 9 cameras of the reference's take shape, 207 Mpx),
warmed, over at least a second of calls per variant: float and uint8 input, heat map + row sums and row sums only; and the wall time
of rerender.compare_result on 12 frames beside the host path on the same saved result (rerender_result + mean_abs_diff per tile).

    python scripts/time_compare.py              both parts
    python scripts/time_compare.py --kernel     the kernel loops only (the run to put under rocprofv3 --kernel-trace --stats)
"""
import ctypes, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from fpc_diffrend_amd import _lib, fit, rerender, scene

HBM_PEAK = 8.0e12        # bytes/s, MI355X spec
# what the project's other streaming kernels reach: the 16-byte copy of the antialias backward, and the undistortion
# kernel's 2 B/px, which is bound by double-precision issue and not by memory
BESIDE = "k_copy_f4_chunk 5.3 TB/s (0.66 of peak), fpcdr_undistort_u8 0.61 TB/s (issue bound)"


def kernel_time(seconds=1.0):
    N, H, W = 108, 1600, 1200
    g = torch.Generator().manual_seed(0)
    ref = torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.uint8).cuda()
    img_u8 = torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.uint8).cuda()
    img_f = (torch.rand((N, H, W), generator=g) * 1.1 - 0.05).cuda()
    heat = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda')
    rows = torch.zeros((N, H), dtype=torch.int32, device='cuda')
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    px = N * H * W
    print(f"fpcdr_compare_u8, {N} x {H} x {W} ({px / 1e6:.0f} Mpx); beside: {BESIDE}")
    for name, img, is_f, hm, bytes_px in (("float, heat + rows", img_f, 1, heat, 8), ("float, rows only", img_f, 1, None, 5),
                                          ("uint8, heat + rows", img_u8, 0, heat, 5), ("uint8, rows only", img_u8, 0, None, 2)):
        def call():
            rows.zero_()        # (the caller hands the sums in zero-filled: part of every use, 0.7 MB)
            _lib.call("fpcdr_compare_u8", P(img), is_f, 255.0, P(ref), P(hm), P(rows), N, H, W, 100, 1100, 0, 1, st)
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
        med = times[len(times) // 2]
        rate = bytes_px * px / (med * 1e-3)
        print(f"  {name:20s} median {med:.3f} ms, min {times[0]:.3f}, max {times[-1]:.3f} over {len(times)} calls; algorithmic {bytes_px} B/px = "
              f"{rate / 1e9:.0f} GB/s = {100 * rate / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")


def result_time(frames=12):
    """A saved result of the reference's run shape (30k-triangle mesh, nine cameras, 1600 x 1200) written from the scene's ground truth
    -- no fit is needed to time the evaluation -- compared with synthetic captures by both paths."""
    sc = scene.cfg('ref', n_frames=frames)
    H, W = sc.resolution
    meshes = (sc.v_base[None] + sc.weights_gt @ sc.blendshapes.T).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        fit.write_result(td, meshes, sc.uv, fit.face_lines(sc.pos_idx, sc.uv_idx), sc.texture, sc.t_gt.tolist(), sc.q_gt.tolist())
        rdir = os.path.join(td, "result")
        rng = np.random.default_rng(0)
        references = rng.integers(0, 141, size=(frames, 9, H, W), dtype=np.uint8)

        def host():
            means = np.empty((frames, 9))
            for i, grid in rerender.rerender_result(rdir, sc):
                for c in range(9):
                    tile = grid[(c // 3) * H:(c // 3 + 1) * H, (c % 3) * W:(c % 3 + 1) * W, 0]
                    means[i, c], _ = rerender.mean_abs_diff(tile, references[i, c])
            return means

        gpu = lambda heat: rerender.compare_result(rdir, sc, references, os.path.join(td, "cmp"), heat=heat)
        want = host()                      # (library load, first launches)
        got = gpu(False)
        print(f"compare_result, {frames} frames x 9 cameras of {H} x {W}: image means equal to the host path's: {bool(np.array_equal(got, want))} "
              f"(largest difference {np.abs(got - want).max():.3g})")
        t = {}
        for name, fn in (("host", host), ("gpu rows", lambda: gpu(False)), ("host", host), ("gpu rows", lambda: gpu(False)), ("gpu heat + png", lambda: gpu(True))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.setdefault(name, []).append(time.perf_counter() - t0)
    print(f"  host path (rerender_result + mean_abs_diff per tile) {min(t['host']):.3f} s; compare_result, CSV only {min(t['gpu rows']):.3f} s "
          f"({min(t['host']) / min(t['gpu rows']):.1f} x); with the {frames * 9} heat-map PNGs {min(t['gpu heat + png']):.3f} s")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU"
    kernel_time()
    if "--kernel" not in sys.argv:
        result_time()

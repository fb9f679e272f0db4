"""HIP-event time of fpcdr_overlay_u8 (k_overlay_u8) at the workload's own size -- the nine 1600 x 1200 views of one frame, and four
frames of nine -- in its three modes, beside the yardstick k_compare_u8 (float input, colour map, no row sums: the same 8 B/px streaming
shape) timed in the same run, alternating with it:

    plain     no raster inputs                          4 (float render) + 1 (capture) + 3 (out)      =  8 B/px
    capture   outside='capture', no wire                 + 16 (rast)                                  = 24 B/px
    wire      outside='capture', wire at half width 0.5  + 16 (rast_db) for the covered pixels         = 24 + 16 * coverage B/px

rast and rast_db are the rasteriser's own output for scene.cfg('ref') (30k triangles, nine cameras), the render is random noise (its
values do not change what is read or written).  Every variant is warmed, then the variants take turns, CALLS calls between two events a
turn, until each has at least a second of timed calls.  Per variant: the median turn, and time per algorithmic byte; the condition of the
change that added the kernel is that each mode's time per byte is no worse than the yardstick's plus the spread (max - min over its turns)
the yardstick itself shows in this run.

    python scripts/time_overlay.py              the table
    python scripts/time_overlay.py --kernel     a few calls of every variant only (the run to put under rocprofv3 --kernel-trace --stats)
"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from fpc_diffrend_amd import _lib, camera, rerender, scene
from fpc_diffrend_amd import ops as dr

HBM_PEAK = 8.0e12        # bytes/s, MI355X spec
CALLS = 10


def raster_of(frames):
    """(rast, rast_db) [frames * 9, 1600, 1200, 4] of the reference-shaped scene's ground-truth meshes, as overlay_result forms them."""
    sc = scene.cfg('ref', n_frames=frames)
    dev = torch.device('cuda')
    meshes = (sc.v_base[None] + sc.weights_gt @ sc.blendshapes.T).astype(np.float32).reshape(frames, -1, 3)
    proj, t_mv = rerender._camera_matrices(sc.cams, (0.0, 170.0, 0.0), dev)
    clip = [camera.transform_clip(rerender._multicam_mvp(proj, t_mv, (sc.t_gt[i], sc.q_gt[i])), torch.tensor(meshes[i], device=dev)[None])
            for i in range(frames)]
    tri = torch.tensor(sc.pos_idx, dtype=torch.int32, device=dev)
    rast, rast_db = dr.rasterize(dr.RasterizeGLContext(device=dev), torch.cat(clip), tri, resolution=(sc.resolution[0], sc.resolution[1]))
    return rast.contiguous(), rast_db.contiguous()


def run(frames, seconds, kernel_only):
    rast, rast_db = raster_of(frames)
    N, H, W, _ = rast.shape
    px = N * H * W
    coverage = float((rast[..., 3] > 0).float().mean())
    g = torch.Generator().manual_seed(0)
    ref = torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.uint8).cuda()
    img = (torch.rand((N, H, W), generator=g) * 1.1 - 0.05).cuda()
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device='cuda')
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    hw2 = float(np.float32(0.5) * np.float32(0.5))

    def overlay(r, d, outside, h):
        return lambda: _lib.call("fpcdr_overlay_u8", P(img), 1, 255.0, P(ref), P(r), P(d), P(out), N, H, W, 128, outside, h, 0x00ff00, 1, st)

    variants = [("k_compare_u8 (yardstick)", 8.0,
                 lambda: _lib.call("fpcdr_compare_u8", P(img), 1, 255.0, P(ref), P(out), None, N, H, W, 100, 1100, 0, 1, st)),
                ("k_overlay_u8 plain", 8.0, overlay(None, None, 0, 0.0)),
                ("k_overlay_u8 capture", 24.0, overlay(rast, None, 1, 0.0)),
                ("k_overlay_u8 wire", 24.0 + 16.0 * coverage, overlay(rast, rast_db, 1, hw2))]
    for _, _, fn in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    wire_share = float(((out[..., 0] == 0) & (out[..., 1] == 255) & (out[..., 2] == 0)).float().mean())
    print(f"{N} images of {H} x {W} ({px / 1e6:.1f} Mpx), coverage {coverage:.4f}, wire pixels {wire_share:.4f} of all; {CALLS} calls a turn")
    if kernel_only:
        return
    turns = {name: [] for name, _, _ in variants}
    t0 = time.perf_counter()
    while min(sum(v) for v in turns.values()) < seconds * 1e3 or len(turns[variants[0][0]]) < 10:
        for name, _, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            turns[name].append(e0.elapsed_time(e1))
        if time.perf_counter() - t0 > 120:
            break
    yard = None
    for name, bpp, _ in variants:
        per_call = np.sort(np.asarray(turns[name])) / CALLS                      # ms
        ps_per_byte = per_call * 1e9 / (bpp * px)                                  # picoseconds per algorithmic byte
        med, lo, hi = float(np.median(ps_per_byte)), float(ps_per_byte[0]), float(ps_per_byte[-1])
        rate = bpp * px / (float(np.median(per_call)) * 1e-3)
        line = (f"  {name:26s} {bpp:5.2f} B/px  median {np.median(per_call):.4f} ms (min {per_call[0]:.4f}, max {per_call[-1]:.4f}, "
                f"{per_call.size} turns)  {med:.4f} ps/B (min {lo:.4f}, max {hi:.4f})  {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of peak")
        if yard is None:
            yard = (med, hi - lo)
            line += f"  spread {hi - lo:.4f} ps/B"
        else:
            line += f"  bar {yard[0] + yard[1]:.4f} ps/B: {'met' if med <= yard[0] + yard[1] else 'MISSED'}"
        print(line)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the GPU"
    kernel_only = "--kernel" in sys.argv
    for frames in (1, 4):
        run(frames, 1.0, kernel_only)

"""Bit-identity of the two windowed pixel losses (fpcdr_blur_loss, fpcdr_norm_loss) between two builds of libfpcdr.so.

    FPCDR_LIB_PATH=/path/to/libfpcdr.so python scripts/window_loss_planes.py OUT.pt        one fresh process per library
    python scripts/window_loss_planes.py --compare A.pt B.pt [--sum-rel R]

The first form runs both losses with the gradient at every shape the GPU tests use (blur_ref.SHAPES, the EXTENT_SHAPES of
tests/test_gpu_blur.py and tests/norm_ref.py, norm_ref.FLAT_SHAPE) and saves every float plane the kernels write -- E and grad of the
blurred loss; stats, d, pq, p and grad of the normalised one -- and the two f64 sums.  The second form holds every plane of B to
torch.equal with A's, and prints the largest relative difference of the sums (they move in their last bits with the order of the
atomics, so they are held to --sum-rel, the spread two runs of ONE library show, where that is given).  Exit status 1 on a difference."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import blur_ref
    import norm_ref
    import test_gpu_blur
    from fpc_diffrend_amd import _lib, ops as dr
    assert torch.cuda.is_available(), "needs the GPU"
    shapes = list(dict.fromkeys(blur_ref.SHAPES + test_gpu_blur.EXTENT_SHAPES + norm_ref.EXTENT_SHAPES + [norm_ref.FLAT_SHAPE]))
    res = {}
    for shape in shapes:
        Bn, H, W, C, k, sigma = shape
        colour, cover, ref = norm_ref.flat_inputs() if shape == norm_ref.FLAT_SHAPE else blur_ref.inputs(Bn, H, W, C)
        rast = torch.zeros(colour.shape[:3] + (4,), device='cuda')
        rast[..., 3] = cover.cuda()
        colour, ref, taps = colour.cuda(), ref.cuda(), blur_ref.taps(k, sigma)
        gs = 1.0 / colour.numel()
        s_blur, g_blur, E = dr.blur_loss_call(colour, rast, ref, taps, gs)
        s_norm, g_norm, planes = dr.norm_loss_call(colour, rast, ref, taps, gs, norm_ref.EPS)
        torch.cuda.synchronize()
        res[shape] = {'E': E.cpu(), 'grad_blur': g_blur.cpu(), 'sum_blur': s_blur.cpu(), 'grad_norm': g_norm.cpu(), 'sum_norm': s_norm.cpu(),
                      **{name: plane.cpu() for name, plane in planes.items()}}
    torch.save(res, out)
    print(f"{_lib.LIB_PATH}: {len(res)} shapes -> {out}")


def compare(a_path, b_path, sum_rel):
    import torch
    a, b = torch.load(a_path), torch.load(b_path)
    assert list(a) == list(b), "the two files hold different shapes"
    bad, worst, planes = [], 0.0, 0
    for shape in a:
        for name, x in a[shape].items():
            y = b[shape][name]
            if name.startswith('sum_'):
                worst = max(worst, abs(float(x) - float(y)) / abs(float(x)))
            else:
                planes += 1
                if not torch.equal(x, y):
                    bad.append((shape, name, int((x != y).sum())))
    print(f"{a_path} vs {b_path}: {len(a)} shapes, {planes} planes, {len(bad)} differ; f64 sums: largest relative difference {worst:.3e}"
          + (f" (allowed {sum_rel:.3e})" if sum_rel is not None else ""))
    for item in bad:
        print("  DIFFERENT", *item)
    return 1 if bad or (sum_rel is not None and worst > sum_rel) else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], float(sys.argv[sys.argv.index("--sum-rel") + 1]) if "--sum-rel" in sys.argv else None))
    run(sys.argv[1])

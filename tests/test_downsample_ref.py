"""CPU: the numpy statement of the Downsample rule (tests/downsample_ref.py) is itself checked -- against the float64 mean, on saturated
input and on exact ties, and against a cascade, which it must NOT equal -- so that the bit-exact comparison of the kernel against it
(tests/test_gpu_downsample.py) means something.  Plus the binding, the kernel's resource claims, and the claim the pyramid rests on: a
render at (H / s, W / s) with the same matrices is aligned with the s x s box reduction."""
import os
import re

import numpy as np
import pytest
import torch

import downsample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = tuple(range(2, 17))


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", FACTORS)
def test_rule_is_the_mean_rounded_half_up(s):
    """(2 S + s^2) // (2 s^2) == floor(S / s^2 + 0.5) in float64 (S / s^2 is at least 1 / (2 s^2) >= 2^-9 away from a tie unless it is
    one exactly, and an exact tie k + 1/2 is a float64), on random images, on the all-255 image and on every attainable sum."""
    rng = np.random.default_rng(100 + s)
    img = rng.integers(0, 256, size=(3, 5 * s, 7 * s), dtype=np.uint8)
    got = R.downsample(img, s)
    mean = img.reshape(3, 5, s, 7, s).astype(np.float64).mean(axis=(2, 4))
    assert got.shape == (3, 5, 7) and got.dtype == np.uint8
    assert np.array_equal(got, np.floor(mean + 0.5).astype(np.uint8))
    full = np.full((2 * s, 3 * s), 255, dtype=np.uint8)
    assert np.array_equal(R.downsample(full, s), np.full((2, 3), 255, dtype=np.uint8))
    assert int(R.block_sums(full, s).max()) == 255 * s * s <= 65280
    S = np.arange(255 * s * s + 1, dtype=np.int64)                     # every sum a block can have
    assert np.array_equal((2 * S + s * s) // (2 * s * s), np.floor(S / float(s * s) + 0.5).astype(np.int64))


@pytest.mark.parametrize("s", [s for s in FACTORS if s % 2 == 0])
def test_ties_round_up(s):
    img, want = R.tie_image(s)
    S = R.block_sums(img, s)
    assert np.all((2 * S + s * s) % (2 * s * s) == 0)
    assert np.array_equal(R.downsample(img, s), want)
    if s == 2:
        assert np.array_equal(img[:2, :2], np.array([[1, 0], [0, 1]], dtype=np.uint8)) and want[0, 0] == 1


def test_a_cascade_is_another_function():
    """2 then 2 is not 4: the inner rounding moves a mean across the outer one's threshold.  A 4 x 4 block whose 2 x 2 quarters have the
    sums 2, 2, 2, 1: the cascade rounds the quarters to 1, 1, 1, 0 (1/2 goes up, 1/4 down), whose mean 3/4 rounds to 1; the direct mean
    7/16 rounds to 0.  The levels of a pyramid are therefore all made from the full-size image."""
    blk = np.zeros((4, 4), dtype=np.uint8)
    blk[0, 0] = blk[1, 1] = 1          # top-left 2 x 2: sum 2
    blk[0, 2] = blk[1, 3] = 1          # top-right: sum 2
    blk[2, 0] = blk[3, 1] = 1          # bottom-left: sum 2
    blk[2, 2] = 1                      # bottom-right: sum 1
    direct = R.downsample(blk, 4)
    cascade = R.downsample(R.downsample(blk, 2), 2)
    assert direct.shape == cascade.shape == (1, 1)
    assert int(direct[0, 0]) == 0 and int(cascade[0, 0]) == 1
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, size=(64, 64), dtype=np.uint8)
    differ = int((R.downsample(img, 4) != R.downsample(R.downsample(img, 2), 2)).sum())
    print(f"random 64 x 64 image: direct 4 and cascade 2, 2 differ at {differ} of 256 pixels")
    assert differ > 0


# ---- 2. the binding ------------------------------------------------------------------------------------------------------------------------
NAME = "fpcdr_downsample_u8"


def test_binding():
    """The entry is declared in the header, bound in _lib.SYMBOLS and exported by the built library; a pure addition: the ABI version
    stays what it was."""
    from fpc_diffrend_amd import _lib
    header = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    lib = _lib.load()
    assert re.search(r"\bint " + NAME + r"\(", header)
    assert NAME in _lib.SYMBOLS and hasattr(lib, NAME)
    assert _lib.ABI_VERSION == lib.fpcdr_abi_version() == 16
    assert int(re.search(r"#define FPCDR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """The entry checks its arguments on the host, so the rejections need no GPU (made-up addresses, never dereferenced); no image at all
    is success, again without a launch."""
    from fpc_diffrend_amd import _lib
    src, dst = 0x100000, 0x900000
    for args, why in (((src, dst, 2, 8, 8, 1), "factor"), ((src, dst, 2, 8, 8, 17), "factor"), ((src, dst, 2, 8, 8, 0), "factor"),
                      ((src, dst, 2, 8, 8, -2), "factor"), ((src, dst, 2, 9, 8, 2), "multiples"), ((src, dst, 2, 8, 10, 4), "multiples"),
                      ((src, dst, 2, 0, 8, 2), "positive"), ((src, dst, 2, 8, -8, 2), "positive"), ((src, dst, -1, 8, 8, 2), "negative"),
                      ((None, dst, 2, 8, 8, 2), "null"), ((src, None, 2, 8, 8, 2), "null"),
                      ((src, src, 2, 8, 8, 2), "overlaps"), ((src, src + 127, 2, 8, 8, 2), "overlaps"), ((src + 31, src, 2, 8, 8, 2), "overlaps")):
        with pytest.raises(RuntimeError, match=NAME + ".*" + why):
            _lib.call(NAME, *args, None)
    _lib.call(NAME, None, None, 0, 8, 8, 2, None)                              # n_images == 0: success, nothing launched
    with pytest.raises(RuntimeError, match=NAME + ".*factor"):
        _lib.call(NAME, None, None, 0, 8, 8, 1, None)


def test_downsample_has_no_cpu_path():
    from fpc_diffrend_amd import ops
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.downsample_images(torch.zeros(2, 8, 8, dtype=torch.uint8), 2)
    with pytest.raises(TypeError):
        ops.downsample_images(np.zeros((2, 8, 8), dtype=np.uint8), 2)


def test_downsample_kernels_have_no_private_segment():
    """a kernel with a private segment is dispatched several times slower.  Every instance of k_downsample_u8 (one per
    factor) keeps everything in registers and uses no LDS; read from the built object (tests/codeobj.py)."""
    import codeobj
    recs = codeobj.kernels("downsample.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = set()
    for name, private, lds in recs:
        if "k_downsample_u8" in name:
            seen.add(name)
            assert private == 0, name
            assert lds == 0, name
    assert len(seen) == len(FACTORS), seen


# ---- 3. what the pyramid rests on ----------------------------------------------------------------------------------------------------------
def test_a_reduced_render_is_aligned_with_the_box_reduction(oracle_ops):
    """The projection chain is pure NDC, so the SAME clip positions rasterised at (H / s, W / s) cover the pixels whose s x s blocks the
    full-size raster covers: make_scene(resolution=(128, 128), n_frames=2), cameras 0, 4 and 8, the true geometry.  Per image, the
    centroid of the covered pixel centres at factor s, in full-size units (j + 0.5) * s, lies within s / 4 full-size pixels of the
    full-size centroid on each axis for s = 2, 4, 8 (a resampling that is half a coarse pixel off would show s / 2).  Measured: the
    largest distance over the six images and both axes is 0.18, 0.39, 1.75."""
    from fpc_diffrend_amd import scene
    from oracle import fit as ofit
    sc = scene.make_scene(resolution=(128, 128), n_frames=2)
    gt = ofit.State(sc, cams=[0, 4, 8])
    with torch.no_grad():
        gt.M1.copy_(torch.eye(2))
        gt.M2.copy_(torch.tensor(sc.weights_gt).t())
        gt.per_frame_t.copy_(torch.tensor(sc.t_gt))
        gt.per_frame_q.copy_(torch.tensor(sc.q_gt))
        pos_clip, _ = ofit.clip_positions(gt, torch.arange(2))

        def centroids(s):
            rast, _ = oracle_ops.rasterize(pos_clip, gt.pos_idx, (128 // s, 128 // s))
            cov = (rast[..., 3] > 0).numpy()
            out = []
            for b in range(cov.shape[0]):
                i, j = np.nonzero(cov[b])
                assert i.size > 0
                out.append(((i.mean() + 0.5) * s, (j.mean() + 0.5) * s))
            return np.array(out)

        full = centroids(1)
        for s in (2, 4, 8):
            d = float(np.abs(centroids(s) - full).max())
            print(f"factor {s}: largest centroid distance {d:.3f} full-size pixels (bound {s / 4})")
            assert d <= s / 4

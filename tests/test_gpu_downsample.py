"""GPU: fpcdr_downsample_u8 / ops.downsample_images against the numpy statement of the Downsample rule (tests/downsample_ref.py, itself
checked in tests/test_downsample_ref.py) -- torch.equal: integers throughout, no tolerance, no excluded pixel."""
import ctypes

import numpy as np
import pytest
import torch

import downsample_ref as R

pytestmark = pytest.mark.gpu
NAME = "fpcdr_downsample_u8"
GUARD = 48      # bytes in front of and behind the output that must stay as they were
FILL = 0xA5


def _mismatch(out, ref):
    d = np.asarray(out) != np.asarray(ref)
    return f"{int(d.sum())} of {d.size} pixels differ, first at {tuple(np.argwhere(d)[0]) if d.any() else None}"


def _call(src_np, s, src_shift=0, dst_shift=0):
    """One call of the C entry on src_np [N,H,W] with the source `src_shift` and the output `dst_shift` bytes off a 256-byte aligned
    address; the output sits between guard bytes, which are checked.  Returns the output as numpy [N,H/s,W/s]."""
    from fpc_diffrend_amd import _lib
    N, H, W = src_np.shape
    Ho, Wo = H // s, W // s
    src_buf = torch.zeros(src_np.size + src_shift, dtype=torch.uint8, device='cuda')
    src = src_buf[src_shift:]
    src.copy_(torch.from_numpy(src_np.reshape(-1)))
    dst_buf = torch.full((GUARD + dst_shift + N * Ho * Wo + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    dst = dst_buf[GUARD + dst_shift: GUARD + dst_shift + N * Ho * Wo]
    assert src_buf.data_ptr() % 256 == 0 and dst_buf.data_ptr() % 256 == 0
    assert src.data_ptr() % 16 == src_shift % 16 and dst.data_ptr() % 16 == (GUARD + dst_shift) % 16
    with torch.cuda.device(src.device):
        _lib.call(NAME, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), N, H, W, s,
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    out = dst_buf.cpu().numpy()
    assert np.all(out[:GUARD + dst_shift] == FILL) and np.all(out[GUARD + dst_shift + N * Ho * Wo:] == FILL), "wrote outside the output"
    assert np.array_equal(src.cpu().numpy(), src_np.reshape(-1)), "the source changed"
    return out[GUARD + dst_shift: GUARD + dst_shift + N * Ho * Wo].reshape(N, Ho, Wo)


def _random(N, H, W, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    img[0, : H // 2] = 255          # saturated blocks and, below, dark ones
    img[-1, H // 2:, : W // 2] = 0
    return img


FACTORS = (2, 3, 4, 5, 8, 16)


@pytest.mark.parametrize("Ho", [1, 70])
@pytest.mark.parametrize("Wo", [1, 15, 16, 17, 33, 80])
@pytest.mark.parametrize("s", FACTORS)
def test_rule(s, Wo, Ho):
    """Three images.  Output widths 1, 15, 16, 17, 33: a row that is one tail, one whole 16-pixel chunk, and whole chunks with tails of 1;
    80 with 70 rows is 350 chunks, two workgroups.  Output at an aligned base (GUARD is a multiple of 16), so whole chunks of rows whose
    own offset allows it leave as 16-byte stores; the source rows start at (n H + r) W mod 16, every residue for the odd factors."""
    src = _random(3, Ho * s, Wo * s, seed=1000 * s + 10 * Wo + Ho)
    want = R.downsample(src, s)
    got = _call(src, s)
    assert np.array_equal(got, want), f"s {s}, {src.shape} -> {want.shape}: " + _mismatch(got, want)


@pytest.mark.parametrize("s", FACTORS)
def test_rows_at_every_alignment(s):
    """Source width s * 33 with 2 x 16 s rows: for an odd factor the source rows start at every residue mod 16, for the others at every
    residue the width allows; output width 33, so output rows start at every residue too.  Both forms of the load and of the store are
    taken inside one call."""
    Wo, Ho = 33, 32
    src = _random(2, Ho * s, Wo * s, seed=77 + s)
    rows = {(r * Wo * s) % 16 for r in range(2 * Ho * s)}
    if s % 2:
        assert rows == set(range(16))
    assert 0 in rows and {(r * Wo) % 16 for r in range(2 * Ho)} == set(range(16))
    want = R.downsample(src, s)
    got = _call(src, s)
    assert np.array_equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("src_shift,dst_shift", [(1, 0), (0, 1), (1, 1), (15, 7)])
@pytest.mark.parametrize("s", FACTORS)
def test_buffers_at_odd_addresses(s, src_shift, dst_shift):
    """Every buffer at a base offset by one byte (and by 15 / 7): rows of 32 s source bytes and 32 output pixels keep the offset of the
    base, so no access of the shifted buffer can take the 16-byte form, and the bytes around the output stay as they were."""
    src = _random(2, 3 * s, 32 * s, seed=5 + s)
    want = R.downsample(src, s)
    got = _call(src, s, src_shift, dst_shift)
    assert np.array_equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("s", FACTORS)
def test_saturated_and_ties(s):
    """All 255 -> 255 (the largest sum, 255 s^2); for the even factors the image whose blocks have means k + 1/2 -> k + 1."""
    full = np.full((2, 2 * s, 48 * s), 255, dtype=np.uint8)
    got = _call(full, s)
    assert np.array_equal(got, np.full((2, 2, 48), 255, dtype=np.uint8)), _mismatch(got, 255)
    if s % 2 == 0:
        img, want = R.tie_image(s, rows=2, cols=3)
        got = _call(img[None], s)[0]
        assert np.array_equal(want, R.downsample(img, s))
        assert np.array_equal(got, want), _mismatch(got, want)


def test_more_images_than_one_launch_holds():
    """65 537 images of 2 x 2 at s = 2: the image is the grid's y, at most 65 535 a launch; the last two go in a second one."""
    import fpc_diffrend_amd.ops as dr
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, size=(65537, 2, 2), dtype=np.uint8)
    out = dr.downsample_images(torch.from_numpy(src).cuda(), 2)
    want = R.downsample(src, 2)
    assert out.shape == (65537, 1, 1) and out.dtype == torch.uint8
    assert torch.equal(out.cpu(), torch.from_numpy(want)), _mismatch(out.cpu().numpy(), want)


def test_bad_arguments_are_rejected_without_a_launch():
    """s of 1 and 17, a size that does not divide, overlapping buffers: an error code with a text, and the prefilled output is unchanged."""
    from fpc_diffrend_amd import _lib
    src = torch.randint(0, 256, (2, 16, 32), dtype=torch.uint8, device='cuda')
    dst = torch.full((2 * 16 * 32,), FILL, dtype=torch.uint8, device='cuda')
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    keep = src.clone()
    with torch.cuda.device(src.device):
        for args, why in (((p(src), p(dst), 2, 16, 32, 1), "factor"), ((p(src), p(dst), 2, 16, 32, 17), "factor"),
                          ((p(src), p(dst), 2, 16, 32, 3), "multiples"), ((p(src), p(dst), 2, 15, 32, 5), "multiples"),
                          ((p(src), p(src), 2, 16, 32, 2), "overlaps"), ((p(src), p(src, 1023), 2, 16, 32, 2), "overlaps"),
                          ((p(dst, 100), p(dst), 1, 16, 32, 2), "overlaps")):
            with pytest.raises(RuntimeError, match=NAME + ".*" + why):
                _lib.call(NAME, *args, st)
        _lib.call(NAME, p(src), p(dst), 0, 16, 32, 2, st)       # no image: success, nothing written
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()) and torch.equal(src, keep)


def test_ops_on_a_4d_tensor():
    """[F, Nc, H, W] -> [F, Nc, H / s, W / s]; a non-contiguous view is made contiguous; the input stays as it was."""
    import fpc_diffrend_amd.ops as dr
    src = _random(6, 24, 40, seed=3).reshape(2, 3, 24, 40)
    t = torch.from_numpy(src).cuda()
    for s in (2, 4, 8):
        out = dr.downsample_images(t, s)
        assert out.shape == (2, 3, 24 // s, 40 // s) and out.dtype == torch.uint8 and out.is_contiguous()
        assert torch.equal(out.cpu(), torch.from_numpy(R.downsample(src, s))), s
    view = t[:, :, :, ::2]                                           # [2,3,24,20], strided
    assert not view.is_contiguous()
    assert torch.equal(dr.downsample_images(view, 4).cpu(), torch.from_numpy(R.downsample(np.ascontiguousarray(src[..., ::2]), 4)))
    plain = dr.downsample_images(t[0, 0], 2)                         # [H,W]
    assert plain.shape == (12, 20) and torch.equal(plain.cpu(), torch.from_numpy(R.downsample(src[0, 0], 2)))
    assert torch.equal(t.cpu(), torch.from_numpy(src))


def test_ops_errors():
    import fpc_diffrend_amd.ops as dr
    t = torch.zeros(2, 16, 32, dtype=torch.uint8, device='cuda')
    for factor in (1, 17, 0, -2):
        with pytest.raises(ValueError, match="2..16"):
            dr.downsample_images(t, factor)
    with pytest.raises(ValueError, match="integer"):
        dr.downsample_images(t, 2.0)
    with pytest.raises(ValueError, match="does not divide"):
        dr.downsample_images(t, 3)
    with pytest.raises(ValueError, match="dtype"):
        dr.downsample_images(t.float(), 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        dr.downsample_images(t.cpu(), 2)
    with pytest.raises(ValueError):
        dr.downsample_images(torch.zeros(16, dtype=torch.uint8, device='cuda'), 2)

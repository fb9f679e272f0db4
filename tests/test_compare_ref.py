"""CPU: the numpy statement of the comparison rule (tests/compare_ref.py) is itself checked -- against the reference's expressions
(comparisons.py:40-48) spelled out per pixel, the rounding cases the rule names, and rerender.mean_abs_diff -- so that the bit-exact
comparison of the kernel against it (tests/test_gpu_compare.py) means something.  Plus the host-side surface that needs no GPU."""
import os

import numpy as np
import pytest

import compare_ref as R
from helpers import comparison_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_zero_difference_is_white():
    for mode in ('colour', 'grey'):
        assert np.array_equal(R.heat_map(np.zeros((2, 3), dtype=np.int32), mode), np.full((2, 3, 3), 255, dtype=np.uint8))


def test_heat_map_over_every_difference():
    """All 511 differences: red channel 255 for d >= 0 and blue 255 for d < 0 in colour mode, s = 255 - 2 |d| up to |d| = 127 and 0
    above, three equal channels in grey mode; and, where the reference's own expressions stay inside uint8 (|d| <= 127), its values."""
    d = np.arange(-255, 256, dtype=np.int32)
    col, grey = R.heat_map(d, 'colour'), R.heat_map(d, 'grey')
    assert col.dtype == grey.dtype == np.uint8 and col.shape == grey.shape == (511, 3)
    s = np.where(np.abs(d) <= 127, 255 - 2 * np.abs(d), 0)
    assert s.min() == 0 and s[np.abs(d) == 127].tolist() == [1, 1] and s[np.abs(d) == 128].tolist() == [0, 0]
    assert np.all(col[d >= 0, 0] == 255) and np.all(col[d < 0, 2] == 255)
    assert np.array_equal(col[:, 1], s)
    assert np.array_equal(col[d >= 0, 2], s[d >= 0]) and np.array_equal(col[d < 0, 0], s[d < 0])
    assert all(np.array_equal(grey[:, c], s) for c in range(3))
    for k, diff in enumerate(d.tolist()):
        if abs(diff) > 127:
            continue
        want = [255, 255 - diff * 2, 255 - diff * 2] if diff >= 0 else [255 + diff * 2, 255 + diff * 2, 255]      # comparisons.py:41-45
        assert col[k].tolist() == want
        assert grey[k].tolist() == [255 - abs(diff) * 2] * 3                                                       # comparisons.py:47-48


def test_float_quantisation_ties_and_specials():
    f = lambda *v: R.quantise(np.array(v, dtype=np.float32), scale=1.0).tolist()
    assert f(0.5, 1.5, 2.5, 254.5, -0.5, 255.5) == [0, 2, 2, 254, 0, 255]                 # round half to EVEN, then the clip
    assert f(np.inf, -np.inf, np.nan, -np.nan) == [255, 0, 0, 0]
    assert f(1e9, -1e9, 256.0, -1.0, 0.0, -0.0, 255.0, 127.49999, 127.50001) == [255, 0, 255, 0, 0, 0, 255, 127, 128]
    # the multiply is ONE float32 multiply, rounded to float32 before the rint: the host path's expression on the same values
    v = np.linspace(0, 1, 4097, dtype=np.float32)
    assert np.array_equal(R.quantise(v, 255.0), np.clip(np.rint(v * np.float32(255.0)), 0, 255).astype(np.uint8))       # rerender_result's
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.quantise(u), u) and np.array_equal(R.quantise(u.astype(np.float32), 1.0), u)


def test_flip_applies_to_the_image_only():
    img, ref = R.u8_pair(2, 5, 7, seed=1)
    d = R.difference(img, ref, flip_rows=True)
    assert np.array_equal(d, img[:, ::-1].astype(np.int32) - ref.astype(np.int32))
    assert np.array_equal(R.difference(img, ref), img.astype(np.int32) - ref.astype(np.int32))


@pytest.mark.parametrize("i", [0, 57, 119])
def test_row_sums_over_the_crop_are_mean_abs_diff(i):
    """Integer row sums / crop width == the row means of rerender.mean_abs_diff (np.mean of an int32 row), exactly, and the image mean
    from them likewise: what the GPU path's CSV text rests on."""
    from fpc_diffrend_amd import rerender
    img, ref = comparison_pair(i)
    _, sums = R.compare(img[None], ref[None], cols=(100, 1100))
    assert sums.dtype == np.int32 and sums.shape == (1, 1600)
    m, rows = rerender.mean_abs_diff(img, ref)
    got = sums[0, 200:1401].astype(np.float64) / 1000
    assert got.shape == rows.shape == (1201,) and np.all(got == rows)
    assert float(got.mean()) == m
    assert np.abs(img.astype(np.int32) - ref.astype(np.int32)).max() <= 16
    m2, rows2 = rerender._means_of_row_sums(sums[0], rerender._crop(1600, 1200, (200, 1401), (100, 1100)))
    assert m2 == m and np.all(rows2 == rows)


def test_row_sums_on_a_crop_clipped_by_a_small_image():
    from fpc_diffrend_amd import rerender
    img, ref = R.u8_pair(1, 37, 53, seed=2)
    for rows, cols in (((200, 1401), (100, 1100)), ((5, 1401), (20, 1100)), ((-3, 30), (-7, 40)), ((0, 37), (0, 53))):
        _, sums = R.compare(img, ref, cols=cols)
        r0, r1, c0, c1 = max(rows[0], 0), min(rows[1], 37), max(cols[0], 0), min(cols[1], 53)
        if r0 >= r1 or c0 >= c1:
            assert not sums.any() if c0 >= c1 else True
            with pytest.raises(ValueError):
                rerender._crop(37, 53, rows, cols)
            continue
        m, row_means = rerender.mean_abs_diff(img[0], ref[0], rows=rows, cols=cols)
        got = sums[0, r0:r1].astype(np.float64) / (c1 - c0)
        assert np.all(got == row_means) and float(got.mean()) == m
        m2, rows2 = rerender._means_of_row_sums(sums[0], rerender._crop(37, 53, rows, cols))
        assert m2 == m and np.all(rows2 == row_means)
    assert not R.row_sums(R.difference(img, ref), cols=(53, 60)).any()          # empty crop: all sums 0


def test_test_inputs_hold_what_the_gpu_tests_need():
    img, ref = R.u8_pair(3, 5, 37, seed=3)
    d = R.difference(img, ref)
    assert (np.abs(d) > 127).any() and (d == 0).any() and (d > 0).any() and (d < 0).any()
    fimg, fref = R.float_pair(3, 9, 48, seed=4)
    assert np.isnan(fimg).any() and np.isposinf(fimg).any() and np.isneginf(fimg).any() and (fimg < 0).any() and (fimg > 255).any()
    finite = fimg[np.isfinite(fimg)]
    assert (np.abs(finite - np.floor(finite) - 0.5) == 0).sum() >= 9          # exact ties


def test_comparison_has_no_cpu_path(tmp_path):
    import torch
    from fpc_diffrend_amd import ops, rerender
    a = np.zeros((4, 4), dtype=np.uint8)
    with pytest.raises(RuntimeError):
        rerender.compare_sequence([a], [a], str(tmp_path), device='cpu')
    with pytest.raises(ValueError):
        ops.compare_images(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.compare_images(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), mode=None, want_rows=False)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """fpcdr_compare_u8 checks its arguments on the host, so the rejections need no GPU (made-up addresses, never dereferenced)."""
    from fpc_diffrend_amd import _lib
    img, ref, out, sums = 0x10000, 0x20000, 0x30000, 0x40000
    for args, why in (((img, 0, 1.0, ref, None, None, 2, 8, 12, 0, 12, 0, 0), "both null"),
                      ((None, 1, 1.0, ref, out, sums, 2, 8, 12, 0, 12, 0, 0), "null pointer"),
                      ((img, 0, 1.0, ref, out, sums, 2, 8, 12, 0, 12, 2, 0), "mode"),
                      ((img, 0, 1.0, ref, out, sums, 2, 8, 0, 0, 12, 0, 0), "sizes"),
                      ((img, 1, 1.0, ref, img + 2 * 8 * 12 * 4 - 1, sums, 2, 8, 12, 0, 12, 0, 0), "heat overlaps"),      # the float image's last byte
                      ((img, 0, 1.0, ref, ref - 2 * 8 * 12 * 3 + 1, sums, 2, 8, 12, 0, 12, 0, 0), "heat overlaps"),      # the heat map's last byte
                      ((img, 0, 1.0, ref, out, out + 2 * 8 * 12 * 3 - 1, 2, 8, 12, 0, 12, 0, 0), "row_sums overlaps"),
                      ((img, 0, 1.0, ref, None, sums, 1, 1, 8421505, 0, 12, 0, 0), "int32")):
        with pytest.raises(RuntimeError, match="fpcdr_compare_u8.*" + why):
            _lib.call("fpcdr_compare_u8", *args, None)


def test_compare_kernels_have_no_private_segment():
    """a kernel with a private segment is dispatched several times slower.  The four instantiations of k_compare_u8 keep
    their 16 pixels and 48 heat-map bytes in packed registers; read from the built object (tests/codeobj.py).  The LDS is the 256-row table of the row sums."""
    import codeobj
    recs = codeobj.kernels("compare.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = 0
    for name, private, lds in recs:
        if "k_compare_u8" in name:
            seen += 1
            assert private == 0, name
            assert lds == 1024, name
    assert seen == 4

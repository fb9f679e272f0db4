"""CPU: the float64 reference of the undistortion rule (tests/undistort_ref.py) is itself checked -- against an independent bilinear
implementation, an affine image, and the direction and size of the map -- so that pinning the kernel to it bit for bit
(tests/test_gpu_undistort.py) means something.  Plus the host-side surface that needs no GPU."""
import os

import numpy as np
import pytest

import undistort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_RIG, W_RIG = 1200, 1600


@pytest.mark.parametrize("intr", [R.K_LONG, R.K_WIDE, R.intrinsics_for(37, 53)], ids=["long", "wide", "odd"])
def test_zero_coefficients_return_the_input(intr):
    for (H, W) in ((37, 53), (5, 1), (240, 320)):
        img = R.noise_image(H, W, 5)
        for flip in (False, True):
            out = R.undistort_image(img, intr, R.DIST['zero'], flip_rows=flip)
            assert np.array_equal(out, img[::-1] if flip else img)
    assert np.array_equal(R.undistort_image(img, intr, R.DIST['zero'], clip_max=140), np.minimum(img, 140))


@pytest.mark.parametrize("dset", ["mild", "strong"])
def test_reference_equals_scipy_bilinear_on_the_interior(dset):
    """scipy.ndimage.map_coordinates(order=1) is an independent bilinear implementation: same bytes wherever all four taps are inside."""
    ndimage = pytest.importorskip("scipy.ndimage")
    img = R.noise_image(H_RIG, W_RIG, 1 if dset == "mild" else 2)
    val, inside = R.undistort_values(img, R.K_LONG, R.DIST[dset])
    u, v = R.source_coordinates(H_RIG, W_RIG, R.K_LONG, R.DIST[dset])
    sp = ndimage.map_coordinates(img.astype(np.float64), [v[inside], u[inside]], order=1)
    out = R.undistort_image(img, R.K_LONG, R.DIST[dset])
    print(f"{dset}: interior {inside.mean():.3f} of the image, max |val - scipy| = {np.abs(val[inside] - sp).max():.2e}, "
          f"largest displacement {np.hypot(u - np.arange(W_RIG)[None, :], v - np.arange(H_RIG)[:, None]).max():.1f} px")
    assert inside.mean() > 0.8
    assert np.array_equal(out[inside], np.floor(sp + 0.5).astype(np.uint8))
    if dset == "strong":      # the zero border: every pixel whose taps are all outside is 0
        allout = (np.floor(u) < -1) | (np.floor(u) >= W_RIG) | (np.floor(v) < -1) | (np.floor(v) >= H_RIG)
        assert allout.any() and (out[allout] == 0).all()


def test_affine_image_is_reproduced_exactly():
    """Bilinear interpolation reproduces an affine image: checks the map (u, v) without the bilinear code."""
    H, W = 48, 64
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    img = (2 * j + i + 10).astype(np.uint8)
    intr = np.array([[400, 0, 31.3], [0, 398, 24.6], [0, 0, 1]], dtype=np.float32)
    for dist in (R.DIST['wide'], np.array([3.0, -20.0, 2e-2, 1e-2, 0.0], dtype=np.float32)):
        u, v = R.source_coordinates(H, W, intr, dist)
        _, inside = R.undistort_values(img, intr, dist)
        out = R.undistort_image(img, intr, dist)
        assert inside.sum() > 0.5 * H * W
        assert np.array_equal(out[inside], np.floor(2 * u + v + 10.5)[inside].astype(np.uint8))


@pytest.mark.parametrize("intr,dist", [(R.K_LONG, R.DIST['strong']), (R.K_WIDE, R.DIST['wide'])], ids=["long-strong", "wide"])
def test_map_direction_and_size(intr, dist):
    """A point at pinhole pixel p_u appears in the raw image at p_d = distort(p_u); undistortion brings a blob drawn at p_d back to
    p_u.  The bound, 0.1 px, is four times the worst centroid error measured for this reference (the centroid of an 8-bit blob moves
    with its sub-pixel placement): an inverted or mis-scaled map misses by the displacement itself, 15-78 px here."""
    fx, fy, cx, cy = R.camera_row(intr, dist)[:4]
    ii, jj = np.meshgrid(np.arange(H_RIG, dtype=np.float64), np.arange(W_RIG, dtype=np.float64), indexing='ij')
    worst, moved = 0.0, []
    for p_u in ((250.3, 200.7), (1380.6, 190.2), (1302.5, 1003.4), (310.8, 1010.1), (801.2, 140.5), (1450.4, 610.9)):
        xd, yd = R.distort_points((p_u[0] - cx) / fx, (p_u[1] - cy) / fy, dist)
        p_d = (fx * float(xd) + cx, fy * float(yd) + cy)
        assert 20 < p_d[0] < W_RIG - 20 and 20 < p_d[1] < H_RIG - 20
        moved.append(np.hypot(p_d[0] - p_u[0], p_d[1] - p_u[1]))
        raw = np.floor(200.0 * np.exp(-((jj - p_d[0]) ** 2 + (ii - p_d[1]) ** 2) / (2 * 3.0 ** 2)) + 0.5).astype(np.uint8)
        out = R.undistort_image(raw, intr, dist).astype(np.float64)
        cu, cv = (out * jj).sum() / out.sum(), (out * ii).sum() / out.sum()
        worst = max(worst, np.hypot(cu - p_u[0], cv - p_u[1]))
    print(f"displacements {min(moved):.1f}-{max(moved):.1f} px, worst centroid error {worst:.4f} px")
    assert min(moved) > 10.0
    assert worst < 0.1


def test_inverse_model_inverts_the_forward_model():
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-0.08, 0.08, 1000), rng.uniform(-0.06, 0.06, 1000)
    for dist in (R.DIST['mild'], R.DIST['strong'], R.DIST['tangential']):
        xi, yi = R.undistort_points(*R.distort_points(x, y, dist), dist)
        assert np.abs(xi - x).max() < 1e-12 and np.abs(yi - y).max() < 1e-12


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_gpu_images_are_far_from_rounding_ties(case):
    """The bit-exact GPU check must not hang on the last bit of a double: no pixel of its images lies within 1e-9 of a rounding tie
    (double-precision differences between orders of operations are about 1e-13)."""
    img, intr, dist = R.gpu_case_inputs(case)
    margin = R.rounding_margin(img, intr, dist)
    print(f"{case[0]}: margin {margin:.3e}")
    assert margin >= 1e-9


def test_gpu_batch_images_are_far_from_rounding_ties():
    images, intr, dist = R.batch_case()
    flat = images.reshape(-1, *images.shape[2:])
    margin = min(R.rounding_margin(flat[n], intr[n % 9], dist[n % 9]) for n in range(flat.shape[0]))
    print(f"batch: margin {margin:.3e}")
    assert margin >= 1e-9
    # nine different camera rows really are nine different maps
    outs = [R.undistort_image(flat[0], intr[c], dist[c]) for c in range(9)]
    assert all(not np.array_equal(outs[a], outs[b]) for a in range(9) for b in range(a))


def _tiny_take(tmp_path, distortion=None):
    from fpc_diffrend_amd import scene
    sc = scene.make_scene(mesh=(8, 4), K=2, n_frames=2, resolution=(24, 32), texshape=(8, 8, 1))
    images = np.random.default_rng(0).integers(0, 141, size=(2, 2, 24, 32), dtype=np.uint8)
    return sc, images, scene.write_take(sc, str(tmp_path / "take"), images, cam_idxs=(0, 1), distortion=distortion)


def test_write_take_distortion_and_load_raw_image(tmp_path):
    from fpc_diffrend_amd import data, scene
    d = np.array([[-0.25, 0.5, 1e-3, -2e-3, 0.125], [0.75, -1.5, 0.0, 4e-3, -0.5]], dtype=np.float32)
    sc, images, (base, bldir, calib, imdir) = _tiny_take(tmp_path, distortion=d)
    cams = sorted(os.listdir(imdir))
    lookup = data.load_calibration(calib, cams)
    assert all(c['dist'].shape == (5, 1) and c['dist'].dtype == np.float32 for c in lookup)
    assert np.array_equal(np.stack([c['dist'].reshape(5) for c in lookup]), d)
    # undistort=False is what it was: the clipped, flipped images, whatever the calibration says
    take = scene.from_take(base, bldir, calib, imdir)
    assert np.array_equal(take.images, images)
    raw = data.load_raw_image(os.path.join(imdir, cams[1], f"{cams[1]}_01.tif"))
    assert raw.dtype == np.uint8 and raw.shape == (24, 32) and np.array_equal(raw, images[1, 1][::-1])
    # default: zeros, as before
    _, _, (_, _, calib0, imdir0) = _tiny_take(tmp_path / "zero")
    assert all(not c['dist'].any() for c in data.load_calibration(calib0, sorted(os.listdir(imdir0))))
    from PIL import Image
    Image.fromarray(np.arange(24 * 32, dtype=np.uint16).reshape(24, 32)).save(tmp_path / "deep.tif")
    with pytest.raises(ValueError):
        data.load_raw_image(str(tmp_path / "deep.tif"))


def test_undistortion_has_no_cpu_path(tmp_path):
    import torch
    from fpc_diffrend_amd import ops, scene
    _, _, (base, bldir, calib, imdir) = _tiny_take(tmp_path)
    with pytest.raises(RuntimeError):
        scene.from_take(base, bldir, calib, imdir, undistort=True, device='cpu')
    with pytest.raises(RuntimeError):
        scene.undistort_take(imdir, calib, str(tmp_path / "out"), device='cpu')
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            scene.from_take(base, bldir, calib, imdir, undistort=True)
    with pytest.raises(ValueError):
        ops.undistort_images(torch.zeros(2, 4, 4, dtype=torch.uint8), np.eye(3)[None], np.zeros((1, 5)))


def test_undistort_kernel_has_no_private_segment():
    """a kernel with a private segment is dispatched several times slower.  k_undistort_u8 keeps its 16 results in
    four packed registers; read from the built object (tests/codeobj.py)."""
    import codeobj
    recs = codeobj.kernels("undistort.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = 0
    for name, private, lds in recs:
        if "k_undistort_u8" in name:
            seen += 1
            assert private == 0, name
            assert lds == 0, name
    assert seen == 1

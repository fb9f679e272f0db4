"""GPU: fpcdr_undistort_u8 / ops.undistort_images against the float64 statement of the rule (tests/undistort_ref.py, itself checked
in tests/test_undistort_ref.py) -- BIT-EXACT, as the project's other integer buffers are against their references -- and the
take-level surface built on it: scene.from_take(undistort=True), scene.undistort_take."""
import os

import numpy as np
import pytest
import torch

import undistort_ref as R

pytestmark = pytest.mark.gpu


def _mismatch(out, ref):
    d = out != ref
    return f"{int(d.sum())} of {d.size} bytes differ, first at {tuple(np.argwhere(d)[0]) if d.any() else None}"


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c[0] for c in R.GPU_CASES])
def test_undistort_is_bit_exact(case):
    """Every byte, no tolerance, no excluded pixel: sizes 1200 x 1600, 1080 x 1920, 37 x 53 (row tails, unaligned rows) and 5 x 1;
    zero, mild, strong (12 % of the taps outside) and purely tangential coefficients; clip 140 / 255; flip on / off; noise and smooth
    images.  No pixel of these images is within 1e-9 of a rounding tie (test_gpu_images_are_far_from_rounding_ties), so a mismatch is
    not the last bit of a double: it is a contracted multiply-add, float where double was meant, or a tap rule."""
    import fpc_diffrend_amd.ops as dr
    _, H, W, _, clip_max, flip, _, _ = case
    img, intr, dist = R.gpu_case_inputs(case)
    ref = R.undistort_image(img, intr, dist, clip_max=clip_max, flip_rows=flip)
    src = torch.from_numpy(img)[None].cuda()
    out = dr.undistort_images(src, intr[None], dist[None], clip_max=clip_max, flip_rows=flip)
    assert out.shape == src.shape and out.dtype == torch.uint8 and out.data_ptr() != src.data_ptr()
    assert torch.equal(src.cpu()[0], torch.from_numpy(img)), "the input was written to"
    assert torch.equal(out.cpu()[0], torch.from_numpy(ref)), _mismatch(out.cpu().numpy()[0], ref)
    # [Nc,5,1], as data.load_calibration holds it, and float64 tables of the same values: same bytes
    out2 = dr.undistort_images(src, torch.tensor(intr, dtype=torch.float64)[None], dist.reshape(1, 5, 1), clip_max=clip_max, flip_rows=flip)
    assert torch.equal(out2, out)


def test_undistort_batch_uses_camera_n_mod_nc():
    """A [3,9,H,W] batch with nine different camera rows: image n is undistorted with row n % 9; the flat [27,H,W] view gives the
    same bytes."""
    import fpc_diffrend_amd.ops as dr
    images, intr, dist = R.batch_case()
    for clip_max, flip in ((140, True), (255, False)):
        ref = R.undistort_batch(images, intr, dist, clip_max=clip_max, flip_rows=flip)
        src = torch.from_numpy(images).cuda()
        out = dr.undistort_images(src, intr, dist, clip_max=clip_max, flip_rows=flip)
        assert out.shape == src.shape
        assert torch.equal(out.cpu(), torch.from_numpy(ref)), _mismatch(out.cpu().numpy(), ref)
        flat = dr.undistort_images(src.reshape(27, *images.shape[2:]), intr, dist, clip_max=clip_max, flip_rows=flip)
        assert torch.equal(flat.reshape(out.shape), out)


def test_undistort_images_rejects_bad_input():
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd import _lib
    img = torch.zeros(2, 8, 12, dtype=torch.uint8, device='cuda')
    K, d = np.stack([R.intrinsics_for(8, 12)] * 2), np.zeros((2, 5), dtype=np.float32)
    dr.undistort_images(img, K, d)
    with pytest.raises(ValueError):
        dr.undistort_images(img.cpu(), K, d)                                   # no CPU path
    with pytest.raises(ValueError):
        dr.undistort_images(img.float(), K, d)
    with pytest.raises(ValueError):
        dr.undistort_images(torch.zeros(2, 8, 24, dtype=torch.uint8, device='cuda')[:, :, ::2], K, d)      # not contiguous
    with pytest.raises(ValueError):
        dr.undistort_images(img[0], K, d)                                      # [H,W]
    with pytest.raises(ValueError):
        dr.undistort_images(img, K[:, :2], d)
    with pytest.raises(ValueError):
        dr.undistort_images(img, K, d[:, :4])
    with pytest.raises(ValueError):
        dr.undistort_images(img, K, d[:1])                                     # one row of coefficients for two cameras
    with pytest.raises(ValueError):
        dr.undistort_images(img.reshape(1, 2, 8, 12), K[:1], d[:1])            # [F,Nc,H,W] with another Nc
    with pytest.raises(ValueError):
        dr.undistort_images(img, K, d, clip_max=256)
    # the C ABI itself: in place, and non-positive sizes
    table = torch.zeros(2, 9, dtype=torch.float64, device='cuda')
    p = lambda t: t.data_ptr()
    for args in ((p(img), p(img), p(table), 2, 8, 12, 2, 255, 0), (p(img), p(torch.empty_like(img)), p(table), 0, 8, 12, 2, 255, 0),
                 (p(img), p(torch.empty_like(img)), p(table), 2, 8, 0, 2, 255, 0), (p(img), p(torch.empty_like(img)), p(table), 2, 8, 12, 0, 255, 0)):
        with pytest.raises(RuntimeError, match="fpcdr_undistort_u8"):
            _lib.call("fpcdr_undistort_u8", *args, None)


# ---- take level ------------------------------------------------------------------------------------------------------------------
CAMS = (0, 3, 6)
# barrel distortion, monotonic over the whole 256 x 256 frame of cfg1's lenses (f = 1130-1230 px): it pulls the head's outline,
# 77 px from the centre, about 8 px inwards, so every undistorted pixel looks INSIDE the raw image
TAKE_DIST = np.array([[-24, 340, 2e-3, -1e-3, 0], [-27, 420, -1e-3, 2e-3, 0], [-28, 450, 1e-3, 1e-3, 0]], dtype=np.float32)
FIT = dict(max_iter=40, lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, weight_laplacian=0.0, init_texture='truth')


@pytest.fixture(scope="module")
def raw_take(tmp_path_factory):
    """cfg1, three cameras: the rendered targets are the ideal (pinhole) images; the raw capture of each is synthesised with the
    test-side inverse model and written as a take whose calibration carries the coefficients."""
    from fpc_diffrend_amd import fit, scene
    tmp = tmp_path_factory.mktemp("raw_take")
    sc = scene.cfg('cfg1', n_frames=4)
    sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
    a = fit.Fitter(sc, fit.FitConfig(cam_idxs=CAMS, **FIT), device='cuda')
    ideal = a.targets.cpu().numpy()[:, :, ::-1]                           # [F,3,H,W], row 0 = top
    intr = [np.asarray(sc.cams[c]['intr'], dtype=np.float32) for c in CAMS]
    raw = np.stack([np.stack([R.distort_image(ideal[f, j], intr[j], TAKE_DIST[j], fill=45) for j in range(3)]) for f in range(4)])
    paths = scene.write_take(sc, str(tmp / "take"), np.ascontiguousarray(raw[:, :, ::-1]), cam_idxs=CAMS, distortion=TAKE_DIST)
    return dict(sc=sc, ideal=ideal, raw=raw, intr=intr, paths=paths, tmp=tmp)


def test_from_take_undistorts_byte_for_byte(raw_take, monkeypatch):
    from fpc_diffrend_amd import scene
    t = raw_take
    base, bldir, calib, imdir = t['paths']
    margin = min(R.rounding_margin(t['raw'][f, j], t['intr'][j], TAKE_DIST[j]) for f in range(4) for j in range(3))
    print(f"take images: rounding margin {margin:.3e}")
    assert margin >= 1e-9
    ref = np.stack([np.stack([R.undistort_image(t['raw'][f, j], t['intr'][j], TAKE_DIST[j], clip_max=140, flip_rows=True)
                              for j in range(3)]) for f in range(4)])
    plain = scene.from_take(base, bldir, calib, imdir)
    assert np.array_equal(plain.images, np.minimum(t['raw'], 140)[:, :, ::-1])          # undistort=False: as before
    take = scene.from_take(base, bldir, calib, imdir, undistort=True)
    assert take.images.dtype == np.uint8 and take.images.shape == ref.shape and take.resolution == (256, 256)
    assert np.array_equal(take.images, ref), _mismatch(take.images, ref)
    assert not np.array_equal(take.images, plain.images)
    # chunks of ONE frame (device memory independent of the take's length): same bytes
    monkeypatch.setattr(scene, "UNDISTORT_CHUNK_BYTES", 1)
    assert np.array_equal(scene.from_take(base, bldir, calib, imdir, undistort=True).images, ref)
    # undistort once, read the result with the default from_take
    out_dir = scene.undistort_take(imdir, calib, str(t['tmp'] / "undistorted"))
    assert sorted(os.listdir(out_dir)) == sorted(os.listdir(imdir))
    assert all(sorted(os.listdir(os.path.join(out_dir, c))) == sorted(os.listdir(os.path.join(imdir, c))) for c in os.listdir(imdir))
    again = scene.from_take(base, bldir, calib, out_dir)
    assert np.array_equal(again.images, ref), _mismatch(again.images, ref)
    from fpc_diffrend_amd import data
    cam = sorted(os.listdir(out_dir))[1]
    full = data.load_raw_image(os.path.join(out_dir, cam, f"{cam}_02.tif"))                # 8-bit TIFF, full range, rows as they are
    assert np.array_equal(full, R.undistort_image(t['raw'][2, 1], t['intr'][1], TAKE_DIST[1]))


def test_undistorted_take_fits_the_pinhole_render(raw_take):
    """What the feature is for: at the ground-truth parameters the pinhole render matches the undistorted images better than the raw
    ones (an inequality only), and the fit loop runs on them."""
    from fpc_diffrend_amd import fit, scene
    t = raw_take
    sc = t['sc']
    # the outline moves by at least 5 px: largest displacement over the foreground of the ideal images
    moved = 0.0
    for j in range(3):
        u, v = R.source_coordinates(256, 256, t['intr'][j], TAKE_DIST[j])
        disp = np.hypot(u - np.arange(256)[None, :], v - np.arange(256)[:, None])
        moved = max(moved, float(disp[t['ideal'][0, j] != 45].max()))
    print(f"largest displacement on the head: {moved:.1f} px")
    assert moved >= 5.0
    base, bldir, calib, imdir = t['paths']
    losses = {}
    for und in (True, False):
        take = scene.from_take(base, bldir, calib, imdir, undistort=und)
        take.texture, take.blendshapes = sc.texture.copy(), sc.blendshapes.copy()        # (the take's own columns come in os.listdir order)
        ft = fit.Fitter(take, fit.FitConfig(cam_idxs=(0, 1, 2), **FIT), device='cuda')
        with torch.no_grad():
            ft.maps['local'].copy_(torch.eye(4, device='cuda'))
            ft.maps_intermediate['local'].copy_(torch.tensor(sc.weights_gt, device='cuda').t())
            ft.per_frame_t.copy_(torch.tensor(sc.t_gt, device='cuda'))
        losses[und] = float(ft.loss_and_backward(slice(0, 4)))
        if und:
            after = float(ft.step())
            assert np.isfinite(after) and all(torch.isfinite(p).all() for p in ft.params)
    print(f"pixel loss at the ground truth: undistorted {losses[True]:.4f}, raw {losses[False]:.4f}")
    assert np.isfinite(losses[True]) and losses[True] < losses[False]

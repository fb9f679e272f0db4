"""GPU: fpcdr_exposure_sums / fpcdr_apply_lut_u8, ops.exposure_sums / ops.apply_lut_u8 and Fitter.equalise_exposure against the numpy
statement of the Exposure rule (tests/exposure_ref.py, itself checked in tests/test_exposure_ref.py) -- torch.equal / array_equal:
integers throughout, no tolerance anywhere in the device tests.

Measured on an MI355X (the 128 x 128 scene, cameras 0 and 4, two frames, truth parameters and texture; captures round(0.75 x + 8) and
round(1.25 x - 6); test_fitter_equalises_the_readme_scene prints them):

    method       loss before   after   equal exposures   a0, a4            b0, b4            rho0, rho4        g0, g4          second call's g
    regression   45.346        1.041   0.017             0.75003 1.24989   8.0003 -5.9901    0.99915 0.99967   1.3332 0.8000   1.00010 0.99990
    moments      45.346        1.041   0.017             0.75067 1.25030   7.9511 -6.0210    0.99915 0.99967   1.3328 0.8002   0.99947 1.00053

Of the 1.041 that remain, 1.0 is the square of the common offset b_common = (8 - 6) / 2 = 1 grey level that the mean level leaves between
all mapped captures and the texture (the texture absorbs it); the rest is the two roundings.  Three steps equalised at iteration 1:
45.346, 1.305, 1.318, eager and in graph mode alike; six steps equalised at iteration 4 behind a capture at iteration 3:
45.346 45.629 45.602 45.592 1.290 1.266, eager and replayed (the two runs printed the same float32 values; the test holds them to the
neighbouring graph tests' bar).

Device times (profiles/exposure_time.txt; 288 images of 1080 x 1920, C = 1, HIP-event medians): fpcdr_exposure_sums 3.35 ms (3.75 TB/s
over 21 B/px; fpcdr_robust_loss without gradient 1.85 ms), fpcdr_apply_lut_u8 0.222 ms (5.37 TB/s of 2 B/px; the torch gather 5.36 ms),
the whole Fitter.equalise_exposure() 13.0 ms (Fitter.bake_texture() 17.9 ms)."""
import ctypes

import numpy as np
import pytest
import torch

import exposure_ref as R

pytestmark = pytest.mark.gpu
NAMES = ("fpcdr_exposure_sums", "fpcdr_apply_lut_u8")
GUARD = 48
FILL = 0xA5
SENTINEL = -0x0123456789ABCDEF


def _dev(a, shift=0):
    """a numpy array on the GPU, `shift` ELEMENTS into a larger buffer whose base is 256-byte aligned"""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(a.size + shift, dtype=torch.from_numpy(a).dtype, device='cuda')
    assert buf.data_ptr() % 256 == 0
    t = buf[shift:]
    t.copy_(torch.from_numpy(a.reshape(-1)))
    return t.reshape(a.shape)


def _sums(colour, rast, ref, mask=None, face_w=None, lo=1, hi=254, shift=0, pre=None):
    """One call of the C entry; sums sits between sentinel rows, which are checked.  Returns int64 numpy [B,6]."""
    from fpc_diffrend_amd import _lib
    B, H, W, C = colour.shape
    t = [_dev(colour, shift), _dev(rast, shift), _dev(ref, shift), None if mask is None else _dev(mask, shift),
         None if face_w is None else _dev(face_w, shift)]
    buf = torch.full((B + 2, 6), SENTINEL, dtype=torch.int64, device='cuda')
    buf[1:-1] = 0 if pre is None else torch.from_numpy(pre).cuda()
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    with torch.cuda.device(buf.device):
        _lib.call(NAMES[0], p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), 0 if face_w is None else len(face_w), lo, hi, B, H, W, C,
                  ctypes.c_void_p(buf[1:].data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    out = buf.cpu().numpy()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all(), "wrote outside sums"
    for x, src in zip(t[:3], (colour, rast, ref)):
        assert np.array_equal(x.cpu().numpy(), src, equal_nan=True), "an input changed"
    return out[1:-1]


@pytest.mark.parametrize("lo,hi", [(0, 255), (1, 139)])
@pytest.mark.parametrize("with_faces", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", R.SIZES)
def test_sums_rule(H, W, B, C, with_mask, with_faces, lo, hi):
    """Every small case of the statement's self-check (R.case: NaN, +-inf, negative and > 1 colours, ties; holes on the border, in the
    corners and singly inside; a face table one short of the largest id with zeros; mask bytes 0, 127, 128, 255): widths 1, 17, 16, 33
    -- a tail alone, a chunk and a tail, one whole chunk, two and a tail -- and 72 x 96 = 432 chunks, two workgroups.  Pre-filled sums
    are added to, the rows around them stay, and a second run gives the same bits."""
    colour, rast, ref, mask, face_w = R.case(B, H, W, C, seed=H * 1000 + W * 10 + B + C)
    kw = dict(mask=mask if with_mask else None, face_w=face_w if with_faces else None, lo=lo, hi=hi)
    want = R.sums(colour, rast, ref, **kw)
    got = _sums(colour, rast, ref, **kw)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(_sums(colour, rast, ref, **kw), got)
    pre = (np.arange(B * 6, dtype=np.int64).reshape(B, 6) + 1) * (1 << 40)
    assert np.array_equal(_sums(colour, rast, ref, pre=pre, **kw), pre + want)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(5, 16), (7, 33), (72, 96)])
def test_sums_at_an_unaligned_base(H, W, C):
    """Every input one ELEMENT into a larger buffer (the captures and the mask one byte, the floats four): no 16-byte form can be taken."""
    colour, rast, ref, mask, face_w = R.case(3, H, W, C, seed=77 + H + C)
    want = R.sums(colour, rast, ref, mask, face_w, 1, 139)
    assert np.array_equal(_sums(colour, rast, ref, mask, face_w, 1, 139, shift=1), want)
    assert np.array_equal(_sums(colour, rast, ref, shift=1), R.sums(colour, rast, ref))


def test_sums_do_not_depend_on_order_or_on_the_split():
    """The images permuted, and the batch split over two calls into one table, give the same per-camera totals (two cameras, image b
    belongs to camera b % 2)."""
    import fpc_diffrend_amd.ops as dr
    colour, rast, ref, mask, face_w = R.case(6, 40, 50, 3, seed=9)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kw = dict(lo=1, hi=200)
    whole = dr.exposure_sums(t(colour), t(rast), t(ref), mask=t(mask), face_weights=t(face_w), **kw)
    assert whole.dtype == torch.int64 and np.array_equal(whole.cpu().numpy(), R.sums(colour, rast, ref, mask, face_w, 1, 200))
    per_cam = whole.reshape(3, 2, 6).sum(0)
    perm = np.array([4, 1, 2, 5, 0, 3])                                         # keeps every image's camera
    assert np.array_equal(perm % 2, np.arange(6) % 2)
    other = dr.exposure_sums(t(colour[perm]), t(rast[perm]), t(ref[perm]), mask=t(mask[perm]), face_weights=t(face_w), **kw)
    assert torch.equal(other.reshape(3, 2, 6).sum(0), per_cam)
    table = torch.zeros(2, 6, dtype=torch.int64, device='cuda')
    for part in (slice(0, 2), slice(2, 6)):
        s = dr.exposure_sums(t(colour[part]), t(rast[part]), t(ref[part]), mask=t(mask[part]), face_weights=t(face_w), **kw)
        table += s.reshape(-1, 2, 6).sum(0)
    assert torch.equal(table, per_cam)
    again = whole.clone()
    assert dr.exposure_sums(t(colour), t(rast), t(ref), sums=again, mask=t(mask), face_weights=t(face_w), **kw) is again
    assert torch.equal(again, 2 * whole)


def test_ops_exposure_sums_errors():
    import fpc_diffrend_amd.ops as dr
    c, r = torch.zeros(2, 8, 8, 3, device='cuda'), torch.zeros(2, 8, 8, 4, device='cuda')
    t = torch.zeros(2, 8, 8, dtype=torch.uint8, device='cuda')
    for kw in (dict(lo=-1), dict(hi=256), dict(lo=9, hi=8), dict(lo=1.0), dict(mask=t[:1]), dict(mask=t.float()), dict(face_weights=torch.zeros(0, device='cuda')),
               dict(sums=torch.zeros(2, 5, dtype=torch.int64, device='cuda')), dict(sums=torch.zeros(2, 6, dtype=torch.int32, device='cuda')),
               dict(face_weights=torch.zeros(4))):
        with pytest.raises(ValueError):
            dr.exposure_sums(c, r, t, **kw)
    for args in ((c[..., :2].permute(0, 2, 1, 3), r, t), (c, r[:1], t), (c, r, t[:, :4]), (torch.zeros(2, 8, 8, 5, device='cuda'), r, t), (c.double(), r, t)):
        with pytest.raises(ValueError):
            dr.exposure_sums(*args)


# ---- apply -------------------------------------------------------------------------------------------------------------------------------
def _tables(Nl, seed):
    rng = np.random.default_rng(seed)
    lut = np.stack([rng.permutation(256) for _ in range(Nl)]).astype(np.uint8)      # permutations
    lut[0] = np.arange(256)                                                        # the identity
    if Nl > 2:
        lut[2] = 77                                                                # a constant
    return lut


def _apply(images, lut, cams, shift=0, expect_error=False):
    """One call of the C entry on images [B,HW], `shift` bytes off an aligned base, between guard bytes, which are checked."""
    from fpc_diffrend_amd import _lib
    B, HW = images.shape
    buf = torch.full((GUARD + shift + B * HW + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 256 == 0
    img = buf[GUARD + shift: GUARD + shift + B * HW]
    img.copy_(torch.from_numpy(images.reshape(-1)))
    t_lut, t_cam = _dev(lut, shift), _dev(np.asarray(cams, dtype=np.int32))
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    with torch.cuda.device(buf.device):
        args = (NAMES[1], p(img), p(t_lut), p(t_cam), lut.shape[0], B, HW, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if expect_error:
            with pytest.raises(RuntimeError, match=NAMES[1] + r".*outside \[0, "):
                _lib.call(*args)
        else:
            _lib.call(*args)
    out = buf.cpu().numpy()
    assert (out[:GUARD + shift] == FILL).all() and (out[GUARD + shift + B * HW:] == FILL).all(), "wrote outside the images"
    assert np.array_equal(t_lut.cpu().numpy(), lut)
    return out[GUARD + shift: GUARD + shift + B * HW].reshape(B, HW)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("Nl", [1, 9])
@pytest.mark.parametrize("H,W", R.SIZES + ((1, 4096 + 5),))
def test_apply_rule(H, W, Nl, shift):
    """Image sizes 1, 51, 80, 231 and 6912 bytes (and 4101: two workgroups with a tail): not multiples of 16 but one, so images start at
    every residue; an aligned base and one a byte off; one table (the identity) and nine (permutations, the identity, a constant).  The
    bytes in front of the first and beyond the last image stay."""
    rng = np.random.default_rng(H * W + Nl)
    B = 5
    images = rng.integers(0, 256, size=(B, H * W), dtype=np.uint8)
    images[0, : min(256, H * W)] = np.arange(min(256, H * W))
    lut = _tables(Nl, seed=Nl)
    cams = rng.integers(0, Nl, size=B)
    cams[-1] = Nl - 1
    got = _apply(images, lut, cams, shift)
    assert np.array_equal(got, R.apply(images, lut, cams))
    if Nl == 1:
        assert np.array_equal(got, images)


def test_apply_with_a_camera_out_of_range():
    """The error is returned, that image is unchanged and the others are mapped; nothing faults."""
    rng = np.random.default_rng(4)
    images = rng.integers(0, 256, size=(4, 300), dtype=np.uint8)
    lut = _tables(3, seed=1)
    for cams in ([1, 3, 2, 1], [1, -1, 2, 1], [1, 2 ** 31 - 1, 2, 1]):
        got = _apply(images, lut, cams, expect_error=True)
        assert np.array_equal(got[1], images[1])
        assert np.array_equal(got, R.apply(images, lut, cams))


def test_ops_apply_lut():
    import fpc_diffrend_amd.ops as dr
    rng = np.random.default_rng(6)
    images = rng.integers(0, 256, size=(6, 2, 9, 21), dtype=np.uint8)
    lut, cams = _tables(3, seed=2), np.array([0, 1, 2, 2, 1, 1], dtype=np.int32)
    t = torch.from_numpy(images).cuda()
    out = dr.apply_lut_u8(t, torch.from_numpy(lut).cuda(), torch.from_numpy(cams).cuda())
    assert out is t and np.array_equal(t.cpu().numpy(), R.apply(images, lut, cams))
    L, c = torch.from_numpy(lut).cuda(), torch.from_numpy(cams).cuda()
    for args in ((t[:, :, ::2], L, c), (t, L[:, :255], c), (t, L, c[:5]), (t, L, c.long()), (t.float(), L, c), (t, L.cpu(), c)):
        with pytest.raises(ValueError):
            dr.apply_lut_u8(*args)
    with pytest.raises(RuntimeError, match="outside"):
        dr.apply_lut_u8(t, L, torch.full((6,), 3, dtype=torch.int32, device='cuda'))


# ---- the Fitter --------------------------------------------------------------------------------------------------------------------------
CAMS = (0, 4)
FR = slice(0, 2)


@pytest.fixture(scope="module")
def take():
    """The 128 x 128 scene, cameras 0 and 4, two frames; `equal`: the Fitter's own rendered captures; `gains`: camera 0's replaced by
    round(0.75 x + 8), camera 4's by round(1.25 x - 6), as the README's exposure scan makes them.  Both stay as they are."""
    from fpc_diffrend_amd import fit, scene
    sc = scene.make_scene(resolution=(128, 128), n_frames=2)
    ft = fit.Fitter(sc, fit.FitConfig(max_iter=10, cam_idxs=CAMS, weight_laplacian=0), device='cuda')
    equal = ft.targets.clone()
    x = equal.to(torch.float32)
    gains = equal.clone()
    gains[:, 0] = torch.round(0.75 * x[:, 0] + 8.0).to(torch.uint8)
    gains[:, 1] = torch.round(1.25 * x[:, 1] - 6.0).clamp(0, 255).to(torch.uint8)
    return sc, equal, gains


def _fitter(take, targets=None, rank=0, world=1, **kw):
    from fpc_diffrend_amd import fit
    sc, _, gains = take
    targets = gains if targets is None else targets
    kw.setdefault('weight_laplacian', 0)
    ft = fit.Fitter(sc, fit.FitConfig(max_iter=10, cam_idxs=CAMS, **kw), device='cuda', rank=rank, world=world,
                    targets=targets[rank * (2 // world): (rank + 1) * (2 // world)] if world > 1 else targets)
    with torch.no_grad():
        ft.init_near_truth(1.0)
        ft.per_frame_q.copy_(torch.tensor(sc.q_gt, device='cuda'))
    return ft


def _spy(monkeypatch):
    """Record what Fitter.equalise_exposure hands to ops.exposure_sums: the render read back from the GPU."""
    from fpc_diffrend_amd import fit
    seen, real = [], fit.dr.exposure_sums

    def spy(colour, rast, ref, **kw):
        seen.append((colour.cpu().numpy(), rast.cpu().numpy(), ref.cpu().numpy(),
                     {k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in kw.items()}))
        return real(colour, rast, ref, **kw)
    monkeypatch.setattr(fit.dr, "exposure_sums", spy)
    return seen


def _statement(seen, old, Nc=2, **kw):
    """The statement on the recorded renders and the old targets [F,Nc,H,W] (numpy): (fit, new targets)."""
    table = np.zeros((Nc, 6), dtype=np.int64)
    for colour, rast, ref, k in seen:
        table += R.sums(colour, rast, ref, k['mask'], k['face_weights'], k['lo'], k['hi']).reshape(-1, Nc, 6).sum(0)
    want = R.fit_gains(table, **kw)
    F, _, H, W = old.shape
    return want, R.apply(old.reshape(F * Nc, H * W), want['lut'], np.arange(F * Nc) % Nc).reshape(old.shape), table


@pytest.mark.parametrize("method", ['regression', 'moments'])
def test_fitter_equalises_the_readme_scene(take, monkeypatch, method):
    """After equalise_exposure() full_targets is the statement applied to the render read back from the GPU and to the old targets, bit
    for bit; the plain pixel loss at the truth falls below a tenth of what it was (45.3 before in the README's scan; what remains is two
    roundings, at most about (1 + g^2) / 12 = 0.23, on top of 0.017: the factor ten is a cap with room); a second call finds g within 1 %
    of 1; the caller's tensor is not written."""
    _, equal, gains = take
    keep = gains.clone()
    ft = _fitter(take)
    assert ft.full_targets is gains
    before = float(ft.loss_and_backward(FR))
    seen = _spy(monkeypatch)
    out = ft.equalise_exposure(method=method, chunk=1)
    assert len(seen) == 2 and seen[0][3]['lo'] == 1 and seen[0][3]['hi'] == 254 and seen[0][3]['mask'] is None and seen[0][3]['face_weights'] is None
    want, new, table = _statement(seen, keep.cpu().numpy(), method=method)
    assert torch.equal(gains, keep) and ft.full_targets is not gains and ft.targets is ft.full_targets
    assert torch.equal(ft.full_targets.cpu(), torch.from_numpy(new))
    assert np.array_equal(out['lut'], want['lut']) and np.array_equal(out['composite'], want['lut']) and out['usable'].all()
    assert np.array_equal(out['n'], table[:, 0].astype(np.float64)) and table[:, 0].min() > 1000
    for key in ('a', 'b', 'rho', 'g'):
        assert np.array_equal(out[key], want[key]), key
    assert torch.equal(ft.target_bg_sumsq, _bg(ft.full_targets))
    after = float(ft.loss_and_backward(FR))
    ref = _fitter(take, targets=equal)
    floor = float(ref.loss_and_backward(FR))
    print(f"EXPOSURE loss {method}: before {before:.3f} after {after:.3f} (equal exposures {floor:.3f});  a {out['a']} b {out['b']} "
          f"rho {out['rho']} g {out['g']}")
    assert after < 0.1 * before
    seen.clear()
    again = ft.equalise_exposure(method=method)
    print(f"EXPOSURE second call {method}: g {again['g']}")
    assert again['usable'].all() and np.abs(again['g'] - 1.0).max() <= 0.01
    assert np.array_equal(again['composite'], R.compose(want['lut'], again['lut']))
    quiet = ft.equalise_exposure(method=method, apply=False)
    assert np.array_equal(quiet['composite'], again['composite'])


def test_fitter_counts_with_masks_face_weights_and_saturation(take, monkeypatch):
    """The Scene's masks, cfg.face_weights and cfg.saturation = 140 reach the sums as the rule says -- the masks' rows of the chunk's
    images, the face table, lo = 1, hi = 139 -- and the table keeps bytes >= 140: full_targets equals the statement, bit for bit."""
    import dataclasses
    from fpc_diffrend_amd import fit
    sc, _, gains = take
    gains = gains.clone()
    gains[:, :, 60:68, 56:72] = 200      # saturated bytes in the middle of the face: they count nothing and stay
    rng = np.random.default_rng(21)
    masks = rng.choice(np.array([0, 127, 128, 255], dtype=np.uint8), size=(2, len(sc.cams), 128, 128), p=(0.1, 0.1, 0.4, 0.4))
    face_w = rng.uniform(0.1, 2.0, size=sc.pos_idx.shape[0]).astype(np.float32)
    face_w[::3] = 0.0
    cfg = fit.FitConfig(max_iter=10, cam_idxs=CAMS, weight_laplacian=0, saturation=140, face_weights=face_w)
    ft = fit.Fitter(dataclasses.replace(sc, masks=masks), cfg, device='cuda', targets=gains)
    with torch.no_grad():
        ft.init_near_truth(1.0)
        ft.per_frame_q.copy_(torch.tensor(sc.q_gt, device='cuda'))
    assert ft.exposure_range() == (1, 139, 140) and int((gains >= 140).sum()) > 0
    seen = _spy(monkeypatch)
    out = ft.equalise_exposure(chunk=1)
    assert len(seen) == 2
    for f, (_, _, ref, k) in enumerate(seen):
        assert (k['lo'], k['hi']) == (1, 139) and np.array_equal(k['face_weights'], face_w)
        assert np.array_equal(k['mask'], masks[f][list(CAMS)]) and np.array_equal(ref, gains[f].cpu().numpy())
    want, new, table = _statement(seen, gains.cpu().numpy(), keep_from=140)
    plain = R.fit_gains(np.zeros((2, 6), dtype=np.int64))['lut']
    assert out['usable'].all() and not np.array_equal(want['lut'], plain)
    assert np.array_equal(out['lut'], want['lut']) and np.array_equal(out['n'], table[:, 0].astype(np.float64))
    assert torch.equal(ft.full_targets.cpu(), torch.from_numpy(new))
    sat = gains >= 140
    assert torch.equal(ft.full_targets[sat], gains[sat]) and int((ft.full_targets >= 140).sum()) == int(sat.sum())
    assert np.isfinite(float(ft.loss_and_backward(FR)))


def _bg(targets):
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd import fit
    return dr.reference_background_sumsq(targets.reshape(-1, *targets.shape[2:]), fit.BACKGROUND).reshape(targets.shape[:2])


def test_an_anchor_cameras_captures_stay(take):
    _, _, gains = take
    ft = _fitter(take)
    out = ft.equalise_exposure(anchor_camera=0)
    assert torch.equal(ft.full_targets[:, 0], gains[:, 0]) and not torch.equal(ft.full_targets[:, 1], gains[:, 1])
    assert out['g'][0] == 1.0 and np.array_equal(out['lut'][0], np.arange(256))
    cfg_way = _fitter(take, equalise_anchor_camera=0)
    cfg_way.equalise_exposure()
    assert torch.equal(cfg_way.full_targets, ft.full_targets)
    with pytest.raises(ValueError, match="cam_idxs"):
        ft.equalise_exposure(anchor_camera=3)


def test_pyramid_levels_follow_the_captures(take):
    """After the call every level's targets equal downsample_images(full_targets, s) and every level's target_bg_sumsq equals
    reference_background_sumsq of them -- in the tensors the levels had."""
    import fpc_diffrend_amd.ops as dr
    ft = _fitter(take, pyramid=((4, 2), (2, 2)))
    held = {s: (lv[0], lv[2]) for s, lv in ft._levels.items()}
    ft.equalise_exposure()
    assert sorted(ft._levels) == [1, 2, 4] and ft._levels[1][0] is ft.full_targets
    for s, (lt, lres, lbg, _) in ft._levels.items():
        want = ft.full_targets if s == 1 else dr.downsample_images(ft.full_targets, s)
        assert torch.equal(lt, want) and torch.equal(lbg, _bg(want)), s
        if s > 1:
            assert lt is held[s][0]
        assert lbg is held[s][1]
    assert ft.targets is ft._levels[4][0] and np.isfinite(float(ft.step()))


def test_steps_equalised_at_iteration_1_eager_and_graph_mode(take):
    """Three steps of a Fitter equalised at iteration 1 through equalise_exposure_at=(1,): eager and hip_graph=True give losses identical
    to every printed digit -- three decimals, as the README's and DESIGN.md's scans print a loss; the targets were cloned at
    construction."""
    _, _, gains = take
    keep = gains.clone()
    traj = {}
    for graph in (False, True):
        ft = _fitter(take, equalise_exposure_at=(1,), hip_graph=graph, lr_base=1e-5, quat_renorm='rows')
        assert ft.full_targets is not gains
        traj[graph] = [f"{float(ft.step()):.3f}" for _ in range(3)]
        assert ft._exposure_total is not None and torch.equal(gains, keep)
    print(f"EXPOSURE steps eager {traj[False]} graph mode {traj[True]}")
    assert traj[False] == traj[True]
    assert float(traj[False][1]) < 0.1 * float(traj[False][0])


def test_a_captured_graph_replays_with_the_equalised_captures(take):
    """Equalised at iteration 4, behind the capture at iteration 3: the tensors the graph reads keep their addresses, so the replays
    of iterations 4 and 5 see the mapped captures -- the loss falls as it does in the eager run."""
    traj = {}
    for graph in (False, True):
        ft = _fitter(take, targets=take[2].clone(), equalise_exposure_at=(4,), hip_graph=graph, lr_base=1e-5, quat_renorm='rows')
        held = ft.full_targets
        traj[graph] = [float(ft.step()) for _ in range(6)]
        assert ft.full_targets is held
        if graph:
            assert ft._graphs is not None
    print(f"EXPOSURE graph replay eager {traj[False]} graphed {traj[True]}")
    for t in traj.values():
        assert t[4] < 0.1 * t[3]
    assert np.allclose(traj[False], traj[True], rtol=2e-3)      # (the bar of the neighbouring graph tests)


def test_two_ranks_fit_the_unsharded_tables(take):
    """Rank 0 and rank 1 of 2, whose `reduce` adds the other's sums, produce the unsharded Fitter's tables bit for bit."""
    whole = _fitter(take)
    want = whole.equalise_exposure()
    own = {}

    def keep(rank, other=None):
        def reduce(table):
            own[rank] = table.clone()
            return table if other is None else table + own[other]
        return reduce

    r0, r1 = _fitter(take, rank=0, world=2), _fitter(take, rank=1, world=2)
    r0.equalise_exposure(reduce=keep(0), apply=False)
    out1 = r1.equalise_exposure(reduce=keep(1, other=0))
    out0 = r0.equalise_exposure(reduce=lambda t: t + own[1])
    for out in (out0, out1):
        assert np.array_equal(out['lut'], want['lut']) and np.array_equal(out['a'], want['a']) and np.array_equal(out['b'], want['b'])
    assert torch.equal(torch.cat([r0.full_targets, r1.full_targets]), whole.full_targets)


def test_state_round_trip(take, tmp_path):
    import json
    ft = _fitter(take)
    assert "exposure_lut" not in ft.state_dict()
    ft.save(str(tmp_path / "plain"))
    assert not (tmp_path / "plain" / "exposure.json").exists()
    out = ft.equalise_exposure()
    sd = ft.state_dict()
    assert np.array_equal(sd["exposure_lut"].numpy(), out['composite'])
    fresh = _fitter(take)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.full_targets, ft.full_targets) and torch.equal(fresh.target_bg_sumsq, ft.target_bg_sumsq)
    fresh.load_state_dict(sd)                                                   # the same table again: nothing happens
    assert torch.equal(fresh.full_targets, ft.full_targets)
    other = _fitter(take)
    other.equalise_exposure(anchor_camera=0)
    with pytest.raises(ValueError, match="exposure table"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="no exposure table"):
        other.load_state_dict(_fitter(take).state_dict())                        # as read against mapped: not equal either
    ft.save(str(tmp_path / "out"))
    rec = json.load(open(tmp_path / "out" / "exposure.json"))
    names = [str(take[0].cams[c]['cam']) for c in CAMS]
    assert sorted(rec) == sorted(names)
    for j, name in enumerate(names):
        assert rec[name]['lut'] == out['composite'][j].tolist() and rec[name]['gain'] == float(out['g'][j]) and rec[name]['rho'] == float(out['rho'][j])


def test_defaults_leave_the_step_as_it_was(take, monkeypatch):
    """With every new option at its default three steps give the losses of the step as it was -- the body of step() before this feature,
    spelt out -- and neither new entry is ever called, nothing is cloned and no table exists."""
    from fpc_diffrend_amd import _lib
    _, _, gains = take
    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    ft, old = _fitter(take, lr_base=1e-5, quat_renorm='rows'), _fitter(take, lr_base=1e-5, quat_renorm='rows')
    calls.clear()      # (the constructors' own calls)
    new_way = [float(ft.step()) for _ in range(3)]
    mark = len(calls)
    old_way = []
    for _ in range(3):
        loss = old._eager_step(old.pick_frames(), old.pick_views(), False)
        old.scheduler.step()
        old.iteration += 1
        old_way.append(float(loss))
    print(f"EXPOSURE defaults: {new_way} / {old_way}")
    assert new_way == old_way and calls[:mark] == calls[mark:] and mark > 0
    assert not set(calls) & set(NAMES)
    assert ft.full_targets is gains and ft._exposure_total is None and "exposure_lut" not in ft.state_dict()

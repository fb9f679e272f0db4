"""GPU: fpcdr_overlay_u8 / ops.overlay_images against the numpy statement of the rule (tests/overlay_ref.py, itself checked in
tests/test_overlay_ref.py) -- everything torch.equal / array_equal: bytes, no tolerance, no excluded pixel -- and the surface built on
it: rerender.overlay_sequence against the reference's host expression, rerender.overlay_result against the host path on
render_multicam's images of the same saved result and against the statement on tensors rendered here with the same operators.

The kernel's chunking (csrc/overlay.hip): one thread owns 16 consecutive pixels of a row, a wave 64 such chunks -- which it walks four at
a time, 16 lanes a chunk, for the raster inputs --, a workgroup 256.  The shapes below are chosen for that: 16 = one chunk a row; 37 = two
whole chunks and a 5-pixel tail, rows that start unaligned; 64 = the four chunks of one trip in one row; 3 x 1600 = 100 chunks a row, rows
that begin in the middle of a wave and a second workgroup; 70 x 48 = 210 chunks, rows that span waves; 300 x 16 = two workgroups, the
second one partly empty."""
import os

import numpy as np
import pytest
import torch

import overlay_ref as R
from helpers import comparison_pair

pytestmark = pytest.mark.gpu

GREEN = (0, 255, 0)


def _mismatch(out, ref):
    d = np.asarray(out) != np.asarray(ref)
    return f"{int(d.sum())} of {d.size} entries differ, first at {tuple(np.argwhere(d)[0]) if d.any() else None}"


def _rgb(c):
    return int(c[0]) | int(c[1]) << 8 | int(c[2]) << 16


def _check(host, dev, use_rast, use_db, weight, outside, wire, half_width, flip):
    """One call of ops.overlay_images against the statement.  host / dev: dicts of the same img, ref, rast, rast_db as numpy / GPU."""
    import fpc_diffrend_amd.ops as dr
    out = dr.overlay_images(dev['img'], dev['ref'], rast=dev['rast'] if use_rast else None, rast_db=dev['rast_db'] if use_db else None,
                            weight=weight, outside=outside, wire=wire, half_width=half_width, scale=255.0, flip_rows=flip)
    want = R.overlay(host['img'], host['ref'], host['rast'] if use_rast else None, host['rast_db'] if use_db else None,
                     w=int(np.rint(weight * 256)), outside_capture=outside == 'capture', hw2=R.hw2_of(half_width) if wire else 0.0,
                     wire_rgb=wire or GREEN, scale=255.0, flip_rows=flip)
    tag = f"rast {use_rast}, db {use_db}, weight {weight}, outside {outside}, wire {wire}, hw {half_width}, flip {flip}, {host['img'].dtype} {host['img'].shape}"
    assert out.dtype == torch.uint8 and tuple(out.shape) == host['ref'].shape + (3,), tag
    assert torch.equal(out.cpu(), torch.from_numpy(want)), tag + ": " + _mismatch(out.cpu().numpy(), want)
    return want


def _inputs(N, H, W, kind, seed):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    img = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8) if kind == "u8" else R.float_image(N, H, W, rng)
    rast, rast_db = R.raster_inputs(N, H, W, rng)
    host = dict(img=img, ref=ref, rast=rast, rast_db=rast_db)
    return host, {k: torch.from_numpy(v).cuda() for k, v in host.items()}


def _unchanged(host, dev):
    for k in host:      # (bytes: NaNs too)
        assert np.array_equal(dev[k].cpu().numpy().reshape(-1).view(np.uint8), host[k].reshape(-1).view(np.uint8)), k


SHAPES = [(2, 5, 16), (3, 7, 37), (2, 9, 64), (1, 3, 1600), (2, 70, 48), (1, 300, 16)]


@pytest.mark.parametrize("kind", ["u8", "float"])
@pytest.mark.parametrize("N,H,W", SHAPES, ids=["x".join(str(s) for s in shp) for shp in SHAPES])
def test_rule_grid(N, H, W, kind):
    """Both input types; flip on and off; without rast (every weight); with rast but without rast_db, both `outside`; the wire at half
    widths 0.5 and 1.0, both `outside`.  The planted non-finite values, exact halves, u = 0, v = 0 and b2 at and below 0 are in every
    input (overlay_ref.float_image, raster_inputs); 20-40 % of the covered pixels are wire at half width 0.5."""
    host, dev = _inputs(N, H, W, kind, seed=1000 * H + W)
    cov = host['rast'][..., 3] > 0
    share = (R.wire_mask(host['rast'], host['rast_db'], R.hw2_of(0.5)) & cov).sum() / cov.sum()
    assert 0.2 <= share <= 0.4, share
    assert 0.45 <= cov.mean() <= 0.75
    for flip in (False, True):
        for weight in (0.0, 0.5, 77 / 256, 1.0):
            _check(host, dev, False, False, weight, 'render', None, 0.5, flip)
        for outside in ('render', 'capture'):
            _check(host, dev, True, False, 0.5, outside, None, 0.5, flip)
            a = _check(host, dev, True, True, 77 / 256, outside, GREEN, 0.5, flip)
            b = _check(host, dev, True, True, 0.5, outside, (255, 0, 7), 1.0, flip)
            assert (a == np.array(GREEN, dtype=np.uint8)).all(-1).sum() < (b == np.array((255, 0, 7), dtype=np.uint8)).all(-1).sum()
        _check(host, dev, True, True, 1.0, 'capture', None, 0.5, flip)           # both raster inputs given, no wire asked for
    # [N,H,W,1], as the render hands it over
    import fpc_diffrend_amd.ops as dr
    out = dr.overlay_images(dev['img'][..., None], dev['ref'], rast=dev['rast'], rast_db=dev['rast_db'], wire=GREEN, flip_rows=True)
    want = R.overlay(host['img'], host['ref'], host['rast'], host['rast_db'], hw2=R.hw2_of(0.5), wire_rgb=GREEN, flip_rows=True)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    _unchanged(host, dev)


@pytest.mark.parametrize("kind", ["u8", "float"])
def test_unaligned_base_addresses(kind):
    """3 x 9 x 48 with every input and the output, one at a time and all together, placed one element into a larger buffer, so that its
    base address is not a multiple of 16 (torch's own allocations are): the element-wise paths.  Through the C ABI, which takes the
    output's address; 0xAA guard bytes around the output stay untouched."""
    from fpc_diffrend_amd import _lib
    N, H, W = 3, 9, 48
    host, dev = _inputs(N, H, W, kind, seed=11)
    want = R.overlay(host['img'], host['ref'], host['rast'], host['rast_db'], w=77, outside_capture=True, hw2=R.hw2_of(0.5),
                     wire_rgb=GREEN, flip_rows=True)

    def shifted(t):
        buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device='cuda')
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v

    names = ['img', 'ref', 'rast', 'rast_db', 'out']
    for moved in [[k] for k in names] + [names, []]:
        t = {k: (shifted(v) if k in moved else v) for k, v in dev.items()}
        obuf = torch.full((N * H * W * 3 + 32,), 0xAA, dtype=torch.uint8, device='cuda')
        o0 = 1 if 'out' in moved else 16
        out = obuf[o0:o0 + N * H * W * 3]
        assert (out.data_ptr() % 16 != 0) == ('out' in moved)
        torch.cuda.synchronize()
        _lib.call("fpcdr_overlay_u8", t['img'].data_ptr(), 1 if kind == "float" else 0, 255.0, t['ref'].data_ptr(), t['rast'].data_ptr(),
                  t['rast_db'].data_ptr(), out.data_ptr(), N, H, W, 77, 1, float(R.hw2_of(0.5)), _rgb(GREEN), 1, None)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu().view(N, H, W, 3), torch.from_numpy(want)), (moved, _mismatch(out.cpu().view(N, H, W, 3).numpy(), want))
        assert bool((obuf[:o0] == 0xAA).all()) and bool((obuf[o0 + N * H * W * 3:] == 0xAA).all()), moved
    _unchanged(host, dev)


def test_more_images_than_one_launch_holds():
    """65 538 images of 2 x 3 with the raster inputs: two launches (gridDim.y ends at 65 535), the second one starting at image 65 535."""
    host, dev = _inputs(65538, 2, 3, "float", seed=21)
    _check(host, dev, True, True, 0.5, 'capture', GREEN, 0.5, True)
    _check(host, dev, False, False, 77 / 256, 'render', None, 0.5, False)


def test_the_rasterisers_own_output():
    """dr.rasterize of a small closed mesh (scene.make_scene's sphere, 8 x 4) seen by two cameras at 64 x 64, then the kernel on the GPU's
    own rast / rast_db: equal to the statement on the same tensors, and a picture with lines in it -- the wire share of the covered
    pixels lies strictly between 5 % and 95 %."""
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd import camera, rerender, scene
    sc = scene.make_scene(mesh=(8, 4), K=2, n_frames=1, resolution=(64, 64), texshape=(16, 16, 1))
    dev = torch.device('cuda')
    proj, t_mv = rerender._camera_matrices([sc.cams[0], sc.cams[4]], (0.0, 170.0, 0.0), dev)
    verts = torch.tensor(sc.v_base.reshape(-1, 3), device=dev)
    pos_clip = camera.transform_clip(rerender._multicam_mvp(proj, t_mv, None), verts[None]).contiguous()
    tri = torch.tensor(sc.pos_idx, dtype=torch.int32, device=dev)
    rast, rast_db = dr.rasterize(dr.RasterizeGLContext(device=dev), pos_clip, tri, resolution=(64, 64))
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(2, 64, 64), dtype=np.uint8)
    ref = rng.integers(0, 256, size=(2, 64, 64), dtype=np.uint8)
    h_rast, h_db = rast.cpu().numpy(), rast_db.cpu().numpy()
    cov = h_rast[..., 3] > 0
    for hw in (0.5, 1.0):
        for flip in (False, True):
            out = dr.overlay_images(torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda(), rast=rast, rast_db=rast_db, outside='capture',
                                    wire=GREEN, half_width=hw, flip_rows=flip)
            want = R.overlay(img, ref, h_rast, h_db, w=128, outside_capture=True, hw2=R.hw2_of(hw), wire_rgb=GREEN, flip_rows=flip)
            assert torch.equal(out.cpu(), torch.from_numpy(want)), _mismatch(out.cpu().numpy(), want)
    share = (R.wire_mask(h_rast, h_db, R.hw2_of(0.5)) & cov).sum() / cov.sum()
    print(f"covered {int(cov.sum())} of {cov.size}, wire share at half width 0.5: {share:.3f}")
    assert cov.sum() > 500 and 0.05 < share < 0.95


# ---- image sequences ---------------------------------------------------------------------------------------------------------------------
def test_overlay_sequence_is_the_reference_blend(tmp_path):
    """Ten pairs of the comparison fixture at 160 x 120, batch=4 (three uploads): the PNGs read back are
    np.clip(np.rint(ref * 0.5 + img * 0.5), 0, 255) of render_result_blended.py:149-154, in three equal channels."""
    from PIL import Image
    from fpc_diffrend_amd import rerender
    pairs = [comparison_pair(i, height=160, width=120) for i in range(10)]
    rerender.overlay_sequence([a for a, _ in pairs], [b for _, b in pairs], str(tmp_path / "ov"), batch=4)
    assert sorted(os.listdir(tmp_path / "ov")) == sorted(f"overlay_{i}.png" for i in range(10))
    for i, (img, ref) in enumerate(pairs):
        got = np.asarray(Image.open(tmp_path / "ov" / f"overlay_{i}.png"))
        want = np.clip(np.rint(ref * 0.5 + img * 0.5), 0, 255).astype(np.uint8)
        assert got.shape == (160, 120, 3) and all(np.array_equal(got[..., k], want) for k in range(3)), (i, _mismatch(got[..., 0], want))
    assert any(((a.astype(int) + b) % 2 == 1).any() for a, b in pairs)          # sums that are odd: the blend falls on a tie there


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_overlay_result_equals_the_host_path_and_the_statement(tmp_path):
    """A saved fit (cfg1, 2 frames, set up as tests/test_gpu_compare.py sets up its own), cameras 1 and 4.  wireframe=False,
    outside='render', weight 0.5: the PNGs are the reference's expression np.clip(np.rint(ref * 0.5 + img * 0.5), 0, 255) on
    render_multicam's host images of the same files, rounded as rerender_result rounds them.  wireframe=True (the defaults): the PNGs
    are the statement applied to colour, rast and rast_db rendered here with the same operators on the same batch."""
    from PIL import Image
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd import camera, fit, rerender, scene
    sc = scene.cfg('cfg1', n_frames=2)
    sc.q_gt[:] = (0.0, 0.0, 0.0, 1.0)
    cfg = fit.FitConfig(max_iter=4, lr_base=5e-3, lr_t=5e-3, lr_q=1e-5, init_texture='truth', optimize_texture=False)
    ft = fit.Fitter(sc, cfg, device='cuda')
    ft.init_near_truth(0.9)
    for _ in range(2):
        ft.step()
    ft.save(str(tmp_path))
    rdir = str(tmp_path / "result")
    H, W = sc.resolution
    cams = (1, 4)
    dev = torch.device('cuda')
    glctx = dr.RasterizeGLContext(device=dev)
    pos_idx = torch.tensor(sc.pos_idx, dtype=torch.int32, device=dev)
    uv = torch.tensor(sc.uv, dtype=torch.float32, device=dev)
    uv_idx = torch.tensor(sc.uv_idx, dtype=torch.int32, device=dev)
    tex = torch.tensor(rerender.read_texture(os.path.join(rdir, "texture.png")), dtype=torch.float32, device=dev)
    t_all, q_all = rerender.read_pose(rdir)
    host = []
    for i in range(2):
        verts = torch.tensor(rerender.read_result_obj(os.path.join(rdir, f"{i}.obj")), device=dev)
        imgs = rerender.render_multicam(glctx, verts, pos_idx, uv, uv_idx, tex, [sc.cams[c] for c in cams], sc.resolution,
                                        pose=(t_all[i], q_all[i]), modelview_offset=(0.0, 170.0, 0.0))
        host.append(np.clip(np.rint(imgs.cpu().numpy()), 0, 255).astype(np.uint8)[..., 0])
    host = np.stack(host)                                                   # [2,2,H,W] uint8, top row first
    assert host.shape == (2, 2, H, W) and (host > 50).mean() > 0.02         # something other than background was drawn
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    pattern = ((y // 8 + 2 * (x // 16)) % 7 - 3) * 4 + np.where((y // 32 + x // 64) % 5 == 0, 150, 0) - np.where((y // 16) % 9 == 0, 140, 0)
    references = np.clip(host.astype(np.int32) + pattern[None, None] + np.arange(2)[None, :, None, None], 0, 255).astype(np.uint8)

    # ---- the reference's picture ----
    rerender.overlay_result(rdir, sc, references, str(tmp_path / "blend"), cams=cams, wireframe=False, outside='render', weight=0.5,
                            batch_frames=2)
    assert sorted(os.listdir(tmp_path / "blend")) == sorted(f"overlay_{c}_{i}.png" for c in cams for i in range(2))
    for j, c in enumerate(cams):
        for i in range(2):
            got = np.asarray(Image.open(tmp_path / "blend" / f"overlay_{c}_{i}.png"))
            want = np.clip(np.rint(references[i, j] * 0.5 + host[i, j] * 0.5), 0, 255).astype(np.uint8)
            assert got.shape == (H, W, 3) and all(np.array_equal(got[..., k], want) for k in range(3)), (c, i, _mismatch(got[..., 0], want))

    # ---- with the wire: the statement on tensors rendered here, the same operators on the same batch ----
    rerender.overlay_result(rdir, sc, lambda f: references[f], str(tmp_path / "wire"), cams=cams, batch_frames=2)
    proj, t_mv = rerender._camera_matrices([sc.cams[c] for c in cams], (0.0, 170.0, 0.0), dev)
    clip = []
    for i in range(2):
        verts = torch.tensor(rerender.read_result_obj(os.path.join(rdir, f"{i}.obj")), device=dev)
        clip.append(camera.transform_clip(rerender._multicam_mvp(proj, t_mv, (t_all[i], q_all[i])), verts[None]))
    pos_clip = torch.cat(clip)
    rast, rast_db = dr.rasterize(glctx, pos_clip, pos_idx, resolution=(H, W))
    texc, _ = dr.interpolate(uv[None, ...], rast, uv_idx)
    colour = dr.antialias(dr.texture(tex[None, ...], texc, filter_mode='linear'), rast, pos_clip, pos_idx)
    colour = torch.where(rast[..., 3:] > 0, colour, torch.tensor(fit.BACKGROUND, device=dev))
    want = R.overlay(colour[..., 0].cpu().numpy(), references.reshape(4, H, W), rast.cpu().numpy(), rast_db.cpu().numpy(), w=128,
                     outside_capture=True, hw2=R.hw2_of(0.5), wire_rgb=GREEN, scale=255.0, flip_rows=True).reshape(2, 2, H, W, 3)
    green = (want == np.array(GREEN, dtype=np.uint8)).all(-1)
    assert 0.01 < green.mean() < 0.5                                          # lines were drawn, and not everywhere
    for j, c in enumerate(cams):
        for i in range(2):
            got = np.asarray(Image.open(tmp_path / "wire" / f"overlay_{c}_{i}.png"))
            assert np.array_equal(got, want[i, j]), (c, i, _mismatch(got, want[i, j]))
            # off the mesh the capture shows unchanged
            off = ~(rast[2 * i + j, :, :, 3] > 0).cpu().numpy()[::-1]
            assert np.array_equal(got[off], np.repeat(references[i, j][off][:, None], 3, axis=1))


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
def test_overlay_images_rejects_bad_input():
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd import _lib
    N, H, W = 2, 8, 12
    img = torch.zeros(N, H, W, dtype=torch.uint8, device='cuda')
    ref = torch.full((N, H, W), 10, dtype=torch.uint8, device='cuda')
    rast = torch.zeros(N, H, W, 4, device='cuda')
    rast_db = torch.zeros(N, H, W, 4, device='cuda')
    assert bool((dr.overlay_images(img, ref) == 5).all())
    assert bool((dr.overlay_images(img, ref, rast=rast, rast_db=rast_db, outside='capture', wire=GREEN) == 10).all())
    bad = [(ValueError, "no CPU path", lambda: dr.overlay_images(img.cpu(), ref)),
           (ValueError, "no CPU path", lambda: dr.overlay_images(img, ref.cpu())),
           (ValueError, "no CPU path", lambda: dr.overlay_images(img, ref, rast=rast.cpu(), outside='capture')),
           (TypeError, "torch.Tensor", lambda: dr.overlay_images(img.cpu().numpy(), ref)),
           (ValueError, "float32 or uint8", lambda: dr.overlay_images(img.double(), ref)),
           (ValueError, "float32 or uint8", lambda: dr.overlay_images(img.to(torch.int32), ref)),
           (ValueError, "ref must be uint8", lambda: dr.overlay_images(img, ref.float())),
           (ValueError, "differ in shape", lambda: dr.overlay_images(img, ref[:, :7])),
           (ValueError, r"\[N,H,W\]", lambda: dr.overlay_images(img[0], ref[0])),
           (ValueError, "one channel", lambda: dr.overlay_images(torch.zeros(N, H, W, 3, device='cuda'), ref)),
           (ValueError, "contiguous", lambda: dr.overlay_images(torch.zeros(N, H, 2 * W, dtype=torch.uint8, device='cuda')[:, :, ::2], ref)),
           (ValueError, "empty", lambda: dr.overlay_images(img[:0], ref[:0])),
           (ValueError, "rast must be float32", lambda: dr.overlay_images(img, ref, rast=rast.double(), outside='capture')),
           (ValueError, "rast_db must be", lambda: dr.overlay_images(img, ref, rast=rast, rast_db=rast_db[..., :2], wire=GREEN)),
           (ValueError, "rast must be", lambda: dr.overlay_images(img, ref, rast=rast[:1], outside='capture')),
           (ValueError, "outside must be", lambda: dr.overlay_images(img, ref, outside='mesh')),
           (ValueError, "outside='capture' needs rast", lambda: dr.overlay_images(img, ref, outside='capture')),
           (ValueError, "wire needs rast and rast_db", lambda: dr.overlay_images(img, ref, rast=rast, wire=GREEN)),
           (ValueError, "wire needs rast and rast_db", lambda: dr.overlay_images(img, ref, wire=GREEN)),
           (ValueError, "three bytes", lambda: dr.overlay_images(img, ref, rast=rast, rast_db=rast_db, wire=(0, 256, 0))),
           (ValueError, "three bytes", lambda: dr.overlay_images(img, ref, rast=rast, rast_db=rast_db, wire=(0, 255))),
           (ValueError, "half_width", lambda: dr.overlay_images(img, ref, rast=rast, rast_db=rast_db, wire=GREEN, half_width=-1.0)),
           (ValueError, "half_width", lambda: dr.overlay_images(img, ref, rast=rast, rast_db=rast_db, wire=GREEN, half_width=float('nan'))),
           (ValueError, "half_width", lambda: dr.overlay_images(img, ref, rast=rast, rast_db=rast_db, wire=GREEN, half_width=1e30)),
           (ValueError, "weight must lie", lambda: dr.overlay_images(img, ref, weight=1.01)),
           (ValueError, "weight must lie", lambda: dr.overlay_images(img, ref, weight=-0.1)),
           (ValueError, "weight must lie", lambda: dr.overlay_images(img, ref, weight=float('nan')))]
    for exc, msg, fn in bad:
        with pytest.raises(exc, match=msg):
            fn()
    # the C ABI itself: every FPCDR_REQUIRE of the entry point, by its message; none of these launches a kernel
    out = torch.full((N, H, W, 3), 0xAA, dtype=torch.uint8, device='cuda')
    p = lambda t: t.data_ptr()
    ok = dict(img=p(img), is_float=0, scale=255.0, ref=p(ref), rast=p(rast), rast_db=p(rast_db), out=p(out), n=N, H=H, W=W, weight=128,
              outside=1, hw2=0.25, rgb=_rgb(GREEN), flip=0)
    fimg = torch.zeros(N * H * W + 1, device='cuda')
    cases = [(dict(img=None), "null pointer"), (dict(ref=None), "null pointer"), (dict(out=None), "null pointer"),
             (dict(n=0), "sizes must be positive"), (dict(H=0), "sizes must be positive"), (dict(W=-1), "sizes must be positive"),
             (dict(H=1 << 30, W=64), "image too large"),
             (dict(weight=257), r"weight_256 must lie in \[0, 256\]"), (dict(weight=-1), r"weight_256 must lie in \[0, 256\]"),
             (dict(hw2=-0.25), "wire_hw2 must be finite and >= 0"), (dict(hw2=float('nan')), "wire_hw2 must be finite and >= 0"),
             (dict(hw2=float('inf')), "wire_hw2 must be finite and >= 0"),
             (dict(rast_db=None), "needs rast and rast_db"), (dict(rast=None, outside=0), "needs rast and rast_db"),
             (dict(rast=None, rast_db=None, hw2=0.0), "outside_capture needs rast"),
             (dict(rast=p(rast) + 2), "4-byte aligned"), (dict(img=p(fimg) + 1, is_float=1), "4-byte aligned"),
             (dict(rgb=1 << 24), "wire_rgb"),
             (dict(out=p(ref)), "out overlaps an input"), (dict(out=p(img)), "out overlaps an input"),
             (dict(img=p(out) + 100), "out overlaps an input"),                                        # ... partly
             (dict(out=p(rast) + 64), "out overlaps an input"), (dict(out=p(rast_db) + N * H * W * 16 - 1), "out overlaps an input")]
    for change, msg in cases:
        a = dict(ok, **change)
        with pytest.raises(RuntimeError, match="fpcdr_overlay_u8: .*" + msg):
            _lib.call("fpcdr_overlay_u8", a['img'], a['is_float'], a['scale'], a['ref'], a['rast'], a['rast_db'], a['out'], a['n'], a['H'],
                      a['W'], a['weight'], a['outside'], a['hw2'], a['rgb'], a['flip'], None)
    torch.cuda.synchronize()
    assert bool((out == 0xAA).all()) and not bool(img.any()) and bool((ref == 10).all())

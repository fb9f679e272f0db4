"""GPU: fpcdr_compare_u8 / ops.compare_images against the numpy statement of the rule (tests/compare_ref.py, itself checked in
tests/test_compare_ref.py) -- everything torch.equal / array_equal: integers, no tolerance, no excluded pixel -- and the surface built
on it: rerender.compare_sequence against the CSV the reference's own compareSequenceNumerical wrote, rerender.compare_result against
the host path on render_multicam's images of the same saved result."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import compare_ref as R
from helpers import comparison_pair

pytestmark = pytest.mark.gpu


def _mismatch(out, ref):
    d = np.asarray(out) != np.asarray(ref)
    return f"{int(d.sum())} of {d.size} entries differ, first at {tuple(np.argwhere(d)[0]) if d.any() else None}"


def _check(img, ref, mode, cols, scale, flip, want_rows=True, gpu_img=None, gpu_ref=None):
    """One call of ops.compare_images against the statement; img / ref: numpy, or already-placed GPU tensors of the same values."""
    import fpc_diffrend_amd.ops as dr
    t_img = torch.from_numpy(img).cuda() if gpu_img is None else gpu_img
    t_ref = torch.from_numpy(ref).cuda() if gpu_ref is None else gpu_ref
    heat, rows = dr.compare_images(t_img, t_ref, mode=mode, cols=cols, scale=scale, flip_rows=flip, want_rows=want_rows)
    want_heat, want_sums = R.compare(img, ref, mode or 'colour', cols, scale, flip)
    tag = f"mode {mode}, cols {cols}, flip {flip}, rows {want_rows}, {img.dtype} {img.shape}"
    if mode is None:
        assert heat is None
    else:
        assert heat.dtype == torch.uint8 and tuple(heat.shape) == img.shape + (3,)
        assert torch.equal(heat.cpu(), torch.from_numpy(want_heat)), tag + ": heat: " + _mismatch(heat.cpu().numpy(), want_heat)
    if not want_rows:
        assert rows is None
    else:
        assert rows.dtype == torch.int32 and tuple(rows.shape) == img.shape[:2]
        assert torch.equal(rows.cpu(), torch.from_numpy(want_sums)), tag + ": sums: " + _mismatch(rows.cpu().numpy(), want_sums)
    # the inputs were not written to
    assert torch.equal(t_ref.cpu(), torch.from_numpy(ref))
    assert np.array_equal(t_img.cpu().numpy().reshape(-1).view(np.uint8), img.reshape(-1).view(np.uint8))          # (bytes: NaNs too)


def _crops(W):
    """inside; clipped at both ends; col0 not a multiple of 16 (and col1 neither); empty (col0 >= W)"""
    return [(W // 4, W - W // 4), (-5, W + 9), (min(17, W - 2), W - 1), (W, W + 40)]


@pytest.mark.parametrize("kind", ["u8", "float"])
@pytest.mark.parametrize("H,W", [(48, 64), (5, 37), (3, 7)], ids=["48x64", "5x37", "3x7"])
def test_rule_grid(H, W, kind):
    """N = 3; 48 x 64: every chunk whole and aligned; 5 x 37: 16-byte accesses where a row happens to start aligned, element by element
    elsewhere, plus the tail; 3 x 7: narrower than one chunk.  uint8 images with |d| > 127 and d = 0; float images (scale 1) with exact
    ties, values below 0 and above 255, NaN and +-inf.  Both modes, flip on and off, every crop; heat only / rows only at one crop."""
    img, ref = (R.u8_pair if kind == "u8" else R.float_pair)(3, H, W, seed=H * 100 + W)
    t_img, t_ref = torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()
    scale = 1.0
    for mode in ('colour', 'grey'):
        for flip in (False, True):
            for cols in _crops(W):
                _check(img, ref, mode, cols, scale, flip, gpu_img=t_img, gpu_ref=t_ref)
            _check(img, ref, mode, _crops(W)[0], scale, flip, want_rows=False, gpu_img=t_img, gpu_ref=t_ref)
    for flip in (False, True):
        _check(img, ref, None, _crops(W)[1], scale, flip, gpu_img=t_img, gpu_ref=t_ref)
    # [N,H,W,1], as the render hands it over
    _check(img, ref, 'colour', _crops(W)[1], scale, True, gpu_img=t_img[..., None], gpu_ref=t_ref)


def test_float_scale_255_is_the_host_quantisation():
    """[0,1] images times 255: the kernel's quantisation is np.clip(np.rint(colour * 255), 0, 255) of rerender_result on the same
    float32 values, k / 510 (the products that fall on or next to a tie) among them."""
    rng = np.random.default_rng(5)
    img = rng.uniform(-0.1, 1.1, size=(2, 9, 48)).astype(np.float32)
    img.reshape(-1)[:511] = (np.arange(511, dtype=np.float32) / np.float32(510.0))
    ref = rng.integers(0, 256, size=img.shape, dtype=np.uint8)
    assert np.array_equal(R.quantise(img, 255.0), np.clip(np.rint(img * np.float32(255.0)), 0, 255).astype(np.uint8))
    for flip in (False, True):
        _check(img, ref, 'colour', (3, 40), 255.0, flip)


@pytest.mark.parametrize("kind", ["u8", "float"])
def test_unaligned_base_addresses(kind):
    """9 x 48 on tensors sliced so that the base address is not a multiple of 16: the loads go element by element (torch's own
    allocations are aligned); and, through the C ABI, a heat map and row sums written at such addresses."""
    from fpc_diffrend_amd import _lib
    N, H, W = 3, 9, 48
    img, ref = (R.u8_pair if kind == "u8" else R.float_pair)(N, H, W, seed=11)

    def shifted(a, off):
        buf = torch.zeros(a.size + 16, dtype=torch.from_numpy(a).dtype, device='cuda')
        v = buf[off:off + a.size].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v

    for oi, orf in ((1, 0), (0, 3), (1, 5)):
        t_img = shifted(img, oi) if oi else torch.from_numpy(img).cuda()
        t_ref = shifted(ref, orf) if orf else torch.from_numpy(ref).cuda()
        for flip in (False, True):
            _check(img, ref, 'colour', (5, 43), 1.0, flip, gpu_img=t_img, gpu_ref=t_ref)
    # outputs at odd addresses: 0xAA guard bytes around the heat map stay untouched
    t_img, t_ref = torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()
    hbuf = torch.full((N * H * W * 3 + 32,), 0xAA, dtype=torch.uint8, device='cuda')
    heat = hbuf[7:7 + N * H * W * 3]
    rbuf = torch.zeros(N * H + 2, dtype=torch.int32, device='cuda')
    rows = rbuf[1:1 + N * H]
    torch.cuda.synchronize()
    _lib.call("fpcdr_compare_u8", t_img.data_ptr(), 1 if kind == "float" else 0, 1.0, t_ref.data_ptr(), heat.data_ptr(), rows.data_ptr(),
              N, H, W, 5, 43, 1, 1, None)
    torch.cuda.synchronize()
    want_heat, want_sums = R.compare(img, ref, 'grey', (5, 43), 1.0, True)
    assert torch.equal(heat.cpu().view(N, H, W, 3), torch.from_numpy(want_heat))
    assert torch.equal(rows.cpu().view(N, H), torch.from_numpy(want_sums))
    assert bool((hbuf[:7] == 0xAA).all()) and bool((hbuf[7 + N * H * W * 3:] == 0xAA).all()) and int(rbuf[0]) == 0 and int(rbuf[-1]) == 0


@pytest.mark.parametrize("H,W", [(2, 4800), (300, 32), (5, 4099)], ids=["2x4800", "300x32", "5x4099"])
def test_row_sums_across_workgroup_boundaries(H, W):
    """2 x 4800: 300 chunks a row, one row spans two workgroups (two atomics meet in one sum); 300 x 32: two chunks a row, one
    workgroup spans 128 rows of its LDS table; 5 x 4099: rows that begin in the middle of a workgroup, and a one-pixel tail.
    All-255 against all-0 images: the largest sums (255 * W per row), then random ones; both input types."""
    full = np.full((2, H, W), 255, dtype=np.uint8)
    zero = np.zeros((2, H, W), dtype=np.uint8)
    for img, ref in ((full, zero), (zero, full), (np.ones((2, H, W), dtype=np.float32), zero)):
        for cols in ((0, W), (1, W - 1)):
            _check(img, ref, None, cols, 255.0, False)
    import fpc_diffrend_amd.ops as dr
    _, rows = dr.compare_images(torch.from_numpy(full).cuda(), torch.from_numpy(zero).cuda(), mode=None, cols=(0, W))
    assert torch.equal(rows.cpu(), torch.full((2, H), 255 * W, dtype=torch.int32))
    img, ref = R.u8_pair(2, H, W, seed=H + W)
    _check(img, ref, 'colour', (W // 3, W - 5), 1.0, True)
    img, ref = R.float_pair(2, H, W, seed=H + W + 1)
    _check(img, ref, 'grey', (-1, W + 1), 1.0, True)


def test_more_images_than_one_launch_holds():
    """65 537 images of 1 x 16: two launches (gridDim.y ends at 65 535), the second one starting at image 65 535."""
    img, ref = R.u8_pair(65537, 1, 16, seed=21)
    _check(img, ref, 'colour', (2, 13), 1.0, True)
    _check(img.astype(np.float32), ref, None, (0, 16), 1.0, False)


# ---- the reference's CSV -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    return [comparison_pair(i) for i in range(120)]


def test_compare_sequence_writes_the_reference_csv(pairs, tmp_path):
    """The 120 image pairs of the fixture through rerender.compare_sequence: the file is, byte for byte, the CSV the reference's own
    compareSequenceNumerical wrote for them (tests/golden/rerender_golden.json: size, hash, image means as text)."""
    from fpc_diffrend_amd import rerender
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rerender_golden.json")) as f:
        g = json.load(f)["compare"]
    assert g["images"] == 120
    means = rerender.compare_sequence([a for a, _ in pairs], [b for _, b in pairs], str(tmp_path / "cmp"), heat=False)
    assert sorted(os.listdir(tmp_path / "cmp")) == [g["file"]] == ["numerical_clip.csv"]
    text = open(tmp_path / "cmp" / g["file"]).read()
    assert len(text) == g["csv_bytes"] and hashlib.sha256(text.encode()).hexdigest() == g["csv_sha256"]
    assert [str(m) for m in means] == g["image_means"]
    assert text.split("\n")[120] == g["last_line"]


@pytest.mark.parametrize("colour", [True, False], ids=["colour", "grey"])
def test_compare_sequence_heat_maps(pairs, tmp_path, colour):
    """heat=True on three of the pairs (batch=2: two uploads): the PNGs read back are the statement's heat maps, and the CSV is the
    host path's for the same three."""
    from PIL import Image
    from fpc_diffrend_amd import rerender
    sel = [pairs[i] for i in (0, 57, 119)]
    imgs, refs = [a for a, _ in sel], [b for _, b in sel]
    means = rerender.compare_sequence(imgs, refs, str(tmp_path / "gpu"), colour=colour, batch=2)
    want = rerender.compare_sequence_numerical(imgs, refs, str(tmp_path / "host" / "numerical_clip.csv"))
    assert means == want
    assert open(tmp_path / "gpu" / "numerical_clip.csv").read() == open(tmp_path / "host" / "numerical_clip.csv").read()
    assert sorted(os.listdir(tmp_path / "gpu")) == ["colcomp_0.png", "colcomp_1.png", "colcomp_2.png", "numerical_clip.csv"]
    for k in range(3):
        got = np.asarray(Image.open(tmp_path / "gpu" / f"colcomp_{k}.png"))
        d = imgs[k].astype(np.int32) - refs[k].astype(np.int32)
        assert got.shape == (1600, 1200, 3) and np.array_equal(got, R.heat_map(d, 'colour' if colour else 'grey')), _mismatch(got, R.heat_map(d))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_compare_result_equals_the_host_path_on_the_same_result(tmp_path):
    """A saved fit (cfg1, 2 frames, as test_rerender_of_saved_result_matches_the_fit_images sets it up) compared on the GPU --
    compare_result: render, quantise, flip, difference without a float image reaching the host -- against the host path on
    render_multicam's images of the same files: np.clip(np.rint(.)), mean_abs_diff, and the statement's heat map.  The forward operators
    write with plain stores, so the rendered values are the same and everything is equal exactly."""
    from PIL import Image
    from fpc_diffrend_amd import fit, rerender, scene
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
    # host path: the nine cameras of each frame from the saved files, as rerender_result renders them, rounded as it rounds them
    dev = torch.device('cuda')
    glctx = rerender.dr.RasterizeGLContext(device=dev)
    pos_idx = torch.tensor(sc.pos_idx, dtype=torch.int32, device=dev)
    uv = torch.tensor(sc.uv, dtype=torch.float32, device=dev)
    uv_idx = torch.tensor(sc.uv_idx, dtype=torch.int32, device=dev)
    tex = torch.tensor(rerender.read_texture(os.path.join(rdir, "texture.png")), dtype=torch.float32, device=dev)
    t_all, q_all = rerender.read_pose(rdir)
    host = []
    for i in range(2):
        verts = torch.tensor(rerender.read_result_obj(os.path.join(rdir, f"{i}.obj")), device=dev)
        imgs = rerender.render_multicam(glctx, verts, pos_idx, uv, uv_idx, tex, sc.cams, sc.resolution, pose=(t_all[i], q_all[i]),
                                        modelview_offset=(0.0, 170.0, 0.0))
        host.append(np.clip(np.rint(imgs.cpu().numpy()), 0, 255).astype(np.uint8)[..., 0])
    host = np.stack(host)                                                   # [2,9,H,W] uint8, top row first
    assert host.shape == (2, 9, H, W) and (host > 50).mean() > 0.02         # something other than background was drawn
    # captures: the render perturbed by a slow pattern in both directions, past 127 in places; not symmetric under a row flip
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    pattern = ((y // 8 + 2 * (x // 16)) % 7 - 3) * 4 + np.where((y // 32 + x // 64) % 5 == 0, 150, 0) - np.where((y // 16) % 9 == 0, 140, 0)
    references = np.clip(host.astype(np.int32) + pattern[None, None] + np.arange(9)[None, :, None, None], 0, 255).astype(np.uint8)
    crop = dict(rows=(20, 231), cols=(30, 230))
    means = rerender.compare_result(rdir, sc, references, str(tmp_path / "gpu"), batch_frames=2, **crop)
    assert means.shape == (2, 9) and means.dtype == np.float64
    for c in range(9):
        want = rerender.compare_sequence_numerical(host[:, c], references[:, c], str(tmp_path / "host" / f"{c}.csv"), **crop)
        assert means[:, c].tolist() == want, (c, means[:, c], want)
        assert open(tmp_path / "gpu" / f"numerical_clip_{c}.csv").read() == open(tmp_path / "host" / f"{c}.csv").read(), c
        for i in range(2):
            got = np.asarray(Image.open(tmp_path / "gpu" / f"colcomp_{c}_{i}.png"))
            want_map = R.heat_map(host[i, c].astype(np.int32) - references[i, c].astype(np.int32), 'colour')
            assert np.array_equal(got, want_map), (c, i, _mismatch(got, want_map))
    assert len(os.listdir(tmp_path / "gpu")) == 9 + 18
    # a subset of cameras and frames, one frame a batch, references from a callable, grey, no heat maps
    sub = rerender.compare_result(rdir, sc, lambda f: references[f][[1, 4]], str(tmp_path / "sub"), cams=(1, 4), frames=[1], colour=False,
                                  heat=False, batch_frames=1, **crop)
    assert sub.shape == (1, 2) and sub[0].tolist() == means[1, [1, 4]].tolist()
    assert sorted(os.listdir(tmp_path / "sub")) == ["numerical_clip_1.csv", "numerical_clip_4.csv"]


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
def test_compare_images_rejects_bad_input():
    import fpc_diffrend_amd.ops as dr
    from fpc_diffrend_amd import _lib
    img = torch.zeros(2, 8, 12, dtype=torch.uint8, device='cuda')
    ref = torch.zeros(2, 8, 12, dtype=torch.uint8, device='cuda')
    heat, rows = dr.compare_images(img, ref)
    assert bool((heat == 255).all()) and not bool(rows.any())
    with pytest.raises(ValueError):
        dr.compare_images(img.cpu(), ref)                                      # no CPU path
    with pytest.raises(ValueError):
        dr.compare_images(img, ref.cpu())
    with pytest.raises(ValueError):
        dr.compare_images(img.double(), ref)                                   # float64
    with pytest.raises(ValueError):
        dr.compare_images(img.to(torch.int32), ref)
    with pytest.raises(ValueError):
        dr.compare_images(img, ref.float())                                    # captures are 8 bit
    with pytest.raises(ValueError):
        dr.compare_images(img, ref[:, :7])                                     # shape mismatch
    with pytest.raises(ValueError):
        dr.compare_images(img[0], ref[0])                                      # [H,W]
    with pytest.raises(ValueError):
        dr.compare_images(torch.zeros(2, 8, 12, 3, device='cuda'), ref)        # more than one channel
    with pytest.raises(ValueError):
        dr.compare_images(torch.zeros(2, 8, 24, dtype=torch.uint8, device='cuda')[:, :, ::2], ref)      # not contiguous
    with pytest.raises(ValueError):
        dr.compare_images(img, ref, mode=None, want_rows=False)                # nothing requested
    with pytest.raises(ValueError):
        dr.compare_images(img, ref, mode='heat')
    with pytest.raises(ValueError):
        dr.compare_images(img[:0], ref[:0])
    # the C ABI itself
    out = torch.empty(2, 8, 12, 3, dtype=torch.uint8, device='cuda')
    sums = torch.zeros(2, 8, dtype=torch.int32, device='cuda')
    p = lambda t: t.data_ptr()
    bad = [(p(img), 0, 1.0, p(ref), None, None, 2, 8, 12, 0, 12, 0, 0),              # nothing to compute
           (None, 0, 1.0, p(ref), p(out), p(sums), 2, 8, 12, 0, 12, 0, 0),
           (p(img), 0, 1.0, None, p(out), p(sums), 2, 8, 12, 0, 12, 0, 0),
           (p(img), 0, 1.0, p(ref), p(out), p(sums), 2, 8, 12, 0, 12, 2, 0),         # mode
           (p(img), 0, 1.0, p(ref), p(out), p(sums), 0, 8, 12, 0, 12, 0, 0),         # sizes
           (p(img), 0, 1.0, p(ref), p(out), p(sums), 2, 0, 12, 0, 12, 0, 0),
           (p(img), 0, 1.0, p(ref), p(out), p(sums), 2, 8, -1, 0, 12, 0, 0),
           (p(img), 0, 1.0, p(ref), p(ref), p(sums), 2, 8, 12, 0, 12, 0, 0),         # heat over ref
           (p(out), 0, 1.0, p(ref), p(out), p(sums), 2, 8, 12, 0, 12, 0, 0),         # heat over img
           (p(out), 0, 1.0, p(ref), p(out) + 100, None, 2, 8, 12, 0, 12, 0, 0),      # ... partly
           (p(img), 0, 1.0, p(ref), p(out), p(out) + 64, 2, 8, 12, 0, 12, 0, 0),     # row sums inside the heat map
           (p(img), 0, 1.0, p(ref), None, p(sums), 1, 1, 8421505, 0, 12, 0, 0)]      # 255 * W past int32 (checked before anything is read)
    for args in bad:
        with pytest.raises(RuntimeError, match="fpcdr_compare_u8"):
            _lib.call("fpcdr_compare_u8", *args, None)
    assert not bool(sums.any())

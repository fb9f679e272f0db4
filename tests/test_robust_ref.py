"""CPU: the float64 restatement of the weighted robust pixel loss (tests/robust_ref.py) checked against torch itself and against high
precision, the host side of the feature (masks through scene.from_take / write_take, FitConfig, the C ABI's new entry) and the highlight
scan on the CPU oracle that is the reason for the design -- no GPU.

The closed-form gradient  grad = covered ? coef * (w * psi) : 0  is the statement tests/test_gpu_robust.py judges the kernel by; here it
is compared with torch.autograd through the textbook expression of rho in float64 at every shape the GPU file uses, entry by entry: |g_i
- auto_i| <= 1e-12 S_i.  Measured here (the largest over the shapes, kinds, scales and option sets; printed as "ROBUSTREF"): 6.1e-16."""
import ctypes
import dataclasses
import decimal
import os
import re
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import robust_ref as RR  # noqa: E402
from helpers import lib_loaded  # noqa: E402

_ids = lambda s: "x".join(str(v) for v in s)


@pytest.mark.parametrize("shape", RR.SMALL_SHAPES + [RR.loop_shape()], ids=_ids)
def test_closed_form_gradient_equals_autograd(shape):
    inp = RR.inputs(*shape)
    big = shape == RR.loop_shape()
    worst = 0.0
    for kind in RR.KINDS:
        for c in ((None,) if kind == 'l2' else RR.SCALES[:1] if big else RR.SCALES):
            for opt in (RR.OPTIONS[-1:] if big else RR.OPTIONS):
                kw = RR.option_kwargs(inp, opt)
                res = RR.robust_loss(inp['colour'], inp['rast_w'], inp['ref'], kind, c, **kw)
                grad, S = res['grad']
                assert grad.dtype == torch.float64
                cd = inp['colour'].double().requires_grad_(True)
                loss = RR.loss_plain(cd, inp['rast_w'], inp['ref'], kind, c, weight=res['w'])
                loss.backward()
                # the statement scales by 255 * float32(1 / n_total), the plain expression by 255 / n_total
                n = inp['colour'].numel()
                auto = cd.grad * (float(np.float32(1.0 / n)) * n)
                z = S == 0
                assert bool((grad[z] == 0).all()) and bool((auto[z] == 0).all())
                assert int(z.sum()) == RR.predicted_zeros(inp['rast_w'], res['w'], shape[3])
                err = float(((grad - auto).abs()[~z] / S[~z]).max()) if bool((~z).any()) else 0.0
                worst = max(worst, err)
                assert err <= 1e-12, (kind, c, opt[0], err)
                # the value: the stable forms against the textbook ones, which cancel for |d| << c (2 c^2 eps64 / rho at worst)
                assert abs(float(res['loss']) - float(loss.detach())) <= 1e-9 * max(float(loss.detach()), 1e-30)
                assert bool((S >= grad.abs() * (1 - 1e-12)).all())
    print(f"ROBUSTREF closed-form-vs-autograd {shape} {worst:.2e}")


def test_shapes_mirror_the_kernels_constants_and_the_inputs_hold_every_special_value():
    src = open(os.path.join(ROOT, "fpc_diffrend_amd", "csrc", "robust.hip")).read()
    assert re.search(rf"WAVE_PX = {RR.WAVE_PX};", src) and re.search(r"BLOCK_PX = 4 \* WAVE_PX;", src) and RR.BLOCK_PX == 4 * RR.WAVE_PX
    assert re.search(rf"BLOCKS_PER_CU = {RR.BLOCKS_PER_CU};", src)
    px = {s[0] * s[1] * s[2] for s in RR.SMALL_SHAPES}
    for edge in (RR.CHUNK, RR.WAVE_PX, RR.BLOCK_PX):
        assert {edge - 1, edge, edge + 1} <= px, edge
    assert {s[3] for s in RR.SMALL_SHAPES} == {1, 3} and any(s[0] == 2 for s in RR.SMALL_SHAPES)
    Bn, H, W, C = RR.loop_shape()
    full = RR.BLOCKS_PER_CU * RR.MI355X_CUS * RR.BLOCK_PX
    assert 2 * full < Bn * H * W < 3 * full and (Bn * H * W) % RR.CHUNK != 0 and (Bn * H * W) % RR.WAVE_PX != 0
    inp = RR.inputs(2, 37, 53, 3)
    assert {0, 1, 254, 255} <= set(inp['mask'].reshape(-1).tolist())
    assert float(inp['face_w'].min()) == 0.0 and float(inp['face_w'].max()) > 1.0
    assert bool((inp['ref'] >= RR.SAT).any()) and bool((inp['ref'] == RR.SAT).any()) and bool((inp['ref'] == RR.SAT - 1).any())
    assert bool((inp['rast_w'] > 0).any()) and bool((inp['rast_w'] == 0).any())
    res = RR.robust_loss(inp['colour'], inp['rast_w'], inp['ref'], 'l2')
    d = (res['grad'][0] / (-2.0 * 255.0 * float(np.float32(1.0 / inp['colour'].numel()))))[inp['rast_w'] > 0].abs()
    for c in RR.SCALES:          # residuals far below, around and far above both scales
        assert bool((d < 0.1 * c).any()) and bool(((d > 0.5 * c) & (d < 2 * c)).any()) and bool((d > 10 * c).any()), c


def test_limits_of_the_robust_functions():
    """rho -> d^2 as c -> infinity: Charbonnier's rho / d^2 = 2 / (1 + sqrt(1 + t)) >= 1 - t / 4 and Geman-McClure's 1 / (1 + t) >= 1 - t,
    t = d^2 / c^2 -- with c = 1e6 and |d| <= 561 (a capture of 255 against a colour of 1.2) t <= 3.2e-7, and 4 eps64 for the roundings.
    Charbonnier's stable form against 2 c^2 (sqrt(1 + d^2 / c^2) - 1) in 60 decimal digits: its roundings are d * d (1), z (1), t (3),
    1 + t (4), the root (half of that, and its own: 3), 1 + h (4), the quotient (1 + 4 + 1 = 6): 8 eps64 relative, eps64 = 2^-53; the
    textbook form misses that by orders of magnitude for |d| << c, which is printed.  Geman-McClure stays below c^2: over the shared
    inputs t <= 7.9e4, so rho / c^2 = t / (1 + t) <= 1 - 1.2e-5, far from the rounding."""
    d = torch.cat([torch.linspace(-561.0, 561.0, 2001, dtype=torch.float64), torch.tensor([1e-3, 0.5, 3.0], dtype=torch.float64)])
    c = 1e6
    t = (d / c) ** 2
    for kind, slack in (('charbonnier', 0.25), ('geman_mcclure', 1.0)):
        rho, psi = RR.rho_psi(d, kind, 1.0 / c)
        assert bool(((d * d - rho) >= -4 * 2.0 ** -53 * d * d).all()) and bool(((d * d - rho) <= (slack * t + 4 * 2.0 ** -53) * d * d).all()), kind
        assert bool(((d - psi).abs() <= (2 * t + 4 * 2.0 ** -53) * d.abs()).all()), kind
    decimal.getcontext().prec = 60
    eps64 = 2.0 ** -53
    worst, worst_naive = 0.0, 0.0
    for cc in RR.SCALES:
        inv_c = RR.inv_scale(cc)
        for dv in (1e-3, 0.01, 0.37, 1.0, 2.0, 19.0, 20.0, 140.0, 561.0):
            rho = float(RR.rho_psi(torch.tensor(dv, dtype=torch.float64), 'charbonnier', inv_c)[0])
            D, IC = decimal.Decimal(dv), decimal.Decimal(inv_c)
            exact = 2 * ((1 + (D * IC) ** 2).sqrt() - 1) / (IC * IC)
            err = abs(float((decimal.Decimal(rho) - exact) / exact))
            c2 = (1.0 / inv_c) ** 2
            naive = 2.0 * c2 * (np.sqrt(1.0 + dv * dv / c2) - 1.0)
            worst, worst_naive = max(worst, err), max(worst_naive, abs(float((decimal.Decimal(naive) - exact) / exact)))
            assert err <= 8 * eps64, (cc, dv, err)
    print(f"ROBUSTREF charbonnier stable form {worst / eps64:.2f} eps64, textbook form {worst_naive / eps64:.3g} eps64")
    assert worst_naive > 100 * worst
    for shape in RR.SMALL_SHAPES[-2:]:
        inp = RR.inputs(*shape)
        for cc in RR.SCALES:
            a = 255.0 * torch.where((inp['rast_w'] > 0)[..., None], inp['colour'].double(), torch.tensor(float(np.float32(RR.BACKGROUND)), dtype=torch.float64))
            rho = RR.rho_psi(inp['ref'].double()[..., None] - a, 'geman_mcclure', RR.inv_scale(cc))[0]
            assert float(rho.max()) < (1.0 / RR.inv_scale(cc)) ** 2 * (1 - 1e-5)


def test_masks_round_trip_through_a_take_and_a_missing_file_raises():
    from fpc_diffrend_amd import scene
    sc = scene.make_scene(resolution=(24, 40), n_frames=2)
    rng = np.random.default_rng(5)
    images = rng.integers(0, 141, size=(2, 2, 24, 40)).astype(np.uint8)
    masks = rng.integers(0, 256, size=(2, 2, 24, 40)).astype(np.uint8)
    masks[0, 0, 0, :4] = (0, 1, 254, 255)
    with tempfile.TemporaryDirectory() as td:
        paths = scene.write_take(sc, td, images, cam_idxs=(0, 4), masks=masks)
        assert len(paths) == 4
        maskdir = os.path.join(td, "masks")
        assert sorted(os.listdir(maskdir)) == sorted(os.listdir(paths[3]))
        take = scene.from_take(*paths, maskdir=maskdir)
        assert take.masks.dtype == np.uint8 and np.array_equal(take.masks, masks) and np.array_equal(take.images, images)
        assert scene.from_take(*paths).masks is None
        cam = sorted(os.listdir(maskdir))[1]
        victim = os.path.join(maskdir, cam, f"{cam}_01.tif")
        os.remove(victim)
        with pytest.raises(ValueError) as ei:
            scene.from_take(*paths, maskdir=maskdir)
        assert victim in str(ei.value)
        from PIL import Image
        Image.fromarray(np.zeros((12, 40), dtype=np.uint8)).save(victim)
        with pytest.raises(ValueError) as ei:
            scene.from_take(*paths, maskdir=maskdir)
        assert victim in str(ei.value)


def test_fitconfig_has_the_robust_fields_off_by_default_and_validates_them():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert (cfg.robust, cfg.robust_scale, cfg.robust_iters, cfg.weight_outside, cfg.saturation, cfg.face_weights, cfg.use_masks) == \
        ('', None, 0, 1.0, 0, None, True)
    assert not cfg.weights_configured()
    names = [f.name for f in dataclasses.fields(fit.FitConfig)]
    assert names.index('robust') > names.index('pyramid_mip') > names.index('norm_iters')
    fit.FitConfig(robust='charbonnier', robust_scale=10.0, robust_iters=5)
    fit.FitConfig(robust='geman_mcclure', robust_scale=2)
    fit.FitConfig(robust='l2', weight_outside=0.0, saturation=140, face_weights=[1.0, 0.0])
    for bad in (dict(robust='cauchy', robust_scale=1.0), dict(robust='charbonnier'), dict(robust='geman_mcclure'),
                dict(robust='charbonnier', robust_scale=0.0), dict(robust='charbonnier', robust_scale=-1.0),
                dict(robust='charbonnier', robust_scale=float('nan')), dict(robust='charbonnier', robust_scale=float('inf')),
                dict(robust='charbonnier', robust_scale=1e-60), dict(robust='charbonnier', robust_scale=1.0, robust_iters=-1),
                dict(weight_outside=-0.5), dict(weight_outside=float('nan')), dict(weight_outside=float('inf')),
                dict(saturation=256), dict(saturation=-1), dict(saturation=1.5),
                dict(robust='charbonnier', robust_scale=5.0, blur_sigma=3.0), dict(robust='l2', norm_sigma=3.0),
                dict(saturation=140, blur_sigma=3.0), dict(weight_outside=0.0, norm_sigma=3.0), dict(face_weights=[1.0], blur_sigma=3.0)):
        with pytest.raises(ValueError):
            fit.FitConfig(**bad)
    # face weights: an array-like or a text file with one number per face, checked against the number of faces
    assert fit.load_face_weights([0.0, 1.0, 2.5], 3).dtype == np.float32
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "w.txt")
        np.savetxt(path, np.asarray([0.0, 1.0, 0.5, 2.0]))
        assert fit.load_face_weights(path, 4).tolist() == [0.0, 1.0, 0.5, 2.0]
        with pytest.raises(ValueError):
            fit.load_face_weights(path, 5)
        with pytest.raises(ValueError):
            fit.load_face_weights(os.path.join(td, "missing.txt"), 4)
    for bad in ([1.0, -0.1, 1.0], [1.0, float('nan'), 1.0], [1.0, float('inf'), 1.0], [[1.0, 1.0, 1.0]], [1.0, 1.0]):
        with pytest.raises(ValueError):
            fit.load_face_weights(bad, 3)


def test_both_libraries_export_the_robust_entry_with_abi_16_and_the_binding_mirrors_the_header():
    """(size and field offsets of the struct against the C compiler's: test_host_logic.py, for every parameter struct of the header)"""
    _lib, lib = lib_loaded()
    assert _lib.ABI_VERSION == 16 and lib.fpcdr_abi_version() == 16
    assert "fpcdr_robust_loss" in _lib.SYMBOLS
    for path in (_lib.LIB_PATH, _lib.TWOCALL_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "fpcdr_robust_loss"), path
    header = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    assert re.search(r"#define FPCDR_ABI_VERSION 16\b", header)
    assert re.search(r"int fpcdr_robust_loss\(const fpcdr_robust_loss_params \*p?, void \*stream\);", header)
    for name, number in _lib.ROBUST_KIND.items():
        assert re.search(rf"#define FPCDR_ROBUST_{name.upper()} {number}\b", header), name
    assert [f for f, _ in _lib.RobustLoss._fields_][:10] == [f for f, _ in _lib.PixelLoss._fields_][:10]      # (the style of the pixel loss's struct)


def test_bad_arguments_give_an_error_code_before_any_launch():
    """Every error of the ABI entry comes from its argument checks, ahead of the first HIP call: this runs without a GPU, on host memory
    the entry never touches.  ops rejects the same on the host, before it looks at the tensors."""
    _lib, lib = lib_loaded()
    Bn, H, W, C, T = 1, 5, 7, 1, 4
    n = Bn * H * W
    col, rast, grad, fw = ((ctypes.c_float * k)() for k in (n * C, 4 * n, n * C, T))
    ref, mask = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * n)()
    sums = (ctypes.c_double * 2)()
    vp = lambda b: ctypes.cast(b, ctypes.c_void_p)

    def params(**over):
        kw = dict(color=vp(col), rast=vp(rast), ref=vp(ref), B=Bn, H=H, W=W, C=C, bg=RR.BACKGROUND, color_scale=255.0, grad_scale=1.0,
                  kind=1, inv_c=0.1, w_outside=1.0, sat=0, mask=vp(mask), face_w=vp(fw), T=T, sums=vp(sums), grad_color=vp(grad))
        kw.update(over)
        return _lib.RobustLoss(**kw)

    bad = [params(kind=3), params(kind=-1), params(inv_c=0.0), params(inv_c=-0.1), params(inv_c=float('nan')), params(inv_c=float('inf')),
           params(kind=2, inv_c=0.0), params(w_outside=-1.0), params(w_outside=float('nan')), params(w_outside=float('inf')),
           params(sat=256), params(sat=-1), params(T=0), params(T=-3), params(color=None), params(rast=None), params(ref=None),
           params(sums=None), params(B=0), params(H=-1), params(W=0), params(C=0), params(sums=ctypes.c_void_p(vp(sums).value + 4)),
           params(color=ctypes.c_void_p(vp(col).value + 2))]
    for i, p in enumerate(bad):
        assert lib.fpcdr_robust_loss(ctypes.byref(p), None) != 0, i
        assert b"fpcdr_robust_loss" in lib.fpcdr_last_error(), i
    assert lib.fpcdr_robust_loss(None, None) != 0
    assert sums[0] == 0.0 and sums[1] == 0.0
    import fpc_diffrend_amd.ops as dr
    inp = RR.inputs(Bn, H, W, C)
    rast_t = torch.zeros(Bn, H, W, 4)
    for kw in (dict(kind='cauchy', scale=1.0), dict(kind='charbonnier', scale=None), dict(kind='charbonnier', scale=0.0),
               dict(kind='geman_mcclure', scale=-2.0), dict(kind='charbonnier', scale=float('nan')), dict(kind='charbonnier', scale=float('inf')),
               dict(kind='l2', scale=None, weight_outside=-1.0), dict(kind='l2', scale=None, weight_outside=float('nan')),
               dict(kind='l2', scale=None, saturation=300), dict(kind='l2', scale=None, saturation=2.5)):
        with pytest.raises(ValueError, match="kind|scale|weight_outside|saturation"):
            dr.robust_loss_call(inp['colour'], rast_t, inp['ref'], kw.pop('kind'), kw.pop('scale'), 1.0, **kw)
    with pytest.raises(ValueError, match="GPU tensor"):                      # no CPU fallback
        dr.robust_pixel_loss(inp['colour'], rast_t, inp['ref'], kind='charbonnier', scale=2.0)
    assert dr.robust_args('charbonnier', 20.0)[1] == RR.inv_scale(20.0)


def test_robust_kernels_have_no_private_segment_and_only_the_reductions_lds():
    """One streaming pass: no private segment, and no LDS beyond the block reduction (two sums x four waves x 4 bytes); read from the
    built object (tests/codeobj.py)."""
    import codeobj
    recs = codeobj.kernels("robust.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = set()
    for name, private, lds in recs:
        if "k_robust_loss" in name:
            seen.add(name)
            assert private == 0 and lds == 32, (name, private, lds)
    assert len(seen) == 3, seen


# ---- the highlight scan on the CPU oracle: the reason for the design -------------------------------------------------------------------
SCAN_C = 10.0


def test_highlight_scan_on_the_oracle(oracle_ops):
    """scene.make_scene(resolution=(128, 128), n_frames=1), cameras (0, 4), everything at the hidden truth; targets the oracle's own
    render, quantised; a disc of radius 6 px at grey level 140 (from_take's clip level) painted into camera 0's target at the image
    centre, over the textured face (82 +- 10 grey levels there); frame 0 moved along per_frame_t[0, 0] by d full-size pixels (1 unit =
    3.494 px).  Four pixel terms in float32: plain L2; Charbonnier and Geman-McClure with c = 10; L2 with a mask that zeroes the disc
    dilated by 2 px.  ONE scene and ONE axis: an illustration of the mechanism, not a measurement of a good c.  Measured here, value (g:
    the derivative along per_frame_t[0, 0], per unit):

        d    plain L2          Charbonnier c=10    Geman-McClure c=10   masked L2
       -2    55.173 (g -34.6)  27.559 (g -20.4)    9.109 (g -7.35)      43.427 (g -35.3)
       -1    34.097 (g -42.8)  16.535 (g -29.1)    5.827 (g -12.9)      22.263 (g -43.1)
        0    11.810 (g +0.288)  3.373 (g -0.0505)  0.351 (g -0.107)      0.017 (g -0.112)
       +1    34.186 (g +48.4)  16.564 (g +31.6)    5.824 (g +13.7)      22.309 (g +47.0)
       +2    55.543 (g +38.7)  27.645 (g +21.0)    9.107 (g +6.71)      43.397 (g +37.3)

    Without the disc the derivative at d = 0 is -0.110 (the quantisation of the targets): the highlight moves it by +0.398 under L2.
    The scan of c at d = 0, derivative (Charbonnier, Geman-McClure): c = 5 (-0.0783, -0.106), 10 (-0.0505, -0.107), 20 (+0.0035,
    -0.106), 40 (+0.0957, -0.0881).  c = 10 is the largest of the four at which the highlight moves Charbonnier's derivative by less
    than a quarter of what it does under L2; a smaller c flattens the basin further (the derivative at d = +-1 is 20 at c = 5, 30 at
    c = 10, 43 under L2)."""
    from fpc_diffrend_amd import scene
    from oracle import fit as ofit
    PX = 3.494
    sc = scene.make_scene(resolution=(128, 128), n_frames=1)

    def state(d):
        st = ofit.State(sc, cams=[0, 4])
        with torch.no_grad():
            st.M1.copy_(torch.eye(1))
            st.M2.copy_(torch.tensor(sc.weights_gt).t())
            st.per_frame_t.copy_(torch.tensor(sc.t_gt))
            st.per_frame_q.copy_(torch.tensor(sc.q_gt))
            st.per_frame_t[0, 0] += d / PX
        return st

    with torch.no_grad():
        st = state(0.0)
        pos_clip, _ = ofit.clip_positions(st, torch.arange(1))
        _, image, rast = ofit.forward_from_clip(st, pos_clip, torch.zeros(2, 128, 128, dtype=torch.uint8))
        clean = torch.round(image[..., 0] * 255.0).clamp(0, 255).to(torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(128), torch.arange(128), indexing='ij')
    r2 = (yy - 64) ** 2 + (xx - 64) ** 2
    assert bool((rast[0, ..., 3][r2 <= 64] > 0).all())                       # the dilated disc lies on the face
    assert float(clean[0][r2 <= 36].float().std()) > 5.0                     # ... over texture
    disc = clean.clone()
    disc[0][r2 <= 36] = 140
    mask = torch.ones(2, 128, 128)
    mask[0][r2 <= 64] = 0.0

    def evaluate(d, targets, columns):
        st = state(d)
        pos_clip, _ = ofit.clip_positions(st, torch.arange(1))
        _, image, rast = ofit.forward_from_clip(st, pos_clip, targets)
        out = []
        for kind, c, w in columns:
            loss = RR.loss_plain(image, rast[..., 3], targets, kind, c, weight=w)
            g, = torch.autograd.grad(loss, st.per_frame_t, retain_graph=True)
            out.append((float(loss.detach()), float(g[0, 0])))
        return out

    columns = [('l2', None, None), ('charbonnier', SCAN_C, None), ('geman_mcclure', SCAN_C, None), ('l2', None, mask)]
    names = ('plain L2', f'Charbonnier c={SCAN_C:g}', f'Geman-McClure c={SCAN_C:g}', 'masked L2')
    table = {}
    for d in (-2, -1, 0, 1, 2):
        table[d] = evaluate(float(d), disc, columns)
        print(f"ROBUSTREF scan d={d:+d}  " + "  ".join(f"{n} {l:.3f} (g {g:+.3g})" for n, (l, g) in zip(names, table[d])))
    scan = [('charbonnier', c, None) for c in (5.0, 10.0, 20.0, 40.0)] + [('geman_mcclure', c, None) for c in (5.0, 10.0, 20.0, 40.0)]
    at0 = evaluate(0.0, disc, scan)
    (l2_clean, g_clean), (l2_clean_masked, _) = evaluate(0.0, clean, [columns[0], columns[3]])
    print(f"ROBUSTREF scan without the disc: L2 {l2_clean:.4f} (g {g_clean:+.3g}), restricted to the unmasked pixels {l2_clean_masked:.6f}")
    print("ROBUSTREF scan of c at d=0  " + "  ".join(f"{k} c={c:g} g {g:+.3g}" for (k, c, _), (_, g) in zip(scan, at0)))
    for col in (1, 2, 3):
        assert table[-1][col][1] < 0 < table[1][col][1], names[col]
        assert abs(table[0][col][1]) < abs(table[0][0][1]), names[col]
    assert table[0][3][0] == l2_clean_masked

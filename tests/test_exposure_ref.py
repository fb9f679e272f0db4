"""CPU: the numpy statement of the Exposure rule (tests/exposure_ref.py) is itself checked -- its array form against a brute-force loop,
its fit against exact affine relations, its tables against the rule's consequences -- so that the bit-exact comparison of the kernels
against it (tests/test_gpu_exposure.py) means something.  Plus the product's host half (exposure.fit_gains, exposure.compose) against
the statement by array_equal, FitConfig's checks, the binding, the kernels' resource claims and the state_dict key set."""
import dataclasses
import os
import re
import types

import numpy as np
import pytest
import torch

import exposure_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fpcdr_exposure_sums", "fpcdr_apply_lut_u8")


# ---- 1. the statement against itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 255), (1, 139)])
@pytest.mark.parametrize("with_faces", [False, True])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", R.SIZES)
def test_sums_equal_the_brute_force_loop(H, W, B, C, with_mask, with_faces, lo, hi):
    colour, rast, ref, mask, face_w = R.case(B, H, W, C, seed=H * 1000 + W * 10 + B + C)
    kw = dict(mask=mask if with_mask else None, face_w=face_w if with_faces else None, lo=lo, hi=hi)
    got, want = R.sums(colour, rast, ref, **kw), R.sums_loops(colour, rast, ref, **kw)
    assert got.dtype == np.int64 and got.shape == (B, 6)
    assert np.array_equal(got, want)
    if H == 72:      # the case is not empty, and every condition takes something away
        assert got[:, 0].sum() > 0
        assert R.counted(rast, ref, None, None, 0, 255).sum() > R.counted(rast, ref, mask, None, 0, 255).sum() > \
            R.counted(rast, ref, mask, face_w, 0, 255).sum() > R.counted(rast, ref, mask, face_w, 1, 139).sum()
    pre = np.arange(B * 6, dtype=np.int64).reshape(B, 6) * 1000
    assert np.array_equal(R.sums(colour, rast, ref, into=pre, **kw), pre + want)


def test_the_interior_rule_fires_on_all_four_sides_and_not_at_the_border():
    rast = np.zeros((1, 5, 5, 4), dtype=np.float32)
    rast[..., 3] = 1.0
    ref = np.full((1, 5, 5), 100, dtype=np.uint8)
    assert R.counted(rast, ref).all()                      # fully covered: the image border asks nothing
    rast[0, 2, 2, 3] = 0.0                                 # one hole: itself and its four neighbours go, the diagonals stay
    ok = R.counted(rast, ref)[0]
    gone = {(2, 2), (1, 2), (3, 2), (2, 1), (2, 3)}
    assert {(y, x) for y in range(5) for x in range(5) if not ok[y, x]} == gone
    rast[0, 2, 2, 3] = np.nan                              # a NaN is not covered
    assert np.array_equal(R.counted(rast, ref)[0], ok)


def test_quantise_is_the_comparison_rule():
    v = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, -1.0, 2.0, np.nan, np.inf, -np.inf, 1.0, 0.0], dtype=np.float32)
    x = v * np.float32(255.0)
    want = [int(np.rint(x[0])), int(np.rint(x[1])), int(np.rint(x[2])), 0, 255, 0, 255, 0, 255, 0]
    assert R.quantise(v).tolist() == want


def _affine_sums(r, t):
    r, t = np.asarray(r, dtype=object), np.asarray(t, dtype=object)
    return [len(r), int(r.sum()), int(t.sum()), int((r * r).sum()), int((t * t).sum()), int((r * t).sum())]


def test_fit_recovers_an_exact_affine_relation():
    """t = a r + b exactly, in integers: a rational (3/4, 5/4; offsets 8 and 2) for both methods, and Vt / Vr a perfect square (a = 2,
    a = 1/2) -- within 1e-12, where every step of the rule rounds at 2^-53."""
    r = np.arange(0, 201, 4)
    for num, den, off in ((3, 4, 8), (5, 4, 2), (2, 1, 5), (1, 2, 30)):
        t = num * r // den + off
        assert np.array_equal(t * den, num * r + off * den)
        S = np.array([_affine_sums(r, t)], dtype=np.int64)
        for method in ('regression', 'moments'):
            out = R.fit_gains(S, method=method)
            assert out['usable'][0]
            assert abs(out['a'][0] - num / den) <= 1e-12 and abs(out['b'][0] - off) <= 1e-12 and abs(out['rho'][0] - 1.0) <= 1e-12
            assert out['g'][0] == 1.0 and np.array_equal(out['lut'], R.IDENTITY(1))      # one camera is its own common level


def _noisy_sums(seed, gains=((0.75, 8.0), (1.25, -6.0), (1.0, 0.0)), sigma=2.0, n=5000):
    rng = np.random.default_rng(seed)
    rows = []
    for a, b in gains:
        r = rng.integers(0, 141, size=n)
        t = np.clip(np.rint(a * r + b + sigma * rng.standard_normal(n)), 0, 255).astype(np.int64)
        rows.append(_affine_sums(r, t))
    return np.array(rows, dtype=np.int64)


def test_equal_cameras_give_identity_tables():
    rng = np.random.default_rng(5)
    r = rng.integers(0, 141, size=4000)
    t = np.clip(np.rint(0.9 * r + 11 + rng.standard_normal(4000)), 0, 255).astype(np.int64)
    S = np.array([_affine_sums(r, t)] * 3, dtype=np.int64)
    for method in ('regression', 'moments'):
        out = R.fit_gains(S, method=method)
        assert out['usable'].all() and np.abs(out['g'] - 1.0).max() <= 4e-16      # (the mean of three equal numbers may round)
        assert np.array_equal(out['lut'], R.IDENTITY(3))


@pytest.mark.parametrize("method", ['regression', 'moments'])
def test_an_anchor_cameras_table_is_the_identity(method):
    S = _noisy_sums(11)
    for k in range(3):
        out = R.fit_gains(S, method=method, anchor=k)
        assert np.array_equal(out['lut'][k], np.arange(256)) and out['g'][k] == 1.0
        assert all(not np.array_equal(out['lut'][c], np.arange(256)) for c in range(3) if c != k)


def test_cameras_that_cannot_be_fitted_get_the_identity():
    S = _noisy_sums(3)
    r = np.arange(0, 100)
    bad = {"negative correlation": _affine_sums(r, 200 - r), "no correlation": _affine_sums([1, 2, 1, 2], [1, 1, 2, 2]),
           "one sample": [1, 50, 60, 2500, 3600, 3000], "no sample": [0] * 6, "flat render": _affine_sums([7] * 50, list(range(50))),
           "flat capture": _affine_sums(list(range(50)), [9] * 50)}
    for why, row in bad.items():
        T = np.vstack([S, np.array([row], dtype=np.int64)])
        out = R.fit_gains(T)
        assert not out['usable'][3] and np.array_equal(out['lut'][3], np.arange(256)), why
        assert out['usable'][:3].all(), why
        assert np.array_equal(out['lut'][:3], R.fit_gains(S)['lut']), why      # ... and does not enter the means
        with pytest.raises(ValueError):
            R.fit_gains(T, anchor=3)
    # a gain ratio beyond max_gain: skipped, the means are not formed again
    far = _affine_sums(r, 2 * r)      # a = 2 against cameras near 1
    T = np.vstack([S, np.array([far], dtype=np.int64)])
    out = R.fit_gains(T, max_gain=1.5, anchor=2)      # (against camera 2, a = 1: g = 1.33, 0.8, 1, 0.5)
    full = R.fit_gains(T, max_gain=4.0, anchor=2)
    assert full['usable'].all() and not np.array_equal(full['lut'][3], np.arange(256))
    assert out['g'][3] == full['g'][3] and out['g'][3] < 1 / 1.5
    assert not out['usable'][3] and np.array_equal(out['lut'][3], np.arange(256))
    assert np.array_equal(out['lut'][:3], full['lut'][:3])


@pytest.mark.parametrize("method", ['regression', 'moments'])
def test_keep_from_leaves_the_saturated_bytes_alone(method):
    out = R.fit_gains(_noisy_sums(8), method=method, keep_from=140)
    lut = out['lut'].astype(int)
    assert out['usable'].all()
    assert np.array_equal(lut[:, 140:], np.tile(np.arange(140, 256), (3, 1)))
    assert lut[:, :140].max() == 139                   # (camera 0 is brightened: its top bytes pile up at 139, none becomes 140)
    free = R.fit_gains(_noisy_sums(8), method=method)['lut'].astype(int)
    assert free[0, :140].max() > 139 and np.array_equal(np.minimum(free[:, :140], 139), lut[:, :140])


def test_composition_is_application_in_turn():
    l1 = R.fit_gains(_noisy_sums(1))['lut']
    l2 = R.fit_gains(_noisy_sums(2, gains=((1.1, -3.0), (0.9, 4.0), (1.3, 0.0))), method='moments')['lut']
    total = R.compose(R.compose(R.IDENTITY(3), l1), l2)
    images = np.tile(np.arange(256, dtype=np.uint8), (6, 2)).reshape(6, 2, 256)      # every byte, twice, in six images
    cams = np.array([0, 1, 2, 2, 1, 0])
    assert np.array_equal(R.apply(images, total, cams), R.apply(R.apply(images, l1, cams), l2, cams))
    assert np.array_equal(R.compose(R.IDENTITY(3), l1), l1) and np.array_equal(R.compose(l1, R.IDENTITY(3)), l1)
    assert np.array_equal(R.apply(images, l1, np.array([0, 3, -1, 2, 1, 0]))[1:3], images[1:3])      # outside the table: untouched


# ---- 2. the product's host half against the statement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("anchor", [None, 0, 2])
@pytest.mark.parametrize("method", ['regression', 'moments'])
def test_product_fit_gains_equals_the_statement(method, anchor):
    from fpc_diffrend_amd import exposure
    for seed in range(6):
        S = _noisy_sums(100 + seed, sigma=float(seed))
        if seed == 5:
            S[1] = (1, 50, 60, 2500, 3600, 3000)           # an unusable camera among them
        for keep_from, max_gain in ((256, 4.0), (140, 4.0), (256, 1.2)):
            want = R.fit_gains(S, method=method, anchor=anchor, max_gain=max_gain, keep_from=keep_from)
            got = exposure.fit_gains(S, method=method, anchor=anchor, max_gain=max_gain, keep_from=keep_from)
            assert got['lut'].dtype == np.uint8 and np.array_equal(got['lut'], want['lut'])
            assert np.array_equal(got['usable'], want['usable'])
            for key in ('a', 'b', 'rho', 'g'):
                assert got[key].dtype == np.float64 and np.array_equal(got[key], want[key], equal_nan=True), key
            assert np.array_equal(got['n'], S[:, 0].astype(np.float64))
            assert np.array_equal(exposure.fit_gains(torch.from_numpy(S), method=method, anchor=anchor, max_gain=max_gain,
                                                     keep_from=keep_from)['lut'], want['lut'])
    l1, l2 = R.fit_gains(_noisy_sums(1))['lut'], R.fit_gains(_noisy_sums(2), method='moments')['lut']
    assert np.array_equal(exposure.compose(l1, l2), R.compose(l1, l2))
    assert exposure.is_identity(R.IDENTITY(4)) and not exposure.is_identity(l1)


def test_product_fit_gains_rejects_bad_arguments():
    from fpc_diffrend_amd import exposure
    S = _noisy_sums(1)
    for kw in (dict(method='median'), dict(max_gain=1.0), dict(max_gain=float('nan')), dict(keep_from=0), dict(keep_from=257),
               dict(keep_from=1.5), dict(anchor=3), dict(anchor=-1)):
        with pytest.raises(ValueError):
            exposure.fit_gains(S, **kw)
    with pytest.raises(ValueError):
        exposure.fit_gains(S.astype(np.float64))
    with pytest.raises(ValueError):
        exposure.fit_gains(S[:, :5])
    T = S.copy()
    T[0] = 0
    with pytest.raises(ValueError, match="not usable"):
        exposure.fit_gains(T, anchor=0)
    with pytest.raises(ValueError):
        exposure.compose(R.IDENTITY(2), R.IDENTITY(3))


def test_fitconfig_has_the_exposure_fields_off_by_default_and_checks_them():
    from fpc_diffrend_amd import fit
    cfg = fit.FitConfig()
    assert (tuple(cfg.equalise_exposure_at), cfg.equalise_method, cfg.equalise_anchor_camera, cfg.equalise_max_gain) == ((), 'regression', None, 4.0)
    assert fit.fit_gains is not None and fit.compose is not None and fit.check_exposure_options is not None
    fit.FitConfig(equalise_exposure_at=(0, 300), equalise_method='moments', equalise_anchor_camera=4, cam_idxs=(0, 4), equalise_max_gain=2)
    for kw in (dict(equalise_exposure_at=(-1,)), dict(equalise_exposure_at=(1.5,)), dict(equalise_exposure_at=(True,)),
               dict(equalise_exposure_at=5), dict(equalise_method='median'), dict(equalise_anchor_camera=3, cam_idxs=(0, 4)),
               dict(equalise_anchor_camera=0.0), dict(equalise_max_gain=1.0), dict(equalise_max_gain=0.5),
               dict(equalise_max_gain=float('inf')), dict(equalise_max_gain=None)):
        with pytest.raises(ValueError, match="equalise"):
            fit.FitConfig(**kw)
    names = [f.name for f in dataclasses.fields(fit.FitConfig)]
    assert {'equalise_exposure_at', 'equalise_method', 'equalise_anchor_camera', 'equalise_max_gain'} <= set(names)


# ---- 3. the binding ------------------------------------------------------------------------------------------------------------------------
def test_binding():
    """The two entries are declared in the header, bound in _lib.SYMBOLS and exported by the built library; pure additions: the ABI
    version stays 16."""
    from fpc_diffrend_amd import _lib
    header = open(os.path.join(ROOT, "include", "fpcdr.h")).read()
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == lib.fpcdr_abi_version() == 16
    assert re.search(r"#define FPCDR_ABI_VERSION 16\b", header)


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """The entries check their arguments on the host, so the rejections need no GPU (made-up addresses, never dereferenced)."""
    from fpc_diffrend_amd import _lib
    col, rast, ref, msk, fw, sums = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    ok = dict(colour=col, rast=rast, ref=ref, mask=msk, face_w=fw, T=10, lo=1, hi=254, n=2, H=8, W=8, C=3, sums=sums)
    order = ('colour', 'rast', 'ref', 'mask', 'face_w', 'T', 'lo', 'hi', 'n', 'H', 'W', 'C', 'sums')
    for change, why in ((dict(colour=None), "null"), (dict(sums=None), "null"), (dict(n=0), "positive"), (dict(W=0), "positive"),
                        (dict(C=0), "1..4"), (dict(C=5), "1..4"), (dict(lo=-1), "lo <= hi"), (dict(hi=256), "lo <= hi"),
                        (dict(lo=9, hi=8), "lo <= hi"), (dict(T=0), "T > 0"), (dict(sums=sums + 4), "8-byte"), (dict(colour=col + 2), "4-byte"),
                        (dict(sums=ref), "overlaps"), (dict(sums=col + 8), "overlaps"), (dict(sums=msk + 120), "overlaps")):
        args = dict(ok, **change)
        with pytest.raises(RuntimeError, match=NAMES[0] + ".*" + why):
            _lib.call(NAMES[0], *[args[k] for k in order], None)
    img, lut, cam = 0x100000, 0x200000, 0x300000
    for args, why in (((None, lut, cam, 2, 3, 64), "null"), ((img, None, cam, 2, 3, 64), "null"), ((img, lut, None, 2, 3, 64), "null"),
                      ((img, lut, cam, 0, 3, 64), "positive"), ((img, lut, cam, 2, 3, 0), "positive"), ((img, lut, cam, 2, -1, 64), "negative"),
                      ((img, img + 100, cam, 2, 3, 64), "overlaps"), ((img, lut, img + 8, 2, 3, 64), "overlaps"),
                      ((img, lut, cam + 2, 2, 3, 64), "4-byte")):
        with pytest.raises(RuntimeError, match=NAMES[1] + ".*" + why):
            _lib.call(NAMES[1], *args, None)
    _lib.call(NAMES[1], None, None, None, 1, 0, 64, None)                      # no image: success, nothing launched


def test_ops_have_no_cpu_path():
    from fpc_diffrend_amd import ops
    c, r, t = torch.zeros(1, 4, 4, 1), torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.exposure_sums(c, r, t)
    with pytest.raises(TypeError):
        ops.exposure_sums(c.numpy(), r, t)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.apply_lut_u8(t, torch.zeros(1, 256, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError):
        ops.apply_lut_u8(t.numpy(), torch.zeros(1, 256, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))


def test_exposure_kernels_have_no_private_segment():
    """every instance of k_exposure_sums (one per channel count) and k_apply_lut_u8 keeps its chunk in registers; LDS:
    the 4 x 6 partial sums of the waves, and one camera's 256-byte table.  Read from the built object (tests/codeobj.py)."""
    import codeobj
    recs = codeobj.kernels("exposure.o")
    if recs is None:
        pytest.skip("no built objects / llvm tools")
    seen = {}
    for name, private, lds in recs:
        assert private == 0, name
        seen[name] = lds
    assert sorted(seen.values()) == [96, 96, 96, 96, 256], seen
    assert sum("k_exposure_sums" in n for n in seen) == 4 and sum("k_apply_lut_u8" in n for n in seen) == 1


# ---- 4. the checkpoint's key set -----------------------------------------------------------------------------------------------------------
KEYS = {"params", "requires_grad", "optimizer", "scheduler", "iteration", "rng", "skipped_steps", "skipped_per_tensor", "result",
        "frame_range", "config", "tex_anchor", "tex_anchor_weights"}


def _fitter_stub():
    """What Fitter.state_dict reads, on the CPU: ten parameters, their Adam and schedule, the counters."""
    from fpc_diffrend_amd import fit
    params = [torch.zeros(2, requires_grad=True) for _ in range(10)]
    opt = torch.optim.Adam(params, lr=1e-3)
    st = types.SimpleNamespace(params=params, optimizer=opt, scheduler=torch.optim.lr_scheduler.LambdaLR(opt, lambda x: 1.0), iteration=0,
                               rng=np.random.default_rng(0), skipped_steps=0, skipped_steps_per_tensor=lambda: [0] * 10,
                               result=torch.zeros(1, 3), frame_lo=0, frame_hi=1, cfg=fit.FitConfig(), _tex_anchor=None, _tex_anchor_w=None,
                               _exposure_total=None)
    return fit, st


def test_a_default_state_dict_has_the_keys_it_had():
    fit, st = _fitter_stub()
    assert set(fit.Fitter.state_dict(st)) == KEYS
    st._exposure_total = R.fit_gains(_noisy_sums(1))['lut']
    sd = fit.Fitter.state_dict(st)
    assert set(sd) == KEYS | {"exposure_lut"}
    assert sd["exposure_lut"].dtype == torch.uint8 and np.array_equal(sd["exposure_lut"].numpy(), st._exposure_total)

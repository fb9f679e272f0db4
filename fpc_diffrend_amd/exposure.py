"""
Per-camera exposure against the fit's own render ("Exposure rule"; device code csrc/exposure.hip): the host half of the rule
-- gains, offsets and 256-entry tables from the integer sums of ops.exposure_sums (fit_gains), the composition of tables (compose) -- and
the checks of FitConfig's options.  Pure numpy and Python integers: nothing here needs a GPU.  fit.py imports these names:
fit.fit_gains, fit.compose, ... are the documented spelling.
"""
import math

import numpy as np

METHODS = ('regression', 'moments')


def identity_lut(n_cameras):
    """uint8 [Nc,256]: every camera's table maps every byte to itself."""
    return np.tile(np.arange(256, dtype=np.uint8), (int(n_cameras), 1))


def _int_rows(sums):
    if hasattr(sums, 'detach'):      # a torch tensor, wherever it lives
        sums = sums.detach().cpu().numpy()
    s = np.asarray(sums)
    if s.ndim != 2 or s.shape[1] != 6 or s.dtype.kind not in 'iu':
        raise ValueError(f"sums must be an integer array [Nc,6] (got {s.dtype} {tuple(s.shape)})")
    return [[int(v) for v in row] for row in s]


def fit_gains(sums, method='regression', anchor=None, max_gain=4.0, keep_from=256):
    """Gains, offsets and tables of the Exposure rule from the per-camera sums [Nc,6] = (n, sum r, sum t, sum r^2, sum t^2, sum r t), t
    the capture byte and r the render byte (ops.exposure_sums, summed over a camera's images and over the ranks).

      method     'regression': a = Cv / Vr, the least-squares slope of t on r (sensor noise does not bias it; misregistration attenuates
                 it, and on the oracle's checkered scene NOT alike in every camera: DESIGN.md 3, the table of the Exposure rule)
                 | 'moments': a = sqrt(Vt / Vr) (immune to misregistration, biased upwards by noise).  Judge by 'rho'
      anchor     a camera (row of sums) whose fit is the common level and whose table is the identity; it must be usable (ValueError).
                 None: the arithmetic means of a and b over the usable cameras
      max_gain   > 1: a camera whose g = a_common / a lies outside [1 / max_gain, max_gain] is skipped (identity, usable = False); the
                 means are not formed again
      keep_from  1..256: bytes >= keep_from stay as they are, and no byte below becomes one (a take's saturation value)

    With Vr = n sum r^2 - (sum r)^2, Vt likewise and Cv = n sum r t - sum r sum t as Python integers, a camera is usable iff n >= 2 and
    Vr, Vt, Cv > 0.  Every float64 below is ONE rounded operation, in this order: a = Cv / Vr (the exact quotient rounded once) or
    sqrt(Vt / Vr); b = (float(sum t) - a * float(sum r)) / float(n); rho = float(Cv) / sqrt(float(Vr * Vt)); the means add in camera order
    from 0.0 and divide by the count; g = a_common / a; lut[v] = min(clip(floor(((v - b) * g + b_common) + 0.5), 0, 255), keep_from - 1) for
    v < keep_from, v otherwise.

    Returns {'a', 'b', 'rho', 'g', 'n': float64 [Nc] (NaN where a camera's sums define none), 'usable': bool [Nc], 'lut': uint8 [Nc,256],
    'a_common', 'b_common': the common level (NaN without a usable camera)}."""
    if method not in METHODS:
        raise ValueError(f"method must be 'regression' or 'moments' (got {method!r})")
    if isinstance(max_gain, bool) or not (float(max_gain) > 1.0 and math.isfinite(float(max_gain))):
        raise ValueError(f"max_gain must be finite and > 1 (got {max_gain!r})")
    if isinstance(keep_from, bool) or int(keep_from) != keep_from or not 1 <= int(keep_from) <= 256:
        raise ValueError(f"keep_from must be an integer in 1..256 (got {keep_from!r})")
    max_gain, keep_from = float(max_gain), int(keep_from)
    rows = _int_rows(sums)
    Nc = len(rows)
    a, b, rho, g = (np.full(Nc, np.nan) for _ in range(4))
    n = np.zeros(Nc)
    usable = np.zeros(Nc, dtype=bool)
    for c, (cn, Sr, St, Srr, Stt, Srt) in enumerate(rows):
        n[c] = float(cn)
        Vr, Vt, Cv = cn * Srr - Sr * Sr, cn * Stt - St * St, cn * Srt - Sr * St
        if cn < 2 or Vr <= 0 or Vt <= 0:
            continue
        rho[c] = float(Cv) / math.sqrt(float(Vr * Vt))
        if Cv <= 0:
            continue
        a[c] = Cv / Vr if method == 'regression' else math.sqrt(Vt / Vr)
        b[c] = (float(St) - a[c] * float(Sr)) / float(cn)
        usable[c] = True
    lut = identity_lut(Nc)
    if anchor is not None:
        if isinstance(anchor, bool) or int(anchor) != anchor or not 0 <= int(anchor) < Nc:
            raise ValueError(f"anchor must be a camera in 0..{Nc - 1} (got {anchor!r})")
        if not usable[int(anchor)]:
            raise ValueError(f"the anchor camera {int(anchor)} is not usable (n = {rows[int(anchor)][0]}, rho = {rho[int(anchor)]})")
        a_bar, b_bar = float(a[int(anchor)]), float(b[int(anchor)])
    else:
        sa, sb, k = 0.0, 0.0, 0
        for c in range(Nc):
            if usable[c]:
                sa, sb, k = sa + float(a[c]), sb + float(b[c]), k + 1
        if k == 0:
            return {'a': a, 'b': b, 'rho': rho, 'g': g, 'n': n, 'usable': usable, 'lut': lut, 'a_common': math.nan, 'b_common': math.nan}
        a_bar, b_bar = sa / float(k), sb / float(k)
    v = np.arange(256, dtype=np.float64)
    for c in range(Nc):
        if not usable[c]:
            continue
        g[c] = a_bar / float(a[c])
        if not (1.0 / max_gain <= g[c] <= max_gain):
            usable[c] = False
            continue
        mapped = np.minimum(np.clip(np.floor(((v - b[c]) * g[c] + b_bar) + 0.5), 0.0, 255.0), float(keep_from - 1))
        lut[c, :keep_from] = mapped[:keep_from].astype(np.uint8)
    return {'a': a, 'b': b, 'rho': rho, 'g': g, 'n': n, 'usable': usable, 'lut': lut, 'a_common': a_bar, 'b_common': b_bar}


def _check_lut(name, t):
    t = np.asarray(t)
    if t.dtype != np.uint8 or t.ndim != 2 or t.shape[1] != 256:
        raise ValueError(f"{name} must be uint8 [Nc,256] (got {t.dtype} {tuple(t.shape)})")
    return t


def compose(total, lut):
    """The table of `total` followed by `lut`, per camera: out[c, v] = lut[c, total[c, v]].  Applying `total` and then `lut` to a
    camera's captures equals applying the result once; the composite of every table a Fitter has applied is the complete record of what
    was done to its captures."""
    total, lut = _check_lut('total', total), _check_lut('lut', lut)
    if total.shape != lut.shape:
        raise ValueError(f"total and lut must have one shape (got {tuple(total.shape)} and {tuple(lut.shape)})")
    return np.take_along_axis(lut, total.astype(np.int64), axis=1)


def is_identity(lut):
    lut = _check_lut('lut', lut)
    return bool(np.array_equal(lut, identity_lut(lut.shape[0])))


def check_exposure_options(cfg):
    """What FitConfig's exposure fields ask (FitConfig.__post_init__), or ValueError.  Needs no GPU."""
    try:
        its = tuple(cfg.equalise_exposure_at)
    except TypeError:
        raise ValueError(f"FitConfig.equalise_exposure_at must be a sequence of iterations (got {cfg.equalise_exposure_at!r})")
    for i in its:
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or i < 0:
            raise ValueError(f"FitConfig.equalise_exposure_at holds integers >= 0 (got {i!r})")
    if cfg.equalise_method not in METHODS:
        raise ValueError(f"FitConfig.equalise_method must be 'regression' or 'moments' (got {cfg.equalise_method!r})")
    k = cfg.equalise_anchor_camera
    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or int(k) not in [int(c) for c in cfg.cam_idxs]):
        raise ValueError(f"FitConfig.equalise_anchor_camera must be one of cam_idxs {tuple(cfg.cam_idxs)} (got {k!r})")
    g = cfg.equalise_max_gain
    try:
        ok = not isinstance(g, bool) and float(g) > 1.0 and math.isfinite(float(g))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"FitConfig.equalise_max_gain must be finite and > 1 (got {g!r})")

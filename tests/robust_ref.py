"""float64 restatement on the CPU of the weighted robust pixel loss (csrc/robust.hip; DESIGN.md 3, "Robust loss rule"): the yardstick of
tests/test_gpu_robust.py, itself checked on the CPU by tests/test_robust_ref.py.  Nothing here imports fpc_diffrend_amd.

The conventions are those of tests/fitstep_ref.py: every function evaluates in `dtype` (float64 by default; float32 gives "the same
formula in float32 by torch", the yardstick e32 of the long sums) and returns, besides each value, a scale S; fitstep_ref.measure()
compares against them in units of u = 2^-24.

The statement, operation by operation (the numbers the kernel is HANDED are float32 and enter as they are: bg, gs = float32(1 / n_total),
inv_c = float32(1 / c), the constant float32(1 / 255), w_outside, the face weights):
    covered = rast.w > 0
    a   = 255 * (covered ? colour : bg)                                                                            n = 1
    d   = ref - a                                       S_d = ref + |a|                                            n = 2
    z   = d * inv_c,  t = z * z
    L2:             rho = d * d,                          s = 1
    CHARBONNIER:    h = sqrt(1 + t),  rho = (2 (d * d)) / (1 + h),  s = 1 / h
    GEMAN_MCCLURE:  k = 1 + t,        rho = (d * d) / k,            s = 1 / (k * k)
    psi = d * s                                         S_psi = S_d
    wm  = mask given ? mask * float32(1 / 255) : 1;     wm = 0 where sat > 0 and ref >= sat                        n = 1
    w   = covered ? wm * (face_w given ? (0 <= id - 1 < T ? face_w[id - 1] : 0) : 1) : wm * w_outside              n = 2
    sums = (sum w * rho, sum w)                         S = (sum w * S_d^2, sum w): every term is positive
    grad = covered ? coef * (w * psi) : 0,  coef = -2 * 255 * gs                S = 2 * 255 * gs * w * S_d, 0 where uncovered
S is carried to first order through the quotient and the root as tests/norm_ref.py does, and it collapses: s <= 1 and |d psi / d d| <= 1
for every kind (L2: 1; Charbonnier: psi' = (1 + t)^(-3/2); Geman-McClure: psi' = (1 - 3 t) / (1 + t)^3, between -1/4 and 1), so
the error d carries (n = 2, of S_d) reaches psi at most as it is, and every rounding of the chain behind it is relative to |psi| <= |d|
<= S_d: S_psi is S_d.  Likewise rho <= d^2 and |rho'| <= 2 |d|: S_rho = S_d^2.  An entry whose weight is 0 (a mask byte of 0, a face
weight of 0, a saturated capture pixel, an id past the table) or that is uncovered has S = 0 and must be exactly 0.

Rounded operations that reach one entry of the gradient, n, by the rules of fitstep_ref (an input 0; a product n_a + n_b + 1; a sum of k
terms max n_i + (k - 1); a product with 2 is exact), PIXEL_N_GRAD's way.  Common: d 2; w 2; coef 2 (gs 1, its product with -2 * 255 2).
    L2:             psi = d: 2.                                                                w * psi 2 + 2 + 1 = 5, coef * that 8
    CHARBONNIER:    the chain behind d: z 1, t = z * z 3, 1 + t 4, the root 5 (it halves what it is handed: not used), s = 1 / h 6,
                    psi = d * s 7; with d's own 2: 9.                                          w * psi 9 + 2 + 1 = 12, coef * that 15
    GEMAN_MCCLURE:  z 1, t 3, k = 1 + t 4, k * k 9, s = 1 / (k * k) 10, psi = d * s 11; with d's own 2: 13.
                                                                                               w * psi 13 + 2 + 1 = 16, coef * that 19
The entry's error is then at most (n + 2) u of S."""
import numpy as np
import torch

from fitstep_ref import U, measure, rel_l2      # noqa: F401  (re-exported: the conventions of the fit step's yardstick)

BACKGROUND = 45.0 / 255.0
KINDS = ('l2', 'charbonnier', 'geman_mcclure')
N_GRAD = {'l2': 8, 'charbonnier': 15, 'geman_mcclure': 19}
SCALES = (2.0, 20.0)                  # c in grey levels: residuals of the inputs lie far below, around and far above both

# the kernel's constants (csrc/robust.hip), mirrored: a wave takes WAVE_PX pixels a trip in 16-pixel chunks, a workgroup BLOCK_PX, and the
# grid is min(ceil(pixels / BLOCK_PX), BLOCKS_PER_CU * compute units)
CHUNK = 16
WAVE_PX = 256
BLOCK_PX = 1024
BLOCKS_PER_CU = 6
MI355X_CUS = 256

# (B, H, W, C): pixel counts one below, at and one above a chunk and a workgroup's trip, a wave's trip, C = 1 and 3, B = 2
SMALL_SHAPES = [(1, 1, CHUNK - 1, 1), (1, 1, CHUNK, 3), (1, 1, CHUNK + 1, 1),
                (1, 3, 85, 3), (1, 16, 16, 1), (1, 1, WAVE_PX + 1, 1),                       # 255, 256, 257 pixels
                (1, 3, 341, 1), (2, 16, 32, 1), (1, 25, 41, 3),                              # 1023, 1024, 1025 pixels
                (2, 37, 53, 3)]


def loop_shape(n_cu=MI355X_CUS):
    """A shape whose pixel count gives every lane of the full grid at least two trips and a ragged third one: B = 2, C = 1."""
    need = 2 * BLOCKS_PER_CU * n_cu * BLOCK_PX + 3 * WAVE_PX + 2 * CHUNK + 5
    W = 1021
    H = (need + 2 * W - 1) // (2 * W)
    return (2, H, W, 1)


def inv_scale(c):
    """float32(1 / c) as a Python float: the number the host forms, hands to the kernel and uses in the statement."""
    return float(np.float32(1.0 / float(c)))


def inputs(Bn, H, W, C, seed=2, T=37):
    """colour in [0, 1.2], rast.w = triangle id + 1 (0 where uncovered, about a third of the pixels), captures over 0..255, mask bytes
    that include 0, 1, 254 and 255, face weights that include 0 and values above 1 -- and, at the first pixels of the buffer, one of
    each special value whatever the shape: residuals |d| << c, about c and >> c for c = 2 and 20, an id above the table."""
    g = torch.Generator().manual_seed(seed)
    n = Bn * H * W
    colour = torch.rand(Bn, H, W, C, generator=g) * 1.2
    ids = torch.randint(1, T + 1, (n,), generator=g).float()
    ids[torch.rand(n, generator=g) < 0.35] = 0.0
    ref = torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
    # a third of the captures close to the render: small residuals
    near = torch.rand(n, generator=g) < 0.4
    base = torch.where(ids > 0, colour.reshape(n, C)[:, 0] * 255.0, torch.tensor(45.0))
    close = (base + torch.randn(n, generator=g) * 2.0).round().clamp(0, 255).to(torch.uint8)
    ref = torch.where(near, close, ref)
    mask = torch.randint(0, 256, (n,), generator=g).to(torch.uint8)
    pick = torch.rand(n, generator=g)
    mask[pick < 0.15] = 0
    mask[pick > 0.6] = 255
    special = torch.tensor([0, 1, 254, 255], dtype=torch.uint8)
    k = min(n, 4)
    mask[:k] = special[:k]
    face_w = torch.rand(T, generator=g) * 1.5
    face_w[0], face_w[1], face_w[2] = 0.0, 2.5, 1.0
    if n >= 12:
        ids[4:8] = torch.tensor([1.0, 2.0, 3.0, 0.0])           # face weights 0, 2.5, 1 and an uncovered pixel
        ref[8:12] = torch.tensor([139, 140, 141, 255], dtype=torch.uint8)      # around the saturation level of the tests
    return dict(colour=colour, rast_w=ids.reshape(Bn, H, W), ref=ref.reshape(Bn, H, W), mask=mask.reshape(Bn, H, W), face_w=face_w, T=T)


SAT = 140


def weights(rast_w, ref_u8, mask=None, face_w=None, w_outside=1.0, sat=0, dtype=torch.float64):
    """w [B,H,W] in `dtype` and covered [B,H,W]."""
    w3 = rast_w.detach().cpu().float()
    cov = w3 > 0
    if mask is not None:
        wm = mask.detach().cpu().to(dtype) * torch.tensor(float(np.float32(1.0) / np.float32(255.0)), dtype=dtype)
    else:
        wm = torch.ones(w3.shape, dtype=dtype)
    if sat > 0:
        wm = torch.where(ref_u8.detach().cpu().to(torch.int64) >= int(sat), torch.zeros((), dtype=dtype), wm)
    fw = torch.ones(w3.shape, dtype=dtype)
    if face_w is not None:
        table = face_w.detach().cpu().to(torch.float32).to(dtype)
        idx = w3.to(torch.int64) - 1
        ok = (idx >= 0) & (idx < table.shape[0])
        fw = torch.where(ok, table[idx.clamp(0, table.shape[0] - 1)], torch.zeros((), dtype=dtype))
    wo = torch.tensor(float(np.float32(w_outside)), dtype=dtype)
    return torch.where(cov, wm * fw, wm * wo), cov


def sqrt_rounded(x):
    """The correctly rounded square root in x's dtype.  torch's float32 root on a CPU is not always (its vectorised path was one unit in the
    last place off on 0.7 % of two million arguments); the float64 root rounded to float32 is (53 >= 2 * 24 + 2 bits: the second rounding
    cannot change the result).  For a statement that is compared bit for bit with the device's sqrtf."""
    return x.sqrt() if x.dtype == torch.float64 else x.double().sqrt().to(x.dtype)


def rho_psi(d, kind, inv_c, sqrt=None):
    """(rho, psi) of a residual tensor by the statement's operations, in d's dtype.  sqrt: the root to use (None: torch's)."""
    dd = d * d
    if kind == 'l2':
        return dd, d
    z = d * inv_c
    t = z * z
    if kind == 'charbonnier':
        h = (1.0 + t).sqrt() if sqrt is None else sqrt(1.0 + t)
        return (2.0 * dd) / (1.0 + h), d * (1.0 / h)
    k = 1.0 + t
    return dd / k, d * (1.0 / (k * k))


def robust_loss(colour, rast_w, ref_u8, kind, c=None, n_total=None, mask=None, face_w=None, w_outside=1.0, sat=0, background=BACKGROUND,
                dtype=torch.float64):
    """-> dict: 'sums' (value [2], S [2]), 'grad' (value, S) [B,H,W,C], 'loss' = sums[0] / n_total, 'w' [B,H,W]."""
    col = colour.detach().to('cpu', dtype)
    w, cov = weights(rast_w, ref_u8, mask, face_w, w_outside, sat, dtype)
    cov4, w4 = cov[..., None], w[..., None]
    r = ref_u8.detach().to('cpu', dtype)[..., None]
    n_total = n_total or col.numel()
    bg = torch.tensor(float(np.float32(background)), dtype=dtype)
    gs = torch.tensor(float(np.float32(1.0 / n_total)), dtype=dtype)
    a = 255.0 * torch.where(cov4, col, bg)
    d = r - a
    Sd = r + a.abs()
    rho, psi = rho_psi(d, kind, inv_scale(c) if kind != 'l2' else 0.0)
    zero = torch.zeros((), dtype=dtype)
    coef = -2.0 * 255.0 * gs
    wC = w4.expand_as(col)
    sums = torch.stack([(wC * rho).sum(), wC.sum()])
    S_sums = torch.stack([(wC * Sd * Sd).sum(), wC.sum()])
    grad = torch.where(cov4, coef * (w4 * psi), zero)
    S = torch.where(cov4, 2.0 * 255.0 * gs * w4 * Sd, zero)
    return {'sums': (sums, S_sums), 'grad': (grad, S), 'loss': sums[0] / float(n_total), 'w': w}


def loss_plain(colour, coverage, ref_u8, kind, c=None, n_total=None, weight=None, background=BACKGROUND):
    """The loss as one plain differentiable torch expression in the dtype of `colour`: rho written the textbook way -- d^2, 2 c^2 (sqrt(1 +
    d^2 / c^2) - 1), d^2 / (1 + d^2 / c^2), with c = 1 / inv_scale(c) -- and a given weight plane [B,H,W] (constants)."""
    dtype = colour.dtype
    cov = (coverage > 0)[..., None]
    bg = torch.tensor(float(np.float32(background)), dtype=dtype, device=colour.device)
    d = ref_u8.to(dtype)[..., None] - 255.0 * torch.where(cov, colour, bg)
    if kind == 'l2':
        rho = d * d
    else:
        c2 = (1.0 / inv_scale(c)) ** 2
        rho = 2.0 * c2 * ((1.0 + d * d / c2).sqrt() - 1.0) if kind == 'charbonnier' else d * d / (1.0 + d * d / c2)
    if weight is not None:
        rho = rho * weight.to(dtype)[..., None]
    return rho.sum() / float(n_total or colour.numel())


def predicted_zeros(rast_w, w, C):
    """Entries of the gradient without any term: uncovered pixels and covered pixels of weight 0, times C."""
    cov = rast_w.detach().cpu() > 0
    return C * int((~cov | (w == 0)).sum())


# option sets of the GPU cases: (name, mask, face weights, sat, w_outside)
OPTIONS = [('plain', False, False, 0, 1.0), ('mask', True, False, 0, 1.0), ('faces', False, True, 0, 0.25), ('sat', False, False, SAT, 0.0),
           ('all', True, True, SAT, 0.25)]


def option_kwargs(inp, opt):
    _, use_mask, use_faces, sat, w_out = opt
    return dict(mask=inp['mask'] if use_mask else None, face_w=inp['face_w'] if use_faces else None, sat=sat, w_outside=w_out)

"""float64 restatement on the CPU of the locally normalised pixel loss (csrc/norm.hip; DESIGN.md 3, "Normalised loss rule"): the
yardstick of tests/test_gpu_norm.py, itself checked on the CPU by tests/test_norm_ref.py.  Nothing here imports fpc_diffrend_amd.

Blur, reflected borders and the fold adjoint are those of tests/blur_ref.py.  The conventions are those of tests/fitstep_ref.py: every
function evaluates in `dtype` (float64 by default; float32 gives "the same formula in float32 by torch", the yardstick e32) and
returns, besides each value, a scale S; fitstep_ref.measure() compares against them in units of u = 2^-24.

The statement, operation by operation:
    a = color_scale * (covered ? colour : bg)      ONE float32 multiply: operands() evaluates it in float32 whatever `dtype` is, because
    t = float(ref)                                 the rounded product IS the operand of the rule; a*a and t*t likewise (rounded once)
    stats():      mu = G x,  m = G (x*x)                                                 S = G |x|, G |x*x|  (sums of the terms' sizes)
    pointwise():  v = max(m - mu*mu, 0),  s = sqrt(v + eps*eps),  n = (x - mu) / s,  d = n_a - n_t,
                  p = (2 d) / s_a,  q = (p * n_a) / s_a,  P = p - q * mu_a
    gradient():   grad_a = (p - G^T P) - a * (G^T q),   grad_colour = covered ? gain * grad_a : 0,   gain = float32(color_scale * gs)
pointwise() and gradient() carry S as a FIRST-ORDER ROUNDING SCALE from the float32 planes they are handed down to each output, by the
rules of tests/rasterize_ref.py (class Q: a sum adds the scales, a product is S_a |b| + |a| S_b, a quotient S_a / |d| + |a / d| S_d /
|d|; an input x has S = |x|), with two more:
    sqrt(x)       S_x / (2 sqrt(x)) + sqrt(x)           the derivative times the operand's scale, plus the root's own rounding
    max(x, 0)     S_x, whether or not the clamp bites   m >= mu^2 holds in exact arithmetic, so the clamp only cuts rounding noise of
                                                        the size S_x describes; float32 and float64 may land on different sides of it
The cancellation of m - mu*mu is thereby in the scale: S_v = |m| + 2 mu^2 against v + eps^2 >= eps^2.  An uncovered entry of the
gradient has no term: S = 0 and it must be exactly 0."""
import numpy as np
import torch
import torch.nn.functional as F

import blur_ref as B
from rasterize_ref import Q

BACKGROUND = B.BACKGROUND
EPS = 2.0

taps = B.taps


EXACT_OPERANDS = False     # set by test_norm_ref.py only, around its autograd check: a and a*a evaluated in `dtype` WITHOUT the float32
                           # roundings -- the differentiable function whose gradient the closed form is (a rounded product has none)


def operands(colour, coverage, ref_u8, background=BACKGROUND, dtype=torch.float64):
    """(a, a*a, t, t*t) [B,H,W,C]: float32 arithmetic (one rounding each, as the kernel's), then converted to `dtype`."""
    work = dtype if EXACT_OPERANDS else torch.float32
    col = colour.detach().to('cpu', work)
    cov = (coverage.detach().cpu() > 0)[..., None]
    bg = torch.tensor(np.float32(background)).to(work)
    a = torch.tensor(np.float32(255.0)).to(work) * torch.where(cov, col, bg)
    t = ref_u8.detach().to('cpu', work)[..., None].expand_as(a).contiguous()
    return tuple(x.to(dtype) for x in (a, a * a, t, t * t))


def stats(colour, coverage, ref_u8, g, background=BACKGROUND, dtype=torch.float64):
    """-> (value, S) [B,H,W,C,4]: (mu_a, m_a, mu_t, m_t) and the blur of the absolute values."""
    ops = operands(colour, coverage, ref_u8, background, dtype)
    val = torch.stack([B.blurred(x, g) for x in ops], dim=-1)
    S = torch.stack([B.blurred(x.abs(), g.abs()) for x in ops], dim=-1)
    return val, S


def _sqrt(x):
    r = x.v.sqrt()
    return Q(r, x.S / (2.0 * r) + r)


def _normalise(x, mu, m, eps2):
    v = m - mu * mu
    v = Q(v.v.clamp(min=0.0), v.S)
    s = _sqrt(v + eps2)
    return (x - mu) / s, s


def pointwise(colour, coverage, ref_u8, stat_planes, eps=EPS, background=BACKGROUND, dtype=torch.float64):
    """From GIVEN statistics planes [B,H,W,C,4] (the float32 ones the kernel wrote): dict name -> (value, S) for d, P, q, p and, without
    a scale, n_a, s_a (float64 intermediates for the tests' own use)."""
    a, _, t, _ = operands(colour, coverage, ref_u8, background, dtype)
    st = stat_planes.detach().to('cpu', dtype)
    inp = lambda x: Q(x, x.abs())
    e32 = torch.tensor(np.float32(eps))
    eps2 = inp((e32 * e32).to(dtype))                       # eps * eps in float32, as the host computes it
    n_a, s_a = _normalise(inp(a), inp(st[..., 0]), inp(st[..., 1]), eps2)
    n_t, _ = _normalise(inp(t), inp(st[..., 2]), inp(st[..., 3]), eps2)
    d = n_a - n_t
    p = (d * 2.0) / s_a
    q = (p * n_a) / s_a
    P = p - q * inp(st[..., 0])
    return {'d': (d.v, d.S), 'P': (P.v, P.S), 'q': (q.v, q.S), 'p': (p.v, p.S), 'n_a': n_a.v, 's_a': s_a.v}


def gradient(colour, coverage, pq, p, g, n_total=None, background=BACKGROUND, dtype=torch.float64):
    """d (sum d^2 / n_total) / d colour from GIVEN planes pq [B,H,W,C,2] and p [B,H,W,C] (the float32 ones the kernel wrote) -> (value, S)."""
    a = operands(colour, coverage, torch.zeros(colour.shape[:3], dtype=torch.uint8), background, dtype)[0]
    cov = (coverage.detach().cpu() > 0)[..., None]
    pqd, pd, gd = pq.detach().to('cpu', dtype), p.detach().to('cpu', dtype), g.to(dtype)
    n_total = n_total or pd.numel()
    gain = (torch.tensor(np.float32(255.0)) * torch.tensor(np.float32(1.0 / n_total))).to(dtype)      # one float32 product, on the host
    adj = lambda x, gg: B.adjoint_axis(B.adjoint_axis(x, gg, 1), gg, 2)
    AP = Q(adj(pqd[..., 0], gd), adj(pqd[..., 0].abs(), gd.abs()))
    AQ = Q(adj(pqd[..., 1], gd), adj(pqd[..., 1].abs(), gd.abs()))
    ga = ((Q(pd, pd.abs()) - AP) - Q(a, a.abs()) * AQ) * gain
    zero = torch.zeros((), dtype=dtype)
    return torch.where(cov, ga.v, zero), torch.where(cov, ga.S, zero)


def loss_and_gradient(colour, coverage, ref_u8, g, eps=EPS, n_total=None, background=BACKGROUND, dtype=torch.float64):
    """The whole statement chained in `dtype`: -> dict with 'stats', 'd', 'P', 'q', 'p', 'grad' as (value, S) and 'sum', 'loss' as values."""
    st = stats(colour, coverage, ref_u8, g, background, dtype)
    pw = pointwise(colour, coverage, ref_u8, st[0], eps, background, dtype)
    pq = torch.stack([pw['P'][0], pw['q'][0]], dim=-1)
    grad = gradient(colour, coverage, pq, pw['p'][0], g, n_total, background, dtype)
    s = (pw['d'][0] * pw['d'][0]).sum()
    out = dict(pw)
    out.update(stats=st, grad=grad, sum=s, loss=s / float(n_total or colour.numel()))
    return out


def normalised(x, g, eps):
    """n(x; eps) for a plane x [B,H,W,C] in its own dtype with taps g as given (no rounding of x*x): the statement the invariance is about."""
    mu, m = B.blurred(x, g), B.blurred(x * x, g)
    return (x - mu) / ((m - mu * mu).clamp(min=0.0) + eps * eps).sqrt()


def loss_plain(colour, coverage, ref_u8, g, eps=EPS, n_total=None, background=BACKGROUND):
    """The whole loss as one plain differentiable torch expression (F.pad(reflect) + conv2d), in the dtype and on the device of `colour`.
    Without the clamp on v: it is the identity in exact arithmetic and the closed-form gradient is used unconditionally, so autograd must
    not be cut off where rounding puts m - mu^2 a hair below 0."""
    Bn, H, W, C = colour.shape
    dtype, dev = colour.dtype, colour.device
    k = g.numel()
    r = (k - 1) // 2
    cov = (coverage > 0)[..., None]
    bg = torch.tensor(float(np.float32(background)), dtype=dtype, device=dev)
    a = 255.0 * torch.where(cov, colour, bg)
    t = ref_u8.to(dtype)[..., None].expand_as(a)
    gg = g.to(dtype).to(dev)

    def blur(x):
        x = F.pad(x.permute(0, 3, 1, 2).reshape(Bn * C, 1, H, W), (r, r, r, r), mode='reflect')
        return F.conv2d(F.conv2d(x, gg.reshape(1, 1, 1, k)), gg.reshape(1, 1, k, 1)).reshape(Bn, C, H, W).permute(0, 2, 3, 1)

    def norm(x):
        mu, m = blur(x), blur(x * x)
        return (x - mu) / (m - mu * mu + eps * eps).sqrt()

    d = norm(a) - norm(t)
    return (d * d).sum() / float(n_total or colour.numel())


# the cases of tests/test_gpu_norm.py beyond blur_ref.SHAPES: (B, H, W, C, kernel size, sigma).  Tile extents of csrc/sep_window.h: the row
# passes take ROW_TX pixels x ROW_TY rows per workgroup, the column passes COL_TX flat columns x COL_TY rows, flat columns being 4 W C
# (forward) or 2 W C (adjoint) wide
ROW_TX, ROW_TY = 256, 4
COL_TX, COL_TY = 64, 64
EXTENT_SHAPES = [(1, 6, ROW_TX - 1, 1, 7, 1.5), (1, 6, ROW_TX, 1, 7, 1.5), (1, 6, ROW_TX + 1, 1, 7, 1.5),
                 (1, COL_TY - 1, 17, 1, 7, 1.5), (1, COL_TY, 16, 1, 7, 1.5), (1, COL_TY + 1, 15, 1, 7, 1.5),
                 (1, 9, 31, 1, 5, 1.0), (1, 9, 32, 1, 5, 1.0), (1, 9, 33, 1, 5, 1.0),       # 2 W around COL_TX (4 W around 2 COL_TX)
                 (1, ROW_TY - 1, 10, 1, 5, 1.0), (1, ROW_TY, 10, 1, 5, 1.0),
                 (1, ROW_TY + 1, 9, 2, 5, 1.0)]                                              # two channels
FLAT_SHAPE = (1, 24, 40, 1, 9, 2.0)
ALL_SHAPES = B.SHAPES + EXTENT_SHAPES


def inputs(Bn, H, W, C, seed=2):
    return B.inputs(Bn, H, W, C, seed)


def flat_inputs():
    """FLAT_SHAPE: the left half uncovered with ref a constant 45 there (a = 255 * bg is 45 up to its rounding): v_a and v_t are
    rounding noise around 0 in that half, the clamp is exercised."""
    Bn, H, W, C = FLAT_SHAPE[:4]
    colour, cover, ref = B.inputs(Bn, H, W, C, seed=7)
    cover[:, :, : W // 2] = 0
    ref[:, :, : W // 2] = 45
    return colour, cover, ref

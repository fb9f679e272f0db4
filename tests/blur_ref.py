"""float64 restatements on the CPU of the blurred pixel loss (csrc/blur.hip; DESIGN.md 3, "Blurred loss rule"): the yardstick of
tests/test_gpu_blur.py, itself checked on the CPU by tests/test_blur_ref.py.  Nothing here imports fpc_diffrend_amd.

The conventions are those of tests/fitstep_ref.py: every function evaluates in `dtype` (float64 by default; float32 gives "the same
formula in float32 by torch", the yardstick of the long sums) and returns, besides each value, its scale S -- the same formula on
absolute values with every subtraction an addition.  fitstep_ref.measure() compares against them in units of u = 2^-24."""
import numpy as np
import torch
import torch.nn.functional as F

BACKGROUND = 45.0 / 255.0


def taps(kernel_size, sigma):
    """g_i = exp(-((i - r) / sigma)^2 / 2), i = 0 .. k - 1, in float64, divided by the sum, rounded to float32 -> tensor [k]."""
    k = int(kernel_size)
    assert k % 2 == 1 and 3 <= k <= 63 and sigma > 0
    x = (np.arange(k, dtype=np.float64) - (k - 1) // 2) / float(sigma)
    g = np.exp(-0.5 * x * x)
    return torch.from_numpy((g / g.sum()).astype(np.float32))


def residual(colour, coverage, ref_u8, background=BACKGROUND, dtype=torch.float64):
    """e = ref - 255 * (coverage > 0 ? colour : background) [B,H,W,C] and its scale; the background is the float32 number the
    kernel is handed."""
    col = colour.detach().to('cpu', dtype)
    cov = (coverage.detach().cpu() > 0)[..., None]
    ref = ref_u8.detach().to('cpu', dtype)[..., None]
    bg = torch.tensor(float(np.float32(background)), dtype=dtype)
    comp = torch.where(cov, col, bg)
    return ref - 255.0 * comp, ref + 255.0 * comp.abs()


def reflect_index(n, r):
    """Source index of the padded positions -r .. n - 1 + r: -j -> j, n - 1 + j -> n - 1 - j (no repeated edge sample)."""
    assert 0 <= r <= n - 1
    p = torch.arange(-r, n + r)
    p = torch.where(p < 0, -p, p)
    return torch.where(p > n - 1, 2 * (n - 1) - p, p)


def blur_axis(x, g, dim):
    """E[i] = sum_k g_k ext[i + k - r] along `dim`, ext the reflected extension of x."""
    k = g.numel()
    r = (k - 1) // 2
    n = x.shape[dim]
    ext = x.index_select(dim, reflect_index(n, r))
    out = torch.zeros_like(x)
    for t in range(k):
        out = out + g[t] * ext.narrow(dim, t, n)
    return out


def blurred(e, g):
    """E = G_y G_x e for e [B,H,W,C]: along W, then along H; each image and channel on its own."""
    g = g.to(e.dtype)
    return blur_axis(blur_axis(e, g, 2), g, 1)


def blurred_residual(colour, coverage, ref_u8, g, background=BACKGROUND, dtype=torch.float64):
    """-> (E, S) with S = blur(|terms|)."""
    e, eabs = residual(colour, coverage, ref_u8, background, dtype)
    return blurred(e, g), blurred(eabs, g.abs())


def loss_sum(E, S):
    """sum E^2 and its scale, from E and the scale of E."""
    return (E * E).sum(), (S * S).sum()


def adjoint_axis(d, g, dim):
    """The adjoint of blur_axis by the fold formula: with d0 = d extended with zeros and c[p] = sum_k g_k d0[p + r - k] for the padded
    positions p = -r .. n - 1 + r, out[j] = c[j], plus c[-j] for 1 <= j <= r, plus c[n - 1 + j] added into n - 1 - j for 1 <= j <= r
    (both folds can land on one entry when n <= 2 r)."""
    k = g.numel()
    r = (k - 1) // 2
    x = d.movedim(dim, -1)
    n = x.shape[-1]
    assert r <= n - 1
    d0 = F.pad(x, (2 * r, 2 * r))                          # d0[q] at index q + 2 r
    c = torch.zeros(x.shape[:-1] + (n + 2 * r,), dtype=x.dtype)      # c[p] at index p + r
    for t in range(k):
        c = c + g[t] * d0[..., 2 * r - t: 2 * r - t + n + 2 * r]     # d0[p + r - t] = index p + 3 r - t, p + r = 0 .. n + 2 r - 1
    out = c[..., r: r + n].clone()
    for j in range(1, r + 1):
        out[..., j] += c[..., r - j]
        out[..., n - 1 - j] += c[..., r + n - 1 + j]
    return out.movedim(-1, dim)


def gradient(E, coverage, g, n_total=None, dtype=torch.float64):
    """d (sum E^2 / n_total) / d colour from a GIVEN plane E (the float32 one the kernel wrote, so that the gradient is judged on it):
    covered ? (-2 * 255 * gs) * (G_x^T G_y^T E) : 0, gs = the float32 1 / n_total -> (value, S)."""
    Ed = E.detach().to('cpu', dtype)
    gd = g.to(dtype)
    cov = (coverage.detach().cpu() > 0)[..., None]
    n_total = n_total or Ed.numel()
    gs = torch.tensor(float(np.float32(1.0 / n_total)), dtype=dtype)
    A = adjoint_axis(adjoint_axis(Ed, gd, 1), gd, 2)
    Aabs = adjoint_axis(adjoint_axis(Ed.abs(), gd.abs(), 1), gd.abs(), 2)
    zero = torch.zeros((), dtype=dtype)
    return torch.where(cov, -2.0 * 255.0 * gs * A, zero), torch.where(cov, 2.0 * 255.0 * gs * Aabs, zero)


def loss_plain(colour, coverage, ref_u8, g, n_total=None, background=BACKGROUND):
    """The whole loss as one plain differentiable torch expression (F.pad(reflect) + two conv2d), in the dtype of `colour`."""
    B, H, W, C = colour.shape
    dtype = colour.dtype
    k = g.numel()
    r = (k - 1) // 2
    cov = (coverage > 0)[..., None]
    bg = torch.tensor(float(np.float32(background)), dtype=dtype, device=colour.device)
    comp = torch.where(cov, colour, bg)
    e = ref_u8.to(dtype)[..., None] - 255.0 * comp
    x = F.pad(e.permute(0, 3, 1, 2).reshape(B * C, 1, H, W), (r, r, r, r), mode='reflect')
    gg = g.to(dtype).to(colour.device)
    E = F.conv2d(F.conv2d(x, gg.reshape(1, 1, 1, k)), gg.reshape(1, 1, k, 1))
    return (E * E).sum() / float(n_total or colour.numel())


# the cases of tests/test_gpu_blur.py (the CPU file checks the fold formula on the same shapes): (B, H, W, C, kernel size, sigma)
SHAPES = [(1, 5, 5, 1, 9, 1.5),          # r = n - 1: every entry folds at both ends
          (1, 16, 16, 1, 31, 5.0),       # the default kernel at the smallest legal image
          (2, 37, 70, 1, 31, 2.0),       # odd extents, two images
          (1, 8, 300, 3, 15, 3.0),       # three channels, W across several row tiles
          (1, 300, 9, 1, 17, 4.0),       # H across several column tiles
          (1, 64, 33, 1, 63, 9.0),       # the largest kernel
          (1, 7, 7, 1, 3, 0.8)]          # the smallest kernel


def inputs(B, H, W, C, seed=2):
    """colour in [0, 1), about 60 % covered (coverage 7 or 0), ref in 0 .. 140: as fitstep_ref.pixel_inputs."""
    gen = torch.Generator().manual_seed(seed)
    colour = torch.rand(B, H, W, C, generator=gen)
    cover = (torch.rand(B, H, W, generator=gen) > 0.4).float() * 7
    ref = torch.randint(0, 141, (B, H, W), generator=gen, dtype=torch.uint8)
    return colour, cover, ref

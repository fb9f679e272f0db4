// Locally normalised pixel loss, value and closed-form gradient, for gfx950 (MI355X).  DESIGN.md 3, "Normalised loss rule".
//
// The reference carries whiten / normalize_highlights (utils.py) and builds torch.nn.LocalResponseNorm(2) at fit.py:510 "for image contrast
// normalization", but wires none of it into its loss.  Here both the render a = color_scale * (covered ? colour : bg) and the capture
// t = ref are normalised by the mean and the deviation of their own Gaussian window before they are compared,
//     mu = G x,  m = G (x x),  v = max(m - mu mu, 0),  s = sqrt(v + eps eps),  n = (x - mu) / s,      d = n_a - n_t,  loss_sum += sum d^2,
// so that a gain and an offset of a camera (x -> alpha x + beta) drop out.  With p = 2 d / s_a, q = p n_a / s_a, P = p - q mu_a the gradient
// is grad_a = p - G^T P - a (G^T q), masked and scaled like k_pixel_loss's.  Taps, reflected borders, the tiling and the column pass
// (with its fold adjoint) are sep_window.h's, shared with blur.hip; k_norm_rows_adj states the fold formula once more, for two planes.
//
// Five streaming passes: rows (from the inputs) -> the four row sums of an entry as one float4; columns over that plane (4 W C flat
// columns) -> (mu_a, m_a, mu_t, m_t); pointwise -> d (+ the f64 sum) and, with a gradient wanted, the planes (P, q) and p; column
// adjoint over (P, q) (2 W C flat columns); row adjoint with the final combine and the coverage mask.  Every plane is written by plain
// stores, one lane per entry, each 1-D sum by fused multiply-add in the order t = 0 .. 2 r: bit-identical from run to run.
#include "sep_window.h"

#include <cmath>

namespace {

// LDS: forward rows 4 * 318 * (4 + 1) floats = 25440 B, adjoint rows 2 * 4 * 318 * 4 floats = 40704 B, columns 32256 B (sep_window.h).
constexpr size_t POINT_BLOCKS = 4096;      // workgroups of the pointwise pass: 16 a CU

// Forward rows: a per entry and t per pixel staged with reflected indices; dst[entry] = (G_x a, G_x a^2, G_x t, G_x t^2).
__global__ void __launch_bounds__(256) k_norm_rows(const float *__restrict__ color, const float4 *__restrict__ rast,
                                                   const uint8_t *__restrict__ ref, float4 *__restrict__ dst, int H, int W, int C, int r,
                                                   float bg, float color_scale, WinTaps taps) {
    __shared__ float sa[ROW_TY][ROW_SPAN * WIN_CMAX];
    __shared__ float st[ROW_TY][ROW_SPAN];
    const int x0 = blockIdx.x * ROW_TX, y0 = blockIdx.y * ROW_TY;
    const size_t img = (size_t)blockIdx.z * H * W;
    const int np = ROW_TX + 2 * r, nq = np * C;      // staged pixels x0 - r .. x0 + ROW_TX + r - 1
    for (int row = 0; row < ROW_TY; ++row) {
        const int y = y0 + row;
        for (int q = threadIdx.x; q < nq; q += 256) {
            int px, c;
            win_split(q, C, px, c);
            int x = x0 - r + px;
            win_reflect(x, W);
            float va = 0.0f, vt = 0.0f;
            if (y < H && x >= 0 && x < W) {
                const size_t pix = img + (size_t)y * W + x;
                va = color_scale * (rast[pix].w > 0.0f ? color[pix * C + c] : bg);
                vt = (float)ref[pix];
            }
            sa[row][q] = va;
            if (c == 0) st[row][px] = vt;
        }
    }
    __syncthreads();
    const int tq = ROW_TX * C, k = 2 * r + 1;
    for (int row = 0; row < ROW_TY; ++row) {
        const int y = y0 + row;
        if (y >= H) break;
        for (int q = threadIdx.x; q < tq; q += 256) {
            int px, c;
            win_split(q, C, px, c);
            const int x = x0 + px;
            if (x >= W) continue;
            const float *pa = &sa[row][q];               // pixel x - r of this channel
            const float *pt = &st[row][px];
            float a1 = 0.0f, a2 = 0.0f, t1 = 0.0f, t2 = 0.0f;
            for (int t = 0; t < k; ++t) {
                const float g = taps.g[t], va = pa[t * C], vt = pt[t];
                a1 = __builtin_fmaf(g, va, a1);
                a2 = __builtin_fmaf(g, va * va, a2);
                t1 = __builtin_fmaf(g, vt, t1);
                t2 = __builtin_fmaf(g, vt * vt, t2);
            }
            dst[(img + (size_t)y * W + x) * C + c] = make_float4(a1, a2, t1, t2);
        }
    }
}

// Column passes over planes of H rows of L floats (sep_window.h, without the sum).  ADJ = false: dst = G_y src.  ADJ = true: dst = G_y^T src.
template <bool ADJ>
__global__ void __launch_bounds__(256) k_norm_cols(const float *__restrict__ src, float *__restrict__ dst, int H, int L, int r,
                                                   WinTaps taps) {
    win_cols<ADJ, false>(src, dst, nullptr, H, L, r, taps);
}

// Pointwise: one lane per entry e = pix * C + c.  d (and, with pq, the planes (P, q) and p) by plain stores; sum d^2 wave -> block ->
// one f64 atomic, as k_pixel_loss.
__global__ void __launch_bounds__(256) k_norm_point(const float *__restrict__ color, const float4 *__restrict__ rast,
                                                    const uint8_t *__restrict__ ref, const float4 *__restrict__ stats,
                                                    float *__restrict__ d_out, float2 *__restrict__ pq, float *__restrict__ p_out,
                                                    double *__restrict__ loss_sum, size_t n_pix, int C, float bg, float color_scale,
                                                    float eps2) {
    __shared__ float s_part[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t n = n_pix * C, stride = (size_t)gridDim.x * 256;
    float sq = 0.0f;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        size_t pix;
        switch (C) {
            case 1: pix = e; break;
            case 2: pix = e >> 1; break;
            case 3: pix = e / 3; break;
            default: pix = e >> 2; break;
        }
        const float a = color_scale * (rast[pix].w > 0.0f ? color[e] : bg);
        const float t = (float)ref[pix];
        const float4 st = stats[e];
        const float va = fmaxf(st.y - st.x * st.x, 0.0f), vt = fmaxf(st.w - st.z * st.z, 0.0f);
        const float s_a = sqrtf(va + eps2), s_t = sqrtf(vt + eps2);
        const float n_a = (a - st.x) / s_a, n_t = (t - st.z) / s_t;
        const float d = n_a - n_t;
        d_out[e] = d;
        sq += d * d;
        if (pq) {
            const float p = (2.0f * d) / s_a;
            const float q = (p * n_a) / s_a;
            pq[e] = make_float2(p - q * st.x, q);
            p_out[e] = p;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (lane == 0) s_part[w] = sq;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss_sum, (double)s_part[0] + (double)s_part[1] + (double)s_part[2] + (double)s_part[3]);
}

// Adjoint rows: src = (G_y^T P, G_y^T q) interleaved per entry, staged with zeros outside the image; AP = G_x^T of the first, AQ of the
// second by the fold formula; dst = covered ? gain * ((p - AP) - a * AQ) : 0.
__global__ void __launch_bounds__(256) k_norm_rows_adj(const float *__restrict__ color, const float4 *__restrict__ rast,
                                                       const float2 *__restrict__ src, const float *__restrict__ p_in,
                                                       float *__restrict__ dst, int H, int W, int C, int r, float color_scale, float gain,
                                                       WinTaps taps) {
    __shared__ float sP[ROW_TY][ROW_SPAN * WIN_CMAX];
    __shared__ float sQ[ROW_TY][ROW_SPAN * WIN_CMAX];
    const int x0 = blockIdx.x * ROW_TX, y0 = blockIdx.y * ROW_TY;
    const size_t img = (size_t)blockIdx.z * H * W;
    const int nq = (ROW_TX + 2 * r) * C;
    for (int row = 0; row < ROW_TY; ++row) {
        const int y = y0 + row;
        for (int q = threadIdx.x; q < nq; q += 256) {
            int px, c;
            win_split(q, C, px, c);
            const int x = x0 - r + px;
            float2 v = make_float2(0.0f, 0.0f);
            if (y < H && x >= 0 && x < W) v = src[(img + (size_t)y * W + x) * C + c];
            sP[row][q] = v.x;
            sQ[row][q] = v.y;
        }
    }
    __syncthreads();
    const int tq = ROW_TX * C, k = 2 * r + 1;
    for (int row = 0; row < ROW_TY; ++row) {
        const int y = y0 + row;
        if (y >= H) break;
        for (int q = threadIdx.x; q < tq; q += 256) {
            int px, c;
            win_split(q, C, px, c);
            const int x = x0 + px;
            if (x >= W) continue;
            float aP = 0.0f, aQ = 0.0f;              // sep_window.h's fold formula, two planes tap by tap
            for (int t = 0; t < k; ++t) {
                const int li = q + (2 * r - t) * C;
                aP = __builtin_fmaf(taps.g[t], sP[row][li], aP);
                aQ = __builtin_fmaf(taps.g[t], sQ[row][li], aQ);
            }
            const int lo = x0 - r;                   // pixel of s[row][0]
            if (x >= 1 && x <= r)                    // c[-x]: sample r - x - t
                for (int t = 0; t < k; ++t) {
                    const int pos = r - x - t, li = (pos - lo) * C + c;
                    if (pos >= 0 && pos < W && li >= 0 && li < nq) {
                        aP = __builtin_fmaf(taps.g[t], sP[row][li], aP);
                        aQ = __builtin_fmaf(taps.g[t], sQ[row][li], aQ);
                    }
                }
            const int j = W - 1 - x;
            if (j >= 1 && j <= r)                    // c[W - 1 + j]: sample W - 1 + j + r - t
                for (int t = 0; t < k; ++t) {
                    const int pos = W - 1 + j + r - t, li = (pos - lo) * C + c;
                    if (pos >= 0 && pos < W && li >= 0 && li < nq) {
                        aP = __builtin_fmaf(taps.g[t], sP[row][li], aP);
                        aQ = __builtin_fmaf(taps.g[t], sQ[row][li], aQ);
                    }
                }
            const size_t pix = img + (size_t)y * W + x, e = pix * C + c;
            float out = 0.0f;
            if (rast[pix].w > 0.0f) {
                const float a = color_scale * color[e];
                out = gain * ((p_in[e] - aP) - a * aQ);
            }
            dst[e] = out;
        }
    }
}

}  // namespace

extern "C" size_t fpcdr_norm_loss_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return (size_t)B * H * W * C * sizeof(float);
}

extern "C" int fpcdr_norm_loss(const fpcdr_norm_loss_params *p, void *stream) {
    FPCDR_REQUIRE(p != nullptr, "null params");
    FPCDR_REQUIRE(p->color && p->rast && p->ref && p->tmp && p->stats && p->d && p->loss_sum, "null pointer");
    FPCDR_REQUIRE(!p->grad_color || (p->pq && p->p), "a gradient needs the planes pq and p");
    FPCDR_REQUIRE(p->B > 0 && p->H > 0 && p->W > 0 && p->C > 0, "sizes must be positive");
    FPCDR_REQUIRE(p->C <= WIN_CMAX, "at most 4 channels");
    FPCDR_REQUIRE(p->B <= 65535 && p->H <= 65535 && (long long)p->W * p->C < (1ll << 28), "sizes out of range");
    FPCDR_REQUIRE(p->radius >= 1 && p->radius <= WIN_RMAX, "kernel size 2 * radius + 1 must be odd and in 3 .. 63");
    FPCDR_REQUIRE(p->radius <= (p->H < p->W ? p->H : p->W) - 1, "reflected borders need radius <= min(H, W) - 1");
    FPCDR_REQUIRE(std::isfinite(p->eps) && p->eps > 0.0f && std::isfinite(p->eps * p->eps), "eps must be finite and positive");
    FPCDR_REQUIRE(((uintptr_t)p->tmp & 15) == 0 && ((uintptr_t)p->stats & 15) == 0 && ((uintptr_t)p->pq & 7) == 0,
                  "tmp and stats must be 16-byte aligned, pq 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int B = p->B, H = p->H, W = p->W, C = p->C, L = W * C, r = p->radius;
    const WinTaps taps = win_taps(p->taps, r);
    const float eps2 = p->eps * p->eps;
    const size_t n_pix = (size_t)B * H * W, n_blocks = (n_pix * C + 255) / 256;
    const dim3 grid_rows = win_grid(W, ROW_TX, H, ROW_TY, B);
    const dim3 grid_cols4 = win_grid(4 * L, COL_TX, H, COL_TY, B), grid_cols2 = win_grid(2 * L, COL_TX, H, COL_TY, B);
    // (a grid-stride loop over at most POINT_BLOCKS workgroups: one f64 atomic per workgroup on one address -- a workgroup per 256
    // entries was 259 k atomics at 32 x 1080p and 3.2 ms of a 0.8 ms pass)
    const dim3 grid_point((unsigned)(n_blocks < POINT_BLOCKS ? n_blocks : POINT_BLOCKS));
    hipLaunchKernelGGL(k_norm_rows, grid_rows, dim3(256), 0, st, p->color, (const float4 *)p->rast, p->ref, (float4 *)p->tmp, H, W, C, r,
                       p->bg, p->color_scale, taps);
    FPCDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_norm_cols<false>, grid_cols4, dim3(256), 0, st, (const float *)p->tmp, p->stats, H, 4 * L, r, taps);
    FPCDR_CHECK_LAUNCH();
    const bool want_grad = p->grad_color != nullptr;
    hipLaunchKernelGGL(k_norm_point, grid_point, dim3(256), 0, st, p->color, (const float4 *)p->rast, p->ref, (const float4 *)p->stats,
                       p->d, want_grad ? (float2 *)p->pq : (float2 *)nullptr, want_grad ? p->p : (float *)nullptr, p->loss_sum, n_pix, C,
                       p->bg, p->color_scale, eps2);
    FPCDR_CHECK_LAUNCH();
    if (!want_grad) return FPCDR_OK;
    hipLaunchKernelGGL(k_norm_cols<true>, grid_cols2, dim3(256), 0, st, (const float *)p->pq, p->tmp, H, 2 * L, r, taps);
    FPCDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_norm_rows_adj, grid_rows, dim3(256), 0, st, p->color, (const float4 *)p->rast, (const float2 *)p->tmp,
                       (const float *)p->p, p->grad_color, H, W, C, r, p->color_scale, p->color_scale * p->grad_scale, taps);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

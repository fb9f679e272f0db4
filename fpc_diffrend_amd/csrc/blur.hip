// Gaussian-blurred L2 pixel loss, value and closed-form gradient, for gfx950 (MI355X).  DESIGN.md 3, "Blurred loss rule".
//
// The reference builds transforms.GaussianBlur(kernel_size=(31, 31)) at fit.py:506 and still names ref_blur / colour_blur in its
// preview code (fit.py:629, :632), but never wires a loss on the blurred residual.  Here: e = ref - color_scale * (covered ? colour : bg)
// (k_pixel_loss's arithmetic), E = G_y G_x e with reflected borders, loss_sum += sum E^2, and -- the loss being the root of the graph --
// grad_color = covered ? (-2 color_scale grad_scale) (G_x^T G_y^T E) : 0 with the true adjoint of the reflecting blur.
//
// Four streaming passes, one read and one write of a float plane each: rows (from the inputs) -> tmp, columns -> blurred (+ sum E^2),
// column adjoint -> tmp, row adjoint (+ mask and scale) -> grad_color.  A workgroup stages its tile plus a halo of `radius` in LDS from
// whole contiguous row segments (the column passes too: a lane owns a COLUMN of the tile, a wave reads 64 neighbouring floats of one
// row), and every lane of a wave reads neighbouring LDS words in the tap loop: no bank conflict.  The forward passes stage the reflected
// samples themselves; the adjoint passes stage the plane extended with zeros and add the two mirrored partial sums
//     out[j] = c[j] + (1 <= j <= r ? c[-j] : 0) + (1 <= n-1-j <= r ? c[2 (n-1) - j] : 0),   c[p] = sum_t g_t d0[p + r - t].
// The taps arrive in the kernel arguments and are indexed by the (uniform) loop counter: scalar loads, no private segment.  Every
// entry is accumulated by one lane in the order t = 0 .. 2 r (main term, fold at the start, fold at the end): bit-reproducible.
#include "common.h"

namespace {

constexpr int BLUR_RMAX = 31;      // 2 r + 1 <= 63
constexpr int BLUR_CMAX = 4;       // channels a staged row segment has room for
// Tile extents (tests/test_gpu_blur.py states the same numbers): the row passes take ROW_TX pixels x ROW_TY rows per workgroup, the
// column passes COL_TX flat columns (x * C + c) x COL_TY rows.  LDS: 4 * (256 + 62) * 4 floats = 20352 B and (64 + 62) * 64 floats =
// 32256 B, so at least four workgroups fit the 160 KiB of a CU.
constexpr int ROW_TX = 256, ROW_TY = 4;
constexpr int COL_TX = 64, COL_TY = 64;

struct BlurTaps {
    float g[64];
};

// flat index q = px * C + c of a row segment -> (px, c), C in 1 .. BLUR_CMAX: constant divisors behind a uniform switch, no integer division
__device__ __forceinline__ void blur_split(int q, int C, int &px, int &c) {
    switch (C) {
        case 1: px = q; c = 0; break;
        case 2: px = q >> 1; c = q & 1; break;
        case 3: px = q / 3; c = q - 3 * px; break;
        default: px = q >> 2; c = q & 3; break;
    }
}

// Row passes.  ADJ = false: residual from the inputs, reflected staging, dst = G_x e.  ADJ = true: src (the column adjoint) staged with
// zeros outside the image, dst = covered ? gain * (G_x^T src) : 0.
template <bool ADJ>
__global__ void __launch_bounds__(256) k_blur_rows(const float *__restrict__ color, const float4 *__restrict__ rast,
                                                   const uint8_t *__restrict__ ref, const float *__restrict__ src,
                                                   float *__restrict__ dst, int H, int W, int C, int r, float bg, float color_scale,
                                                   float gain, BlurTaps taps) {
    __shared__ float s[ROW_TY][(ROW_TX + 2 * BLUR_RMAX) * BLUR_CMAX];
    const int x0 = blockIdx.x * ROW_TX, y0 = blockIdx.y * ROW_TY;
    const size_t img = (size_t)blockIdx.z * H * W;
    const int nq = (ROW_TX + 2 * r) * C;          // staged floats of a row: pixels x0 - r .. x0 + ROW_TX + r - 1
    for (int row = 0; row < ROW_TY; ++row) {
        const int y = y0 + row;
        for (int q = threadIdx.x; q < nq; q += 256) {
            int px, c;
            blur_split(q, C, px, c);
            int x = x0 - r + px;
            float v = 0.0f;
            if (!ADJ) {
                if (x < 0) x = -x;
                if (x > W - 1) x = 2 * (W - 1) - x;      // (below 0 only past the last sample any output of the image takes)
            }
            if (y < H && x >= 0 && x < W) {
                const size_t pix = img + (size_t)y * W + x;
                if (ADJ) {
                    v = src[pix * C + c];
                } else {
                    const float col = rast[pix].w > 0.0f ? color[pix * C + c] : bg;
                    v = (float)ref[pix] - col * color_scale;
                }
            }
            s[row][q] = v;
        }
    }
    __syncthreads();
    const int tq = ROW_TX * C, k = 2 * r + 1;
    for (int row = 0; row < ROW_TY; ++row) {
        const int y = y0 + row;
        if (y >= H) break;
        for (int q = threadIdx.x; q < tq; q += 256) {
            int px, c;
            blur_split(q, C, px, c);
            const int x = x0 + px;
            if (x >= W) continue;
            const float *sp = &s[row][q];               // pixel x - r of this channel
            float acc = 0.0f;
            if (!ADJ) {
                for (int t = 0; t < k; ++t) acc = __builtin_fmaf(taps.g[t], sp[t * C], acc);
                dst[(img + (size_t)y * W + x) * C + c] = acc;
            } else {
                for (int t = 0; t < k; ++t) acc = __builtin_fmaf(taps.g[t], sp[(2 * r - t) * C], acc);
                const int lo = x0 - r;                   // pixel of s[row][0]
                if (x >= 1 && x <= r)                    // c[-x]: sample r - x - t
                    for (int t = 0; t < k; ++t) {
                        const int pos = r - x - t, li = (pos - lo) * C + c;
                        if (pos >= 0 && pos < W && li >= 0 && li < nq) acc = __builtin_fmaf(taps.g[t], s[row][li], acc);
                    }
                const int j = W - 1 - x;
                if (j >= 1 && j <= r)                    // c[W - 1 + j]: sample W - 1 + j + r - t
                    for (int t = 0; t < k; ++t) {
                        const int pos = W - 1 + j + r - t, li = (pos - lo) * C + c;
                        if (pos >= 0 && pos < W && li >= 0 && li < nq) acc = __builtin_fmaf(taps.g[t], s[row][li], acc);
                    }
                const size_t pix = img + (size_t)y * W + x;
                dst[pix * C + c] = rast[pix].w > 0.0f ? gain * acc : 0.0f;
            }
        }
    }
}

// Column passes over planes of H rows of L = W * C floats.  ADJ = false: reflected staging, dst = G_y src and loss_sum += sum dst^2
// (wave -> block -> one f64 atomic, as k_pixel_loss).  ADJ = true: zero-extended staging, dst = G_y^T src.
template <bool ADJ>
__global__ void __launch_bounds__(256) k_blur_cols(const float *__restrict__ src, float *__restrict__ dst,
                                                   double *__restrict__ loss_sum, int H, int L, int r, BlurTaps taps) {
    __shared__ float s[COL_TY + 2 * BLUR_RMAX][COL_TX];
    __shared__ float s_part[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * COL_TX + lane, y0 = blockIdx.y * COL_TY;
    const size_t base = (size_t)blockIdx.z * H * L;
    const int ny = COL_TY + 2 * r, k = 2 * r + 1;
    for (int row = w; row < ny; row += 4) {              // rows y0 - r .. y0 + COL_TY + r - 1
        int y = y0 - r + row;
        if (!ADJ) {
            if (y < 0) y = -y;
            if (y > H - 1) y = 2 * (H - 1) - y;
        }
        float v = 0.0f;
        if (y >= 0 && y < H && q < L) v = src[base + (size_t)y * L + q];
        s[row][lane] = v;
    }
    __syncthreads();
    float sq = 0.0f;
    for (int i = 0; i < COL_TY / 4; ++i) {
        const int row = w * (COL_TY / 4) + i, y = y0 + row;      // (uniform over the wave)
        if (y >= H) break;
        if (q >= L) continue;
        float acc = 0.0f;
        if (!ADJ) {
            for (int t = 0; t < k; ++t) acc = __builtin_fmaf(taps.g[t], s[row + t][lane], acc);
            sq += acc * acc;
        } else {
            for (int t = 0; t < k; ++t) acc = __builtin_fmaf(taps.g[t], s[row + 2 * r - t][lane], acc);
            const int lo = y0 - r;                       // row of s[0]
            if (y >= 1 && y <= r)
                for (int t = 0; t < k; ++t) {
                    const int pos = r - y - t, li = pos - lo;
                    if (pos >= 0 && pos < H && li >= 0 && li < ny) acc = __builtin_fmaf(taps.g[t], s[li][lane], acc);
                }
            const int j = H - 1 - y;
            if (j >= 1 && j <= r)
                for (int t = 0; t < k; ++t) {
                    const int pos = H - 1 + j + r - t, li = pos - lo;
                    if (pos >= 0 && pos < H && li >= 0 && li < ny) acc = __builtin_fmaf(taps.g[t], s[li][lane], acc);
                }
        }
        dst[base + (size_t)y * L + q] = acc;
    }
    if (!ADJ) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o, 64);
        if (lane == 0) s_part[w] = sq;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(loss_sum, (double)s_part[0] + (double)s_part[1] + (double)s_part[2] + (double)s_part[3]);
    }
}

}  // namespace

extern "C" size_t fpcdr_blur_loss_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return (size_t)B * H * W * C * sizeof(float);
}

extern "C" int fpcdr_blur_loss(const fpcdr_blur_loss_params *p, void *stream) {
    FPCDR_REQUIRE(p != nullptr, "null params");
    FPCDR_REQUIRE(p->color && p->rast && p->ref && p->tmp && p->blurred && p->loss_sum, "null pointer");
    FPCDR_REQUIRE(p->B > 0 && p->H > 0 && p->W > 0 && p->C > 0, "sizes must be positive");
    FPCDR_REQUIRE(p->C <= BLUR_CMAX, "at most 4 channels");
    FPCDR_REQUIRE(p->B <= 65535 && p->H <= 65535 && (long long)p->W * p->C < (1ll << 30), "sizes out of range");
    FPCDR_REQUIRE(p->radius >= 1 && p->radius <= BLUR_RMAX, "kernel size 2 * radius + 1 must be odd and in 3 .. 63");
    FPCDR_REQUIRE(p->radius <= (p->H < p->W ? p->H : p->W) - 1, "reflected borders need radius <= min(H, W) - 1");
    const hipStream_t st = (hipStream_t)stream;
    const int B = p->B, H = p->H, W = p->W, C = p->C, L = W * C, r = p->radius;
    BlurTaps taps;
    for (int t = 0; t < 64; ++t) taps.g[t] = t <= 2 * r ? p->taps[t] : 0.0f;
    const dim3 grid_rows((W + ROW_TX - 1) / ROW_TX, (H + ROW_TY - 1) / ROW_TY, B);
    const dim3 grid_cols((L + COL_TX - 1) / COL_TX, (H + COL_TY - 1) / COL_TY, B);
    hipLaunchKernelGGL(k_blur_rows<false>, grid_rows, dim3(256), 0, st, p->color, (const float4 *)p->rast, p->ref, (const float *)nullptr,
                       p->tmp, H, W, C, r, p->bg, p->color_scale, 0.0f, taps);
    FPCDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_blur_cols<false>, grid_cols, dim3(256), 0, st, (const float *)p->tmp, p->blurred, p->loss_sum, H, L, r, taps);
    FPCDR_CHECK_LAUNCH();
    if (!p->grad_color) return FPCDR_OK;
    hipLaunchKernelGGL(k_blur_cols<true>, grid_cols, dim3(256), 0, st, (const float *)p->blurred, p->tmp, (double *)nullptr, H, L, r, taps);
    FPCDR_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_blur_rows<true>, grid_rows, dim3(256), 0, st, (const float *)nullptr, (const float4 *)p->rast,
                       (const uint8_t *)nullptr, (const float *)p->tmp, p->grad_color, H, W, C, r, p->bg, p->color_scale,
                       -2.0f * p->color_scale * p->grad_scale, taps);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

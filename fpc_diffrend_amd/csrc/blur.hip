// Gaussian-blurred L2 pixel loss, value and closed-form gradient, for gfx950 (MI355X).  DESIGN.md 3, "Blurred loss rule".
//
// The reference builds transforms.GaussianBlur(kernel_size=(31, 31)) at fit.py:506 and still names ref_blur / colour_blur in its
// preview code (fit.py:629, :632), but never wires a loss on the blurred residual.  Here: e = ref - color_scale * (covered ? colour : bg)
// (k_pixel_loss's arithmetic), E = G_y G_x e with reflected borders, loss_sum += sum E^2, and -- the loss being the root of the graph --
// grad_color = covered ? (-2 color_scale grad_scale) (G_x^T G_y^T E) : 0 with the true adjoint of the reflecting blur.
//
// Four streaming passes, one read and one write of a float plane each: rows (from the inputs) -> tmp, columns -> blurred (+ sum E^2),
// column adjoint -> tmp, row adjoint (+ mask and scale) -> grad_color.  The tiling, the taps in the kernel arguments, the column pass and
// the fold adjoint are sep_window.h's, shared with norm.hip; the row kernel here keeps its own staging (the residual) and forward tap loop.
#include "sep_window.h"

namespace {

// Row passes.  ADJ = false: residual from the inputs, reflected staging, dst = G_x e.  ADJ = true: src (the column adjoint) staged with
// zeros outside the image, dst = covered ? gain * (G_x^T src) : 0.
template <bool ADJ>
__global__ void __launch_bounds__(256) k_blur_rows(const float *__restrict__ color, const float4 *__restrict__ rast,
                                                   const uint8_t *__restrict__ ref, const float *__restrict__ src,
                                                   float *__restrict__ dst, int H, int W, int C, int r, float bg, float color_scale,
                                                   float gain, WinTaps taps) {
    __shared__ float s[ROW_TY][ROW_SPAN * WIN_CMAX];
    const int x0 = blockIdx.x * ROW_TX, y0 = blockIdx.y * ROW_TY;
    const size_t img = (size_t)blockIdx.z * H * W;
    const int nq = (ROW_TX + 2 * r) * C;          // staged floats of a row: pixels x0 - r .. x0 + ROW_TX + r - 1
    for (int row = 0; row < ROW_TY; ++row) {
        const int y = y0 + row;
        for (int q = threadIdx.x; q < nq; q += 256) {
            int px, c;
            win_split(q, C, px, c);
            int x = x0 - r + px;
            float v = 0.0f;
            if (!ADJ) win_reflect(x, W);
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
            win_split(q, C, px, c);
            const int x = x0 + px;
            if (x >= W) continue;
            const float *sp = &s[row][q];               // pixel x - r of this channel
            float acc = 0.0f;
            if (!ADJ) {
                for (int t = 0; t < k; ++t) acc = __builtin_fmaf(taps.g[t], sp[t * C], acc);
                dst[(img + (size_t)y * W + x) * C + c] = acc;
            } else {
                win_fold_adjoint(acc, [&](int li) { return s[row][li]; }, q, x, W, r, x0 - r, C, c, nq, taps);
                const size_t pix = img + (size_t)y * W + x;
                dst[pix * C + c] = rast[pix].w > 0.0f ? gain * acc : 0.0f;
            }
        }
    }
}

// Column passes over planes of H rows of L = W * C floats (sep_window.h).  ADJ = false: dst = G_y src and loss_sum += sum dst^2.
// ADJ = true: dst = G_y^T src.
template <bool ADJ>
__global__ void __launch_bounds__(256) k_blur_cols(const float *__restrict__ src, float *__restrict__ dst,
                                                   double *__restrict__ loss_sum, int H, int L, int r, WinTaps taps) {
    win_cols<ADJ, !ADJ>(src, dst, loss_sum, H, L, r, taps);
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
    FPCDR_REQUIRE(p->C <= WIN_CMAX, "at most 4 channels");
    FPCDR_REQUIRE(p->B <= 65535 && p->H <= 65535 && (long long)p->W * p->C < (1ll << 30), "sizes out of range");
    FPCDR_REQUIRE(p->radius >= 1 && p->radius <= WIN_RMAX, "kernel size 2 * radius + 1 must be odd and in 3 .. 63");
    FPCDR_REQUIRE(p->radius <= (p->H < p->W ? p->H : p->W) - 1, "reflected borders need radius <= min(H, W) - 1");
    const hipStream_t st = (hipStream_t)stream;
    const int B = p->B, H = p->H, W = p->W, C = p->C, L = W * C, r = p->radius;
    const WinTaps taps = win_taps(p->taps, r);
    const dim3 grid_rows = win_grid(W, ROW_TX, H, ROW_TY, B), grid_cols = win_grid(L, COL_TX, H, COL_TY, B);
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

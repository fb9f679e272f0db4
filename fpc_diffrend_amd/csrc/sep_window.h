// What the two windowed pixel losses share (blur.hip: k_blur_rows, k_blur_cols; norm.hip: k_norm_rows, k_norm_cols, k_norm_point,
// k_norm_rows_adj).  Not part of the C ABI.  A separable window of 2 r + 1 taps with reflected borders, applied to float planes in
// streaming passes: a workgroup of 256 stages its tile plus a halo of r in LDS from whole contiguous row segments, and
// every lane of a wave reads neighbouring LDS words in the tap loop: no bank conflict.  The forward passes stage the reflected samples
// themselves; the adjoint passes stage the plane extended with zeros and add the two mirrored partial sums
//     out[j] = c[j] + (1 <= j <= r ? c[-j] : 0) + (1 <= n-1-j <= r ? c[2 (n-1) - j] : 0),   c[p] = sum_t g_t d0[p + r - t].
// The taps arrive in the kernel arguments and are indexed by the (uniform) loop counter: scalar loads, no private segment.  Every entry
// is accumulated by one lane in the order t = 0 .. 2 r (main term, fold at the start, fold at the end): bit-reproducible.
#pragma once
#include "common.h"

namespace {

constexpr int WIN_RMAX = 31;       // 2 r + 1 <= 63
constexpr int WIN_CMAX = 4;        // channels a staged row segment has room for
// Tile extents (tests/test_gpu_blur.py and tests/norm_ref.py state the same numbers): the row passes take ROW_TX pixels x ROW_TY rows per
// workgroup, the column passes COL_TX flat columns x COL_TY rows.  LDS of a staged row plane 4 * (256 + 62) * 4 floats = 20352 B (blur
// one, norm forward one and a quarter, norm adjoint two), of the columns (64 + 62) * 64 floats = 32256 B: at least four workgroups fit
// the 160 KiB of a CU.
constexpr int ROW_TX = 256, ROW_TY = 4;
constexpr int COL_TX = 64, COL_TY = 64;
constexpr int ROW_SPAN = ROW_TX + 2 * WIN_RMAX;      // staged pixels of a row at the largest radius

struct WinTaps {
    float g[64];
};

// flat index q = px * C + c of a row segment -> (px, c), C in 1 .. WIN_CMAX: constant divisors behind a uniform switch, no integer division
__device__ __forceinline__ void win_split(int q, int C, int &px, int &c) {
    switch (C) {
        case 1: px = q; c = 0; break;
        case 2: px = q >> 1; c = q & 1; break;
        case 3: px = q / 3; c = q - 3 * px; break;
        default: px = q >> 2; c = q & 3; break;
    }
}

// i -> the sample of a line of n that index i reads with reflected borders (forward staging; below 0 only past the last sample any output
// of the line takes)
__device__ __forceinline__ void win_reflect(int &i, int n) {
    if (i < 0) i = -i;
    if (i > n - 1) i = 2 * (n - 1) - i;
}

// The fold formula, for output j of a line of n samples staged with zeros outside the line: acc = out[j].  at(li) reads staged index li;
// sample pos of the line has the index (pos - lo) * step + off, the staged indices are 0 .. lim - 1, and i0 is the index of sample j - r.
// (k_norm_rows_adj, which folds two planes at once, keeps a loop nest of its own: through this helper it ran 2 % slower,
// profiles/window_share_ab.txt.)
template <typename At>
__device__ __forceinline__ void win_fold_adjoint(float &acc, At at, int i0, int j, int n, int r, int lo, int step, int off, int lim,
                                                 const WinTaps &taps) {
    const int k = 2 * r + 1;
    for (int t = 0; t < k; ++t) acc = __builtin_fmaf(taps.g[t], at(i0 + (2 * r - t) * step), acc);
    if (j >= 1 && j <= r)                        // c[-j]: sample r - j - t
        for (int t = 0; t < k; ++t) {
            const int pos = r - j - t, li = (pos - lo) * step + off;
            if (pos >= 0 && pos < n && li >= 0 && li < lim) acc = __builtin_fmaf(taps.g[t], at(li), acc);
        }
    const int m = n - 1 - j;
    if (m >= 1 && m <= r)                        // c[n - 1 + m]: sample n - 1 + m + r - t
        for (int t = 0; t < k; ++t) {
            const int pos = n - 1 + m + r - t, li = (pos - lo) * step + off;
            if (pos >= 0 && pos < n && li >= 0 && li < lim) acc = __builtin_fmaf(taps.g[t], at(li), acc);
        }
}

// sum of sq over the workgroup of 256 (wave -> block), then one f64 atomic, as k_pixel_loss.  (k_norm_point keeps a tail of its own: with
// this one the compiler emits other code for it than before.)
__device__ __forceinline__ void win_block_sum(float sq, double *loss_sum) {
    __shared__ float s_part[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (lane == 0) s_part[w] = sq;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(loss_sum, (double)s_part[0] + (double)s_part[1] + (double)s_part[2] + (double)s_part[3]);
}

// Column pass over planes of H rows of L floats, the body of k_blur_cols / k_norm_cols: a lane owns a COLUMN of the tile, a wave reads 64
// neighbouring floats of one row.  ADJ = false: reflected staging, dst = G_y src and, with SUM_SQ, loss_sum += sum dst^2 (wave -> block
// -> one f64 atomic, as k_pixel_loss).  ADJ = true: zero-extended staging, dst = G_y^T src by the fold formula.  (The pointers are the
// kernel's __restrict__ ones; qualified again here, the inlined body compiles to other code than it did in the kernels.)
template <bool ADJ, bool SUM_SQ>
__device__ __forceinline__ void win_cols(const float *src, float *dst, double *loss_sum, int H, int L, int r, const WinTaps &taps) {
    __shared__ float s[COL_TY + 2 * WIN_RMAX][COL_TX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * COL_TX + lane, y0 = blockIdx.y * COL_TY;
    const size_t base = (size_t)blockIdx.z * H * L;
    const int ny = COL_TY + 2 * r, k = 2 * r + 1;
    for (int row = w; row < ny; row += 4) {              // rows y0 - r .. y0 + COL_TY + r - 1
        int y = y0 - r + row;
        if (!ADJ) win_reflect(y, H);
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
            if (SUM_SQ) sq += acc * acc;
        } else {
            win_fold_adjoint(acc, [&](int li) { return s[li][lane]; }, row, y, H, r, y0 - r, 1, 0, ny, taps);
        }
        dst[base + (size_t)y * L + q] = acc;
    }
    if (SUM_SQ) win_block_sum(sq, loss_sum);
}

// the taps of a call in the kernel-argument form: taps[0 .. 2 r], zeros behind them
inline WinTaps win_taps(const float *taps, int r) {
    WinTaps w;
    for (int t = 0; t < 64; ++t) w.g[t] = t <= 2 * r ? taps[t] : 0.0f;
    return w;
}

// workgroups of tx x ty over nx x ny, one layer per image
inline dim3 win_grid(int nx, int tx, int ny, int ty, int B) { return dim3((nx + tx - 1) / tx, (ny + ty - 1) / ty, B); }

}  // namespace

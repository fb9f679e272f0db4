// Comparison of re-rendered images with the captures (include/fpcdr.h, fpcdr_compare_u8; reference src/torch/comparisons.py:
// compareSequence's per-pixel heat map, :36-48, and the integer differences behind compareSequenceNumerical's row means, :64-75).  The
// rule is DESIGN.md 3, "Comparison rule": quantise the rendered image (float: one float32 multiply, NaN -> 0, round half to even, clip;
// uint8: as it is), flip ITS rows if asked, difference against the capture, heat-map colour from the difference, and the sum of
// |difference| of every row over a column crop -- integers throughout, bit for bit the numpy statement of tests/compare_ref.py.
//
// One thread owns 16 consecutive pixels of one output row, read and written in the two forms of u8_chunk.h: one 16-byte load of the
// capture, four of a float image (one of a uint8 image), the 48 heat-map bytes as three 16-byte stores.
// Row sums: the 256 chunks of a workgroup are consecutive in (row, column) order, so they span at most 256 rows: an LDS table of those
// rows takes one integer ds_add per thread with something to add, and is flushed with ONE global integer atomic per touched row and
// workgroup.  Integer adds commute: the sums do not depend on the order of arrival.  No private segment.
#include "u8_chunk.h"

namespace {

// four pixels (bytes of q and r) -> their |d| inside the crop added to `sum`, their 12 heat-map bytes in w0..w2
template <int MODE>
__device__ __forceinline__ void compare4(uint32_t q, uint32_t r, int j, int c0, int c1, int &sum, uint32_t &w0, uint32_t &w1, uint32_t &w2) {
    uint32_t px[4];      // (constant indices only: registers)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int d = (int)((q >> (8 * p)) & 255u) - (int)((r >> (8 * p)) & 255u);
        const int a = d < 0 ? -d : d;
        const uint32_t s = (uint32_t)max(255 - 2 * a, 0);
        sum += (j + p >= c0 && j + p < c1) ? a : 0;
        // bytes in memory order: channel 0 lowest
        if (MODE == 0) px[p] = d >= 0 ? (255u | s << 8 | s << 16) : (s | s << 8 | 255u << 16);
        else           px[p] = s * 0x010101u;
    }
    w0 = px[0] | px[1] << 24;
    w1 = px[1] >> 8 | px[2] << 16;
    w2 = px[2] >> 16 | px[3] << 8;
}

// grid: x over the H * Wc 16-pixel chunks of one image (Wc = ceil(W / 16)), y over the images of this launch (image number
// first_image + blockIdx.y: nothing 64-bit is divided per thread).  c0, c1: the crop clipped to [0, W] by the host.
template <bool IS_FLOAT, int MODE>
__global__ void __launch_bounds__(256) k_compare_u8(const void *__restrict__ img_, float scale, const uint8_t *__restrict__ ref,
                                                    uint8_t *__restrict__ heat, int32_t *__restrict__ row_sums, long long first_image, int H,
                                                    int W, fpcdr_div by_wc, int c0, int c1, int flip_rows) {
    __shared__ int rows_lds[256];
    const unsigned Wc = by_wc.d, total = (unsigned)H * Wc;
    const unsigned t0 = blockIdx.x * 256u, t = t0 + threadIdx.x;
    const bool live = t < total;
    const unsigned tc = live ? t : total - 1;                  // (a thread past the image computes nothing and adds nothing)
    const int i = (int)fpcdr_divide(tc, by_wc);
    const int j0 = (int)(tc - (unsigned)i * Wc) * 16;
    const long long n = first_image + blockIdx.y;
    const bool whole = j0 + 16 <= W;
    if (row_sums) rows_lds[threadIdx.x] = 0;

    int sum = 0;
    if (live) {
        // the capture: row i.  The rendered image: row i, or H - 1 - i of a raster with row 0 at the bottom.  Pixels past W stay 0 in
        // both: d = 0
        uint32_t rw[4] = {0u, 0u, 0u, 0u}, qw[4] = {0u, 0u, 0u, 0u};
        load_chunk_u8(ref + (n * H + i) * W + j0, whole, j0, W, rw);
        load_chunk_render<IS_FLOAT>(img_, (n * H + (flip_rows ? H - 1 - i : i)) * W + j0, scale, whole, j0, W, qw);
        // ---- differences, heat-map bytes ----
        uint32_t w[12];
#pragma unroll
        for (int g = 0; g < 4; ++g) compare4<MODE>(qw[g], rw[g], j0 + 4 * g, c0, c1, sum, w[3 * g], w[3 * g + 1], w[3 * g + 2]);
        if (heat) store_chunk_rgb(heat + ((n * H + i) * W + j0) * 3, whole, j0, W, w);
    }
    // ---- row sums: LDS table of the rows this workgroup's chunks span, one global atomic per touched row ----
    if (row_sums) {        // (uniform: the barriers are reached by every thread or by none)
        const int i_first = (int)fpcdr_divide(t0, by_wc);
        __syncthreads();
        if (sum != 0) atomicAdd(&rows_lds[i - i_first], sum);
        __syncthreads();
        const int v = rows_lds[threadIdx.x];     // (slot k = row i_first + k; a slot past the workgroup's last row was never added to)
        if (v != 0) atomicAdd(row_sums + n * H + i_first + (int)threadIdx.x, v);
    }
}

}  // namespace

extern "C" int fpcdr_compare_u8(const void *img, int img_is_float, float scale, const uint8_t *ref, uint8_t *heat, int32_t *row_sums,
                                int64_t n_images, int H, int W, int col0, int col1, int mode, int flip_rows, void *stream) {
    FPCDR_REQUIRE(img != nullptr && ref != nullptr, "null pointer");
    FPCDR_REQUIRE(heat != nullptr || row_sums != nullptr, "heat and row_sums are both null: nothing to compute");
    FPCDR_REQUIRE(n_images > 0 && H > 0 && W > 0, "sizes must be positive");
    FPCDR_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (colour) or 1 (grey)");
    FPCDR_REQUIRE((long long)W * 255 <= 0x7fffffffLL, "a row sum of 255 * W does not fit int32");
    const int Wc = fpcdr_cdiv(W, 16);
    FPCDR_REQUIRE((long long)H * Wc <= (1LL << 31) - 256, "image too large");
    const size_t px = (size_t)n_images * H * W;
    const size_t img_bytes = px * (img_is_float ? 4 : 1), rows_bytes = (size_t)n_images * H * 4;
    FPCDR_REQUIRE(!overlap(heat, px * 3, img, img_bytes) && !overlap(heat, px * 3, ref, px), "heat overlaps img or ref");
    FPCDR_REQUIRE(!overlap(row_sums, rows_bytes, img, img_bytes) && !overlap(row_sums, rows_bytes, ref, px) &&
                  !overlap(row_sums, rows_bytes, heat, px * 3), "row_sums overlaps another buffer");
    const int c0 = col0 < 0 ? 0 : col0, c1 = col1 > W ? W : col1;      // (c0 >= c1: an empty crop, every sum stays 0)
    const fpcdr_div by_wc = fpcdr_make_div((uint32_t)Wc);
    const unsigned bx = (unsigned)fpcdr_cdiv((long long)H * Wc, 256);
    auto kern = img_is_float ? (mode == 0 ? k_compare_u8<true, 0> : k_compare_u8<true, 1>)
                             : (mode == 0 ? k_compare_u8<false, 0> : k_compare_u8<false, 1>);
    for_image_batches(n_images, [&](long long n0, unsigned ny) {
        hipLaunchKernelGGL(kern, dim3(bx, ny), dim3(256), 0, (hipStream_t)stream, img, scale, ref, heat, row_sums, n0, H, W, by_wc, c0, c1,
                           flip_rows ? 1 : 0);
    });
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

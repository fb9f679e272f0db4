// Overlay of re-rendered images on the captures, with the mesh's edges drawn from the rasteriser's own output (include/fpcdr.h,
// fpcdr_overlay_u8; reference src/torch/render_result_blended.py:149-154, the half-transparent blend, and its wireframe variant :58,
// :68-69, whose lines come from a painted texture that a user of this project does not have).  The rule is DESIGN.md 3, "Overlay rule":
// quantise the render as the comparison does, blend it with the capture in integers (weight in 1/256, round half to even), optionally
// keep the capture off the mesh, and paint a pixel in the wire colour where one of its triangle's three barycentrics b is within half a
// line width of zero to first order, b * b < hw2 * |grad b|^2 in unfused float32 -- bit for bit the numpy statement of
// tests/overlay_ref.py.
//
// Two decompositions of the same 16-pixel chunks meet in one kernel, because the inputs come in two widths:
//   * img, ref and out are 4, 1 and 3 bytes a pixel.  As in k_compare_u8 one thread OWNS 16 consecutive pixels of one output row, read
//     and written in the two forms of u8_chunk.h: four 16-byte loads of a float render (one of a uint8 one), one 16-byte load of the
//     capture and the 48 output bytes as three 16-byte stores.
//   * rast and rast_db are 16 bytes a pixel.  A thread that read them for its own 16 pixels would put the lanes of one load 256 bytes
//     apart.  Instead the wave walks its 64 chunks four at a time: in trip k lane l takes pixel l & 15 of chunk 4 k + (l >> 4), so the 16
//     lanes of a chunk read 256 consecutive bytes in one instruction (1 KiB a wave where the four chunks lie in one row).  The lane
//     loads rast, and -- only if the pixel is covered and a wire is asked for -- rast_db, and decides "covered" and "wire".
//   The exchange between the two is two bits a pixel, and it goes BETWEEN LANES, not through LDS: a ballot of each decision is a 64-bit
//   scalar that already holds the 16 bits of each of the trip's four chunks next to each other, so the owner of chunk c keeps
//   (ballot of trip c >> 2) >> 16 (c & 3) -- one compare, one 64-bit shift and two selects per trip, no LDS traffic, no barrier and no
//   bank conflicts to think about; an LDS table of the two bits would cost a write, a barrier and a read for the same 4 bytes a thread.
// What is read is decided by template arguments and uniform branches, not by lanes: RAST = 0 reads neither raster input (no wire, and
// nothing to keep off the mesh), RAST = 1 reads rast only (outside_capture without a wire), RAST = 2 reads rast and, for covered
// pixels, rast_db.  Every output byte is written once with a plain store; no atomics, no LDS, no private segment.
#include "u8_chunk.h"

namespace {

// four floats at p: one 16-byte load, or four 4-byte ones where the base is not 16-byte aligned (`aligned` is uniform)
__device__ __forceinline__ float4 load4(const float *p, bool aligned) {
    if (aligned) return *reinterpret_cast<const float4 *>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// b within half a line width of zero, to first order: float32, unfused (-ffp-contract=off), in exactly this order; false for a NaN
__device__ __forceinline__ bool wire_on(float b, float x, float y, float hw2) { return b * b < hw2 * ((x * x) + (y * y)); }

// four pixels (bytes of q and c; bit p of cov / wire = pixel p) -> their 12 output bytes in w0..w2
template <int RAST>
__device__ __forceinline__ void overlay4(uint32_t q, uint32_t c, int weight, uint32_t cov, uint32_t wire, bool outside_capture,
                                         uint32_t wire_rgb, uint32_t &w0, uint32_t &w1, uint32_t &w2) {
    uint32_t px[4];      // (constant indices only: registers)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t qq = (q >> (8 * p)) & 255u, cc = (c >> (8 * p)) & 255u;
        const uint32_t t = (uint32_t)weight * qq + (uint32_t)(256 - weight) * cc;       // <= 256 * 255
        uint32_t m = t >> 8;
        const uint32_t rem = t & 255u;
        m += (rem > 128u || (rem == 128u && (m & 1u))) ? 1u : 0u;                        // t / 256 rounded half to even
        if (RAST > 0 && outside_capture && !((cov >> p) & 1u)) m = cc;
        px[p] = m * 0x010101u;                                                           // bytes in memory order: channel 0 lowest
        if (RAST == 2 && ((wire >> p) & 1u)) px[p] = wire_rgb;
    }
    w0 = px[0] | px[1] << 24;
    w1 = px[1] >> 8 | px[2] << 16;
    w2 = px[2] >> 16 | px[3] << 8;
}

// grid: x over the H * Wc 16-pixel chunks of one image (Wc = ceil(W / 16)), y over the images of this launch (image number
// first_image + blockIdx.y: nothing 64-bit is divided per thread).  RAST = 2 is launched with hw2 > 0 only.
template <bool IS_FLOAT, int RAST>
__global__ void __launch_bounds__(256) k_overlay_u8(const void *__restrict__ img_, float scale, const uint8_t *__restrict__ ref,
                                                    const float *__restrict__ rast, const float *__restrict__ rast_db,
                                                    uint8_t *__restrict__ out, long long first_image, int H, int W, fpcdr_div by_wc,
                                                    int weight, int outside_capture, float hw2, uint32_t wire_rgb, int flip_rows) {
    const unsigned Wc = by_wc.d, total = (unsigned)H * Wc;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const long long n = first_image + blockIdx.y;

    // ---- the raster inputs: lane = pixel, four chunks a trip; the owner of a chunk keeps its 16 + 16 bits of the two ballots ----
    uint32_t covbits = 0u, wirebits = 0u;
    if (RAST > 0) {       // (every lane of the wave walks all 16 trips: the ballots are taken outside any divergent branch)
        const unsigned lane = threadIdx.x & 63u, wave_t0 = t - lane;
        const bool aligned = (((size_t)rast | (size_t)rast_db) & 15) == 0;      // uniform
        for (unsigned k0 = 0; k0 < 16u; k0 += 4u) {
            // four trips at a time, so that four loads of rast, then the loads of rast_db, are in flight together.  A lane without a
            // pixel (past the image's chunks, or past W in a row tail) reads the image's nearest pixel instead and decides nothing:
            // the loads of rast are unconditional, and nothing of their result shows.
            long long at[4];
            float4 r[4], d[4];
            bool cov[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned tt = wave_t0 + 4u * (k0 + q) + (lane >> 4);
                const unsigned tc = tt < total ? tt : total - 1u;
                const int ii = (int)fpcdr_divide(tc, by_wc);
                const int jj = (int)(tc - (unsigned)ii * Wc) * 16 + (int)(lane & 15u);
                // row ii of the output is row H - 1 - ii of a raster with row 0 at the bottom
                at[q] = ((n * H + (flip_rows ? H - 1 - ii : ii)) * W + (jj < W ? jj : W - 1)) * 4;
                r[q] = load4(rast + at[q], aligned);
                cov[q] = tt < total && jj < W;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                cov[q] = cov[q] && r[q].w > 0.0f;
                d[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (RAST == 2 && cov[q]) d[q] = load4(rast_db + at[q], aligned);      // (du/dX, du/dY, dv/dX, dv/dY)
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bool wire = false;
                if (RAST == 2) {
                    const float s = (1.0f - r[q].x) - r[q].y;
                    const float b2 = s < 0.0f ? 0.0f : s;                 // (a select: a NaN stays a NaN)
                    const float gx = d[q].x + d[q].z, gy = d[q].y + d[q].w;
                    wire = cov[q] && (wire_on(r[q].x, d[q].x, d[q].y, hw2) || wire_on(r[q].y, d[q].z, d[q].w, hw2) || wire_on(b2, gx, gy, hw2));
                }
                const unsigned long long cm = __ballot(cov[q]), wm = __ballot(wire);
                if ((lane >> 2) == k0 + q) {
                    const unsigned sh = 16u * (lane & 3u);
                    covbits = (uint32_t)(cm >> sh) & 0xffffu;
                    wirebits = (uint32_t)(wm >> sh) & 0xffffu;
                }
            }
        }
    }
    if (t >= total) return;

    const int i = (int)fpcdr_divide(t, by_wc);
    const int j0 = (int)(t - (unsigned)i * Wc) * 16;
    const bool whole = j0 + 16 <= W;
    // the capture: row i.  The rendered image: row i, or H - 1 - i of a raster with row 0 at the bottom.  Pixels past W are not written
    uint32_t cw[4] = {0u, 0u, 0u, 0u}, qw[4] = {0u, 0u, 0u, 0u};
    load_chunk_u8(ref + (n * H + i) * W + j0, whole, j0, W, cw);
    load_chunk_render<IS_FLOAT>(img_, (n * H + (flip_rows ? H - 1 - i : i)) * W + j0, scale, whole, j0, W, qw);
    // ---- blend, coverage, wire: the 48 output bytes ----
    uint32_t w[12];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        overlay4<RAST>(qw[g], cw[g], weight, covbits >> (4 * g), wirebits >> (4 * g), outside_capture != 0, wire_rgb, w[3 * g], w[3 * g + 1],
                       w[3 * g + 2]);
    store_chunk_rgb(out + ((n * H + i) * W + j0) * 3, whole, j0, W, w);
}

template <bool IS_FLOAT>
auto pick(int rast_mode) {
    return rast_mode == 0 ? k_overlay_u8<IS_FLOAT, 0> : rast_mode == 1 ? k_overlay_u8<IS_FLOAT, 1> : k_overlay_u8<IS_FLOAT, 2>;
}

}  // namespace

extern "C" int fpcdr_overlay_u8(const void *img, int img_is_float, float scale, const uint8_t *ref, const float *rast, const float *rast_db,
                                uint8_t *out, int64_t n_images, int H, int W, int weight_256, int outside_capture, float wire_hw2,
                                uint32_t wire_rgb, int flip_rows, void *stream) {
    FPCDR_REQUIRE(img != nullptr && ref != nullptr && out != nullptr, "null pointer");
    FPCDR_REQUIRE(n_images > 0 && H > 0 && W > 0, "sizes must be positive");
    const int Wc = fpcdr_cdiv(W, 16);
    FPCDR_REQUIRE((long long)H * Wc <= (1LL << 31) - 256, "image too large");
    FPCDR_REQUIRE(weight_256 >= 0 && weight_256 <= 256, "weight_256 must lie in [0, 256]");
    FPCDR_REQUIRE(wire_hw2 >= 0.0f && wire_hw2 <= 3.4028234663852886e38f, "wire_hw2 must be finite and >= 0");      // (false for a NaN)
    FPCDR_REQUIRE(!(wire_hw2 > 0.0f) || (rast != nullptr && rast_db != nullptr), "a wire (wire_hw2 > 0) needs rast and rast_db");
    FPCDR_REQUIRE(!outside_capture || rast != nullptr, "outside_capture needs rast");
    FPCDR_REQUIRE(((uintptr_t)rast & 3) == 0 && ((uintptr_t)rast_db & 3) == 0 && (!img_is_float || ((uintptr_t)img & 3) == 0),
                  "float buffers must be 4-byte aligned");
    FPCDR_REQUIRE((wire_rgb >> 24) == 0, "wire_rgb is r | g << 8 | b << 16");
    const size_t px = (size_t)n_images * H * W;
    const size_t img_bytes = px * (img_is_float ? 4 : 1);
    FPCDR_REQUIRE(!overlap(out, px * 3, img, img_bytes) && !overlap(out, px * 3, ref, px) && !overlap(out, px * 3, rast, px * 16) &&
                  !overlap(out, px * 3, rast_db, px * 16), "out overlaps an input");
    // what is read: nothing of the raster without a wire and with nothing to keep off the mesh; rast_db only for a wire
    const int rast_mode = wire_hw2 > 0.0f ? 2 : outside_capture ? 1 : 0;
    const fpcdr_div by_wc = fpcdr_make_div((uint32_t)Wc);
    const unsigned bx = (unsigned)fpcdr_cdiv((long long)H * Wc, 256);
    auto kern = img_is_float ? pick<true>(rast_mode) : pick<false>(rast_mode);
    for_image_batches(n_images, [&](long long n0, unsigned ny) {
        hipLaunchKernelGGL(kern, dim3(bx, ny), dim3(256), 0, (hipStream_t)stream, img, scale, ref, rast, rast_db, out, n0, H, W, by_wc,
                           weight_256, outside_capture ? 1 : 0, wire_hw2, wire_rgb, flip_rows ? 1 : 0);
    });
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

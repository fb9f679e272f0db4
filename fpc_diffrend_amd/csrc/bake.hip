// A start texture baked from the captures (include/fpcdr.h: fpcdr_bake_accumulate_u8, fpcdr_bake_resolve, fpcdr_bake_dilate).  The rule
// is DESIGN.md 3, "Bake rule": every covered pixel of every view splats its capture into the four texels the 'linear' texture lookup
// would read for it (make_taps of texsample.h: the forward's own indices and fractions), with the bilinear weights quantised to 1/256 per
// axis; a texel's value is the weighted mean of what landed on it, and unfilled texels next to filled ones take the mean of those
// neighbours.  The sums are 64-bit INTEGERS: adds commute, so the result does not depend on the order of the launches, of the lanes or
// of the ranks that share the frames -- bit for bit the numpy statement of tests/bake_ref.py.
//
// k_bake_accumulate: one lane per pixel.  A lane reads its pixel's rast.w (4 bytes) and leaves if the pixel is not covered; a covered
// one reads its texture coordinate (one 8-byte load where the base is 8-byte aligned, two 4-byte loads otherwise), its capture byte, and
// issues up to eight 64-bit integer atomics without a return value: (num, den) of a texel sit side by side in one 16-byte slot.  Taps of
// weight 0 are skipped.  k_bake_resolve, k_bake_dilate: one lane per texel, plain loads and stores.  No LDS, no private segment.
#include "texsample.h"
#include "u8_chunk.h"

namespace {

__device__ __forceinline__ bool covered(const float *w) { return *w > 0.0f; }      // (false for a NaN)

// grid: x over the H * W pixels of one image, y over the images of this launch (image number first_image + blockIdx.y)
__global__ void __launch_bounds__(256) k_bake_accumulate(const float *__restrict__ texc, const float *__restrict__ rast,
                                                         const uint8_t *__restrict__ ref, unsigned long long *__restrict__ acc,
                                                         long long first_image, int H, int W, fpcdr_div by_w, int Ht, int Wt, int mode,
                                                         int interior_only, int flip_rows, int texc_8b) {
    const unsigned total = (unsigned)H * (unsigned)W;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    const long long p = (first_image + blockIdx.y) * (long long)total + t;      // pixel number in the batch
    const float *rw = rast + p * 4 + 3;
    if (!covered(rw)) return;
    const int i = (int)fpcdr_divide(t, by_w), j = (int)(t - (unsigned)i * (unsigned)W);
    if (interior_only) {      // the four neighbours that lie inside the image are covered too
        bool in = true;
        if (i > 0) in = in && covered(rw - 4 * (long long)W);
        if (i < H - 1) in = in && covered(rw + 4 * (long long)W);
        if (j > 0) in = in && covered(rw - 4);
        if (j < W - 1) in = in && covered(rw + 4);
        if (!in) return;
    }
    float u, v;
    if (texc_8b) {
        const float2 q = *reinterpret_cast<const float2 *>(texc + p * 2);
        u = q.x; v = q.y;
    } else {
        u = texc[p * 2]; v = texc[p * 2 + 1];
    }
    if (!(__builtin_isfinite(u) && __builtin_isfinite(v))) return;
    const unsigned c = ref[p + ((flip_rows ? H - 1 - i : i) - i) * (long long)W];      // the flip applies to ref only
    const Taps tp = make_taps(u, v, Ht, Wt, 1, mode);
    // exact: fx, fy lie in [0, 1] (1.0f where x - floor(x) rounds up), their products with 256 are exact, floor is exact
    const unsigned ax = (unsigned)(int)floorf(tp.fx * 256.0f), ay = (unsigned)(int)floorf(tp.fy * 256.0f);
    const unsigned bx = 256u - ax, by = 256u - ay;
    auto add = [&](int texel, unsigned w) {
        if (w == 0u) return;
        unsigned long long *slot = acc + 2 * (size_t)texel;
        atomicAdd(slot, (unsigned long long)(w * c));          // (w * c <= 65536 * 255: no overflow in 32 bits)
        atomicAdd(slot + 1, (unsigned long long)w);
    };
    add(tp.i00, bx * by);
    add(tp.i10, ax * by);
    add(tp.i01, bx * ay);
    add(tp.i11, ax * ay);
}

__global__ void __launch_bounds__(256) k_bake_resolve(const unsigned long long *__restrict__ acc, float *__restrict__ tex,
                                                      uint8_t *__restrict__ filled, unsigned n_texels, double color_scale,
                                                      unsigned long long min_den, int acc_16b) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_texels) return;
    unsigned long long num, den;
    if (acc_16b) {
        const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(acc + 2 * (size_t)t);
        num = q.x; den = q.y;
    } else {
        num = acc[2 * (size_t)t]; den = acc[2 * (size_t)t + 1];
    }
    const bool f = den >= min_den;
    tex[t] = f ? (float)((double)num / ((double)den * color_scale)) : 0.0f;      // one multiply, one division, one rounding to float
    filled[t] = f ? 1 : 0;
}

// one Jacobi pass: reads tex_in / filled_in only
__global__ void __launch_bounds__(256) k_bake_dilate(const float *__restrict__ tex_in, const uint8_t *__restrict__ filled_in,
                                                     float *__restrict__ tex_out, uint8_t *__restrict__ filled_out, int Ht, int Wt,
                                                     fpcdr_div by_wt) {
    const unsigned n_texels = (unsigned)Ht * (unsigned)Wt;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n_texels) return;
    float val = tex_in[t];
    uint8_t f = filled_in[t];
    if (!f) {
        const int y = (int)fpcdr_divide(t, by_wt), x = (int)(t - (unsigned)y * (unsigned)Wt);
        float sum = 0.0f;
        int count = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = y + dy, xx = x + dx;
                if (yy < 0 || yy >= Ht || xx < 0 || xx >= Wt) continue;      // (no wrap: a chart's gutter is local)
                const unsigned s = (unsigned)yy * (unsigned)Wt + (unsigned)xx;
                if (filled_in[s]) { sum += tex_in[s]; ++count; }
            }
        }
        if (count > 0) { val = sum / (float)count; f = 1; }
    }
    tex_out[t] = val;
    filled_out[t] = f;
}

}  // namespace

extern "C" int fpcdr_bake_accumulate_u8(const float *texc, const float *rast, const uint8_t *ref, uint64_t *acc, int64_t n_images, int H,
                                        int W, int Ht, int Wt, int boundary_mode, int interior_only, int flip_rows, void *stream) {
    FPCDR_REQUIRE(texc != nullptr && rast != nullptr && ref != nullptr && acc != nullptr, "null pointer");
    FPCDR_REQUIRE(n_images > 0 && H > 0 && W > 0 && Ht > 0 && Wt > 0, "sizes must be positive");
    FPCDR_REQUIRE(boundary_mode == FPCDR_BOUNDARY_WRAP || boundary_mode == FPCDR_BOUNDARY_CLAMP, "boundary_mode must be wrap or clamp");
    FPCDR_REQUIRE(((uintptr_t)acc & 7) == 0, "acc must be 8-byte aligned");
    FPCDR_REQUIRE(((uintptr_t)texc & 3) == 0 && ((uintptr_t)rast & 3) == 0, "texc and rast must be 4-byte aligned");
    FPCDR_REQUIRE((long long)H * W <= (1LL << 31) - 256, "image too large");
    FPCDR_REQUIRE((long long)Ht * Wt <= (1LL << 30), "texture too large");
    const size_t px = (size_t)n_images * H * W, acc_bytes = (size_t)Ht * Wt * 16;
    FPCDR_REQUIRE(!overlap(acc, acc_bytes, texc, px * 8) && !overlap(acc, acc_bytes, rast, px * 16) && !overlap(acc, acc_bytes, ref, px),
                  "acc overlaps an input");
    const fpcdr_div by_w = fpcdr_make_div((uint32_t)W);
    const unsigned bx = (unsigned)fpcdr_cdiv((long long)H * W, 256);
    const int texc_8b = ((uintptr_t)texc & 7) == 0 ? 1 : 0;
    for_image_batches(n_images, [&](long long n0, unsigned ny) {
        hipLaunchKernelGGL(k_bake_accumulate, dim3(bx, ny), dim3(256), 0, (hipStream_t)stream, texc, rast, ref,
                           reinterpret_cast<unsigned long long *>(acc), n0, H, W, by_w, Ht, Wt, boundary_mode, interior_only ? 1 : 0,
                           flip_rows ? 1 : 0, texc_8b);
    });
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_bake_resolve(const uint64_t *acc, float *tex, uint8_t *filled, int Ht, int Wt, double color_scale, uint64_t min_den,
                                  void *stream) {
    FPCDR_REQUIRE(acc != nullptr && tex != nullptr && filled != nullptr, "null pointer");
    FPCDR_REQUIRE(Ht > 0 && Wt > 0, "sizes must be positive");
    FPCDR_REQUIRE(min_den >= 1, "min_den must be at least 1");
    FPCDR_REQUIRE(((uintptr_t)acc & 7) == 0, "acc must be 8-byte aligned");
    FPCDR_REQUIRE(((uintptr_t)tex & 3) == 0, "tex must be 4-byte aligned");
    FPCDR_REQUIRE((long long)Ht * Wt <= (1LL << 30), "texture too large");
    FPCDR_REQUIRE(color_scale > 0.0 && color_scale <= 1.7976931348623157e308, "color_scale must be positive and finite");
    const size_t n = (size_t)Ht * Wt;
    FPCDR_REQUIRE(!overlap(tex, n * 4, acc, n * 16) && !overlap(filled, n, acc, n * 16) && !overlap(tex, n * 4, filled, n),
                  "tex, filled and acc overlap");
    hipLaunchKernelGGL(k_bake_resolve, dim3((unsigned)fpcdr_cdiv((long long)n, 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long *>(acc), tex, filled, (unsigned)n, color_scale, (unsigned long long)min_den,
                       ((uintptr_t)acc & 15) == 0 ? 1 : 0);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_bake_dilate(const float *tex_in, const uint8_t *filled_in, float *tex_out, uint8_t *filled_out, int Ht, int Wt,
                                 void *stream) {
    FPCDR_REQUIRE(tex_in != nullptr && filled_in != nullptr && tex_out != nullptr && filled_out != nullptr, "null pointer");
    FPCDR_REQUIRE(Ht > 0 && Wt > 0, "sizes must be positive");
    FPCDR_REQUIRE(((uintptr_t)tex_in & 3) == 0 && ((uintptr_t)tex_out & 3) == 0, "tex_in and tex_out must be 4-byte aligned");
    FPCDR_REQUIRE((long long)Ht * Wt <= (1LL << 30), "texture too large");
    const size_t n = (size_t)Ht * Wt;
    FPCDR_REQUIRE(!overlap(tex_out, n * 4, tex_in, n * 4) && !overlap(tex_out, n * 4, filled_in, n) && !overlap(filled_out, n, tex_in, n * 4) &&
                  !overlap(filled_out, n, filled_in, n) && !overlap(tex_out, n * 4, filled_out, n),
                  "an output overlaps an input or the other output: a pass reads only its input buffers");
    hipLaunchKernelGGL(k_bake_dilate, dim3((unsigned)fpcdr_cdiv((long long)n, 256)), dim3(256), 0, (hipStream_t)stream, tex_in, filled_in,
                       tex_out, filled_out, Ht, Wt, fpcdr_make_div((uint32_t)Wt));
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

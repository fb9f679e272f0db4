// Box reduction of the captures for a resolution pyramid (include/fpcdr.h, fpcdr_downsample_u8).  The rule is DESIGN.md 3, "Downsample
// rule": the output pixel is the exact mean of its s x s source block, rounded half up, rounded once -- (2 * sum + s * s) / (2 * s * s)
// in integers, bit for bit the numpy statement of tests/downsample_ref.py.  Rows are not flipped.
//
// A streaming kernel in the style of k_compare_u8: one thread owns 16 consecutive pixels of one OUTPUT row, i.e. S source rows of 16 * S
// consecutive bytes, which it reads once, row by row, as S 16-byte loads where the row's address allows and element by element in a row
// tail or at an unaligned base (u8_chunk.h; the S chunks of a row are 16 bytes apart, so ONE test serves the row and its loads leave
// together).  The bytes of a word are summed with word arithmetic: for S = 2 a mask-and-add leaves the two pair sums of a word in its
// 16-bit halves, which are then added over the two rows as they are; for S >= 3 a word holds bytes of at most two outputs, and each part
// goes through v_sad_u8 (sum of |byte - 0| over the word, added to the accumulator) behind a compile-time mask -- a whole word, no mask,
// where S is a multiple of 4.  S is a template parameter, so which output a byte belongs to is known at compile time and every array
// index is a constant: registers, no LDS, no private segment.  The 16 results leave as one 16-byte store where whole and aligned.
#include "u8_chunk.h"

namespace {

// S 16-byte chunks of one source row at p -> w[0 .. 4 * S) (zeroed by the caller).  col0: the source column of p; bytes at or past W stay 0
template <int S>
__device__ __forceinline__ void load_row(const uint8_t *p, bool whole, int col0, int W, uint32_t (&w)[4 * S]) {
    if (whole && ((size_t)p & 15) == 0) {
        const uint4 *p4 = reinterpret_cast<const uint4 *>(p);
        uint4 v[S];
#pragma unroll
        for (int c = 0; c < S; ++c) v[c] = p4[c];
#pragma unroll
        for (int c = 0; c < S; ++c) { w[4 * c] = v[c].x; w[4 * c + 1] = v[c].y; w[4 * c + 2] = v[c].z; w[4 * c + 3] = v[c].w; }
    } else {
#pragma unroll
        for (int c = 0; c < S; ++c) {
            uint32_t q[4] = {w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]};
            load_chunk_u8(p + 16 * c, false, col0 + 16 * c, W, q);
            w[4 * c] = q[0]; w[4 * c + 1] = q[1]; w[4 * c + 2] = q[2]; w[4 * c + 3] = q[3];
        }
    }
}

// 16 output bytes in o[0..3] -> p
__device__ __forceinline__ void store_chunk_u8(uint8_t *p, bool whole, int j0, int W, const uint32_t (&o)[4]) {
    if (whole && ((size_t)p & 15) == 0) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (j0 + k < W) p[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
}

// the bytes b of a word (0..3) that lie in [lo, hi) as a mask of whole bytes
constexpr uint32_t byte_mask(int lo, int hi) {
    uint32_t m = 0u;
    for (int b = 0; b < 4; ++b)
        if (b >= lo && b < hi) m |= 255u << (8 * b);
    return m;
}

// grid: x over the Ho * Wc 16-pixel chunks of one output image (Wc = ceil(Wo / 16)), y over the images of this launch (image number
// first_image + blockIdx.y).  H = Ho * S, W = Wo * S: the host has checked it.
template <int S>
__global__ void __launch_bounds__(256) k_downsample_u8(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, long long first_image,
                                                       int Ho, int Wo, fpcdr_div by_wc) {
    const unsigned Wc = by_wc.d, total = (unsigned)Ho * Wc;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    const int i = (int)fpcdr_divide(t, by_wc);
    const int j0 = (int)(t - (unsigned)i * Wc) * 16;
    const long long n = first_image + blockIdx.y;
    const bool whole = j0 + 16 <= Wo;              // (then the 16 * S source bytes of every row exist as well)
    const int W = Wo * S;
    const uint8_t *p = src + ((n * Ho + i) * S) * (long long)W + (long long)j0 * S;
    uint32_t out[4];

    if constexpr (S == 2) {
        // ---- pairs: (w & 0x00ff00ff) + ((w >> 8) & 0x00ff00ff) = the sums of bytes (0, 1) and (2, 3) in the 16-bit halves ----
        uint32_t acc[8];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            uint32_t w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            load_row<2>(p + (long long)a * W, whole, j0 * 2, W, w);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const uint32_t h = (w[m] & 0x00ff00ffu) + ((w[m] >> 8) & 0x00ff00ffu);
                acc[m] = a == 0 ? h : acc[m] + h;          // (a half holds at most 4 * 255)
            }
        }
        // (2 * sum + 4) / 8 = (sum + 2) >> 2, on both halves at once: at most 1022 a half, no carry between them
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t x = ((acc[2 * g] + 0x00020002u) >> 2) & 0x00ff00ffu, y = ((acc[2 * g + 1] + 0x00020002u) >> 2) & 0x00ff00ffu;
            out[g] = (x & 255u) | (x >> 16) << 8 | (y & 255u) << 16 | (y >> 16) << 24;
        }
    } else {
        uint32_t acc[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0u;
        // (rows one after the other for the large factors: S * S loads in flight would cost the registers that hide their latency)
        constexpr int ROWS_UNROLLED = S <= 4 ? S : 1;
#pragma unroll ROWS_UNROLLED
        for (int a = 0; a < S; ++a) {
            uint32_t w[4 * S];
#pragma unroll
            for (int m = 0; m < 4 * S; ++m) w[m] = 0u;
            load_row<S>(p + (long long)a * W, whole, j0 * S, W, w);
#pragma unroll
            for (int m = 0; m < 4 * S; ++m) {
                // word m holds the row's bytes 4m .. 4m + 3: those of output k0 = 4m / S, and from byte `cut` on of output k0 + 1
                const int k0 = (4 * m) / S, cut = (k0 + 1) * S - 4 * m;        // (constants after unrolling)
                if (cut >= 4) {
                    acc[k0] = __builtin_amdgcn_sad_u8(w[m], 0u, acc[k0]);
                } else {
                    acc[k0] = __builtin_amdgcn_sad_u8(w[m] & byte_mask(0, cut), 0u, acc[k0]);
                    acc[k0 + 1] = __builtin_amdgcn_sad_u8(w[m] & byte_mask(cut, 4), 0u, acc[k0 + 1]);
                }
            }
        }
        // a sum is at most 255 * S * S <= 65 280: 2 * sum + S * S fits easily; the divisor is a constant (a multiply-high)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint32_t o = 0u;
#pragma unroll
            for (int b = 0; b < 4; ++b) o |= ((2u * acc[4 * g + b] + (uint32_t)(S * S)) / (uint32_t)(2 * S * S)) << (8 * b);
            out[g] = o;
        }
    }
    store_chunk_u8(dst + (n * Ho + i) * (long long)Wo + j0, whole, j0, Wo, out);
}

}  // namespace

extern "C" int fpcdr_downsample_u8(const uint8_t *src, uint8_t *dst, int64_t n_images, int H, int W, int s, void *stream) {
    FPCDR_REQUIRE(n_images >= 0 && H > 0 && W > 0, "n_images must not be negative, H and W must be positive");
    FPCDR_REQUIRE(s >= 2 && s <= 16, "the factor s must lie in 2..16");
    FPCDR_REQUIRE(H % s == 0 && W % s == 0, "H and W must be multiples of the factor s");
    if (n_images == 0) return FPCDR_OK;
    FPCDR_REQUIRE(src != nullptr && dst != nullptr, "null pointer");
    const int Ho = H / s, Wo = W / s;
    const int Wc = fpcdr_cdiv(Wo, 16);
    FPCDR_REQUIRE((long long)Ho * Wc <= (1LL << 31) - 256, "image too large");
    FPCDR_REQUIRE(!overlap(dst, (size_t)n_images * Ho * Wo, src, (size_t)n_images * H * W), "dst overlaps src");
    const fpcdr_div by_wc = fpcdr_make_div((uint32_t)Wc);
    const unsigned bx = (unsigned)fpcdr_cdiv((long long)Ho * Wc, 256);
    void (*kern)(const uint8_t *, uint8_t *, long long, int, int, fpcdr_div) = nullptr;
    switch (s) {
#define FPCDR_DS_CASE(S) case S: kern = k_downsample_u8<S>; break;
        FPCDR_DS_CASE(2) FPCDR_DS_CASE(3) FPCDR_DS_CASE(4) FPCDR_DS_CASE(5) FPCDR_DS_CASE(6) FPCDR_DS_CASE(7) FPCDR_DS_CASE(8) FPCDR_DS_CASE(9)
        FPCDR_DS_CASE(10) FPCDR_DS_CASE(11) FPCDR_DS_CASE(12) FPCDR_DS_CASE(13) FPCDR_DS_CASE(14) FPCDR_DS_CASE(15) FPCDR_DS_CASE(16)
#undef FPCDR_DS_CASE
    }
    for_image_batches(n_images, [&](long long n0, unsigned ny) {
        hipLaunchKernelGGL(kern, dim3(bx, ny), dim3(256), 0, (hipStream_t)stream, src, dst, n0, Ho, Wo, by_wc);
    });
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

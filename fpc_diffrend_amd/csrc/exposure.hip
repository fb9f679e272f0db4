// Per-camera exposure from the fit's own render (include/fpcdr.h: fpcdr_exposure_sums, fpcdr_apply_lut_u8).  The rule is DESIGN.md 3,
// "Exposure rule": over the interior covered pixels of every image, the six integer moments (n, sum r, sum t, sum r^2, sum t^2, sum r t)
// of the render byte r = quantise(colour, 255) and the capture byte t; the gains, offsets and 256-entry tables are fitted from them on the
// host, and the tables are applied to the captures in place.  Integers throughout, 64-bit sums: adds commute, so the result does not
// depend on the order of the launches, of the lanes or of the ranks that share the images -- bit for bit the numpy statement of
// tests/exposure_ref.py.
//
// k_exposure_sums: one thread owns 16 consecutive pixels of one row (u8_chunk.h).  It reads the coverage (rast.w, 4 bytes a pixel) of
// its own 18 columns and, only where one of its pixels is covered, of the rows above and below; the capture (and the mask) as one 16-byte
// load where whole and aligned; the 16 * C floats of the colour as 4 * C 16-byte loads, only where a pixel counts.  Six 32-bit partial
// sums per thread (16 * C <= 64 samples of at most 255^2), summed over the wave with DPP row operations, over the four waves through
// LDS, then ONE 64-bit integer atomic per sum and workgroup -- none for a workgroup without a counted sample.  Constant indices only:
// registers, no private segment, no float atomics.
// k_apply_lut_u8: one thread owns 16 consecutive bytes of one image; the camera's 256-byte table is staged in LDS once per workgroup.
#include <vector>

#include "u8_chunk.h"

namespace {

__device__ __forceinline__ bool covered(float w) { return w > 0.0f; }      // (false for a NaN)

// full-wave unsigned sum with DPP row operations (wave_sum_dpp's steps on integers); valid in lane 63
__device__ __forceinline__ uint32_t wave_sum_u32_lane63(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
    return v;
}

// 16 output bytes in o[0..3] -> p
__device__ __forceinline__ void store_chunk_bytes(uint8_t *p, bool whole, int j0, int W, const uint32_t (&o)[4]) {
    if (whole && ((size_t)p & 15) == 0) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (j0 + k < W) p[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
}

// grid: x over the H * Wc 16-pixel chunks of one image (Wc = ceil(W / 16)), y over the images of this launch (image number
// first_image + blockIdx.y)
template <int C>
__global__ void __launch_bounds__(256) k_exposure_sums(const float *__restrict__ colour, const float *__restrict__ rast,
                                                       const uint8_t *__restrict__ ref, const uint8_t *__restrict__ mask,
                                                       const float *__restrict__ face_w, int T, int lo, int hi,
                                                       unsigned long long *__restrict__ sums, long long first_image, int H, int W,
                                                       fpcdr_div by_wc) {
    __shared__ uint32_t part[4][6];
    const unsigned Wc = by_wc.d, total = (unsigned)H * Wc;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const long long n = first_image + blockIdx.y;
    uint32_t s[6] = {0u, 0u, 0u, 0u, 0u, 0u};      // n, sum r, sum t, sum r^2, sum t^2, sum r t

    if (t < total) {
        const int i = (int)fpcdr_divide(t, by_wc);
        const int j0 = (int)(t - (unsigned)i * Wc) * 16;
        const bool whole = j0 + 16 <= W;
        const long long p0 = (n * H + i) * (long long)W + j0;      // the chunk's first pixel in the batch
        const float *rw = rast + p0 * 4 + 3;
        // ---- coverage of columns j0 - 1 .. j0 + 16 of this row: bit k + 1 = column j0 + k; a column outside the image asks nothing ----
        float wv[16];      // (the ids of the face weights)
        uint32_t cen = 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            wv[k] = j0 + k < W ? rw[4 * k] : 0.0f;
            cen |= (covered(wv[k]) ? 1u : 0u) << (k + 1);
        }
        uint32_t m = (cen >> 1) & 0xffffu;
        if (m) {
            const uint32_t outside = ~(W - j0 >= 17 ? 0x3ffffu : (1u << (W - j0 + 1)) - 1u);      // columns >= W: bits W - j0 + 1 and up
            uint32_t side = cen | outside;
            side |= (j0 == 0 || covered(rw[-4])) ? 1u : 0u;
            if (j0 + 16 < W && covered(rw[64])) side |= 1u << 17;
            m &= side & (side >> 2);      // left and right neighbours
            if (i > 0) {
                uint32_t up = 0u;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (j0 + k < W) up |= (covered(rw[4 * k - 4 * (long long)W]) ? 1u : 0u) << k;
                m &= up;
            }
            if (i < H - 1) {
                uint32_t dn = 0u;
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (j0 + k < W) dn |= (covered(rw[4 * k + 4 * (long long)W]) ? 1u : 0u) << k;
                m &= dn;
            }
        }
        uint32_t tw[4] = {0u, 0u, 0u, 0u};
        if (m) {
            // ---- the capture bytes, lo <= t <= hi; the mask's byte >= 128; the face's weight > 0 ----
            load_chunk_u8(ref + p0, whole, j0, W, tw);
            uint32_t mw[4] = {0u, 0u, 0u, 0u};
            if (mask) load_chunk_u8(mask + p0, whole, j0, W, mw);
            uint32_t ok = 0u;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int tv = (int)((tw[k >> 2] >> (8 * (k & 3))) & 255u);
                bool in = tv >= lo && tv <= hi;
                if (mask) in = in && ((mw[k >> 2] >> (8 * (k & 3))) & 128u) != 0u;
                ok |= (in ? 1u : 0u) << k;
            }
            m &= ok;
            if (face_w) {
                uint32_t fw = 0u;
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if ((m >> k) & 1u) {
                        const int id = (int)wv[k];
                        // (an id past the table does not count, and reads nothing out of bounds)
                        if ((unsigned)(id - 1) < (unsigned)T && face_w[id - 1] > 0.0f) fw |= 1u << k;
                    }
                }
                m &= fw;
            }
        }
        if (m) {
            // ---- the render bytes of the pixels that count: element e of the chunk's 16 * C floats is channel e % C of pixel e / C ----
            const float *cp = colour + p0 * C;
            auto add = [&](int k, float v) {
                if ((m >> k) & 1u) {
                    const uint32_t r = quantise(v, 255.0f), tv = (tw[k >> 2] >> (8 * (k & 3))) & 255u;
                    s[0] += 1u; s[1] += r; s[2] += tv; s[3] += r * r; s[4] += tv * tv; s[5] += r * tv;
                }
            };
            if (whole && ((size_t)cp & 15) == 0) {
                const float4 *c4 = reinterpret_cast<const float4 *>(cp);
#pragma unroll
                for (int q = 0; q < 4 * C; ++q) {
                    const float4 v = c4[q];
                    add((4 * q) / C, v.x); add((4 * q + 1) / C, v.y); add((4 * q + 2) / C, v.z); add((4 * q + 3) / C, v.w);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16 * C; ++e)
                    if (j0 + e / C < W) add(e / C, cp[e]);
            }
        }
    }
    // ---- wave by wave, then across the four waves through LDS: one 64-bit integer atomic per sum and workgroup ----
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const uint32_t v = wave_sum_u32_lane63(s[q]);      // (at most 64 * 64 * 255^2 < 2^32)
        if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const unsigned long long v = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v != 0ull) atomicAdd(sums + n * 6 + threadIdx.x, v);
    }
}

// grid: x over the ceil(HW / 16) 16-byte chunks of one image in turns of 256, y over the images of this launch.  An image whose camera
// is outside [0, Nl) is left as it is (uniform over the workgroup: the barrier is reached by every thread or by none)
__global__ void __launch_bounds__(256) k_apply_lut_u8(uint8_t *__restrict__ images, const uint8_t *__restrict__ lut,
                                                      const int32_t *__restrict__ cam_of_image, int Nl, long long first_image,
                                                      long long HW) {
    __shared__ uint8_t table[256];
    const long long n = first_image + blockIdx.y;
    const int cam = cam_of_image[n];
    if (cam < 0 || cam >= Nl) return;
    table[threadIdx.x] = lut[(size_t)cam * 256 + threadIdx.x];
    __syncthreads();
    const long long c = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;      // the chunk's first byte in its image
    if (c >= HW) return;
    const bool whole = c + 16 <= HW;
    const int left = whole ? 16 : (int)(HW - c);      // (the "row" of u8_chunk.h is the image: columns 0 .. left of this chunk)
    uint8_t *p = images + n * HW + c;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    load_chunk_u8(p, whole, 0, left, w);
    uint32_t o[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        o[g] = (uint32_t)table[w[g] & 255u] | (uint32_t)table[(w[g] >> 8) & 255u] << 8 | (uint32_t)table[(w[g] >> 16) & 255u] << 16 |
               (uint32_t)table[w[g] >> 24] << 24;
    store_chunk_bytes(p, whole, 0, left, o);
}

}  // namespace

extern "C" int fpcdr_exposure_sums(const float *colour, const float *rast, const uint8_t *ref, const uint8_t *mask, const float *face_w,
                                   int T, int lo, int hi, int64_t n_images, int H, int W, int C, int64_t *sums, void *stream) {
    FPCDR_REQUIRE(colour != nullptr && rast != nullptr && ref != nullptr && sums != nullptr, "null pointer");
    FPCDR_REQUIRE(n_images > 0 && H > 0 && W > 0, "sizes must be positive");
    FPCDR_REQUIRE(C >= 1 && C <= 4, "C must lie in 1..4");
    FPCDR_REQUIRE(0 <= lo && lo <= hi && hi <= 255, "0 <= lo <= hi <= 255 is required");
    FPCDR_REQUIRE(!face_w || T > 0, "face_w needs T > 0");
    FPCDR_REQUIRE(((uintptr_t)sums & 7) == 0, "sums must be 8-byte aligned");
    FPCDR_REQUIRE(((uintptr_t)colour & 3) == 0 && ((uintptr_t)rast & 3) == 0 && ((uintptr_t)face_w & 3) == 0,
                  "colour, rast and face_w must be 4-byte aligned");
    const int Wc = fpcdr_cdiv(W, 16);
    FPCDR_REQUIRE((long long)H * Wc <= (1LL << 31) - 256, "image too large");
    const size_t px = (size_t)n_images * H * W, sums_bytes = (size_t)n_images * 48;
    FPCDR_REQUIRE(!overlap(sums, sums_bytes, colour, px * C * 4) && !overlap(sums, sums_bytes, rast, px * 16) &&
                  !overlap(sums, sums_bytes, ref, px) && !overlap(sums, sums_bytes, mask, px) &&
                  !overlap(sums, sums_bytes, face_w, face_w ? (size_t)T * 4 : 0), "sums overlaps an input");
    const fpcdr_div by_wc = fpcdr_make_div((uint32_t)Wc);
    const unsigned bx = (unsigned)fpcdr_cdiv((long long)H * Wc, 256);
    auto kern = C == 1 ? k_exposure_sums<1> : C == 2 ? k_exposure_sums<2> : C == 3 ? k_exposure_sums<3> : k_exposure_sums<4>;
    for_image_batches(n_images, [&](long long n0, unsigned ny) {
        hipLaunchKernelGGL(kern, dim3(bx, ny), dim3(256), 0, (hipStream_t)stream, colour, rast, ref, mask, face_w, face_w ? T : 0, lo, hi,
                           reinterpret_cast<unsigned long long *>(sums), n0, H, W, by_wc);
    });
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_apply_lut_u8(uint8_t *images, const uint8_t *lut, const int32_t *cam_of_image, int Nl, int64_t n_images,
                                  int64_t HW, void *stream) {
    FPCDR_REQUIRE(n_images >= 0 && HW > 0 && Nl > 0, "n_images must not be negative, HW and Nl must be positive");
    if (n_images == 0) return FPCDR_OK;
    FPCDR_REQUIRE(images != nullptr && lut != nullptr && cam_of_image != nullptr, "null pointer");
    FPCDR_REQUIRE(((uintptr_t)cam_of_image & 3) == 0, "cam_of_image must be 4-byte aligned");
    FPCDR_REQUIRE(HW <= (1LL << 35), "image too large");
    const size_t bytes = (size_t)n_images * (size_t)HW;
    FPCDR_REQUIRE(!overlap(images, bytes, lut, (size_t)Nl * 256) && !overlap(images, bytes, cam_of_image, (size_t)n_images * 4),
                  "images overlaps lut or cam_of_image");
    // the cameras are read back once, so that an index outside [0, Nl) is an error code, not a silent gap (this waits for the stream:
    // the entry is meant for one or two calls per fit, outside any capture)
    std::vector<int32_t> cams((size_t)n_images);
    if (hipMemcpyAsync(cams.data(), cam_of_image, (size_t)n_images * 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        fpcdr_set_error("%s: cannot read cam_of_image back (a device pointer on a stream that is not capturing is required)", __func__);
        return FPCDR_EINVAL;
    }
    long long bad = -1;
    for (int64_t b = 0; b < n_images; ++b)
        if ((cams[(size_t)b] < 0 || cams[(size_t)b] >= Nl) && bad < 0) bad = (long long)b;
    const unsigned bx = (unsigned)fpcdr_cdiv(fpcdr_cdiv(HW, 16), 256);
    for_image_batches(n_images, [&](long long n0, unsigned ny) {
        hipLaunchKernelGGL(k_apply_lut_u8, dim3(bx, ny), dim3(256), 0, (hipStream_t)stream, images, lut, cam_of_image, Nl, n0, (long long)HW);
    });
    FPCDR_CHECK_LAUNCH();
    if (bad >= 0) {
        fpcdr_set_error("%s: cam_of_image[%lld] = %d is outside [0, %d): that image is left as it is, the others are mapped", __func__, bad,
                        (int)cams[(size_t)bad], Nl);
        return FPCDR_EINVAL;
    }
    return FPCDR_OK;
}

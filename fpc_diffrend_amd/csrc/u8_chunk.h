// What the image-pair kernels share (compare.hip: k_compare_u8, overlay.hip: k_overlay_u8; the launch loop also undistort.hip).  Not part
// of the C ABI.  One thread owns 16 consecutive pixels of one row, starting at column j0: uint8 pixels travel as four 32-bit words, pixel
// k in byte k & 3 of word k >> 2, and the 16 RGB pixels of an output as twelve.  Every access has two forms, chosen per chunk: ONE
// 16-byte instruction (three for the 48 output bytes) where the chunk is whole (j0 + 16 <= W) and its address 16-byte aligned
// (16-byte stores reach 5-6 TB/s, 4- and 8-byte ones 1-1.7), and element by element in a row tail (W not a multiple of
// 16) or at an unaligned base, where the pixels past W are not touched.  The loaders take their four words ZEROED BY THE CALLER
// (`uint32_t w[4] = {0u, 0u, 0u, 0u}`): the element-wise form ORs its bytes in, so a pixel past W stays 0, and with the zeros in the kernel,
// ahead of the branch, the compiler keeps the 16-byte forms where they sat when all this was written in place (zeroed inside the helpers,
// ahead of their branch, it moved the render's 16-byte load out of line: uint8 comparison 4-18 % slower, profiles/compare_u8.txt 3).  Constant indices only: registers.
#pragma once
#include "common.h"

namespace {

// float -> 8 bit by the Comparison rule, the one float rule every output of these kernels rests on: x = v * scale in
// float32 (the library is built with -ffp-contract=off, and there is nothing to fuse with); NaN -> 0; rintf is round-half-to-even
// (v_rndne_f32); +-inf clip like any other value
__device__ __forceinline__ uint32_t quantise(float v, float scale) {
    const float x = v * scale;
    float y = rintf(x);
    y = y < 0.0f ? 0.0f : y;
    y = y > 255.0f ? 255.0f : y;
    y = x != x ? 0.0f : y;
    return (uint32_t)y;
}
__device__ __forceinline__ uint32_t quantise4(float4 v, float scale) {
    return quantise(v.x, scale) | quantise(v.y, scale) << 8 | quantise(v.z, scale) << 16 | quantise(v.w, scale) << 24;
}

// 16 uint8 pixels at p -> w[0..3] (zeroed by the caller)
__device__ __forceinline__ void load_chunk_u8(const uint8_t *p, bool whole, int j0, int W, uint32_t (&w)[4]) {
    if (whole && ((size_t)p & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (j0 + k < W) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    }
}

// 16 pixels of the rendered image, `off` elements into img -> their 8-bit values in w[0..3] (zeroed by the caller): float32 quantised, or
// uint8 as it is
template <bool IS_FLOAT>
__device__ __forceinline__ void load_chunk_render(const void *img, long long off, float scale, bool whole, int j0, int W, uint32_t (&w)[4]) {
    if (!IS_FLOAT) {
        load_chunk_u8(static_cast<const uint8_t *>(img) + off, whole, j0, W, w);
        return;
    }
    const float *p = static_cast<const float *>(img) + off;
    if (whole && ((size_t)p & 15) == 0) {
        const float4 *p4 = reinterpret_cast<const float4 *>(p);
        const float4 a = p4[0], b = p4[1], c = p4[2], d = p4[3];
        w[0] = quantise4(a, scale); w[1] = quantise4(b, scale); w[2] = quantise4(c, scale); w[3] = quantise4(d, scale);
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (j0 + k < W) w[k >> 2] |= quantise(p[k], scale) << (8 * (k & 3));
    }
}

// w[0..11], the 48 bytes of 16 RGB pixels in memory order -> p
__device__ __forceinline__ void store_chunk_rgb(uint8_t *p, bool whole, int j0, int W, const uint32_t (&w)[12]) {
    if (whole && ((size_t)p & 15) == 0) {
        uint4 *p4 = reinterpret_cast<uint4 *>(p);
        p4[0] = make_uint4(w[0], w[1], w[2], w[3]);
        p4[1] = make_uint4(w[4], w[5], w[6], w[7]);
        p4[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 48; ++k)
            if (j0 + k / 3 < W) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a != nullptr && b != nullptr && x < y + nb && y < x + na;
}

// launch(first image, images) for n_images in turns of at most 65535: the image is gridDim.y, and the kernel adds its first_image
template <typename Launch>
inline void for_image_batches(int64_t n_images, Launch &&launch) {
    for (int64_t n0 = 0; n0 < n_images; n0 += 65535) launch((long long)n0, (unsigned)(n_images - n0 < 65535 ? n_images - n0 : 65535));
}

}  // namespace

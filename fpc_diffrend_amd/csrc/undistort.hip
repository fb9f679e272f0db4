// Lens undistortion of 8-bit images at ingest (include/fpcdr.h, fpcdr_undistort_u8; reference src/undistort.py: cv2.undistort over every
// image of a take, new camera matrix = old one).  The rule is DESIGN.md 3, "Undistortion rule": OpenCV's five-coefficient model evaluated
// in unfused IEEE double (the library is built with -ffp-contract=off), bilinear taps with a zero border, round half up, clip, optional
// row flip -- bit for bit the float64 statement of tests/undistort_ref.py.
//
// One thread produces 16 consecutive output bytes of one row and writes them with ONE 16-byte store where the address allows (DESIGN.md
// 4.2: 16-byte stores reach 5-6 TB/s, 4- and 8-byte ones 1-1.7); a row tail (W not a multiple of 16) or an unaligned row goes out byte
// by byte.  No private segment, no LDS.
#include "u8_chunk.h"

namespace {

// one output pixel: (column j, y of its row and y*y) -> value before the row flip
__device__ __forceinline__ uint32_t undistort_one(const uint8_t *__restrict__ img, int H, int W, int j, double y, double yy,
                                                 double fx, double fy, double cx, double cy, double k1, double k2, double p1x2, double p2x2,
                                                 double p1, double p2, double k3, double clip_max) {
    const double x = ((double)j - cx) / fx;
    const double xx = x * x;
    const double r2 = xx + yy;
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double xy = x * y;
    const double xd = x * rad + (p1x2 * xy + p2 * (r2 + 2.0 * xx));
    const double yd = y * rad + (p1 * (r2 + 2.0 * yy) + p2x2 * xy);
    const double u = fx * xd + cx;
    const double v = fy * yd + cy;
    const double u0 = floor(u), v0 = floor(v);
    // at least one tap inside (false when u, v are not numbers); otherwise the zero border, whatever the weights: taps and weights 0
    const bool near = u0 >= -1.0 && u0 < (double)W && v0 >= -1.0 && v0 < (double)H;
    const double a = near ? u - u0 : 0.0, b = near ? v - v0 : 0.0;
    const int iu = near ? (int)u0 : -1, iv = near ? (int)v0 : -1;      // in [-1, W - 1], [-1, H - 1]
    // the four loads are unconditional, from addresses clamped into the image, and a tap outside is then replaced by 0: no branch, so
    // that the loads of a thread's pixels go out together instead of one pixel's after the other's have come back
    const bool c0 = iu >= 0, c1 = near && iu + 1 < W, r0 = iv >= 0, r1 = near && iv + 1 < H;
    const uint8_t *row0 = img + (long long)(r0 ? iv : 0) * W;
    const uint8_t *row1 = img + (long long)(r1 ? iv + 1 : H - 1) * W;
    const int col0 = c0 ? iu : 0, col1 = c1 ? iu + 1 : W - 1;
    const uint32_t b00 = row0[col0], b01 = row0[col1], b10 = row1[col0], b11 = row1[col1];
    const double t00 = (r0 && c0) ? (double)b00 : 0.0;
    const double t01 = (r0 && c1) ? (double)b01 : 0.0;
    const double t10 = (r1 && c0) ? (double)b10 : 0.0;
    const double t11 = (r1 && c1) ? (double)b11 : 0.0;
    const double top = t00 + a * (t01 - t00);
    const double bot = t10 + a * (t11 - t10);
    const double val = top + b * (bot - top);
    return (uint32_t)fmin(floor(val + 0.5), clip_max);
}

// grid: x over the H * ceil(W / 16) threads of one image, y over the images of this launch (image number first_image + blockIdx.y:
// nothing 64-bit is divided per thread)
__global__ void __launch_bounds__(256) k_undistort_u8(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                      const double *__restrict__ cam_table, long long first_image, int H, int W, int Wc,
                                                      int n_cam, int clip_max, int flip_rows) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (unsigned)H * (unsigned)Wc) return;
    const int i = (int)(t / (unsigned)Wc);
    const int j0 = (int)(t - (unsigned)i * (unsigned)Wc) * 16;
    const long long n = first_image + blockIdx.y;
    const double *c = cam_table + (n % n_cam) * 9;
    const double fx = c[0], fy = c[1], cx = c[2], cy = c[3], k1 = c[4], k2 = c[5], p1 = c[6], p2 = c[7], k3 = c[8];
    const double p1x2 = 2.0 * p1, p2x2 = 2.0 * p2;
    const double y = ((double)i - cy) / fy;
    const double yy = y * y;
    const uint8_t *img = src + n * H * W;
    // four pixels per trip of a loop that is NOT unrolled: their sixteen loads are in flight together.  (Unrolled, the compiler hoists all
    // 64 loads and holds every pixel's weights and addresses at once: 276 registers, one wave per SIMD.)  The sixteen results are
    // shifted into two 64-bit registers -- no array, so no private segment.
    uint64_t lo = 0, hi = 0;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        uint32_t word = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
            // (a column past the row's end is computed like any other -- its taps are clamped into the image -- and never stored)
            word |= undistort_one(img, H, W, j0 + 4 * q + p, y, yy, fx, fy, cx, cy, k1, k2, p1x2, p2x2, p1, p2, k3, (double)clip_max) << (8 * p);
        const uint64_t sh = (uint64_t)word << (32 * (q & 1));
        lo |= q < 2 ? sh : 0;
        hi |= q < 2 ? 0 : sh;
    }
    uint8_t *out = dst + (n * H + (flip_rows ? H - 1 - i : i)) * W + j0;
    if (j0 + 16 <= W && ((size_t)out & 15) == 0) {
        *reinterpret_cast<uint4 *>(out) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        return;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (j0 + k < W) out[k] = (uint8_t)((k < 8 ? lo : hi) >> (8 * (k & 7)));
}

}  // namespace

extern "C" int fpcdr_undistort_u8(const uint8_t *src, uint8_t *dst, const double *cam_table, int64_t n_images, int H, int W, int n_cam,
                                  int clip_max, int flip_rows, void *stream) {
    FPCDR_REQUIRE(src != nullptr && dst != nullptr && cam_table != nullptr, "null pointer");
    FPCDR_REQUIRE(src != dst, "src and dst must be different buffers (every output pixel reads four input pixels elsewhere)");
    FPCDR_REQUIRE(n_images > 0 && H > 0 && W > 0 && n_cam > 0, "sizes must be positive");
    FPCDR_REQUIRE(clip_max >= 0 && clip_max <= 255, "clip_max outside [0, 255]");
    const int Wc = fpcdr_cdiv(W, 16);
    FPCDR_REQUIRE((long long)H * Wc <= (1LL << 31) - 256, "image too large");
    const unsigned bx = (unsigned)fpcdr_cdiv((long long)H * Wc, 256);
    for_image_batches(n_images, [&](long long n0, unsigned ny) {
        hipLaunchKernelGGL(k_undistort_u8, dim3(bx, ny), dim3(256), 0, (hipStream_t)stream, src, dst, cam_table, n0, H, W, Wc, n_cam, clip_max,
                           flip_rows);
    });
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

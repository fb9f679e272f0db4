// Weighted robust pixel loss, value and closed-form gradient in ONE streaming pass, for gfx950 (MI355X).  DESIGN.md 3, "Robust loss rule".
//
// The reference's only defence against pixels its model cannot explain is np.clip(img, 0, 140) at fit.py:531; utils.py:12-35 carries
// reduceHighlights / normalize_highlights and wires neither.  Here the operand of k_pixel_loss, d = ref - color_scale * (covered ? colour :
// bg), goes through one of three kinds -- L2 rho = d^2, Charbonnier rho = 2 c^2 (sqrt(1 + d^2 / c^2) - 1) in its form without the
// cancellation, Geman-McClure rho = d^2 / (1 + d^2 / c^2) -- and is weighted by constants of the step: a per-pixel byte mask, a per-face
// weight looked up through the triangle id of rast, a weight for everything outside the mesh, and a saturation level of the capture from
// which on a pixel counts nothing.  sums[0] += w rho, sums[1] += w, grad_colour = covered ? (-2 color_scale grad_scale) (w psi) : 0 with
// psi = rho'(d) / 2.  No transcendental: one IEEE square root and IEEE divisions (the library is built without fast-math; hipcc's
// correctly rounded float32 divide and square root are its default and are not switched off).
//
// Two decompositions of the same pixels meet, as in overlay.hip, because the inputs come in two widths:
//   * colour, rast and the gradient are 4 .. 16 bytes a pixel: lane = pixel, so the 64 lanes of a load or store touch consecutive entries,
//     as in k_pixel_loss.
//   * ref and mask are ONE byte a pixel.  A wave takes WAVE_PX = 256 consecutive pixels a trip; lanes 0 .. 15 each OWN one of their 16
//     chunks of 16 pixels and read it in the two forms of u8_chunk.h (one 16-byte load where the chunk is whole and its address aligned,
//     byte by byte in the tail of the buffer or at an unaligned base).  In sub-trip k lane l works on pixel 64 k + l, whose byte is byte
//     l & 3 of word (l >> 2) & 3 of the owner 4 k + (l >> 4): four lane reads (ds_bpermute, no LDS memory) and three selects a buffer.
// The loads of a trip are issued in two stages ahead of the arithmetic -- rast.w of the four sub-trips and the byte chunks, then the
// first channel's colour and the face weights of the covered pixels -- so that a wave has eight loads in flight, not one (loaded inside
// each sub-trip's own branch the call took 1.44 x the time of k_pixel_loss at the same bytes; staged, 0.96: profiles/robust_time.txt).
// A grid-stride loop over at most BLOCKS_PER_CU workgroups a CU (72 registers a lane: seven waves a SIMD): two float64 atomics a workgroup, whatever the size.  Lane sums in float32
// -> wave (shuffles) -> block (LDS, 32 bytes: the only LDS) -> one float64 atomic each.  The gradient is written by plain stores, every
// entry once: bit-identical from run to run.  The kind is a template argument: the L2 instantiation carries no square root and no division.
// Constant indices only: no private segment.
#include "u8_chunk.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int WAVE_PX = 256;               // pixels of a wave's trip: 16 chunks of 16
constexpr int BLOCK_PX = 4 * WAVE_PX;      // pixels of a workgroup's trip (256 threads)
constexpr int BLOCKS_PER_CU = 6;           // the grid is min(ceil(pixels / BLOCK_PX), BLOCKS_PER_CU * compute units)

// byte (l & 3) of word (l >> 2) & 3 of lane `src`: the byte of this lane's pixel from the chunk's owner.  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t owner_byte(const uint32_t (&w)[4], int src, int lane) {
    const uint32_t a = (uint32_t)__shfl((int)w[0], src, 64), b = (uint32_t)__shfl((int)w[1], src, 64);
    const uint32_t c = (uint32_t)__shfl((int)w[2], src, 64), d = (uint32_t)__shfl((int)w[3], src, 64);
    const int j = (lane >> 2) & 3;
    const uint32_t word = j == 0 ? a : j == 1 ? b : j == 2 ? c : d;
    return (word >> (8 * (lane & 3))) & 255u;
}

template <int KIND>
__global__ void __launch_bounds__(256) k_robust_loss(const float *__restrict__ color, const float *__restrict__ rast,
                                                     const uint8_t *__restrict__ ref, const uint8_t *__restrict__ mask,
                                                     const float *__restrict__ face_w, int T, long long npix, int C, float bg,
                                                     float color_scale, float grad_scale, float inv_c, float w_outside, int sat,
                                                     double *__restrict__ sums, float *__restrict__ grad_color) {
    __shared__ float s_part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n_tiles = (npix + WAVE_PX - 1) / WAVE_PX;
    const float coef = -2.0f * color_scale * grad_scale;      // (k_pixel_loss's expression: kind L2 without weights gives its bits)
    float acc_rho = 0.0f, acc_w = 0.0f;
    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < n_tiles; tile += (long long)gridDim.x * 4) {      // (uniform over the wave)
        const long long p0 = tile * WAVE_PX;
        // ---- stage 1: every load that depends on nothing, in flight together: rast.w of the four sub-trips, the byte chunks ----
        long long at[4];
        bool live[4];
        float rw3[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = p0 + 64 * k + lane;
            live[k] = i < npix;
            at[k] = live[k] ? i : npix - 1;      // (a lane past the buffer reads its last pixel and decides nothing)
            rw3[k] = rast[4 * at[k] + 3];
        }
        uint32_t rw[4] = {0u, 0u, 0u, 0u}, mw[4] = {0u, 0u, 0u, 0u};
        const long long j0 = p0 + 16 * lane;
        if (lane < 16 && j0 < npix) {
            const int rem = npix - j0 < 16 ? (int)(npix - j0) : 16;      // pixels of this chunk inside the buffer
            load_chunk_u8(ref + j0, rem == 16, 0, rem, rw);
            if (mask) load_chunk_u8(mask + j0, rem == 16, 0, rem, mw);
        }
        // ---- stage 2: what depends on rast.w -- the first channel's colour and the face weight of covered pixels -- in flight together ----
        bool covered[4];
        float col0[4], fw[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            covered[k] = live[k] && rw3[k] > 0.0f;
            col0[k] = bg;
            fw[k] = 1.0f;
            if (covered[k]) {
                col0[k] = color[at[k] * C];
                if (face_w) {
                    const int id = (int)rw3[k];
                    fw[k] = (unsigned)(id - 1) < (unsigned)T ? face_w[id - 1] : 0.0f;      // (a wrong table length reads nothing out of bounds)
                }
            }
        }
        // (the lane reads stand outside anything a lane may skip: every lane of the wave takes part in each)
        uint32_t rbyte[4], mbyte[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int src = 4 * k + (lane >> 4);
            rbyte[k] = owner_byte(rw, src, lane);
            mbyte[k] = mask ? owner_byte(mw, src, lane) : 255u;      // (uniform branch)
        }
        // ---- stage 3: the rule ----
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!live[k]) continue;
            const long long i = at[k];
            const uint32_t rb = rbyte[k], mb = mbyte[k];
            const float r = (float)rb;
            float wm = mask ? (float)mb * (1.0f / 255.0f) : 1.0f;
            if (sat > 0 && (int)rb >= sat) wm = 0.0f;
            const float w = covered[k] ? wm * fw[k] : wm * w_outside;
            for (int c = 0; c < C; ++c) {
                const float col = c == 0 ? col0[k] : (covered[k] ? color[i * C + c] : bg);
                const float a = color_scale * col;
                const float d = r - a;
                const float dd = d * d;
                float rho = dd, s = 1.0f;
                if (KIND != FPCDR_ROBUST_L2) {
                    const float z = d * inv_c;
                    const float t = z * z;
                    if (KIND == FPCDR_ROBUST_CHARBONNIER) {
                        const float h = sqrtf(1.0f + t);
                        rho = (2.0f * dd) / (1.0f + h);
                        s = 1.0f / h;
                    } else {
                        const float q = 1.0f + t;
                        rho = dd / q;
                        s = 1.0f / (q * q);
                    }
                }
                const float psi = d * s;
                acc_rho += w * rho;
                acc_w += w;
                if (grad_color) grad_color[i * C + c] = covered[k] ? coef * (w * psi) : 0.0f;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        acc_rho += __shfl_xor(acc_rho, o, 64);
        acc_w += __shfl_xor(acc_w, o, 64);
    }
    if (lane == 0) {
        s_part[0][wave] = acc_rho;
        s_part[1][wave] = acc_w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(sums, (double)s_part[0][0] + (double)s_part[0][1] + (double)s_part[0][2] + (double)s_part[0][3]);
        atomicAdd(sums + 1, (double)s_part[1][0] + (double)s_part[1][1] + (double)s_part[1][2] + (double)s_part[1][3]);
    }
}

// The all-background share of the WEIGHTED one-pass objective (objective.hip; DESIGN.md 3, "Weighted objective rule"): an empty pixel
// always shows the background, so its term w0 * rho(ref - bg_scaled), w0 = wm * w_outside, depends on the capture and the mask alone.  Per
// image (gridDim.y) the sums of w0 * rho and of w0.  A thread owns chunks of 16 consecutive pixels, read in the two forms of u8_chunk.h;
// lane sums in float32 -> wave -> block -> one float64 atomic per sum and workgroup, as above.  Constant indices only: no private segment.
template <int KIND>
__global__ void __launch_bounds__(256) k_robust_bg(const uint8_t *__restrict__ ref, const uint8_t *__restrict__ mask, long long px, float bgs,
                                                   float inv_c, float w_outside, int sat, double *__restrict__ out) {
    __shared__ float s_part[2][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *r = ref + (size_t)blockIdx.y * px;
    const uint8_t *m = mask ? mask + (size_t)blockIdx.y * px : nullptr;
    const long long n_chunks = (px + 15) / 16;
    float acc_rho = 0.0f, acc_w = 0.0f;
    for (long long ch = (long long)blockIdx.x * 256 + threadIdx.x; ch < n_chunks; ch += (long long)gridDim.x * 256) {
        const long long j0 = ch * 16;
        const int rem = px - j0 < 16 ? (int)(px - j0) : 16;      // pixels of this chunk inside the image
        uint32_t rw[4] = {0u, 0u, 0u, 0u}, mw[4] = {0u, 0u, 0u, 0u};
        load_chunk_u8(r + j0, rem == 16, 0, rem, rw);
        if (m) load_chunk_u8(m + j0, rem == 16, 0, rem, mw);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k >= rem) continue;
            const uint32_t rb = (rw[k >> 2] >> (8 * (k & 3))) & 255u, mb = (mw[k >> 2] >> (8 * (k & 3))) & 255u;
            float wm = m ? (float)mb * (1.0f / 255.0f) : 1.0f;
            if (sat > 0 && (int)rb >= sat) wm = 0.0f;
            const float w0 = wm * w_outside;
            const float d = (float)rb - bgs;
            const float dd = d * d;
            float rho = dd;
            if (KIND != FPCDR_ROBUST_L2) {
                const float z = d * inv_c;
                const float t = z * z;
                if (KIND == FPCDR_ROBUST_CHARBONNIER) rho = (2.0f * dd) / (1.0f + sqrtf(1.0f + t));
                else rho = dd / (1.0f + t);
            }
            acc_rho += w0 * rho;
            acc_w += w0;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        acc_rho += __shfl_xor(acc_rho, o, 64);
        acc_w += __shfl_xor(acc_w, o, 64);
    }
    if (lane == 0) {
        s_part[0][wave] = acc_rho;
        s_part[1][wave] = acc_w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(out + 2 * (size_t)blockIdx.y, (double)s_part[0][0] + (double)s_part[0][1] + (double)s_part[0][2] + (double)s_part[0][3]);
        atomicAdd(out + 2 * (size_t)blockIdx.y + 1, (double)s_part[1][0] + (double)s_part[1][1] + (double)s_part[1][2] + (double)s_part[1][3]);
    }
}

}  // namespace

extern "C" int fpcdr_ref_bg_wsum(const uint8_t *ref, const uint8_t *mask, int64_t n_images, int64_t px_per_image, float bg_scaled, int32_t kind,
                                 float inv_c, float w_outside, int32_t sat, double *out, void *stream) {
    FPCDR_REQUIRE(ref && out, "null pointer");
    FPCDR_REQUIRE(n_images > 0 && n_images <= 65535 && px_per_image > 0, "bad sizes");
    FPCDR_REQUIRE(kind == FPCDR_ROBUST_L2 || kind == FPCDR_ROBUST_CHARBONNIER || kind == FPCDR_ROBUST_GEMAN_MCCLURE,
                  "kind must be FPCDR_ROBUST_L2, _CHARBONNIER or _GEMAN_MCCLURE");
    FPCDR_REQUIRE(kind == FPCDR_ROBUST_L2 || (std::isfinite(inv_c) && inv_c > 0.0f),
                  "inv_c = 1 / scale must be finite and positive for a kind other than L2");
    FPCDR_REQUIRE(std::isfinite(w_outside) && w_outside >= 0.0f, "w_outside must be finite and not negative");
    FPCDR_REQUIRE(sat >= 0 && sat <= 255, "sat must lie in 0 .. 255 (0: off)");
    FPCDR_REQUIRE(((uintptr_t)out & 7) == 0, "a misaligned buffer");
    const long long n_chunks = ((long long)px_per_image + 15) / 16;
    const unsigned blocks = (unsigned)std::min<long long>(64, (n_chunks + 255) / 256);      // (a thread: at least one chunk, up to 64 workgroups an image)
    auto kern = kind == FPCDR_ROBUST_L2 ? k_robust_bg<FPCDR_ROBUST_L2>
              : kind == FPCDR_ROBUST_CHARBONNIER ? k_robust_bg<FPCDR_ROBUST_CHARBONNIER> : k_robust_bg<FPCDR_ROBUST_GEMAN_MCCLURE>;
    hipLaunchKernelGGL(kern, dim3(blocks, (unsigned)n_images), dim3(256), 0, (hipStream_t)stream, ref, mask, (long long)px_per_image, bg_scaled,
                       inv_c, w_outside, sat, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_robust_loss(const fpcdr_robust_loss_params *p, void *stream) {
    FPCDR_REQUIRE(p != nullptr, "null params");
    FPCDR_REQUIRE(p->color && p->rast && p->ref && p->sums, "null pointer");
    FPCDR_REQUIRE(p->B > 0 && p->H > 0 && p->W > 0 && p->C > 0, "sizes must be positive");
    FPCDR_REQUIRE(p->kind == FPCDR_ROBUST_L2 || p->kind == FPCDR_ROBUST_CHARBONNIER || p->kind == FPCDR_ROBUST_GEMAN_MCCLURE,
                  "kind must be FPCDR_ROBUST_L2, _CHARBONNIER or _GEMAN_MCCLURE");
    FPCDR_REQUIRE(p->kind == FPCDR_ROBUST_L2 || (std::isfinite(p->inv_c) && p->inv_c > 0.0f),
                  "inv_c = 1 / scale must be finite and positive for a kind other than L2");
    FPCDR_REQUIRE(std::isfinite(p->w_outside) && p->w_outside >= 0.0f, "w_outside must be finite and not negative");
    FPCDR_REQUIRE(p->sat >= 0 && p->sat <= 255, "sat must lie in 0 .. 255 (0: off)");
    FPCDR_REQUIRE(!p->face_w || p->T > 0, "face_w needs T > 0");
    FPCDR_REQUIRE(((uintptr_t)p->sums & 7) == 0 && ((uintptr_t)p->color & 3) == 0 && ((uintptr_t)p->rast & 3) == 0 &&
                  ((uintptr_t)p->face_w & 3) == 0 && ((uintptr_t)p->grad_color & 3) == 0, "a misaligned buffer");
    const long long npix = (long long)p->B * p->H * p->W;
    const long long want = (npix + BLOCK_PX - 1) / BLOCK_PX, cap = (long long)BLOCKS_PER_CU * fpcdr_cu_count();
    const dim3 grid((unsigned)(want < cap ? want : cap));
    auto kern = p->kind == FPCDR_ROBUST_L2 ? k_robust_loss<FPCDR_ROBUST_L2>
              : p->kind == FPCDR_ROBUST_CHARBONNIER ? k_robust_loss<FPCDR_ROBUST_CHARBONNIER> : k_robust_loss<FPCDR_ROBUST_GEMAN_MCCLURE>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, p->color, p->rast, p->ref, p->mask, p->face_w, p->face_w ? p->T : 0, npix,
                       p->C, p->bg, p->color_scale, p->grad_scale, p->inv_c, p->w_outside, p->sat, p->sums, p->grad_color);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

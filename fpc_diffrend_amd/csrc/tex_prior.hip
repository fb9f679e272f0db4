// The texture prior of the fit step for gfx950 (MI355X; DESIGN.md 3, "Texture prior rule"): a smoothness term over the pairs of
// neighbouring texels and a hold to an anchor texture, value and gradient from ONE launch, and a finish kernel behind the kernel boundary
// that forms the parts and the value and leaves the two double accumulators zero for the next call (the contract of csrc/mesh_reg.hip;
// its finish divides F accumulators by one divisor and weights their sum once, this one weights two parts separately: a finish of its own).
#include "common.h"

#include <cmath>

namespace {

// The tile of a workgroup: TY rows of TX texels, a thread holds RUN consecutive texels of one row (16 x 16 threads).  A wave is four rows
// of 64 texels: with C = 1 every load instruction of the wave's own texels is four 256-byte row segments of 16 bytes a lane.  The rows
// above and below a thread's run are the runs of the threads above and below it in the same workgroup (the same lines, through the
// vector L1), the texels left and right of it are in the neighbouring lanes' registers (DPP); only the tile's halo -- one row above, one
// below, one texel left and right -- is read a second time, by the neighbouring workgroup: (TY + 2) / TY = 1.125 of the bytes in the
// worst case, from L2 when the neighbour is on the same XCD.
constexpr int TEX_RUN = 4, TEX_TX = 64, TEX_TY = 16;
// The workgroups of a launch.  Every workgroup ends in two double adds to the SAME two addresses, which the memory side takes one after
// the other, ~6 ns each: at one tile a workgroup the 4096 x 4096 texture's 16384 workgroups spent 200 us of a 212 us call queueing there,
// whatever the tile's shape, and the call's time did not depend on its bytes (profiles/tex_prior_time.txt).  So a workgroup walks several
// tiles in strides of the grid and adds once: at most TEX_MAX_WGS workgroups (four a CU: 76 us at 4096 x 4096 x 1, against 98 us with 512
// and 81 us with 2048), two tiles a workgroup from 512 tiles on (1024 x 1024 x 1: 15.4 us with 512 workgroups, 19.4 us with 1024), one
// tile a workgroup for the small textures whose tiles do not fill the chip anyway.
constexpr int TEX_MAX_WGS = 1024;
static inline int tex_prior_workgroups(int n_tiles) {
    if (n_tiles <= 256) return n_tiles;
    const int half = (n_tiles + 1) / 2;
    return half < 256 ? 256 : (half > TEX_MAX_WGS ? TEX_MAX_WGS : half);
}

// RUN texels of C channels from row `row` (a texel offset) starting at column x0, columns clamped to Wt - 1 (in bounds, whatever the
// flags; a clamped copy is switched off by its pair's select).  vec: the run is whole and its first float 16-byte aligned.
template <int C>
__device__ __forceinline__ void load_run(const float *__restrict__ p, size_t row, int x0, int Wt, bool vec, float (&o)[TEX_RUN][C]) {
    if (vec) {
        const float4 *q = reinterpret_cast<const float4 *>(p + (row + (size_t)x0) * C);
        float f[TEX_RUN * C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const float4 v = q[i];
            f[4 * i] = v.x; f[4 * i + 1] = v.y; f[4 * i + 2] = v.z; f[4 * i + 3] = v.w;
        }
#pragma unroll
        for (int k = 0; k < TEX_RUN; ++k)
#pragma unroll
            for (int c = 0; c < C; ++c) o[k][c] = f[k * C + c];
    } else {
#pragma unroll
        for (int k = 0; k < TEX_RUN; ++k) {
            const float *q = p + (row + (size_t)min(x0 + k, Wt - 1)) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[k][c] = q[c];
        }
    }
}

template <int C>
__device__ __forceinline__ void load_texel(const float *__restrict__ p, size_t texel, float (&o)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = p[texel * C + c];
}

// One pair seen from its end p: g += m rho'(s) (p - q), and the pair's value m rho(s); s = |p - q|^2 over the channels,
// rho(s) = s (ic = 0) or 2 s / (1 + sqrt(1 + s / c^2)), rho' = 1 or 1 / sqrt(1 + s / c^2) (the motion term's form: no cancellation).
// on = the pair exists; a pair that does not, or whose weight m is 0, adds exactly 0 by a SELECT: a NaN in a texel whose pairs all weigh
// nothing stays where it is.  Seen from q the differences are the exact negatives, s and m the same numbers.
template <int C>
__device__ __forceinline__ float pair_term(const float (&p)[C], const float (&q)[C], float m, bool on, float ic, float (&g)[C]) {
    float d[C], s = 0.0f, zz = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        d[c] = p[c] - q[c];
        s += d[c] * d[c];
        const float z = d[c] * ic;
        zz += z * z;
    }
    float rho = s, dr = 1.0f;
    if (ic > 0.0f) {
        const float h = sqrtf(1.0f + zz);
        rho = (2.0f * s) / (1.0f + h);
        dr = 1.0f / h;
    }
    const bool live = on && m > 0.0f;
    const float k = m * dr;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] += live ? k * d[c] : 0.0f;
    return live ? m * rho : 0.0f;
}

// A float of the lane to the left (FROM_LEFT) or right within the DPP row of 16 lanes; a lane without one keeps `edge`.
template <bool FROM_LEFT>
__device__ __forceinline__ float row_neighbour(float v, float edge) {
    return __int_as_float(FROM_LEFT ? __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x111, 0xF, 0xF, false)     // row_shr:1
                                    : __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x101, 0xF, 0xF, false));   // row_shl:1
}

// One thread per run of four texels.  It forms the gradient of its own texels from their four neighbours (left, right, up, down, in
// that order: a gather, every entry stored once, no float atomics) and adds only their RIGHT and DOWN pairs to the value, so every
// pair is counted once.  The texel left of a run is the last texel of the lane to the left, the texel right of it the first of the
// lane to the right: they come through DPP from that lane's registers (TXT, the threads of a tile's row, is a multiple of the DPP
// row's 16 lanes, so the lanes of a DPP row sit side by side in one texture row); only the first and last lane of a DPP row load
// theirs.  EVERY lane therefore loads, a lane without a texel at clamped -- in bounds -- coordinates, and is switched off by selects.
// A workgroup walks its tiles in strides of the grid (tex_prior_workgroups) and keeps its waves' sums as doubles; its two partial sums
// go to acc[0] (smoothness) and acc[1] (anchor), one relaxed agent-scope add each, once.
// coef_s = 2 w_s / (Ht Wt), coef_a = 2 w_a / (Ht Wt).  VEC: Wt is a multiple of four and every pointer is 16-byte aligned (the host
// decides); a run that is not whole cannot occur then.  Constant indices only: no private segment.
template <int C, bool VEC>
__global__ void __launch_bounds__(256) k_tex_prior(const float *__restrict__ tex, const float *__restrict__ anchor,
                                                   const float *__restrict__ smooth_w, const float *__restrict__ anchor_w, float ic,
                                                   float coef_s, float coef_a, int Ht, int Wt, int tiles_x, int n_tiles,
                                                   float *__restrict__ grad, double *__restrict__ acc) {
    constexpr int TXT = TEX_TX / TEX_RUN;      // the threads of a tile's row
    static_assert(TXT % 16 == 0 && TXT * TEX_TY == 256, "a DPP row of 16 lanes lies within one row of the tile; 256 threads a tile");
    const int tx = threadIdx.x % TXT, ty = threadIdx.x / TXT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sum_smooth = 0.0, sum_anchor = 0.0;      // the wave's sums over the workgroup's tiles
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
        const int y = tile_y * TEX_TY + ty, x0 = (tile_x * TXT + tx) * TEX_RUN;
        const bool valid = y < Ht && x0 < Wt;
        const int yc = min(y, Ht - 1), xc = VEC ? min(x0, Wt - TEX_RUN) : min(x0, Wt - 1);
        const size_t row = (size_t)yc * Wt, row_u = (size_t)max(yc - 1, 0) * Wt, row_d = (size_t)min(yc + 1, Ht - 1) * Wt;
        const int xl = min(max(x0 - 1, 0), Wt - 1), xr = min(x0 + TEX_RUN, Wt - 1);
        const bool has_u = y > 0, has_d = y + 1 < Ht, has_l = x0 > 0;
        const bool edge_l = (threadIdx.x & 15) == 0, edge_r = (threadIdx.x & 15) == 15;
        float v_smooth = 0.0f, v_anchor = 0.0f;      // (a thread without a texel: 0)
        float t[TEX_RUN][C], tu[TEX_RUN][C], td[TEX_RUN][C], tl[C], tr[C];
        load_run<C>(tex, row, xc, Wt, VEC, t);
        load_run<C>(tex, row_u, xc, Wt, VEC, tu);
        load_run<C>(tex, row_d, xc, Wt, VEC, td);
#pragma unroll
        for (int c = 0; c < C; ++c) tl[c] = tr[c] = 0.0f;
        if (edge_l) load_texel<C>(tex, row + xl, tl);
        if (edge_r) load_texel<C>(tex, row + xr, tr);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            tl[c] = row_neighbour<true>(t[TEX_RUN - 1][c], tl[c]);
            tr[c] = row_neighbour<false>(t[0][c], tr[c]);
        }
        float w[TEX_RUN][1], wu[TEX_RUN][1], wd[TEX_RUN][1], wl[1], wr[1];
        if (smooth_w) {
            load_run<1>(smooth_w, row, xc, Wt, VEC, w);
            load_run<1>(smooth_w, row_u, xc, Wt, VEC, wu);
            load_run<1>(smooth_w, row_d, xc, Wt, VEC, wd);
            wl[0] = wr[0] = 0.0f;
            if (edge_l) load_texel<1>(smooth_w, row + xl, wl);
            if (edge_r) load_texel<1>(smooth_w, row + xr, wr);
            wl[0] = row_neighbour<true>(w[TEX_RUN - 1][0], wl[0]);
            wr[0] = row_neighbour<false>(w[0][0], wr[0]);
        } else {
#pragma unroll
            for (int k = 0; k < TEX_RUN; ++k) w[k][0] = wu[k][0] = wd[k][0] = 1.0f;
            wl[0] = wr[0] = 1.0f;
        }
        float g[TEX_RUN][C];
#pragma unroll
        for (int k = 0; k < TEX_RUN; ++k) {
            const bool in = valid && x0 + k < Wt, has_r = x0 + k + 1 < Wt;
#pragma unroll
            for (int c = 0; c < C; ++c) g[k][c] = 0.0f;
            if (k == 0) pair_term<C>(t[0], tl, fminf(w[0][0], wl[0]), in && has_l, ic, g[0]);
            else pair_term<C>(t[k], t[k - 1], fminf(w[k][0], w[k - 1][0]), in, ic, g[k]);
            float vr;
            if (k == TEX_RUN - 1) vr = pair_term<C>(t[k], tr, fminf(w[k][0], wr[0]), in && has_r, ic, g[k]);
            else vr = pair_term<C>(t[k], t[k + 1], fminf(w[k][0], w[k + 1][0]), in && has_r, ic, g[k]);
            pair_term<C>(t[k], tu[k], fminf(w[k][0], wu[k][0]), in && has_u, ic, g[k]);
            const float vd = pair_term<C>(t[k], td[k], fminf(w[k][0], wd[k][0]), in && has_d, ic, g[k]);
            v_smooth += vr + vd;
#pragma unroll
            for (int c = 0; c < C; ++c) g[k][c] = coef_s * g[k][c];
        }
        if (anchor) {
            float a[TEX_RUN][C], aw[TEX_RUN][1];
            load_run<C>(anchor, row, xc, Wt, VEC, a);
            if (anchor_w) load_run<1>(anchor_w, row, xc, Wt, VEC, aw);
#pragma unroll
            for (int k = 0; k < TEX_RUN; ++k) {
                const float wk = anchor_w ? aw[k][0] : 1.0f;
                const bool live = valid && x0 + k < Wt && wk > 0.0f;
                const float ca = coef_a * wk;
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float d = t[k][c] - a[k][c];
                    s += d * d;
                    g[k][c] += live ? ca * d : 0.0f;
                }
                v_anchor += live ? wk * s : 0.0f;
            }
        }
        if (grad && valid) {
            float *o = grad + (row + (size_t)x0) * C;
            if (VEC) {
                float f[TEX_RUN * C];
#pragma unroll
                for (int k = 0; k < TEX_RUN; ++k)
#pragma unroll
                    for (int c = 0; c < C; ++c) f[k * C + c] = g[k][c];
#pragma unroll
                for (int i = 0; i < C; ++i) reinterpret_cast<float4 *>(o)[i] = make_float4(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < TEX_RUN; ++k)
                    if (x0 + k < Wt) {
#pragma unroll
                        for (int c = 0; c < C; ++c) o[k * C + c] = g[k][c];
                    }
            }
        }
        // the tile's value: both lane values summed over the wave (DPP), kept as doubles across the tiles
        sum_smooth += (double)wave_sum_dpp(v_smooth);
        sum_anchor += (double)wave_sum_dpp(v_anchor);
    }
    // the value tail: the four waves' sums through LDS, one relaxed agent-scope add for each part
    __shared__ double s_part[2][4];
    if (lane == 0) { s_part[0][wave] = sum_smooth; s_part[1][wave] = sum_anchor; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *p = s_part[threadIdx.x];
        __hip_atomic_fetch_add(&acc[threadIdx.x], p[0] + p[1] + p[2] + p[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// part = acc / (Ht Wt), out = w_s part[0] + w_a part[1], and the accumulators zeroed for the next call.  The kernel boundary in front of
// it orders the adds before its loads.
__global__ void __launch_bounds__(64) k_tex_prior_finish(double *__restrict__ acc, double n_texels, float w_smooth, float w_anchor,
                                                         float *__restrict__ part, float *__restrict__ out) {
    if (threadIdx.x == 0) {
        const double p0 = acc[0] / n_texels, p1 = acc[1] / n_texels;
        part[0] = (float)p0;
        part[1] = (float)p1;
        out[0] = (float)((double)w_smooth * p0 + (double)w_anchor * p1);
        acc[0] = 0.0;
        acc[1] = 0.0;
    }
}

template <int C>
void launch_tex_prior(bool vec, hipStream_t st, const float *tex, const float *anchor, const float *smooth_w, const float *anchor_w,
                      float ic, float coef_s, float coef_a, int Ht, int Wt, float *grad, double *acc) {
    const int tiles_x = fpcdr_cdiv(Wt, TEX_TX), n_tiles = tiles_x * fpcdr_cdiv(Ht, TEX_TY);
    const dim3 grid(tex_prior_workgroups(n_tiles));
    if (vec)
        hipLaunchKernelGGL((k_tex_prior<C, true>), grid, dim3(256), 0, st, tex, anchor, smooth_w, anchor_w, ic, coef_s, coef_a, Ht, Wt,
                           tiles_x, n_tiles, grad, acc);
    else
        hipLaunchKernelGGL((k_tex_prior<C, false>), grid, dim3(256), 0, st, tex, anchor, smooth_w, anchor_w, ic, coef_s, coef_a, Ht, Wt,
                           tiles_x, n_tiles, grad, acc);
}

}  // namespace

extern "C" int fpcdr_tex_prior(const float *tex, const float *anchor, const float *smooth_w, const float *anchor_w, float inv_c,
                               float w_smooth, float w_anchor, float *grad_tex, void *acc, float *part, float *out, int32_t Ht,
                               int32_t Wt, int32_t C, void *stream) {
    FPCDR_REQUIRE(tex && acc && part && out, "null pointer");
    FPCDR_REQUIRE(Ht > 0 && Wt > 0 && C >= 1 && C <= 4, "bad sizes (C must be 1..4)");
    FPCDR_REQUIRE((long long)Ht * Wt * C <= 0x7fffffffLL , "texture too large");
    FPCDR_REQUIRE(anchor || !anchor_w, "anchor_w without an anchor");
    FPCDR_REQUIRE(std::isfinite(inv_c) && inv_c >= 0.0f, "inv_c = 1 / scale must be finite and not negative (0: L2)");
    FPCDR_REQUIRE(std::isfinite(w_smooth) && w_smooth >= 0.0f && std::isfinite(w_anchor) && w_anchor >= 0.0f,
                  "the weights must be finite and not negative");
    FPCDR_REQUIRE(((size_t)acc & 7) == 0, "acc must be 8-byte aligned");
    const double n = (double)Ht * (double)Wt;
    const float coef_s = (float)(2.0 * (double)w_smooth / n), coef_a = (float)(2.0 * (double)w_anchor / n);
    const bool vec = Wt % TEX_RUN == 0 &&
                     ((((size_t)tex | (size_t)anchor | (size_t)smooth_w | (size_t)anchor_w | (size_t)grad_tex) & 15) == 0);
    const hipStream_t st = (hipStream_t)stream;
    switch (C) {
    case 1: launch_tex_prior<1>(vec, st, tex, anchor, smooth_w, anchor_w, inv_c, coef_s, coef_a, Ht, Wt, grad_tex, (double *)acc); break;
    case 2: launch_tex_prior<2>(vec, st, tex, anchor, smooth_w, anchor_w, inv_c, coef_s, coef_a, Ht, Wt, grad_tex, (double *)acc); break;
    case 3: launch_tex_prior<3>(vec, st, tex, anchor, smooth_w, anchor_w, inv_c, coef_s, coef_a, Ht, Wt, grad_tex, (double *)acc); break;
    default: launch_tex_prior<4>(vec, st, tex, anchor, smooth_w, anchor_w, inv_c, coef_s, coef_a, Ht, Wt, grad_tex, (double *)acc); break;
    }
    hipLaunchKernelGGL(k_tex_prior_finish, dim3(1), dim3(64), 0, st, (double *)acc, n, w_smooth, w_anchor, part, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

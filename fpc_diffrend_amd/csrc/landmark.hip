// The landmark term of the fit step for gfx950 (MI355X) ("Landmark rule"): named points of the mesh held to their detected
// 2D positions in the captures, a reprojection error in full-resolution raster pixels.
//   k_landmark_points   one workgroup per image: every landmark projected, its value partial, its gradient with respect to the point
//                       (g_q, to a scratch) and the image's gradient with respect to its matrix, reduced over the workgroup
//   k_landmark_gather   one lane per (frame, vertex) over ALL vertices: the vertex's landmark corners summed over the frame's images in a
//                       fixed order -- no float atomics; a vertex without a landmark writes 0, so the kernel is also the fill of grad_x
//   k_penalty_finish<false> with divisor Nc L (penalty_finish.h): per_f, the value, the accumulators zeroed again
#include "landmark_entry.h"
#include "penalty_finish.h"

#include <cmath>

namespace {

// The tables lm_vtx, lm_bary, lm_w and an entry's read and residual: landmark_entry.h.  obs [F Nc,L,3] = (u*, v*, kappa) in raster pixels of
// the W x H capture.  An entry is live when kappa > 0, omega > 0 and p.w > 1e-6; what is not live is switched off by SELECTS, so that a NaN in
// an observation nobody made, or the quotient of a point behind the camera, stays where it is.  coef = weight / (F Nc L).  g_q (may be
// null: value only) [F Nc,L,3]; g_mvp (null with it) [F Nc,4,4]: the twelve entries of the rows x, y, w summed over the workgroup -- DPP
// within a wave, the four waves' partials through LDS in wave order -- and stored whole, row z as 0.  res_out (may be null) [F Nc,L,2] =
// (u - u*, v - v*), NaN where the entry is not live.  Constant indices only: no private segment.
__global__ void __launch_bounds__(256) k_landmark_points(const float *__restrict__ x, const float *__restrict__ mvp,
                                                         const int32_t *__restrict__ lm_vtx, const float *__restrict__ lm_bary,
                                                         const float *__restrict__ lm_w, const float *__restrict__ obs, float ic, float half_w,
                                                         float half_h, int Nc, int V, int L, float coef, float *__restrict__ g_q,
                                                         float *__restrict__ g_mvp, float *__restrict__ res_out, double *__restrict__ acc) {
    __shared__ float s_m[4][12];
    const int n = blockIdx.x;
    const int f = n / Nc;
    const float *xf = x + (size_t)f * V * 3;
    const float *m = mvp + (size_t)n * 16;
    float mx[4], my[4], mw[4];      // the rows x, y, w of the image's matrix (block-uniform)
#pragma unroll
    for (int i = 0; i < 4; ++i) { mx[i] = m[i]; my[i] = m[4 + i]; mw[i] = m[12 + i]; }
    float value = 0.0f;
    float gm[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) gm[i] = 0.0f;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        float p[3];
        LandmarkEntry e;
        landmark_entry(xf, lm_vtx, lm_bary, lm_w, obs + ((size_t)n * L + l) * 3, L, l, p, e);
        const float q[4] = {p[0], p[1], p[2], 1.0f};
        const float px = ((mx[0] * q[0] + mx[1] * q[1]) + mx[2] * q[2]) + mx[3];
        const float py = ((my[0] * q[0] + my[1] * q[1]) + my[2] * q[2]) + my[3];
        const float pw = ((mw[0] * q[0] + mw[1] * q[1]) + mw[2] * q[2]) + mw[3];
        LandmarkResidual r;
        landmark_residual(px, py, pw, e, half_w, half_h, ic, r);
        const bool live = r.live;
        const float sw = r.sw, ru = r.ru, rv = r.rv, d = r.d, wk = e.wk;
        if (live) value += wk * r.rho;
        if (res_out) {
            float *ro = res_out + ((size_t)n * L + l) * 2;
            ro[0] = live ? ru : __builtin_nanf("");
            ro[1] = live ? rv : __builtin_nanf("");
        }
        if (g_q) {
            const float k2 = (coef * wk) * (d * 2.0f);
            const float gu = k2 * ru, gv = k2 * rv;
            const float ax = gu * half_w, ay = gv * half_h;
            float gp[3];      // d value / d (p.x, p.y, p.w)
            gp[0] = live ? ax / sw : 0.0f;
            gp[1] = live ? ay / sw : 0.0f;
            gp[2] = live ? -((ax * px + ay * py) / (sw * sw)) : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                gm[i] += gp[0] * q[i];
                gm[4 + i] += gp[1] * q[i];
                gm[8 + i] += gp[2] * q[i];
            }
            float *g = g_q + ((size_t)n * L + l) * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) g[i] = live ? (mx[i] * gp[0] + my[i] * gp[1]) + mw[i] * gp[2] : 0.0f;
        }
    }
    if (g_mvp) {      // (block-uniform)
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const float t = wave_sum_dpp(gm[i]);
            if (lane == 0) s_m[wave][i] = t;
        }
        __syncthreads();
        if (threadIdx.x < 16) {
            const int row = threadIdx.x >> 2, col = threadIdx.x & 3;
            const int k = (row == 3 ? 8 : 4 * row) + col;      // rows x, y -> 0..7, row w -> 8..11
            const float t = row == 2 ? 0.0f : (s_m[0][k] + s_m[1][k]) + (s_m[2][k] + s_m[3][k]);
            g_mvp[(size_t)n * 16 + threadIdx.x] = t;
        }
    }
    block_add_f64(value, &acc[f]);
}

// grad_x[f,v,:] = sum over the vertex's slots (lm_inc [K,V] slot-major: entries 3 l + k, ascending, pads -1 trailing) of
// lm_bary[k][l] * sum_c g_q[f Nc + c, l, :], c ascending: one lane sums one entry in a fixed order and stores it, bit-identical from run to
// run.  Nearly every vertex has no slot and stores 0 after ONE coalesced read of the table's first row; the few that have one read Nc
// triples per slot, four images a round (their loads in flight together, added in image order).
__global__ void __launch_bounds__(256) k_landmark_gather(const float *__restrict__ g_q, const int32_t *__restrict__ lm_inc,
                                                         const float *__restrict__ lm_bary, int Nc, int V, int L, int K,
                                                         float *__restrict__ grad_x) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int k = 0; k < K; ++k) {
        const int e = lm_inc[(size_t)k * V + v];
        if (e < 0) break;
        const int l = e / 3, corner = e - 3 * l;
        const float b = lm_bary[(size_t)corner * L + l];
        const float *g = g_q + ((size_t)f * Nc * L + l) * 3;
        float tx = 0.0f, ty = 0.0f, tz = 0.0f;
        for (int c0 = 0; c0 < Nc; c0 += 4) {
            float cx[4], cy[4], cz[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool on = c0 + j < Nc;
                const float *gc = g + (size_t)(on ? c0 + j : c0) * L * 3;
                cx[j] = on ? gc[0] : 0.0f; cy[j] = on ? gc[1] : 0.0f; cz[j] = on ? gc[2] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { tx += cx[j]; ty += cy[j]; tz += cz[j]; }
        }
        sx += b * tx; sy += b * ty; sz += b * tz;
    }
    float *o = grad_x + ((size_t)f * V + v) * 3;
    o[0] = sx; o[1] = sy; o[2] = sz;
}

}  // namespace

extern "C" int fpcdr_landmark_penalty(const float *x, const float *mvp, const int32_t *lm_vtx, const float *lm_bary, const float *lm_w,
                                      const int32_t *lm_inc, const float *obs, float inv_c, int32_t width, int32_t height, float *scratch,
                                      float *grad_x, float *grad_mvp, float *res_out, void *acc, float *per, float *out, float weight,
                                      int32_t F, int32_t Nc, int32_t V, int32_t L, int32_t K, void *stream) {
    FPCDR_REQUIRE(x && mvp && lm_vtx && lm_bary && obs && acc && per && out, "null pointer");
    FPCDR_REQUIRE(F > 0 && Nc > 0 && V > 0 && L > 0 && K > 0 && F <= 65535 && (long long)F * Nc <= 0x7fffffffLL, "bad sizes");
    FPCDR_REQUIRE(width > 0 && height > 0, "width and height must be positive");
    FPCDR_REQUIRE(std::isfinite(inv_c) && inv_c >= 0.0f, "inv_c = 1 / scale must be finite and not negative (0: L2)");
    FPCDR_REQUIRE(((size_t)acc & 7) == 0, "acc must be 8-byte aligned");
    FPCDR_REQUIRE((grad_x != nullptr) == (grad_mvp != nullptr), "grad_x and grad_mvp are null together (value only) or not at all");
    FPCDR_REQUIRE(!grad_x || (scratch && lm_inc), "grad_x needs scratch and lm_inc");
    const float coef = weight / (((float)F * (float)Nc) * (float)L);
    hipLaunchKernelGGL(k_landmark_points, dim3(F * Nc), dim3(256), 0, (hipStream_t)stream, x, mvp, lm_vtx, lm_bary, lm_w, obs, inv_c,
                       0.5f * (float)width, 0.5f * (float)height, Nc, V, L, coef, grad_x ? scratch : nullptr, grad_mvp, res_out, (double *)acc);
    if (grad_x)
        hipLaunchKernelGGL(k_landmark_gather, dim3(fpcdr_cdiv(V, 256), F), dim3(256), 0, (hipStream_t)stream, scratch, lm_inc, lm_bary, Nc, V,
                           L, K, grad_x);
    hipLaunchKernelGGL(k_penalty_finish<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, (double *)acc, F, (double)Nc * (double)L, weight,
                       per, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

// One entry of the Landmark rule, the ONE statement that the landmark term (landmark.hip) and the pose solve (landmark_pose.hip,
// whose cost is defined as the term's) both evaluate.  How the point is projected, and what is made of the residual -- gradients there,
// normal equations here --, stays with each kernel.  Constant indices only: no private segment.
#pragma once

#include "common.h"

// the observation (u*, v*), wk = omega kappa, and seen = kappa > 0 && omega > 0: the part of the live test that does not need p.w
struct LandmarkEntry { float us, vs, wk; bool seen; };

// the three corners of landmark l and their weights, from lm_vtx [3,L] int32 and lm_bary [3,L] float32, corner-major
struct LandmarkCorners { int i0, i1, i2; float b0, b1, b2; };

__device__ __forceinline__ LandmarkCorners landmark_corners(const int32_t *__restrict__ lm_vtx, const float *__restrict__ lm_bary, int L, int l) {
    return {lm_vtx[l], lm_vtx[(size_t)L + l], lm_vtx[2 * (size_t)L + l], lm_bary[l], lm_bary[(size_t)L + l], lm_bary[2 * (size_t)L + l]};
}

// landmark l is the point p = sum_k lm_bary[k][l] xf[lm_vtx[k][l]]; lm_w [L] or null: 1.  o: the entry's (u*, v*, kappa) in raster pixels.
__device__ __forceinline__ void landmark_entry(const float *__restrict__ xf, const int32_t *__restrict__ lm_vtx,
                                               const float *__restrict__ lm_bary, const float *__restrict__ lm_w,
                                               const float *__restrict__ o, int L, int l, float (&p)[3], LandmarkEntry &e) {
    const LandmarkCorners c = landmark_corners(lm_vtx, lm_bary, L, l);
    const int i0 = c.i0, i1 = c.i1, i2 = c.i2;
    const float b0 = c.b0, b1 = c.b1, b2 = c.b2;
    const float omega = lm_w ? lm_w[l] : 1.0f;
    const float us = o[0], vs = o[1], kappa = o[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = (b0 * xf[3 * (size_t)i0 + i] + b1 * xf[3 * (size_t)i1 + i]) + b2 * xf[3 * (size_t)i2 + i];
    e = {us, vs, omega * kappa, kappa > 0.0f && omega > 0.0f};
}

// live = seen && p.w > 1e-6, sw = p.w where live (else 1: what is not live is switched off by SELECTS, never by a product with 0), the NDC
// point, the residual in raster pixels of the capture with half sizes (half_w, half_h), s = |r|^2, the robust pair rho(s), d = rho'(s)
struct LandmarkResidual { bool live; float sw, nx, ny, ru, rv, s, rho, d; };

__device__ __forceinline__ void landmark_residual(float px, float py, float pw, const LandmarkEntry &e, float half_w, float half_h, float ic,
                                                  LandmarkResidual &r) {
    r.live = e.seen && pw > 1e-6f;
    r.sw = r.live ? pw : 1.0f;
    r.nx = px / r.sw, r.ny = py / r.sw;
    r.ru = ((r.nx * 0.5f + 0.5f) * (2.0f * half_w) - 0.5f) - e.us;
    r.rv = ((r.ny * 0.5f + 0.5f) * (2.0f * half_h) - 0.5f) - e.vs;
    r.s = r.ru * r.ru + r.rv * r.rv;
    r.rho = r.s, r.d = 1.0f;
    if (ic > 0.0f) {      // (ic = 1 / scale; 0: rho(s) = s) the Charbonnier form without the cancellation, as the motion term has it
        const float zu = r.ru * ic, zv = r.rv * ic;
        const float h = sqrtf(1.0f + (zu * zu + zv * zv));
        r.rho = (2.0f * r.s) / (1.0f + h);
        r.d = 1.0f / h;
    }
}

// The per-frame rigid pose solve from the landmarks for gfx950 (MI355X) ("Pose solve rule"): damped Gauss-Newton on the
// Landmark rule's cost over a frame's rotation and translation, every trial inside ONE launch.
//   k_landmark_pose   one workgroup of 256 per frame.  A pass strides the frame's Nc L entries, every lane with 29 partial sums (the 21
//                     entries of A's upper triangle, the 6 of b, the cost E and the live count), reduces them -- DPP within a wave, the
//                     four waves' partials through LDS in wave order -- and leaves cost AND normal equations of the pose it was given:
//                     a trial's evaluation is also the next trial's linearisation, so a trial is one pass.  Lane 0 solves the damped 6 x 6
//                     system in float64 (Cholesky, unrolled, constant indices: no private segment), publishes the trial pose through LDS
//                     and keeps or rejects it.  No float atomics, a fixed order: bit-identical from run to run.
#include "landmark_entry.h"

#include <cmath>

namespace {

constexpr int POSE_N = 29;      // A (21, upper triangle, row-major), b (6), E, the number of live entries

// the partial sums of one pass at the pose s_pose = (q [4] as stored, t [3]) -> s_new[POSE_N]; ends behind a barrier (an entry: landmark_entry.h)
__device__ __forceinline__ void pose_pass(const float *__restrict__ xf, const float *__restrict__ proj, const float *__restrict__ base,
                                          const int32_t *__restrict__ lm_vtx, const float *__restrict__ lm_bary,
                                          const float *__restrict__ lm_w, const float *__restrict__ obs_f, float ic, float half_w, float half_h,
                                          int Nc, int L, const float *s_pose, float (*s_part)[POSE_N], float *s_new) {
    // R(q / |q|), roma's XYZW form as clip.hip's rigid() has it (block-uniform)
    const float q0 = s_pose[0], q1 = s_pose[1], q2 = s_pose[2], q3 = s_pose[3];
    const float t0 = s_pose[4], t1 = s_pose[5], t2 = s_pose[6];
    const float qn = sqrtf((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
    const float x = q0 / qn, y = q1 / qn, z = q2 / qn, w = q3 / qn;
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const float r00 = 1.0f - (tyy + tzz), r01 = txy - twz, r02 = txz + twy;
    const float r10 = txy + twz, r11 = 1.0f - (txx + tzz), r12 = tyz - twx;
    const float r20 = txz - twy, r21 = tyz + twx, r22 = 1.0f - (txx + tyy);
    float acc[POSE_N];
#pragma unroll
    for (int i = 0; i < POSE_N; ++i) acc[i] = 0.0f;
    const int n = Nc * L;
    for (int e = threadIdx.x; e < n; e += 256) {
        const int c = e / L, l = e - c * L;
        const float *B = base + (size_t)c * 16, *P = proj + (size_t)c * 16;
        float p[3], yb[3], a[3], zz[3];
        LandmarkEntry en;
        landmark_entry(xf, lm_vtx, lm_bary, lm_w, obs_f + (size_t)e * 3, L, l, p, en);
#pragma unroll
        for (int i = 0; i < 3; ++i) yb[i] = ((B[4 * i] * p[0] + B[4 * i + 1] * p[1]) + B[4 * i + 2] * p[2]) + B[4 * i + 3];
        a[0] = (r00 * yb[0] + r01 * yb[1]) + r02 * yb[2];
        a[1] = (r10 * yb[0] + r11 * yb[1]) + r12 * yb[2];
        a[2] = (r20 * yb[0] + r21 * yb[1]) + r22 * yb[2];
        zz[0] = a[0] + t0; zz[1] = a[1] + t1; zz[2] = a[2] + t2;
        const float px = ((P[0] * zz[0] + P[1] * zz[1]) + P[2] * zz[2]) + P[3];
        const float py = ((P[4] * zz[0] + P[5] * zz[1]) + P[6] * zz[2]) + P[7];
        const float pw = ((P[12] * zz[0] + P[13] * zz[1]) + P[14] * zz[2]) + P[15];
        LandmarkResidual r;
        landmark_residual(px, py, pw, en, half_w, half_h, ic, r);
        const bool live = r.live;
        const float sw = r.sw, nx = r.nx, ny = r.ny, ru = r.ru, rv = r.rv, wk = en.wk;
        const float wd = wk * r.d;
        const float ku = half_w / sw, kv = half_h / sw;
        float ju[6], jv[6];      // the residual's Jacobian: (a x g, g)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            ju[3 + i] = ku * (P[i] - nx * P[12 + i]);
            jv[3 + i] = kv * (P[4 + i] - ny * P[12 + i]);
        }
        ju[0] = a[1] * ju[5] - a[2] * ju[4]; ju[1] = a[2] * ju[3] - a[0] * ju[5]; ju[2] = a[0] * ju[4] - a[1] * ju[3];
        jv[0] = a[1] * jv[5] - a[2] * jv[4]; jv[1] = a[2] * jv[3] - a[0] * jv[5]; jv[2] = a[0] * jv[4] - a[1] * jv[3];
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j, ++k) {
                const float term = wd * (ju[i] * ju[j] + jv[i] * jv[j]);
                acc[k] += live ? term : 0.0f;
            }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const float term = wd * (ju[i] * ru + jv[i] * rv);
            acc[21 + i] += live ? term : 0.0f;
        }
        const float term = wk * r.rho;
        acc[27] += live ? term : 0.0f;
        acc[28] += live ? 1.0f : 0.0f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < POSE_N; ++i) {
        const float t = wave_sum_dpp(acc[i]);
        if (lane == 0) s_part[wave][i] = t;
    }
    __syncthreads();
    if (threadIdx.x < POSE_N) s_new[threadIdx.x] = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
    __syncthreads();
}

// (A + lambda diag A) delta = -b by Cholesky in float64 (s_cur: the sums of a pass); rotation = 0: the translation block alone, delta[0..2]
// = 0.  false: a pivot is not positive.  Fully unrolled: every index is a constant.
__device__ __forceinline__ bool pose_solve(const float *s_cur, double lambda, int rotation, double *delta) {
    double M[6][6], rhs[6];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) {
            double v = (double)s_cur[k];
            if (i == j) v = v + lambda * v;
            if (!rotation && i < 3) v = i == j ? 1.0 : 0.0;
            M[i][j] = v;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) rhs[i] = (!rotation && i < 3) ? 0.0 : -(double)s_cur[21 + i];
    bool ok = true;
    double Lc[6][6];      // the lower factor
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = M[j][j];
#pragma unroll
        for (int m = 0; m < j; ++m) dj -= Lc[j][m] * Lc[j][m];
        ok = ok && dj > 0.0;
        const double r = sqrt(ok ? dj : 1.0);
        Lc[j][j] = r;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = M[j][i];
#pragma unroll
            for (int m = 0; m < j; ++m) v -= Lc[i][m] * Lc[j][m];
            Lc[i][j] = v / r;
        }
    }
    double yv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = rhs[i];
#pragma unroll
        for (int m = 0; m < i; ++m) v -= Lc[i][m] * yv[m];
        yv[i] = v / Lc[i][i];
    }
    double dl[6];
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = yv[i];
#pragma unroll
        for (int m = i + 1; m < 6; ++m) v -= Lc[m][i] * dl[m];
        dl[i] = v / Lc[i][i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        ok = ok && dl[i] - dl[i] == 0.0;      // (finite)
        delta[i] = dl[i];
    }
    return ok;
}

// (sin h, cos h) for h >= 0 from +, -, * alone, so that tests/pose_ref.py can restate it to the bit (a library's sine differs from
// another's in the last place): h is halved until it is at most 1/16, the series are summed by Horner (their first neglected terms are
// below 1e-24), and the angle is doubled back.  Each doubling at most doubles the error: 2^6 roundings (7e-15; 1.1e-15
// measured) up to h = pi, the half angle of a full turn.
__device__ __forceinline__ void pose_sincos(double h, double &s, double &c) {
    int k = 0;
    while (h > 0.0625 && k < 64) { h *= 0.5; ++k; }
    const double x = h * h;
    const double sc = 1.0 + x * (-1.0 / 6.0 + x * (1.0 / 120.0 + x * (-1.0 / 5040.0 + x * (1.0 / 362880.0 + x * (-1.0 / 39916800.0)))));
    c = 1.0 + x * (-0.5 + x * (1.0 / 24.0 + x * (-1.0 / 720.0 + x * (1.0 / 40320.0 + x * (-1.0 / 3628800.0 + x * (1.0 / 479001600.0))))));
    s = sc * h;
    for (int i = 0; i < k; ++i) {
        const double s2 = (2.0 * s) * c;
        c = 1.0 - 2.0 * (s * s);
        s = s2;
    }
}

// q' = normalise(exp(delta_omega / 2) (x) q / |q|), t' = t + delta_t, in float64, rounded once
__device__ __forceinline__ void pose_trial(const float *s_best, const double *delta, int rotation, float *s_pose) {
    if (rotation) {
        const double th2 = (delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2];
        const double th = sqrt(th2);
        double sn = 0.0, cs = 1.0;
        pose_sincos(0.5 * th, sn, cs);
        const double sh = th2 < 1e-16 ? 0.5 : sn / th;      // sin(theta / 2) / theta
        const double ax = sh * delta[0], ay = sh * delta[1], az = sh * delta[2], aw = th2 < 1e-16 ? 1.0 : cs;
        const double b0 = s_best[0], b1 = s_best[1], b2 = s_best[2], b3 = s_best[3];
        const double bn = sqrt((b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3));
        const double bx = b0 / bn, by = b1 / bn, bz = b2 / bn, bw = b3 / bn;
        const double cx = ((aw * bx + ax * bw) + ay * bz) - az * by;      // the Hamilton product a (x) b, XYZW
        const double cy = ((aw * by - ax * bz) + ay * bw) + az * bx;
        const double cz = ((aw * bz + ax * by) - ay * bx) + az * bw;
        const double cw = ((aw * bw - ax * bx) - ay * by) - az * bz;
        const double cn = sqrt((cx * cx + cy * cy) + (cz * cz + cw * cw));
        s_pose[0] = (float)(cx / cn); s_pose[1] = (float)(cy / cn); s_pose[2] = (float)(cz / cn); s_pose[3] = (float)(cw / cn);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) s_pose[4 + i] = (float)((double)s_best[4 + i] + delta[3 + i]);
}

__global__ void __launch_bounds__(256) k_landmark_pose(const float *__restrict__ x, const float *__restrict__ proj, const float *__restrict__ base,
                                                       const int32_t *__restrict__ lm_vtx, const float *__restrict__ lm_bary,
                                                       const float *__restrict__ lm_w, const float *__restrict__ obs, float *__restrict__ q,
                                                       float *__restrict__ t, float ic, float half_w, float half_h, int iters, int rotation,
                                                       double lambda0, int Nc, int V, int L, float *__restrict__ info,
                                                       float *__restrict__ normal_out) {
    __shared__ float s_part[4][POSE_N];
    __shared__ float s_new[POSE_N], s_cur[POSE_N];
    __shared__ float s_pose[8], s_best[8];
    __shared__ int s_go, s_try;
    const int f = blockIdx.x;
    const float *xf = x + (size_t)f * V * 3;
    const float *obs_f = obs + (size_t)f * Nc * L * 3;
    if (threadIdx.x < 7) {
        const float v = threadIdx.x < 4 ? q[4 * (size_t)f + threadIdx.x] : t[3 * (size_t)f + (threadIdx.x - 4)];
        s_pose[threadIdx.x] = v;
        s_best[threadIdx.x] = v;
    }
    __syncthreads();
    pose_pass(xf, proj, base, lm_vtx, lm_bary, lm_w, obs_f, ic, half_w, half_h, Nc, L, s_pose, s_part, s_new);
    if (threadIdx.x < POSE_N) {
        s_cur[threadIdx.x] = s_new[threadIdx.x];
        if (normal_out && threadIdx.x < 28) normal_out[28 * (size_t)f + threadIdx.x] = s_new[threadIdx.x];
    }
    double lambda = lambda0;      // (lane 0's)
    int accepted = 0;
    float e_in = 0.0f;
    if (threadIdx.x == 0) {
        e_in = s_new[27];
        s_go = (iters > 0 && s_new[28] >= 3.0f) ? 1 : 0;      // fewer than 3 live entries: the frame stays as it is
    }
    __syncthreads();
    if (s_go) {      // (block-uniform)
        for (int it = 0; it < iters; ++it) {
            if (threadIdx.x == 0) {
                double delta[6];
                const bool ok = pose_solve(s_cur, lambda, rotation, delta);
                if (ok) pose_trial(s_best, delta, rotation, s_pose);
                else lambda = fmin(lambda * 10.0, 1e9);
                s_try = ok ? 1 : 0;
            }
            __syncthreads();
            if (s_try) {      // (block-uniform)
                pose_pass(xf, proj, base, lm_vtx, lm_bary, lm_w, obs_f, ic, half_w, half_h, Nc, L, s_pose, s_part, s_new);
                const bool keep = s_new[28] >= s_cur[28] && s_new[27] < s_cur[27];      // (every lane reads the same sums)
                __syncthreads();
                if (keep) {
                    if (threadIdx.x < POSE_N) s_cur[threadIdx.x] = s_new[threadIdx.x];
                    if (threadIdx.x < 7) s_best[threadIdx.x] = s_pose[threadIdx.x];
                }
                if (threadIdx.x == 0) {
                    if (keep) { lambda = fmax(lambda / 10.0, 1e-9); ++accepted; }
                    else lambda = fmin(lambda * 10.0, 1e9);
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        if (accepted > 0) {
            if (rotation) {
                q[4 * (size_t)f + 0] = s_best[0]; q[4 * (size_t)f + 1] = s_best[1]; q[4 * (size_t)f + 2] = s_best[2]; q[4 * (size_t)f + 3] = s_best[3];
            }
            t[3 * (size_t)f + 0] = s_best[4]; t[3 * (size_t)f + 1] = s_best[5]; t[3 * (size_t)f + 2] = s_best[6];
        }
        info[4 * (size_t)f + 0] = e_in;
        info[4 * (size_t)f + 1] = s_cur[27];
        info[4 * (size_t)f + 2] = s_cur[28];
        info[4 * (size_t)f + 3] = (float)accepted;
    }
}

}  // namespace

extern "C" int fpcdr_landmark_pose(const float *x, const float *proj, const float *base, const int32_t *lm_vtx, const float *lm_bary,
                                   const float *lm_w, const float *obs, float *q, float *t, float inv_c, int32_t width, int32_t height,
                                   int32_t iters, int32_t rotation, float lambda0, float *info, float *normal_out, int32_t F, int32_t Nc,
                                   int32_t V, int32_t L, void *stream) {
    FPCDR_REQUIRE(x && proj && base && lm_vtx && lm_bary && obs && q && t && info, "null pointer");
    FPCDR_REQUIRE(F > 0 && Nc > 0 && V > 0 && L > 0 && (long long)Nc * L <= (1LL << 24) && (long long)F * Nc <= 0x7fffffffLL, "bad sizes");
    FPCDR_REQUIRE(width > 0 && height > 0, "width and height must be positive");
    FPCDR_REQUIRE(iters >= 0, "iters must not be negative");
    FPCDR_REQUIRE(std::isfinite(inv_c) && inv_c >= 0.0f, "inv_c = 1 / scale must be finite and not negative (0: L2)");
    FPCDR_REQUIRE(std::isfinite(lambda0) && lambda0 > 0.0f, "lambda0 must be finite and positive");
    FPCDR_REQUIRE(((((size_t)x | (size_t)proj | (size_t)base | (size_t)lm_vtx | (size_t)lm_bary | (size_t)lm_w | (size_t)obs | (size_t)q |
                     (size_t)t | (size_t)info | (size_t)normal_out) & 3) == 0), "every buffer must be 4-byte aligned");
    hipLaunchKernelGGL(k_landmark_pose, dim3(F), dim3(256), 0, (hipStream_t)stream, x, proj, base, lm_vtx, lm_bary, lm_w, obs, q, t, inv_c,
                       0.5f * (float)width, 0.5f * (float)height, iters, rotation ? 1 : 0, (double)lambda0, Nc, V, L, info, normal_out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

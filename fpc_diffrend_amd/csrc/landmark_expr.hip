// The per-frame blend-weight solve from the landmarks for gfx950 (MI355X) ("Expression solve rule"): damped Gauss-Newton on the
// Landmark rule's cost plus a ridge over a frame's Kb blend weights, every trial inside ONE launch.
//   k_expr_basis      the landmark basis A [3L,Kb] = the rows of the blend basis at the landmarks' corners, once per call, into the scratch.
//   k_landmark_expr   one workgroup of 256 per frame.  A pass: one lane per landmark walks the frame's cameras and leaves the landmark's
//                     3 x 3 block S_l (6) and 3-vector s_l in LDS (float32), its cost and live count go through the pose kernel's
//                     fixed-order reduction.  A pass leaves cost AND (through S_l, s_l) the normal equations of the weights it was given:
//                     a trial's evaluation is also the next trial's linearisation.  A trial assembles H = sum_l A_l^T S_l A_l (packed lower
//                     triangle) and g in float64 in LDS -- a wave per row, a lane per column --, adds ridge and damping, factors it in place
//                     (right-looking Cholesky, two barriers a column), substitutes forward and back, and evaluates the trial weights.
//                     The undamped H is NOT kept: the factorisation overwrites it, and a trial -- kept or rejected -- rebuilds it from the
//                     S_l of the best weights (two S buffers: the best weights' and the trial's).  No float atomics, a fixed order.
//   Two sizes of the one kernel: Kb <= 32 and L <= 128 in 15 KB of LDS (123 registers: four workgroups a CU), anything up to
//   Kb = 160 and L = 512 in 145 KB (one).  Constant indices only in every per-lane array: no private segment.
#include "landmark_entry.h"

#include <cmath>

namespace {

constexpr int EXPR_KB_MAX = 160, EXPR_L_MAX = 512;      // (fpcdr_landmark_expr refuses anything larger)
constexpr int EXPR_KB_SMALL = 32, EXPR_L_SMALL = 128;

__device__ __forceinline__ int tri(int i, int k) { return ((i * (i + 1)) >> 1) + k; }      // (i >= k) packed lower triangle, row-major

__global__ void __launch_bounds__(256) k_expr_basis(const float *__restrict__ B, const int32_t *__restrict__ lm_vtx,
                                                    const float *__restrict__ lm_bary, float *__restrict__ A, int L, int Kb) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3LL * L * Kb) return;
    const int row = (int)(idx / Kb), k = (int)(idx - (long long)row * Kb);
    const int l = row / 3, a = row - 3 * l;
    const LandmarkCorners c = landmark_corners(lm_vtx, lm_bary, L, l);
    A[idx] = (c.b0 * B[(3 * (size_t)c.i0 + a) * Kb + k] + c.b1 * B[(3 * (size_t)c.i1 + a) * Kb + k]) + c.b2 * B[(3 * (size_t)c.i2 + a) * Kb + k];
}

// One pass at the weights w_in + s_dw: S[l] = (S_l: 00 01 02 11 12 22, s_l: 0 1 2) of every landmark, s_en = (E, live entries); ends
// behind a barrier (an entry: landmark_entry.h)
__device__ __forceinline__ void expr_pass(const float *__restrict__ xf, const float *__restrict__ mvp_f, const float *__restrict__ A,
                                          const int32_t *__restrict__ lm_vtx, const float *__restrict__ lm_bary,
                                          const float *__restrict__ lm_w, const float *__restrict__ obs_f, float ic, float half_w, float half_h,
                                          int Nc, int L, int Kb, const float *s_dw, float (*S)[9], float (*s_part)[2], float *s_en) {
    float e_acc = 0.0f, n_acc = 0.0f;
    for (int l = threadIdx.x; l < L; l += 256) {
        const float *A0 = A + 3 * (size_t)l * Kb, *A1 = A0 + Kb, *A2 = A1 + Kb;
        float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;      // A_l (w' - w_in), k ascending
        for (int k = 0; k < Kb; ++k) {
            const float dw = s_dw[k];
            d0 += A0[k] * dw; d1 += A1[k] * dw; d2 += A2[k] * dw;
        }
        float acc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[i] = 0.0f;
        float el = 0.0f, nl = 0.0f;
        for (int c = 0; c < Nc; ++c) {
            const float *M = mvp_f + (size_t)c * 16;
            float p[3];
            LandmarkEntry en;
            landmark_entry(xf, lm_vtx, lm_bary, lm_w, obs_f + ((size_t)c * L + l) * 3, L, l, p, en);
            const float q0 = p[0] + d0, q1 = p[1] + d1, q2 = p[2] + d2;
            const float px = ((M[0] * q0 + M[1] * q1) + M[2] * q2) + M[3];
            const float py = ((M[4] * q0 + M[5] * q1) + M[6] * q2) + M[7];
            const float pw = ((M[12] * q0 + M[13] * q1) + M[14] * q2) + M[15];
            LandmarkResidual r;
            landmark_residual(px, py, pw, en, half_w, half_h, ic, r);
            const bool live = r.live;
            const float we = en.wk * r.d;
            const float ku = half_w / r.sw, kv = half_h / r.sw;
            float gu[3], gv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                gu[i] = ku * (M[i] - r.nx * M[12 + i]);
                gv[i] = kv * (M[4 + i] - r.ny * M[12 + i]);
            }
            int k = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = i; j < 3; ++j, ++k) {
                    const float term = we * (gu[i] * gu[j] + gv[i] * gv[j]);
                    acc[k] += live ? term : 0.0f;
                }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float term = we * (gu[i] * r.ru + gv[i] * r.rv);
                acc[6 + i] += live ? term : 0.0f;
            }
            const float term = en.wk * r.rho;
            el += live ? term : 0.0f;
            nl += live ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) S[l][i] = acc[i];
        e_acc += el;
        n_acc += nl;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float te = wave_sum_dpp(e_acc), tn = wave_sum_dpp(n_acc);
    if (lane == 0) { s_part[wave][0] = te; s_part[wave][1] = tn; }
    __syncthreads();
    if (threadIdx.x < 2) s_en[threadIdx.x] = ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
    __syncthreads();
}

// H = sum_l A_l^T S_l A_l (packed lower triangle into s_M) and g = sum_l A_l^T s_l (into s_g) in float64, l ascending: a wave per row i, a
// lane per column k <= i; u = S_l a_i, the term (u0 a_k0 + u1 a_k1) + u2 a_k2.  Ends behind a barrier.
__device__ __forceinline__ void expr_assemble(const float *__restrict__ A, const float (*S)[9], int L, int Kb, double *s_M, double *s_g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < Kb; i += 4)
        for (int k = lane; k <= i; k += 64) {
            double h = 0.0;
            for (int l = 0; l < L; ++l) {
                const float *Al = A + 3 * (size_t)l * Kb;
                const double ai0 = Al[i], ai1 = Al[Kb + i], ai2 = Al[2 * Kb + i];
                const double ak0 = Al[k], ak1 = Al[Kb + k], ak2 = Al[2 * Kb + k];
                const double s00 = S[l][0], s01 = S[l][1], s02 = S[l][2], s11 = S[l][3], s12 = S[l][4], s22 = S[l][5];
                const double u0 = (s00 * ai0 + s01 * ai1) + s02 * ai2;
                const double u1 = (s01 * ai0 + s11 * ai1) + s12 * ai2;
                const double u2 = (s02 * ai0 + s12 * ai1) + s22 * ai2;
                h += (u0 * ak0 + u1 * ak1) + u2 * ak2;
            }
            s_M[tri(i, k)] = h;
        }
    for (int k = threadIdx.x; k < Kb; k += 256) {
        double g = 0.0;
        for (int l = 0; l < L; ++l) {
            const float *Al = A + 3 * (size_t)l * Kb;
            g += ((double)Al[k] * (double)S[l][6] + (double)Al[Kb + k] * (double)S[l][7]) + (double)Al[2 * Kb + k] * (double)S[l][8];
        }
        s_g[k] = g;
    }
    __syncthreads();
}

// C = E + rs sum_k w_k^2 in float64, k ascending (every lane forms the same sum)
__device__ __forceinline__ double expr_cost(float E, double rs, const float *s_wv, int Kb) {
    double s = 0.0;
    for (int k = 0; k < Kb; ++k) s += (double)s_wv[k] * (double)s_wv[k];
    return (double)E + rs * s;
}

template <int KB, int LB>
__global__ void __launch_bounds__(256) k_landmark_expr(const float *__restrict__ x, const float *__restrict__ mvp, const float *__restrict__ A,
                                                       const int32_t *__restrict__ lm_vtx, const float *__restrict__ lm_bary,
                                                       const float *__restrict__ lm_w, const float *__restrict__ obs, float *__restrict__ w,
                                                       float ic, float half_w, float half_h, int iters, double lambda0, double rs, int Nc, int V,
                                                       int L, int Kb, float *__restrict__ info, double *__restrict__ normal_out) {
    __shared__ double s_M[KB * (KB + 1) / 2];      // H, then the damped matrix, then its lower factor (the diagonal: s_diag)
    __shared__ double s_g[KB], s_y[KB], s_d[KB], s_diag[KB];
    __shared__ float s_S[2][LB][9];
    __shared__ float s_w[KB], s_wt[KB], s_win[KB], s_dw[KB];
    __shared__ int s_dead[KB];
    __shared__ float s_part[4][2], s_en[2];
    __shared__ int s_finite;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NT = (Kb * (Kb + 1)) >> 1;
    const float *xf = x + (size_t)f * V * 3;
    const float *mvp_f = mvp + (size_t)f * Nc * 16;
    const float *obs_f = obs + (size_t)f * Nc * L * 3;
    float *wf = w + (size_t)f * Kb;
    for (int k = tid; k < Kb; k += 256) {
        const float v = wf[k];
        s_w[k] = v; s_wt[k] = v; s_win[k] = v; s_dw[k] = 0.0f;
    }
    __syncthreads();
    int cur = 0;
    expr_pass(xf, mvp_f, A, lm_vtx, lm_bary, lm_w, obs_f, ic, half_w, half_h, Nc, L, Kb, s_dw, s_S[cur], s_part, s_en);
    float E = s_en[0], n = s_en[1];      // (every lane reads the same sums)
    double C = expr_cost(E, rs, s_w, Kb);
    const double C_in = C;
    if (normal_out) {
        double *no = normal_out + (size_t)f * (NT + Kb + 2);
        expr_assemble(A, s_S[cur], L, Kb, s_M, s_g);
        for (int e = tid; e < NT; e += 256) no[e] = s_M[e];
        for (int k = tid; k < Kb; k += 256) no[NT + k] = s_g[k];
        if (tid == 0) { no[NT + Kb] = (double)E; no[NT + Kb + 1] = (double)n; }
        __syncthreads();
    }
    double lambda = lambda0;      // (every lane's: the decisions are block-uniform)
    int accepted = 0;
    const int trials = n >= 3.0f ? iters : 0;      // fewer than 3 live entries: the frame stays as it is
    for (int it = 0; it < trials; ++it) {
        expr_assemble(A, s_S[cur], L, Kb, s_M, s_g);
        // M = H + rs I; a weight with M_kk == 0 is switched off by selects: its row and column the identity, its right-hand side 0
        for (int k = tid; k < Kb; k += 256) s_dead[k] = (s_M[tri(k, k)] + rs == 0.0) ? 1 : 0;
        if (tid == 0) s_finite = 1;
        __syncthreads();
        for (int i = wave; i < Kb; i += 4)
            for (int k = lane; k <= i; k += 64) {
                double v = s_M[tri(i, k)];
                if (i == k) {
                    const double m = v + rs;
                    v = m + lambda * m;
                }
                if (s_dead[i] | s_dead[k]) v = i == k ? 1.0 : 0.0;
                s_M[tri(i, k)] = v;
            }
        for (int k = tid; k < Kb; k += 256) s_g[k] = s_dead[k] ? 0.0 : -(s_g[k] + rs * (double)s_w[k]);
        __syncthreads();
        // right-looking Cholesky: column j is finished, then every remaining entry takes its one update
        bool ok = true;
        for (int j = 0; j < Kb; ++j) {
            const double dj = s_M[tri(j, j)];
            ok = ok && dj > 0.0;
            const double r = sqrt(ok ? dj : 1.0);
            const int i = j + 1 + tid;
            if (i < Kb) s_M[tri(i, j)] = s_M[tri(i, j)] / r;
            if (tid == 0) s_diag[j] = r;
            __syncthreads();
            for (int i2 = j + 1 + wave; i2 < Kb; i2 += 4) {
                const double lij = s_M[tri(i2, j)];
                for (int k = j + 1 + lane; k <= i2; k += 64) s_M[tri(i2, k)] = s_M[tri(i2, k)] - lij * s_M[tri(k, j)];
            }
            __syncthreads();
        }
        // L y = rhs by columns (an entry's updates in ascending j), L^T delta = y by columns (descending j)
        for (int j = 0; j < Kb; ++j) {
            const double yj = s_g[j] / s_diag[j];
            const int i = j + 1 + tid;
            if (i < Kb) s_g[i] = s_g[i] - s_M[tri(i, j)] * yj;
            if (tid == 0) s_y[j] = yj;
            __syncthreads();
        }
        for (int j = Kb - 1; j >= 0; --j) {
            const double dj = s_y[j] / s_diag[j];
            if (tid < j) s_y[tid] = s_y[tid] - s_M[tri(j, tid)] * dj;
            if (tid == 0) s_d[j] = dj;
            __syncthreads();
        }
        for (int k = tid; k < Kb; k += 256) {
            const double dl = s_d[k];
            if (!(dl - dl == 0.0)) s_finite = 0;      // (finite)
            const float wn = (float)((double)s_w[k] + dl);
            s_wt[k] = wn;
            s_dw[k] = wn - s_win[k];
        }
        __syncthreads();
        const bool tryit = ok && s_finite != 0;      // (block-uniform)
        bool keep = false;
        if (tryit) {
            expr_pass(xf, mvp_f, A, lm_vtx, lm_bary, lm_w, obs_f, ic, half_w, half_h, Nc, L, Kb, s_dw, s_S[cur ^ 1], s_part, s_en);
            const float E2 = s_en[0], n2 = s_en[1];
            const double C2 = expr_cost(E2, rs, s_wt, Kb);
            keep = n2 >= n && C2 < C;
            if (keep) { E = E2; n = n2; C = C2; cur ^= 1; }
        }
        __syncthreads();
        if (keep) {
            for (int k = tid; k < Kb; k += 256) s_w[k] = s_wt[k];
            lambda = fmax(lambda / 10.0, 1e-9);
            ++accepted;
        } else {
            lambda = fmin(lambda * 10.0, 1e9);
        }
        __syncthreads();
    }
    if (accepted > 0)
        for (int k = tid; k < Kb; k += 256) wf[k] = s_w[k];
    if (tid == 0) {
        info[4 * (size_t)f + 0] = (float)C_in;
        info[4 * (size_t)f + 1] = (float)C;
        info[4 * (size_t)f + 2] = n;
        info[4 * (size_t)f + 3] = (float)accepted;
    }
}

}  // namespace

extern "C" size_t fpcdr_landmark_expr_scratch_bytes(int32_t F, int32_t L, int32_t Kb) {
    (void)F;      // (the landmark basis is shared by all frames)
    if (L <= 0 || Kb <= 0) return 0;
    return 3 * (size_t)L * (size_t)Kb * sizeof(float);
}

extern "C" int fpcdr_landmark_expr(const float *x, const float *mvp, const float *basis, const int32_t *lm_vtx, const float *lm_bary,
                                   const float *lm_w, const float *obs, float *w, float inv_c, float ridge, int32_t width, int32_t height,
                                   int32_t iters, float lambda0, float *info, double *normal_out, void *scratch, size_t scratch_bytes,
                                   int32_t F, int32_t Nc, int32_t V, int32_t L, int32_t Kb, void *stream) {
    FPCDR_REQUIRE(x && mvp && basis && lm_vtx && lm_bary && obs && w && info, "null pointer");
    FPCDR_REQUIRE(F > 0 && Nc > 0 && V > 0 && L > 0 && Kb > 0 && (long long)F * Nc <= 0x7fffffffLL && (long long)Nc * L <= (1LL << 24), "bad sizes");
    FPCDR_REQUIRE(Kb <= EXPR_KB_MAX, "Kb must not exceed 160");
    FPCDR_REQUIRE(L <= EXPR_L_MAX, "L must not exceed 512");
    FPCDR_REQUIRE(width > 0 && height > 0, "width and height must be positive");
    FPCDR_REQUIRE(iters >= 0, "iters must not be negative");
    FPCDR_REQUIRE(std::isfinite(inv_c) && inv_c >= 0.0f, "inv_c = 1 / scale must be finite and not negative (0: L2)");
    FPCDR_REQUIRE(std::isfinite(ridge) && ridge >= 0.0f, "ridge must be finite and not negative");
    FPCDR_REQUIRE(std::isfinite(lambda0) && lambda0 > 0.0f, "lambda0 must be finite and positive");
    FPCDR_REQUIRE(scratch && scratch_bytes >= fpcdr_landmark_expr_scratch_bytes(F, L, Kb), "scratch is missing or smaller than fpcdr_landmark_expr_scratch_bytes");
    FPCDR_REQUIRE(((((size_t)x | (size_t)mvp | (size_t)basis | (size_t)lm_vtx | (size_t)lm_bary | (size_t)lm_w | (size_t)obs | (size_t)w |
                     (size_t)info | (size_t)scratch) & 3) == 0), "every float32 / int32 buffer must be 4-byte aligned");
    FPCDR_REQUIRE(((size_t)normal_out & 7) == 0, "normal_out must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float *A = (float *)scratch;
    hipLaunchKernelGGL(k_expr_basis, dim3(fpcdr_cdiv(3LL * L * Kb, 256)), dim3(256), 0, st, basis, lm_vtx, lm_bary, A, L, Kb);
    FPCDR_CHECK_LAUNCH();
    const double rs = ((double)ridge * (double)Nc) * (double)L;
    const float hw = 0.5f * (float)width, hh = 0.5f * (float)height;
    if (Kb <= EXPR_KB_SMALL && L <= EXPR_L_SMALL)
        hipLaunchKernelGGL((k_landmark_expr<EXPR_KB_SMALL, EXPR_L_SMALL>), dim3(F), dim3(256), 0, st, x, mvp, A, lm_vtx, lm_bary, lm_w, obs, w, inv_c,
                           hw, hh, iters, (double)lambda0, rs, Nc, V, L, Kb, info, normal_out);
    else
        hipLaunchKernelGGL((k_landmark_expr<EXPR_KB_MAX, EXPR_L_MAX>), dim3(F), dim3(256), 0, st, x, mvp, A, lm_vtx, lm_bary, lm_w, obs, w, inv_c, hw,
                           hh, iters, (double)lambda0, rs, Nc, V, L, Kb, info, normal_out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

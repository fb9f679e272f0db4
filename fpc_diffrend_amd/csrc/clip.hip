// transform_clip for a minibatch, forward and backward, and the chain of matrices in front of it (below), for gfx950 (MI355X).
//
// Performs the work of reference src/torch/camera.py:11-23 (`posw @ mvp.T` on homogeneous vertices) for all
// B = F x Nc images of a step at once: image b = f * Nc + c uses vertex buffer f and matrix b.  The reference (and
// fpc_diffrend_amd.camera.transform_clip) leave this to torch.matmul; at [288,15002,4] x [4,4] the batched GEMM
// picked by the BLAS library costs 0.3 ms forward and 0.6 ms backward for 69 MB of traffic, so the fit loop uses
// these streaming kernels instead (the views of a frame read the same vertices through L2).
#include "common.h"

namespace {

__global__ void __launch_bounds__(256) k_clip_fwd(const float *__restrict__ mvp, const float *__restrict__ verts, int V, int Nc,
                                                  float4 *__restrict__ out) {
    const int b = blockIdx.y, f = b / Nc;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float *m = mvp + (size_t)b * 16;   // wave-uniform: scalar loads
    const float *p = verts + ((size_t)f * V + v) * 3;
    const float x = p[0], y = p[1], z = p[2];
    float4 o;
    o.x = x * m[0] + y * m[1] + z * m[2] + m[3];
    o.y = x * m[4] + y * m[5] + z * m[6] + m[7];
    o.z = x * m[8] + y * m[9] + z * m[10] + m[11];
    o.w = x * m[12] + y * m[13] + z * m[14] + m[15];
    out[(size_t)b * V + v] = o;
}

// d/d verts: thread = (frame, vertex), sums over the frame's Nc views (no atomics)
__global__ void __launch_bounds__(256) k_clip_bwd_verts(const float *__restrict__ mvp, const float4 *__restrict__ g, int V, int Nc,
                                                        float *__restrict__ g_verts) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    float gx = 0.f, gy = 0.f, gz = 0.f;
    for (int c = 0; c < Nc; ++c) {
        const int b = f * Nc + c;
        const float *m = mvp + (size_t)b * 16;
        const float4 q = g[(size_t)b * V + v];
        gx += q.x * m[0] + q.y * m[4] + q.z * m[8] + q.w * m[12];
        gy += q.x * m[1] + q.y * m[5] + q.z * m[9] + q.w * m[13];
        gz += q.x * m[2] + q.y * m[6] + q.z * m[10] + q.w * m[14];
    }
    float *o = g_verts + ((size_t)f * V + v) * 3;
    o[0] = gx; o[1] = gy; o[2] = gz;
}

// d/d mvp[b][i][j] = sum_v g[b][v][i] * (x,y,z,1)[j]: wave DPP sums, then 16 atomics per wave
constexpr int MVP_VPB = 2048;   // vertices per workgroup of k_clip_bwd_mvp (8 per thread)
__global__ void __launch_bounds__(256) k_clip_bwd_mvp(const float *__restrict__ verts, const float4 *__restrict__ g, int V, int Nc,
                                                      float *__restrict__ g_mvp) {
    // grad_mvp[b] = sum_v grad_out[b][v] (x) (verts[v], 1): per-thread partial sums over 8 vertices, one DPP reduction per
    // wave, LDS across the four waves, then 16 atomics per workgroup (same-address atomics are what this kernel waits for)
    __shared__ float s_part[4][16];
    const int b = blockIdx.y, f = b / Nc;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    const int v_end = min((int)(blockIdx.x + 1) * MVP_VPB, V);
    for (int v = blockIdx.x * MVP_VPB + threadIdx.x; v < v_end; v += 256) {
        const float4 q = g[(size_t)b * V + v];
        const float *p = verts + ((size_t)f * V + v) * 3;
        const float pw[4] = {p[0], p[1], p[2], 1.0f};
        const float gi[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i * 4 + j] += gi[i] * pw[j];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float s = wave_sum_dpp(acc[i]);
        if (lane == 0) s_part[wave][i] = s;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const float s = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
        if (s != 0.0f) atomicAdd(g_mvp + (size_t)b * 16 + threadIdx.x, s);
    }
}

// Both gradients from ONE pass over grad_out (69 MB at 288 x 15 k vertices, read twice by the two kernels above: 2 x 16 us): a thread
// takes CLIP_VPT vertices of one frame (a workgroup 256 * CLIP_VPT consecutive ones) through all views, as k_clip_bwd_verts does for
// one; the 16 products of a view are summed over the thread's vertices first, then over the wave (DPP), then over the four waves through
// an LDS row per view: one atomic per (view, entry) and workgroup.  (One vertex per thread spends the kernel on the 144 wave sums.)
constexpr int CLIP_VIEWS = 16;      // views per LDS round
constexpr int CLIP_VPT = 4;
__global__ void __launch_bounds__(256) k_clip_bwd_both(const float *__restrict__ mvp, const float *__restrict__ verts,
                                                       const float4 *__restrict__ g, int V, int Nc, float *__restrict__ g_verts,
                                                       float *__restrict__ g_mvp) {
    __shared__ float s_part[CLIP_VIEWS][4][16];
    const int f = blockIdx.y;
    const int v0 = blockIdx.x * (256 * CLIP_VPT) + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float pw[CLIP_VPT][4], gx[CLIP_VPT], gy[CLIP_VPT], gz[CLIP_VPT];
    bool ok[CLIP_VPT];
#pragma unroll
    for (int u = 0; u < CLIP_VPT; ++u) {
        const int v = v0 + u * 256;
        ok[u] = v < V;
        const float *pv = verts + ((size_t)f * V + (ok[u] ? v : 0)) * 3;
        pw[u][0] = ok[u] ? pv[0] : 0.0f; pw[u][1] = ok[u] ? pv[1] : 0.0f; pw[u][2] = ok[u] ? pv[2] : 0.0f; pw[u][3] = ok[u] ? 1.0f : 0.0f;
        gx[u] = 0.f; gy[u] = 0.f; gz[u] = 0.f;
    }
    for (int c0 = 0; c0 < Nc; c0 += CLIP_VIEWS) {
        const int nc = min(CLIP_VIEWS, Nc - c0);
        for (int c = 0; c < nc; ++c) {
            const int b = f * Nc + c0 + c;
            const float *m = mvp + (size_t)b * 16;
            float4 q[CLIP_VPT];
#pragma unroll
            for (int u = 0; u < CLIP_VPT; ++u) q[u] = ok[u] ? g[(size_t)b * V + v0 + u * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
            float acc[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
            for (int u = 0; u < CLIP_VPT; ++u) {
                gx[u] += q[u].x * m[0] + q[u].y * m[4] + q[u].z * m[8] + q[u].w * m[12];
                gy[u] += q[u].x * m[1] + q[u].y * m[5] + q[u].z * m[9] + q[u].w * m[13];
                gz[u] += q[u].x * m[2] + q[u].y * m[6] + q[u].z * m[10] + q[u].w * m[14];
                const float gi[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i * 4 + j] += gi[i] * pw[u][j];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float sm = wave_sum_dpp(acc[i]);
                if (lane == 0) s_part[c][wave][i] = sm;
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nc * 16; e += 256) {
            const int c = e >> 4, i = e & 15;
            const float sm = s_part[c][0][i] + s_part[c][1][i] + s_part[c][2][i] + s_part[c][3][i];
            if (sm != 0.0f) atomicAdd(g_mvp + (size_t)(f * Nc + c0 + c) * 16 + i, sm);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < CLIP_VPT; ++u)
        if (ok[u]) {
            float *o = g_verts + ((size_t)f * V + v0 + u * 256) * 3;
            o[0] = gx[u]; o[1] = gy[u]; o[2] = gz[u];
        }
}

// ---------------------------------------------------------------------------------------------
// mvp[f,c] = P_c . Rt(q_f, t_f) . (Rt(q_c, t_c) . MV_c)      reference fit.py:541-553, camera.py:117-132 and
// roma.unitquat_to_rotmat (XYZW, applied WITHOUT normalisation, as the reference does after its whole-tensor
// "renormalisation", fit.py:616-618).  One thread per (frame, camera); ~120 tiny torch launches otherwise.
struct M4 { float m[4][4]; };
__device__ __forceinline__ M4 m4_load(const float *p) {
    M4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) r.m[i][j] = p[4 * i + j];
    return r;
}
__device__ __forceinline__ M4 m4_mul(const M4 &a, const M4 &b) {
    M4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += a.m[i][k] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
__device__ __forceinline__ M4 m4_mul_tn(const M4 &a, const M4 &b) {   // a^T b
    M4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += a.m[k][i] * b.m[k][j];
            r.m[i][j] = s;
        }
    return r;
}
__device__ __forceinline__ M4 m4_mul_nt(const M4 &a, const M4 &b) {   // a b^T
    M4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s += a.m[i][k] * b.m[j][k];
            r.m[i][j] = s;
        }
    return r;
}
__device__ __forceinline__ M4 rigid(const float *q, const float *t) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    M4 r;
    r.m[0][0] = 1.0f - (tyy + tzz); r.m[0][1] = txy - twz;          r.m[0][2] = txz + twy;          r.m[0][3] = t[0];
    r.m[1][0] = txy + twz;          r.m[1][1] = 1.0f - (txx + tzz); r.m[1][2] = tyz - twx;          r.m[1][3] = t[1];
    r.m[2][0] = txz - twy;          r.m[2][1] = tyz + twx;          r.m[2][2] = 1.0f - (txx + tyy); r.m[2][3] = t[2];
    r.m[3][0] = 0.0f; r.m[3][1] = 0.0f; r.m[3][2] = 0.0f; r.m[3][3] = 1.0f;
    return r;
}
// dL/d(q, t) from dL/d rigid(q, t): adds 7 values
__device__ __forceinline__ void rigid_bwd(const float *q, const M4 &G, float *gq, float *gt) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float (*g)[4] = G.m;
    const float gx = 2.0f * (y * (g[0][1] + g[1][0]) + z * (g[0][2] + g[2][0]) + w * (g[2][1] - g[1][2])) - 4.0f * x * (g[1][1] + g[2][2]);
    const float gy = 2.0f * (x * (g[0][1] + g[1][0]) + z * (g[1][2] + g[2][1]) + w * (g[0][2] - g[2][0])) - 4.0f * y * (g[0][0] + g[2][2]);
    const float gz = 2.0f * (x * (g[0][2] + g[2][0]) + y * (g[1][2] + g[2][1]) + w * (g[1][0] - g[0][1])) - 4.0f * z * (g[0][0] + g[1][1]);
    const float gw = 2.0f * (z * (g[1][0] - g[0][1]) + y * (g[0][2] - g[2][0]) + x * (g[2][1] - g[1][2]));
    atomicAdd(gq + 0, gx); atomicAdd(gq + 1, gy); atomicAdd(gq + 2, gz); atomicAdd(gq + 3, gw);
    atomicAdd(gt + 0, g[0][3]); atomicAdd(gt + 1, g[1][3]); atomicAdd(gt + 2, g[2][3]);
}

// The rows of the parameter tables that step entry (f, c) reads.  IDX = false: frame f, view c, camera c (the entries without index
// arrays; the three pointers are null and never read).  IDX = true: the frames / views of the step are given as INDEX arrays into the full
// parameter tables (the reference's run shape draws one random (camera, frame) per step: as torch ops that was seven index_select launches
// forward and four zero-fill + index_add pairs backward around kernels that take 3 us).  frame_idx [Fb] or null (frames 0 .. Fb - 1);
// view_idx [Nc] or null: rows of proj / t_mv; cam_of_view [views] or null: row of q_cam / t_cam for a view (the cameras a Fitter was
// given).  (A template argument, not a test of the pointers at run time: each form keeps the instruction stream it had as a kernel of its own.)
template <bool IDX>
__device__ __forceinline__ void mvp_rows(const long long *frame_idx, const long long *view_idx, const long long *cam_of_view, int f, int c,
                                         int &fr, int &cv, int &cp) {
    fr = (IDX && frame_idx) ? (int)frame_idx[f] : f;
    cv = (IDX && view_idx) ? (int)view_idx[c] : c;
    cp = (IDX && cam_of_view) ? (int)cam_of_view[cv] : cv;
}

template <bool IDX>
__global__ void k_mvp_fwd(const float *__restrict__ proj, const float *__restrict__ t_mv, const float *__restrict__ q_cam,
                          const float *__restrict__ t_cam, const float *__restrict__ q_frame, const float *__restrict__ t_frame,
                          const long long *__restrict__ frame_idx, const long long *__restrict__ view_idx,
                          const long long *__restrict__ cam_of_view, int Fb, int Nc, float *__restrict__ mvp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Fb * Nc) return;
    const int f = i / Nc, c = i - f * Nc;
    int fr, cv, cp;
    mvp_rows<IDX>(frame_idx, view_idx, cam_of_view, f, c, fr, cv, cp);
    const M4 B = m4_mul(rigid(q_cam + 4 * cp, t_cam + 3 * cp), m4_load(t_mv + 16 * cv));
    const M4 X = m4_mul(rigid(q_frame + 4 * fr, t_frame + 3 * fr), B);
    const M4 M = m4_mul(m4_load(proj + 16 * cv), X);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) mvp[(size_t)i * 16 + 4 * r + k] = M.m[r][k];
}

// The backward adds into the FULL tables (zeroed by the caller); two step entries that name the same row add into it, as index_select's
// backward does.
template <bool IDX>
__global__ void k_mvp_bwd(const float *__restrict__ proj, const float *__restrict__ t_mv, const float *__restrict__ q_cam,
                          const float *__restrict__ t_cam, const float *__restrict__ q_frame, const float *__restrict__ t_frame,
                          const long long *__restrict__ frame_idx, const long long *__restrict__ view_idx,
                          const long long *__restrict__ cam_of_view, const float *__restrict__ g_mvp, int Fb, int Nc,
                          float *__restrict__ gq_cam, float *__restrict__ gt_cam, float *__restrict__ gq_frame, float *__restrict__ gt_frame) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Fb * Nc) return;
    const int f = i / Nc, c = i - f * Nc;
    int fr, cv, cp;
    mvp_rows<IDX>(frame_idx, view_idx, cam_of_view, f, c, fr, cv, cp);
    const M4 MV = m4_load(t_mv + 16 * cv);
    const M4 B = m4_mul(rigid(q_cam + 4 * cp, t_cam + 3 * cp), MV);
    const M4 A = rigid(q_frame + 4 * fr, t_frame + 3 * fr);
    const M4 gX = m4_mul_tn(m4_load(proj + 16 * cv), m4_load(g_mvp + (size_t)i * 16));   // P^T dL/dM
    const M4 gA = m4_mul_nt(gX, B);                                                       // dL/dX B^T
    const M4 gC = m4_mul_nt(m4_mul_tn(A, gX), MV);                                        // (A^T dL/dX) MV^T
    rigid_bwd(q_frame + 4 * fr, gA, gq_frame + 4 * fr, gt_frame + 3 * fr);
    rigid_bwd(q_cam + 4 * cp, gC, gq_cam + 4 * cp, gt_cam + 3 * cp);
}

}  // namespace

extern "C" int fpcdr_mvp_fwd_indexed(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                                     const float *t_frame, const int64_t *frame_idx, const int64_t *view_idx, const int64_t *cam_of_view,
                                     float *mvp, int32_t Fb, int32_t Nc, void *stream) {
    FPCDR_REQUIRE(proj && t_mv && q_cam && t_cam && q_frame && t_frame && mvp, "null pointer");
    FPCDR_REQUIRE(Fb > 0 && Nc > 0, "bad sizes");
    hipLaunchKernelGGL(k_mvp_fwd<true>, dim3(fpcdr_cdiv((long long)Fb * Nc, 64)), dim3(64), 0, (hipStream_t)stream, proj, t_mv, q_cam, t_cam,
                       q_frame, t_frame, (const long long *)frame_idx, (const long long *)view_idx, (const long long *)cam_of_view, Fb, Nc, mvp);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_mvp_bwd_indexed(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                                     const float *t_frame, const int64_t *frame_idx, const int64_t *view_idx, const int64_t *cam_of_view,
                                     const float *grad_mvp, float *gq_cam, float *gt_cam, float *gq_frame, float *gt_frame, int32_t Fb,
                                     int32_t Nc, void *stream) {
    FPCDR_REQUIRE(proj && t_mv && q_cam && t_cam && q_frame && t_frame && grad_mvp && gq_cam && gt_cam && gq_frame && gt_frame,
                  "null pointer");
    FPCDR_REQUIRE(Fb > 0 && Nc > 0, "bad sizes");
    hipLaunchKernelGGL(k_mvp_bwd<true>, dim3(fpcdr_cdiv((long long)Fb * Nc, 64)), dim3(64), 0, (hipStream_t)stream, proj, t_mv, q_cam, t_cam,
                       q_frame, t_frame, (const long long *)frame_idx, (const long long *)view_idx, (const long long *)cam_of_view, grad_mvp,
                       Fb, Nc, gq_cam, gt_cam, gq_frame, gt_frame);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_mvp_fwd(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                             const float *t_frame, float *mvp, int32_t Fb, int32_t Nc, void *stream) {
    FPCDR_REQUIRE(proj && t_mv && q_cam && t_cam && q_frame && t_frame && mvp, "null pointer");
    FPCDR_REQUIRE(Fb > 0 && Nc > 0, "bad sizes");
    const long long *none = nullptr;
    hipLaunchKernelGGL(k_mvp_fwd<false>, dim3(fpcdr_cdiv((long long)Fb * Nc, 64)), dim3(64), 0, (hipStream_t)stream, proj, t_mv, q_cam,
                       t_cam, q_frame, t_frame, none, none, none, Fb, Nc, mvp);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_mvp_bwd(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                             const float *t_frame, const float *grad_mvp, float *gq_cam, float *gt_cam, float *gq_frame,
                             float *gt_frame, int32_t Fb, int32_t Nc, void *stream) {
    FPCDR_REQUIRE(proj && t_mv && q_cam && t_cam && q_frame && t_frame && grad_mvp && gq_cam && gt_cam && gq_frame && gt_frame,
                  "null pointer");
    FPCDR_REQUIRE(Fb > 0 && Nc > 0, "bad sizes");
    const long long *none = nullptr;
    hipLaunchKernelGGL(k_mvp_bwd<false>, dim3(fpcdr_cdiv((long long)Fb * Nc, 64)), dim3(64), 0, (hipStream_t)stream, proj, t_mv, q_cam,
                       t_cam, q_frame, t_frame, none, none, none, grad_mvp, Fb, Nc, gq_cam, gt_cam, gq_frame, gt_frame);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_transform_clip_fwd(const float *mvp, const float *verts, float *out, int32_t F, int32_t Nc, int32_t V,
                                        void *stream) {
    FPCDR_REQUIRE(mvp && verts && out, "null pointer");
    FPCDR_REQUIRE(F > 0 && Nc > 0 && V > 0 && (long long)F * Nc <= 65535, "bad sizes");
    hipLaunchKernelGGL(k_clip_fwd, dim3(fpcdr_cdiv(V, 256), F * Nc), dim3(256), 0, (hipStream_t)stream, mvp, verts, V, Nc,
                       (float4 *)out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_transform_clip_bwd(const float *mvp, const float *verts, const float *grad_out, float *grad_verts,
                                        float *grad_mvp, int32_t F, int32_t Nc, int32_t V, void *stream) {
    FPCDR_REQUIRE(mvp && verts && grad_out, "null pointer");
    FPCDR_REQUIRE(F > 0 && Nc > 0 && V > 0 && (long long)F * Nc <= 65535, "bad sizes");
    hipStream_t st = (hipStream_t)stream;
    if (grad_verts && grad_mvp) {
        hipLaunchKernelGGL(k_clip_bwd_both, dim3(fpcdr_cdiv(V, 256 * CLIP_VPT), F), dim3(256), 0, st, mvp, verts, (const float4 *)grad_out, V, Nc,
                           grad_verts, grad_mvp);
        FPCDR_CHECK_LAUNCH();
        return FPCDR_OK;
    }
    if (grad_verts)
        hipLaunchKernelGGL(k_clip_bwd_verts, dim3(fpcdr_cdiv(V, 256), F), dim3(256), 0, st, mvp, (const float4 *)grad_out, V, Nc,
                           grad_verts);
    if (grad_mvp)
        hipLaunchKernelGGL(k_clip_bwd_mvp, dim3(fpcdr_cdiv(V, MVP_VPB), F * Nc), dim3(256), 0, st, verts, (const float4 *)grad_out, V,
                           Nc, grad_mvp);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

// The bending term ("Bend rule"): every hinge's dihedral angle against its angle in a rest shape.
//   k_bend_hinges   one lane per (mesh, hinge): t = 1 - cos(theta - theta_rest) and the four gradient vectors of the hinge's corners
//   k_bend_gather   one lane per (mesh, vertex): the vertex's hinge corners summed in a fixed order -- no float atomics
//   k_bend_finish   per_f, the value, the accumulators zeroed again (k_stretch_finish's contract with divisor H)
#include "common.h"

// Where k_bend_hinges leaves the three floats of corner `role` of hinge h of one mesh, and where k_bend_gather finds them.
//   1: [4,3,H]   component-major: each of the twelve stores of the hinge pass is coalesced over the wave; the gather reads three words
//                H apart, from lines its neighbouring lanes (vertices whose hinges are neighbours in the table) read too
//   0: [H,4,3]   the corner's three floats are adjacent (one 12-byte read per slot of the gather), but a lane of the hinge pass writes
//                twelve words 48 bytes from its neighbour's: every store instruction touches 24 lines of 128 bytes for 256 bytes
// Measured both ways at 32 meshes of the 15002-vertex sphere (profiles/bend_time.txt): 111 us a call against 200 us.  1 is the layout
// of the ABI; 0 remains as a build option for that measurement (scripts/time_bend.py --alt-lib).
#ifndef FPCDR_BEND_COMPONENT_MAJOR
#define FPCDR_BEND_COMPONENT_MAJOR 1
#endif
__device__ __forceinline__ size_t bend_slot(int h, int role, int k, int H) {
    return FPCDR_BEND_COMPONENT_MAJOR ? (size_t)(role * 3 + k) * (size_t)H + (size_t)h : ((size_t)h * 4 + role) * 3 + k;
}

// hinge_vtx [4,H] role-major: p0, p1 (the edge in the direction face f0 runs through it), q0 (f0's third vertex), q1 (f1's; stored as
// -1 - q1 where f1 runs through the edge in the SAME direction as f0, sigma = -1).  rest_cs [2,H] = (cos, sin) of the rest angle, or null:
// (1, 0).  coef = weight / (F H).  hinge_grad (may be null: value only) receives d value / d corner for a unit upstream.
__global__ void __launch_bounds__(256) k_bend_hinges(const float *__restrict__ x, const int32_t *__restrict__ hinge_vtx,
                                                     const float *__restrict__ rest_cs, int V, int H, float coef,
                                                     float *__restrict__ hinge_grad, double *__restrict__ acc) {
    __shared__ double s_part[4];
    const int f = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.x * blockDim.x + threadIdx.x;
    float t = 0.0f;      // (a lane without a hinge: 0)
    if (h < H) {
        const float *xf = x + (size_t)f * V * 3;
        const int i0 = hinge_vtx[h], i1 = hinge_vtx[(size_t)H + h], j0 = hinge_vtx[2 * (size_t)H + h];
        int j1 = hinge_vtx[3 * (size_t)H + h];
        const float sigma = j1 < 0 ? -1.0f : 1.0f;
        if (j1 < 0) j1 = -1 - j1;
        const float p0x = xf[3 * (size_t)i0], p0y = xf[3 * (size_t)i0 + 1], p0z = xf[3 * (size_t)i0 + 2];
        const float p1x = xf[3 * (size_t)i1], p1y = xf[3 * (size_t)i1 + 1], p1z = xf[3 * (size_t)i1 + 2];
        const float q0x = xf[3 * (size_t)j0], q0y = xf[3 * (size_t)j0 + 1], q0z = xf[3 * (size_t)j0 + 2];
        const float q1x = xf[3 * (size_t)j1], q1y = xf[3 * (size_t)j1 + 1], q1z = xf[3 * (size_t)j1 + 2];
        const float ex = p1x - p0x, ey = p1y - p0y, ez = p1z - p0z;
        const float ax = q0x - p0x, ay = q0y - p0y, az = q0z - p0z;
        const float bx = q1x - p0x, by = q1y - p0y, bz = q1z - p0z;
        // n0 = e x a,  n1 = sigma (b x e)
        const float n0x = ey * az - ez * ay, n0y = ez * ax - ex * az, n0z = ex * ay - ey * ax;
        const float n1x = sigma * (by * ez - bz * ey), n1y = sigma * (bz * ex - bx * ez), n1z = sigma * (bx * ey - by * ex);
        const float e2 = ex * ex + ey * ey + ez * ez;
        const float m0 = n0x * n0x + n0y * n0y + n0z * n0z, m1 = n1x * n1x + n1y * n1y + n1z * n1z;
        const bool live = e2 > 0.0f && m0 > 0.0f && m1 > 0.0f;      // a degenerate hinge: c = s = 0, t = 1, no gradient
        const float L = live ? sqrtf(e2) : 1.0f, l0 = live ? sqrtf(m0) : 1.0f, l1 = live ? sqrtf(m1) : 1.0f;
        const float u0x = n0x / l0, u0y = n0y / l0, u0z = n0z / l0;
        const float u1x = n1x / l1, u1y = n1y / l1, u1z = n1z / l1;
        const float hx = ex / L, hy = ey / L, hz = ez / L;
        float c = u0x * u1x + u0y * u1y + u0z * u1z;
        float s = (u0y * u1z - u0z * u1y) * hx + (u0z * u1x - u0x * u1z) * hy + (u0x * u1y - u0y * u1x) * hz;
        if (!live) { c = 0.0f; s = 0.0f; }
        const float cr = rest_cs ? rest_cs[h] : 1.0f, sr = rest_cs ? rest_cs[(size_t)H + h] : 0.0f;
        const float cd = c * cr + s * sr, sd = s * cr - c * sr;
        t = cd > 0.0f ? (sd * sd) / (1.0f + cd) : 1.0f - cd;
        if (hinge_grad) {
            // d theta / d corner: a0 = n0 / |n0|^2, a1 = sigma n1 / |n1|^2, times d t / d theta = sin delta and coef
            const float k = live ? sd * coef : 0.0f;
            const float sm0 = live ? m0 : 1.0f, sm1 = live ? m1 : 1.0f;
            const float a0x = n0x / sm0, a0y = n0y / sm0, a0z = n0z / sm0;
            // (a1 by the consistently oriented normal (q1 - p0) x e = sigma n1: flipping f1's orientation moves theta by pi, not its slope)
            const float a1x = sigma * n1x / sm1, a1y = sigma * n1y / sm1, a1z = sigma * n1z / sm1;
            // ((q0 - p1) . e) / L, ((q1 - p1) . e) / L, ((p0 - q0) . e) / L, ((p0 - q1) . e) / L
            const float w00 = ((q0x - p1x) * ex + (q0y - p1y) * ey + (q0z - p1z) * ez) / L;
            const float w01 = ((q1x - p1x) * ex + (q1y - p1y) * ey + (q1z - p1z) * ez) / L;
            const float w10 = ((p0x - q0x) * ex + (p0y - q0y) * ey + (p0z - q0z) * ez) / L;
            const float w11 = ((p0x - q1x) * ex + (p0y - q1y) * ey + (p0z - q1z) * ez) / L;
            float *g = hinge_grad + (size_t)f * H * 12;
            const float kL = -(k * L), nk = -k;
            g[bend_slot(h, 0, 0, H)] = nk * (w00 * a0x + w01 * a1x);
            g[bend_slot(h, 0, 1, H)] = nk * (w00 * a0y + w01 * a1y);
            g[bend_slot(h, 0, 2, H)] = nk * (w00 * a0z + w01 * a1z);
            g[bend_slot(h, 1, 0, H)] = nk * (w10 * a0x + w11 * a1x);
            g[bend_slot(h, 1, 1, H)] = nk * (w10 * a0y + w11 * a1y);
            g[bend_slot(h, 1, 2, H)] = nk * (w10 * a0z + w11 * a1z);
            g[bend_slot(h, 2, 0, H)] = kL * a0x;
            g[bend_slot(h, 2, 1, H)] = kL * a0y;
            g[bend_slot(h, 2, 2, H)] = kL * a0z;
            g[bend_slot(h, 3, 0, H)] = kL * a1x;
            g[bend_slot(h, 3, 1, H)] = kL * a1y;
            g[bend_slot(h, 3, 2, H)] = kL * a1z;
        }
    }
    const float ws = wave_sum_dpp(t);
    if (lane == 0) s_part[wave] = (double)ws;
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_fetch_add(&acc[f], s_part[0] + s_part[1] + s_part[2] + s_part[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grad_x[f,v,:] = the sum of the hinge corners at v, slot by slot (hinge_inc [K,V] slot-major: 4 h + role, ascending, pads -1 trailing);
// one lane sums one entry in a fixed order and stores it: bit-identical from run to run; a vertex without a slot gets 0.
__global__ void __launch_bounds__(256) k_bend_gather(const float *__restrict__ hinge_grad, const int32_t *__restrict__ hinge_inc, int V,
                                                     int H, int K, float *__restrict__ grad_x) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float *g = hinge_grad + (size_t)f * H * 12;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    // eight slots a round: their entries are fetched together, then their corners, then added in slot order.  (Slot by slot, every add
    // waits for two dependent loads, and the lane of a pole -- 240 corners on the sphere -- outlasts the rest of the kernel: 45 us of a
    // 156 us call.)  A pad adds 0.
    for (int k0 = 0; k0 < K; k0 += 8) {
        int e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = k0 + j < K ? hinge_inc[(size_t)(k0 + j) * V + v] : -1;
        if (e[0] < 0) break;
        float cx[8], cy[8], cz[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool on = e[j] >= 0;
            const int h = on ? e[j] >> 2 : 0, role = on ? e[j] & 3 : 0;
            cx[j] = on ? g[bend_slot(h, role, 0, H)] : 0.0f;
            cy[j] = on ? g[bend_slot(h, role, 1, H)] : 0.0f;
            cz[j] = on ? g[bend_slot(h, role, 2, H)] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { sx += cx[j]; sy += cy[j]; sz += cz[j]; }
    }
    float *o = grad_x + ((size_t)f * V + v) * 3;
    o[0] = sx; o[1] = sy; o[2] = sz;
}

// per_f, the value, and the accumulators zeroed for the next call; H = 0: everything 0
__global__ void __launch_bounds__(256) k_bend_finish(double *__restrict__ acc, int F, int H, float weight, float *__restrict__ per,
                                                     float *__restrict__ out) {
    __shared__ double s_tot[256];
    double tot = 0.0;
    for (int i = threadIdx.x; i < F; i += blockDim.x) {
        const double p = H > 0 ? acc[i] / (double)H : 0.0;
        per[i] = (float)p;
        tot += p;
        acc[i] = 0.0;
    }
    s_tot[threadIdx.x] = tot;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) s_tot[threadIdx.x] += s_tot[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)((double)weight * s_tot[0] / (double)F);
}

extern "C" int fpcdr_bend_penalty(const float *x, const int32_t *hinge_vtx, const float *rest_cs, const int32_t *hinge_inc, float *hinge_grad,
                                  float *grad_x, void *acc, float *per, float *out, float weight, int32_t F, int32_t V, int32_t H,
                                  int32_t K, void *stream) {
    FPCDR_REQUIRE(x && acc && per && out, "null pointer");
    FPCDR_REQUIRE(F > 0 && V > 0 && H >= 0 && K > 0 && F <= 65535, "bad sizes");
    FPCDR_REQUIRE(hinge_vtx || H == 0, "null pointer (hinge_vtx)");
    FPCDR_REQUIRE(((size_t)acc & 7) == 0, "acc must be 8-byte aligned");
    FPCDR_REQUIRE(!grad_x || (hinge_inc && (hinge_grad || H == 0)), "grad_x needs hinge_inc and hinge_grad");
    const float coef = H > 0 ? weight / ((float)F * (float)H) : 0.0f;
    if (H > 0)
        hipLaunchKernelGGL(k_bend_hinges, dim3(fpcdr_cdiv(H, 256), F), dim3(256), 0, (hipStream_t)stream, x, hinge_vtx, rest_cs, V, H, coef,
                           grad_x ? hinge_grad : nullptr, (double *)acc);
    if (grad_x)
        hipLaunchKernelGGL(k_bend_gather, dim3(fpcdr_cdiv(V, 256), F), dim3(256), 0, (hipStream_t)stream, hinge_grad, hinge_inc, V, H, K, grad_x);
    hipLaunchKernelGGL(k_bend_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (double *)acc, F, H, weight, per, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

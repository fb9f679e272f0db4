// The mesh regularisers of the fit step for gfx950 (MI355X): the uniform Laplacian (gather, and the penalty forward and backward), the
// stretch term, the bending term and the motion term across the frames.  The penalties share one contract: the value kernel's workgroups
// add float partials to their mesh's double accumulator (block_add_f64), and one finish kernel behind the kernel boundary
// (k_penalty_finish) forms per_f and the value and leaves the accumulators zero for the next call.  Both live in penalty_finish.h, which
// the landmark term (landmark.hip) shares.
#include "penalty_finish.h"

#include <cmath>

namespace {

// Uniform-Laplacian gather over a static, padded one-ring table (reference regulariser, fit.py:581 via pytorch3d):
//   mode 0 (forward):   out[f][v] = inv_deg[v] * sum_n x[f][n] - x[f][v]            (L x,   L = D^-1 A - I)
//   mode 1 (backward):  out[f][v] = sum_n inv_deg[n] * x[f][n] - x[f][v]            (L^T x, L^T = A D^-1 - I)
// nbr [V,D] holds neighbour indices, entries >= V are padding.  Both directions are gathers: no atomics.
// ring_walk: one vertex's ring, acc[i] = sum over the ring's slots d (neighbour n) of term(owner, d, n, in, c)[i].  `owner` is the vertex
// whose ring slot d belongs to (the calling lane's own in the unrolled part, the heavy vertex's in the wave part below), so a term may
// read per-slot tables [D,V] and the owner's own data; `in` = the slot holds a neighbour -- a pad slot is handed a valid index and must
// give zeros.
// Slot-major table: consecutive threads read consecutive entries; a vertex's ring is stored front to back, so the
// first pad ends it (a UV sphere has two poles of degree ~100 among vertices of degree 6).  Eight slots are
// fetched together and their neighbours gathered together: the kernel is a chain of dependent loads otherwise
// (one slot per trip is ~100 dependent round trips for the two pole threads, 40 us of a launch whose other threads are done after 3).
// Rings longer than the first eight slots (a pole, the centre of a fan) are finished by the WHOLE WAVE, one such vertex at a time: lane l
// takes slots 8 + l, 72 + l, ..., N DPP sums hand the result to the owner.  (Left to its own thread a ring of 150 is 19 dependent
// rounds of index load + gather, ~40 us during which the launch's other 480 k threads have long finished.)  Every lane of the wave must
// call this, `ok` = the lane has a vertex.
template <int N, typename Term>
__device__ __forceinline__ void ring_walk(const int32_t *__restrict__ nbr, int V, int D, int v, bool ok, Term term, float (&acc)[N]) {
    constexpr int U = 8;
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.f;
    int nb[U];
#pragma unroll
    for (int d = 0; d < U; ++d) nb[d] = (ok && d < D) ? nbr[(size_t)d * V + v] : V;
    {
        float c[U][N];
#pragma unroll
        for (int d = 0; d < U; ++d) {
            const bool in = nb[d] < V;
            term(ok ? v : 0, d, in ? nb[d] : (ok ? v : 0), in, c[d]);
        }
#pragma unroll
        for (int d = 0; d < U; ++d)
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] += c[d][i];
    }
    const int lane = threadIdx.x & 63;
    unsigned long long heavy = __ballot(D > U && nb[U - 1] < V);
    while (heavy) {
        const int leader = __builtin_ctzll(heavy);
        heavy &= heavy - 1;
        const int hv = __shfl(v, leader, 64);
        float p[N];
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = 0.f;
        for (int d = U + lane; d < D; d += 64) {
            const int n = nbr[(size_t)d * V + hv];
            if (n < V) {
                float c[N];
                term(hv, d, n, true, c);
#pragma unroll
                for (int i = 0; i < N; ++i) p[i] += c[i];
            }
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float t = wave_sum_dpp(p[i]);
            if (lane == leader) acc[i] += t;
        }
    }
}

// The Laplacian's use of the walk: sum over the ring of w_n * fetch(n), w_n = inv_deg[n] (mode 1) or 1 (mode 0).
template <typename Fetch>
__device__ __forceinline__ void ring_sum(const int32_t *__restrict__ nbr, const float *__restrict__ inv_deg, int V, int D, int mode, int v, bool ok,
                                         Fetch fetch, float &sx, float &sy, float &sz) {
    float acc[3];
    ring_walk<3>(nbr, V, D, v, ok, [&](int, int, int n, bool in, float (&c)[3]) {
        const float w = in ? (mode ? inv_deg[n] : 1.0f) : 0.0f;
        float gx, gy, gz;
        fetch(n, gx, gy, gz);
        c[0] = w * gx; c[1] = w * gy; c[2] = w * gz;
    }, acc);
    sx = acc[0]; sy = acc[1]; sz = acc[2];
}

// (MODE is a template argument: as a kernel argument the unrolled ring walk branched on it slot by slot)
template <int MODE>
__global__ void __launch_bounds__(256) k_lap_gather(const float *__restrict__ x, const int32_t *__restrict__ nbr,
                                                    const float *__restrict__ inv_deg, int V, int D, float *__restrict__ out) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = v < V;
    const float *xf = x + (size_t)f * V * 3;
    float sx, sy, sz;
    ring_sum(nbr, inv_deg, V, D, MODE, v, ok, [&](int n, float &a, float &b, float &c) { a = xf[3 * n]; b = xf[3 * n + 1]; c = xf[3 * n + 2]; },
             sx, sy, sz);
    if (!ok) return;
    const float s = MODE ? 1.0f : inv_deg[v];
    float *o = out + ((size_t)f * V + v) * 3;
    o[0] = s * sx - xf[3 * v]; o[1] = s * sy - xf[3 * v + 1]; o[2] = s * sz - xf[3 * v + 2];
}

// The Laplacian term of the reference's objective (fit.py:581: weight * mesh_laplacian_smoothing(mesh)^2, one mesh per step; a batch
// takes the mean of the squares) as ONE launch each way instead of a gather and a dozen torch kernels:
//   per_f = mean_v || (L x_f)_v ||,   value = weight / F * sum_f per_f^2.
// Forward: every workgroup adds its vertices' norms to its mesh's double accumulator (one relaxed device-scope add per workgroup);
// k_penalty_finish<true> with divisor V behind it forms the value and stores per_f for the backward.
// REST: the term measures against a rest shape, d = L x - rest_lap (rest_lap [V,3] = L x_rest, made once by this very kernel without
// REST, so that d is exactly 0 at x = x_rest); `lap` then holds d, which the backward kernel takes as it takes L x.
template <bool REST>
__global__ void __launch_bounds__(256) k_lap_penalty_fwd(const float *__restrict__ x, const int32_t *__restrict__ nbr,
                                                         const float *__restrict__ inv_deg, const float *__restrict__ rest_lap, int F, int V, int D,
                                                         float *__restrict__ lap, double *__restrict__ acc) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    float nrm = 0.0f;
    const float *xf = x + (size_t)f * V * 3;
    float sx, sy, sz;
    ring_sum(nbr, inv_deg, V, D, 0, v, v < V, [&](int n, float &a, float &b, float &c) { a = xf[3 * n]; b = xf[3 * n + 1]; c = xf[3 * n + 2]; },
             sx, sy, sz);
    if (v < V) {
        const float s = inv_deg[v];
        float lx = s * sx - xf[3 * v], ly = s * sy - xf[3 * v + 1], lz = s * sz - xf[3 * v + 2];
        if (REST) { lx -= rest_lap[3 * v]; ly -= rest_lap[3 * v + 1]; lz -= rest_lap[3 * v + 2]; }
        float *o = lap + ((size_t)f * V + v) * 3;
        o[0] = lx; o[1] = ly; o[2] = lz;
        nrm = sqrtf(lx * lx + ly * ly + lz * lz);
    }
    block_add_f64(nrm, &acc[f]);
}

// Backward: d value / d x = L^T y,  y_v = c_f * lap_v / ||lap_v||,  c_f = upstream * weight * 2 per_f / (F V)  (0 where lap_v = 0,
// as torch's norm does); y is formed on the fly from the saved Laplacian inside the transposed gather.
__global__ void __launch_bounds__(256) k_lap_penalty_bwd(const float *__restrict__ lap, const int32_t *__restrict__ nbr,
                                                         const float *__restrict__ inv_deg, const float *__restrict__ per,
                                                         const float *__restrict__ upstream, int F, int V, int D, float weight,
                                                         float *__restrict__ grad_x) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = v < V;
    const float *lf = lap + (size_t)f * V * 3;
    const float cf = upstream[0] * weight * 2.0f * per[f] / ((float)F * (float)V);
    auto y = [&](int n, float &a, float &b, float &c) {
        const float lx = lf[3 * n], ly = lf[3 * n + 1], lz = lf[3 * n + 2];
        const float nr = sqrtf(lx * lx + ly * ly + lz * lz);
        const float s = nr > 0.0f ? cf / nr : 0.0f;
        a = s * lx; b = s * ly; c = s * lz;
    };
    float sx, sy, sz, yx, yy, yz;
    ring_sum(nbr, inv_deg, V, D, 1, v, ok, y, sx, sy, sz);
    if (!ok) return;
    y(v, yx, yy, yz);
    float *o = grad_x + ((size_t)f * V + v) * 3;
    o[0] = sx - yx; o[1] = sy - yy; o[2] = sz - yz;
}

// The stretch term ("Stretch rule"): every edge's length against its length in a rest shape (rest_len [D,V], aligned with nbr;
// null: against the constant `target`, the reference's mesh_edge_loss, fit.py:580),
//   per_f = 1 / (2 E) sum_v sum_d s^2,  s = |x_n - x_v| - l,   value = weight / F * sum_f per_f   (every edge is seen from both ends).
// Value partials AND the gradient from one walk of the ring: d value / d x_v = coef * sum_d (s / len) (x_v - x_n), coef = 2 weight / (F E),
// needs v's own ring only -- a gather, no float atomics; a slot of length 0 gives 0, as torch's norm does.  The value goes the way of
// k_lap_penalty_fwd: one double add per workgroup, k_penalty_finish<false> with divisor 2 E behind the kernel boundary (E = 0: everything 0).
__global__ void __launch_bounds__(256) k_stretch_penalty(const float *__restrict__ x, const int32_t *__restrict__ nbr,
                                                         const float *__restrict__ rest_len, float target, int V, int D, float coef,
                                                         float *__restrict__ grad_x, double *__restrict__ acc) {
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = v < V;
    const float *xf = x + (size_t)f * V * 3;
    float a[4];      // sum_d (s / len) (x_v - x_n), and sum_d s^2
    ring_walk<4>(nbr, V, D, v, ok, [&](int o, int d, int n, bool in, float (&c)[4]) {
        const float ex = xf[3 * n] - xf[3 * o], ey = xf[3 * n + 1] - xf[3 * o + 1], ez = xf[3 * n + 2] - xf[3 * o + 2];
        const float len = sqrtf(ex * ex + ey * ey + ez * ez);
        const float l = rest_len ? (in ? rest_len[(size_t)d * V + o] : 0.0f) : target;
        const float s = len - l;
        const float q = (in && len > 0.0f) ? s / len : 0.0f;
        c[0] = -(q * ex); c[1] = -(q * ey); c[2] = -(q * ez);
        c[3] = in ? s * s : 0.0f;
    }, a);
    if (ok && grad_x) {
        float *o = grad_x + ((size_t)f * V + v) * 3;
        o[0] = coef * a[0]; o[1] = coef * a[1]; o[2] = coef * a[2];
    }
    block_add_f64(a[3], &acc[f]);      // (a lane without a vertex has no slot: 0)
}

// The bending term ("Bend rule"): every hinge's dihedral angle against its angle in a rest shape.
//   k_bend_hinges   one lane per (mesh, hinge): t = 1 - cos(theta - theta_rest) and the four gradient vectors of the hinge's corners
//   k_bend_gather   one lane per (mesh, vertex): the vertex's hinge corners summed in a fixed order -- no float atomics
//   k_penalty_finish<false> with divisor H: per_f, the value, the accumulators zeroed again (H = 0: everything 0)

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
    const int f = blockIdx.y;
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
    block_add_f64(t, &acc[f]);
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

// The motion term ("Motion rule"): the step's meshes held smooth in TIME, a difference across the frames of one vertex,
//   ORDER 2: a_f = x_{f-1} - 2 x_f + x_{f+1}   (m_f = 1 iff both neighbours are in the call and one frame number away)
//   ORDER 1: a_f = x_{f+1} - x_f               (m_f = 1 iff frame f + 1 is in the call and one frame number away)
//   s = |a|^2,  rho(s) = s  (ic = 0)  or  2 c^2 (sqrt(1 + s / c^2) - 1) in the form without the cancellation (csrc/robust.hip),
//   per_f = m_f / V sum_v w_v rho(s_{f,v}),   value = weight / F * sum_f per_f.
// One lane per (frame, vertex), not one per vertex walking the frames: at V = 15 k the walk is 59 workgroups for 256 CUs, each a chain
// of F dependent rounds; the grid of F x V / 256 workgroups fills the chip at every size the fit uses, and the price -- every position is
// read by the lanes of up to 2 ORDER + 1 frames -- is paid in L2 (32 x 15002 x 12 bytes = 5.8 MB).  The lane forms the stencils centred
// on f - 1, f, f + 1 (ORDER 1: on f - 1, f) from x at f - ORDER .. f + ORDER of its own vertex: its own stencil gives the value partial,
// all of them give the gradient  coef * (b_{f-1} - 2 b_f + b_{f+1})  (ORDER 1: coef * (b_{f-1} - b_f)),  b = m w rho'(s) a,
// coef = 2 weight / (F V) -- a gather: no float atomics, no scratch, every entry stored once.  The frame numbers are read here, on the
// device (frame_t null: consecutive), block-uniform: a captured step whose subset changes per replay replays correctly.  A frame index
// outside 0 .. F - 1 is clamped for the load (in bounds, whatever the flags) and its stencils are switched off by SELECTS, not by a
// product with 0, so that a NaN in a frame no valid stencil reaches stays where it is.  Constant indices only: no private segment.
template <int ORDER>
__global__ void __launch_bounds__(256) k_motion_penalty(const float *__restrict__ x, const int64_t *__restrict__ frame_t,
                                                        const float *__restrict__ vertex_w, float ic, int F, int V, float coef,
                                                        float *__restrict__ grad_x, double *__restrict__ acc) {
    constexpr int NF = 2 * ORDER + 1;      // the frames f - ORDER .. f + ORDER, slot k = frame f - ORDER + k
    const int f = blockIdx.y;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    // step[k]: the slots k and k + 1 are both frames of the call, one frame number apart
    bool step[NF - 1];
#pragma unroll
    for (int k = 0; k < NF - 1; ++k) {
        const int g = f - ORDER + k;
        const bool in = g >= 0 && g + 1 < F;
        const int gc = in ? g : 0;
        step[k] = in && (frame_t ? frame_t[gc + 1] - frame_t[gc] == 1 : true);
    }
    float value = 0.0f;      // (a lane without a vertex: 0)
    if (v < V) {
        float p[NF][3];
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            const int g = min(max(f - ORDER + k, 0), F - 1);
            const float *xg = x + ((size_t)g * V + v) * 3;
            p[k][0] = xg[0]; p[k][1] = xg[1]; p[k][2] = xg[2];
        }
        const float w = vertex_w ? vertex_w[v] : 1.0f;
        // the stencils: ORDER 2 centred on the slots 1, 2, 3 (the lane's own: 2), ORDER 1 from the slots 0, 1 (the lane's own: 1)
        constexpr int NS = ORDER == 2 ? 3 : 2, OWN = 1;
        float b[NS][3];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const bool m = ORDER == 2 ? (step[j] && step[j + 1]) : step[j];
            float a[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)      // (two differences of neighbouring positions, each exact where the positions are within a factor of 2)
                a[i] = ORDER == 2 ? (p[j][i] - p[j + 1][i]) + (p[j + 2][i] - p[j + 1][i]) : p[j + 1][i] - p[j][i];
            const float s = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
            float rho = s, d = 1.0f;
            if (ic > 0.0f) {
                const float zx = a[0] * ic, zy = a[1] * ic, zz = a[2] * ic;
                const float h = sqrtf(1.0f + (zx * zx + zy * zy + zz * zz));
                rho = (2.0f * s) / (1.0f + h);
                d = 1.0f / h;
            }
            const float q = w * d;
#pragma unroll
            for (int i = 0; i < 3; ++i) b[j][i] = m ? q * a[i] : 0.0f;
            if (j == OWN) value = m ? w * rho : 0.0f;
        }
        if (grad_x) {
            float *o = grad_x + ((size_t)f * V + v) * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = coef * (ORDER == 2 ? (b[0][i] + b[2][i]) - 2.0f * b[1][i] : b[0][i] - b[1][i]);
        }
    }
    block_add_f64(value, &acc[f]);
}

// (both Laplacian forward entries; rest_lap null: the plain term)
void lap_penalty_fwd(const float *x, const int32_t *nbr, const float *inv_deg, const float *rest_lap, float *lap, void *acc, float *per,
                     float *out, float weight, int32_t F, int32_t V, int32_t D, void *stream) {
    // acc: F doubles (+ one spare 8-byte slot: the size of earlier ABI versions), zero on entry and zero again when the call has run
    const dim3 grid(fpcdr_cdiv(V, 256), F);
    if (rest_lap)
        hipLaunchKernelGGL(k_lap_penalty_fwd<true>, grid, dim3(256), 0, (hipStream_t)stream, x, nbr, inv_deg, rest_lap, F, V, D, lap, (double *)acc);
    else
        hipLaunchKernelGGL(k_lap_penalty_fwd<false>, grid, dim3(256), 0, (hipStream_t)stream, x, nbr, inv_deg, rest_lap, F, V, D, lap, (double *)acc);
    hipLaunchKernelGGL(k_penalty_finish<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, (double *)acc, F, (double)V, weight, per, out);
}

}  // namespace

extern "C" int fpcdr_laplacian_gather(const float *x, const int32_t *nbr, const float *inv_deg, float *out, int32_t F, int32_t V,
                                      int32_t D, int32_t transpose, void *stream) {
    FPCDR_REQUIRE(x && nbr && inv_deg && out, "null pointer");
    FPCDR_REQUIRE(F > 0 && V > 0 && D > 0 && F <= 65535, "bad sizes");
    if (transpose)
        hipLaunchKernelGGL(k_lap_gather<1>, dim3(fpcdr_cdiv(V, 256), F), dim3(256), 0, (hipStream_t)stream, x, nbr, inv_deg, V, D, out);
    else
        hipLaunchKernelGGL(k_lap_gather<0>, dim3(fpcdr_cdiv(V, 256), F), dim3(256), 0, (hipStream_t)stream, x, nbr, inv_deg, V, D, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

// What both Laplacian forward entries ask of their arguments (a macro: FPCDR_REQUIRE reports the name of the entry it stands in)
#define LAP_PENALTY_FWD_REQUIRE()                                                      \
    FPCDR_REQUIRE(x && nbr && inv_deg && lap && acc && per && out, "null pointer");    \
    FPCDR_REQUIRE(F > 0 && V > 0 && D > 0 && F <= 65535, "bad sizes");                 \
    FPCDR_REQUIRE(((size_t)acc & 7) == 0, "acc must be 8-byte aligned")

extern "C" int fpcdr_laplacian_penalty_fwd(const float *x, const int32_t *nbr, const float *inv_deg, float *lap, void *acc, float *per,
                                           float *out, float weight, int32_t F, int32_t V, int32_t D, void *stream) {
    LAP_PENALTY_FWD_REQUIRE();
    lap_penalty_fwd(x, nbr, inv_deg, nullptr, lap, acc, per, out, weight, F, V, D, stream);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_laplacian_penalty_rest_fwd(const float *x, const int32_t *nbr, const float *inv_deg, const float *rest_lap, float *lap,
                                                void *acc, float *per, float *out, float weight, int32_t F, int32_t V, int32_t D,
                                                void *stream) {
    LAP_PENALTY_FWD_REQUIRE();
    lap_penalty_fwd(x, nbr, inv_deg, rest_lap, lap, acc, per, out, weight, F, V, D, stream);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}
#undef LAP_PENALTY_FWD_REQUIRE

extern "C" int fpcdr_laplacian_penalty_bwd(const float *lap, const int32_t *nbr, const float *inv_deg, const float *per,
                                           const float *upstream, float *grad_x, float weight, int32_t F, int32_t V, int32_t D,
                                           void *stream) {
    FPCDR_REQUIRE(lap && nbr && inv_deg && per && upstream && grad_x, "null pointer");
    FPCDR_REQUIRE(F > 0 && V > 0 && D > 0 && F <= 65535, "bad sizes");
    hipLaunchKernelGGL(k_lap_penalty_bwd, dim3(fpcdr_cdiv(V, 256), F), dim3(256), 0, (hipStream_t)stream, lap, nbr, inv_deg, per, upstream,
                       F, V, D, weight, grad_x);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_stretch_penalty(const float *x, const int32_t *nbr, const float *rest_len, float target, float *grad_x, void *acc,
                                     float *per, float *out, float weight, int32_t F, int32_t V, int32_t D, int32_t E, void *stream) {
    FPCDR_REQUIRE(x && nbr && acc && per && out, "null pointer");
    FPCDR_REQUIRE(F > 0 && V > 0 && D > 0 && F <= 65535 && E >= 0, "bad sizes");
    FPCDR_REQUIRE(((size_t)acc & 7) == 0, "acc must be 8-byte aligned");
    const float coef = E > 0 ? 2.0f * weight / ((float)F * (float)E) : 0.0f;
    hipLaunchKernelGGL(k_stretch_penalty, dim3(fpcdr_cdiv(V, 256), F), dim3(256), 0, (hipStream_t)stream, x, nbr, rest_len, target, V, D, coef,
                       grad_x, (double *)acc);
    hipLaunchKernelGGL(k_penalty_finish<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, (double *)acc, F, 2.0 * (double)E, weight, per, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_motion_penalty(const float *x, const int64_t *frame_t, const float *vertex_w, float inv_c, int32_t order, float *grad_x,
                                    void *acc, float *per, float *out, float weight, int32_t F, int32_t V, void *stream) {
    FPCDR_REQUIRE(x && acc && per && out, "null pointer");
    FPCDR_REQUIRE(F > 0 && V > 0 && F <= 65535, "bad sizes");
    FPCDR_REQUIRE(order == 1 || order == 2, "order must be 1 or 2");
    FPCDR_REQUIRE(std::isfinite(inv_c) && inv_c >= 0.0f, "inv_c = 1 / scale must be finite and not negative (0: L2)");
    FPCDR_REQUIRE(((size_t)acc & 7) == 0, "acc must be 8-byte aligned");
    const float coef = 2.0f * weight / ((float)F * (float)V);
    const dim3 grid(fpcdr_cdiv(V, 256), F);
    if (order == 2)
        hipLaunchKernelGGL(k_motion_penalty<2>, grid, dim3(256), 0, (hipStream_t)stream, x, frame_t, vertex_w, inv_c, F, V, coef, grad_x,
                           (double *)acc);
    else
        hipLaunchKernelGGL(k_motion_penalty<1>, grid, dim3(256), 0, (hipStream_t)stream, x, frame_t, vertex_w, inv_c, F, V, coef, grad_x,
                           (double *)acc);
    hipLaunchKernelGGL(k_penalty_finish<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, (double *)acc, F, (double)V, weight, per, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
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
    hipLaunchKernelGGL(k_penalty_finish<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, (double *)acc, F, (double)H, weight, per, out);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

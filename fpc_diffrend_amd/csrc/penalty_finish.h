// What the penalty terms in front of the objective share (mesh_reg.hip: the mesh regularisers; landmark.hip: the landmark term).  Not part
// of the C ABI.  The contract: the value kernel's workgroups add float partials to their mesh's double accumulator (block_add_f64), and
// one finish kernel behind the kernel boundary (k_penalty_finish) forms per_f and the value and leaves the accumulators zero for the
// next call.
#pragma once
#include "common.h"

namespace {

// The value tail of a penalty kernel: the workgroup's 256 lane values summed (DPP within a wave, the four waves' partials as doubles
// through LDS) and added to *dst by ONE relaxed agent-scope add.  Every thread of the workgroup must call it, once per kernel.
__device__ __forceinline__ void block_add_f64(float lane_value, double *dst) {
    __shared__ double s_part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float ws = wave_sum_dpp(lane_value);
    if (lane == 0) s_part[wave] = (double)ws;
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_fetch_add(dst, s_part[0] + s_part[1] + s_part[2] + s_part[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The finish of every penalty, one workgroup: p_f = acc[f] / divisor (divisor 0, a mesh without edges or hinges: 0), per[f] = p_f,
// value = weight / F * sum_f p_f (SQUARE: p_f^2, the Laplacian term), and the accumulators zeroed for the next call.  The kernel boundary
// in front of it orders the value kernel's adds before its loads, no fence or ticket.  (r3 let the last workgroup to finish do this behind
// a ticket counter with relaxed atomics: correct on gfx950, where agent-scope read-modify-writes execute at the memory side, but
// not by the memory model; a release fence per workgroup writes the XCD's whole L2 back and slowed a concurrent store stream 4x.)
template <bool SQUARE>
__global__ void __launch_bounds__(256) k_penalty_finish(double *__restrict__ acc, int F, double divisor, float weight, float *__restrict__ per,
                                                        float *__restrict__ out) {
    __shared__ double s_tot[256];
    double tot = 0.0;
    for (int i = threadIdx.x; i < F; i += blockDim.x) {
        const double p = divisor > 0.0 ? acc[i] / divisor : 0.0;
        per[i] = (float)p;
        tot += SQUARE ? p * p : p;
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

}  // namespace

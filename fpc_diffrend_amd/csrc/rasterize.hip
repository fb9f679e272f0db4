// rasterize forward / backward for gfx950 (MI355X).
//
// Performs the work of `dr.rasterize(glctx, pos_clip, pos_idx, resolution)` at reference
// src/torch/fit.py:151, which the reference delegates to nvdiffrast + the OpenGL hardware
// rasteriser (context at fit.py:484).  MI355X exposes no graphics pipeline, so this is a complete
// software pipeline designed for CDNA4:
//
//   k_setup   (bin_raster.h) one thread per (image, triangle): clip -> 24.8 fixed point (double arithmetic, rules R1-R3 of DESIGN.md) and
//             the float32 depth plane of R6; writes a 40-byte record + an 8-byte pixel bounding box, the 256-triangle chunk box, folds
//             the image-wide bounding box and, for the one-pass objective, appends the triangle to the lists of the bins it touches.
//   k_bins    one 256-thread workgroup per 32x32-pixel bin.  The raster phase (bin_raster.h: bin_raster) collects the triangles whose
//             boxes touch the bin -- from the bin's list, or by scanning chunk boxes and then the 8-byte boxes of the live chunks --
//             and resolves them into a depth buffer in LDS, one 64-bit (depth, triangle) key per pixel: a small triangle is walked
//             over its box by ONE LANE (exact integer edge functions, float32 depth plane, ds_min_u64 on a hit), the few large ones go
//             through a tile path (edge equations in LDS, one 16x16 tile per wave, four pixels per lane, winners in registers, folded
//             into the same buffer).  No global atomics, no depth buffer in HBM, and the result -- the minimum over (depth, index)
//             -- does not depend on scheduling.  Two read-outs follow it here: the operator's (k_bins: perspective-correct
//             barycentrics and their screen-space derivatives in f32, rast / rast_db written exactly once in 512-byte row segments;
//             an untouched bin streams zeros) and the one-pass objective's (k_bins_list / k_bins_queue: a 4 KB plane of ids + silhouette bits).
//   k_grad    one workgroup per bin, four pixels per thread: recomputes the shading terms, chains (dL/du, dL/dv, dL/d db) to the
//             three clip-space vertices, sums runs of equal triangle with one segmented scan per wave pass and adds them into an LDS
//             vertex table that is flushed once.
//
// Top to bottom: set-up, bin lists and raster core (bin_raster.h), the two read-outs, k_grad, the entry points.
//
// Arithmetic that decides integer outputs uses only + - * / floor on IEEE doubles, exact integers and
// explicit fmaf, and is compiled with -ffp-contract=off, so it agrees bit for bit with oracle/raster_ref.c.
#include "common.h"

#include <stdlib.h>
#include <algorithm>

namespace {

#include "texsample.h"
#include "raster_math.h"
#include "sil_bits.h"

#include "bin_raster.h"

// first kernel of the one-pass objective: image boxes + zeroed live map, raw occupancy map, queue headers and per-bin triangle counts
// (grid-stride), plus the caller's output buffers (zero_outputs): the gradient tables are 70 MB at 288 x 15 k vertices, so 16-byte
// stores and a grid that fills the chip
__global__ void __launch_bounds__(256) k_init_objective(ImgBox *ibox, int B, uint32_t *__restrict__ live_words, long long n_live_words,
                                                        uint32_t *__restrict__ occ_words, long long n_occ_words, int32_t *__restrict__ hdr,
                                                        int32_t *__restrict__ hdr_bwd, int32_t *__restrict__ bin_cnt, long long n_bins,
                                                        FpcdrZeroList zl) {
    const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    if (i0 < B) ibox[i0] = {0x7fffffff, 0x7fffffff, -1, -1, 0, 0, 0, 0};
    if (i0 < 16) { hdr[i0] = 0; hdr_bwd[i0] = 0; }
    for (long long i = i0; i < n_live_words; i += stride) live_words[i] = 0u;
    for (long long i = i0; i < n_occ_words; i += stride) occ_words[i] = 0u;
    if (bin_cnt)
        for (long long i = i0; i < n_bins; i += stride) bin_cnt[i] = 0;
    for (int r = 0; r < zl.count; ++r) {
        uint32_t *p = zl.p[r];
        const long long n = zl.n[r];
        long long done = 0;
        if (((size_t)p & 15) == 0) {
            uint4 *q = reinterpret_cast<uint4 *>(p);
            const long long n4 = n >> 2;
            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
            long long i = i0;
            for (; i + 3 * stride < n4; i += 4 * stride) { q[i] = z; q[i + stride] = z; q[i + 2 * stride] = z; q[i + 3 * stride] = z; }
            for (; i < n4; i += stride) q[i] = z;
            done = n4 << 2;
        }
        for (long long i = done + i0; i < n; i += stride) p[i] = 0u;
    }
}

// ---------------------------------------------------------------------------------------------
// Operator read-out (fpcdr_rasterize_fwd), grid form: one workgroup per bin, grid (OX, OY, B).  Every pixel of the bin is written exactly
// once.  op_hint: out, plane 0 of the region hint, or null.
template <bool WRITE_DB>
__global__ void __launch_bounds__(256) FPCDR_BINS_WPE k_bins(const float4 *__restrict__ pos, const int32_t *__restrict__ tri,
                                              int V, int T, int H, int W, const TriRec *__restrict__ recs,
                                              const TriBox *__restrict__ boxes, const TriBox *__restrict__ cboxes,
                                              const ImgBox *__restrict__ ibox, float4 *__restrict__ rast,
                                              float4 *__restrict__ rast_db, uint8_t *__restrict__ op_hint) {
    __shared__ BinLds lds;
    __shared__ float s_fy[BIN];      // NDC y of the bin's 32 rows: one IEEE division per row instead of one per pixel
    const int b = blockIdx.z, bxi = blockIdx.x, byi = blockIdx.y;
    const int bin_x0 = bxi * BIN, bin_y0 = byi * BIN;
    const int tid = threadIdx.x;
    const int total_hits = bin_raster<false>(lds, b, bxi, byi, gridDim.x, gridDim.y, T, H, W, recs, boxes, cboxes, ibox).hits;
    if (op_hint && tid == 0) op_hint[((size_t)b * gridDim.y + byi) * gridDim.x + bxi] = total_hits > 0 ? 1 : 0;
    if (total_hits == 0) {
        // ---- nothing touches this bin (most bins of a dense call): stream the empty result, two full 512-byte rows of
        // rast per wave instruction instead of the shading loop's 8x8 quadrant pattern ----
        for (int i = tid; i < BIN * BIN; i += 256) {
            const int px = bin_x0 + (i % BIN), py = bin_y0 + (i / BIN);
            if (px >= W || py >= H) continue;
            const size_t off = ((size_t)b * H + py) * W + px;
            rast[off] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (WRITE_DB) rast_db[off] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    // From here on a thread owns the four pixels (tid & 31, (tid >> 5) + 8 k) of the bin: the 32 lanes of a half wave write
    // one 512-byte row segment of rast per instruction (the raster's 8 x 8 quadrant pattern gave 128-byte pieces).
    if (tid < BIN) s_fy[tid] = (2.0f * (float)(bin_y0 + tid) + 1.0f) / (float)H - 1.0f;
    __syncthreads();      // (the raster phase's folded winners, and s_fy)
    int win[4];
    const int zx = tid & 31, zy0 = tid >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long z = lds.s_z[(zy0 + 8 * k) * BIN + zx];
        win[k] = z == Z_EMPTY ? -1 : (int)(unsigned int)z;
    }
    const float sx = 2.0f / (float)W, sy = 2.0f / (float)H;
    const float4 *p = pos + (size_t)b * V;
    const int px = bin_x0 + zx;
    // Every gather below goes through a 32-bit byte offset from a wave-uniform base (common.h ld32 / at32): per-image vertex and index
    // arrays, and the bin's own pixels at bin_off + zy * W + zx.
    struct I3 { int a, b, c; };
    const size_t bin_off = ((size_t)b * H + bin_y0) * W + bin_x0;
    float4 *const rast_bin = rast + bin_off;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int zy = zy0 + 8 * k, py = bin_y0 + zy;
        if (px >= W || py >= H) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f), d = make_float4(0.f, 0.f, 0.f, 0.f);
        const int t = win[k];
        if (t >= 0) {
            const I3 ti = ld32(reinterpret_cast<const I3 *>(tri), t);
            const float fx = (2.0f * (float)px + 1.0f) / (float)W - 1.0f;
            const float fy = s_fy[zy];
            Shade sd = shade_pixel(ld32(p, ti.a), ld32(p, ti.b), ld32(p, ti.c), fx, fy, sx, sy);
            o = make_float4(sd.u, sd.v, sd.zw, (float)(t + 1));
            d = make_float4(sd.dudx, sd.dudy, sd.dvdx, sd.dvdy);
        }
        const unsigned int poff = (unsigned int)(zy * W + zx);      // pixel offset inside the bin's window of the image
        at32(rast_bin, poff) = o;
        if (WRITE_DB) rast_db[bin_off + poff] = d;
    }
}

// ---------------------------------------------------------------------------------------------
// IDS read-out (one-pass objective, objective.hip): raster only -- the bin's winners leave as a 4 KB plane of ids and nothing else is written.
struct IdsArgs {
    uint8_t *occ;            // out [B, OY, OX], 1 = some triangle's bounding box touches the bin.  Bins with 0 are NOT written; the shading
                             // kernels treat their pixels as empty (k_list_count<2> turns this byte map into the window masks they read)
    const uint8_t *sil;      // [B,T] silhouette bits (k_sil2, or k_setup's SIL form)
    uint32_t *idp;           // out, per-bin planes of (triangle + 1) | silhouette bits << 24, [bin][32][32]
    const int32_t *bin_cnt, *bin_list;      // per-bin triangle lists of k_setup<true> (or null: every bin scans the chunk boxes)
};
__device__ __forceinline__ void bin_ids(BinLds &lds, const int b, const int bxi, const int byi, const int OX, const int OY, int T, int H, int W,
                                        const TriRec *__restrict__ recs, const TriBox *__restrict__ boxes, const TriBox *__restrict__ cboxes,
                                        const ImgBox *__restrict__ ibox, const IdsArgs &a) {
    const int bin_x0 = bxi * BIN, bin_y0 = byi * BIN;
    const int tid = threadIdx.x;
    const size_t bin_lin = ((size_t)b * OY + byi) * OX + bxi;
    const int total_hits = bin_raster<true>(lds, b, bxi, byi, OX, OY, T, H, W, recs, boxes, cboxes, ibox, a.bin_cnt, a.bin_list, a.sil).hits;
    if (tid == 0) a.occ[bin_lin] = total_hits > 0 ? 1 : 0;
    if (total_hits == 0) return;      // nothing of this image in the bin: no plane is written, the consumers skip it too
    __syncthreads();      // (the raster phase's folded winners)
    // the plane of this bin's winners, 16 bytes per thread (four adjacent pixels of row tid >> 3); the silhouette bits of a pixel's
    // triangle ride above its id, so that the shading kernel classifies pixel pairs from ids alone
    const int r = tid >> 3, c4 = (tid & 7) * 4;
    unsigned int e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned long long z = lds.s_z[r * BIN + c4 + j];
        // (the tile path resolves whole 16 x 16 tiles: a winner beyond the image's right / top border is not a pixel)
        const unsigned int key = (unsigned int)z;      // (triangle << 3) | silhouette bits
        const bool none = z == Z_EMPTY || bin_x0 + c4 + j >= W || bin_y0 + r >= H;
        e[j] = none ? 0u : (((key & 7u) << 24) | ((key >> 3) + 1u));
    }
    reinterpret_cast<uint4 *>(a.idp + bin_lin * (BIN * BIN))[tid] = make_uint4(e[0], e[1], e[2], e[3]);
}

// list form: one workgroup per entry of the list of live bins (the bins some chunk box touches, ~20 % of a face-rig frame).
// Dispatching one workgroup per bin of the whole batch costs 0.21 ms for 588 k workgroups that mostly leave at once; the caller
// sizes this launch from the count of an EARLIER call (`cap`), and whatever lies beyond it is swept up by the strided form
// below, so the result never depends on the hint.
// (Both spell the walk out instead of calling fpcdr_list_entry / fpcdr_list_sweep of common.h: through the helper the compiler schedules
//  k_bins_list's inner loop, tuned instruction by instruction, differently.)
__global__ void __launch_bounds__(256) FPCDR_BINS_WPE k_bins_list(const int32_t *__restrict__ list, const int32_t *__restrict__ count,
                                              int cap, int OX, int OY, fpcdr_bin_decode dc, int T, int H, int W,
                                              const TriRec *__restrict__ recs, const TriBox *__restrict__ boxes,
                                              const TriBox *__restrict__ cboxes, const ImgBox *__restrict__ ibox, IdsArgs a) {
    __shared__ BinLds lds;
    const int item = fpcdr_list_item(*count, cap);      // (XCD x takes the x-th eighth of the entries: common.h)
    if (item < 0) return;
    const int lin = __builtin_amdgcn_readfirstlane(list[item]);
    int b, byi, bxi;
    fpcdr_decode_bin(lin, dc, b, byi, bxi);
    bin_ids(lds, b, bxi, byi, OX, OY, T, H, W, recs, boxes, cboxes, ibox, a);
}

// strided form: entries first, first + gridDim.x, ... of the list.  The loop variable is scalar by construction, so the loop
// and the body's barriers stay uniform for the compiler.  (A dynamic pop -- thread 0's atomic handed round through LDS
// between two barriers -- made LLVM's structurizer wrap the barrier pair in a second loop level, and waves repeated
// barriers out of step; and the body inlined into a loop runs ~25 % slower than stand-alone, which is why this form only
// sweeps up what the hinted launch above did not reach.)
__global__ void __launch_bounds__(256) k_bins_queue(const int32_t *__restrict__ list, const int32_t *__restrict__ count,
                                              int first, int OX, int OY, fpcdr_bin_decode dc, int T, int H, int W,
                                              const TriRec *__restrict__ recs, const TriBox *__restrict__ boxes,
                                              const TriBox *__restrict__ cboxes, const ImgBox *__restrict__ ibox, IdsArgs a) {
    __shared__ BinLds lds;
    const int n = *count;
    for (int item = first + blockIdx.x; item < n; item += gridDim.x) {
        const int lin = __builtin_amdgcn_readfirstlane(list[item]);
        int b, byi, bxi;
        fpcdr_decode_bin(lin, dc, b, byi, bxi);
        bin_ids(lds, b, bxi, byi, OX, OY, T, H, W, recs, boxes, cboxes, ibox, a);
        __syncthreads();     // the next bin's first LDS writes must not overtake this bin's last LDS reads
    }
}

// region hint, plane 1: plane 0 OR-ed over the 3 x 3 neighbourhood
__global__ void __launch_bounds__(256) k_hint_dilate(const uint8_t *__restrict__ raw, int B, int OY, int OX, uint8_t *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * OY * OX) return;
    const int x = (int)(i % OX), y = (int)((i / OX) % OY);
    const uint8_t *img = raw + (i - (long long)y * OX - x);
    uint8_t m = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int cx = x + dx, cy = y + dy;
            if (cx >= 0 && cx < OX && cy >= 0 && cy < OY) m |= img[cy * OX + cx];
        }
    out[i] = m ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
template <bool HAS_DDB>
__global__ void __launch_bounds__(256) k_grad(const float4 *__restrict__ pos, const int32_t *__restrict__ tri,
                                              const float4 *__restrict__ rast, const float4 *__restrict__ dy,
                                              const float4 *__restrict__ ddb, int B, int V, int T, int H, int W,
                                              float *__restrict__ grad_pos, const uint8_t *__restrict__ hint) {
    // One workgroup per 32 x 32-pixel bin, four pixels per thread.  A wave pass covers two adjacent 32-pixel rows, the second
    // one right to left, so that the pixels of one triangle sit next to each other in lane order: ONE segmented scan sums the
    // nine gradient components of every run of equal triangle (common.h wave_segment_reduce9), the run tails add into the
    // workgroup's LDS vertex table, which is flushed once.  (The per-vertex loop with shuffle butterflies this replaces made
    // the kernel LDS-bound at 3.9 ms for cfg3; nine global atomics per run tail instead of the table: 7.4 ms.)
    if (hint && !fpcdr_hint_on(hint, 0, B, H, W, blockIdx.z, blockIdx.y * 32, blockIdx.x * 32)) return;   // empty bin: nothing to read
    __shared__ int s_vkey[FPCDR_VT_SLOTS];
        __shared__ double s_vacc[FPCDR_VT_SLOTS][3];
    const VTable vt = {s_vkey, s_vacc};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = (lane & 32) ? 63 - lane : lane;
    const int px = blockIdx.x * 32 + col;
    const int b = blockIdx.z;
    // pass 1: which of this thread's four pixels carry a gradient (most bins of an image: none at all)
    float4 rr[4], gg[4], gdd[4];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = blockIdx.y * 32 + wave * 8 + 2 * k + (lane >> 5);
        rr[k] = make_float4(0.f, 0.f, 0.f, 0.f); gg[k] = rr[k]; gdd[k] = rr[k];
        if (px < W && py < H) {
            const size_t off = ((size_t)b * H + py) * W + px;
            rr[k] = rast[off];
            const int t = (int)rr[k].w - 1;
            if (t >= 0 && t < T) {
                gg[k] = dy[off];
                if (HAS_DDB) gdd[k] = ddb[off];
                any |= gg[k].x != 0.f || gg[k].y != 0.f || gdd[k].x != 0.f || gdd[k].y != 0.f || gdd[k].z != 0.f || gdd[k].w != 0.f;
            } else {
                rr[k].w = 0.f;
            }
        }
    }
    if (!__builtin_amdgcn_readfirstlane(__syncthreads_or(any ? 1 : 0))) return;
    vtable_init(vt, tid, 256);
    __syncthreads();
    float *gp = grad_pos + (size_t)b * V * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = blockIdx.y * 32 + wave * 8 + 2 * k + (lane >> 5);
        int tkey = -1;
        int vk[3] = {0, 0, 0};
        float gv9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const float4 g = gg[k], gd = gdd[k];
        if (rr[k].w > 0.f && (g.x != 0.f || g.y != 0.f || gd.x != 0.f || gd.y != 0.f || gd.z != 0.f || gd.w != 0.f)) {
            const int t = (int)rr[k].w - 1;
            vk[0] = tri[3 * t]; vk[1] = tri[3 * t + 1]; vk[2] = tri[3 * t + 2];
            const float4 *p = pos + (size_t)b * V;
            const float fx = (2.0f * (float)px + 1.0f) / (float)W - 1.0f;
            const float fy = (2.0f * (float)py + 1.0f) / (float)H - 1.0f;
            float g0[3], g1[3], g2[3];
            shade_pixel_bwd<HAS_DDB>(p[vk[0]], p[vk[1]], p[vk[2]], fx, fy, 2.0f / (float)W, 2.0f / (float)H, g, gd, g0, g1, g2);
            gv9[0] = g0[0]; gv9[1] = g0[1]; gv9[2] = g0[2];
            gv9[3] = g1[0]; gv9[4] = g1[1]; gv9[5] = g1[2];
            gv9[6] = g2[0]; gv9[7] = g2[1]; gv9[8] = g2[2];
            tkey = t;
        }
        wave_segment_reduce9(tkey, gv9, [&](int, const float (&sm)[9]) { vtable_add(vt, gp, vk, sm); });
    }
    __syncthreads();
    vtable_flush(vt, gp, tid, 256);
}


}  // namespace

extern "C" size_t fpcdr_rasterize_scratch_bytes(int32_t B, int32_t T) {
    if (B <= 0 || T <= 0) return 0;
    return raster_scratch(nullptr, B, T).bytes;
}

extern "C" int fpcdr_rasterize_fwd(const fpcdr_rasterize_fwd_params *p, void *stream) {
    FPCDR_REQUIRE(p != nullptr, "null params");
    FPCDR_REQUIRE(p->pos && p->tri && p->scratch && p->rast, "null pointer");
    FPCDR_REQUIRE(p->B > 0 && p->V > 0 && p->T > 0 && p->H > 0 && p->W > 0, "sizes must be positive");
    FPCDR_REQUIRE(p->H <= 32767 && p->W <= 32767, "resolution above 32767 is not supported");
    FPCDR_REQUIRE(p->B <= 65535, "more than 65535 images per call");
    FPCDR_REQUIRE(p->T < (1 << 24), "more than 2^24 triangles (rast stores triangle index + 1 as a float)");
    hipStream_t st = (hipStream_t)stream;
    const RasterScratch rs = raster_scratch(p->scratch, p->B, p->T);
    hipLaunchKernelGGL(k_init_ibox, dim3(fpcdr_cdiv(p->B, 256)), dim3(256), 0, st, rs.ibox, p->B);
    dim3 grid(fpcdr_cdiv(p->W, BIN), fpcdr_cdiv(p->H, BIN), p->B);
    const size_t nbins = (size_t)p->B * grid.y * grid.x;
    // (Tried: the empty result of the bins no chunk box touches streamed by a row-wise fill kernel, k_bins on the rest -- 1.5 ms of
    // fill + 1.3 ms for the occupied fifth of the bins, one after the other, against 2.33 ms here: in ONE kernel the memory-bound
    // empty bins overlap the compute-bound occupied ones.  r3: a stride permutation of each image's bins in dispatch order, so that
    // occupied and empty bins are in flight together at every moment, changes nothing -- 2.25 ms for strides 0 / n/55 / n/7 / n/1.6:
    // the long-lived occupied workgroups pile up on the CUs by themselves and the fill shares their 7 slots per CU.)
    launch_setup(st, p->pos, p->tri, p->B, p->V, p->T, p->H, p->W, rs, nullptr, p->ranges);
    if (p->rast_db)
        hipLaunchKernelGGL(k_bins<true>, grid, dim3(256), 0, st, (const float4 *)p->pos, p->tri, p->V, p->T, p->H, p->W,
                           rs.recs, rs.boxes, rs.cboxes, rs.ibox, (float4 *)p->rast, (float4 *)p->rast_db, p->hint);
    else
        hipLaunchKernelGGL(k_bins<false>, grid, dim3(256), 0, st, (const float4 *)p->pos, p->tri, p->V, p->T, p->H, p->W,
                           rs.recs, rs.boxes, rs.cboxes, rs.ibox, (float4 *)p->rast, (float4 *)nullptr, p->hint);
    if (p->hint)
        hipLaunchKernelGGL(k_hint_dilate, dim3(fpcdr_cdiv((long long)nbins, 256)), dim3(256), 0, st, p->hint, p->B, (int)grid.y, (int)grid.x,
                           p->hint + nbins);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

extern "C" int fpcdr_rasterize_bwd(const fpcdr_rasterize_bwd_params *p, void *stream) {
    FPCDR_REQUIRE(p != nullptr, "null params");
    FPCDR_REQUIRE(p->pos && p->tri && p->rast && p->dy && p->grad_pos, "null pointer");
    FPCDR_REQUIRE(p->B > 0 && p->V > 0 && p->T > 0 && p->H > 0 && p->W > 0, "sizes must be positive");
    FPCDR_REQUIRE(p->B <= 65535, "more than 65535 images per call");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(fpcdr_cdiv(p->W, 32), fpcdr_cdiv(p->H, 32), p->B);
    if (p->ddb)
        hipLaunchKernelGGL(k_grad<true>, grid, dim3(256), 0, st, (const float4 *)p->pos, p->tri, (const float4 *)p->rast,
                           (const float4 *)p->dy, (const float4 *)p->ddb, p->B, p->V, p->T, p->H, p->W, p->grad_pos, p->hint);
    else
        hipLaunchKernelGGL(k_grad<false>, grid, dim3(256), 0, st, (const float4 *)p->pos, p->tri, (const float4 *)p->rast,
                           (const float4 *)p->dy, (const float4 *)nullptr, p->B, p->V, p->T, p->H, p->W, p->grad_pos, p->hint);
    FPCDR_CHECK_LAUNCH();
    return FPCDR_OK;
}

// First half of fpcdr_objective_fwd (objective.hip; not part of the C ABI): set-up, the list of live bins, the rasteriser in its IDS form
// (id planes only) and the ordered list of OCCUPIED bins + window masks for the shading kernels.  The caller has run k_sil2.
int fpcdr_launch_raster_ids(const fpcdr_objective_params *p, hipStream_t st, const int32_t **occ_list, const int32_t **n_occ_dev,
                            const FpcdrZeroList &zl_in, bool sil_in_setup) {
    const RasterScratch rs = raster_scratch(p->scratch, p->B, p->T);
    const int OX = fpcdr_cdiv(p->W, BIN), OY = fpcdr_cdiv(p->H, BIN);
    const size_t nbins = (size_t)p->B * OY * OX;
    FPCDR_REQUIRE(nbins < 0x7ffffff0ULL, "too many bins for one call");
    const fpcdr_queue_layout q = fpcdr_queue_layout_of(p->B, p->H, p->W, true);
    char *cm = (char *)p->cmask, *oc = (char *)p->occ;
    int32_t *hdr = (int32_t *)(cm + q.cm_hdr), *bin_list = (int32_t *)(cm + q.cm_bin_list), *olist = (int32_t *)(cm + q.cm_fix_list);
    uint8_t *live = (uint8_t *)(cm + q.cm_live);
    int32_t *hdr_occ = (int32_t *)(oc + q.occ_hdr);
    uint8_t *occ_raw = (uint8_t *)(oc + q.occ_raw);
    // per-bin triangle lists (p->binlist: counts, then BL_CAP slots per bin), or the chunk scan for every bin when the caller gave none
    int32_t *bin_cnt = (int32_t *)p->binlist, *tri_lists = bin_cnt ? bin_cnt + align_up(nbins, 64) : nullptr;
    // list building: two launches per round (k_list_count, k_list_write_sum) up to LW_MAX_BLOCKS workgroups, three beyond
    const int nblk = fpcdr_cdiv((long long)nbins, 256);
    const bool two_launch_lists = nblk <= LW_MAX_BLOCKS;
    int32_t *blk = (int32_t *)(cm + q.cm_blk);
    // the largest buffer of the list, if it is 16-byte aligned, is left to the set-up kernel (see k_setup)
    FpcdrZeroList zl = zl_in;
    uint4 *big16 = nullptr;
    long long big_n16 = 0;
    {
        int big = -1;
        for (int r = 0; r < zl.count; ++r)
            if (zl.n[r] >= (1ll << 20) && ((size_t)zl.p[r] & 15) == 0 && (zl.n[r] & 3) == 0 && (big < 0 || zl.n[r] > zl.n[big])) big = r;
        if (big >= 0) {
            big16 = reinterpret_cast<uint4 *>(zl.p[big]);
            big_n16 = zl.n[big] >> 2;
            zl.p[big] = zl.p[zl.count - 1]; zl.n[big] = zl.n[zl.count - 1]; --zl.count;
        }
    }
    long long zero_words = 0;
    for (int r = 0; r < zl.count; ++r) zero_words += zl.n[r];
    const int init_grid = (int)std::min<long long>(2048, std::max<long long>(256, zero_words / 4096));
    hipLaunchKernelGGL(k_init_objective, dim3(init_grid), dim3(256), 0, st, rs.ibox, p->B, (uint32_t *)live, (long long)(align_up(nbins, 4) / 4),
                       (uint32_t *)oc, (long long)(q.occ_hdr / 4), hdr, hdr_occ, bin_cnt, (long long)nbins, zl);
    // (sil_in_setup: the caller has not computed the silhouette bits -- the set-up kernel does, one walk of the index -> position chain)
#define SETUP(BL, SL)                                                                                                              \
    hipLaunchKernelGGL((k_setup<BL, SL>), dim3(fpcdr_cdiv(p->T, 256), p->B), dim3(256), 0, st, (const float4 *)p->pos, p->tri,     \
                       p->B, p->V, p->T, p->H, p->W, rs.recs, rs.boxes, rs.cboxes, rs.ibox, live, (const int32_t *)nullptr, bin_cnt, tri_lists, \
                       p->adj, p->sil, rs.clip, big16, big_n16)
    if (bin_cnt) { if (sil_in_setup) SETUP(true, true); else SETUP(true, false); }
    else { if (sil_in_setup) SETUP(false, true); else SETUP(false, false); }
#undef SETUP
    // (the triangles with a vertex at w <= 0, normally none: one workgroup per image looks at its list's count and leaves)
    if (bin_cnt)
        hipLaunchKernelGGL(k_setup_clip<true>, dim3(p->B), dim3(256), 0, st, (const float4 *)p->pos, p->tri, p->V, p->T, p->H, p->W, rs.recs, rs.boxes,
                           rs.cboxes, rs.ibox, live, bin_cnt, tri_lists, rs.clip);
    else
        hipLaunchKernelGGL(k_setup_clip<false>, dim3(p->B), dim3(256), 0, st, (const float4 *)p->pos, p->tri, p->V, p->T, p->H, p->W, rs.recs, rs.boxes,
                           rs.cboxes, rs.ibox, live, (int32_t *)nullptr, (int32_t *)nullptr, rs.clip);
    int32_t *n_bins = hdr_occ + 2, *n_occ = hdr_occ + 3;      // (include/fpcdr.h FPCDR_OCC_COUNTS_OFFSET)
    launch_list_round<0>(st, two_launch_lists, live, nbins, OY, OX, blk, bin_list, nullptr, n_bins, nullptr, nullptr, p->tex, p->Ht, p->Wt, p->C,
                         p->boundary_mode, p->empty_color);
    const IdsArgs ia = {occ_raw, p->sil, p->idp, bin_cnt, tri_lists};
    const fpcdr_bin_decode dc = fpcdr_make_bin_decode(OX, OY);
    const int cap_bins = (p->cap_bins > 0 && (size_t)p->cap_bins < nbins) ? p->cap_bins : (int)nbins;
    // the silhouette bits computed by the caller on another stream (sil_ready): the rasteriser kernel is their first reader
    if (p->sil_ready && p->sil_event)
        FPCDR_REQUIRE(hipStreamWaitEvent(st, (hipEvent_t)p->sil_event, 0) == hipSuccess, "hipStreamWaitEvent(sil_event) failed");
    hipLaunchKernelGGL(k_bins_list, dim3(fpcdr_list_grid(cap_bins)), dim3(256), 0, st, bin_list, n_bins, cap_bins, OX, OY, dc, p->T, p->H, p->W,
                       rs.recs, rs.boxes, rs.cboxes, rs.ibox, ia);
    if ((size_t)cap_bins < nbins)
        hipLaunchKernelGGL(k_bins_queue, dim3(FPCDR_SWEEP_WGS), dim3(256), 0, st, bin_list, n_bins, cap_bins, OX, OY, dc, p->T, p->H, p->W,
                           rs.recs, rs.boxes, rs.cboxes, rs.ibox, ia);
    launch_list_round<2>(st, two_launch_lists, occ_raw, nbins, OY, OX, blk, olist, nullptr, n_occ, nullptr, p->occ);
    FPCDR_CHECK_LAUNCH();
    *occ_list = olist;
    *n_occ_dev = n_occ;
    return FPCDR_OK;
}

extern "C" size_t fpcdr_binlist_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t nbins = (size_t)B * FPCDR_OCC_DIM(H) * FPCDR_OCC_DIM(W);
    return (align_up(nbins, 64) + nbins * BL_CAP) * sizeof(int32_t);
}

extern "C" size_t fpcdr_idplane_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * FPCDR_OCC_DIM(H) * FPCDR_OCC_DIM(W) * (BIN * BIN) * sizeof(uint32_t);
}

extern "C" size_t fpcdr_occ_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return fpcdr_queue_layout_of(B, H, W).occ_bytes;
}

extern "C" size_t fpcdr_cmask_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return fpcdr_queue_layout_of(B, H, W).cm_bytes;
}

extern "C" size_t fpcdr_objective_cmask_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return fpcdr_queue_layout_of(B, H, W, true).cm_bytes;
}

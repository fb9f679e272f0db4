// The rasteriser core shared by rasterize.hip (the product: operator and id planes) and fused.hip (the two-call form): triangle set-up,
// the ordered bin lists, the raster phase of one 32x32 bin (bin_raster) and the host code that launches set-up and a list round.
// Everything behind the raster phase -- what a kernel does with the bin's resolved depth buffer -- belongs to the including file.
// Included inside the translation unit's anonymous namespace, after texsample.h and sil_bits.h; each unit instantiates what it launches.
#pragma once
#include "common.h"

constexpr int SUBPIX = 256;
constexpr int HALFPIX = 128;
constexpr double GUARD = 16777216.0;  // 2^24

#define FPCDR_BIN 32   // measured at cfg3: 64 -> 5.2 ms, 32 -> 3.6 ms (fused forward): smaller bins balance the rim better
constexpr int BIN = FPCDR_BIN;   // pixels per bin side
constexpr int TILE = 16;         // pixels per tile side; a wave covers a tile with 4 pixels per lane (2x2 quads of 8x8)
constexpr int QUAD = 8;
constexpr int TILES_X = BIN / TILE;
constexpr int NTILES = TILES_X * TILES_X;   // 4 tiles per bin
constexpr int BATCH = 256;       // triangles expanded in LDS at a time (= block size)
constexpr int TILES_PER_WAVE = NTILES / 4;  // 1 (x 4 pixels per lane)
static_assert(TILES_PER_WAVE >= 1, "a bin needs at least one tile per wave");

struct __attribute__((aligned(8))) TriRec {  // 40 bytes
    int32_t X0, Y0, X1, Y1, X2, Y2;   // snapped vertices (R2)
    float zA, zB, z0;                 // depth plane anchored at vertex 0 (R6)
    int32_t tid;                      // the triangle this record is (a piece of): its slot, except for the second piece of a clipped one
};
struct __attribute__((aligned(8))) TriBox {  // inclusive pixel bbox; x0 > x1 = dropped
    int16_t x0, y0, x1, y1;
};
struct ImgBox { int32_t x0, y0, x1, y1, n_over, n_clip, pad1, pad2; };  // box folded with atomicMin/atomicMax; n_over: overflow records (below); n_clip: entries of the image's clip list

// Per-image record slots.  A triangle that crosses the near plane is clipped into one or two pieces (rule R1): the first takes the
// triangle's own slot t, the second is appended to the image's OVERFLOW region -- slots [Tp, Tp + n_over), Tp = T rounded up to whole
// 256-slot chunks -- with an atomic counter.  The region has room for every triangle (it is only ever touched where clipping
// happens: none of it in the fit loop), so the scratch buffer holds 2 Tp slots per image.  Overflow chunks carry no chunk box: a bin
// scans all of them.
__host__ __device__ inline int padded_slots(int T) { return (T + 255) / 256 * 256; }

struct __attribute__((aligned(16))) EdgeRec {  // LDS, 80 bytes
    int32_t A0, B0, A1, B1, A2, B2;
    int32_t nb;       // bit e (0..2) set: edge e does NOT own ties (E == 0 is outside); bit 3: small triangle
    int32_t id;       // triangle index
    union {
        long long C[3];                              // general path: biased constants C_e - nb_e (int64)
        struct { int32_t X1, Y1, X2, Y2, X0, Y0; } v;  // small path: anchor vertex of edge 0, 1, 2
    };
    float zA, zB, z0;   // depth plane (R6), anchored at (X0, Y0)
    int32_t X0, Y0;     // (also for the general path, whose union holds C[])
    int32_t pad[3];
};
static_assert(sizeof(EdgeRec) == 96, "EdgeRec layout");
// A triangle whose extent is at most 64 pixels in x and y takes the 32-bit path: for every pixel of a tile its
// bounding box touches, |P - anchor| <= 16384 + 2048 sub-pixel units and |A|,|B| <= 16384, so each edge
// function fits in int32 and the products fit v_mad_i32_i24.  Same integers, fewer and full-rate instructions.
constexpr int SMALL_EXTENT = 16384;
// Triangles of the 32-bit class whose bounding box covers at most LANE_MAX pixels of the bin are rasterised by ONE LANE
// each (a loop over the box, winners folded into the bin's LDS depth buffer with 64-bit atomic min); the others go
// through the tile path in rounds of BIGB.  On the 30k-triangle rig a triangle's box holds ~50 pixels, a 16x16 tile
// 256: one lane per triangle issues ~4x fewer instructions than one wave per (triangle, tile).
#define FPCDR_LANE_MAX 256
constexpr int LANE_MAX = FPCDR_LANE_MAX;
constexpr int BIGB = 64;         // triangles per round of the tile path
// (r5, measured and dropped: EARLY Z -- the lane path in two halves by the sign of the triangle's area, i.e. the layer of a closed mesh that
//  faces the camera first, the bin's depth buffer summarised as one maximum per 8 x 8 block in between, and a triangle of the second half
//  whose nearest depth lies behind every block its box touches skips its walk.  Exact (ids bit-identical at 1080p / 4K), and slower: 571 ->
//  681 us with the facing layer first, 881 with the other first -- the lanes of a wave walk in lockstep, so two half-empty passes cost two
//  walks unless a whole wave's triangles are culled; compacting the survivors first would need two more barriers and a prefix per batch.)
// latency-bound: 7 waves per SIMD (r2 sweep of the LOSS list kernel: 5 -> 2.23 ms, 6 -> 2.23, 7 -> 2.11, 8 -> 2.20; its 22 KB of LDS allow 7 workgroups per CU)
#define FPCDR_BINS_WPE __attribute__((amdgpu_waves_per_eu(7, 8)))
#define FPCDR_SCAN_K 4
constexpr int SCAN_K = FPCDR_SCAN_K;        // live chunks whose bounding boxes are tested per scan iteration

// (depth, triangle) as one ordered 64-bit key: smaller depth first, ties to the smaller triangle index (R6).
// d + 0.0f turns -0.0 into +0.0, so that the integer order of the keys is the float order of the depths.
__device__ __forceinline__ unsigned long long zpack(float d, int id) {
    unsigned int u = __float_as_uint(d + 0.0f);
    u ^= (unsigned int)((int)u >> 31) | 0x80000000u;   // sign set: ~u; sign clear: u | top bit
    return ((unsigned long long)u << 32) | (unsigned int)id;
}
constexpr unsigned long long Z_EMPTY = ~0ull;

__device__ __forceinline__ long long floordiv256(long long a) { return a >> 8; }  // arithmetic shift = floor

// ---------------------------------------------------------------------------------------------
// One piece (a triangle, or a piece of a clipped one) in double clip coordinates -> record + pixel box: rules R2, R3, R6.
__device__ __forceinline__ bool setup_piece(const double (&v)[3][4], int H, int W, int tid, TriRec &r, TriBox &box) {
    long long X[3], Y[3];
    double zw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double dw = v[i][3];
        if (!(dw > 0.0)) return false;
        const double rw = 1.0 / dw;      // (R2: one double division per vertex, not three: k_setup is bound by vector issue)
        const double xs = v[i][0] * rw;
        const double ys = v[i][1] * rw;
        const double fx = floor((xs * 0.5 + 0.5) * (double)(W * SUBPIX) + 0.5);
        const double fy = floor((ys * 0.5 + 0.5) * (double)(H * SUBPIX) + 0.5);
        if (!(fabs(fx) <= GUARD) || !(fabs(fy) <= GUARD)) return false;
        X[i] = (long long)fx;
        Y[i] = (long long)fy;
        zw[i] = v[i][2] * rw;
    }
    const long long D = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    if (D == 0) return false;
    const double Dd = (double)D;
    const long long xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
    const long long ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
    long long px0 = floordiv256(xmin - HALFPIX + SUBPIX - 1), px1 = floordiv256(xmax - HALFPIX);
    long long py0 = floordiv256(ymin - HALFPIX + SUBPIX - 1), py1 = floordiv256(ymax - HALFPIX);
    px0 = max(px0, 0ll); py0 = max(py0, 0ll);
    px1 = min(px1, (long long)W - 1); py1 = min(py1, (long long)H - 1);
    if (px0 > px1 || py0 > py1) return false;
    box = {(int16_t)px0, (int16_t)py0, (int16_t)px1, (int16_t)py1};
    r.X0 = (int32_t)X[0]; r.Y0 = (int32_t)Y[0];
    r.X1 = (int32_t)X[1]; r.Y1 = (int32_t)Y[1];
    r.X2 = (int32_t)X[2]; r.Y2 = (int32_t)Y[2];
    const double dz1 = zw[1] - zw[0], dz2 = zw[2] - zw[0];
    r.zA = (float)((dz1 * (double)(Y[2] - Y[0]) - dz2 * (double)(Y[1] - Y[0])) / Dd);
    r.zB = (float)((dz2 * (double)(X[1] - X[0]) - dz1 * (double)(X[2] - X[0])) / Dd);
    r.z0 = (float)zw[0];
    r.tid = tid;
    return true;
}

// NEAR-PLANE CLIPPING LIVES IN ITS OWN KERNEL (r5).  clip_pieces works on small double arrays indexed at run time -- 400 bytes of private
// segment per lane -- and a kernel with a private segment pays for it on every dispatch, taken or not (the fit loop's rig stays 140 units in
// front of the near plane: never).  k_setup therefore only APPENDS the index of a triangle with a vertex at w <= 0 to its image's clip list
// and leaves the slot dropped; k_setup_clip -- one small workgroup per image, normally finding an empty list -- clips those triangles,
// fills the slot with the first piece (folding its box into the chunk box the set-up kernel stored, the image box and the bin lists) and
// appends the second to the overflow slots.  The rasteriser's result does not depend on the order of records or list entries.
//
// Rule R1 for a triangle with some w <= 0: Sutherland-Hodgman against the near plane z + w >= 0, in double, every crossing computed
// from the vertex inside to the one outside (the same arithmetic, in the same order, as oracle/raster_ref.c clip_pieces).  Returns the
// number of pieces (0 = dropped) and their vertices.
__device__ __noinline__ int clip_pieces(const float4 (&v)[3], double (&pc)[2][3][4]) {
    double d[3], poly[4][4], vd[3][4];
    for (int i = 0; i < 3; ++i) {
        vd[i][0] = (double)v[i].x; vd[i][1] = (double)v[i].y; vd[i][2] = (double)v[i].z; vd[i][3] = (double)v[i].w;
        d[i] = vd[i][2] + vd[i][3];
        if (!(d[i] == d[i])) return 0;
    }
    int n = 0;
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3;
        const bool in_i = d[i] >= 0.0, in_j = d[j] >= 0.0;
        if (in_i) {
            for (int c = 0; c < 4; ++c) poly[n][c] = vd[i][c];
            ++n;
        }
        if (in_i != in_j) {
            const int a = in_i ? i : j, bb = in_i ? j : i;
            const double t = d[a] / (d[a] - d[bb]);
            for (int c = 0; c < 4; ++c) poly[n][c] = vd[a][c] + t * (vd[bb][c] - vd[a][c]);
            ++n;
        }
    }
    if (n < 3) return 0;
    for (int i = 0; i < n; ++i)
        if (!(poly[i][3] > 0.0)) return 0;
    for (int k = 0; k + 2 < n; ++k)
        for (int c = 0; c < 4; ++c) { pc[k][0][c] = poly[0][c]; pc[k][1][c] = poly[k + 1][c]; pc[k][2][c] = poly[k + 2][c]; }
    return n - 2;
}

// Per-bin triangle lists (BINLIST instantiation, the one-pass objective): the raster kernel's search for "which triangles touch my bin"
// -- chunk boxes, then the 8-byte boxes of ~2 000 triangles of the live chunks, three barriers -- was 290 us of its 700 at cfg3 for a
// quarter of its instructions: a chain of dependent loads, not work (profiles/r04_raster_ablation.txt).  Here the set-up kernel, which
// holds every triangle's box anyway, bins its 256 triangles over the <= BL_LOCAL bins of its chunk box in LDS (count, one global
// fetch-add per touched bin for the segment's place in the bin's list, fill) and the raster kernel reads its list: one count, one
// gather.  A bin's list holds BL_CAP record slots; a bin that overflows (thousands of tiny triangles in one bin) keeps its count and
// falls back to the chunk scan.  Order inside a list depends on scheduling; the winner of a pixel -- min over (depth, index) -- does not.
constexpr int BL_CAP = 256;        // entries per bin list (a bin of the 30k rig holds ~120)
constexpr int BL_LOCAL = 64;       // local bins of a chunk box binned in LDS (8 x 8); larger chunk boxes: per-triangle global appends

__device__ __forceinline__ void binlist_append_global(int32_t *__restrict__ bin_cnt, int32_t *__restrict__ bin_list, uint8_t *__restrict__ live,
                                                      size_t img_bins, int OX, TriBox bx, int slot) {
    for (int gy = bx.y0 / BIN; gy <= bx.y1 / BIN; ++gy)
        for (int gx = bx.x0 / BIN; gx <= bx.x1 / BIN; ++gx) {
            const size_t gb = img_bins + (size_t)gy * OX + gx;
            const int pos = atomicAdd(&bin_cnt[gb], 1);
            if (pos < BL_CAP) bin_list[gb * BL_CAP + pos] = slot;
            live[gb] = 1;
        }
}

// A position that has been gathered stays gathered: the empty statement makes the four components live in vector registers HERE, so the
// compiler can neither split the 16-byte load into the pieces each later use wants, nor sink it behind a branch, nor fetch it again.
__device__ __forceinline__ void pin_loaded(float4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// SIL: the thread also classifies its triangle's three edges for the antialias step (sil_bits.h) -- it holds the triangle's own three
// vertices already, the three across the edges are gathered beside them (the stand-alone kernel, k_sil2, is 62 us at 288 x 30 k of
// which this form leaves ~10: the same chain of index load -> position gather, walked once instead of twice).
template <bool BINLIST = false, bool SIL = false>
__global__ void __launch_bounds__(256) k_setup(const float4 *__restrict__ pos, const int32_t *__restrict__ tri,
                                                int B, int V, int T, int H, int W, TriRec *__restrict__ recs,
                                                TriBox *__restrict__ boxes, TriBox *__restrict__ cboxes,
                                                ImgBox *__restrict__ ibox, uint8_t *__restrict__ live,
                                                const int32_t *__restrict__ ranges, int32_t *__restrict__ bin_cnt = nullptr,
                                                int32_t *__restrict__ bin_list = nullptr, const int32_t *__restrict__ adj = nullptr,
                                                uint8_t *__restrict__ sil = nullptr, int32_t *__restrict__ clip = nullptr,
                                                uint4 *__restrict__ zero16 = nullptr, long long n_zero16 = 0) {
    // (one-pass objective: the caller's position-gradient table -- 69 MB at 288 x 15 k vertices -- is zero-filled HERE, a 16-byte store or
    //  two per thread beside the gathers this kernel waits for, instead of by the call's first kernel, where it was 12 us on its own)
    if (zero16) {
        const long long nthreads = (long long)gridDim.x * gridDim.y * blockDim.x;
        for (long long i = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; i < n_zero16; i += nthreads)
            zero16[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    // grid: x over 256-triangle chunks, y = image.  A block never straddles two images, so the union of
    // its triangles' bounding boxes can be reduced in the block: it is stored as the CHUNK box (meshes
    // keep neighbouring triangles at neighbouring indices, so a bin later skips most chunks with one
    // test) and folded into the image box with at most four atomics per block.
    __shared__ int s_box[4][4];
    const int b = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int Tp = padded_slots(T);
    const size_t img_slot = (size_t)b * 2 * Tp;
    const int OX = (W + BIN - 1) / BIN, OY = (H + BIN - 1) / BIN;
    int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = -1, by1 = -1;
    if (t < T) {
        const size_t gid = img_slot + t;
        TriBox box = {1, 1, 0, 0};
        // TWO ROUND TRIPS, NOT EIGHT (profiles/setup_load_chain.txt).  The kernel is a chain of dependent loads -- half its issue slots
        // idle at full occupancy -- and the compiler, left alone, lengthens the chain: it fetched the adjacency triple only after the
        // vertex triple had passed its test, x / y / w of the six vertices for the silhouette bits, w of the own three again for the
        // w > 0 test, and sank each vertex's x, y, z into the iteration of setup_piece that uses it.  So: (1) both index triples at once
        // -- t < T is all they need; (2) the six positions (three without SIL), each ONE 16-byte load, all in flight before the first
        // use and pinned below so that none is split, sunk or fetched again.  A hoisted load runs for triangles the tests below reject:
        // an index that is invalid or unused reads vertex 0, as in sil_classify -- no load ever leaves the table.
        const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        int ad[3] = {-1, -1, -1};
        if (SIL) { ad[0] = adj[3 * t]; ad[1] = adj[3 * t + 1]; ad[2] = adj[3 * t + 2]; }
        // (index validity only decides the silhouette bits, as in sil_classify: `ok` may also carry the range test)
        const bool vok = !(i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V);
        bool ok = vok;
        if (ranges) {      // range mode: the image renders its own slice of the triangle list
            const long long first = ranges[2 * b], count = ranges[2 * b + 1];
            ok = ok && t >= first && t < first + count;
        }
        const float4 *p = pos + (size_t)b * V;
        float4 v0 = ld32(p, vok ? (unsigned int)i0 : 0u);      // (kept as scalars: an array handed to the out-of-line clipper would
        float4 v1 = ld32(p, vok ? (unsigned int)i1 : 0u);      //  live in scratch memory on the common path too)
        float4 v2 = ld32(p, vok ? (unsigned int)i2 : 0u);
        float4 o0 = v0, o1 = v0, o2 = v0;
        if (SIL) {
            o0 = ld32(p, (ad[0] >= 0 && ad[0] < V) ? (unsigned int)ad[0] : 0u);
            o1 = ld32(p, (ad[1] >= 0 && ad[1] < V) ? (unsigned int)ad[1] : 0u);
            o2 = ld32(p, (ad[2] >= 0 && ad[2] < V) ? (unsigned int)ad[2] : 0u);
        }
        pin_loaded(v0); pin_loaded(v1); pin_loaded(v2);
        if (SIL) {
            pin_loaded(o0); pin_loaded(o1); pin_loaded(o2);
            const unsigned int bits = vok ? sil_bits_of(v0, v1, v2, o0, o1, o2, ad, V, 0.5f * (float)W, 0.5f * (float)H) : 0u;
            sil[(size_t)b * T + t] = (uint8_t)bits;
        }
        if (ok) {
            TriRec r;
            if (v0.w > 0.0f && v1.w > 0.0f && v2.w > 0.0f) {      // (R1) the usual case: the triangle as it is
                const double vd[3][4] = {{(double)v0.x, (double)v0.y, (double)v0.z, (double)v0.w},
                                         {(double)v1.x, (double)v1.y, (double)v1.z, (double)v1.w},
                                         {(double)v2.x, (double)v2.y, (double)v2.z, (double)v2.w}};
                if (setup_piece(vd, H, W, t, r, box)) {
                    recs[gid] = r;
                    bx0 = box.x0; by0 = box.y0; bx1 = box.x1; by1 = box.y1;
                } else {
                    box = {1, 1, 0, 0};
                }
            } else {      // a vertex at or behind w = 0: k_setup_clip's (the slot stays dropped until then)
                clip[(size_t)b * Tp + atomicAdd(&ibox[b].n_clip, 1)] = t;
            }
        }
        boxes[gid] = box;
    }
    const TriBox mybox = {(int16_t)(bx1 >= 0 ? bx0 : 1), (int16_t)(bx1 >= 0 ? by0 : 1), (int16_t)(bx1 >= 0 ? bx1 : 0), (int16_t)(bx1 >= 0 ? by1 : 0)};
    // image bounding box: wave reduce -> block reduce -> at most four atomics per block
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        bx0 = min(bx0, __shfl_xor(bx0, o, 64)); by0 = min(by0, __shfl_xor(by0, o, 64));
        bx1 = max(bx1, __shfl_xor(bx1, o, 64)); by1 = max(by1, __shfl_xor(by1, o, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_box[wave][0] = bx0; s_box[wave][1] = by0; s_box[wave][2] = bx1; s_box[wave][3] = by1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            bx0 = min(bx0, s_box[w][0]); by0 = min(by0, s_box[w][1]);
            bx1 = max(bx1, s_box[w][2]); by1 = max(by1, s_box[w][3]);
        }
        TriBox cb = {1, 1, 0, 0};
        if (bx1 >= 0) {
            cb = {(int16_t)bx0, (int16_t)by0, (int16_t)bx1, (int16_t)by1};
            atomicMin(&ibox[b].x0, bx0); atomicMin(&ibox[b].y0, by0);
            atomicMax(&ibox[b].x1, bx1); atomicMax(&ibox[b].y1, by1);
        }
        cboxes[(size_t)b * gridDim.x + blockIdx.x] = cb;
        if (live) { s_box[0][0] = bx0; s_box[0][1] = by0; s_box[0][2] = bx1; s_box[0][3] = by1; }
    }
    if (BINLIST) {
        // ---- per-bin lists: the chunk's triangles over the bins of the chunk box ----
        __shared__ int s_cnt[BL_LOCAL], s_base[BL_LOCAL];
        __syncthreads();
        const int cx0 = s_box[0][0], cy0 = s_box[0][1], cx1 = s_box[0][2], cy1 = s_box[0][3];
        if (cx1 < 0) return;                                  // (uniform) no triangle of this chunk reaches the image
        const int gx0 = cx0 / BIN, gy0 = cy0 / BIN, nx = cx1 / BIN - gx0 + 1, ny = cy1 / BIN - gy0 + 1;
        const size_t img_bins = (size_t)b * OY * OX;
        const bool has = mybox.x0 <= mybox.x1;
        if (nx * ny > BL_LOCAL) {                             // (uniform) a huge chunk box: every triangle appends for itself
            if (has) binlist_append_global(bin_cnt, bin_list, live, img_bins, OX, mybox, t);
            return;
        }
        if ((int)threadIdx.x < BL_LOCAL) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        const int tx0 = has ? mybox.x0 / BIN - gx0 : 0, tx1 = has ? mybox.x1 / BIN - gx0 : -1;
        const int ty0 = has ? mybox.y0 / BIN - gy0 : 0, ty1 = has ? mybox.y1 / BIN - gy0 : -1;
        for (int ly = ty0; ly <= ty1; ++ly)
            for (int lxb = tx0; lxb <= tx1; ++lxb) atomicAdd(&s_cnt[ly * nx + lxb], 1);
        __syncthreads();
        if ((int)threadIdx.x < nx * ny) {
            const int lb = threadIdx.x, c = s_cnt[lb];
            if (c > 0) {
                const size_t gb = img_bins + (size_t)(gy0 + lb / nx) * OX + gx0 + lb % nx;
                s_base[lb] = atomicAdd(&bin_cnt[gb], c);      // this chunk's segment of the bin's list
                live[gb] = 1;
            }
            s_cnt[lb] = 0;                                    // (reused as the fill cursor)
        }
        __syncthreads();
        for (int ly = ty0; ly <= ty1; ++ly)
            for (int lxb = tx0; lxb <= tx1; ++lxb) {
                const int lb = ly * nx + lxb;
                const int pos = s_base[lb] + atomicAdd(&s_cnt[lb], 1);
                if (pos < BL_CAP) bin_list[(img_bins + (size_t)(gy0 + ly) * OX + gx0 + lxb) * BL_CAP + pos] = t;
            }
        return;
    }
    if (live) {
        // work-queue mode: every bin the chunk box touches becomes a work item of k_bins_queue (a superset of the bins
        // some triangle's box touches; all writers store 1)
        __syncthreads();
        const int cx0 = s_box[0][0], cy0 = s_box[0][1], cx1 = s_box[0][2], cy1 = s_box[0][3];
        if (cx1 >= 0) {
            const int gx0 = cx0 / BIN, gy0 = cy0 / BIN, nx = cx1 / BIN - gx0 + 1, ny = cy1 / BIN - gy0 + 1;
            for (int k = threadIdx.x; k < nx * ny; k += blockDim.x)
                live[((size_t)b * OY + gy0 + k / nx) * OX + gx0 + k % nx] = 1;
        }
    }
}

// The triangles k_setup put on the clip lists (see clip_pieces): grid (1, B), the workgroup strides over its image's list.
template <bool BINLIST>
__global__ void __launch_bounds__(256) k_setup_clip(const float4 *__restrict__ pos, const int32_t *__restrict__ tri, int V, int T, int H, int W,
                                                     TriRec *__restrict__ recs, TriBox *__restrict__ boxes, TriBox *__restrict__ cboxes,
                                                     ImgBox *__restrict__ ibox, uint8_t *__restrict__ live, int32_t *__restrict__ bin_cnt,
                                                     int32_t *__restrict__ bin_list, const int32_t *__restrict__ clip) {
    const int b = blockIdx.x;
    const int n = ibox[b].n_clip;
    if (n == 0) return;
    const int Tp = padded_slots(T);
    const size_t img_slot = (size_t)b * 2 * Tp;
    const int OX = (W + BIN - 1) / BIN, OY = (H + BIN - 1) / BIN;
    const size_t img_bins = (size_t)b * OY * OX;
    const float4 *p = pos + (size_t)b * V;
    auto mark = [&](const TriBox &bx, int slot) {      // image box, bin lists / live map of one piece
        atomicMin(&ibox[b].x0, (int)bx.x0); atomicMin(&ibox[b].y0, (int)bx.y0);
        atomicMax(&ibox[b].x1, (int)bx.x1); atomicMax(&ibox[b].y1, (int)bx.y1);
        if (BINLIST) binlist_append_global(bin_cnt, bin_list, live, img_bins, OX, bx, slot);
        else if (live)
            for (int gy = bx.y0 / BIN; gy <= bx.y1 / BIN; ++gy)
                for (int gx = bx.x0 / BIN; gx <= bx.x1 / BIN; ++gx) live[img_bins + (size_t)gy * OX + gx] = 1;
    };
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int t = clip[(size_t)b * Tp + k];
        const float4 vv[3] = {p[tri[3 * t]], p[tri[3 * t + 1]], p[tri[3 * t + 2]]};      // (k_setup checked the indices)
        double pc[2][3][4];
        const int np = clip_pieces(vv, pc);
        TriRec r;
        TriBox box;
        if (np >= 1 && setup_piece(pc[0], H, W, t, r, box)) {
            // first piece: the triangle's own slot; its box joins the chunk box k_setup stored (bins skip chunks by that box)
            recs[img_slot + t] = r;
            boxes[img_slot + t] = box;
            unsigned long long *cb = reinterpret_cast<unsigned long long *>(cboxes + (size_t)b * (Tp / 256) + t / 256);
            unsigned long long seen = *cb;
            for (;;) {
                TriBox o;
                __builtin_memcpy(&o, &seen, 8);
                TriBox u = box;
                if (o.x0 <= o.x1) u = {(int16_t)min(o.x0, box.x0), (int16_t)min(o.y0, box.y0), (int16_t)max(o.x1, box.x1), (int16_t)max(o.y1, box.y1)};
                unsigned long long want;
                __builtin_memcpy(&want, &u, 8);
                const unsigned long long got = atomicCAS(cb, seen, want);
                if (got == seen) break;
                seen = got;
            }
            mark(box, t);
        }
        if (np == 2 && setup_piece(pc[1], H, W, t, r, box)) {
            // second piece: appended to the image's overflow slots (no chunk box there: bins scan every overflow chunk)
            const int q = atomicAdd(&ibox[b].n_over, 1);
            recs[img_slot + Tp + q] = r;
            boxes[img_slot + Tp + q] = box;
            mark(box, Tp + q);
        }
    }
}

__global__ void k_init_ibox(ImgBox *ibox, int B) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) ibox[i] = {0x7fffffff, 0x7fffffff, -1, -1, 0, 0, 0, 0};
}

// ---- ordered compaction of per-bin flags into lists (ascending bin index: neighbouring bins, which share vertices and
// texels, stay neighbours in launch order; appending with atomics scrambles them at wave granularity and cost the
// backward pass 10 %) -- three tiny kernels: per-block counts, one-workgroup scan, ordered write ----
constexpr int NLISTS = 2;   // lists built per round (round A: live bins; round B: antialias-fix bins, backward bins)

// flags of bin i for round A (live map) / round B (window mask m of the raw occupancy map)
__device__ __forceinline__ unsigned int window_mask(const uint8_t *__restrict__ raw, long long i, int OY, int OX) {
    const int x = (int)(i % OX), y = (int)((i / OX) % OY);
    const uint8_t *img = raw + (i - (long long)y * OX - x);
    unsigned int m = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 2; ++dx) {
            const int cx = x + dx, cy = y + dy;
            if (cx >= 0 && cx < OX && cy >= 0 && cy < OY && img[cy * OX + cx]) m |= 1u << ((dy + 1) * 4 + dx + 1);
        }
    return m;
}
__device__ __forceinline__ bool wbit(unsigned int m, int dx, int dy) { return (m >> ((dy + 1) * 4 + dx + 1)) & 1u; }

// ROUND_B: 0 = round A (live map); 1 = round B of the two-pass objective; 2 = round B of the one-pass objective (objective.hip):
// list 0 = the occupied bins themselves, no second list
template <int ROUND_B>
__device__ __forceinline__ void bin_flags(const uint8_t *__restrict__ map, long long i, long long nbins, int OY, int OX, bool (&f)[NLISTS],
                                          unsigned int &m) {
    f[0] = false; f[1] = false; m = 0;
    if (i >= nbins) return;
    if (!ROUND_B) { f[0] = map[i] != 0; return; }
    m = window_mask(map, i, OY, OX);
    if (ROUND_B == 2) { f[0] = wbit(m, 0, 0); return; }
    f[0] = wbit(m, 0, 0) || wbit(m, 1, 0) || wbit(m, 0, 1);                                        // k_aa_fix
    f[1] = f[0] || wbit(m, -1, 0) || wbit(m, 0, -1);                                              // k_render_aa_bwd
}

template <int ROUND_B>
__global__ void __launch_bounds__(256) k_list_count(const uint8_t *__restrict__ map, long long nbins, int OY, int OX,
                                                    int32_t *__restrict__ blk_counts, uint16_t *__restrict__ win,
                                                    const float *__restrict__ tex, int Ht, int Wt, int C, int boundary,
                                                    float *__restrict__ empty_out) {
    __shared__ int s_c[NLISTS][4];
    if (!ROUND_B && blockIdx.x == 0 && threadIdx.x == 0) {   // the colour of an empty pixel: the texture at uv = (0,0)
        const Taps tp0 = make_taps(0.0f, 0.0f, Ht, Wt, C, boundary);
        for (int c = 0; c < 4; ++c) empty_out[c] = c < C ? bilerp(tex, tp0, c, C) : 0.0f;
    }
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool f[NLISTS];
    unsigned int m;
    bin_flags<ROUND_B>(map, i, nbins, OY, OX, f, m);
    if (ROUND_B && i < nbins) win[i] = (uint16_t)m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NLISTS; ++k) {
        const int c = __popcll(__ballot(f[k]));
        if (lane == 0) s_c[k][wave] = c;
    }
    __syncthreads();
    if (threadIdx.x < NLISTS)
        blk_counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = s_c[threadIdx.x][0] + s_c[threadIdx.x][1] + s_c[threadIdx.x][2] + s_c[threadIdx.x][3];
}

// one workgroup: exclusive scan of the per-block counts of each list, in place; totals to count[k]
__global__ void __launch_bounds__(1024) k_list_scan(int32_t *__restrict__ blk_counts, int nblk, int32_t *__restrict__ count0,
                                                    int32_t *__restrict__ count1) {
    __shared__ int s_w[16];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = 0; k < NLISTS; ++k) {
        int32_t *c = blk_counts + (size_t)k * nblk;
        if (tid == 0) s_carry = 0;
        __syncthreads();
        for (int base = 0; base < nblk; base += 1024) {
            const int i = base + tid;
            const int v = i < nblk ? c[i] : 0;
            int incl = v;      // inclusive scan inside the wave
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            if (lane == 63) s_w[wave] = incl;
            __syncthreads();
            int woff = 0;
            for (int w = 0; w < wave; ++w) woff += s_w[w];
            const int carry = s_carry;
            if (i < nblk) c[i] = carry + woff + incl - v;
            __syncthreads();
            if (tid == 1023) s_carry = carry + woff + incl;
            __syncthreads();
        }
        if (tid == 0) { int32_t *dst = k == 0 ? count0 : count1; if (dst) *dst = s_carry; }
        __syncthreads();
    }
}

template <int ROUND_B>
__global__ void __launch_bounds__(256) k_list_write(const uint8_t *__restrict__ map, long long nbins, int OY, int OX,
                                                    const int32_t *__restrict__ blk_offsets, int32_t *__restrict__ list0,
                                                    int32_t *__restrict__ list1) {
    __shared__ int s_c[NLISTS][4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool f[NLISTS];
    unsigned int m;
    bin_flags<ROUND_B>(map, i, nbins, OY, OX, f, m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long bal[NLISTS];
#pragma unroll
    for (int k = 0; k < NLISTS; ++k) {
        bal[k] = __ballot(f[k]);
        if (lane == 0) s_c[k][wave] = __popcll(bal[k]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NLISTS; ++k) {
        int32_t *list = k == 0 ? list0 : list1;
        if (!list || !f[k]) continue;
        int off = blk_offsets[(size_t)k * gridDim.x + blockIdx.x];
        for (int w = 0; w < wave; ++w) off += s_c[k][w];
        list[off + __popcll(bal[k] & ((1ull << lane) - 1ull))] = (int32_t)i;
    }
}

// ---- the same ordered compaction as TWO launches (one-pass objective: each round's three launches sit in the call's serial path):
// k_list_count as above, then a write kernel in which every workgroup sums the counts of the workgroups before it itself (2 295 counts at
// 288 x 1080p: nine loads per thread) instead of reading offsets a one-workgroup scan kernel has left.  Up to LW_MAX_BLOCKS workgroups;
// the three-launch form beyond.  (A ONE-launch form -- workgroups publish their totals with a valid bit and wait for their predecessors'
// -- was measured at 587 k bins: 21 / 33 us per round with 2 048 bins per workgroup, 40 / 41 us with 256, against 17 / 24 us for the three
// launches: the waiting costs more than the launches.)
constexpr int LW_MAX_BLOCKS = 16384;
template <int ROUND_B>
__global__ void __launch_bounds__(256) k_list_write_sum(const uint8_t *__restrict__ map, long long nbins, int OY, int OX,
                                                        const int32_t *__restrict__ blk_counts, int32_t *__restrict__ list0,
                                                        int32_t *__restrict__ list1, int32_t *__restrict__ count0, int32_t *__restrict__ count1) {
    __shared__ int s_c[NLISTS][4];
    __shared__ int s_pre[NLISTS][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nblk = gridDim.x, b = blockIdx.x;
    int pre[NLISTS] = {0, 0};
    for (int j = tid; j < b; j += 256) {
        pre[0] += blk_counts[j];
        if (list1) pre[1] += blk_counts[(size_t)nblk + j];
    }
    const long long i = (long long)b * 256 + tid;
    bool f[NLISTS];
    unsigned int m;
    bin_flags<ROUND_B>(map, i, nbins, OY, OX, f, m);
    unsigned long long bal[NLISTS];
#pragma unroll
    for (int k = 0; k < NLISTS; ++k) {
        bal[k] = __ballot(f[k]);
        int v = pre[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) { s_c[k][wave] = __popcll(bal[k]); s_pre[k][wave] = v; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NLISTS; ++k) {
        int32_t *list = k == 0 ? list0 : list1;
        if (!list) continue;
        const int base = s_pre[k][0] + s_pre[k][1] + s_pre[k][2] + s_pre[k][3];
        int off = base;
        for (int w = 0; w < wave; ++w) off += s_c[k][w];
        if (f[k]) list[off + __popcll(bal[k] & ((1ull << lane) - 1ull))] = (int32_t)i;
        if (b == nblk - 1 && tid == 0) {
            int32_t *dst = k == 0 ? count0 : count1;
            if (dst) *dst = base + s_c[k][0] + s_c[k][1] + s_c[k][2] + s_c[k][3];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Fine raster of one 16x16 tile against the triangles of the current batch whose bit is set in `mrow`.  Each lane
// owns FOUR pixels of the tile -- (lx,ly) in each 8x8 quadrant -- so one LDS fetch of a triangle feeds four
// independent coverage / depth chains (the loop is latency-bound, not ALU-bound).  (Px,Py) is the lane's sample
// point in quadrant 0; quadrant q adds (q&1, q>>1) * 8 pixels.  SMALL selects the 32-bit path (SMALL_EXTENT).
template <bool SMALL>
__device__ __forceinline__ void fine_tile(const unsigned long long *mrow, const EdgeRec *s_tri, int Px, int Py, float (&bd)[4],
                                          int (&bi)[4]) {
    constexpr int STEP = QUAD * SUBPIX;   // 2048 sub-pixel units between quadrants
    for (int wd = 0; wd < BIGB / 64; ++wd) {
        unsigned long long m = mrow[wd];
        const unsigned int mlo = __builtin_amdgcn_readfirstlane((unsigned int)m);
        const unsigned int mhi = __builtin_amdgcn_readfirstlane((unsigned int)(m >> 32));
        m = ((unsigned long long)mhi << 32) | mlo;
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const EdgeRec &e = s_tri[wd * 64 + j];
            const int nb = e.nb;
            const int id = e.id;
            const float zA = e.zA, zB = e.zB, z0 = e.z0;
            const int rx = Px - e.X0, ry = Py - e.Y0;   // offset from the depth plane's anchor (quadrant 0)
            if (SMALL) {
                // E'_e = A (Px - Xa) + B (Py - Ya) - nb_e in int32 with 24-bit multiplies; other quadrants by addition
                const int A0 = e.A0, B0 = e.B0, A1 = e.A1, B1 = e.B1, A2 = e.A2, B2 = e.B2;
                const int b0 = __mul24(A0, Px - e.v.X1) + __mul24(B0, Py - e.v.Y1) - (nb & 1);
                const int b1 = __mul24(A1, Px - e.v.X2) + __mul24(B1, Py - e.v.Y2) - ((nb >> 1) & 1);
                const int b2 = __mul24(A2, rx) + __mul24(B2, ry) - ((nb >> 2) & 1);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int E0 = b0 + ((q & 1) ? A0 * STEP : 0) + ((q >> 1) ? B0 * STEP : 0);
                    const int E1 = b1 + ((q & 1) ? A1 * STEP : 0) + ((q >> 1) ? B1 * STEP : 0);
                    const int E2 = b2 + ((q & 1) ? A2 * STEP : 0) + ((q >> 1) ? B2 * STEP : 0);
                    if ((E0 | E1 | E2) >= 0) {
                        const float d = __fmaf_rn(zA, (float)(rx + (q & 1) * STEP), __fmaf_rn(zB, (float)(ry + (q >> 1) * STEP), z0));
                        if (d >= -1.0f && d <= 1.0f && (d < bd[q] || (d == bd[q] && id < bi[q]))) { bd[q] = d; bi[q] = id; }
                    }
                }
            } else {
                const long long A0 = e.A0, B0 = e.B0, A1 = e.A1, B1 = e.B1, A2 = e.A2, B2 = e.B2;
                const long long b0 = A0 * Px + (B0 * Py + e.C[0]);
                const long long b1 = A1 * Px + (B1 * Py + e.C[1]);
                const long long b2 = A2 * Px + (B2 * Py + e.C[2]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long long E0 = b0 + ((q & 1) ? A0 * STEP : 0) + ((q >> 1) ? B0 * STEP : 0);
                    const long long E1 = b1 + ((q & 1) ? A1 * STEP : 0) + ((q >> 1) ? B1 * STEP : 0);
                    const long long E2 = b2 + ((q & 1) ? A2 * STEP : 0) + ((q >> 1) ? B2 * STEP : 0);
                    if ((E0 | E1 | E2) >= 0) {
                        const float d = __fmaf_rn(zA, (float)(rx + (q & 1) * STEP), __fmaf_rn(zB, (float)(ry + (q >> 1) * STEP), z0));
                        if (d >= -1.0f && d <= 1.0f && (d < bd[q] || (d == bd[q] && id < bi[q]))) { bd[q] = d; bi[q] = id; }
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// LDS of one bin's raster phase.  The kernel declares it __shared__ and hands it to bin_raster; afterwards s_z holds the bin's winners
// and the lists are dead (the two-call read-out stages its colour planes in s_list and s_tri).  The members stand in the order in which
// the compiler had laid them out as separate arrays -- large and aligned first, the scalars last, every array on a 16-byte boundary:
// with s_nbig between s_big and s_clist, as they were once declared, the id-plane kernel ran 2 % slower (profiles/raster_split_ab.txt).
struct BinLds {
    unsigned long long s_z[BIN * BIN];   // the bin's depth buffer: zpack(depth, triangle), Z_EMPTY = nothing yet
    EdgeRec s_tri[BIGB];     // tile path: edge equations of the current round
    int s_list[(SCAN_K + 1) * BATCH];   // pending triangle indices (any order), consumed from the top
    int s_big[BATCH];        // tile path: triangles of the current batch waiting for a round
    int s_clist[256];        // live chunks of the current segment (ascending)
    unsigned long long s_mask[2][2][NTILES][BIGB / 64];   // [round parity][0 = 32-bit class, 1 = the rest]
    int s_wtot[2][4];        // hits each wave appended in a scan iteration (double-buffered by iteration parity)
    int s_nbig;
    int s_pending, s_nlive;
};
struct BinHits {
    bool live;   // the image's bounding box touches the bin (else nothing below ran and s_z is not initialised)
    int hits;    // block-uniform: triangles whose bounding box touches this bin
};

// The raster phase of one 32x32 bin (bxi, byi) of image b; OX x OY bins per image.  Resolves every triangle of the image that touches the
// bin into lds.s_z: the lane walk's winners directly, the tile path's register winners folded in at the end -- they are all there once the
// CALLER has passed a barrier (which also publishes whatever its read-out has staged in LDS meanwhile).  Every branch is uniform over
// the workgroup.
// IDS (one-pass objective): the depth key carries the triangle's silhouette bits (sil: [B,T]) below its index, and a bin whose triangle
// list (bin_cnt / bin_list of k_setup<true>, or null: every bin scans the chunk boxes) did not overflow reads it instead of scanning.
template <bool IDS>
__device__ __forceinline__ BinHits bin_raster(BinLds &lds, const int b, const int bxi, const int byi, const int OX, const int OY, int T, int H,
                                              int W, const TriRec *__restrict__ recs, const TriBox *__restrict__ boxes,
                                              const TriBox *__restrict__ cboxes, const ImgBox *__restrict__ ibox,
                                              const int32_t *__restrict__ bin_cnt = nullptr, const int32_t *__restrict__ bin_list = nullptr,
                                              const uint8_t *__restrict__ sil = nullptr) {
    auto &s_z = lds.s_z; auto &s_tri = lds.s_tri; auto &s_big = lds.s_big; auto &s_nbig = lds.s_nbig; auto &s_clist = lds.s_clist;
    auto &s_mask = lds.s_mask; auto &s_list = lds.s_list; auto &s_pending = lds.s_pending; auto &s_nlive = lds.s_nlive; auto &s_wtot = lds.s_wtot;

    const int bin_x0 = bxi * BIN, bin_y0 = byi * BIN;
    const int bin_x1 = min(bin_x0 + BIN, W) - 1, bin_y1 = min(bin_y0 + BIN, H) - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx = lane & 7, ly = lane >> 3;
    const size_t bin_lin = ((size_t)b * OY + byi) * OX + bxi;

    float best_d[TILES_PER_WAVE][4];
    int best_id[TILES_PER_WAVE][4];
#pragma unroll
    for (int k = 0; k < TILES_PER_WAVE; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) { best_d[k][q] = 2.0f; best_id[k][q] = -1; }

    int total_hits = 0;   // block-uniform: triangles whose bounding box touches this bin
    // IDS: the bin's list count and this thread's entry of the list are requested HERE, beside the image box, not behind the depth
    // buffer's initialisation and its barrier: two hops less in the chain count -> entry -> record that every workgroup waits through.
    // The entry goes to s_list with the initialisation (it must not live in a register across the walk: 72 are what seven workgroups per
    // CU leave); entries at or beyond the count are never read, and the list holds BL_CAP = 256 slots per bin: the address is valid.
    static_assert(BL_CAP == BATCH, "one list entry per thread");
    const int cnt_early = (IDS && bin_cnt) ? bin_cnt[bin_lin] : -1;
    const int entry_early = (IDS && bin_cnt) ? bin_list[bin_lin * BL_CAP + tid] : 0;
    const ImgBox ib = ibox[b];
    const bool bin_live = !(ib.x1 < bin_x0 || ib.x0 > bin_x1 || ib.y1 < bin_y0 || ib.y0 > bin_y1);

    if (bin_live) {
        for (int k = tid; k < BIN * BIN; k += 256) s_z[k] = Z_EMPTY;
        for (int k = tid; k < 4 * NTILES * (BIGB / 64); k += 256) (&s_mask[0][0][0][0])[k] = 0ull;
        if (tid == 0) { s_nbig = 0; s_pending = 0; s_nlive = 0; }
        if (IDS && bin_cnt) s_list[tid] = entry_early;
        __syncthreads();
        // record slots of the image: [0, T) one per triangle, [Tp, Tp + n_over) the second pieces of clipped triangles (k_setup); slot =
        // chunk * 256 + lane in both regions (Tp is chunk-aligned), and the overflow chunks, which carry no chunk box, are all scanned
        const int Tp = padded_slots(T), n_over = ib.n_over, slot_end = Tp + n_over;
        const TriBox *bx = boxes + (size_t)b * 2 * Tp;
        const TriRec *rc = recs + (size_t)b * 2 * Tp;
        const int n_prim = Tp / 256, n_chunks = n_prim + (n_over + 255) / 256;
        const TriBox *cbx = cboxes + (size_t)b * n_prim;
        const unsigned long long below = (1ull << lane) - 1ull;
        int pending = 0;  // block-uniform copy of s_pending: entries waiting in s_list
        int round_no = 0; // block-uniform: tile-path rounds done (parity selects the mask buffer)
        // The winner of a pixel is the minimum of (depth, triangle index), which does not depend on the order in which
        // triangles arrive: lists are filled with one LDS atomic per wave and consumed from the top, no ordered compaction.
        auto process_batch = [&](const int n) {
            // consumes entries [pending - n, pending) of s_list; a barrier has been passed since they were appended
            // ---- lane path: a thread rasterises one triangle of the batch over its bounding box; a batch of at most 128 (64)
            // triangles -- the usual bin of a face mesh holds ~120 -- is walked by 2 (4) threads per triangle, rows interleaved,
            // so that all four waves share the work ----
            const int split = n <= 64 ? 4 : (n <= 128 ? 2 : 1);
            if (tid < n * split) {
                const int part = (tid >= n) + (tid >= 2 * n) + (tid >= 3 * n);
                const int t = s_list[pending - n + (tid - part * n)];
                // IDS: the triangle's silhouette bits ride BELOW its index in the depth key -- (index << 3) | bits keeps the order of the
                // indices (rule R6) -- so that the read-out has them with the winner: one byte gather per (bin, triangle), in flight beside
                // the record's, instead of a dependent one per pixel at the workgroup's end
                unsigned int silb = IDS ? (unsigned int)ld32(sil + (size_t)b * T, (unsigned int)(t < T ? t : 0)) : 0u;
                const TriRec r = ld32(rc, t);
                const TriBox q = ld32(bx, t);
                if (IDS && t >= T) silb = (unsigned int)ld32(sil + (size_t)b * T, (unsigned int)r.tid);      // (second piece of a clipped triangle)
                const int zkey = IDS ? (int)(((unsigned int)r.tid << 3) | silb) : r.tid;
                const int ext_x = max(r.X0, max(r.X1, r.X2)) - min(r.X0, min(r.X1, r.X2));
                const int ext_y = max(r.Y0, max(r.Y1, r.Y2)) - min(r.Y0, min(r.Y1, r.Y2));
                const int x0 = max((int)q.x0, bin_x0), x1 = min((int)q.x1, bin_x1);
                const int y0 = max((int)q.y0, bin_y0), y1 = min((int)q.y1, bin_y1);
                const int bw = x1 - x0 + 1, area = bw * (y1 - y0 + 1);
                if (ext_x <= SMALL_EXTENT && ext_y <= SMALL_EXTENT && area <= LANE_MAX) {
                    // every sample lies inside the triangle's box: |P - anchor| <= 16384 + 128, |A|,|B| <= 16384, so the
                    // edge functions fit int32 and their products v_mad_i32_i24 (same integers as the other paths)
                    const int D = (r.X1 - r.X0) * (r.Y2 - r.Y0) - (r.Y1 - r.Y0) * (r.X2 - r.X0);
                    const int sg = D > 0 ? 1 : -1;
                    const int A0 = -(r.Y2 - r.Y1) * sg, B0 = (r.X2 - r.X1) * sg;
                    const int A1 = -(r.Y0 - r.Y2) * sg, B1 = (r.X0 - r.X2) * sg;
                    const int A2 = -(r.Y1 - r.Y0) * sg, B2 = (r.X1 - r.X0) * sg;
                    // R5 tie rule, folded into the constants: E' = E - 1 for an edge that does not own E == 0
                    const int n0 = ((-A0 > 0) || (A0 == 0 && B0 < 0)) ? 0 : 1;
                    const int n1 = ((-A1 > 0) || (A1 == 0 && B1 < 0)) ? 0 : 1;
                    const int n2 = ((-A2 > 0) || (A2 == 0 && B2 < 0)) ? 0 : 1;
                    const int Px = x0 * SUBPIX + HALFPIX, Py = (y0 + part) * SUBPIX + HALFPIX;
                    int R0 = __mul24(A0, Px - r.X1) + __mul24(B0, Py - r.Y1) - n0;   // edge functions at the row start
                    int R1 = __mul24(A1, Px - r.X2) + __mul24(B1, Py - r.Y2) - n1;
                    int R2 = __mul24(A2, Px - r.X0) + __mul24(B2, Py - r.Y0) - n2;
                    const int A0s = A0 * SUBPIX, A1s = A1 * SUBPIX, A2s = A2 * SUBPIX;
                    unsigned long long *zrow = &s_z[(y0 + part - bin_y0) * BIN + (x0 - bin_x0)];
                    const int bh = y1 - y0 + 1;
                    // rows outside, columns inside (the flattened loop that this replaces spent two thirds of its instructions on
                    // wrap-around selects).  A trip carries five running values: the three edge functions, the LDS address of the sample
                    // -- whose comparison with the row's end is the loop test, no column counter beside it -- and the depth plane's x
                    // offset AS A FLOAT: |Px - X0| and |Py - Y0| stay below 2^24 and move in steps of SUBPIX, so the float is the
                    // integer's conversion bit for bit at every sample, for one addition instead of an addition and a conversion.
                    // Listing: 6 vector instructions per sample + 2 for the inside test + 5 on a hit (profiles/bins_sample_loop.txt).
                    static_assert(SMALL_EXTENT + HALFPIX + BIN * SUBPIX < (1 << 24), "the lane walk's running floats are exact");
                    const int B0s = B0 * SUBPIX * split, B1s = B1 * SUBPIX * split, B2s = B2 * SUBPIX * split;
                    const float rxf0 = (float)(Px - r.X0);
                    float ryf = (float)(Py - r.Y0);
                    for (int rr = part; rr < bh; rr += split) {
                        int E0 = R0, E1 = R1, E2 = R2;
                        float rxf = rxf0;
                        const float dzr = __fmaf_rn(r.zB, ryf, r.z0);
                        for (unsigned long long *zp = zrow, *const zend = zrow + bw; zp < zend; ++zp) {
                            if ((E0 | E1 | E2) >= 0) {
                                const float d = __fmaf_rn(r.zA, rxf, dzr);
                                if (d >= -1.0f && d <= 1.0f) atomicMin(zp, zpack(d, zkey));
                            }
                            E0 += A0s; E1 += A1s; E2 += A2s; rxf += (float)SUBPIX;
                        }
                        R0 += B0s; R1 += B1s; R2 += B2s;
                        ryf += (float)(SUBPIX * split);
                        zrow += BIN * split;
                    }
                } else if (part == 0) {
                    s_big[atomicAdd(&s_nbig, 1)] = t;
                }
            }
            __syncthreads();
            // ---- tile path, BIGB triangles per round (block-uniform loop; rare on the meshes this is built for) ----
            const int nbig = __builtin_amdgcn_readfirstlane(s_nbig);
            for (int base = 0; base < nbig; base += BIGB, ++round_no) {
                const int m = min(BIGB, nbig - base);
                unsigned long long (*mask)[NTILES][BIGB / 64] = s_mask[round_no & 1];
                bool any_large = false;
                if (tid < m) {
                    const int t = s_big[base + tid];
                    const TriRec r = ld32(rc, t);
                    const TriBox q = ld32(bx, t);
                    EdgeRec e;
                    e.id = IDS ? (int)(((unsigned int)r.tid << 3) | (unsigned int)ld32(sil + (size_t)b * T, (unsigned int)r.tid)) : r.tid;      // (the depth key's low word)
                    e.zA = r.zA; e.zB = r.zB; e.z0 = r.z0;
                    e.X0 = r.X0; e.Y0 = r.Y0;
                    const int ext_x = max(r.X0, max(r.X1, r.X2)) - min(r.X0, min(r.X1, r.X2));
                    const int ext_y = max(r.Y0, max(r.Y1, r.Y2)) - min(r.Y0, min(r.Y1, r.Y2));
                    const bool small = ext_x <= SMALL_EXTENT && ext_y <= SMALL_EXTENT;
                    int nb = 0;
                    // edge 0: (1,2)  edge 1: (2,0)  edge 2: (0,1);  A = -(Yb - Ya) s, B = (Xb - Xa) s
                    if (small) {   // everything fits in int32
                        const int D = (r.X1 - r.X0) * (r.Y2 - r.Y0) - (r.Y1 - r.Y0) * (r.X2 - r.X0);
                        const int sg = D > 0 ? 1 : -1;
                        e.A0 = -(r.Y2 - r.Y1) * sg; e.B0 = (r.X2 - r.X1) * sg;
                        e.A1 = -(r.Y0 - r.Y2) * sg; e.B1 = (r.X0 - r.X2) * sg;
                        e.A2 = -(r.Y1 - r.Y0) * sg; e.B2 = (r.X1 - r.X0) * sg;
                        nb = 8;
                        e.v.X1 = r.X1; e.v.Y1 = r.Y1; e.v.X2 = r.X2; e.v.Y2 = r.Y2; e.v.X0 = r.X0; e.v.Y0 = r.Y0;
                    } else {
                        any_large = true;
                        const long long X0 = r.X0, Y0 = r.Y0, X1 = r.X1, Y1 = r.Y1, X2 = r.X2, Y2 = r.Y2;
                        const long long D = (X1 - X0) * (Y2 - Y0) - (Y1 - Y0) * (X2 - X0);
                        const long long sg = D > 0 ? 1 : -1;
                        e.A0 = (int32_t)(-(Y2 - Y1) * sg); e.B0 = (int32_t)((X2 - X1) * sg);
                        e.A1 = (int32_t)(-(Y0 - Y2) * sg); e.B1 = (int32_t)((X0 - X2) * sg);
                        e.A2 = (int32_t)(-(Y1 - Y0) * sg); e.B2 = (int32_t)((X1 - X0) * sg);
                    }
                    // R5 tie rule: an edge owns E == 0 iff its direction (dx,dy) = (B,-A) has dy > 0, or dy == 0 and dx < 0
                    nb |= ((-e.A0 > 0) || (e.A0 == 0 && e.B0 < 0)) ? 0 : 1;
                    nb |= ((-e.A1 > 0) || (e.A1 == 0 && e.B1 < 0)) ? 0 : 2;
                    nb |= ((-e.A2 > 0) || (e.A2 == 0 && e.B2 < 0)) ? 0 : 4;
                    if (!small) {
                        e.C[0] = -((long long)e.A0 * r.X1 + (long long)e.B0 * r.Y1) - (nb & 1);
                        e.C[1] = -((long long)e.A1 * r.X2 + (long long)e.B1 * r.Y2) - ((nb >> 1) & 1);
                        e.C[2] = -((long long)e.A2 * r.X0 + (long long)e.B2 * r.Y0) - ((nb >> 2) & 1);
                    }
                    e.nb = nb;
                    s_tri[tid] = e;
                    const int tx0 = (max((int)q.x0, bin_x0) - bin_x0) >> 4, tx1 = (min((int)q.x1, bin_x1) - bin_x0) >> 4;
                    const int ty0 = (max((int)q.y0, bin_y0) - bin_y0) >> 4, ty1 = (min((int)q.y1, bin_y1) - bin_y0) >> 4;
                    const unsigned long long bit = 1ull << (tid & 63);
                    for (int ty = ty0; ty <= ty1; ++ty)
                        for (int tx = tx0; tx <= tx1; ++tx) atomicOr(&mask[small ? 0 : 1][ty * TILES_X + tx][tid >> 6], bit);
                }
                const int large_round = __builtin_amdgcn_readfirstlane(__syncthreads_or(any_large ? 1 : 0));
                // fine raster: this wave's 16x16 tile, four pixels per lane, winners in registers
#pragma unroll
                for (int k = 0; k < TILES_PER_WAVE; ++k) {
                    const int tile = wave * TILES_PER_WAVE + k;
                    const int px = bin_x0 + (tile % TILES_X) * TILE + lx, py = bin_y0 + (tile / TILES_X) * TILE + ly;
                    fine_tile<true>(mask[0][tile], s_tri, px * SUBPIX + HALFPIX, py * SUBPIX + HALFPIX, best_d[k], best_id[k]);
                    if (large_round)
                        fine_tile<false>(mask[1][tile], s_tri, px * SUBPIX + HALFPIX, py * SUBPIX + HALFPIX, best_d[k], best_id[k]);
                }
                __syncthreads();
                // this parity's masks are next written two rounds from now, with a barrier in between
                for (int k = tid; k < 2 * NTILES * (BIGB / 64); k += 256) (&mask[0][0][0])[k] = 0ull;
            }
            if (tid == 0) { s_pending = pending - n; s_nbig = 0; }
            pending -= n;
            __syncthreads();
        };
        // ---- the bin's own triangle list (one count, one gather), unless it overflowed ----
        const int n_listed = (IDS && bin_cnt) ? __builtin_amdgcn_readfirstlane(cnt_early) : -1;
        if (n_listed >= 0 && n_listed <= BL_CAP) {
            total_hits = n_listed;
            if (n_listed > 0) {      // (the list is in s_list[0 .. n_listed): one batch)
                pending = n_listed;
                process_batch(n_listed);
            }
        } else
        for (int seg = 0; seg < n_chunks; seg += 256) {
            // ---- which of the next 256 chunks touch this bin?  (one box test per chunk) ----
            {
                const int c = seg + tid;
                bool live = false;
                if (c < n_prim) {
                    const TriBox q = ld32(cbx, c);
                    live = (q.x0 <= q.x1) && !(q.x1 < bin_x0 || q.x0 > bin_x1 || q.y1 < bin_y0 || q.y0 > bin_y1);
                } else if (c < n_chunks) {
                    live = true;
                }
                const unsigned long long bal = __ballot(live);
                int base = 0;
                if (lane == 0 && bal) base = atomicAdd(&s_nlive, __popcll(bal));
                base = __builtin_amdgcn_readfirstlane(base);
                if (live) s_clist[base + __popcll(bal & below)] = c;
            }
            __syncthreads();
            const int n_live = __builtin_amdgcn_readfirstlane(s_nlive);
            // ---- scan the bounding boxes of SCAN_K live chunks per iteration (independent loads in flight) ----
            for (int ci = 0, it = 0; ci < n_live; ci += SCAN_K, ++it) {
                bool hit[SCAN_K];
                int tt[SCAN_K];
#pragma unroll
                for (int k = 0; k < SCAN_K; ++k) {
                    hit[k] = false;
                    tt[k] = (ci + k < n_live) ? s_clist[ci + k] * 256 + tid : slot_end;
                    if (tt[k] >= T && tt[k] < Tp) tt[k] = slot_end;      // (padding of the last triangle chunk)
                }
                TriBox qk[SCAN_K];
#pragma unroll
                for (int k = 0; k < SCAN_K; ++k) qk[k] = ld32(bx, min(tt[k], slot_end - 1));
                unsigned long long bal[SCAN_K];
                int total = 0;
#pragma unroll
                for (int k = 0; k < SCAN_K; ++k) {
                    const TriBox q = qk[k];
                    hit[k] = tt[k] < slot_end && (q.x0 <= q.x1) && !(q.x1 < bin_x0 || q.x0 > bin_x1 || q.y1 < bin_y0 || q.y0 > bin_y1);
                    bal[k] = __ballot(hit[k]);
                    total += __popcll(bal[k]);
                }
                int base = 0;
                if (lane == 0 && total) base = atomicAdd(&s_pending, total);
                if (lane == 0) s_wtot[it & 1][wave] = total;
                base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
                for (int k = 0; k < SCAN_K; ++k) {
                    if (hit[k]) s_list[base + __popcll(bal[k] & below)] = tt[k];
                    base += __popcll(bal[k]);
                }
                __syncthreads();
                // block-uniform by construction: the four waves' counts of THIS iteration (a fast wave may already be
                // adding the next iteration's hits to s_pending, so that counter must not be re-read here)
                const int added = __builtin_amdgcn_readfirstlane(s_wtot[it & 1][0] + s_wtot[it & 1][1] + s_wtot[it & 1][2] + s_wtot[it & 1][3]);
                pending += added;
                total_hits += added;
                while (pending >= BATCH) process_batch(BATCH);
            }
            if (seg + 256 < n_chunks) {   // another segment follows: recycle the chunk list
                __syncthreads();
                if (tid == 0) s_nlive = 0;
                __syncthreads();
            }
        }
        while (pending > 0) process_batch(min(pending, BATCH));
        // ---- fold the tile path's register winners into the depth buffer (no barrier here: see above) ----
#pragma unroll
        for (int k = 0; k < TILES_PER_WAVE; ++k) {
            const int tile = wave * TILES_PER_WAVE + k;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int zx = (tile % TILES_X) * TILE + (q & 1) * QUAD + lx, zy = (tile / TILES_X) * TILE + (q >> 1) * QUAD + ly;
                if (best_id[k][q] >= 0) atomicMin(&s_z[zy * BIN + zx], zpack(best_d[k][q], best_id[k][q]));
            }
        }
    }
    return {bin_live, total_hits};
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// layout of the caller's scratch buffer: records and boxes (2 Tp slots per image: triangles + overflow), chunk boxes, image boxes, clip lists
struct RasterScratch { TriRec *recs; TriBox *boxes, *cboxes; ImgBox *ibox; int32_t *clip; size_t bytes; };
static RasterScratch raster_scratch(void *base, int B, int T) {
    const size_t n = (size_t)B * 2 * (size_t)padded_slots(T), nc = (size_t)B * (size_t)(padded_slots(T) / 256);
    char *s = (char *)base;
    RasterScratch r;
    r.recs = (TriRec *)s;
    r.boxes = (TriBox *)(s + align_up(n * sizeof(TriRec), 256));
    r.cboxes = (TriBox *)((char *)r.boxes + align_up(n * sizeof(TriBox), 256));
    r.ibox = (ImgBox *)((char *)r.cboxes + align_up(nc * sizeof(TriBox), 256));
    r.clip = (int32_t *)((char *)r.ibox + align_up((size_t)B * sizeof(ImgBox), 256));      // [B][Tp] clip lists (k_setup -> k_setup_clip)
    r.bytes = (size_t)((char *)r.clip - s) + align_up((size_t)B * (size_t)padded_slots(T) * sizeof(int32_t), 256);
    return r;
}

// Set-up of a call without per-bin triangle lists: every triangle's record and boxes, then the clipped ones.  The caller has initialised
// the image boxes.  live: the map of bins some chunk box touches (work-queue mode), or null; ranges: per-image slices of tri, or null.
static void launch_setup(hipStream_t st, const float *pos, const int32_t *tri, int B, int V, int T, int H, int W, const RasterScratch &rs,
                         uint8_t *live, const int32_t *ranges) {
    hipLaunchKernelGGL(k_setup<false>, dim3(fpcdr_cdiv(T, 256), B), dim3(256), 0, st, (const float4 *)pos, tri, B, V, T, H, W, rs.recs, rs.boxes,
                       rs.cboxes, rs.ibox, live, ranges, (int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr, (uint8_t *)nullptr, rs.clip);
    hipLaunchKernelGGL(k_setup_clip<false>, dim3(B), dim3(256), 0, st, (const float4 *)pos, tri, V, T, H, W, rs.recs, rs.boxes, rs.cboxes, rs.ibox,
                       live, (int32_t *)nullptr, (int32_t *)nullptr, rs.clip);
}

// One list round: the flagged bins of `map` in ascending order to list0 / list1 (bin_flags<ROUND_B>), their numbers to count0 / count1;
// blk: [2][ceil(nbins / 256)] per-block counts.  sum_in_write: two launches (k_list_write_sum) instead of three.  Round A also leaves the
// colour of an empty pixel in empty_out; round B the window masks in win.
template <int ROUND_B>
static void launch_list_round(hipStream_t st, bool sum_in_write, const uint8_t *map, size_t nbins, int OY, int OX, int32_t *blk, int32_t *list0,
                              int32_t *list1, int32_t *count0, int32_t *count1, uint16_t *win, const float *tex = nullptr, int Ht = 0,
                              int Wt = 0, int C = 0, int boundary = 0, float *empty_out = nullptr) {
    const int nblk = fpcdr_cdiv((long long)nbins, 256);
    hipLaunchKernelGGL(k_list_count<ROUND_B>, dim3(nblk), dim3(256), 0, st, map, (long long)nbins, OY, OX, blk, win, tex, Ht, Wt, C, boundary,
                       empty_out);
    if (sum_in_write)
        hipLaunchKernelGGL(k_list_write_sum<ROUND_B>, dim3(nblk), dim3(256), 0, st, map, (long long)nbins, OY, OX, blk, list0, list1, count0, count1);
    else {
        hipLaunchKernelGGL(k_list_scan, dim3(1), dim3(1024), 0, st, blk, nblk, count0, count1);
        hipLaunchKernelGGL(k_list_write<ROUND_B>, dim3(nblk), dim3(256), 0, st, map, (long long)nbins, OY, OX, blk, list0, list1);
    }
}

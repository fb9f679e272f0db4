/*
 * fpcdr.h -- C ABI of the MI355X (gfx950) differentiable-raster path.
 *
 * Drop-in boundary.  In the reference the four operators are Python calls
 * into the third-party package nvdiffrast (reference src/torch/fit.py:13); the reference itself
 * has no FFI.  Each entry point below states the reference call site whose work it performs; the
 * Python binding that preserves the nvdiffrast signatures is fpc_diffrend_amd/ops.py and the
 * binding a maintainer of the reference would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no torch / HIP types: device pointers are void-free typed pointers into HBM, the
 *     stream is passed as void* (a hipStream_t); every launch is asynchronous on that stream;
 *   - the CALLER owns every buffer, including scratch; the library allocates nothing and keeps no
 *     state between calls (re-entrant, any number of devices / streams);
 *   - all tensors are contiguous, float32 / int32, NHWC images with row 0 = bottom scanline;
 *   - gradient outputs documented "accumulated" are added to with atomics and must be zeroed (or
 *     hold a running sum) on entry; all other outputs are fully overwritten;
 *   - return value 0 = launched, otherwise an FPCDR_E* code; fpcdr_last_error() gives the
 *     message (thread-local).  No exception crosses the boundary.
 */
#ifndef FPCDR_H
#define FPCDR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPCDR_ABI_VERSION 16

enum {
    FPCDR_OK = 0,
    FPCDR_EINVAL = 1,   /* bad argument (null pointer, non-positive size, unsupported mode) */
    FPCDR_ELAUNCH = 2   /* the HIP runtime refused the launch */
};

int fpcdr_abi_version(void);
const char *fpcdr_last_error(void);

/* ------------------------------------------------------------------------------------------ */
/* rasterize -- dr.rasterize(glctx, pos, tri, resolution)        reference fit.py:151 (ctx :484) */
/* ------------------------------------------------------------------------------------------ */

/* REGION HINTS.  A face rig covers ~12 % of a 1080p frame; the other pixels of rast are zero, of the texture-coordinate image
 * zero, of the colour image one constant.  fpcdr_rasterize_fwd can leave a map of that: two planes of B x OY x OX bytes
 * (OY, OX = FPCDR_OCC_DIM(H), (W): 32 x 32-pixel bins); plane 0: 1 = some triangle's bounding box touches the bin (else every
 * pixel of the bin is EMPTY); plane 1: plane 0 OR-ed over the 3 x 3 neighbourhood.  An operator that is handed the hint of its
 * input (`hint` fields below; NULL = none) does not READ that input in empty bins -- it writes what the input implies -- which
 * halves the HBM traffic of the operator chain of fit.py:151-160.  Results are identical with and without hints.  A hint is
 * valid only for the very tensor it was produced with (the Python binding drops it when the tensor was modified). */
#define FPCDR_HINT_BYTES(B, H, W) ((size_t)2 * (B) * FPCDR_OCC_DIM(H) * FPCDR_OCC_DIM(W))

/* bytes of scratch fpcdr_rasterize_fwd needs for B images of T triangles: per image two record slots per triangle (one for the
 * triangle, one for the second piece of a triangle clipped against the near plane), their pixel boxes, chunk and image boxes */
size_t fpcdr_rasterize_scratch_bytes(int32_t B, int32_t T);

typedef struct {
    const float *pos;     /* [B,V,4] clip-space positions */
    const int32_t *tri;   /* [T,3] */
    int32_t B, V, T, H, W;
    void *scratch;        /* fpcdr_rasterize_scratch_bytes(B,T) bytes, 16-byte aligned */
    float *rast;          /* out [B,H,W,4] = (u, v, z/w, triangle index + 1; 0 = empty) */
    float *rast_db;       /* out [B,H,W,4] = (du/dx, du/dy, dv/dx, dv/dy) per pixel, or NULL */
    uint8_t *hint;        /* optional out, FPCDR_HINT_BYTES(B,H,W): REGION HINT of rast (see below), or NULL */
    const int32_t *ranges; /* optional [B,2] on the device: image b renders triangles [ranges[b][0], ranges[b][0] + ranges[b][1]) only
                              (nvdiffrast's range mode; triangle ids stay indices into tri), or NULL: every image renders all T */
} fpcdr_rasterize_fwd_params;
int fpcdr_rasterize_fwd(const fpcdr_rasterize_fwd_params *p, void *stream);

typedef struct {
    const float *pos;     /* [B,V,4] */
    const int32_t *tri;   /* [T,3] */
    const float *rast;    /* [B,H,W,4] forward output */
    const float *dy;      /* [B,H,W,4] dL/d rast (only .x .y are used: z/w and id carry no gradient) */
    const float *ddb;     /* [B,H,W,4] dL/d rast_db, or NULL */
    int32_t B, V, T, H, W;
    float *grad_pos;      /* [B,V,4] accumulated (x, y, w components; z receives nothing) */
    const uint8_t *hint;  /* optional: region hint of rast (empty bins are skipped without reading dy / rast) */
} fpcdr_rasterize_bwd_params;
int fpcdr_rasterize_bwd(const fpcdr_rasterize_bwd_params *p, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* shared by the fused entry points                                                              */
/* ------------------------------------------------------------------------------------------ */

#define FPCDR_MAX_MIP 16

#define FPCDR_LOSS_SLOTS 256
#define FPCDR_OCC_BIN 32
#define FPCDR_OCC_DIM(n) (((n) + FPCDR_OCC_BIN - 1) / FPCDR_OCC_BIN)
/* bytes of the occupancy buffer (occ) and of the scratch buffer (cmask) of the fused entry points: fpcdr_objective_fwd below, and the
 * two-call form of include/fpcdr_twocall.h */
/* After a call of the two-call form (fpcdr_twocall.h: fpcdr_render_loss_fwd), int32 counts[4] at byte offset FPCDR_OCC_COUNTS_OFFSET(B,H,W) of occ hold: [0] bins the backward
 * call visits, [2] live bins of the rasteriser, [3] bins of the antialias pass -- what a caller feeds back (with a margin) as
 * cap_bwd / cap_bins / cap_fix of its NEXT calls. */
#define FPCDR_OCC_COUNTS_OFFSET(B, H, W) ((((size_t)(B) * FPCDR_OCC_DIM(H) * FPCDR_OCC_DIM(W) * 4) + 3) / 4 * 4)
size_t fpcdr_occ_bytes(int32_t B, int32_t H, int32_t W);
size_t fpcdr_cmask_bytes(int32_t B, int32_t H, int32_t W);
/* the scratch buffer of fpcdr_objective_fwd alone (its cmask): a quarter of the above (ABI v10) */
size_t fpcdr_objective_cmask_bytes(int32_t B, int32_t H, int32_t W);

/* out[i] += sum over the px_per_image pixels of image i of (ref - bg_scaled)^2, i < n_images; ref [n_images, px_per_image]
 * uint8, out f64 (zero-filled by the caller).  The part of the pixel loss (fit.py:579) that a sparse fpcdr_aa_loss_fwd
 * leaves to the caller: it depends on the reference images only, so a fit loop computes it once. */
int fpcdr_ref_bg_sumsq(const uint8_t *ref, int64_t n_images, int64_t px_per_image, float bg_scaled, double *out, void *stream);

/* Value of the pixel objective: out[0] = float((sum of the n_slots loss slots + bg_coeff * bg_sumsq[0]) / n_total), one launch.
 * bg_sumsq: device scalar (the all-background share of the sparse mode, fpcdr_ref_bg_sumsq summed over the call's images), or NULL. */
int fpcdr_objective_value(const double *loss_slots, int32_t n_slots, const double *bg_sumsq, double bg_coeff, double n_total,
                          float *out, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* ONE-PASS pixel objective (ABI v8, v9) -- reference fit.py:151-161 + the pixel term of :579, VALUE AND GRADIENT in one call.
 *
 * The pixel objective is a scalar, so its gradient with respect to pos and tex does not depend on anything the caller does
 * afterwards: it is d(objective)/d(input) times one upstream scalar.  This entry point therefore computes value and gradient
 * together, while every covered pixel's barycentrics, taps, texels and vertices are still in registers, instead of writing
 * rast / colour / d loss/d colour (24 B/px) for a second call to read back and re-derive (fpcdr_render_loss_fwd +
 * fpcdr_render_aa_bwd; profiles/r04_backward_ablation.txt: 45 % of that backward's instructions were re-derivation):
 *   1. the rasteriser (same kernels and rules as fpcdr_rasterize_fwd) leaves only a 4-byte id per pixel of the occupied
 *      32 x 32 bins: (triangle + 1) | silhouette bits << 24;
 *   2. one shading kernel per occupied bin: barycentrics, texture lookup, background + squared error, and -- with the loss
 *      gradient of the UN-antialiased colour -- texture / interpolate / rasterize backward into grad_tex / grad_pos (per-bin LDS
 *      accumulators, one flush).  Pixels one of whose four pixel pairs has different ids and a triangle with a silhouette edge
 *      (read from the id planes, neighbours' border lines included) are DEFERRED: their (u, v, z/w), colour and gradient are also
 *      written, sparsely, to rec / color / grad_aa;
 *   3. two small kernels over the deferred pixels only (a few per cent of the covered ones): the exact antialias blend, the
 *      correction of their loss terms, and the scatter of the DIFFERENCE of their gradient (everything is linear in it).
 * grad_pos / grad_tex hold d(objective)/d(pos), d(objective)/d(tex) with the objective = grad_scale * sum of squares; the caller
 * multiplies by its upstream scalar.  Same value and gradients as the operator chain (tests/test_gpu_objective.py).
 * 'linear' lookup, or -- mip = 1 -- the reference's mip-mapped branch; C in {1, 3, 4}; instanced mode. */
size_t fpcdr_idplane_bytes(int32_t B, int32_t H, int32_t W);   /* 4 KB per 32 x 32 bin of the batch */
size_t fpcdr_binlist_bytes(int32_t B, int32_t H, int32_t W);   /* per-bin triangle lists: a count + 256 slots per bin (1 KB per bin) */

typedef struct {
    const float *pos;       /* [B,V,4] */
    const int32_t *tri;     /* [T,3] */
    const int32_t *adj;     /* [T,3] fpcdr_topology_build */
    int32_t B, V, T, H, W;
    void *scratch;          /* fpcdr_rasterize_scratch_bytes(B,T) */
    const float *uv;        /* [Vt,2] */
    const int32_t *uv_tri;  /* [T,3] */
    int32_t Vt;
    const float *tri_uv;    /* optional [T,3,2] = uv[uv_tri] */
    const float *tex;       /* [Ht,Wt,C] */
    int32_t Ht, Wt, C, boundary_mode;
    const uint8_t *ref;     /* [B,H,W] reference images, 8 bit */
    float bg, color_scale, grad_scale;
    uint8_t *sil;           /* scratch [B,T] */
    uint32_t *idp;          /* scratch, fpcdr_idplane_bytes(B,H,W), 16-byte aligned */
    uint16_t *occ;          /* scratch+out, fpcdr_occ_bytes(B,H,W): window masks; counts at FPCDR_OCC_COUNTS_OFFSET: [0] bins with a deferred
                               pixel, [2] live bins of the rasteriser, [3] occupied bins (cap_def / cap_bins / cap_occ of the next call) */
    uint32_t *cmask;        /* scratch, fpcdr_objective_cmask_bytes(B,H,W), 8-byte aligned */
    float *rec;             /* scratch [B,H,W,4]: (u, v, z/w, -) of DEFERRED pixels only (dense addressing, sparse writes; or rec_slots, below) */
    float *color;           /* scratch [B,H,W,C]: colour of deferred pixels only */
    float *grad_aa;         /* scratch [B,H,W,C]: d(objective)/d(antialiased colour) of deferred pixels only */
    float *empty_color;     /* out [4]: the colour of an empty pixel (the texture at uv = (0,0)) */
    double *loss_sum;       /* [FPCDR_LOSS_SLOTS] f64 accumulated: difference to an all-background image, as the sparse mode of fpcdr_aa_loss_fwd does */
    float *grad_pos;        /* [B,V,4] accumulated, or NULL */
    float *grad_tex;        /* [Ht,Wt,C] accumulated, or NULL (both NULL: value only) */
    int32_t cap_bins, cap_occ; /* launch-size hints (0 = none), as in fpcdr_aa_loss_fwd_params */
    int32_t cap_def;        /* launch-size hint for the kernels over the bins that hold a deferred pixel (count at [0] of the occ header) */
    int32_t sil_ready;      /* 1: `sil` already holds fpcdr_silhouette_bits() of this pos / tri / adj (a caller computes it on a second
                               stream beside the rasteriser's set-up kernel: ~70 us of a 2.7 ms call at 288 x 1080p); 0: computed here */
    uint64_t *flags;        /* optional (tests / diagnostics; NULL in production): the antialias flag planes of fpcdr_antialias_fwd --
                               which pixel pairs were blended --, fpcdr_antialias_flags_bytes(B,H,W), zero-filled by the caller */
    /* the reference's enable_mip branch (fit.py:153-155): interpolate with the rasteriser's screen-space derivatives and texture
     * 'linear-mipmap-linear', inside the same kernels (the derivatives never exist in HBM) */
    int32_t mip;            /* 1 = mip-mapped lookup */
    int32_t n_levels;       /* levels below tex, 0 .. FPCDR_MAX_MIP */
    const float *tex_mip[FPCDR_MAX_MIP];   /* tex_mip[l - 1] = level l, [Ht >> l, Wt >> l, C] (fpcdr_mip_downsample) */
    float *grad_tex_mip[FPCDR_MAX_MIP];    /* per level, accumulated (the caller folds them into grad_tex: fpcdr_mip_downsample_bwd) */
    void *binlist;          /* optional scratch, fpcdr_binlist_bytes(B,H,W), 4-byte aligned: per-bin triangle lists written by the set-up kernel
                               and read by the rasteriser (one count + one gather per bin instead of the scan of the chunks' boxes: 0.2 ms of
                               the call at 288 x 1080p); NULL: every bin scans.  Same result */
    void *sil_event;        /* with sil_ready = 1: optional hipEvent_t recorded behind the caller's fpcdr_silhouette_bits on ITS stream; the
                               call makes `stream` wait for it right before the first kernel that reads sil (behind the set-up kernels, which
                               is the point: they overlap).  NULL: sil is complete in stream order */
    /* ABI v9: the launches around the call folded into its first and its last kernel (each was 5-20 us of a 2.6 ms call's serial tail) */
    int32_t zero_outputs;   /* 1: the call's first kernel zero-fills loss_sum, grad_pos, grad_tex and grad_tex_mip (they need no initialisation);
                               0: they are accumulated into, as above */
    int32_t counts_seq;     /* any number that differs from call to call (see counts_out) */
    int32_t *counts_out;    /* optional [8]: a sequence lock.  The last kernel writes counts_seq to [6], then the four counters at
                               FPCDR_OCC_COUNTS_OFFSET of occ to [0..3], [5] += 1 if this call ran out of record slots (CUMULATIVE: only the
                               reader ever resets it), [7] = 1 if [1] is meaningful (compact records or count_only; a dense call counts no
                               slots), then counts_seq to [4], with system-scope fences in between.  May be HOST memory the device can write
                               (hipHostMalloc / pinned): the launch hints of the next call then need no device-to-host copy in the stream.
                               A reader takes [4], the counters, then [6]: the counters belong to ONE call iff [4] == [6] */
    const double *bg_sumsq; /* optional [1] (with value_out): the sum over the call's images of fpcdr_ref_bg_sumsq */
    double bg_coeff;        /* its coefficient (the number of colour channels) */
    double n_total;         /* the mean's denominator */
    float *value_out;       /* optional [1]: (sum of loss_sum + bg_coeff * bg_sumsq[0]) / n_total, what fpcdr_objective_value computes, from the
                               last kernel of the call */
    void *zero_extra;       /* optional: zero_extra_bytes (a multiple of 4) of the caller's own that the first kernel zero-fills as well -- a fit
                               step's small accumulators (the gradients of the camera matrices, poses and blend weights that its backward
                               kernels add into) instead of one fill launch each */
    int64_t zero_extra_bytes;
    /* ABI v10: COMPACT records.  rec / color / grad_aa are addressed by pixel of the whole batch above -- 24 B per pixel allocated (14 GB
     * at 288 x 1080p) for the 0.2 % of the pixels that are deferred.  With rec_slots > 0 they hold rec_slots SLOTS of 1 024 pixels instead
     * ([rec_slots * 1024, 4] / [.., C] / [.., C]); every occupied bin that shows a triangle with a silhouette edge -- the only bins that can
     * hold a deferred pixel -- takes the next slot.  The number of such bins is counted by every call (counts_out[1]; it keeps counting
     * beyond rec_slots), so a caller sizes rec_slots from the previous call on the batch, with a margin; a call that runs out of slots
     * bumps counts_out[5]: ITS RESULTS ARE THEN INVALID (the bins without a slot were shaded without their antialias pairs) and it SAYS SO
     * IN THE SAME CALL -- value_out receives NaN and skip_out 1 -- so that no optimiser step consumes them (fpcdr_adam_params.skip_flag).
     * The next call on the batch is sized from the demand this one counted.  A caller without a previous call asks first: count_only = 1
     * runs the rasteriser alone and reports the exact number for this very batch through counts_out (no record buffers, no gradients
     * needed). */
    int32_t rec_slots;      /* 0: dense addressing */
    int32_t count_only;
    int32_t *slot_map;      /* scratch with rec_slots > 0: one int32 per 32 x 32 bin of the batch (B * FPCDR_OCC_DIM(H) * FPCDR_OCC_DIM(W)) */
    /* ABI v11 */
    float *skip_out;        /* optional DEVICE [1]: the last kernel WRITES 1.0f when the call ran out of record slots (its value and gradients
                               are invalid), 0.0f otherwise.  Handed to fpcdr_adam_step as skip_flag the update of that step does not
                               happen; under data parallelism the caller sums it over the ranks first (it may be an element of the gradient
                               bucket), so that every rank skips the same step */
} fpcdr_objective_params;
int fpcdr_objective_fwd(const fpcdr_objective_params *p, void *stream);

/* sil[b][t] = 3 bits, "edge e of triangle t is a silhouette edge in image b" (boundary edge, or the two triangles' opposite vertices
 * project to the same side: DESIGN.md "Antialias rules"), as fpcdr_antialias_fwd and fpcdr_objective_fwd compute it themselves.
 * pos [B,V,4], tri [T,3], adj [T,3] (fpcdr_topology_build), sil out [B,T] bytes. */
int fpcdr_silhouette_bits(const float *pos, const int32_t *tri, const int32_t *adj, int32_t B, int32_t V, int32_t T, int32_t H, int32_t W,
                          uint8_t *sil, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* interpolate -- dr.interpolate(attr, rast, tri[, rast_db, diff_attrs])  reference fit.py:154,157 */
/* ------------------------------------------------------------------------------------------ */

#define FPCDR_MAX_ATTR 32

typedef struct {
    const float *attr;    /* [Ba,Vt,A], Ba = 1 (broadcast) or B */
    const float *rast;    /* [B,H,W,4] */
    const int32_t *tri;   /* [T,3] index buffer of attr (e.g. uv_idx) */
    const float *rast_db; /* [B,H,W,4] or NULL when n_diff == 0 */
    int32_t B, H, W, Ba, Vt, A, T;
    int32_t n_diff;                     /* number of attributes with pixel differentials */
    int32_t diff_idx[FPCDR_MAX_ATTR];   /* their indices into A (diff_attrs='all' -> 0..A-1) */
    float *out;           /* out [B,H,W,A] */
    float *out_da;        /* out [B,H,W,2*n_diff] = (da/dx, da/dy) per selected attribute, or NULL */
    const uint8_t *hint;  /* optional: region hint of rast -- empty bins are written as zeros without reading rast */
} fpcdr_interpolate_fwd_params;
int fpcdr_interpolate_fwd(const fpcdr_interpolate_fwd_params *p, void *stream);

typedef struct {
    const float *attr, *rast;
    const int32_t *tri;
    const float *rast_db;
    const float *dy;      /* [B,H,W,A] */
    const float *dda;     /* [B,H,W,2*n_diff] or NULL */
    int32_t B, H, W, Ba, Vt, A, T;
    int32_t n_diff;
    int32_t diff_idx[FPCDR_MAX_ATTR];
    float *grad_attr;     /* [Ba,Vt,A] accumulated, or NULL (attr needs no gradient, as in fit.py:431) */
    float *grad_rast;     /* out [B,H,W,4] (.z .w are written as 0) */
    float *grad_rast_db;  /* out [B,H,W,4], or NULL when n_diff == 0 */
    const uint8_t *hint;  /* optional: region hint of rast -- empty bins get zero gradients without reading dy / rast */
} fpcdr_interpolate_bwd_params;
int fpcdr_interpolate_bwd(const fpcdr_interpolate_bwd_params *p, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* texture -- dr.texture(tex, uv[, uv_da], filter_mode, boundary_mode, max_mip_level)             */
/*                                                                   reference fit.py:155,158    */
/* ------------------------------------------------------------------------------------------ */

enum { FPCDR_FILTER_NEAREST = 0, FPCDR_FILTER_LINEAR = 1, FPCDR_FILTER_LINEAR_MIPMAP_NEAREST = 2,
       FPCDR_FILTER_LINEAR_MIPMAP_LINEAR = 3 };
enum { FPCDR_BOUNDARY_WRAP = 0, FPCDR_BOUNDARY_CLAMP = 1, FPCDR_BOUNDARY_ZERO = 2 };   /* ZERO: texture padded with zeros */

/* level l+1 [N,Ht/2,Wt/2,C] = 2x2 box filter of level l [N,Ht,Wt,C] (Ht, Wt even) */
int fpcdr_mip_downsample(const float *src, float *dst, int32_t N, int32_t Ht, int32_t Wt, int32_t C, void *stream);
/* gradient of the above: grad_src [N,Ht,Wt,C] += 0.25 * grad_dst of its 2x2 parent (plain add, not atomic) */
int fpcdr_mip_downsample_bwd(const float *grad_dst, float *grad_src, int32_t N, int32_t Ht, int32_t Wt, int32_t C,
                             void *stream);

typedef struct {
    const float *tex[FPCDR_MAX_MIP + 1];  /* tex[0] = [Bt,Ht,Wt,C]; tex[l] = level l of the chain */
    int32_t n_levels;                     /* number of mip levels beyond level 0 (0 for non-mip filters) */
    const float *uv;                      /* [B,H,W,2] */
    const float *uv_da;                   /* [B,H,W,4] = (du/dx,du/dy,dv/dx,dv/dy) or NULL */
    const float *mip_level_bias;          /* [B,H,W] or NULL */
    int32_t B, H, W, Bt, Ht, Wt, C;
    int32_t filter_mode, boundary_mode;
    float *out;                           /* out [B,H,W,C] */
    const uint8_t *hint;                  /* optional (filter nearest / linear, Bt = 1): region hint of uv -- uv is (0,0) in empty
                                             bins, which get the texture's value there without reading uv */
    float *empty_color;                   /* with hint: out [C], that value (the hint of `out` for fpcdr_antialias_fwd) */
} fpcdr_texture_fwd_params;
int fpcdr_texture_fwd(const fpcdr_texture_fwd_params *p, void *stream);

typedef struct {
    const float *tex[FPCDR_MAX_MIP + 1];
    int32_t n_levels;
    const float *uv, *uv_da, *mip_level_bias;
    const float *dy;                      /* [B,H,W,C] */
    int32_t B, H, W, Bt, Ht, Wt, C;
    int32_t filter_mode, boundary_mode;
    float *grad_tex[FPCDR_MAX_MIP + 1];   /* per level, accumulated; grad_tex[0] may be NULL (tex needs no grad) */
    float *grad_uv;                       /* out [B,H,W,2] or NULL */
    float *grad_uv_da;                    /* out [B,H,W,4] or NULL */
    float *grad_mip_level_bias;           /* out [B,H,W] or NULL */
    const uint8_t *hint;                  /* optional (filter linear, C = 1, Bt = 1): region hint of uv, which is then not read
                                             in empty bins */
} fpcdr_texture_bwd_params;
int fpcdr_texture_bwd(const fpcdr_texture_bwd_params *p, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* antialias -- dr.antialias(color, rast, pos, tri)                       reference fit.py:160   */
/* ------------------------------------------------------------------------------------------ */

/* Edge adjacency of an index buffer, built once per `tri` tensor (nvdiffrast's "topology hash").
 * adj[t][e], e = edge opposite to corner e (joins corners (e+1)%3 and (e+2)%3):
 *    >= 0  vertex index opposite to the edge in the one other triangle sharing it
 *    -1    boundary edge (no other triangle)      -2  shared by more than two triangles */
size_t fpcdr_topology_scratch_bytes(int32_t T);
int fpcdr_topology_build(const int32_t *tri, int32_t T, void *scratch, int32_t *adj /* out [T,3] */, void *stream);

/* words (uint64) per flag bit-plane row */
#define FPCDR_AA_ROW_WORDS(W) (((W) + 63) / 64)
/* bytes of the flag planes written by the forward pass and read by the backward pass */
size_t fpcdr_antialias_flags_bytes(int32_t B, int32_t H, int32_t W);

typedef struct {
    const float *color;   /* [B,H,W,C] */
    const float *rast;    /* [B,H,W,4] */
    const float *pos;     /* [B,V,4] */
    const int32_t *tri;   /* [T,3] */
    const int32_t *adj;   /* [T,3] from fpcdr_topology_build */
    int32_t B, H, W, C, V, T;
    uint8_t *sil;         /* scratch+saved [B,T]: per image, bit e set = edge e of t is a silhouette edge */
    uint64_t *flags;      /* saved, fpcdr_antialias_flags_bytes(): plane 0 = pair (p, p+x) blended, plane 1 = (p, p+y) */
    float *out;           /* out [B,H,W,C] */
    const uint8_t *hint;  /* optional: region hint of rast.  Where a bin and its eight neighbours are empty no pixel pair can be
                             blended: out = color there without reading rast */
    const float *empty_color; /* optional, with hint: [C], the value of `color` in empty bins (fpcdr_texture_fwd): it is then not
                             read there either */
} fpcdr_antialias_fwd_params;
int fpcdr_antialias_fwd(const fpcdr_antialias_fwd_params *p, void *stream);

typedef struct {
    const float *color, *rast, *pos;
    const int32_t *tri, *adj;
    const float *dy;      /* [B,H,W,C] */
    int32_t B, H, W, C, V, T;
    const uint8_t *sil;   /* from the forward pass */
    const uint64_t *flags;
    float pos_gradient_boost;
    float *grad_color;    /* out [B,H,W,C] */
    float *grad_pos;      /* [B,V,4] accumulated (x, y, w) */
} fpcdr_antialias_bwd_params;
int fpcdr_antialias_bwd(const fpcdr_antialias_bwd_params *p, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* transform_clip for a minibatch                                      reference camera.py:11-23 */
/* ------------------------------------------------------------------------------------------ */

/* out[b][v] = mvp[b] . (verts[b / Nc][v], 1)      mvp [F*Nc,4,4] row-major, verts [F,V,3], out [F*Nc,V,4] */
int fpcdr_transform_clip_fwd(const float *mvp, const float *verts, float *out, int32_t F, int32_t Nc, int32_t V, void *stream);
/* grad_verts [F,V,3] (overwritten, may be NULL); grad_mvp [F*Nc,4,4] (accumulated: zero it first; may be NULL) */
int fpcdr_transform_clip_bwd(const float *mvp, const float *verts, const float *grad_out, float *grad_verts, float *grad_mvp,
                             int32_t F, int32_t Nc, int32_t V, void *stream);

/* mvp[f*Nc + c] = proj[c] . Rt(q_frame[f], t_frame[f]) . Rt(q_cam[c], t_cam[c]) . t_mv[c]      reference fit.py:541-553
 * (camera.rigid_grad, camera.py:128-132; roma.unitquat_to_rotmat on XYZW quaternions, NOT normalised, like the
 * reference after fit.py:616-618).  proj, t_mv [Nc,4,4] row-major; q [.,4]; t [.,3]; mvp [Fb*Nc,4,4].
 * bwd: the four gradient buffers are accumulated (zero them first).                                               */
int fpcdr_mvp_fwd(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                  const float *t_frame, float *mvp, int32_t Fb, int32_t Nc, void *stream);
int fpcdr_mvp_bwd(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                  const float *t_frame, const float *grad_mvp, float *gq_cam, float *gt_cam, float *gq_frame, float *gt_frame,
                  int32_t Fb, int32_t Nc, void *stream);
/* The same for a step that names its frames and views by INDEX into the full parameter tables (reference fit.py:525-526 draws one random
 * camera and frame per iteration and selects their rows with one-hot products, fit.py:547-550).  frame_idx [Fb] / view_idx [Nc]: int64 device
 * arrays or NULL (= 0 .. n - 1); view_idx indexes proj / t_mv, cam_of_view [views] (or NULL = identity) maps a view to its row of q_cam /
 * t_cam.  The backward ADDS into the full-size tables gq_cam / gt_cam / gq_frame / gt_frame (the caller zero-fills them). */
int fpcdr_mvp_fwd_indexed(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                          const float *t_frame, const int64_t *frame_idx, const int64_t *view_idx, const int64_t *cam_of_view, float *mvp,
                          int32_t Fb, int32_t Nc, void *stream);
int fpcdr_mvp_bwd_indexed(const float *proj, const float *t_mv, const float *q_cam, const float *t_cam, const float *q_frame,
                          const float *t_frame, const int64_t *frame_idx, const int64_t *view_idx, const int64_t *cam_of_view,
                          const float *grad_mvp, float *gq_cam, float *gt_cam, float *gq_frame, float *gt_frame, int32_t Fb, int32_t Nc,
                          void *stream);


/* uniform mesh Laplacian (reference fit.py:581, pytorch3d mesh_laplacian_smoothing 'uniform'), gather form:
 *   transpose = 0: out = L x,  L = D^-1 A - I;   transpose = 1: out = L^T x (the backward of the former)
 * x, out [F,V,3]; nbr [D,V] int32 one-ring table, slot-major: nbr[d][v] = d-th neighbour of v, rings stored front to
 * back and padded with indices >= V; inv_deg [V].                                                              */
int fpcdr_laplacian_gather(const float *x, const int32_t *nbr, const float *inv_deg, float *out, int32_t F, int32_t V, int32_t D,
                           int32_t transpose, void *stream);

/* The Laplacian term of the objective in two launches forward (gather + norms, then a one-workgroup finish at the kernel boundary) and one backward (reference fit.py:581 squares pytorch3d's mesh_laplacian_smoothing of
 * the ONE mesh of its step; a batch takes the mean of the squares):
 *   per[f] = mean_v || (L x_f)_v ||,   out[0] = weight / F * sum_f per[f]^2,   L = D^-1 A - I as in fpcdr_laplacian_gather.
 * lap [F,V,3] and per [F] are saved for the backward call.  acc: (F + 1) * 8 bytes, 8-byte aligned, ZERO on entry; the call leaves
 * it zero again.  Backward: grad_x [F,V,3] = upstream[0] * d out / d x (overwritten, not accumulated). */
int fpcdr_laplacian_penalty_fwd(const float *x, const int32_t *nbr, const float *inv_deg, float *lap, void *acc, float *per, float *out,
                                float weight, int32_t F, int32_t V, int32_t D, void *stream);
int fpcdr_laplacian_penalty_bwd(const float *lap, const int32_t *nbr, const float *inv_deg, const float *per, const float *upstream,
                                float *grad_x, float weight, int32_t F, int32_t V, int32_t D, void *stream);

/* The same term measured against a REST shape ("Rest Laplacian rule"): d = L x_f - rest_lap takes the place of L x_f,
 *   per[f] = mean_v || d_{f,v} ||,   out[0] = weight / F * sum_f per[f]^2;   lap [F,V,3] receives d, and fpcdr_laplacian_penalty_bwd takes
 * it unchanged.  rest_lap [V,3] = L x_rest, or NULL: the call IS fpcdr_laplacian_penalty_fwd, bit for bit -- and that is how rest_lap
 * is made (F = 1, x = x_rest, rest_lap = NULL, read `lap`): the same device code, so that d is exactly 0 at x_f = x_rest.       */
int fpcdr_laplacian_penalty_rest_fwd(const float *x, const int32_t *nbr, const float *inv_deg, const float *rest_lap /* [V,3] or NULL */,
                                     float *lap, void *acc, float *per, float *out, float weight, int32_t F, int32_t V, int32_t D,
                                     void *stream);

/* Edge lengths against their rest lengths ("Stretch rule"), value and gradient in one call (two launches):
 *   s = || x_n - x_v || - l  for every real slot d of vertex v (n = nbr[d][v]),  l = rest_len[d][v], or `target` when rest_len is NULL
 *   per[f] = 1 / (2 E) * sum_v sum_d s^2   (every edge is seen from both ends),   out[0] = weight / F * sum_f per[f]
 *   grad_x [F,V,3] = d out / d x for a unit upstream (overwritten; a slot of length 0 contributes 0), or NULL: value only.
 * rest_len [D,V] float32, slot-major, aligned entry for entry with nbr, pads 0.  E: the number of edges (sum of the degrees / 2);
 * E = 0 gives value 0 and gradient 0.  acc: (F + 1) * 8 bytes, 8-byte aligned, ZERO on entry; the call leaves it zero again.
 * With rest_len = NULL and target = 0.1 this is the reference's mesh_edge_loss(mesh, 0.1) (fit.py:580).                         */
int fpcdr_stretch_penalty(const float *x, const int32_t *nbr, const float *rest_len /* [D,V] or NULL */, float target,
                          float *grad_x /* [F,V,3] for unit upstream, or NULL: value only */, void *acc /* F+1 doubles, zero in, zero out */,
                          float *per, float *out, float weight, int32_t F, int32_t V, int32_t D, int32_t E, void *stream);

/* Dihedral angles against their rest angles ("Bend rule"), value and gradient in one call (three launches):
 *   t_h = 1 - cos(theta_h - theta_rest_h)  for every hinge h (an edge with exactly two faces),   per[f] = 1 / H * sum_h t_h,
 *   out[0] = weight / F * sum_f per[f];   a hinge with a zero-length edge or a zero-area face has t = 1 and no gradient.
 * hinge_vtx [4,H] int32, role-major: p0, p1, q0, q1; a hinge whose two faces run through the edge in the same direction stores -1 - q1.
 * rest_cs [2,H] float32 = (cos, sin) of the rest angles, or NULL: (1, 0) -- the reference's mesh_normal_consistency (fit.py:582).
 * hinge_inc [K,V] int32, slot-major: the hinge corners 4 h + role at every vertex, ascending, pads -1 trailing.
 * grad_x [F,V,3] = d out / d x for a unit upstream (overwritten), summed per vertex in slot order from hinge_grad -- caller-owned scratch
 * of F * H * 12 floats, laid out [F,4,3,H] (role, component, hinge), which the call leaves filled with the corners' gradients; no float atomics: both are
 * bit-identical from run to run.  grad_x = NULL: value only, hinge_inc and hinge_grad may be NULL.  H = 0 gives value 0 and gradient 0
 * (hinge_vtx and hinge_grad may then be NULL).  acc: (F + 1) * 8 bytes, 8-byte aligned, ZERO on entry; the call leaves it zero again. */
int fpcdr_bend_penalty(const float *x, const int32_t *hinge_vtx, const float *rest_cs /* [2,H] or NULL */, const int32_t *hinge_inc,
                       float *hinge_grad /* scratch, F*H*12 floats */, float *grad_x /* [F,V,3] for unit upstream, or NULL: value only */,
                       void *acc /* F+1 doubles, zero in, zero out */, float *per, float *out, float weight, int32_t F, int32_t V,
                       int32_t H, int32_t K, void *stream);

/* The meshes of a call held smooth in TIME ("Motion rule"), value and gradient in one call (two launches):
 *   order 2:  a_{f,v} = x_{f-1,v} - 2 x_{f,v} + x_{f+1,v},  m_f = 1 iff 1 <= f <= F - 2, t_f - t_{f-1} = 1 and t_{f+1} - t_f = 1
 *   order 1:  a_{f,v} = x_{f+1,v} - x_{f,v},                m_f = 1 iff f <= F - 2 and t_{f+1} - t_f = 1          (m_f = 0 otherwise)
 *   s = || a ||^2,   rho(s) = s  (inv_c = 0: L2)   or   2 c^2 (sqrt(1 + s / c^2) - 1),  c = 1 / inv_c  (Charbonnier, as fpcdr_robust_loss)
 *   per[f] = m_f / V * sum_v w_v rho(s_{f,v}),   out[0] = weight / F * sum_f per[f]   (divided by F, not by the number of valid stencils)
 *   grad_x [F,V,3] = d out / d x for a unit upstream (overwritten: a gather over f - order .. f + order of the entry's own vertex, no
 *   float atomics, bit-identical from run to run), or NULL: value only.
 * frame_t [F] int64, strictly increasing: the frame numbers of the meshes, read on the device; NULL: consecutive.  vertex_w [V] float32,
 * finite and >= 0, or NULL: 1.  F < order + 1, or no valid stencil: value 0, per 0, gradient 0.  An order outside {1, 2} or an inv_c that
 * is negative or not finite is an error.  acc: (F + 1) * 8 bytes, 8-byte aligned, ZERO on entry; the call leaves it zero again.     */
int fpcdr_motion_penalty(const float *x, const int64_t *frame_t /* [F] or NULL */, const float *vertex_w /* [V] or NULL */,
                         float inv_c /* 0: L2 */, int32_t order, float *grad_x /* [F,V,3] or NULL: value only */,
                         void *acc /* F+1 doubles, zero in, zero out */, float *per, float *out, float weight, int32_t F, int32_t V,
                         void *stream);

/* Named points of the mesh held to their detected 2D positions ("Landmark rule"), value and both gradients in one call
 * (three launches).  Landmark l is the point q = sum_k lm_bary[k][l] * x[f][lm_vtx[k][l]] (k = 0..2); image n = f * Nc + c (frame-major):
 *   p = mvp[n] . (q, 1),   u = (p.x / p.w * 0.5 + 0.5) * width - 0.5,   v = (p.y / p.w * 0.5 + 0.5) * height - 0.5   (raster pixels of
 *   the width x height capture: pixel centres at integers, row 0 at the bottom),   s = (u - u*)^2 + (v - v*)^2,
 *   rho(s) = s  (inv_c = 0: L2)   or   2 c^2 (sqrt(1 + s / c^2) - 1),  c = 1 / inv_c in pixels  (Charbonnier, as fpcdr_motion_penalty)
 *   per[f] = 1 / (Nc L) * sum_c sum_l lm_w[l] kappa[n][l] rho(s),   out[0] = weight / F * sum_f per[f]   (divided by the number of
 *   entries, not by the sum of the confidences).
 * An entry counts when kappa > 0, lm_w[l] > 0 and p.w > 1e-6; any other contributes exactly 0 to the value and to every gradient.
 * lm_vtx [3,L] int32 and lm_bary [3,L] float32, corner-major (a landmark at a vertex: (v, v, v) with (1, 0, 0)); lm_w [L] float32 >= 0 or
 * NULL: 1; obs [F*Nc,L,3] float32 = (u*, v*, kappa >= 0).  lm_inc [K,V] int32, slot-major: the landmark corners 3 l + k at every vertex,
 * ascending, pads -1 trailing.  The vertex ids are NOT checked on the device.
 * grad_x [F,V,3] and grad_mvp [F*Nc,4,4] = d out / d x and d out / d mvp for a unit upstream (overwritten, every entry: a vertex without
 * a landmark gets 0, row z of a matrix gets 0), NULL together: value only (scratch and lm_inc may then be NULL).  scratch: caller-owned,
 * F * Nc * L * 3 floats, left filled with d out / d q.  No float atomics: every output is bit-identical from run to run.
 * res_out [F*Nc,L,2] or NULL: (u - u*, v - v*), NaN where the entry does not count.  A negative or non-finite inv_c is an error.
 * acc: (F + 1) * 8 bytes, 8-byte aligned, ZERO on entry; the call leaves it zero again.                                         */
int fpcdr_landmark_penalty(const float *x, const float *mvp, const int32_t *lm_vtx, const float *lm_bary, const float *lm_w /* [L] or NULL */,
                           const int32_t *lm_inc, const float *obs, float inv_c /* 0: L2 */, int32_t width, int32_t height,
                           float *scratch /* F*Nc*L*3 floats */, float *grad_x /* [F,V,3] or NULL: value only */,
                           float *grad_mvp /* [F*Nc,4,4], NULL with grad_x */, float *res_out /* [F*Nc,L,2] or NULL */,
                           void *acc /* F+1 doubles, zero in, zero out */, float *per, float *out, float weight, int32_t F, int32_t Nc,
                           int32_t V, int32_t L, int32_t K, void *stream);

/* Every frame's rigid pose solved from its landmarks ("Pose solve rule"), ONE launch for all F frames, every trial inside it.
 * A pure addition: FPCDR_ABI_VERSION stays 16.  The chain is the fit's, mvp[f,c] = proj[c] . Rt(q_f, t_f) . base[c] with
 * base[c] = Rt(q_c, t_c) . MV_c . T(0,170,0) as fpcdr_mvp_fwd forms it in float32; for frame f, image c and landmark l (the tables and obs
 * of fpcdr_landmark_penalty):
 *   y = base[c] (q_l, 1) (three rows),  a = R(q_f / |q_f|) y,  z = a + t_f,  p = proj[c] (z, 1) (rows x, y, w),  u, v, live, the residual
 *   r, s = |r|^2, rho and d = rho'(s) exactly as fpcdr_landmark_penalty has them;  E_f = sum over the live entries of lm_w kappa rho(s).
 *   g_u = (width / 2) / p.w * (proj_x[0:3] - (p.x / p.w) proj_w[0:3]), g_v with height and proj_y;  J_u = (a x g_u, g_u), J_v alike: the
 *   residual's Jacobian for a left-multiplied rotation increment and a translation increment;  with w = lm_w kappa d:
 *   A = sum w (J_u^T J_u + J_v^T J_v),  b = sum w (J_u r_u + J_v r_v), summed over the frame's Nc L entries in a fixed order (no float
 *   atomics: bit-identical from run to run).
 * A trial solves (A + lambda diag A) delta = -b in float64 by Cholesky (a pivot that is not positive: a rejected trial), forms
 * q' = normalise(exp(delta_omega / 2) (x) q / |q|) and t' = t + delta_t, rounded to float32, and is accepted iff it has at least as many
 * live entries and a smaller E; then lambda <- max(lambda / 10, 1e-9), otherwise lambda <- min(10 lambda, 1e9).  `iters` trials, lambda
 * starting at lambda0.  rotation = 0: the translation block alone; q is not written.  A frame with fewer than 3 live entries at its
 * input pose, or without an accepted trial, keeps q and t bit for bit.
 * q [F,4] (XYZW) and t [F,3]: in and out.  info [F,4] = (E at the input pose, E at the returned pose, live entries at the returned pose,
 * accepted trials).  normal_out [F,28] or NULL: A's upper triangle row-major (21), b (6) and E at the INPUT pose; iters = 0 returns only
 * this (and info).  The vertex ids are NOT checked on the device.  A negative or non-finite inv_c, a lambda0 that is not finite and
 * positive, Nc * L > 2^24 are errors.                                                                                                */
int fpcdr_landmark_pose(const float *x /* [F,V,3] */, const float *proj /* [Nc,4,4] */, const float *base /* [Nc,4,4] */,
                        const int32_t *lm_vtx, const float *lm_bary, const float *lm_w /* [L] or NULL */, const float *obs /* [F*Nc,L,3] */,
                        float *q /* [F,4] */, float *t /* [F,3] */, float inv_c /* 0: L2 */, int32_t width, int32_t height, int32_t iters,
                        int32_t rotation, float lambda0, float *info /* [F,4] */, float *normal_out /* [F,28] or NULL */, int32_t F,
                        int32_t Nc, int32_t V, int32_t L, void *stream);

/* Every frame's blend weights solved from its landmarks ("Expression solve rule"), two launches for all F frames (the landmark
 * basis, then every trial of every frame).  A pure addition: FPCDR_ABI_VERSION stays 16.  The pose is fixed: mvp [F*Nc,4,4] are the step's
 * own matrices and the Landmark rule's chain p = mvp (q, 1) is used as it stands; x [F,V,3] are the meshes AT the weights w [F,Kb] (in and
 * out), basis [3V,Kb] row-major the blend basis.  A [3L,Kb] = the basis rows at the landmarks' corners, (b0 B0 + b1 B1) + b2 B2, float32.
 *   q_l(w') = q_l(x) + A_l (w' - w_in) (float32, k ascending; at w' = w_in the entry is fpcdr_landmark_penalty's to the bit);  u, v, live,
 *   the residual r, rho and d = rho'(s) as there;  E_f = sum over the live entries of lm_w kappa rho(s);  C_f = E_f + rs sum_k w_k^2
 *   (float64, k ascending) with rs = ridge Nc L.
 *   g_u = (width / 2) / p.w * (mvp_x[0:3] - (p.x / p.w) mvp_w[0:3]), g_v alike;  per landmark, in float32, over the cameras ascending with
 *   w_e = lm_w kappa d:  S_l = sum w_e (g_u g_u^T + g_v g_v^T),  s_l = sum w_e (g_u r_u + g_v r_v);  then in float64, l ascending:
 *   H = sum_l A_l^T S_l A_l (packed lower triangle, row-major: entry (i, k <= i) at i (i + 1) / 2 + k),  g = sum_l A_l^T s_l.
 * A trial factors M + lambda diag M, M = H + rs I, by right-looking Cholesky in float64 (a pivot that is not positive, or a step that is
 * not finite: a rejected trial) for the right-hand side -(g + rs w), forms w' = float32(w + delta), and is accepted iff it has at least as
 * many live entries and a smaller C; then lambda <- max(lambda / 10, 1e-9), otherwise min(10 lambda, 1e9).  A weight whose M_kk is exactly 0
 * stays bit for bit.  A frame with fewer than 3 live entries at its input, or without an accepted trial, keeps w bit for bit.
 * info [F,4] = (C at the input, C at the returned weights, live entries there, accepted trials).  normal_out or NULL: per frame
 * Kb (Kb + 1) / 2 + Kb + 2 float64 = the packed H, g, E, the live count, at the INPUT weights; iters = 0 returns only this (and info).
 * scratch: fpcdr_landmark_expr_scratch_bytes(F, L, Kb) bytes (the landmark basis: 3 L Kb floats).  Kb <= 160 and L <= 512; anything larger,
 * a negative or non-finite inv_c or ridge, a lambda0 that is not finite and positive, a misaligned buffer (4 bytes; normal_out 8) are errors
 * before any launch.  The vertex ids are NOT checked on the device.                                                                    */
size_t fpcdr_landmark_expr_scratch_bytes(int32_t F, int32_t L, int32_t Kb);
int fpcdr_landmark_expr(const float *x /* [F,V,3] */, const float *mvp /* [F*Nc,4,4] */, const float *basis /* [3V,Kb] */,
                        const int32_t *lm_vtx, const float *lm_bary, const float *lm_w /* [L] or NULL */, const float *obs /* [F*Nc,L,3] */,
                        float *w /* [F,Kb] */, float inv_c /* 0: L2 */, float ridge, int32_t width, int32_t height, int32_t iters,
                        float lambda0, float *info /* [F,4] */, double *normal_out /* or NULL */, void *scratch, size_t scratch_bytes,
                        int32_t F, int32_t Nc, int32_t V, int32_t L, int32_t Kb, void *stream);

/* The texture's prior ("Texture prior rule"), value and gradient in one call (two launches): smoothness over the pairs of
 * horizontally and vertically neighbouring texels -- none across the border -- and a hold to an anchor texture.
 *   s_pq = || t_p - t_q ||^2 over the C channels,   rho(s) = s  (inv_c = 0: L2)   or   2 s / (1 + sqrt(1 + s / c^2)),  c = 1 / inv_c
 *   part[0] = 1 / (Ht Wt) * sum_pairs min(smooth_w[p], smooth_w[q]) rho(s_pq),   part[1] = 1 / (Ht Wt) * sum_p anchor_w[p] || t_p - a_p ||^2
 *   out[0] = w_smooth * part[0] + w_anchor * part[1]
 *   grad_tex [Ht,Wt,C] = d out / d tex for a unit upstream (overwritten: every texel gathers its four neighbours, no float atomics,
 *   bit-identical from run to run), or NULL: value only.
 * tex, anchor [Ht,Wt,C] float32, C in 1..4; anchor NULL: no anchor term (part[1] = 0; anchor_w must then be NULL too).  smooth_w, anchor_w
 * [Ht,Wt] float32, finite and >= 0, or NULL: 1.  A pair whose weight is 0 and a texel whose anchor weight is 0 contribute exactly 0 to
 * value and gradient, whatever the texel holds.  A negative or non-finite inv_c or weight is an error.  acc: 2 * 8 bytes, 8-byte
 * aligned, ZERO on entry; the call leaves it zero again.                                                                        */
int fpcdr_tex_prior(const float *tex, const float *anchor /* or NULL */, const float *smooth_w /* [Ht,Wt] or NULL */,
                    const float *anchor_w /* [Ht,Wt] or NULL */, float inv_c /* 0: L2 */, float w_smooth, float w_anchor,
                    float *grad_tex /* [Ht,Wt,C] or NULL: value only */, void *acc /* 2 doubles, zero in, zero out */, float *part /* [2] */,
                    float *out, int32_t Ht, int32_t Wt, int32_t C, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* blend -- V = v_base + Bmat . w     reference fit.py:115-122 (prior), :58-62 (free)            */
/* ------------------------------------------------------------------------------------------ */

/* out[f][i] = v_base[i] + sum_k Bmat[i][k] * w[f][k]     (f32 MFMA, exact f32 accumulation)
 *   v_base [M] (may be NULL = 0), Bmat [M,K] row-major, w [F,K], out [F,M]                      */
int fpcdr_blend_fwd(const float *v_base, const float *Bmat, const float *w, float *out, int32_t M, int32_t K,
                    int32_t F, void *stream);
/* grad_w[f][k] += sum_i grad_out[f][i] * Bmat[i][k]  (accumulated: zero grad_w first)           */
int fpcdr_blend_bwd_w(const float *Bmat, const float *grad_out, float *grad_w, int32_t M, int32_t K, int32_t F,
                      void *stream);
/* The same sum with a workspace instead of float atomics (pure additions: FPCDR_ABI_VERSION stays 16): the basis is read once, per-slab
 * partial sums [slabs,F,K] go to `workspace` and are added into grad_w in a fixed order, so grad_w holds the same bits on every run.
 * grad_w is accumulated into as above (zero it first).  workspace: at least fpcdr_blend_bwd_w_workspace_bytes(M, K, F) bytes of
 * device memory, 16-byte aligned, contents irrelevant on entry and undefined afterwards.  workspace NULL, K > 224, or a Bmat,
 * grad_out or workspace that is not 16-byte aligned: the call is fpcdr_blend_bwd_w.                                              */
size_t fpcdr_blend_bwd_w_workspace_bytes(int32_t M, int32_t K, int32_t F);
int fpcdr_blend_bwd_w_ws(const float *Bmat, const float *grad_out, float *grad_w, void *workspace, size_t workspace_bytes,
                         int32_t M, int32_t K, int32_t F, void *stream);
/* grad_B[i][k] = sum_f grad_out[f][i] * w[f][k]      (free-form basis m3, reference fit.py:60; overwritten) */
int fpcdr_blend_bwd_basis(const float *w, const float *grad_out, float *grad_B, int32_t M, int32_t K, int32_t F,
                          void *stream);

/* The rig's weight algebra in front of the blend (ABI v9; reference fit.py:115-116 maps_intermediate . (maps . one-hot frame), :58-62
 * m2 . (m1 . one-hot frame)): w[fb][k] = sum_f mi[k][f] * maps[f][col(fb)], col(fb) = cols ? cols[fb] : col0 + fb -- the batch's frames
 * select columns of maps -- in the [Fb,K] layout fpcdr_blend_fwd reads.  mi [K,Fr], maps [Fr,Fc] row-major, cols [Fb] int64 or NULL.
 * bwd: grad_mi [K,Fr] and grad_maps [Fr,Fc] are OVERWRITTEN (columns no frame selects get zero); either may be NULL. */
int fpcdr_rig_weights_fwd(const float *mi, const float *maps, const int64_t *cols, int32_t col0, int32_t K, int32_t Fr, int32_t Fc,
                          int32_t Fb, float *w, void *stream);
int fpcdr_rig_weights_bwd(const float *mi, const float *maps, const int64_t *cols, int32_t col0, const float *grad_w, int32_t K,
                          int32_t Fr, int32_t Fc, int32_t Fb, float *grad_mi, float *grad_maps, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* background composite + L2 pixel loss        reference fit.py:161 and the pixel term of :579   */
/* ------------------------------------------------------------------------------------------ */

/* loss_sum += sum over pixels, channels of (ref - color_scale * c)^2, c = covered ? color : bg
 * grad_color = grad_scale * d(that sum)/d color  (0 at uncovered pixels); one pass.              */
typedef struct {
    const float *color;    /* [B,H,W,C] */
    const float *rast;     /* [B,H,W,4]; covered = rast.w > 0 */
    const uint8_t *ref;    /* [B,H,W] 8-bit reference image, broadcast over C (reference: greyscale, C = 1) */
    int32_t B, H, W, C;
    float bg;              /* background colour, reference 45/255 */
    float color_scale;     /* reference 255 */
    float grad_scale;      /* 1 / (number of elements of the global mean) */
    double *loss_sum;      /* accumulated, one f64 */
    float *grad_color;     /* out [B,H,W,C], or NULL */
} fpcdr_pixel_loss_params;
int fpcdr_pixel_loss(const fpcdr_pixel_loss_params *p, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* optimiser update        reference fit.py:493-505 (Adam, ten parameter groups), :610-618       */
/* ------------------------------------------------------------------------------------------ */

/* One Adam step (torch.optim.Adam arithmetic: betas, eps; no weight decay, no amsgrad) of up to FPCDR_ADAM_MAX_TENSORS
 * parameter tensors in ONE launch, each with its own learning rate and bias corrections (tensors that start training later
 * -- the learned basis of the combined mode, fit.py:603-608 -- count their own steps).  A tensor with `renorm` set is
 * afterwards divided by the Euclidean norm of the WHOLE tensor, the reference's quaternion "normalisation" (fit.py:616-618);
 * it may come without a gradient (grad = NULL), then only the division happens.  Everything is updated in place.          */
#define FPCDR_ADAM_MAX_TENSORS 16
typedef struct {
    float *param;          /* [n] */
    const float *grad;     /* [n], or NULL */
    float *exp_avg;        /* [n] first moment  (unused when grad is NULL) */
    float *exp_avg_sq;     /* [n] second moment */
    int64_t n;
    float step_size;       /* lr / (1 - beta1^step): the group's learning rate of this step (schedule applied by the caller) over
                              the first bias correction, divided in double precision as torch does */
    float bc2_sqrt;        /* sqrt(1 - beta2^step) */
    int32_t renorm;        /* 0: none; 1: divided by the norm of the WHOLE tensor (above); 2 (a pure addition): every row of four divided by
                              its own norm, one lane a row -- n % 4 == 0 ("Quaternion normalisation") */
    int32_t table_row;    /* ABI v10, with fpcdr_adam_params.step_table: this tensor's row of the table (step_size / bc2_sqrt above unused);
                              ABI v12, with fpcdr_adam_params.skipped: its entry of skipped_per_tensor */
    /* ABI v11, with fpcdr_adam_params.skipped: what step_size / bc2_sqrt were formed from -- the tensor's step count (this step included)
     * and its learning rate --, so that the kernel can re-form them for the steps that were not skipped */
    int32_t step;
    float lr;
} fpcdr_adam_tensor;
typedef struct {
    int32_t n_tensors;
    float beta1, beta2, eps;
    float one_minus_beta1, one_minus_beta2;   /* rounded from the double-precision differences, as torch does */
    fpcdr_adam_tensor t[FPCDR_ADAM_MAX_TENSORS];
    /* ABI v10: optional DEVICE table of (step_size, bc2_sqrt) pairs, row t[i].table_row for tensor i; when given it replaces the two fields
     * of t[] -- a step captured in a HIP graph replays fixed kernel arguments, and its learning-rate schedule and bias corrections arrive
     * through this table (one small host-to-device copy per step in front of the replay) */
    const float *step_table;
    /* ABI v11: a step whose gradients are invalid is SKIPPED ON THE DEVICE (no host read-back, no exception between two collectives):
     * skip_flag  optional DEVICE [1]; when it holds a non-zero value the launch touches neither parameters nor moments (nor the
     *            quaternion division) -- fpcdr_objective_params.skip_out, summed over the ranks
     * skipped    optional DEVICE [1] counter of the steps skipped so far, kept by this kernel (+1 per skipped launch).  The host's step
     *            counters and learning-rate schedule have moved on regardless: with *skipped = s > 0 (and no step_table) the kernel forms
     *            step_size = lr * lr_skip_gain^s / (1 - beta1_f64^(step - s_t)) and bc2_sqrt = sqrt(1 - beta2_f64^(step - s_t)) itself,
     *            in double,
     *            i.e. the update of the run that never drew the skipped steps (s_t: skipped_per_tensor below)
     * lr_skip_gain  lr(i - 1) / lr(i) of the caller's schedule (1 for a constant rate; the reference's lr_ramp^(i / max_iter) decays by
     *            a constant factor per step, fit.py:506-507)
     * ABI v12:
     * skipped_per_tensor  DEVICE [FPCDR_ADAM_MAX_TENSORS], required with `skipped`: s_t = skipped_per_tensor[t[i].table_row], the skipped
     *            launches in which tensor i HAD a gradient (the steps its host counter took and its update never did), kept by this kernel.
     *            The bias corrections come off the tensor's own count: a tensor that starts training after a skip (the learned basis of
     *            the combined mode) has step <= s, and step - s would be a zero or negative step count.  The learning rate keeps the
     *            global s: the schedule is shared by all groups.  With `skipped`, the tensors' table_rows must be distinct
     * beta1_f64, beta2_f64  required with `skipped`: the betas in double precision, as the caller's own bias corrections use them
     *            (1 - (double)0.999f is 1.3e-5 away from 1 - 0.999: the first re-formed updates would be 6e-6 off torch's) */
    const float *skip_flag;
    int32_t *skipped;
    double lr_skip_gain;
    int32_t *skipped_per_tensor;
    double beta1_f64, beta2_f64;
} fpcdr_adam_params;
int fpcdr_adam_step(const fpcdr_adam_params *p, void *stream);

/* ABI v13.  Lens undistortion of 8-bit images at ingest (reference src/undistort.py: cv2.undistort(image, intrinsic, dist) over every
 * image of a take, the new camera matrix equal to the old one).  src, dst: [n_images, H, W] uint8 on the device, different buffers;
 * image n belongs to camera n % n_cam (the [F, n_cam, H, W] layout).  cam_table: DEVICE [n_cam][9] doubles
 * fx, fy, cx, cy, k1, k2, p1, p2, k3 (OpenCV's five-coefficient model).  For the output pixel at row i FROM THE TOP, column j, in
 * unfused IEEE double ("Undistortion rule"):
 *   x = (j - cx) / fx, y = (i - cy) / fy, r2 = x x + y y, rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *   xd = x rad + ((2 p1)(x y) + p2 (r2 + 2 (x x))),  yd = y rad + (p1 (r2 + 2 (y y)) + (2 p2)(x y)),  u = fx xd + cx,  v = fy yd + cy,
 *   bilinear over the four source pixels around (v, u) with a tap outside the image = 0 (top = t00 + a (t01 - t00), bot likewise,
 *   val = top + b (bot - top)),  out = min(floor(val + 0.5), clip_max),
 * written to row i, or to row H - 1 - i when flip_rows is set.  Any H, W. */
int fpcdr_undistort_u8(const uint8_t *src, uint8_t *dst, const double *cam_table, int64_t n_images, int H, int W, int n_cam,
                       int clip_max, int flip_rows, void *stream);

/* ABI v14.  Comparison of re-rendered images with the captures (reference src/torch/comparisons.py: the per-pixel heat map of
 * compareSequence, :36-48, and the integer differences behind the row means of compareSequenceNumerical, :64-75).
 *   img       [n_images, H, W], one channel: float32 (img_is_float != 0) or uint8; device memory
 *   ref       [n_images, H, W] uint8, top row first, as on disk
 *   heat      [n_images, H, W, 3] uint8, fully overwritten; or NULL
 *   row_sums  [n_images, H] int32, ACCUMULATED with integer atomics: the caller hands it in zero-filled; or NULL (not both NULL)
 * For the output pixel at row i FROM THE TOP, column j ("Comparison rule"):
 *   r = flip_rows ? H - 1 - i : i                    (the flip applies to img only: a raster has row 0 at the bottom)
 *   q = img[n, r, j] if uint8; else x = img[n, r, j] * scale (one float32 multiply), NaN -> 0, else clip(rint(x), 0, 255), rint = round
 *       half to even
 *   d = q - ref[n, i, j],  s = max(255 - 2 |d|, 0)
 *   heat[n, i, j, :] = mode 0 (colour): d >= 0 ? (255, s, s) : (s, s, 255);  mode 1 (grey): (s, s, s)
 *   row_sums[n, i] += sum of |d| over the columns j in [col0, col1) that lie in [0, W)
 * Integers throughout: the sums are exact and do not depend on the order of the adds.  Any H, W with 255 * W below 2^31; no buffer may
 * overlap an output.  Row means, image means and the CSV text of the reference are the host's (float64(sum) / columns). */
int fpcdr_compare_u8(const void *img, int img_is_float, float scale, const uint8_t *ref, uint8_t *heat, int32_t *row_sums,
                     int64_t n_images, int H, int W, int col0, int col1, int mode, int flip_rows, void *stream);

/* ABI v15.  Overlay of re-rendered images on the captures, with the mesh's edges drawn from the rasteriser's output (reference
 * src/torch/render_result_blended.py:149-154: ref * 0.5 + img * 0.5, rounded and clipped; its wireframe variant, :58, :68-69, draws
 * the lines from a painted texture instead).
 *   img       [n_images, H, W], one channel: float32 (img_is_float != 0) or uint8; device memory
 *   ref       [n_images, H, W] uint8, top row first, as on disk
 *   rast      [n_images, H, W, 4] float32 (u, v, z/w, triangle + 1) as fpcdr_rasterize_fwd writes it, or NULL
 *   rast_db   [n_images, H, W, 4] float32 (du/dX, du/dY, dv/dX, dv/dY), or NULL; wire_hw2 > 0 needs both, outside_capture needs rast
 *   out       [n_images, H, W, 3] uint8, fully overwritten, every byte once; overlaps no input
 *   weight_256  the render's weight in 1/256, in [0, 256];  wire_hw2: squared half width of a line in pixels, finite, 0 = no wire
 *   wire_rgb  r | g << 8 | b << 16
 * For the output pixel at row i FROM THE TOP, column j ("Overlay rule"):
 *   r   = flip_rows ? H - 1 - i : i                  (the flip applies to img, rast and rast_db: a raster has row 0 at the bottom)
 *   q   = the Comparison rule's q of img[n, r, j];  c = ref[n, i, j]
 *   t   = weight_256 q + (256 - weight_256) c;  m = t / 256 rounded half to EVEN, in integers
 *   cov = rast ? rast[n, r, j, 3] > 0 : true;  if (rast && outside_capture && !cov) m = c
 *   out[n, i, j, :] = (m, m, m)
 *   if (wire_hw2 > 0 && cov):  (u, v) = rast[n, r, j, 0..1], (ux, uy, vx, vy) = rast_db[n, r, j, :], s = (1 - u) - v,
 *       b2 = s < 0 ? 0 : s, gx = ux + vx, gy = uy + vy, on(b, x, y) := b b < wire_hw2 ((x x) + (y y)) in unfused float32;
 *       if (on(u, ux, uy) || on(v, vx, vy) || on(b2, gx, gy)) out[n, i, j, :] = wire_rgb
 * rast is not read when neither a wire nor outside_capture asks for it, rast_db only for covered pixels of a call with a wire.  Any H,
 * W; float buffers 4-byte aligned (16-byte accesses where the addresses allow). */
int fpcdr_overlay_u8(const void *img, int img_is_float, float scale, const uint8_t *ref, const float *rast, const float *rast_db,
                     uint8_t *out, int64_t n_images, int H, int W, int weight_256, int outside_capture, float wire_hw2,
                     uint32_t wire_rgb, int flip_rows, void *stream);

/* ABI v16.  Gaussian-blurred L2 pixel loss for coarse-to-fine fits (the reference builds transforms.GaussianBlur(kernel_size=(31, 31))
 * at src/torch/fit.py:506 and names ref_blur / colour_blur in its preview code, :629 and :632, but wires no loss on them).  DESIGN.md 3,
 * "Blurred loss rule":
 *   e          = ref - color_scale * (rast.w > 0 ? color : bg)          per image, pixel and channel: fpcdr_pixel_loss's arithmetic
 *   E          = G_y G_x e       separable, k = 2 * radius + 1 taps per axis, each image and each channel on its own; borders REFLECTED
 *                                without repeating the edge sample (index -j -> j, n - 1 + j -> n - 1 - j: torch's mode='reflect')
 *   loss_sum  += sum E^2         one float64, accumulated with an atomic
 *   grad_color = rast.w > 0 ? (-2 * color_scale * grad_scale) * (G_x^T G_y^T E) : 0,   G^T the true adjoint of the reflecting blur
 * An uncovered pixel gets no gradient, but its residual enters E.  taps[0 .. 2 * radius] are used as given (ops.gaussian_taps: exp(-(i -
 * radius)^2 / (2 sigma^2)) in float64, normalised, rounded to float32 -- torchvision's GaussianBlur kernel as recalled; parity with
 * torchvision itself is NOT pinned by any test).  The caller owns every buffer: tmp and blurred are float planes of B * H * W * C
 * (fpcdr_blur_loss_scratch_bytes each); blurred holds E on return; grad_color may be NULL, then only the value is computed (two of the
 * four passes).  E and grad_color are accumulated in a fixed order without atomics: bit-identical from run to run.
 * Errors, before any launch: a NULL pointer, sizes <= 0, C > 4, B or H > 65535, radius outside 1 .. 31, radius > min(H, W) - 1.
 * (Declared tag-first: a struct with an embedded array, not one of the pointer-and-size blocks above.) */
typedef struct fpcdr_blur_loss_params fpcdr_blur_loss_params;
struct fpcdr_blur_loss_params {
    const float *color;    /* [B,H,W,C] */
    const float *rast;     /* [B,H,W,4]; covered = rast.w > 0 */
    const uint8_t *ref;    /* [B,H,W] 8-bit capture, broadcast over C */
    int32_t B, H, W, C;
    float bg;              /* background colour, reference 45/255 */
    float color_scale;     /* reference 255 */
    float grad_scale;      /* 1 / (number of elements of the global mean) */
    int32_t radius;        /* (kernel size - 1) / 2 */
    float taps[64];        /* taps[0 .. 2 * radius]; the rest is ignored */
    float *tmp;            /* scratch [B,H,W,C] */
    float *blurred;        /* out [B,H,W,C]: E */
    double *loss_sum;      /* accumulated, one f64 */
    float *grad_color;     /* out [B,H,W,C], or NULL */
};
size_t fpcdr_blur_loss_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
int fpcdr_blur_loss(const fpcdr_blur_loss_params *p, void *stream);

/* A start texture baked from the captures (the reference starts from uniform noise when a take has no texture, src/torch/fit.py:438).
 * Pure additions: FPCDR_ABI_VERSION stays 16, no existing entry or struct changes.  DESIGN.md 3, "Bake rule": the diagonal
 * least-squares solution of the 'linear' texture lookup's own sampling, in integers.
 *
 * fpcdr_bake_accumulate_u8:
 *   texc  [n_images, H, W, 2] float32, the interpolated texture coordinates;  rast [n_images, H, W, 4] float32, only .w is read
 *   ref   [n_images, H, W] uint8;  acc [Ht, Wt, 2] unsigned 64-bit (num, den) per texel, ACCUMULATED: the caller zero-fills it
 * For the pixel at raster row i (row 0 at the bottom), column j of image n:
 *   cov(i, j) = rast[n, i, j, 3] > 0  (a NaN is not covered);  (u, v) = texc[n, i, j, :]
 *   the pixel contributes if cov(i, j), u and v are finite and, with interior_only, cov holds at each of (i +- 1, j), (i, j +- 1)
 *   that lies inside the image
 *   c = ref[n, flip_rows ? H - 1 - i : i, j]                      (the flip applies to ref only)
 *   the four texels and the fractions fx, fy are those of the 'linear' lookup under boundary_mode (wrap or clamp), in its float32
 *   arithmetic;  ax = (int)floor(fx * 256), ay likewise, in 0..256
 *   w00 = (256 - ax)(256 - ay), w10 = ax (256 - ay), w01 = (256 - ax) ay, w11 = ax ay              (integers, sum 65536)
 *   for each tap k with w_k > 0:  acc[t_k].num += w_k c,  acc[t_k].den += w_k     (clamp: two taps may name one texel; both add)
 * Integer atomics: the sums do not depend on the order of the adds, of the calls or of the images.
 *
 * fpcdr_bake_resolve:  filled = den >= min_den;  tex = filled ? (float)((double)num / ((double)den * color_scale)) : 0
 *   tex [Ht, Wt] float32, filled [Ht, Wt] bytes 0 / 1, both fully overwritten.
 *
 * fpcdr_bake_dilate: one Jacobi pass.  An unfilled texel with a filled one among its eight neighbours inside the texture (no wrap)
 *   becomes the float32 sum of those neighbours, added in the order dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner) from 0, divided by
 *   (float)count, and is marked filled in filled_out; every other texel and mark is copied.  The pass reads tex_in / filled_in only.
 *
 * Errors, before any launch: a NULL pointer, sizes <= 0, a boundary mode other than wrap / clamp, an acc that is not 8-byte aligned,
 * min_den == 0, an output that overlaps an input.  texc and rast may sit at any 4-byte aligned address, ref at any address (wider
 * accesses are used where the addresses allow). */
int fpcdr_bake_accumulate_u8(const float *texc, const float *rast, const uint8_t *ref, uint64_t *acc, int64_t n_images, int H, int W,
                             int Ht, int Wt, int boundary_mode, int interior_only, int flip_rows, void *stream);
int fpcdr_bake_resolve(const uint64_t *acc, float *tex, uint8_t *filled, int Ht, int Wt, double color_scale, uint64_t min_den,
                       void *stream);
int fpcdr_bake_dilate(const float *tex_in, const uint8_t *filled_in, float *tex_out, uint8_t *filled_out, int Ht, int Wt, void *stream);

/* Box reduction of 8-bit images by an integer factor: the levels of a resolution pyramid of the captures.  A pure addition:
 * FPCDR_ABI_VERSION stays 16.  DESIGN.md 3, "Downsample rule".
 *   src [n_images, H, W] uint8, dst [n_images, H / s, W / s] uint8, fully overwritten
 *   S(n, i, j) = sum of src[n, i * s + a, j * s + b] over 0 <= a, b < s                      (an integer of at most 65 280)
 *   dst[n, i, j] = (2 * S + s * s) / (2 * s * s) in integer division: the exact mean, rounded half up, rounded once
 * Rows are not flipped.  Make every level from the full-size image: a cascade of reductions rounds more than once and gives other bytes.
 * Errors, before any launch: s outside 2..16, H or W not positive or not a multiple of s, n_images < 0, a NULL pointer, buffers that
 * overlap.  n_images == 0 is success without a launch.  src and dst may sit at any address (wider accesses are used where it allows). */
int fpcdr_downsample_u8(const uint8_t *src, uint8_t *dst, int64_t n_images, int H, int W, int s, void *stream);

/* Per-camera exposure from the fit's own render: the integer moments the gains are fitted from, and the 256-entry tables applied to the
 * captures in place.  Pure additions: FPCDR_ABI_VERSION stays 16, no existing entry or struct changes.  DESIGN.md 3, "Exposure rule".
 *
 * fpcdr_exposure_sums:
 *   colour [n_images, H, W, C] float32, C in 1..4;  rast [n_images, H, W, 4] float32, only .w is read;  ref [n_images, H, W] uint8
 *   mask   [n_images, H, W] uint8 or NULL;  face_w [T] float32 or NULL (then T is not read)
 *   sums   [n_images, 6] signed 64-bit (n, sum r, sum t, sum r^2, sum t^2, sum r t) per image, ACCUMULATED: the caller zero-fills it
 * For the pixel at row i, column j of image n (target row i is raster row i: nothing is flipped):
 *   cov(i, j) = rast[n, i, j, 3] > 0  (a NaN is not covered);  t = ref[n, i, j]
 *   the pixel counts iff cov(i, j), cov holds at each of (i +- 1, j), (i, j +- 1) that lies inside the image (fpcdr_bake_accumulate_u8's
 *   interior_only), mask[n, i, j] >= 128 (with a mask), face_w[id - 1] > 0 for id = (int)rast[n, i, j, 3] (with face weights; an id
 *   outside 1..T does not count and reads nothing), and lo <= t <= hi
 *   for every channel k of a pixel that counts:  r = the Comparison rule's byte of colour[n, i, j, k] * 255 (float32 product, NaN -> 0,
 *   round half to even, clip to 0..255);  sums[n] += (1, r, t, r r, t t, r t)
 * Integer atomics, one per sum and workgroup: the sums do not depend on the order of the adds, of the calls or of the images.
 * Errors, before any launch: a NULL colour / rast / ref / sums, sizes <= 0, C outside 1..4, lo / hi outside 0 <= lo <= hi <= 255, face_w
 * with T <= 0, sums not 8-byte aligned or overlapping an input.  colour, rast and face_w may sit at any 4-byte aligned address, ref and
 * mask at any address (wider accesses are used where the addresses allow).
 *
 * fpcdr_apply_lut_u8:  images[b, p] = lut[cam_of_image[b], images[b, p]] for 0 <= p < HW, in place
 *   images [n_images, HW] uint8;  lut [Nl, 256] uint8;  cam_of_image [n_images] int32 -- all DEVICE memory
 *   An image whose cam_of_image lies outside [0, Nl) is left as it is and every other image is mapped; the entry then returns
 *   FPCDR_EINVAL (it reads cam_of_image back first, so it waits for the stream and cannot be captured into a graph).
 * Errors, before any launch: a NULL pointer, HW or Nl <= 0, n_images < 0, images overlapping lut or cam_of_image.  n_images == 0 is
 * success without a launch.  images and lut may sit at any address. */
int fpcdr_exposure_sums(const float *colour, const float *rast, const uint8_t *ref, const uint8_t *mask, const float *face_w, int T,
                        int lo, int hi, int64_t n_images, int H, int W, int C, int64_t *sums, void *stream);
int fpcdr_apply_lut_u8(uint8_t *images, const uint8_t *lut, const int32_t *cam_of_image, int Nl, int64_t n_images, int64_t HW,
                       void *stream);

/* Locally normalised pixel loss: a pixel term that does not see a camera's exposure, gain or black level (the reference carries
 * whiten / normalize_highlights in utils.py and builds torch.nn.LocalResponseNorm(2) at src/torch/fit.py:510, but wires none of it
 * into its loss).  A pure addition: FPCDR_ABI_VERSION stays 16.  DESIGN.md 3, "Normalised loss rule"; taps, reflected borders and
 * the adjoint G^T are those of fpcdr_blur_loss.  Per image, pixel and channel, in float32, every operation rounded once:
 *   a  = color_scale * (rast.w > 0 ? color : bg)            t = (float)ref                    (t is the same for every channel)
 *   for x in (a, t):  mu = G x,  m = G (x * x),  v = max(m - mu * mu, 0),  s = sqrt(v + eps * eps),  n = (x - mu) / s
 *   d  = n_a - n_t                                          loss_sum += sum d^2               one float64, accumulated with an atomic
 *   p  = (2 d) / s_a,  q = (p * n_a) / s_a,  P = p - q * mu_a
 *   grad_color = rast.w > 0 ? (color_scale * grad_scale) * ((p - G^T P) - a * (G^T q)) : 0
 * An uncovered pixel gets no gradient, but its a = color_scale * bg enters the windows of its neighbours.  The caller owns every
 * buffer, in units of U = fpcdr_norm_loss_scratch_bytes(B, H, W, C) (one float per entry): tmp 4 U (scratch), stats 4 U, on return
 * (mu_a, m_a, mu_t, m_t) per entry, d 1 U, and for a gradient pq 2 U, on return (P, q) per entry, and p 1 U.  tmp and stats are 16-byte
 * aligned, pq 8-byte.  grad_color may be NULL: then only the value is computed (three of the five passes) and pq, p are not touched.
 * Every plane and grad_color are written by plain stores in a fixed order: bit-identical from run to run.
 * Errors, before any launch: a NULL pointer, sizes <= 0, C > 4, B or H > 65535, W * C >= 2^28, radius outside 1 .. 31, radius >
 * min(H, W) - 1, an eps that is not finite and > 0, a misaligned plane. */
typedef struct fpcdr_norm_loss_params fpcdr_norm_loss_params;
struct fpcdr_norm_loss_params {
    const float *color;    /* [B,H,W,C] */
    const float *rast;     /* [B,H,W,4]; covered = rast.w > 0 */
    const uint8_t *ref;    /* [B,H,W] 8-bit capture, broadcast over C */
    int32_t B, H, W, C;
    float bg;              /* background colour, reference 45/255 */
    float color_scale;     /* reference 255 */
    float grad_scale;      /* 1 / (number of elements of the global mean) */
    float eps;             /* in grey levels, finite and > 0; the project's default is 2 */
    int32_t radius;        /* (kernel size - 1) / 2 */
    float taps[64];        /* taps[0 .. 2 * radius]; the rest is ignored */
    float *tmp;            /* scratch [B,H,W,C,4] */
    float *stats;          /* out [B,H,W,C,4]: (mu_a, m_a, mu_t, m_t) */
    float *d;              /* out [B,H,W,C]: n_a - n_t */
    float *pq;             /* out [B,H,W,C,2]: (P, q); may be NULL when grad_color is */
    float *p;              /* out [B,H,W,C]; may be NULL when grad_color is */
    double *loss_sum;      /* accumulated, one f64 */
    float *grad_color;     /* out [B,H,W,C], or NULL */
};
size_t fpcdr_norm_loss_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
int fpcdr_norm_loss(const fpcdr_norm_loss_params *p, void *stream);

/* Weighted robust pixel loss: a pixel term that can be told "do not trust these pixels", "do not trust these triangles" and "large
 * residuals are outliers" (the reference's only defence is np.clip(img, 0, 140) at src/torch/fit.py:531; utils.py:12-35 carries
 * reduceHighlights / normalize_highlights and wires neither).  A pure addition: FPCDR_ABI_VERSION stays 16.  DESIGN.md 3, "Robust loss
 * rule".  Per image, pixel and channel, in float32, unfused, every operation rounded once (IEEE square root and divisions):
 *   covered = rast.w > 0        a = color_scale * (covered ? color : bg)        d = (float)ref - a        z = d * inv_c        t = z * z
 *   L2:             rho = d * d                                  s = 1
 *   CHARBONNIER:    h = sqrt(1 + t),  rho = (2 (d * d)) / (1 + h),  s = 1 / h           = 2 c^2 (sqrt(1 + d^2 / c^2) - 1), without the cancellation
 *   GEMAN_MCCLURE:  k = 1 + t,        rho = (d * d) / k,            s = 1 / (k * k)
 *   psi = d * s                                                                          = rho'(d) / 2
 *   wm  = mask ? (float)mask * float32(1 / 255) : 1;   wm = 0 where sat > 0 and ref >= sat
 *   w   = covered ? wm * (face_w ? (0 <= id - 1 < T ? face_w[id - 1] : 0) : 1) : wm * w_outside,      id = (int)rast.w
 *   sums[0] += w * rho,  sums[1] += w                 two float64, accumulated with atomics (lane float32 -> wave -> block, as fpcdr_pixel_loss)
 *   grad_color = covered ? (-2 * color_scale * grad_scale) * (w * psi) : 0
 * The weights are constants of the call.  With kind L2, no mask, no face_w, sat 0 and w_outside 1 the gradient is fpcdr_pixel_loss's bit
 * for bit.  grad_color may be NULL: then only the sums are computed.  grad_color is written by plain stores, every entry once:
 * bit-identical from run to run.  The byte buffers may sit at any address (16-byte loads are used where base and length allow), the
 * float buffers at any multiple of 4.
 * Errors, before any launch: a NULL params, color, rast, ref or sums; sizes <= 0; an unknown kind; inv_c not finite or <= 0 for a kind
 * other than L2; w_outside negative or not finite; sat outside 0 .. 255; face_w with T <= 0; a float buffer that is not 4-byte aligned
 * or sums not 8-byte aligned. */
#define FPCDR_ROBUST_L2 0
#define FPCDR_ROBUST_CHARBONNIER 1
#define FPCDR_ROBUST_GEMAN_MCCLURE 2
typedef struct fpcdr_robust_loss_params fpcdr_robust_loss_params;
struct fpcdr_robust_loss_params {
    const float *color;    /* [B,H,W,C] */
    const float *rast;     /* [B,H,W,4]; covered = rast.w > 0, rast.w = triangle id + 1 */
    const uint8_t *ref;    /* [B,H,W] 8-bit capture, broadcast over C */
    int32_t B, H, W, C;
    float bg;              /* background colour, reference 45/255 */
    float color_scale;     /* reference 255 */
    float grad_scale;      /* 1 / (number of elements of the global mean) */
    int32_t kind;          /* FPCDR_ROBUST_* */
    float inv_c;           /* float32(1 / c), c the scale in grey levels; ignored for L2 */
    float w_outside;       /* weight of uncovered pixels, finite and >= 0; 1 = as fpcdr_pixel_loss */
    int32_t sat;           /* 1 .. 255: capture pixels >= sat get weight 0; 0 = off */
    const uint8_t *mask;   /* [B,H,W] 255 = trust, 0 = ignore, or NULL */
    const float *face_w;   /* [T] one weight per triangle, finite and >= 0, or NULL */
    int32_t T;             /* entries of face_w */
    double *sums;          /* accumulated, two f64: sum of w * rho, sum of w */
    float *grad_color;     /* out [B,H,W,C], or NULL */
};
int fpcdr_robust_loss(const fpcdr_robust_loss_params *p, void *stream);

/* WEIGHTED one-pass objective: the weights and the three kinds of fpcdr_robust_loss inside the kernels of fpcdr_objective_fwd, so that a
 * fit with masks, face weights, a saturation level, weight_outside != 1 or a robust kind keeps the one-pass step (the operator path writes
 * the image, rast and the gradient planes to memory and reads them back).  Pure additions: FPCDR_ABI_VERSION stays 16, no existing entry
 * or struct changes, and the plain kernels contain none of this.  DESIGN.md 3, "Weighted objective rule".  Per pixel and channel, with
 * rho, psi, wm, w = wm * face_w[id - 1] and w0 = wm * w_outside exactly as above (d0 = ref - color_scale * bg, dd / dn the residual of the
 * un-antialiased / the blended colour, K = -2 color_scale grad_scale):
 *   covered pixel            loss_sum += w rho(dd) - w0 rho(d0)          d objective / d colour = K (w psi(dd))
 *   blended (deferred) pixel loss_sum += w rho(dn) - w rho(dd)           d objective / d antialiased colour = K (w psi(dn))
 *   value_out = (sum of loss_sum + bg_coeff * bg_sumsq[0]) / n_total,    bg_sumsq[0] = the sum over the call's images of
 *                                                                        fpcdr_ref_bg_wsum's out[i][0] (an empty pixel always shows
 *                                                                        the background: its term depends on the capture alone)
 *   wsum[slot] += C * (w - w0) over the covered pixels: the sum of all weights of the call is
 *                 sum of the FPCDR_WSUM_SLOTS slots + C * (sum over the call's images of out[i][1])
 * The weights carry no gradient; the mean's denominator stays n_total.  With kind L2, no mask, no face_w, w_outside 1 and sat 0 every
 * per-pixel term is fpcdr_objective_fwd's bit for bit.  The mask byte is read where the capture byte is, the face weight is one gather on
 * the pixel's triangle (an id past T_weights weighs 0).  Everything else -- scratch, hints, records, NaN / skip_out / counts_out on a call
 * short of record slots, count_only -- is fpcdr_objective_fwd's, through `base`.
 * Errors, before any launch: what fpcdr_objective_fwd refuses in `base`; base.mip != 0 (the mip branch has no weighted form); an unknown
 * kind; inv_c not finite or <= 0 for a kind other than L2; w_outside negative or not finite; sat outside 0 .. 255; face_w with
 * T_weights <= 0 or not 4-byte aligned; wsum NULL or not 8-byte aligned. */
#define FPCDR_WSUM_SLOTS 32
typedef struct fpcdr_objective_weighted_params fpcdr_objective_weighted_params;
struct fpcdr_objective_weighted_params
{   /* (its size is held to the ctypes mirror's by tests/test_weighted_objective_host.py) */
    fpcdr_objective_params base;
    int32_t kind;          /* FPCDR_ROBUST_* */
    float inv_c;           /* float32(1 / c); ignored for L2 */
    float w_outside;       /* weight of uncovered pixels, finite and >= 0 */
    int32_t sat;           /* 1 .. 255: capture pixels >= sat get weight 0; 0 = off */
    int32_t T_weights;     /* entries of face_w */
    const uint8_t *mask;   /* [B,H,W] 255 = trust, 0 = ignore, or NULL; any address */
    const float *face_w;   /* [T_weights] finite and >= 0, or NULL */
    double *wsum;          /* [FPCDR_WSUM_SLOTS] f64, zero-filled by the call's first kernel and accumulated by its shading kernel */
};
int fpcdr_objective_weighted_fwd(const fpcdr_objective_weighted_params *p, void *stream);

/* Per image, the all-background share of the weighted objective and of its weights: out[i][0] += sum over the px_per_image pixels of
 * image i of w0 * rho(ref - bg_scaled), out[i][1] += sum of w0, w0 = wm * w_outside with wm from the mask byte and sat as above.  ref
 * [n_images, px_per_image] uint8, mask the same or NULL, both at any address (16-byte loads where base and length allow); out
 * [n_images][2] f64, zero-filled by the caller.  Lane sums in float32 -> wave -> block -> one float64 atomic per sum and workgroup.  It
 * depends on the captures alone: a fit loop computes it once per level and kind.  Errors as fpcdr_robust_loss's for kind, inv_c,
 * w_outside and sat; NULL ref or out; counts <= 0; out not 8-byte aligned. */
int fpcdr_ref_bg_wsum(const uint8_t *ref, const uint8_t *mask, int64_t n_images, int64_t px_per_image, float bg_scaled, int32_t kind,
                      float inv_c, float w_outside, int32_t sat, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FPCDR_H */

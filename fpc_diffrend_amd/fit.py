"""
Fit loop -- host-side mirror of the reference's src/torch/fit.py, batched for MI355X.

The reference optimises ONE random (camera, frame) image per Adam step (fit.py:524-526).  Here a step
pushes `frames_per_step` frames x all selected cameras through the four raster ops as one minibatch
(nvdiffrast's own B axis, which the reference always leaves at 1, camera.py:22), and frames shard
data-parallel over ranks with ONE RCCL all-reduce of the flat gradient bucket per step
(fpc_diffrend_amd/dist.py).  Function names and argument meaning follow the reference:

    blend / blend_free / blend_combined   fit.py:103-129 / 47-62 / 66-99   (MFMA kernel behind them)
    render                                fit.py:134-162 (same signature; batched mtx / pos allowed)
    setup_dataset / setup_dataset_free    fit.py:183-230 / 166-178         (from a synthetic Scene)
    Fitter.step                           the body of the loop fit.py:524-642
    Fitter.save                           fit.py:235-286

Reference quirks are reproduced and flagged where they matter:
  Q1 the stray early `return` at fit.py:426-427 is treated as a bug (the intended loop is built);
  Q2 mesh-edge loss uses the literal target 0.1 (fit.py:580);
  Q3 quaternions are divided by the Frobenius norm of the WHOLE tensor (fit.py:616-618);
  Q5 RNG is seeded explicitly (the reference's is not);
  Q6 regularisers with weight 0 are skipped (their gradient is exactly zero either way);
  Q7 the Laplacian term enters squared (fit.py:581).
"""
import ctypes
import gc
import json
import math
import os
import time
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, camera
from . import ops as dr
from .exposure import check_exposure_options, compose, fit_gains, identity_lut, is_identity
from .landmarks import (LandmarkSet, check_expression_options, check_landmark_options, check_pose_options, landmark_incidence,
                        landmark_inv_scale, landmark_penalty, landmark_tables, project_landmarks, read_landmarks, solve_expression, solve_pose,
                        write_landmarks)
from .mesh_reg import (MeshTopology, RestShape, _check_item_weights, _uniform_laplacian, bend_penalty, check_motion_options,
                       hinge_incidence, hinge_rest_cs, hinge_vertices, laplacian_penalty, mesh_edge_loss, mesh_laplacian_smoothing,
                       mesh_normal_consistency, motion_inv_scale, motion_penalty, rest_edge_lengths, stretch_penalty)
from .ops import _ptr, _stream
from .tex_prior import chart_map, check_tex_prior_options, load_texel_weights, tex_prior_inv_scale, texture_prior

BACKGROUND = 45.0 / 255.0  # reference fit.py:161


# ----------------------------------------------------------------------------------------------
# V = v_base + Bmat . w   on the f32 matrix cores
# ----------------------------------------------------------------------------------------------

class ZeroPool:
    """Small zero-filled accumulators for the backward kernels of ONE fit step (gradients of the camera matrices, the poses, the blend
    weights: three fill launches of 5-7 us in the step's serial tail otherwise).  The Fitter makes one per step around a fresh flat
    buffer, hands that buffer to the pixel objective, whose first kernel zero-fills it (ops.pixel_objective(zero_extra=...)), and
    passes the pool itself to the functions whose backward takes views of it (blend_batched / transform_clip_batched / _mvp_func,
    argument `pool`).  No pool (None), a pool on another device, or an exhausted one: plain torch.zeros.  An object handed over
    explicitly, not module state: two Fitters in one process, or a backward run outside a step, cannot meet each other's buffer."""

    def __init__(self, buf=None):
        self.buf, self.off = buf, 0

    def zeros(self, shape, device):
        n = int(np.prod(shape))
        if self.buf is not None and self.buf.device == device and self.off + n <= self.buf.numel():
            v = self.buf[self.off:self.off + n].view(shape)
            self.off += (n + 3) // 4 * 4      # (16-byte aligned views)
            return v
        return torch.zeros(shape, dtype=torch.float32, device=device)


def _pool_zeros(pool, shape, device):
    return pool.zeros(shape, device) if pool is not None else torch.zeros(shape, dtype=torch.float32, device=device)


class _blend_func(torch.autograd.Function):
    """out[F,M] = v_base[M] + w[F,K] . Bmat[M,K]^T   (fpcdr_blend_fwd / _bwd_w / _bwd_basis)."""

    @staticmethod
    def forward(ctx, v_base, Bmat, w, pool=None):
        lib = _lib.load()
        M, K = Bmat.shape
        F = w.shape[0]
        out = torch.empty(F, M, dtype=torch.float32, device=w.device)
        _lib.call("fpcdr_blend_fwd", _ptr(v_base), _ptr(Bmat), _ptr(w), _ptr(out), M, K, F, _stream())
        ctx.save_for_backward(Bmat, w)
        ctx.pool = pool
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        Bmat, w = ctx.saved_tensors
        M, K = Bmat.shape
        F = w.shape[0]
        g = g.contiguous()
        g_vb = g.sum(dim=0) if ctx.needs_input_grad[0] else None
        g_B = None
        if ctx.needs_input_grad[1]:
            g_B = torch.empty_like(Bmat)
            _lib.call("fpcdr_blend_bwd_basis", _ptr(w), _ptr(g), _ptr(g_B), M, K, F, _stream())
        g_w = None
        if ctx.needs_input_grad[2]:
            g_w = _pool_zeros(ctx.pool, tuple(w.shape), w.device)
            # per-slab partial sums instead of float atomics (csrc/blend.hip): the workspace is scratch for this one call
            ws = torch.empty(lib.fpcdr_blend_bwd_w_workspace_bytes(M, K, F) // 4, dtype=torch.float32, device=w.device)
            _lib.call("fpcdr_blend_bwd_w_ws", _ptr(Bmat), _ptr(g), _ptr(g_w), _ptr(ws), ws.numel() * 4, M, K, F, _stream())
        return g_vb, g_B, g_w, None


class _transform_clip_func(torch.autograd.Function):
    """camera.transform_clip for a minibatch on the GPU (fpcdr_transform_clip_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, mvp, verts, pool=None):
        B, F, V = mvp.shape[0], verts.shape[0], verts.shape[1]
        out = torch.empty(B, V, 4, dtype=torch.float32, device=verts.device)
        _lib.call("fpcdr_transform_clip_fwd", _ptr(mvp), _ptr(verts), _ptr(out), F, B // F, V, _stream())
        ctx.save_for_backward(mvp, verts)
        ctx.pool = pool
        return out

    @staticmethod
    def backward(ctx, g):
        mvp, verts = ctx.saved_tensors
        B, F, V = mvp.shape[0], verts.shape[0], verts.shape[1]
        g = g.contiguous()
        g_mvp = _pool_zeros(ctx.pool, tuple(mvp.shape), mvp.device) if ctx.needs_input_grad[0] else None
        g_verts = torch.empty_like(verts) if ctx.needs_input_grad[1] else None
        _lib.call("fpcdr_transform_clip_bwd", _ptr(mvp), _ptr(verts), _ptr(g), _ptr(g_verts), _ptr(g_mvp), F, B // F, V, _stream())
        return g_mvp, g_verts, None


class _rig_weights_func(torch.autograd.Function):
    """(mi @ maps[:, ids]).t() as one launch each way (fpcdr_rig_weights_fwd / _bwd): reference fit.py:115-116 (and :58-62 with m2, m1)."""

    @staticmethod
    def forward(ctx, mi, maps, ids, validate=True):
        K, Fr = mi.shape
        Fc = maps.shape[1]
        if isinstance(ids, slice):
            lo, hi, step = ids.indices(Fc)
            assert step == 1
            cols, col0, Fb = None, lo, hi - lo
        else:
            cols, col0, Fb = ids.to(torch.int64).contiguous(), 0, int(ids.shape[0])
            # maps[:, ids] / index_select raise on an index outside [-Fc, Fc); the kernels wrap negatives and cannot raise (they write
            # NaN rows forward and no gradient backward): checked here, at the price of one host read -- callers that made the indices
            # themselves from a valid range (Fitter.pick_frames) pass validate=False
            if validate and Fb and bool(((cols < -Fc) | (cols >= Fc)).any()):
                raise IndexError(f"rig_weights: frame index out of range for {Fc} columns")
        w = torch.empty(Fb, K, dtype=torch.float32, device=mi.device)
        _lib.call("fpcdr_rig_weights_fwd", _ptr(mi), _ptr(maps), _ptr(cols), col0, K, Fr, Fc, Fb, _ptr(w), _stream())
        ctx.save_for_backward(mi, maps, *([cols] if cols is not None else []))
        ctx.geom = (col0, K, Fr, Fc, Fb, cols is not None)
        return w

    @staticmethod
    def backward(ctx, g):
        col0, K, Fr, Fc, Fb, has_cols = ctx.geom
        mi, maps = ctx.saved_tensors[:2]
        cols = ctx.saved_tensors[2] if has_cols else None
        g_mi = torch.empty_like(mi) if ctx.needs_input_grad[0] else None
        g_maps = torch.empty_like(maps) if ctx.needs_input_grad[1] else None
        _lib.call("fpcdr_rig_weights_bwd", _ptr(mi), _ptr(maps), _ptr(cols), col0, _ptr(g.contiguous()), K, Fr, Fc, Fb, _ptr(g_mi), _ptr(g_maps),
                  _stream())
        return g_mi, g_maps, None, None


def rig_weights(mi, maps, ids, validate=True):
    """(mi @ maps[:, ids]).t(), [Fb,K]: the blend weights of a batch of frames (ids: a slice or an index tensor) from the rig's two maps --
    on the GPU one launch each way instead of a GEMM, a transposing copy and, backward, two GEMMs and the slice's zero-fill + copy.
    An index tensor follows maps[:, ids]: negative entries count from the end, anything outside [-Fc, Fc) raises IndexError
    (validate=False skips that host-side check, and the read of the indices it costs, for indices known to be in range)."""
    if mi.is_cuda and mi.dtype == torch.float32 and mi.is_contiguous() and maps.is_contiguous() and \
            not (isinstance(ids, slice) and ids.step not in (None, 1)):
        return _rig_weights_func.apply(mi, maps, ids, validate)
    return torch.matmul(mi, maps[:, ids]).t()


def transform_clip_batched(mvp, verts, pool=None):
    """mvp [F*Nc,4,4], verts [F,V,3] on the GPU -> pos_clip [F*Nc,V,4]; same values as camera.transform_clip.  pool: a ZeroPool the
    backward takes its small zero-filled accumulator from."""
    assert mvp.shape[0] % verts.shape[0] == 0
    return _transform_clip_func.apply(mvp.contiguous(), verts.contiguous(), pool)


def blend_batched(v_base, Bmat, w, pool=None):
    """v_base [M], Bmat [M,K], w [F,K] -> [F,M] on the GPU matrix cores (pool: see transform_clip_batched)."""
    return _blend_func.apply(v_base.contiguous() if v_base is not None else None, Bmat.contiguous(), w.contiguous(), pool)


def _frame_matrix(frames):
    """Reference passes a one-hot vector [F] (fit.py:536); a batch is a matrix of one-hot columns [F,Fb]."""
    return frames if frames.dim() == 2 else frames[:, None]


def blend(v_base, maps, maps_intermediate, dataset, frames):
    """Rig equation, reference fit.py:103-129.  frames: one-hot [F] or one-hot columns [F,Fb]."""
    fm = _frame_matrix(frames)
    mapped = torch.matmul(maps['local'], fm)
    if 'global' not in dataset:
        mapped = torch.matmul(maps_intermediate['local'], mapped)
    out = blend_batched(v_base, dataset['local'], mapped.t())
    return out[0] if frames.dim() == 1 else out


def blend_free(v_base, m1, m2, m3, frames):
    """Learned basis, reference fit.py:47-62."""
    fm = _frame_matrix(frames)
    basis = torch.matmul(m2, torch.matmul(m1, fm))
    out = blend_batched(v_base, m3, basis.t())
    return out[0] if frames.dim() == 1 else out


def blend_combined(v_base, m1, m2, m3, maps, maps_intermediate, datasets, frames, learned_coefficient=1.0):
    """Rig prior + learned correctives, reference fit.py:66-99."""
    fm = _frame_matrix(frames)
    mi = torch.matmul(maps_intermediate['local'], torch.matmul(maps['local'], fm))
    basis = torch.matmul(m2, torch.matmul(m1, fm))
    out = blend_batched(v_base, datasets['local'], mi.t())
    out = out + learned_coefficient * blend_batched(None, m3, basis.t())
    return out[0] if frames.dim() == 1 else out


# ----------------------------------------------------------------------------------------------
# render -- reference fit.py:134-162
# ----------------------------------------------------------------------------------------------

def render_layers(glctx, mtx, pos, pos_idx, uv, uv_idx, tex, resolution, enable_mip, max_mip_level, fused=False):
    """The op chain of reference render() up to and including antialias; returns (colour, rast_out)."""
    pos_clip = camera.transform_clip(mtx, pos)
    return render_from_clip(glctx, pos_clip, pos_idx, uv, uv_idx, tex, resolution, enable_mip, max_mip_level, fused)


def render_from_clip(glctx, pos_clip, pos_idx, uv, uv_idx, tex, resolution, enable_mip, max_mip_level, fused=False):
    """reference fit.py:151-160 (rasterize -> interpolate -> texture -> antialias) on given clip-space positions.
    fused=True (non-mip only) runs the first three as one kernel pair (ops.render_textured): same values."""
    if fused and not enable_mip:
        colour, rast_out = dr.render_textured(glctx, pos_clip, pos_idx, uv, uv_idx, tex, resolution)
        colour = dr.antialias(colour, rast_out, pos_clip, pos_idx)
        return colour, rast_out
    rast_out, rast_out_db = dr.rasterize(glctx, pos_clip, pos_idx, resolution=(resolution[0], resolution[1]))
    if enable_mip:
        texc, texd = dr.interpolate(uv[None, ...], rast_out, uv_idx, rast_db=rast_out_db, diff_attrs='all')
        colour = dr.texture(tex[None, ...], texc, texd, filter_mode='linear-mipmap-linear', max_mip_level=max_mip_level)
    else:
        texc, _ = dr.interpolate(uv[None, ...], rast_out, uv_idx)
        colour = dr.texture(tex[None, ...], texc, filter_mode='linear')
    colour = dr.antialias(colour, rast_out, pos_clip, pos_idx)
    return colour, rast_out


def render(glctx, mtx, pos, pos_idx, uv, uv_idx, tex, resolution, enable_mip, max_mip_level):
    """Same signature as the reference's render() (fit.py:134).  mtx [4,4] + pos [V,3] returns [H,W,C]
    like the reference; mtx [B,4,4] (+ pos [F,V,3]) returns the whole minibatch [B,H,W,C]."""
    colour, rast_out = render_layers(glctx, mtx, pos, pos_idx, uv, uv_idx, tex, resolution, enable_mip, max_mip_level)
    colour = torch.where(rast_out[..., 3:] > 0, colour, torch.tensor(BACKGROUND, device=colour.device))
    single = (not isinstance(mtx, np.ndarray) and mtx.dim() == 2) or (isinstance(mtx, np.ndarray) and mtx.ndim == 2)
    return colour[0] if single else colour


def pixel_loss_fused(colour, rast_out, ref_u8, n_total=None):
    """Background composite (fit.py:161) + sum((ref - 255 colour)^2) (fit.py:579) and its gradient in one
    pass (ops.pixel_loss_call).  Returns (sum_sq [1] f64 tensor, d mean / d colour [B,H,W,C]) with mean over n_total elements."""
    n_total = n_total or colour.numel()
    return dr.pixel_loss_call(colour, rast_out, ref_u8, 1.0 / n_total, BACKGROUND)


def pixel_loss_blurred(colour, rast_out, ref_u8, taps, n_total=None):
    """pixel_loss_fused with the residual Gaussian-blurred before it is squared ("Blurred loss rule"; fpcdr_blur_loss):
    returns (sum E^2 [1] f64 tensor, d mean / d colour [B,H,W,C]) with mean over n_total elements."""
    n_total = n_total or colour.numel()
    acc, grad, _ = dr.blur_loss_call(colour, rast_out, ref_u8, taps, 1.0 / n_total, BACKGROUND)
    return acc, grad


def pixel_loss_normalised(colour, rast_out, ref_u8, taps, eps, n_total=None):
    """pixel_loss_fused with render and capture each normalised by its own Gaussian window before they are compared (DESIGN.md 3,
    "Normalised loss rule"; fpcdr_norm_loss): returns (sum d^2 [1] f64 tensor, d mean / d colour [B,H,W,C]) with mean over n_total elements."""
    n_total = n_total or colour.numel()
    acc, grad, _ = dr.norm_loss_call(colour, rast_out, ref_u8, taps, 1.0 / n_total, eps, True, BACKGROUND)
    return acc, grad


def pixel_loss_robust(colour, rast_out, ref_u8, kind, scale, n_total=None, mask=None, face_weights=None, weight_outside=1.0, saturation=0):
    """pixel_loss_fused with every residual passed through the robust function `kind` ('l2' | 'charbonnier' | 'geman_mcclure', scale c in
    grey levels) and weighted by the mask byte, the face weight of its triangle, weight_outside off the mesh and 0 from `saturation` on
    ("Robust loss rule"; fpcdr_robust_loss): returns (sums [2] f64 tensor = (sum of w * rho, sum of w), d mean / d colour
    [B,H,W,C]) with mean over n_total elements -- not over the sum of the weights."""
    n_total = n_total or colour.numel()
    return dr.robust_loss_call(colour, rast_out, ref_u8, kind, scale, 1.0 / n_total, mask=mask, face_weights=face_weights,
                               weight_outside=weight_outside, saturation=saturation, background=BACKGROUND, check_weights=False)


def _load_weights(weights, n, option, item):
    """FitConfig.<option> -- an array-like [n] or the path of a text file with one number per <item> -- as a float32 array [n], or
    ValueError: another length, an entry that is not finite or is negative (mesh_reg._check_item_weights)."""
    if isinstance(weights, (str, os.PathLike)):
        try:
            w = np.loadtxt(weights, dtype=np.float64, ndmin=1)
        except (OSError, ValueError) as e:
            raise ValueError(f"FitConfig.{option}: cannot read {weights}: {e}")
    else:
        w = np.asarray(weights, dtype=np.float64)
    return _check_item_weights(w, (n,), option, item)


def load_face_weights(face_weights, n_faces):
    """FitConfig.face_weights -- an array-like [T] or the path of a text file with one number per face -- as a float32 array [T], or
    ValueError: another length than the mesh has faces, an entry that is not finite or is negative."""
    return _load_weights(face_weights, n_faces, 'face_weights', 'face')


def load_motion_vertex_weights(vertex_weights, n_vertices):
    """FitConfig.motion_vertex_weights -- an array-like [V] or the path of a text file with one number per vertex, read as
    load_face_weights reads its file -- as a float32 array [V], or ValueError."""
    return _load_weights(vertex_weights, n_vertices, 'motion_vertex_weights', 'vertex')


def motion_options(cfg, n_vertices, n_local):
    """What FitConfig.weight_motion > 0 asks of the other options, of the mesh (n_vertices) and of a rank's shard (n_local frames), or
    ValueError; -> (inv_c: the float32 inverse of motion_scale, 0.0 without one; the vertex weights as a float32 array [V], or None)."""
    need = cfg.motion_order + 1
    if n_local < need:
        raise ValueError(f"FitConfig.weight_motion > 0 with motion_order={cfg.motion_order} needs at least {need} frames in a rank's shard "
                         f"(this one has {n_local}): the stencils end at the shard's borders")
    w = None if cfg.motion_vertex_weights is None else load_motion_vertex_weights(cfg.motion_vertex_weights, n_vertices)
    return motion_inv_scale(cfg.motion_scale), w


class PriorTerm:
    """One term a fit step evaluates in front of the pixel objective, stated once (the table of Fitter._build_prior_terms): the public
    penalty fn(*args, *weights, **kw) with (args, kw) = inputs(vtx, ids) -- vtx [Fb,V,3] the step's meshes, ids their frame numbers (None:
    consecutive, else the sorted int64 device tensor) -- and one log key per weight.  The Fitter evaluates it in two forms:
      term(vtx, ids) -> scalar     the step's: weights / world (the gradients are summed over the ranks) and the keywords `step` of the
                                   eager hand-over: the gradient is made with the value, d loss / d term = 1 exactly;
      term.log(vtx, ids) -> dict   the log's: per key the value with that weight alone, at its full size (0.0 and no launch for a
                                   weight of 0): a fresh accumulator, and no gradient under the caller's torch.no_grad()."""

    def __init__(self, fn, inputs, weights, keys, world, **step):
        self.fn, self.inputs, self.weights, self.keys, self.step = fn, inputs, tuple(weights), tuple(keys), step
        self.shares = tuple(w / world for w in self.weights)

    def __call__(self, vtx, ids):
        args, kw = self.inputs(vtx, ids)
        return self.fn(*args, *self.shares, **kw, **self.step)

    def log(self, vtx, ids):
        args, kw = self.inputs(vtx, ids)
        alone = lambda j: (w if k == j else 0.0 for k, w in enumerate(self.weights))
        return {key: float(self.fn(*args, *alone(j), **kw)) if self.weights[j] else 0.0 for j, key in enumerate(self.keys)}


def pixel_term(cfg, i, weighted=False):
    """The pixel term of iteration i under FitConfig cfg ("Which pixel term an iteration runs"), a function of the iteration
    alone, so that a resumed run continues on the right side of every switch.  weighted: masks in use, face weights, saturation > 0 or
    weight_outside != 1.  ->  None: the path the other flags select;  ('blur', taps);  ('norm', taps, norm_eps);  ('robust', kind,
    scale): cfg.robust inside robust_iters, ('robust', 'l2', None) when only weights are on.  The name and the arguments that
    pixel_loss_blurred / _normalised / _robust take between ref_u8 and n_total.  Needs no GPU."""
    for kind in ('blur', 'norm'):
        sigma, iters = float(getattr(cfg, kind + '_sigma')), getattr(cfg, kind + '_iters')
        if sigma > 0 and not (iters and i >= iters):
            if kind == 'blur' and cfg.blur_sigma_end is not None:      # geometrically from blur_sigma to blur_sigma_end
                n = iters or cfg.max_iter
                sigma = sigma * (float(cfg.blur_sigma_end) / sigma) ** (min(i, n - 1) / max(n - 1, 1))
            taps = dr.gaussian_taps(getattr(cfg, kind + '_kernel_size'), sigma)
            return ('blur', taps) if kind == 'blur' else ('norm', taps, cfg.norm_eps)
    if cfg.robust and not (cfg.robust_iters and i >= cfg.robust_iters):
        return 'robust', cfg.robust, cfg.robust_scale
    return ('robust', 'l2', None) if weighted else None


def step_path(cfg, term, mip, channels=1):
    """Which of its four forms a step runs under FitConfig cfg when its pixel term is `term` (pixel_term's answer), the active level's
    enable_mip is `mip` and the texture has `channels` ("Which pixel term an iteration runs") -> (form, weighted):
      'one_pass'   ops.pixel_objective, value and gradient from one call: fused_objective, fused_render, fused_loss, texture shading with
                   1, 3 or 4 channels, one_pass and sparse_objective, and no term of its own -- or, weighted = True, the robust term
                   under cfg.weighted_one_pass on a level without mip ("Weighted objective rule"; a pyramid level under
                   pyramid_mip, the cheap levels, stays on the operator path);
      'two_call'   ops.pixel_objective's two-call form: the same flags without one_pass or without sparse_objective (mip needs the
                   latter), and no term of its own: a windowed or weighted loss needs the image in memory;
      'operators'  render_from_clip or render_vertex and the fused pixel term (pixel_term_loss): fused_loss otherwise;
      'torch'      the reference's torch loss on the operators' image: fused_loss=False.
    Needs no GPU."""
    objective = bool(cfg.fused_objective and cfg.fused_render and cfg.fused_loss and cfg.shading == 'texture' and channels in (1, 3, 4))
    if objective and cfg.one_pass and cfg.sparse_objective:
        weighted = bool(cfg.weighted_one_pass and term is not None and term[0] == 'robust' and not mip)
        if term is None or weighted:
            return 'one_pass', weighted
    elif objective and term is None and (not mip or cfg.sparse_objective):
        return 'two_call', False
    return ('operators' if cfg.fused_loss else 'torch'), False


def weighted_one_pass_term(cfg, term, mip, channels=1):
    """Whether an iteration whose pixel term is `term` runs the WEIGHTED one-pass objective (ops.pixel_objective with weights) instead of
    render_from_clip + pixel_loss_robust: step_path's second answer.  Needs no GPU."""
    return step_path(cfg, term, mip, channels)[1]


def pixel_term_loss(term, colour, rast_out, ref_u8, n_total, **weights):
    """(sums f64, d mean / d colour) of `term` (pixel_term's answer; None: the plain L2); weights: pixel_loss_robust's keyword arguments."""
    if term is None:
        return pixel_loss_fused(colour, rast_out, ref_u8, n_total)
    call = {'blur': pixel_loss_blurred, 'norm': pixel_loss_normalised, 'robust': pixel_loss_robust}[term[0]]
    return call(colour, rast_out, ref_u8, *term[1:], n_total, **weights)


def check_pixel_terms(cfg, has_masks=False):
    """What a windowed (blur_sigma > 0, norm_sigma > 0) or a weighted pixel term (FitConfig.weights_configured(), or has_masks: the Scene
    has masks, and use_masks takes them) asks of the other options, or ValueError.  FitConfig itself refuses what it can see without a
    Scene; this is the whole statement once the Scene is known.  Needs no GPU."""
    weights = "robust / face_weights / saturation / weight_outside" if cfg.weights_configured() else \
        "the Scene's masks (use_masks=False ignores them)" if (has_masks and cfg.use_masks) else None
    windows = [kind for kind in ('blur', 'norm') if getattr(cfg, kind + '_sigma') > 0]
    for what, loss in [(k + "_sigma > 0", {'blur': "blurred", 'norm': "normalised"}[k]) for k in windows] + [(weights, "robust")] * bool(weights):
        if not cfg.fused_loss:
            raise ValueError(f"FitConfig: {what} needs fused_loss=True: the {loss} loss replaces pixel_loss_fused")
        if cfg.hip_graph:      # ('auto' counts as on)
            raise ValueError(f"FitConfig: {what} cannot be combined with hip_graph: the term, and with it the step's launches, changes from "
                             "one iteration to the next, and the step leaves the captured path")
    for kind in windows:      # (raises for a bad kernel size or sigma)
        dr.gaussian_taps(getattr(cfg, kind + '_kernel_size'), getattr(cfg, kind + '_sigma'))
        if kind == 'blur' and cfg.blur_sigma_end is not None:
            dr.gaussian_taps(cfg.blur_kernel_size, cfg.blur_sigma_end)
    if 'norm' in windows and not (float(cfg.norm_eps) > 0.0 and float(cfg.norm_eps) < float('inf')):
        raise ValueError(f"FitConfig.norm_eps must be finite and positive (got {cfg.norm_eps})")
    if windows and weights:
        raise ValueError(f"FitConfig: {weights} cannot be combined with blur_sigma > 0 or norm_sigma > 0: weighting the windowed losses "
                         "is a different rule")


class _mvp_func(torch.autograd.Function):
    """Model-view-projection matrices of a minibatch in one kernel each way.  Without index tensors (fpcdr_mvp_fwd / _bwd): every row of
    q_frame / t_frame is a frame of the step, every row of q_cam / t_cam a view, Fb and Nc are the table shapes.  With any of them
    (fpcdr_mvp_fwd_indexed / _bwd_indexed) the step names its Fb frames / Nc views by index into the FULL parameter tables: no
    index_select launches in front, no zero-fill + index_add pairs behind.  frame_idx [Fb] / view_idx [Nc]: int64 device tensors or None;
    cam_of_view: the Fitter's cam_sel (view -> row of q_cam / t_cam) or None."""

    @staticmethod
    def forward(ctx, q_cam, t_cam, q_frame, t_frame, proj, t_mv, frame_idx=None, view_idx=None, cam_of_view=None, Fb=None, Nc=None, pool=None):
        ctx.pool = pool
        q_cam, t_cam, q_frame, t_frame = (a.contiguous() for a in (q_cam, t_cam, q_frame, t_frame))
        idx = (frame_idx, view_idx, cam_of_view)
        ctx.have = tuple(t is not None for t in idx)
        if not any(ctx.have):
            Fb, Nc = q_frame.shape[0], q_cam.shape[0]
        ctx.dims = (Fb, Nc)
        out = torch.empty(Fb * Nc, 4, 4, dtype=torch.float32, device=q_cam.device)
        tables = (_ptr(proj), _ptr(t_mv), _ptr(q_cam), _ptr(t_cam), _ptr(q_frame), _ptr(t_frame))
        if any(ctx.have):
            _lib.call("fpcdr_mvp_fwd_indexed", *tables, *(_ptr(t) for t in idx), _ptr(out), Fb, Nc, _stream())
        else:
            _lib.call("fpcdr_mvp_fwd", *tables, _ptr(out), Fb, Nc, _stream())
        ctx.save_for_backward(q_cam, t_cam, q_frame, t_frame, proj, t_mv, *(t for t in idx if t is not None))
        return out

    @staticmethod
    def backward(ctx, g):
        q_cam, t_cam, q_frame, t_frame, proj, t_mv = ctx.saved_tensors[:6]
        rest = list(ctx.saved_tensors[6:])
        idx = [rest.pop(0) if h else None for h in ctx.have]
        Fb, Nc = ctx.dims
        nq, nf = q_cam.shape[0], q_frame.shape[0]      # the gradients cover the whole tables (without index tensors: Nc and Fb rows)
        grads = _pool_zeros(ctx.pool, (7 * (nq + nf),), g.device)
        gq_cam, gt_cam = grads[:4 * nq].view(nq, 4), grads[4 * nq:7 * nq].view(nq, 3)
        gq_frame, gt_frame = grads[7 * nq:7 * nq + 4 * nf].view(nf, 4), grads[7 * nq + 4 * nf:].view(nf, 3)
        tables = (_ptr(proj), _ptr(t_mv), _ptr(q_cam), _ptr(t_cam), _ptr(q_frame), _ptr(t_frame))
        outs = (_ptr(gq_cam), _ptr(gt_cam), _ptr(gq_frame), _ptr(gt_frame), Fb, Nc, _stream())
        if any(ctx.have):
            _lib.call("fpcdr_mvp_bwd_indexed", *tables, *(_ptr(t) for t in idx), _ptr(g.contiguous()), *outs)
        else:
            _lib.call("fpcdr_mvp_bwd", *tables, _ptr(g.contiguous()), *outs)
        return (gq_cam, gt_cam, gq_frame, gt_frame) + (None,) * 8


_mvp_indexed_func = _mvp_func      # (the name under which the tests call it with index tensors)


# ----------------------------------------------------------------------------------------------
# configuration / parameters
# ----------------------------------------------------------------------------------------------

class GroupedAdam(torch.optim.Optimizer):
    """torch.optim.Adam's update (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad) for all parameter groups in ONE
    launch of `fpcdr_adam_step`, the whole-tensor quaternion division of the reference's loop folded in (reference
    fit.py:493-505 ten groups with their own learning rates, :610-618 step + division).  torch's fused Adam launches twice
    per group, and the two divisions are four small launches each: two dozen ~5 us launches in the serial tail of a 5 ms
    step.  State layout and names are torch.optim.Adam's ('step', 'exp_avg', 'exp_avg_sq'), so LambdaLR, state_dict() and
    checkpoints work unchanged (the update is the same formula evaluated in a slightly different order -- step_size * (m / denom) --
    so a run with grouped_adam on and one with it off agree to a few ulps per step, not bit for bit).  `renorm` = the parameters
    divided by their whole-tensor norm after every step; renorm_rows: every row of four of them by its own norm instead
    (fpcdr_adam_tensor.renorm = 2; FitConfig.quat_renorm='rows')."""

    def __init__(self, groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, renorm=(), capturable=False, renorm_rows=False):
        super().__init__(groups, dict(lr=lr, betas=betas, eps=eps))
        self._renorm = {id(p) for p in renorm}
        self._renorm_kind = 2 if renorm_rows else 1
        assert not renorm_rows or all(p.numel() % 4 == 0 for p in renorm), "renorm_rows: the tensors hold quaternions"
        n = sum(len(g['params']) for g in self.param_groups)
        assert n <= _lib.ADAM_MAX_TENSORS, "more parameter tensors than one fpcdr_adam_step call takes"
        # capturable: the launch may be captured in a HIP graph.  Its per-tensor (step_size, bc2_sqrt) then come from a device table
        # that prepare() fills before every replay -- the step counters advance there, on the host, and step() leaves them alone
        self.capturable = bool(capturable)
        self._table_host = self._table_dev = None
        self._ring, self._ring_i = [], 0
        # steps skipped on the device (fpcdr_adam_params.skip_flag / skipped / skipped_per_tensor, include/fpcdr.h ABI v11, v12): `skip_flag`
        # is a one-element float32 device tensor the launch reads -- non-zero: this step's gradients are invalid, touch nothing --, set by
        # the caller before every step() (None: never skip); `skipped` the device counter of skipped steps the kernel keeps, and
        # `skipped_per_tensor` its count per tensor (by position in the optimiser, _rows) of the skipped steps in which that tensor had a
        # gradient: those its state['step'] counted and its update never took; `lr_skip_gain` = lr(i - 1) / lr(i) of the schedule.  (The
        # counters stay out of self.state: it holds torch.optim.Adam's keys only)
        self.skip_flag = None
        self.skipped = None
        self.skipped_per_tensor = None
        self.lr_skip_gain = 1.0

    def enable_skips(self, lr_skip_gain=1.0):
        """Allocate the device counters of skipped steps (see __init__); returns the global one."""
        if self.skipped is None:
            dev = self.param_groups[0]['params'][0].device
            self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
            self.skipped_per_tensor = torch.zeros(_lib.ADAM_MAX_TENSORS, dtype=torch.int32, device=dev)
        self.lr_skip_gain = float(lr_skip_gain)
        return self.skipped

    def _rows(self):
        """(group, parameter, row of the device table) of EVERY parameter: a parameter's row is its position in the optimiser, whatever
        gradients exist at the moment (prepare() runs in front of the backward pass, step() behind it)."""
        out = []
        for g in self.param_groups:
            for p in g['params']:
                out.append((g, p, len(out)))
        return out

    @torch.no_grad()
    def prepare(self, host_out=None):
        """capturable mode, once per step IN FRONT of the (captured or eager) launch: advance the step counters and write the
        per-tensor (step_size, bc2_sqrt) -- with the learning rates the scheduler has set by now -- into the device table.  host_out: a
        pinned float32 view of at least 2 * ADAM_MAX_TENSORS values that the CALLER copies to table_dev() itself (a fit step packs it
        with its other per-step inputs into one copy); default: an own pinned buffer and an own asynchronous copy.
        A parameter counts a step when it is trainable NOW (requires_grad): in this mode the call comes before the backward pass, so
        "has a gradient" -- torch.optim.Adam's rule, and step()'s in the plain mode -- is not known yet; the fit loop's trainable
        parameters all receive one every step."""
        assert self.capturable
        self.table_dev()
        if host_out is None:
            # (the copy below reads the pinned buffer when the GPU gets to it: a ring of buffers, each guarded by the event of its last copy,
            #  so that a host running several steps ahead never rewrites a table that is still waiting to be copied)
            if not self._ring:
                self._ring = [[torch.zeros(2 * _lib.ADAM_MAX_TENSORS, dtype=torch.float32).pin_memory(), None] for _ in range(4)]
            slot = self._ring[self._ring_i % len(self._ring)]
            self._ring_i += 1
            if slot[1] is not None:
                slot[1].synchronize()
            self._table_host = slot[0]
        host = self._table_host if host_out is None else host_out
        for g, p, k in self._rows():
            host[2 * k], host[2 * k + 1] = 0.0, 1.0
            if p.requires_grad:
                b1, b2 = g['betas']
                st = self._state_of(p)
                st['step'] += 1
                n_step = float(st['step'])
                host[2 * k] = float(g['lr']) / (1.0 - b1 ** n_step)
                host[2 * k + 1] = math.sqrt(1.0 - b2 ** n_step)
        if host_out is None:
            self._table_dev.copy_(self._table_host, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()

    def set_table_dev(self, view):
        """Use `view` (a float32 device tensor of 2 * ADAM_MAX_TENSORS values) as the table: a caller that copies it together with its own
        per-step inputs (Fitter, graph mode) hands prepare() the matching host view and does the copy itself."""
        assert view.dtype == torch.float32 and view.numel() >= 2 * _lib.ADAM_MAX_TENSORS and view.is_contiguous()
        self._table_dev = view

    def table_dev(self):
        if self._table_dev is None:
            dev = self.param_groups[0]['params'][0].device
            self._table_dev = torch.zeros(2 * _lib.ADAM_MAX_TENSORS, dtype=torch.float32, device=dev)
        return self._table_dev

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st['step'] = torch.zeros((), dtype=torch.float32)
            st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if st['step'].is_cuda:      # (a checkpoint written by torch.optim.Adam(fused=True) keeps its counters on the GPU:
            st['step'] = st['step'].cpu()      # one copy here instead of a host sync per tensor and step)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        P = _lib.AdamParams()
        k = 0
        keep = []
        row = -1
        if self.capturable:
            P.step_table = self.table_dev().data_ptr()
        if self.skip_flag is not None:
            assert self.skip_flag.dtype == torch.float32 and self.skip_flag.is_cuda and self.skip_flag.numel() >= 1
            P.skip_flag = self.skip_flag.data_ptr()
            keep.append(self.skip_flag)
            if self.skipped is not None:
                P.skipped, P.lr_skip_gain = self.skipped.data_ptr(), self.lr_skip_gain
                P.skipped_per_tensor = self.skipped_per_tensor.data_ptr()
        for g in self.param_groups:
            b1, b2 = g['betas']
            assert (b1, b2, g['eps']) == (self.param_groups[0]['betas'] + (self.param_groups[0]['eps'],)), \
                "one launch takes one (betas, eps) for all groups"
            P.beta1, P.beta2, P.eps, P.one_minus_beta1, P.one_minus_beta2 = b1, b2, g['eps'], 1.0 - b1, 1.0 - b2
            P.beta1_f64, P.beta2_f64 = b1, b2
            for p in g['params']:
                row += 1
                ren = id(p) in self._renorm
                if p.grad is None and self.capturable and p.requires_grad:
                    # prepare() counted a step for this tensor in front of the backward pass (it cannot know which gradients will exist):
                    # a trainable tensor without one would leave its bias corrections ahead of torch.optim.Adam's
                    raise RuntimeError("GroupedAdam(capturable=True): a trainable parameter received no gradient this step "
                                       f"(tensor {row} of the optimiser, shape {tuple(p.shape)})")
                if p.grad is None and not ren:
                    continue
                assert p.is_contiguous() and p.dtype == torch.float32
                t = P.t[k]
                t.param, t.n, t.renorm, t.table_row = p.data_ptr(), p.numel(), self._renorm_kind if ren else 0, row
                t.step_size, t.bc2_sqrt = 0.0, 1.0
                if p.grad is not None:
                    st = self._state_of(p)
                    grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    keep.append(grad)
                    t.grad, t.exp_avg, t.exp_avg_sq = grad.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr()
                    if not self.capturable:      # (capturable: prepare() advanced the counter and filled the device table)
                        st['step'] += 1
                        n_step = float(st['step'])
                        t.step_size, t.bc2_sqrt = float(g['lr']) / (1.0 - b1 ** n_step), math.sqrt(1.0 - b2 ** n_step)
                    t.step, t.lr = int(st['step']), float(g['lr'])
                k += 1
        P.n_tensors = k
        _lib.call("fpcdr_adam_step", ctypes.byref(P), _stream())
        return None


@dataclass
class FitConfig:
    """Keyword arguments of the reference's fitTake (fit.py:323-357) that act on the live loop, with the
    values of its main.py:13-47 as defaults; unused reference kwargs are left out."""
    max_iter: int = 80000
    lr_base: float = 10e-4
    lr_tex_coef: float = 0.5
    lr_ramp: float = 0.005
    lr_t: float = 10e-6
    lr_q: float = 10e-6
    enable_mip: bool = False
    max_mip_level: int = 6
    resolution: Optional[Sequence[int]] = None     # (H, W); default: the scene's.  On a take from disk (scene.from_take) a size that is the
                                                   # images' divided by one integer factor in 2..16 fits at that size: the captures are
                                                   # reduced once, at construction (ops.downsample_images)
    weight_laplacian: float = 5000.0
    weight_meshedge: float = 0.0
    weight_normalconsistency: float = 0.0
    laplacian_relative: bool = False    # the Laplacian term measures against the base mesh's own differentials, || L x - L v_base || in
                                    # place of || L x || ("Rest Laplacian rule"; the reference's unwired
                                    # laplacian_regularization, fit.py:292-319): zero, with a zero gradient, at the base mesh, where the
                                    # plain term pulls towards a flat blob.  Existing weights carry over.  False: nothing changes
    weight_stretch: float = 0.0     # > 0: every edge is held to its length in the base mesh ("Stretch rule"), value and
                                    # gradient from one call in front of the objective.  0 = off: nothing changes
    weight_bend: float = 0.0        # > 0: every hinge is held to its dihedral angle in the base mesh ("Bend rule"), value and
                                    # gradient from one call in front of the objective.  0 = off: nothing changes
    weight_motion: float = 0.0      # > 0: the step's meshes are held smooth in TIME ("Motion rule"): every vertex's
                                    # acceleration (or velocity) across adjacent frames of the step is penalised, in head-local space -- the
                                    # per-frame pose is not touched.  Frames of different ranks are not coupled; a random subset
                                    # (frames_per_step) couples only the frames it draws that are adjacent in the take.  0 = off: nothing
                                    # changes, no launch, no allocation
    motion_order: int = 2           # 2: acceleration x_{f-1} - 2 x_f + x_{f+1} (constant velocity is free);  1: velocity x_{f+1} - x_f
    motion_scale: Optional[float] = None     # the Charbonnier scale c in the mesh's length units, finite and > 0: quadratic below c, linear
                                    # above it, so that a blink or a plosive is not smoothed away.  None: plain squares.  No default value --
                                    # nobody has measured one
    motion_vertex_weights: object = None     # one weight per vertex, finite and >= 0 (0: lips and eyelids left free; large: skull and neck
                                    # held stiff): an array-like [V] or the path of a text file with one number per vertex
    weight_tex_smooth: float = 0.0  # > 0: neighbouring texels are held together ("Texture prior rule"): the texels no camera
                                    # sees, or a mask takes out, get a gradient from their neighbours instead of none, and high-frequency
                                    # texture that explains a misplaced mesh is charged for.  Value and gradient from one call in front of
                                    # the objective, on the texture itself, whatever the pyramid level or mip.  0 = off: nothing changes
    tex_smooth_scale: Optional[float] = None     # the Charbonnier scale c in texture units (0..1), finite and > 0: quadratic below c, linear
                                    # above it, so that an edge of the texture is not smeared.  None: plain squares.  No default value --
                                    # nobody has measured one
    tex_smooth_weights: object = None            # one weight per texel, finite and >= 0; a pair takes the smaller of its two: an array-like
                                    # [Ht,Wt], the path of an 8-bit image (byte / 255, oriented as the texture.png a fit writes), or
                                    # 'chart': 1 on the texels the render can read (fit.chart_map), 0 elsewhere.  None: 1
    weight_tex_anchor: float = 0.0  # > 0: the texture is held to the texture the Fitter started with (after init_texture; re-snapshot with
                                    # Fitter.set_texture_anchor): under norm_sigma it is what keeps the level and contrast of a baked or
                                    # supplied texture.  0 = off: nothing changes
    tex_anchor_weights: object = None            # as tex_smooth_weights, per texel.  None: 1 -- or, with init_texture='bake', the bake's
                                    # `filled` map: only the texels a capture reached are held
    weight_landmark: float = 0.0    # > 0: named points of the mesh are held to their detected 2D positions in the captures (DESIGN.md 3,
                                    # "Landmark rule"; Scene.landmark_points / Scene.landmarks, scene.from_take(landmarkpath=...)): the
                                    # reprojection error in full-resolution pixels, value and the gradients for the vertices AND the poses
                                    # from one call in front of the objective, the same term at every pyramid level.  0 = off: nothing is
                                    # built, allocated or launched.  > 0 on a Scene without landmarks is a ValueError
    landmark_scale: Optional[float] = None       # the Charbonnier scale c in pixels, finite and > 0: quadratic below c, linear above it, so
                                    # a wrong detection does not outweigh the others.  None: plain squares.  No default value -- nobody has
                                    # measured one
    landmark_iters: int = 0         # 0 = the term is on for every iteration; n = for iterations i < n, then the run continues without it
    landmark_weights: object = None              # one weight per landmark, finite and >= 0, in place of the points' own 'weight': an
                                    # array-like [L] or the path of a text file with one number per landmark
    use_landmarks: bool = True      # False: a Scene's landmarks are ignored, whatever weight_landmark says
    init_pose: str = "keep"         # 'keep' | 'landmarks': every frame's rigid pose is solved from its landmarks at the end of construction
                                    # (Fitter.align_to_landmarks; DESIGN.md 3, "Pose solve rule"), before init_texture='bake' reads the pose.
                                    # Needs a Scene with landmarks and use_landmarks, not weight_landmark > 0
    init_pose_iters: int = 20       # the trials of that solve
    init_pose_rotation: bool = True             # False: the translation alone (the only form quat_renorm='tensor' keeps on several frames)
    init_expression: str = "keep"   # 'keep' | 'landmarks': every frame's blend weights are solved from its landmarks at the end of
                                    # construction (Fitter.solve_expression; DESIGN.md 3, "Expression solve rule"), after init_pose and before
                                    # init_texture='bake'.  mode 'prior' or 'combined'; needs a Scene with landmarks and use_landmarks
    init_expression_iters: int = 20             # the trials of that solve
    init_expression_ridge: float = 0.0          # its ridge towards neutral, px^2 per unit weight^2 (no recommended value: none is measured)
    init_landmark_rounds: int = 1   # the pose solve (init_pose='landmarks') and then the expression solve (init_expression='landmarks') run
                                    # this many times in turn: the two are solved alternately, not jointly
    quat_renorm: str = "tensor"     # 'tensor': the reference's division of q_opt and per_frame_q by the norm of the WHOLE tensor after every
                                    # step (quirk Q3) | 'rows': every quaternion divided by its own norm, so that a rotation survives the loop
    cam_idxs: Sequence[int] = (0, 1, 2, 3, 4, 5, 6, 7, 8)
    mode: str = "prior"
    regularize_correctives: bool = False
    regularize_prior: bool = False
    # build-side additions
    frames_per_step: int = 0        # 0 = every frame of this rank's shard, each step
    views_per_step: int = 0         # 0 = every camera of cam_idxs; k = a random subset of k cameras per step.  frames_per_step = 1 with
                                    # views_per_step = 1 is the reference's own run shape: ONE random (camera, frame) image per
                                    # iteration (fit.py:525-526)
    seed: int = 0
    optimize_texture: bool = True
    init_texture: str = "truth"     # 'truth' | 'random' (reference: np.random.uniform when no texpath, fit.py:438) | 'bake': drawn as for
                                    # 'random', then replaced by Fitter.bake_texture() over the shard's frames and the selected cameras
    fused_loss: bool = True         # False = reference-style torch.where + torch.mean chain
    fused_render: bool = True       # rasterize + interpolate + texture as one kernel pair (non-mip); False = four separate ops
    fused_objective: bool = True    # with fused_render and fused_loss: the whole pixel term as three kernels (ops.pixel_objective)
    grouped_adam: bool = True       # all ten Adam groups + the quaternion division as one launch (False: torch.optim.Adam(fused=True))
    sparse_objective: bool = True   # the three kernels skip image regions far from any geometry (same result)
    one_pass: bool = True           # fused path without mip: value AND gradient of the pixel term from one call (fpcdr_objective_fwd: the
                                    # kernel that shades a pixel chains its gradient back; False: forward call + backward call)
    queued_backward: bool = True    # fused path: the backward kernel runs over the list of occupied bins the forward left (with launch
                                    # hints) instead of one workgroup per bin of the batch (cfg3: 2.35 M waves dispatched, five in six
                                    # to leave at once -- 1.85 -> 1.74 ms); eager steps only, a HIP graph has no hints
    hip_graph: object = False       # capture forward+backward and the Adam update as two HIP graphs (launch-bound
                                    # small batches: cfg2 3.2 -> 1.8 ms / step; no gain once a step is GPU-bound: the graph
                                    # cannot use the launch hints).  'auto': graphs when a step draws few enough images for the
                                    # ~100 launches to cost more than the kernels (images x 32-pixel bins <= GRAPH_AUTO_BINS:
                                    # the reference's one-image steps, 1.6 -> 0.9 ms; not the 288-image batch)
    shading: str = "texture"        # 'texture' = reference render(); 'vertex' = rasterize + interpolate of a per-vertex
                                    # grey only (BASELINE.json configs[1]: "raster+interp only, no texture")
    blur_sigma: float = 0.0         # > 0: the pixel term is the mean square of the Gaussian-BLURRED residual (fit.pixel_loss_blurred;
                                    # DESIGN.md 3, "Blurred loss rule") on the operator path: every pixel within the kernel's radius of a
                                    # silhouette pulls on it, so a start several pixels off converges.  0 = off: nothing changes
    blur_sigma_end: Optional[float] = None   # with a value: sigma goes geometrically from blur_sigma to it over the blurred iterations
    blur_kernel_size: int = 31      # odd, 3 .. 63 (the reference's GaussianBlur(kernel_size=(31, 31)), fit.py:506)
    blur_iters: int = 0             # 0 = every iteration is blurred; n = iterations i < n, then the run continues on the path the other
                                    # flags select (the one-pass objective by default)
    norm_sigma: float = 0.0         # > 0: the pixel term is the LOCALLY NORMALISED loss (fit.pixel_loss_normalised; DESIGN.md 3, "Normalised
                                    # loss rule") on the operator path: render and capture are each reduced by the mean and divided by the
                                    # deviation of their own Gaussian window of this sigma, so a camera's exposure, gain and black level drop
                                    # out.  The logged loss is then DIMENSIONLESS (a mean of squared differences of normalised values, not of
                                    # grey levels).  Within a window the loss sees neither the absolute level nor the contrast of the texture:
                                    # use it with a baked or supplied start texture (init_texture='bake'), not from noise.  0 = off: nothing
                                    # changes.  Not together with blur_sigma > 0 (ValueError)
    norm_kernel_size: int = 31      # odd, 3 .. 63
    norm_eps: float = 2.0           # in grey levels, > 0: added (squared) to the window's variance, so flat regions stay finite and quiet
    norm_iters: int = 0             # 0 = every iteration is normalised; n = iterations i < n, then the run continues on the path the other
                                    # flags select
    pyramid: Sequence[Tuple[int, int]] = ()   # coarse-to-fine on a resolution pyramid of the captures: entries (factor, iterations) in order,
                                    # e.g. ((8, 300), (4, 300), (2, 400)) = iterations 0-299 at 1/8 of the size, 300-599 at 1/4, 600-999 at
                                    # 1/2, everything after at full size (a factor of 1 is allowed in an entry).  A level renders at
                                    # (H / factor, W / factor) with the same matrices -- the projection chain is pure NDC -- against the
                                    # captures box-reduced by that factor ("Downsample rule"), on the one-pass objective,
                                    # touching 1 / factor^2 of the pixels.  () = off: a step is exactly the path it was
    pyramid_mip: bool = True        # a step at a factor above 1 runs with enable_mip=True (max_mip_level as configured), whatever enable_mip
                                    # says for full size; False: enable_mip everywhere.  On by default because the coarse levels are useless
                                    # without it: the texture aliases under the 4-8 x larger pixel footprints, and on the CPU oracle's scan
                                    #  the gradient at factor 8 then has the WRONG sign from 3 pixels of offset on
    robust: str = ''                # 'l2' | 'charbonnier' | 'geman_mcclure': the pixel term is the WEIGHTED ROBUST loss (fit.pixel_loss_robust;
                                    # DESIGN.md 3, "Robust loss rule") on the operator path: like d^2 for residuals far below robust_scale,
                                    # 2 c |d| (Charbonnier) or c^2 (Geman-McClure) far above it, so highlights and occluders stop outweighing
                                    # the pixels the model can explain.  '' = off
    robust_scale: Optional[float] = None     # the scale c in grey levels, finite and > 0.  No default -- nobody has measured one: required
                                    # when robust is 'charbonnier' or 'geman_mcclure' (ValueError without), ignored for 'l2'
    robust_iters: int = 0           # 0 = every iteration uses `robust`; n = iterations i < n, then the run continues on the path the other
                                    # flags select (with weights on: the same term with kind 'l2')
    weight_outside: float = 1.0     # the weight of pixels the mesh does not cover (they are compared with the background), finite, >= 0
    saturation: int = 0             # 1..255: a capture pixel at or above it counts nothing (scene.from_take clips at 140); 0 = off
    face_weights: object = None     # one weight per triangle, finite and >= 0 (0: mouth socket, eyeballs, scalp): an array-like [T] or the
                                    # path of a text file with one number per face
    use_masks: bool = True          # a Scene with masks (scene.from_take(maskdir=...)) weights every pixel by its mask byte / 255
                                    # Any of these -- robust inside robust_iters, masks in use, face_weights, saturation > 0, weight_outside
                                    # != 1 -- makes the iteration run render_from_clip + pixel_loss_robust in the place of the one-pass
                                    # objective (kind 'l2' when only weights are on).  Not together with blur_sigma > 0 or norm_sigma > 0,
                                    # nor with hip_graph (ValueError).  All off: a step is exactly the path it was
    weighted_one_pass: bool = False # an iteration on the robust term runs the WEIGHTED ONE-PASS objective ("Weighted objective
                                    # rule") where it can -- fused_objective, fused_render, fused_loss, one_pass, sparse_objective, texture
                                    # shading, a level without mip (fit.weighted_one_pass_term) -- and the operator path elsewhere: the same
                                    # term, the image never in memory.  False: the operator path everywhere, as it was.  hip_graph with
                                    # weights keeps raising
    equalise_exposure_at: Sequence[int] = ()  # iterations at whose START step() calls Fitter.equalise_exposure() ("Exposure
                                    # rule"): every camera's gain and offset are fitted against the fit's own render, and this rank's
                                    # captures are mapped onto one common level, once, in place -- plain 8-bit targets again, so every fast
                                    # path runs on as it stands and nothing is paid per step.  Meant for one or two entries, once the
                                    # geometry is roughly right (after the norm_sigma or landmark iterations).  () = off: nothing is built,
                                    # allocated, cloned or launched, and a step is exactly the path it was
    equalise_method: str = 'regression'       # 'regression' | 'moments' (exposure.fit_gains)
    equalise_anchor_camera: Optional[int] = None   # a value of cam_idxs: that camera's captures stay as they are, bit for bit, and the
                                    # others are mapped onto its level.  None: onto the mean level of the usable cameras
    equalise_max_gain: float = 4.0  # > 1: a camera whose gain ratio lies outside [1 / max_gain, max_gain] is left alone.  A cap, not a
                                    # measurement: beyond two stops 8-bit data has nothing left to map
    log_interval: int = 0           # every n steps one JSON line {it, loss, lr, frames_per_s} (reference print, fit.py:621-623); an
                                    # iteration on the robust term adds "wsum", the sum of its weights over rank 0's batch
    reg_log_interval: int = 500     # every n steps the regulariser breakdown MEL / LAP / MNC (reference fit.py:597-601)
    log_path: Optional[str] = None  # JSON-lines file (appended); None with log_interval > 0 = stdout

    def __post_init__(self):
        if self.blur_sigma > 0 and self.norm_sigma > 0:
            raise ValueError("FitConfig.blur_sigma > 0 and norm_sigma > 0 exclude each other: an iteration has one pixel term")
        if self.robust not in ('', 'l2', 'charbonnier', 'geman_mcclure'):
            raise ValueError(f"FitConfig.robust must be '', 'l2', 'charbonnier' or 'geman_mcclure' (got {self.robust!r})")
        if self.robust not in ('', 'l2') and self.robust_scale is None:
            raise ValueError(f"FitConfig.robust={self.robust!r} needs robust_scale, in grey levels: there is no default")
        try:
            dr.robust_args(self.robust or 'l2', self.robust_scale, self.weight_outside, self.saturation)
        except (TypeError, ValueError) as e:
            raise ValueError(f"FitConfig (robust_scale, weight_outside, saturation): {e}")
        if isinstance(self.robust_iters, bool) or int(self.robust_iters) != self.robust_iters or self.robust_iters < 0:
            raise ValueError(f"FitConfig.robust_iters must be an integer >= 0 (got {self.robust_iters!r})")
        if self.weights_configured() and (self.blur_sigma > 0 or self.norm_sigma > 0):
            raise ValueError("FitConfig: robust, face_weights, saturation > 0 and weight_outside != 1 cannot be combined with blur_sigma > 0 "
                             "or norm_sigma > 0: weighting the windowed losses is a different rule")
        check_motion_options(self)
        check_tex_prior_options(self)
        check_landmark_options(self)
        check_pose_options(self)
        check_expression_options(self)
        check_exposure_options(self)

    def weights_configured(self):
        """Whether the options alone (without a Scene's masks) put iterations on the weighted robust pixel term."""
        return bool(self.robust) or self.face_weights is not None or self.saturation > 0 or float(self.weight_outside) != 1.0


def setup_dataset(blendshapes, n_frames, device):
    """reference fit.py:183-230: datasets['local'] = B[3V,K], maps['local'] = zeros[F,F], maps_intermediate = eye(K,F)."""
    datasets = {'local': torch.as_tensor(blendshapes, dtype=torch.float32, device=device).contiguous()}
    K = datasets['local'].shape[1]
    maps = {'local': torch.zeros(n_frames, n_frames, dtype=torch.float32, device=device)}
    maps_intermediate = {'local': torch.eye(K, n_frames, dtype=torch.float32, device=device)}
    return datasets, maps, maps_intermediate, torch.zeros(n_frames, dtype=torch.float32, device=device)


def setup_dataset_free(n_frames, n_vertices_x3, device):
    """reference fit.py:166-178."""
    m1 = torch.eye(n_frames, dtype=torch.float32, device=device)
    m2 = torch.eye(n_frames, dtype=torch.float32, device=device)
    m3 = torch.zeros((n_vertices_x3, n_frames), dtype=torch.float32, device=device)
    return m1, m2, m3, torch.zeros(n_frames, dtype=torch.float32, device=device)


def shard_indices(ft, frame_ids, view_ids=None):
    """The frames (and views) of a pass over Fitter ft's shard as checked int64 index tensors on its device: frame_ids None: all of this
    rank's frames, else a sequence or an integer tensor of any shape, flattened; view_ids: positions in cam_idxs, the same, None stays
    None.  IndexError as Fitter.check_indices raises it.  -> (frames, views)."""
    dev = ft.device
    frames = torch.arange(ft.frame_lo, ft.frame_hi, device=dev) if frame_ids is None else torch.as_tensor(frame_ids).to(dev).reshape(-1)
    views = None if view_ids is None else torch.as_tensor(view_ids).to(dev).reshape(-1)
    ft.check_indices(frames, views)
    return frames.long(), None if views is None else views.long()


def sum_over_ranks(t, world, reduce=None):
    """The convention of every pass that sums a table over the shards (bake_texture, equalise_exposure, align_to_landmarks): reduce(t) -> t
    sums the tensor over the ranks where the caller gives one; None: one all_reduce(SUM), in place, when world > 1 and torch.distributed
    is available and initialised, else t as it is.  Every rank then goes on from the same table, whatever the sharding."""
    if reduce is not None:
        return reduce(t)
    if world > 1:
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized():
            tdist.all_reduce(t, op=tdist.ReduceOp.SUM)
    return t


class Fitter:
    """State + one optimisation step of the fit loop for a take: a synthetic Scene (scene.cfg: targets are rendered from
    its hidden ground truth) or one read from disk (scene.from_take: targets are its reference images).

    rank / world: this process optimises frames [rank * F / world, (rank + 1) * F / world); parameters are
    replicated; `reduce_fn(flat_grad)` (dist.GradBucket) sums gradients over ranks before Adam.
    """

    def __init__(self, sc, cfg: FitConfig, device='cuda', rank=0, world=1, targets=None, reduce_fn=None):
        assert cfg.mode in ('prior', 'free', 'combined'), f"No valid mode ('{cfg.mode}')"
        self.sc, self.cfg, self.device = sc, cfg, torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError("Fitter runs on an MI355X (device='cuda'): the HIP path has no CPU fallback")
        self.rank, self.world, self.reduce_fn = rank, world, reduce_fn
        dev = self.device
        F = sc.n_frames
        from . import dist as _fdist
        self.n_frames = F
        self.frame_lo, self.frame_hi = _fdist.shard_frames(F, rank, world)      # (raises when F does not divide evenly over the ranks)
        motion = motion_options(cfg, sc.n_vertices, self.frame_hi - self.frame_lo) if cfg.weight_motion else None      # (or ValueError)
        self.resolution = tuple(cfg.resolution or sc.resolution)
        self.full_resolution = self.resolution      # (the captures' size; `resolution` is the active pyramid level's, the same without one)
        self._pyramid = self._check_pyramid(cfg, self.resolution)
        # the mip flag of the active level (_set_level): cfg.enable_mip at full size and wherever pyramid_mip is off
        self.enable_mip = bool(cfg.enable_mip)
        mip_at_levels = bool(cfg.pyramid_mip and cfg.shading == 'texture' and any(s > 1 for s, _ in self._pyramid))
        self.cam_idxs = list(cfg.cam_idxs)
        # ---- static scene tensors (fit.py:424-432) ----
        self.v_base = torch.tensor(sc.v_base, dtype=torch.float32, device=dev)
        self.pos_idx = torch.tensor(sc.pos_idx, dtype=torch.int32, device=dev)
        self.uv = torch.tensor(sc.uv, dtype=torch.float32, device=dev)
        self.uv_idx = torch.tensor(sc.uv_idx, dtype=torch.int32, device=dev)
        self.topo = MeshTopology(sc.pos_idx, sc.n_vertices, dev)
        if cfg.shading == 'vertex':
            tex_np = np.asarray(sc.texture, dtype=np.float32)
            iu = np.clip((sc.uv[:, 0] * tex_np.shape[1]).astype(int), 0, tex_np.shape[1] - 1)
            iv = np.clip((sc.uv[:, 1] * tex_np.shape[0]).astype(int), 0, tex_np.shape[0] - 1)
            self.vcol = torch.tensor(tex_np[iv, iu, :1], dtype=torch.float32, device=dev)      # [Vt,1]
        # ---- parameters (fit.py:433-480) ----
        gen = torch.Generator().manual_seed(cfg.seed)
        if cfg.init_texture == 'truth':
            tex = torch.tensor(sc.texture, dtype=torch.float32)
        else:
            tex = torch.rand(sc.texture.shape, generator=gen)
        self.tex_opt = tex.to(dev).requires_grad_(cfg.optimize_texture)
        self.t_opt = torch.zeros([9, 3], dtype=torch.float32, device=dev, requires_grad=True)
        q = torch.zeros([9, 4], dtype=torch.float32, device=dev)
        q[:, 3] = 1.0
        self.q_opt = q.requires_grad_(True)
        self.per_frame_t = torch.zeros([F, 3], dtype=torch.float32, device=dev, requires_grad=True)
        q = torch.zeros([F, 4], dtype=torch.float32, device=dev)
        q[:, 3] = 1.0
        self.per_frame_q = q.requires_grad_(True)
        self.datasets, self.maps, self.maps_intermediate, _ = setup_dataset(sc.blendshapes, F, dev)
        self.m1, self.m2, self.m3, _ = setup_dataset_free(F, self.v_base.shape[0], dev)
        corrective_lr = cfg.lr_base
        if cfg.mode == 'prior':
            self.maps['local'].requires_grad = True
            self.maps_intermediate['local'].requires_grad = True
        elif cfg.mode == 'free':
            for m in (self.m1, self.m2, self.m3):
                m.requires_grad = True
        else:
            self.maps['local'].requires_grad = True
            self.maps_intermediate['local'].requires_grad = True
            corrective_lr = cfg.lr_base * 0.1
        self.glctx = dr.RasterizeGLContext(output_db=bool(cfg.enable_mip or mip_at_levels), device=dev)
        # ---- optimiser: the reference's ten groups, same order (fit.py:493-505) ----
        groups = [{"params": self.m1, 'lr': corrective_lr}, {"params": self.m2, 'lr': corrective_lr},
                  {"params": self.m3, 'lr': corrective_lr}, {"params": self.maps['local'], 'lr': cfg.lr_base},
                  {"params": self.maps_intermediate['local'], 'lr': cfg.lr_base}, {"params": self.t_opt, 'lr': cfg.lr_t},
                  {"params": self.q_opt, 'lr': cfg.lr_q}, {"params": self.per_frame_t, 'lr': cfg.lr_t},
                  {"params": self.per_frame_q, 'lr': cfg.lr_q}, {"params": self.tex_opt, 'lr': cfg.lr_base * cfg.lr_tex_coef}]
        # the pixel terms ("Which pixel term an iteration runs"): what they and a Scene's masks ask of the other options
        sc_masks = sc.masks if cfg.use_masks else None
        self.face_w = None
        if cfg.face_weights is not None:
            self.face_w = torch.from_numpy(load_face_weights(cfg.face_weights, int(sc.pos_idx.shape[0]))).to(dev)
        check_pixel_terms(cfg, sc.masks is not None)
        self._weighted = sc_masks is not None or self.face_w is not None or cfg.saturation > 0 or float(cfg.weight_outside) != 1.0
        if cfg.hip_graph == 'auto':
            self.use_graph = self.auto_graph((cfg.frames_per_step or (self.frame_hi - self.frame_lo)) * (cfg.views_per_step or len(self.cam_idxs)),
                                             self.resolution)
        else:
            self.use_graph = bool(cfg.hip_graph)
        rows = cfg.quat_renorm == 'rows'
        if self.use_graph and cfg.grouped_adam:
            # a replayed update reads its learning rates and bias corrections from a device table (GroupedAdam.prepare): ONE launch in the
            # graph.  (torch.optim.Adam(capturable=True) is ~13 multi-tensor launches per parameter group: 140 of the 190 dispatches of a
            # replayed one-image step, 0.6 ms of 4.5 us nodes)
            self.optimizer = GroupedAdam(groups, lr=cfg.lr_base, renorm=(self.q_opt, self.per_frame_q), capturable=True, renorm_rows=rows)
        elif self.use_graph:      # replayed updates read the learning rates from device memory
            for g in groups:
                g['lr'] = torch.tensor(float(g['lr']), dtype=torch.float32, device=dev)
            self.optimizer = torch.optim.Adam(groups, lr=torch.tensor(cfg.lr_base, dtype=torch.float32, device=dev), capturable=True)
        else:
            self.optimizer = GroupedAdam(groups, lr=cfg.lr_base, renorm=(self.q_opt, self.per_frame_q), renorm_rows=rows) if cfg.grouped_adam \
                else torch.optim.Adam(groups, lr=cfg.lr_base, fused=True)
        # a step whose pixel objective ran out of record slots (ops.pixel_objective, skip_out) is skipped ON THE DEVICE: the call's last
        # kernel writes the flag, the gradient bucket carries it over the ranks, the Adam launch reads it -- no host read-back, no
        # exception on one rank between two collectives.  The kernel also re-forms bias corrections and learning rates for the steps
        # that did happen (lr_skip_gain = lr(i - 1) / lr(i) of LambdaLR's lr_ramp^(i / max_iter), fit.py:506-507)
        self._skip_flag = torch.zeros(1, dtype=torch.float32, device=dev)
        self._skip_cur = None
        self._grouped = isinstance(self.optimizer, GroupedAdam)      # (decided here, once: the optimiser is never replaced)
        if self._grouped and not self.optimizer.capturable:
            self.optimizer.enable_skips(lr_skip_gain=float(cfg.lr_ramp) ** (-1.0 / float(cfg.max_iter)))
        self._graphs, self._graph_key, self._frame_idx, self._view_idx = None, None, None, None
        self._stage_dev = None       # (graph mode: the fixed device buffer of a step's inputs, _stage_inputs)
        self._targets_f32 = None     # (the reference torch chain's float copy of the targets, made by its first step)
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self._zero = torch.zeros((), dtype=torch.float32, device=dev)
        self._background = torch.tensor(BACKGROUND, device=dev)     # (a device scalar made once: no host copy inside a HIP-graph capture)
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(
            self.optimizer, lr_lambda=lambda x: cfg.lr_ramp ** (float(x) / float(cfg.max_iter)))
        self.params = [g["params"][0] for g in self.optimizer.param_groups]
        # ---- camera constants (fit.py:514-521, 541-546) ----
        P, TMV = [], []
        trans = camera.translate(0.0, 170.0, 0.0)
        for c in self.cam_idxs:
            cal = sc.cams[c]
            P.append(camera.intrinsic_to_projection(cal['intr']))
            TMV.append(camera.extrinsic_to_modelview(cal['rot'], cal['trans_calib']) @ trans)
        self.proj = torch.tensor(np.stack(P), dtype=torch.float32, device=dev)
        self.t_mv = torch.tensor(np.stack(TMV), dtype=torch.float32, device=dev)
        self.cam_sel = torch.tensor(self.cam_idxs, dtype=torch.long, device=dev)
        self.rng = np.random.default_rng(cfg.seed + 1000 * rank)
        # final shapes (fit.py:457); every rank fills the rows of its own frames, gather_result() joins the shards
        self._result_full = torch.zeros(F, self.v_base.shape[0], dtype=torch.float32, device=dev)
        self._result_pending = None
        self.iteration = 0
        self._log_file, self._log_t, self._log_it = None, None, 0
        # ---- reference images, resident in HBM as 8 bit [F_local, n_cam, H, W] (fit.py:529-533) ----
        # exposure ("Exposure rule"): the composite table applied to this rank's captures so far (None: the identity), the last
        # fit, and whether the targets are the Fitter's own -- a tensor it was handed is never written into
        self._exposure_total, self._exposure_fit = None, None
        self._equalise_at = frozenset(int(i) for i in cfg.equalise_exposure_at)
        self._targets_own = targets is None
        if targets is not None:
            self.targets = targets
            if self._equalise_at:      # (cloned once, here; without the option: at the first call of equalise_exposure)
                self.targets, self._targets_own = targets.clone(), True
        elif sc.images is not None:      # a take from disk: this rank's frames x the selected cameras
            self.targets = torch.from_numpy(np.ascontiguousarray(sc.images[self.frame_lo:self.frame_hi][:, self.cam_idxs])).to(dev)
            if tuple(sc.images.shape[2:]) != self.resolution:      # a fixed reduced size: the captures box-reduced once
                self.targets = dr.downsample_images(self.targets, self._take_factor(tuple(sc.images.shape[2:]), self.resolution))
        else:
            assert sc.weights_gt is not None, "a Scene needs reference images (scene.from_take) or a synthetic ground truth"
            self.targets = self.render_targets()
        # the pixel loss of an all-background image, per (frame, camera): depends on the targets only (sparse objective)
        t = self.targets
        self.target_bg_sumsq = dr.reference_background_sumsq(t.reshape(-1, *self.resolution), BACKGROUND).reshape(t.shape[:2])
        self._shard_sums = {}        # (the cached sums over the whole shard, _rows_sum)
        self.full_targets = self.targets      # (always the captures; `targets` is the active pyramid level's, the same tensor without one)
        # ---- the masks of the captures, sharded and reduced exactly as the targets: 8 bit [F_local, n_cam, H, W], or None ----
        self.masks = None
        if sc_masks is not None:
            take_res = tuple(sc.images.shape[2:]) if sc.images is not None else tuple(sc.resolution)
            if tuple(sc_masks.shape) != (F, len(sc.cams)) + take_res or sc_masks.dtype != np.uint8:
                raise ValueError(f"Scene.masks must be uint8 {(F, len(sc.cams)) + take_res} (got {sc_masks.dtype} {tuple(sc_masks.shape)})")
            self.masks = torch.from_numpy(np.ascontiguousarray(sc_masks[self.frame_lo:self.frame_hi][:, self.cam_idxs])).to(dev)
            if take_res != self.resolution:       # a fixed reduced size: the box mean is the fractional weight of a coarse pixel
                self.masks = dr.downsample_images(self.masks, self._take_factor(take_res, self.resolution))
            if tuple(self.masks.shape) != tuple(self.targets.shape):
                raise ValueError(f"the masks {tuple(self.masks.shape)} do not match the targets {tuple(self.targets.shape)}")
        self.full_masks = self.masks
        self._wsum = None                     # (the sum of the weights of the last iteration on the robust term, for the step log)
        self._bg_wsum = {}                    # weighted one-pass: (level, kind, scale) -> [F_local * n_cam, 2] f64, cached like target_bg_sumsq
        # ---- pyramid levels: per factor in use (targets, (H, W), target_bg_sumsq, masks), each made from this rank's full-size targets ----
        self._levels, self._level = None, 1
        if self._pyramid:
            self._levels = {1: (self.targets, self.resolution, self.target_bg_sumsq, self.masks)}
            for s in sorted({s for s, _ in self._pyramid if s > 1}):
                lt = dr.downsample_images(self.full_targets, s)
                lres = (self.resolution[0] // s, self.resolution[1] // s)
                lm = dr.downsample_images(self.full_masks, s) if self.full_masks is not None else None
                self._levels[s] = (lt, lres, dr.reference_background_sumsq(lt.reshape(-1, *lres), BACKGROUND).reshape(lt.shape[:2]), lm)
        self._lmk, self._lmk_obs, self._lmk_res = None, None, None      # (_landmark_tables: built on first use, by the term or by align_to_landmarks)
        self._lmk_on, self._lmk_scratch = False, None      # (the landmark TERM's own: _build_landmarks)
        for _ in range(cfg.init_landmark_rounds):      # (in front of the bake, which reads the pose and the shape)
            if cfg.init_pose == 'landmarks':
                self.align_to_landmarks(iters=cfg.init_pose_iters, rotation=cfg.init_pose_rotation)
            if cfg.init_expression == 'landmarks':
                self.solve_expression(iters=cfg.init_expression_iters, ridge=cfg.init_expression_ridge)
        baked = None
        if cfg.init_texture == 'bake':
            _, baked = self.bake_texture()
        self._build_prior_terms(motion, baked)
        self._build_landmarks()
        if self._levels is not None:
            self._set_level(self.pyramid_factor())

    # ------------------------------------------------------------------------------------------
    def _build_prior_terms(self, motion, baked):
        """self._reg_terms: the step's eager terms as one PriorTerm each, in the fixed order Laplacian, stretch, bend, motion, texture, and
        what they need on the device (a weight of 0: nothing is built, allocated or launched).  motion, baked: __init__'s, or None."""
        cfg, dev, n_local = self.cfg, self.device, self.frame_hi - self.frame_lo
        # within a mesh: the base mesh is the rest shape of the terms that measure against it (the plain Laplacian has none)
        self.rest = RestShape(self.topo, self.v_base) if (cfg.laplacian_relative or cfg.weight_stretch or cfg.weight_bend) else None
        self._lap_rest = self.rest if cfg.laplacian_relative else None
        self._bnd_scratch = None
        if cfg.weight_bend:      # the hinge tables, and the scratch of the corner gradients for the most frames a step takes
            n_hinges = self.topo.hinges()[2]
            assert self.rest.bend_cs.shape == (2, n_hinges)      # (built here, not in the first step)
            self._bnd_scratch = torch.empty(max(n_local * n_hinges * 12, 1), dtype=torch.float32, device=dev)
        self._motion_w = torch.from_numpy(motion[1]).to(dev) if (cfg.weight_motion and motion[1] is not None) else None
        # the texture's prior ("Texture prior rule"): its maps, and the anchor = the texture as it stands now
        self._tex_anchor, self._tex_anchor_w, self._tex_smooth_w, self._tex_chart = None, None, None, None
        self._tex_prior_on = bool(cfg.weight_tex_smooth or cfg.weight_tex_anchor)
        if cfg.weight_tex_smooth:
            self._tex_smooth_w = self._texel_weights(cfg.tex_smooth_weights, 'tex_smooth_weights')
        if cfg.weight_tex_anchor:
            w = cfg.tex_anchor_weights
            if w is None and baked is not None:      # only the texels a capture reached are worth holding
                w = baked.to(torch.float32)
            self.set_texture_anchor(weights=w)
        # ONE accumulator buffer serves every term: the calls are ordered on the step's one stream, and each leaves the buffer zero (the
        # finish kernels of csrc/mesh_reg.hip and csrc/tex_prior.hip)
        self._reg_acc = torch.zeros(n_local + 1, dtype=torch.float64, device=dev)
        on_mesh = lambda rest: lambda vtx, ids: ((vtx, self.topo), dict(rest=rest))
        # this rank's frames only (the stencils end at the shard's borders), and of a random subset the frames adjacent in the take (the
        # kernel reads the frame numbers on the device: pick_frames' are sorted and distinct)
        on_frames = lambda vtx, ids: ((vtx,), dict(frame_ids=ids, order=cfg.motion_order, scale=cfg.motion_scale,
                                                   vertex_weights=self._motion_w, validate=False))
        # once per step on the texture itself, whatever the level or mip (read at the call: set_texture_anchor may add the weights later)
        on_texture = lambda vtx, ids: ((self.tex_opt,), dict(anchor=self._tex_anchor, smooth_weights=self._tex_smooth_w,
                                                             anchor_weights=self._tex_anchor_w, scale=cfg.tex_smooth_scale, validate=False))
        # (on, fn, inputs, weights, log keys, the step form's own keywords); LAP is logged by the torch form, fused_loss or not
        table = [(cfg.weight_laplacian and cfg.fused_loss, laplacian_penalty, on_mesh(self._lap_rest), [cfg.weight_laplacian], [], {}),
                 (cfg.weight_stretch, stretch_penalty, on_mesh(self.rest), [cfg.weight_stretch], ["STR"], {}),
                 (cfg.weight_bend, bend_penalty, on_mesh(self.rest), [cfg.weight_bend], ["BND"], dict(scratch=self._bnd_scratch)),
                 (cfg.weight_motion, motion_penalty, on_frames, [cfg.weight_motion], ["MOT"], {}),
                 (self._tex_prior_on, texture_prior, on_texture, [cfg.weight_tex_smooth, cfg.weight_tex_anchor], ["TEXS", "TEXA"], {})]
        self._reg_terms = [PriorTerm(fn, inputs, weights, keys, self.world, eager_grad=True, unit_upstream=True, acc=self._reg_acc, **step)
                           for on, fn, inputs, weights, keys, step in table if on]

    def _build_landmarks(self):
        """Switch the landmark term on ("Landmark rule"), or ValueError: the tables (_landmark_tables) and the scratch of the
        points' gradients for the most images a step takes.  weight_landmark = 0 or use_landmarks = False: nothing is built.  The term is
        not one of _reg_terms: it reads the matrices and the step's rows too, so loss_and_backward evaluates it itself (_landmark_term)
        and hands it over with them."""
        cfg = self.cfg
        if not cfg.weight_landmark or not cfg.use_landmarks:
            return
        lms, obs, _ = self._landmark_tables("FitConfig.weight_landmark > 0")
        self._lmk_on, self._lmk_scratch = True, torch.empty(obs.shape[0] * lms.n * 3, dtype=torch.float32, device=self.device)

    def _landmark_tables(self, who):
        """(the LandmarkSet with the configured weights, this rank's observations [F_local * n_cam, L, 3] laid out as the targets are, the
        observations' pixel grid) on the device, or ValueError in the name of `who`: built on first use and kept, for the landmark term
        and for Fitter.align_to_landmarks alike (which needs them without weight_landmark > 0)."""
        cfg, sc, dev = self.cfg, self.sc, self.device
        if self._lmk is not None:
            return self._lmk, self._lmk_obs, self._lmk_res
        if sc.landmarks is None or not sc.landmark_points:
            raise ValueError(f"{who} needs a Scene with landmarks (Scene.landmark_points and Scene.landmarks; "
                             "scene.from_take(landmarkpath=...)), or use_landmarks=False")
        lms = LandmarkSet(sc.landmark_points, sc.n_vertices, sc.pos_idx, dev)
        if cfg.landmark_weights is not None:
            lms = lms.with_weights(_load_weights(cfg.landmark_weights, lms.n, 'landmark_weights', 'landmark'))
        obs = np.asarray(sc.landmarks)
        if obs.shape != (self.n_frames, len(sc.cams), lms.n, 3):
            raise ValueError(f"Scene.landmarks must be [{self.n_frames},{len(sc.cams)},{lms.n},3] (got {tuple(obs.shape)})")
        obs = np.ascontiguousarray(obs[self.frame_lo:self.frame_hi][:, self.cam_idxs], dtype=np.float32)
        if not (np.isfinite(obs[..., 2]).all() and (obs[..., 2] >= 0).all()):
            raise ValueError("Scene.landmarks: the confidences must be finite and not negative (0: not observed)")
        obs[..., :2] = np.where(obs[..., 2:] > 0, obs[..., :2], 0.0)      # (what nobody observed is not read; keep it finite)
        if not np.isfinite(obs).all():
            raise ValueError("Scene.landmarks: the position of an observed landmark is not finite")
        # the pixel grid of the observations: the captures as read (a take fitted at a fixed reduced size keeps its landmarks' own grid:
        # the projection chain is pure NDC), which is full_resolution everywhere else
        res = tuple(sc.images.shape[2:]) if sc.images is not None else tuple(self.full_resolution)
        self._lmk, self._lmk_obs, self._lmk_res = lms, torch.from_numpy(obs.reshape(-1, lms.n, 3)).to(dev), res
        return self._lmk, self._lmk_obs, self._lmk_res

    @torch.no_grad()
    def align_to_landmarks(self, frame_ids=None, iters=20, rotation=True, reduce=None):
        """Solve every frame's rigid pose from its landmarks ("Pose solve rule"; fit.solve_pose), in ONE launch, at the
        current meshes (Fitter.vertices) and camera poses: the first stage of a landmark-driven fit, for a take whose head is not where
        the calibration puts it -- Adam at lr_t = 1e-5 cannot travel there.  Every camera of cam_idxs, the configured landmark_scale and
        landmark_weights.  Needs a Scene with landmarks and use_landmarks, NOT weight_landmark > 0: a fit may use its landmarks for the
        start only; the tables are built on first use.

          frame_ids  frames of this rank's shard (None: all of them), a sequence or an integer tensor
          iters      trials of the damped Gauss-Newton solve
          rotation   False: the translation alone.  True on more than one frame needs quat_renorm='rows': the whole-tensor division
                     (quirk Q3) scales every row to 1 / sqrt(F), and rigid() applies q as it stands, R(q / sqrt(F)) = I + (R(q) - I) / F
          reduce     reduce(delta) -> delta sums the float32 [F,7] table of (q, t) changes, zero outside this rank's frames, over the ranks
                     (sum_over_ranks' convention).  The replicated parameters stay identical on every rank

        per_frame_q / per_frame_t are written in place (a captured graph replays with them); Adam's moments stay as they are: call it
        before the first step.  Returns {'before', 'after'}: the mean live |residual| in pixels over the solved frames, and 'info'
        [Fb,4] = (cost before, cost after, live entries, accepted trials) per frame."""
        cfg, dev = self.cfg, self.device
        if not cfg.use_landmarks:
            raise ValueError("Fitter.align_to_landmarks needs FitConfig.use_landmarks")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise ValueError(f"Fitter.align_to_landmarks: iters must be an integer >= 0 (got {iters!r})")
        if rotation and cfg.quat_renorm == 'tensor' and self.n_frames > 1:
            raise ValueError("Fitter.align_to_landmarks(rotation=True) on more than one frame needs FitConfig.quat_renorm='rows': under "
                             "'tensor' every step divides per_frame_q by the norm of the WHOLE tensor, each row comes out at 1 / sqrt(F), "
                             "and the solved rotation is turned back to almost none (use rotation=False, or quat_renorm='rows')")
        lms, obs_all, res = self._landmark_tables("Fitter.align_to_landmarks")
        frames, _ = shard_indices(self, frame_ids)
        Fb, Nc = int(frames.shape[0]), len(self.cam_idxs)
        verts = self.vertices(frames, validate=False).reshape(Fb, -1, 3).contiguous()
        # base[c] = Rt(q_c, t_c) . MV_c . T(0,170,0), the float32 product k_mvp_fwd forms: its own launch with the frame at the identity and
        # the identity for the projection (a product with the identity is exact)
        eye_q = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=dev)
        all_cams = self.cam_idxs == list(range(self.q_opt.shape[0]))
        q_c, t_c = (self.q_opt, self.t_opt) if all_cams else (self.q_opt[self.cam_sel], self.t_opt[self.cam_sel])
        base = _mvp_func.apply(q_c.detach(), t_c.detach(), eye_q, torch.zeros(1, 3, dtype=torch.float32, device=dev),
                               torch.eye(4, dtype=torch.float32, device=dev).expand(Nc, 4, 4).contiguous(), self.t_mv,
                               None, None, None, None, None, None)
        obs = obs_all.index_select(0, self._target_rows(frames))
        q, t = self.per_frame_q.detach().index_select(0, frames).contiguous(), self.per_frame_t.detach().index_select(0, frames).contiguous()
        q0, t0 = q.clone(), t.clone()

        def mean_residual():      # (over the solved frames, at the parameters as they stand)
            rr = self.landmark_residuals(frames)
            live = ~torch.isnan(rr[..., 0])
            return float(rr[live].double().norm(dim=1).mean()) if bool(live.any()) else float('nan')

        before = mean_residual()
        info = solve_pose(verts, self.proj, base, lms, obs, q, t, res, scale=cfg.landmark_scale, iters=int(iters), rotation=bool(rotation))
        delta = torch.zeros(self.n_frames, 7, dtype=torch.float32, device=dev)
        delta.index_copy_(0, frames, torch.cat([q - q0, t - t0], dim=1))
        delta = sum_over_ranks(delta, self.world, reduce)
        # (every rank applies the same sum to the same table, its own rows included: a row nobody solved adds an exact 0, a solved row
        #  is its old value plus the rounded difference -- the solved value itself from the identity start, within an ulp of it otherwise)
        self.per_frame_q.add_(delta[:, :4])
        self.per_frame_t.add_(delta[:, 4:])
        return {'before': before, 'after': mean_residual(), 'info': info}

    @torch.no_grad()
    def solve_expression(self, frame_ids=None, iters=20, ridge=None, reduce=None):
        """Solve every frame's blend weights from its landmarks ("Expression solve rule"; fit.solve_expression), in ONE launch,
        at the current meshes (Fitter.vertices), matrices (Fitter.mvp) and weights: the stage after align_to_landmarks of a
        landmark-driven fit -- an open jaw is tens of pixels, and Adam moves a weight by lr_base a visit.  Every camera of cam_idxs, the
        configured landmark_scale and landmark_weights.  Needs a Scene with landmarks and use_landmarks, NOT weight_landmark > 0.
        mode 'prior' or 'combined' (the correctives stay where they are); mode='free' has no rig weights: ValueError.

          frame_ids  frames of this rank's shard (None: all of them), a sequence or an integer tensor
          iters      trials of the damped Gauss-Newton solve
          ridge      the pull towards neutral, px^2 per unit weight^2 (None: FitConfig.init_expression_ridge, whose default is 0)
          reduce     reduce(delta) -> delta sums the float32 [F,Kb] table of weight changes, zero outside this rank's frames, over the
                     ranks (sum_over_ranks' convention).  The replicated parameters stay identical on every rank

        Write-back: with W = maps_intermediate . maps ([Kb,F], the product the step forms), every rank writes maps_intermediate <- W +
        delta^T and maps <- the identity, in place (a captured graph replays with them).  Any [Kb,F] table is representable so, whatever
        Kb and F, and a product with the identity is exact: rig_weights() then returns the table itself, and a frame nobody solved keeps
        its weights bit for bit.  On one rank (world = 1, no reduce) the solved rows are the kernel's output bit for bit, from any
        start; across ranks every rank must form the same table from the summed change, W + (solved - W): the solved weights bit for
        bit from a neutral start, within an ulp of them otherwise.  A frame may be named once (ValueError).  This RESETS the factorisation the optimiser has been working on and leaves Adam's moments as they are: call it before the
        first step.  Returns {'before', 'after'}: the mean live |residual| in pixels over the solved frames, and 'info' [Fb,4] = (cost
        before, cost after, live entries, accepted trials) per frame."""
        cfg, dev = self.cfg, self.device
        if cfg.mode == 'free':
            raise ValueError("Fitter.solve_expression needs mode='prior' or 'combined': mode='free' has no rig weights to solve")
        if not cfg.use_landmarks:
            raise ValueError("Fitter.solve_expression needs FitConfig.use_landmarks")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise ValueError(f"Fitter.solve_expression: iters must be an integer >= 0 (got {iters!r})")
        ridge = cfg.init_expression_ridge if ridge is None else ridge
        if isinstance(ridge, bool) or not isinstance(ridge, (int, float)) or not np.isfinite(ridge) or ridge < 0:
            raise ValueError(f"Fitter.solve_expression: ridge must be finite and not negative (got {ridge!r})")
        lms, obs_all, res = self._landmark_tables("Fitter.solve_expression")
        frames, _ = shard_indices(self, frame_ids)
        Fb = int(frames.shape[0])
        if int(torch.unique(frames).shape[0]) != Fb:      # (a frame named twice would be written twice, in no fixed order)
            raise ValueError("Fitter.solve_expression: frame_ids names a frame more than once")
        mi, maps = self.maps_intermediate['local'], self.maps['local']
        verts = self.vertices(frames, validate=False).reshape(Fb, -1, 3).contiguous()
        mvp = self.mvp(frames, None, validate=False)
        obs = obs_all.index_select(0, self._target_rows(frames))
        table = rig_weights(mi.detach(), maps.detach(), slice(0, self.n_frames)).contiguous()      # W^T [F,Kb]
        w = table.index_select(0, frames).contiguous()
        w0 = w.clone()

        def mean_residual():      # (over the solved frames, at the parameters as they stand)
            rr = self.landmark_residuals(frames)
            live = ~torch.isnan(rr[..., 0])
            return float(rr[live].double().norm(dim=1).mean()) if bool(live.any()) else float('nan')

        before = mean_residual()
        info = solve_expression(verts, mvp, self.datasets['local'], lms, obs, w, res, scale=cfg.landmark_scale, ridge=float(ridge), iters=int(iters))
        delta = torch.zeros(self.n_frames, w.shape[1], dtype=torch.float32, device=dev)
        delta.index_copy_(0, frames, w - w0)
        delta = sum_over_ranks(delta, self.world, reduce)
        # (every rank applies the same sum to the same table: a row nobody solved adds an exact 0)
        table = table + delta
        if self.world == 1 and reduce is None:      # nobody else to agree with: the solved rows are the kernel's output itself
            table.index_copy_(0, frames, w)
        mi.copy_(table.t())
        maps.copy_(torch.eye(self.n_frames, dtype=torch.float32, device=dev))
        return {'before': before, 'after': mean_residual(), 'info': info}

    def landmark_on(self, i=None):
        """Whether iteration i (default: the current one) runs the landmark term (FitConfig.weight_landmark, landmark_iters)."""
        i = self.iteration if i is None else i
        return self._lmk_on and (not self.cfg.landmark_iters or i < self.cfg.landmark_iters)

    def _landmark_term(self, vtx, mvp, rows, step=True, residuals=None):
        """The landmark term on the step's meshes vtx [Fb,V,3], matrices mvp [Fb*Nc,4,4] and rows (_target_rows) of the observation table.
        step: the step's form -- the weight / world, the shared accumulator, the gradients made with the value for a unit upstream; else
        the log's: the full weight, a fresh accumulator."""
        cfg = self.cfg
        obs = self._take(self._lmk_obs, 0, rows)
        kw = dict(eager_grad=True, unit_upstream=True, acc=self._reg_acc, scratch=self._lmk_scratch) if step else {}
        return landmark_penalty(vtx, mvp, self._lmk, obs, cfg.weight_landmark / self.world if step else cfg.weight_landmark, self._lmk_res,
                                scale=cfg.landmark_scale, residuals=residuals, validate=False, **kw)

    @torch.no_grad()
    def landmark_residuals(self, frame_ids=None, view_ids=None):
        """(u - u*, v - v*) of every landmark at the current parameters, [Fb,Nc,L,2] in full-resolution pixels, NaN where the entry does
        not count (not observed, a landmark of weight 0, a point behind its camera): the number to look at to judge an alignment.
        frame_ids: frames of this rank's shard (None: all of them), a slice or an integer tensor; view_ids: positions in cam_idxs."""
        if self._lmk is None:      # (neither the term nor align_to_landmarks has built them)
            raise ValueError("Fitter.landmark_residuals needs FitConfig.weight_landmark > 0 on a Scene with landmarks")
        lms, obs_all, lres = self._lmk, self._lmk_obs, self._lmk_res
        frames = slice(self.frame_lo, self.frame_hi) if frame_ids is None else frame_ids
        if torch.is_tensor(frames):
            frames = frames.to(self.device, torch.long)
        if view_ids is not None:
            view_ids = torch.as_tensor(view_ids, dtype=torch.long, device=self.device)
        self.check_indices(frames, view_ids)
        Fb, Nc = self._n(frames), (len(self.cam_idxs) if view_ids is None else int(view_ids.shape[0]))
        vtx = self.vertices(frames, validate=False).reshape(Fb, -1, 3)
        res = torch.empty(Fb * Nc, lms.n, 2, dtype=torch.float32, device=self.device)
        landmark_penalty(vtx, self.mvp(frames, view_ids, validate=False), lms, self._take(obs_all, 0, self._target_rows(frames, view_ids)),
                         self.cfg.weight_landmark, lres, scale=self.cfg.landmark_scale, residuals=res, validate=False)
        return res.reshape(Fb, Nc, lms.n, 2)

    def texture_chart(self):
        """fit.chart_map of this Fitter's UV mesh at its texture's resolution, float32 [Ht,Wt], built on the first call and kept."""
        if self._tex_chart is None:
            self._tex_chart = chart_map(self.uv, self.uv_idx, self.tex_opt.shape[0], self.tex_opt.shape[1])
        return self._tex_chart

    def _texel_weights(self, weights, option):
        """A per-texel map of FitConfig (see tex_smooth_weights) or of set_texture_anchor as a float32 device tensor [Ht,Wt], or None."""
        if weights is None:
            return None
        Ht, Wt = int(self.tex_opt.shape[0]), int(self.tex_opt.shape[1])
        if isinstance(weights, str) and weights == 'chart':
            return self.texture_chart()
        if torch.is_tensor(weights):
            weights = weights.detach().cpu().numpy()
        return torch.from_numpy(load_texel_weights(weights, Ht, Wt, option)).to(self.device)

    @torch.no_grad()
    def set_texture_anchor(self, tex=None, weights=None):
        """Re-snapshot the anchor of FitConfig.weight_tex_anchor: tex [Ht,Wt,C] (None: the texture as it stands now), weights as
        FitConfig.tex_anchor_weights (None: the weights stay as they are).  The buffers a captured step reads are written in place, so
        it replays with the new anchor; the first set of weights of a Fitter that had none is a new capture."""
        if not self.cfg.weight_tex_anchor:
            raise ValueError("Fitter.set_texture_anchor needs FitConfig.weight_tex_anchor > 0: without it no step reads an anchor")
        src = self.tex_opt if tex is None else torch.as_tensor(tex, dtype=torch.float32)
        if tuple(src.shape) != tuple(self.tex_opt.shape):
            raise ValueError(f"Fitter.set_texture_anchor: tex must be {tuple(self.tex_opt.shape)} (got {tuple(src.shape)})")
        src = src.detach().to(self.device, torch.float32)
        if not bool(torch.isfinite(src).all()):
            raise ValueError("Fitter.set_texture_anchor: the anchor must be finite")
        if self._tex_anchor is None:
            self._tex_anchor = src.clone().contiguous()
        else:
            self._tex_anchor.copy_(src)
        if weights is not None:
            w = self._texel_weights(weights, 'tex_anchor_weights')
            if self._tex_anchor_w is None:
                self._tex_anchor_w = w.clone()
                self._graphs, self._graph_key = None, None
            else:
                self._tex_anchor_w.copy_(w)

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _check_pyramid(cfg, resolution):
        """FitConfig.pyramid as a tuple of (factor, iterations); ValueError for a malformed entry, a factor that does not divide the
        resolution, or a combination with hip_graph."""
        levels = []
        for entry in tuple(cfg.pyramid or ()):
            try:
                s, n = entry
                ok = int(s) == s and int(n) == n and not isinstance(s, bool) and not isinstance(n, bool)
            except (TypeError, ValueError):
                ok = False
            if not ok or not 1 <= int(s) <= 16 or int(n) < 0:
                raise ValueError(f"FitConfig.pyramid holds entries (factor in 1..16, iterations >= 0) (got {entry!r})")
            s, n = int(s), int(n)
            if resolution[0] % s or resolution[1] % s:
                raise ValueError(f"FitConfig.pyramid: the factor {s} does not divide the resolution {resolution[0]} x {resolution[1]}")
            levels.append((s, n))
        if levels and cfg.hip_graph:
            raise ValueError("FitConfig.pyramid cannot be combined with hip_graph: the captured shapes would change from one level to "
                             "the next")
        return tuple(levels)

    @staticmethod
    def _take_factor(take_res, resolution):
        """The one integer factor in 2..16 by which FitConfig.resolution divides a take's image size on both axes; ValueError otherwise."""
        (Ht, Wt), (H, W) = take_res, resolution
        s = Ht // H if H > 0 else 0
        if not (2 <= s <= 16 and H * s == Ht and W * s == Wt):
            raise ValueError(f"FitConfig.resolution {H} x {W} differs from the take's images ({Ht} x {Wt}) and is not their size divided by "
                             "one integer factor in 2..16")
        return s

    def pyramid_factor(self, i=None):
        """The pyramid factor of iteration i (default: the current one): 1 without a pyramid and after its last entry.  A function of the
        iteration alone, like blur_taps, so a resumed run lands on the right level."""
        i = self.iteration if i is None else i
        for s, n in self._pyramid:
            if i < n:
                return s
            i -= n
        return 1

    def _level_bg_wsum(self, kind, scale):
        """[F_local * n_cam, 2] f64: per image of the active level, the all-background share of the weighted one-pass objective of (kind,
        scale) and of its weights (ops.reference_background_weighted) -- made once per level and kind, as target_bg_sumsq is per level."""
        key = (self._level, kind, scale)
        if key not in self._bg_wsum:
            masks = self.masks.reshape(-1, *self.resolution) if self.masks is not None else None
            self._bg_wsum[key] = dr.reference_background_weighted(self.targets.reshape(-1, *self.resolution), masks, kind, scale,
                                                                  self.cfg.weight_outside, self.cfg.saturation, BACKGROUND)
        return self._bg_wsum[key]

    def _set_level(self, s):
        """Make the level of factor s the active one: `resolution`, `targets`, `target_bg_sumsq` and `enable_mip` are that level's, and the
        caches keyed to them are dropped.  full_resolution / full_targets keep naming the captures."""
        if s == self._level:
            return
        self.targets, self.resolution, self.target_bg_sumsq, self.masks = self._levels[s]
        self.enable_mip = bool(self.cfg.enable_mip or (s > 1 and self.cfg.pyramid_mip))
        self._shard_sums, self._targets_f32 = {}, None
        self._level = s

    @staticmethod
    def _n(frame_ids):
        return frame_ids.stop - frame_ids.start if isinstance(frame_ids, slice) else len(frame_ids)

    def check_indices(self, frame_ids, view_ids=None):
        """Raise IndexError for frame numbers outside the take or outside this rank's shard, and for view positions outside cam_idxs.
        The indexed kernels behind mvp() / vertices() / loss_and_backward() gather from -- and scatter-add into -- the full parameter
        tables WITHOUT bounds checks (the index_select calls they replaced raised): a caller's own index tensors are checked here,
        once, on the host (one read-back per tensor); the loop's own draws (pick_frames / pick_views) are in range by construction."""
        if isinstance(frame_ids, slice):
            lo, hi = frame_ids.start or 0, frame_ids.stop
            if frame_ids.step not in (None, 1) or hi is None or not (self.frame_lo <= lo <= hi <= self.frame_hi):
                raise IndexError(f"frames {frame_ids} outside this rank's frames [{self.frame_lo}, {self.frame_hi})")
        else:
            f = torch.as_tensor(frame_ids)
            if f.dtype not in (torch.int64, torch.int32) or f.dim() != 1 or f.numel() == 0:
                raise IndexError("frame_ids must be a non-empty 1-D integer tensor or a slice")
            lo, hi = int(f.min()), int(f.max())
            if lo < self.frame_lo or hi >= self.frame_hi:
                raise IndexError(f"frame numbers {lo}..{hi} outside this rank's frames [{self.frame_lo}, {self.frame_hi})")
        if view_ids is not None:
            v = torch.as_tensor(view_ids)
            if v.dtype not in (torch.int64, torch.int32) or v.dim() != 1 or v.numel() == 0:
                raise IndexError("view_ids must be a non-empty 1-D integer tensor")
            lo, hi = int(v.min()), int(v.max())
            if lo < 0 or hi >= len(self.cam_idxs):
                raise IndexError(f"view positions {lo}..{hi} outside cam_idxs (0..{len(self.cam_idxs) - 1})")

    def mvp(self, frame_ids, view_ids=None, pool=None, validate=True):
        """mvp[f,c] = P_c . Rt(q_f,t_f) . Rt(q_c,t_c) . MV_c . T(0,170,0)   (fit.py:541-553), [Fb*Nc,4,4].
        view_ids: positions in cam_idxs of the cameras of this step (a device index tensor; None = all of them).  pool: the step's ZeroPool.
        validate: check_indices (index tensors only; the loop's own calls pass False)."""
        if validate and (torch.is_tensor(frame_ids) or view_ids is not None):
            self.check_indices(frame_ids, view_ids)
        all_cams = self.cam_idxs == list(range(self.q_opt.shape[0]))    # no gather (and no sort in its backward) then
        if view_ids is not None or torch.is_tensor(frame_ids):
            # rows named by index: one launch each way on the full parameter tables (the gathers happen inside the kernels)
            if isinstance(frame_ids, slice):
                f_idx = torch.arange(frame_ids.start, frame_ids.stop, device=self.device)
            else:
                f_idx = frame_ids
            Nc = len(self.cam_idxs) if view_ids is None else int(view_ids.shape[0])
            return _mvp_func.apply(self.q_opt, self.t_opt, self.per_frame_q, self.per_frame_t, self.proj, self.t_mv, f_idx.contiguous(),
                                   view_ids, None if all_cams else self.cam_sel, int(f_idx.shape[0]), Nc, pool)
        q_c, t_c = (self.q_opt, self.t_opt) if all_cams else (self.q_opt[self.cam_sel], self.t_opt[self.cam_sel])
        return _mvp_func.apply(q_c, t_c, self._take(self.per_frame_q, 0, frame_ids), self._take(self.per_frame_t, 0, frame_ids), self.proj, self.t_mv,
                               None, None, None, None, None, pool)

    @staticmethod
    def _take(t, dim, ids):
        """t[ids] / t[:, ids] for a slice or an index tensor.  A tensor goes through index_select: its backward is ONE index_add
        launch where advanced indexing sorts the indices first (seven launches) -- a fifth of a one-image step's launches."""
        if isinstance(ids, slice):
            if ids.step in (None, 1) and (ids.start or 0) == 0 and ids.stop is not None and ids.stop >= t.shape[dim]:
                return t      # every frame (one rank, frames_per_step = 0): no slice node, whose backward is a zero-fill and a copy
            return t[ids] if dim == 0 else t[:, ids]
        return t.index_select(dim, ids)

    def _step_masks(self, rows):
        """The masks of the rows a batch names (_target_rows) [n, H, W], or None without masks."""
        return self._take(self.masks.reshape(-1, *self.resolution), 0, rows) if self.masks is not None else None

    def _rows_sum(self, name, key, table, rows):
        """The sum over `rows` of a per-image table [F_local * n_cam, ...].  A slice is the whole shard, every view: the same numbers every
        step, kept under `name` for as long as `key` and the slice stay what they were; an index tensor is summed anew."""
        if isinstance(rows, slice):
            key = (key, rows.start, rows.stop)
            if self._shard_sums.get(name, (None,))[0] != key:
                self._shard_sums[name] = (key, table[rows].sum(0))
            return self._shard_sums[name][1]
        t = table.index_select(0, rows)
        return t.reshape(()) if t.numel() == 1 else t.sum(0)

    def _target_rows(self, frame_ids, view_ids=None):
        """The rows of the flat [F_local * n_cam, H, W] view of `targets` (and of target_bg_sumsq, flattened) that a batch names: frame numbers
        of the take (a slice or an index tensor) x positions in cam_idxs (None: every camera).  A contiguous range of frames with every
        camera is a slice -- a view, no launch --, anything else ONE row tensor for index_select, frame-major as the batch is."""
        n_cam = self.targets.shape[1]
        if isinstance(frame_ids, slice):
            lo, hi = frame_ids.start - self.frame_lo, frame_ids.stop - self.frame_lo
            if view_ids is None:
                return slice(lo * n_cam, hi * n_cam)
            f_idx = torch.arange(lo, hi, device=self.device)
        else:
            f_idx = frame_ids - self.frame_lo if self.frame_lo else frame_ids
        cams = torch.arange(n_cam, device=self.device) if view_ids is None else view_ids
        return (f_idx[:, None] * n_cam + cams[None, :]).reshape(-1)

    def vertices(self, frame_ids, iteration=None, pool=None, validate=True):
        """Blended vertex buffers [Fb,3V] for a batch of frames (fit.py:555-562).  The reference multiplies by a
        one-hot frame vector (fit.py:536, 115-116); M e_f is column f of M, so the batch selects columns
        (a slice -- no copy -- when the frames are a contiguous range).  validate: check_indices for an index tensor."""
        if validate and torch.is_tensor(frame_ids):
            if int(frame_ids.min()) < 0 or int(frame_ids.max()) >= self.n_frames:
                raise IndexError(f"frame numbers outside the take (0..{self.n_frames - 1})")
        if self.cfg.mode in ('prior', 'combined'):
            # (validate=False: the frame indices are pick_frames' own, drawn from this rank's range)
            out = blend_batched(self.v_base, self.datasets['local'],
                                rig_weights(self.maps_intermediate['local'], self.maps['local'], frame_ids, validate=False), pool)
            if self.cfg.mode == 'prior':
                return out
        basis_t = rig_weights(self.m2, self.m1, frame_ids, validate=False)                                            # [Fb,F]
        if self.cfg.mode == 'free':
            return blend_batched(self.v_base, self.m3, basis_t, pool)
        return out + 0.5 * blend_batched(None, self.m3, basis_t, pool)    # learned_coefficient=0.5, fit.py:562

    @torch.no_grad()
    def bake_texture(self, frame_ids=None, view_ids=None, interior_only=False, dilate=8, assign=True, reduce=None, chunk=4):
        """A start texture from the captures at the CURRENT parameters ("Bake rule"): every covered pixel of the chosen
        targets splats its capture into the four texels the forward would read for it; a texel is the weighted mean of what landed on
        it, texels next to filled ones take their neighbours' mean (`dilate` passes), the rest 0.5.  A noise texture (the reference's
        start without a texpath, fit.py:438) leaves the first thousands of steps without a usable pose or shape gradient.

          frame_ids      frames of this rank's shard (None: all of them), a sequence or an integer tensor
          view_ids       positions in cam_idxs (None: every selected camera)
          interior_only  leave out silhouette pixels, whose capture holds background
          assign         copy the result into tex_opt (Adam's moments stay as they are: call it before the first step)
          reduce         reduce(acc) -> acc sums the int64 accumulator over the ranks (sum_over_ranks' convention).  Integer sums: every
                         rank resolves the same bits, whatever the sharding
          chunk          frames rasterised at a time

        Returns (tex [Ht,Wt,C] float32, filled [Ht,Wt] bool: the texels a capture reached)."""
        dev = self.device
        H, W = self.full_resolution
        Ht, Wt, C = self.tex_opt.shape
        frames, views = shard_indices(self, frame_ids, view_ids)
        glctx = dr.RasterizeGLContext(output_db=False, device=dev)
        targets = self.full_targets.reshape(-1, H, W)
        acc = torch.zeros(Ht, Wt, 2, dtype=torch.int64, device=dev)
        for lo in range(0, int(frames.shape[0]), max(1, int(chunk))):
            ids = frames[lo:lo + max(1, int(chunk))].contiguous()
            verts = self.vertices(ids, validate=False).reshape(int(ids.shape[0]), -1, 3)
            pos_clip = transform_clip_batched(self.mvp(ids, views, validate=False), verts)
            rast, _ = dr.rasterize(glctx, pos_clip, self.pos_idx, resolution=(H, W))
            texc, _ = dr.interpolate(self.uv[None, ...], rast, self.uv_idx)
            # (the targets' row 0 is the bottom row, as the raster's: no flip)
            dr.bake_accumulate(texc, rast, targets.index_select(0, self._target_rows(ids, views)), acc, interior_only=interior_only)
        acc = sum_over_ranks(acc, self.world, reduce)
        plane, filled = dr.bake_resolve(acc, color_scale=255.0, dilate=dilate)
        tex = plane[..., None].expand(Ht, Wt, C).contiguous()
        if assign:
            self.tex_opt.copy_(tex)
        return tex, filled

    def render_full(self, glctx, frame_ids):
        """(colour [Fb*Nc,H,W,C], rast) of the frames `frame_ids` (an index tensor) x every camera of cam_idxs at full resolution and the
        current parameters, through the path a step's operator render takes: render_from_clip with cfg.enable_mip, or render_vertex
        under vertex shading.  glctx: a context with output_db when cfg.enable_mip."""
        cfg = self.cfg
        H, W = self.full_resolution
        verts = self.vertices(frame_ids, validate=False).reshape(int(frame_ids.shape[0]), -1, 3)
        pos_clip = transform_clip_batched(self.mvp(frame_ids, validate=False), verts)
        if cfg.shading == 'vertex':
            return self.render_vertex(glctx, pos_clip, (H, W))
        return render_from_clip(glctx, pos_clip, self.pos_idx, self.uv, self.uv_idx, self.tex_opt, (H, W), bool(cfg.enable_mip),
                                cfg.max_mip_level, cfg.fused_render)

    def exposure_range(self):
        """(lo, hi, keep_from) of the Exposure rule for this Fitter: captures at or above cfg.saturation (> 0) mean "saturated", stay that
        byte and count nothing; 0 and 255 (clipped black, clipped white) count nothing either."""
        keep_from = int(self.cfg.saturation) if self.cfg.saturation > 0 else 256
        return 1, min(keep_from, 255) - 1, keep_from

    @torch.no_grad()
    def equalise_exposure(self, frame_ids=None, method=None, anchor_camera=None, max_gain=None, reduce=None, chunk=4, apply=True):
        """Fit every camera's gain and offset against the fit's OWN render at the current parameters and map this rank's captures onto one
        common level, in place ("Exposure rule"): the step a take with unequal cameras needs before the plain pixel term --
        one-pass objective, weighted one-pass, pyramid, hip_graph -- can fit it.  Call it once the geometry is roughly right (after the
        norm_sigma or landmark iterations), once or twice per fit: every application rounds again.

          frame_ids      frames of this rank's shard whose renders are compared (None: all of them), a sequence or an integer tensor
          method         'regression' | 'moments' (None: cfg.equalise_method)
          anchor_camera  a value of cam_idxs whose captures stay as they are (None: cfg.equalise_anchor_camera; without either the
                         common level is the mean over the usable cameras)
          max_gain       None: cfg.equalise_max_gain
          reduce         reduce(sums) -> sums adds the int64 [Nc,6] table over the ranks (sum_over_ranks' convention).  Integer sums:
                         every rank fits the same tables, whatever the sharding
          chunk          frames rendered at a time
          apply          False: fit and report only; the captures, the composite table and the captured graphs stay as they are

        With the Scene's masks (use_masks), cfg.face_weights and the range of exposure_range().  ALL of this rank's full_targets are mapped,
        then everything derived from them is made again in place -- every pyramid level's targets (from the full-size ones) and
        target_bg_sumsq, the float copy of the torch loss, the cached sums; tensors a captured graph reads keep their addresses.  Targets
        handed in through targets= are cloned first (once), which discards a captured graph.  Returns exposure.fit_gains' dict plus
        'composite': the uint8 [Nc,256] table of everything applied to this rank's captures so far."""
        cfg, dev = self.cfg, self.device
        H, W = self.full_resolution
        Nc = len(self.cam_idxs)
        method = cfg.equalise_method if method is None else method
        max_gain = cfg.equalise_max_gain if max_gain is None else max_gain
        anchor_camera = cfg.equalise_anchor_camera if anchor_camera is None else anchor_camera
        anchor = None
        if anchor_camera is not None:
            if isinstance(anchor_camera, bool) or anchor_camera not in self.cam_idxs:
                raise ValueError(f"Fitter.equalise_exposure: anchor_camera must be one of cam_idxs {tuple(self.cam_idxs)} (got {anchor_camera!r})")
            anchor = self.cam_idxs.index(anchor_camera)
        frames, _ = shard_indices(self, frame_ids)
        lo, hi, keep_from = self.exposure_range()
        glctx = dr.RasterizeGLContext(output_db=bool(cfg.enable_mip), device=dev)
        targets = self.full_targets.reshape(-1, H, W)
        masks = self.full_masks.reshape(-1, H, W) if self.full_masks is not None else None
        table = torch.zeros(Nc, 6, dtype=torch.int64, device=dev)
        for c0 in range(0, int(frames.shape[0]), max(1, int(chunk))):
            ids = frames[c0:c0 + max(1, int(chunk))].contiguous()
            colour, rast = self.render_full(glctx, ids)
            rows = self._target_rows(ids)
            sums = dr.exposure_sums(colour.contiguous(), rast, targets.index_select(0, rows), mask=None if masks is None else masks.index_select(0, rows),
                                    face_weights=self.face_w, lo=lo, hi=hi)
            table += sums.reshape(int(ids.shape[0]), Nc, 6).sum(0)
        table = sum_over_ranks(table, self.world, reduce)
        out = fit_gains(table, method=method, anchor=anchor, max_gain=max_gain, keep_from=keep_from)
        if apply:
            self._apply_exposure(out['lut'])
            self._exposure_fit = out
        out['composite'] = identity_lut(Nc) if self._exposure_total is None else self._exposure_total.copy()
        return out

    @torch.no_grad()
    def _apply_exposure(self, lut):
        """Map this rank's full_targets through lut uint8 [Nc,256] in place, fold it into the composite table, and make everything
        derived from the targets again, in place (equalise_exposure).  An identity table changes nothing and launches nothing."""
        if is_identity(lut):
            return
        H, W = self.full_resolution
        Nc = len(self.cam_idxs)
        if not self._targets_own:      # the caller's tensor: cloned once; a captured graph reads the old one
            own = self.full_targets.clone()
            if self.targets is self.full_targets:
                self.targets = own
            if self._levels is not None:
                self._levels[1] = (own,) + tuple(self._levels[1][1:])
            self.full_targets, self._targets_own = own, True
            self._graphs, self._graph_key = None, None
        full = self.full_targets
        n_img = full.numel() // (H * W)
        cams = (torch.arange(n_img, device=self.device) % Nc).to(torch.int32)
        dr.apply_lut_u8(full.reshape(n_img, H * W), torch.from_numpy(np.ascontiguousarray(lut)).to(self.device), cams)
        bg = lambda t, res: dr.reference_background_sumsq(t.reshape(-1, *res), BACKGROUND).reshape(t.shape[:2])
        if self._levels is None:
            self.target_bg_sumsq.copy_(bg(full, (H, W)))
        else:      # every level from the full-size captures, never a cascade
            for s, (lt, lres, lbg, _) in self._levels.items():
                if s > 1:
                    lt.copy_(dr.downsample_images(full, s))
                lbg.copy_(bg(lt, lres))
        if self._targets_f32 is not None:
            self._targets_f32.copy_(self.targets.to(torch.float32))
        self._bg_wsum = {}
        for name in list(self._shard_sums):      # the cached sums over the shard: a captured graph reads the plain term's
            key, val = self._shard_sums[name]
            if name == 'bg_sumsq':
                val.copy_(self.target_bg_sumsq.reshape(-1)[key[1]:key[2]].sum(0))
            else:
                del self._shard_sums[name]
        total = identity_lut(Nc) if self._exposure_total is None else self._exposure_total
        total = compose(total, lut)
        self._exposure_total = None if is_identity(total) else total

    @torch.no_grad()
    def render_targets(self, chunk=4):
        """Synthetic reference images: the hidden ground truth (weights, pose, texture) rendered through the
        same ops, quantised to 8 bit and clipped to [0,140] like the reference's loader (fit.py:531)."""
        sc, dev = self.sc, self.device
        H, W = self.full_resolution
        Nc = len(self.cam_idxs)
        out = torch.empty(self.frame_hi - self.frame_lo, Nc, H, W, dtype=torch.uint8, device=dev)
        tex = torch.tensor(sc.texture, dtype=torch.float32, device=dev)
        w_gt = torch.tensor(sc.weights_gt, dtype=torch.float32, device=dev)
        t_gt = torch.tensor(sc.t_gt, dtype=torch.float32, device=dev)
        q_gt = torch.tensor(sc.q_gt, dtype=torch.float32, device=dev)
        ctx = dr.RasterizeGLContext(output_db=False, device=dev)
        for lo in range(self.frame_lo, self.frame_hi, chunk):
            ids = torch.arange(lo, min(lo + chunk, self.frame_hi), device=dev)
            verts = blend_batched(self.v_base, self.datasets['local'], w_gt[ids]).reshape(len(ids), -1, 3)
            rigid = camera.rigid_grad(t_gt[ids], camera.unitquat_to_rotmat(q_gt[ids]))
            mvp = torch.matmul(self.proj[None], torch.matmul(rigid[:, None], self.t_mv[None])).reshape(-1, 4, 4)
            if self.cfg.shading == 'vertex':
                img, rast_t = self.render_vertex(ctx, transform_clip_batched(mvp, verts), (H, W))
                img = torch.where(rast_t[..., 3:] > 0, img, torch.tensor(BACKGROUND, device=dev))
            else:
                img = render(ctx, mvp, verts, self.pos_idx, self.uv, self.uv_idx, tex, (H, W), False, 0)
            img = torch.clamp(torch.round(img[..., 0] * 255.0), 0, 140).to(torch.uint8)
            out[lo - self.frame_lo: lo - self.frame_lo + len(ids)] = img.reshape(len(ids), Nc, H, W)
        return out

    def render_vertex(self, glctx, pos_clip, resolution=None):
        """rasterize + interpolate only (no texture, no antialias): per-vertex grey through the uv index buffer,
        background composited like fit.py:161.  resolution: default the active level's.  Returns (colour [B,H,W,1], rast)."""
        rast, _ = dr.rasterize(glctx, pos_clip, self.pos_idx, resolution=resolution or self.resolution)
        col, _ = dr.interpolate(self.vcol[None], rast, self.uv_idx)
        return col, rast

    # ------------------------------------------------------------------------------------------
    def pick_frames(self):
        n_local = self.frame_hi - self.frame_lo
        k = self.cfg.frames_per_step or n_local
        if k >= n_local:
            return slice(self.frame_lo, self.frame_hi)     # the whole shard: views, no gathers
        sel = torch.tensor(np.sort(self.rng.choice(n_local, size=k, replace=False)) + self.frame_lo, dtype=torch.long)
        if not self.use_graph:
            return sel.to(self.device)
        if self._frame_idx is None:     # graphs read the minibatch's frame numbers from one fixed buffer
            self._frame_idx = torch.empty(k, dtype=torch.long, device=self.device)
        self._frame_idx.copy_(sel)
        return self._frame_idx

    def _stage_inputs(self):
        """Graph mode: everything a replayed step reads that changes from step to step -- the frame numbers and camera positions drawn for
        it, the optimiser's (step size, bias correction) table -- goes through ONE pinned buffer and ONE asynchronous copy into fixed
        device memory (three copies from pageable memory before: 130 us of host-side gaps in a 0.33 ms one-image step).  A ring of
        pinned buffers, each guarded by the event of its copy, lets the host run ahead.  Returns (frame_ids, view_ids, prepared)."""
        n_local = self.frame_hi - self.frame_lo
        kf = self.cfg.frames_per_step if 0 < self.cfg.frames_per_step < n_local else 0
        kv = self.cfg.views_per_step if 0 < self.cfg.views_per_step < len(self.cam_idxs) else 0
        cap = self._grouped and self.optimizer.capturable
        if self._stage_dev is None:
            n = kf + kv + _lib.ADAM_MAX_TENSORS          # int64 words; the table's 2 x ADAM_MAX_TENSORS floats are ADAM_MAX_TENSORS of them
            self._stage_dev = torch.zeros(n, dtype=torch.int64, device=self.device)
            self._stage_ring = []
            for _ in range(4):
                t = torch.zeros(n, dtype=torch.int64).pin_memory()
                self._stage_ring.append([t, t.numpy(), t[kf + kv:].view(torch.float32).numpy(), None])
            self._stage_i = 0
            self._frame_idx = self._stage_dev[:kf] if kf else None
            self._view_idx = self._stage_dev[kf:kf + kv] if kv else None
            if cap:
                self.optimizer.set_table_dev(self._stage_dev[kf + kv:].view(torch.float32))
        slot = self._stage_ring[self._stage_i % len(self._stage_ring)]
        self._stage_i += 1
        if slot[3] is not None:
            slot[3].synchronize()
        if kf:
            slot[1][:kf] = np.sort(self.rng.choice(n_local, size=kf, replace=False)) + self.frame_lo
        if kv:
            slot[1][kf:kf + kv] = np.sort(self.rng.choice(len(self.cam_idxs), size=kv, replace=False))
        if cap:
            self.optimizer.prepare(host_out=slot[2])
        if kf or kv or cap:
            self._stage_dev.copy_(slot[0], non_blocking=True)
            slot[3] = torch.cuda.Event()
            slot[3].record()
        frame_ids = self._frame_idx if kf else slice(self.frame_lo, self.frame_hi)
        return frame_ids, (self._view_idx if kv else None), cap

    def pick_views(self):
        """The cameras of this step: None = all of cam_idxs, else a device tensor of k random positions in cam_idxs."""
        k = self.cfg.views_per_step
        if not k or k >= len(self.cam_idxs):
            return None
        sel = torch.tensor(np.sort(self.rng.choice(len(self.cam_idxs), size=k, replace=False)), dtype=torch.long)
        if not self.use_graph:
            return sel.to(self.device)
        if self._view_idx is None:      # graphs read the step's camera numbers from one fixed buffer
            self._view_idx = torch.empty(k, dtype=torch.long, device=self.device)
        self._view_idx.copy_(sel)
        return self._view_idx

    def _mode_switch(self):
        # fit.py:603-608 switches the learned basis on AFTER the forward pass of the first iteration i > max_iter / 2, so
        # it receives its first gradient in the iteration after that one
        if self.cfg.mode == 'combined' and (self.iteration - 1) > self.cfg.max_iter / 2:
            for m in (self.m1, self.m2, self.m3):
                m.requires_grad = True

    def _term_args(self, name, i=None):
        """pixel_term's arguments of the term `name` at iteration i (default: the current one), or None when that iteration runs another."""
        term = pixel_term(self.cfg, self.iteration if i is None else i, self._weighted)
        return term[1:] if term is not None and term[0] == name else None

    def blur_taps(self, i=None):
        """The taps of the blurred pixel loss at iteration i (default: the current one), or None when that iteration is not blurred."""
        return (self._term_args('blur', i) or (None,))[0]

    def norm_taps(self, i=None):
        """The taps of the normalised pixel loss at iteration i (default: the current one), or None when that iteration is not normalised."""
        return (self._term_args('norm', i) or (None,))[0]

    def robust_term(self, i=None):
        """(kind, scale) of the weighted robust pixel term at iteration i (default: the current one), or None when it does not run it."""
        return self._term_args('robust', i)

    def loss_and_backward(self, frame_ids, view_ids=None, validate=True):
        """Forward + backward of fit.py:556-611 for a batch of frames x cameras (view_ids: see mvp).  Returns the loss (tensor).
        validate: check a caller's index tensors on the host first (check_indices); step() passes False for its own draws."""
        if validate and not torch.cuda.is_current_stream_capturing():
            self.check_indices(frame_ids, view_ids)
        cfg = self.cfg
        i = self.iteration
        if self._levels is not None:      # (before anything below reads the resolution, the targets or the mip flag)
            self._set_level(self.pyramid_factor(i))
        mip = self.enable_mip
        self._mode_switch()
        self._skip_cur = None
        Fb, Nc = self._n(frame_ids), (len(self.cam_idxs) if view_ids is None else int(view_ids.shape[0]))
        C = self.tex_opt.shape[2]
        term = pixel_term(cfg, i, self._weighted)
        robust = term is not None and term[0] == 'robust'
        form, weighted_shot = step_path(cfg, term, mip, C)      # (the step's path, asked once)
        one_pass, one_shot = form == 'one_pass', form in ('one_pass', 'two_call')
        # one flat buffer for the small accumulators of this step's backward kernels, zero-filled by the objective's first kernel; the
        # pool around it goes to the functions whose backward takes views of it
        zero_buf, pool = None, None
        if one_pass:
            n_pose = (self.q_opt.shape[0] + self.per_frame_q.shape[0]) if (view_ids is not None or torch.is_tensor(frame_ids)) else (Fb + Nc)
            zero_buf = torch.empty(Fb * Nc * 16 + 7 * n_pose + 64 + Fb * (self.datasets['local'].shape[1] + self.m3.shape[1]),
                                   dtype=torch.float32, device=self.device)
            pool = ZeroPool(zero_buf)
        vtx_pos = self.vertices(frame_ids, pool=pool, validate=False)                 # [Fb,3V]
        vtx_pos_split = vtx_pos.reshape(Fb, -1, 3)
        mvp = self.mvp(frame_ids, view_ids, pool, validate=False)
        n_img_global = Fb * Nc * self.world
        # the step's reference images.  A random (frame, view) subset is ONE gather of the images it names from the flat [F * Nc, H, W]
        # table (the reference's run shape draws one image per step: selecting the frame's nine images first and the view second copied
        # 17 MB for 1.9 MB -- 39 of the step's ~330 us of kernels)
        rows = self._target_rows(frame_ids, view_ids)
        ref = self._take(self.targets.reshape(-1, *self.resolution), 0, rows)
        n_total = n_img_global * self.resolution[0] * self.resolution[1] * C
        pos_clip = transform_clip_batched(mvp, vtx_pos_split, pool)  # camera.transform_clip (camera.py:11-23), batched
        if cfg.shading == 'vertex':
            colour, rast_out = self.render_vertex(self.glctx, pos_clip)
            n_total = n_img_global * self.resolution[0] * self.resolution[1]
        elif not one_shot:
            colour, rast_out = render_from_clip(self.glctx, pos_clip, self.pos_idx, self.uv, self.uv_idx, self.tex_opt,
                                                self.resolution, mip, cfg.max_mip_level, cfg.fused_render)
        # regularisers (fit.py:578-595): evaluated on this rank's meshes, averaged over all ranks
        reg = self._zero
        if cfg.weight_meshedge:
            reg = reg + cfg.weight_meshedge * mesh_edge_loss(vtx_pos_split, self.topo, 0.1)
        if cfg.weight_laplacian and not cfg.fused_loss:
            # the reference squares the value of ONE mesh per step (fit.py:581): a batch is the mean of the squares
            reg = reg + cfg.weight_laplacian * (mesh_laplacian_smoothing(vtx_pos_split, self.topo, per_mesh=True, rest=self._lap_rest) ** 2).mean()
        if cfg.weight_normalconsistency:
            reg = reg + cfg.weight_normalconsistency * mesh_normal_consistency(vtx_pos_split, self.topo)
        if cfg.regularize_correctives and cfg.mode == 'combined' and i > cfg.max_iter / 2:
            basis = torch.matmul(self.m2, self._take(self.m1, 1, frame_ids))
            reg = reg + torch.mean(torch.matmul(self.m3, basis) ** 2)
        if cfg.regularize_prior and cfg.mode == 'prior':
            mi = torch.matmul(self.maps_intermediate['local'], self._take(self.maps['local'], 1, frame_ids))
            reg = reg + torch.mean(mi ** 2)
        chained = reg is not self._zero      # (some term above was added)
        if self.world > 1 and chained:
            reg = reg / self.world
        # the eager terms (_build_prior_terms), their gradients made here with their values; a slice of frames is consecutive (no frame
        # numbers to hand over), an index tensor names them
        step_ids = frame_ids if torch.is_tensor(frame_ids) else None
        terms = [reg_term(vtx_pos_split, step_ids) for reg_term in self._reg_terms]
        if self.landmark_on(i):      # (on the step's matrices too: both gradients come with the value)
            terms.append(self._landmark_term(vtx_pos_split, mvp, rows))
        self.optimizer.zero_grad(set_to_none=True)
        if one_shot:
            bg_sum = None
            if cfg.sparse_objective and not weighted_shot:
                bg_sum = self._rows_sum('bg_sumsq', None, self.target_bg_sumsq.reshape(-1), rows)
            self._skip_cur = self._skip_target() if one_pass else None
            wkw = {}
            if weighted_shot:      # the same weights pixel_loss_robust takes, and the level's all-background share of this term
                mask = self._step_masks(rows)
                bgw = self._rows_sum('bg_wsum', (self._level, term[1], term[2]), self._level_bg_wsum(term[1], term[2]), rows)
                sums = (None, torch.empty(1, dtype=torch.float64, device=self.device))
                wkw = dict(robust=(term[1], term[2]), mask=mask, face_weights=self.face_w, weight_outside=cfg.weight_outside,
                           saturation=cfg.saturation, ref_bg_wsum=bgw, wsum_out=sums[1], check_weights=False)
            pix = dr.pixel_objective(self.glctx, pos_clip, self.pos_idx, self.uv, self.uv_idx, self.tex_opt, ref, self.resolution,
                                     n_total, BACKGROUND, sparse=cfg.sparse_objective, ref_bg_sumsq=bg_sum,
                                     enable_mip=mip, max_mip_level=cfg.max_mip_level,
                                     queued_backward=cfg.queued_backward and not self.use_graph,
                                     one_pass=cfg.one_pass, unit_upstream=True, zero_extra=zero_buf,      # (the seeds below are 1)
                                     skip_out=self._skip_cur, **wkw)
            self._backward(pix, self._one, reg, *terms)
            value = pix.detach()
        elif cfg.fused_loss:
            weights = {}
            if robust:
                weights = dict(mask=self._step_masks(rows), face_weights=self.face_w, weight_outside=cfg.weight_outside, saturation=cfg.saturation)
            sums, g_colour = pixel_term_loss(term, colour, rast_out, ref, n_total, **weights)
            self._backward(colour, g_colour, reg, *terms)
            value = sums[0].to(torch.float32) / n_total
        else:
            col = torch.where(rast_out[..., 3:] > 0, colour, self._background)
            # the reference holds its target image as float32 on the GPU (fit.py:531-532); the 8-bit batch is converted once
            if self._targets_f32 is None:
                self._targets_f32 = self.targets.to(torch.float32)
            ref_f = self._take(self._targets_f32.reshape(-1, *self.resolution), 0, rows).reshape(Fb * Nc, *self.resolution, 1)
            loss = torch.mean((ref_f - col * 255) ** 2) / self.world + reg
            for t in terms:
                loss = loss + t
            loss.backward()
        if cfg.fused_loss:      # the value, summed after the backward pass has been enqueued.  An add is a launch: the one-pass step
            # has none for a reg that is the constant 0; the operator path has always had it, and keeps its launches
            loss = value + reg.detach() if (chained or not one_shot) else value
            for t in terms:
                loss = loss + t.detach()
        self._wsum = sums[1].reshape(()) if robust else None      # (the sum of the weights of an iteration on the robust term, for the step log)
        self._store_result(frame_ids, vtx_pos.detach())
        return loss.detach()

    def _backward(self, root, seed, *terms):
        """The step's backward pass: `root` seeded with `seed`, and every regulariser term that has a graph with d loss / d term = 1,
        handed over as a cached device scalar (`(pix + reg).backward()` would put an add and a fill between the forward and the backward
        kernel: the loss's value is summed after the pass has been enqueued)."""
        roots, seeds = [root], [seed]
        for term in terms:
            if term is not None and term.requires_grad:
                roots.append(term)
                seeds.append(self._one)
        torch.autograd.backward(roots, seeds)

    @property
    def result(self):
        """[F,3V] the last vertices computed for every frame (reference fit.py: `result[i] = vtx_pos` each iteration)."""
        self._flush_result()
        return self._result_full

    def _flush_result(self):
        if self._result_pending is not None:
            ids, v = self._result_pending
            self._result_pending = None
            self._result_full[ids] = v

    def _store_result(self, frame_ids, v):
        # a step over the same contiguous frame range as the last one (the whole shard, every step) replaces its rows: the tensor is kept
        # and copied into the table when somebody reads it (or when another range comes), not 5.8 MB in the serial tail of every step
        if isinstance(frame_ids, slice) and not self.use_graph and not torch.cuda.is_current_stream_capturing():
            if self._result_pending is not None and self._result_pending[0] != frame_ids:
                self._flush_result()
            self._result_pending = (frame_ids, v)
        else:
            self._flush_result()
            self._result_full[frame_ids] = v

    def _skip_target(self):
        """Where this step's pixel objective writes its "my results are invalid" flag (None: the optimiser cannot skip): the gradient
        bucket's extra element when the reducer has one (dist.GradBucket.flag -- summed over the ranks with the gradients), else the
        Fitter's own float (all-reduced on its own in _eager_step() when there are other ranks)."""
        if not self._grouped or self.optimizer.skipped is None:
            return None
        flag = getattr(self.reduce_fn, "flag", None) if self.reduce_fn is not None else None
        return flag if flag is not None else self._skip_flag

    @property
    def skipped_steps(self):
        """Steps skipped on the device so far (a host read-back: call it where a synchronisation is acceptable)."""
        sk = getattr(self.optimizer, "skipped", None)
        return int(sk.item()) if sk is not None else 0

    def skipped_steps_per_tensor(self):
        """Per parameter tensor (self.params order): the skipped steps in which it had a gradient -- its state['step'] counted them, its
        update did not (a host read-back)."""
        sk = getattr(self.optimizer, "skipped_per_tensor", None)
        return [int(v) for v in sk[:len(self.params)].tolist()] if sk is not None else [0] * len(self.params)

    def _update(self, prepared=False):
        if not self._grouped:
            self.optimizer.step()
            with torch.no_grad():   # fit.py:616-618 (Q3: whole-tensor norm)
                if self.cfg.quat_renorm == 'rows':      # (every quaternion by its own norm, summed as the kernel sums it)
                    for q in (self.q_opt, self.per_frame_q):
                        q /= torch.sqrt((q[:, 0:1] * q[:, 0:1] + q[:, 1:2] * q[:, 1:2]) + (q[:, 2:3] * q[:, 2:3] + q[:, 3:4] * q[:, 3:4]))
                    return
                self.q_opt /= torch.sum(self.q_opt ** 2) ** 0.5
                self.per_frame_q /= torch.sum(self.per_frame_q ** 2) ** 0.5
            return
        if self.optimizer.capturable and not prepared:
            self.optimizer.prepare()      # (an eager step of a graph-mode Fitter: warm-up, or a new set of trainable tensors)
        self.optimizer.skip_flag = self._skip_cur
        self.optimizer.step()             # (the division of fit.py:616-618 happens inside the launch)

    def _eager_step(self, frame_ids, view_ids, prepared):
        """Forward + backward, gradient all-reduce and update as plain launches: a step outside graph mode, and a graph-mode Fitter's
        warm-up steps and the one step after its set of trainable tensors has changed."""
        loss = self.loss_and_backward(frame_ids, view_ids, validate=False)
        if self.reduce_fn is not None:
            self.reduce_fn(self.params)
        # the skip flag of this step's objective, on its way to the update.  Inert in graph mode: an optimiser made for replay has no skip
        # counters (__init__ enables them for a GroupedAdam that is not capturable only), so _skip_target() gave loss_and_backward None
        if self._skip_cur is not None and getattr(self.reduce_fn, "flag", None) is not None:
            self._skip_cur = self.reduce_fn.flag      # (the bucket lays itself out anew when the set of trainable tensors changes)
        if self.world > 1 and self._skip_cur is self._skip_flag:      # (a reducer without a flag element: the flag travels alone)
            import torch.distributed as tdist
            if tdist.is_initialized():
                tdist.all_reduce(self._skip_flag, op=tdist.ReduceOp.SUM)
        self._update(prepared)
        return loss

    def step(self):
        """One Adam step (fit.py:524-618): forward, backward, gradient all-reduce, update, schedule, renormalise."""
        prepared = False
        if self._equalise_at and self.iteration in self._equalise_at:
            self.equalise_exposure()
        if self._levels is not None:
            self._set_level(self.pyramid_factor())
        self._mode_switch()      # (before the optimiser's table of this step is written: a parameter that turns trainable now counts this step)
        if self.use_graph:
            frame_ids, view_ids, prepared = self._stage_inputs()
        else:
            frame_ids = self.pick_frames()
            view_ids = self.pick_views()
        if self.use_graph and self.iteration >= self.GRAPH_WARMUP:
            loss = self._step_graphed(frame_ids, view_ids, prepared)
        else:
            loss = self._eager_step(frame_ids, view_ids, prepared)
        self.scheduler.step()
        if self.cfg.log_interval:
            self._log_step(frame_ids, loss)
        self.iteration += 1
        return loss

    # ------------------------------------------------------------------------------------------
    def _log_step(self, frame_ids, loss):
        """JSON-lines step log on rank 0: the reference prints loss and learning rates every log_interval iterations
        (fit.py:621-623; reading the loss is its one host sync) and the regulariser breakdown every 500 (fit.py:597-601)."""
        cfg, i = self.cfg, self.iteration
        if self.rank != 0:
            return
        rec = None
        if i % cfg.log_interval == 0:
            now = time.perf_counter()
            rec = {"it": i, "frames": self._n(frame_ids) * self.world, "loss": float(loss),
                   "lr": [float(x) for x in self.scheduler.get_last_lr()]}
            if self._wsum is not None:      # an iteration on the robust term: the sum of its weights (the effective entry count)
                rec["wsum"] = float(self._wsum)
            if self._log_t is not None and i > self._log_it:
                rec["frames_per_s"] = self._n(frame_ids) * self.world * (i - self._log_it) / (now - self._log_t)
            self._log_t, self._log_it = time.perf_counter(), i
        if cfg.reg_log_interval and i % cfg.reg_log_interval == 0:
            with torch.no_grad():
                v = self.vertices(frame_ids, validate=False).reshape(self._n(frame_ids), -1, 3)
                rec = rec or {"it": i}
                rec["MEL"] = float(cfg.weight_meshedge * mesh_edge_loss(v, self.topo, 0.1))
                rec["LAP"] = float(cfg.weight_laplacian * (mesh_laplacian_smoothing(v, self.topo, per_mesh=True, rest=self._lap_rest) ** 2).mean())
                rec["STR"], rec["BND"] = 0.0, 0.0      # (always there; the later terms' keys only with the term on)
                rec["MNC"] = float(cfg.weight_normalconsistency * mesh_normal_consistency(v, self.topo))
                for reg_term in self._reg_terms:
                    rec.update(reg_term.log(v, frame_ids if torch.is_tensor(frame_ids) else None))
                if self.landmark_on(i):      # (the term at its full weight, over every camera of the step's frames)
                    rec["LMK"] = float(self._landmark_term(v, self.mvp(frame_ids, validate=False), self._target_rows(frame_ids), step=False))
        if rec is None:
            return
        line = json.dumps(rec)
        if cfg.log_path:
            if self._log_file is None:
                os.makedirs(os.path.dirname(os.path.abspath(cfg.log_path)), exist_ok=True)
                self._log_file = open(cfg.log_path, "a")
            self._log_file.write(line + "\n")
            self._log_file.flush()
        else:
            print(line, flush=True)

    GRAPH_WARMUP = 3    # eager steps before capture (allocator, Adam state, scratch and topology caches settle)
    GRAPH_AUTO_BINS = 40960   # hip_graph='auto': graphs up to this many 32 x 32-pixel bins per step (~20 images of 1920 x 1080)

    @classmethod
    def auto_graph(cls, images_per_step, resolution):
        """The rule of FitConfig.hip_graph='auto'."""
        H, W = resolution
        return images_per_step * ((H + 31) // 32) * ((W + 31) // 32) <= cls.GRAPH_AUTO_BINS

    def _step_graphed(self, frame_ids, view_ids=None, prepared=False):
        """Replay (capturing first if needed) graph A = forward + backward into fixed gradient buffers and graph B =
        Adam + quaternion renormalisation; the gradient all-reduce runs between them, outside any graph.  The set of
        trainable tensors is part of the key: 'combined' mode switches the free-form basis on half way (fit.py:603-608)."""
        switch = self.cfg.mode == 'combined' and (self.iteration - 1) > self.cfg.max_iter / 2
        key = (switch, tuple(p.requires_grad for p in self.params), self.landmark_on())
        if self._graph_key != key:
            # new set of trainable tensors: one eager step first, so that Adam creates their state outside a capture
            self._graph_key, self._graphs = key, None
            return self._eager_step(frame_ids, view_ids, prepared)
        cap_adam = self._grouped and self.optimizer.capturable
        if self._graphs is None:
            if _lib.TIMER is not None:
                raise RuntimeError("per-kernel timing (KernelTimer) cannot be recorded inside a HIP graph")
            torch.cuda.synchronize()
            # ONE graph when nothing has to run between the backward pass and the update (a single rank); with a gradient all-reduce the
            # update is a second graph behind it
            one_graph = self.reduce_fn is None
            ga, gb = torch.cuda.CUDAGraph(), (None if one_graph else torch.cuda.CUDAGraph())
            self.optimizer.zero_grad(set_to_none=True)
            # no garbage collection inside a capture: a dead Fitter is CYCLIC garbage (the closures of its prior terms), so it is freed
            # whenever the collector happens to run, and freeing its pinned buffers records events, which is not permitted while a stream
            # captures -- the process aborts.  torch.cuda.graph() does not collect first: collect here, and keep the collector off
            gc_was_on = gc.isenabled()
            gc.collect()
            gc.disable()
            try:
                with torch.cuda.graph(ga):
                    loss = self.loss_and_backward(frame_ids, view_ids, validate=False)
                    if one_graph:
                        self._update(prepared=True)
                if not one_graph:
                    with torch.cuda.graph(gb, pool=ga.pool()):
                        self._update(prepared=True)
            finally:
                if gc_was_on:
                    gc.enable()
            self._graphs = (ga, gb, loss)      # capture does not execute: fall through to the first replay
        ga, gb, loss = self._graphs
        if cap_adam and not prepared:
            self.optimizer.prepare()           # step counters, learning rates of this step -> the device table the captured launch reads
        ga.replay()
        if gb is not None:
            if self.reduce_fn is not None:
                self.reduce_fn(self.params)
            gb.replay()
        return loss

    @torch.no_grad()
    def init_near_truth(self, scale=0.8):
        """Start at `scale` x the synthetic ground truth (prior mode): M1 = I, M2 = scale * W_gt^T, per-frame pose.
        The checkered synthetic texture makes the pixel loss non-convex beyond about half a check."""
        sc, dev = self.sc, self.device
        self.maps['local'].copy_(torch.eye(self.n_frames, device=dev))
        self.maps_intermediate['local'].copy_(scale * torch.tensor(sc.weights_gt, device=dev).t())
        self.per_frame_t.copy_(scale * torch.tensor(sc.t_gt, device=dev))
        # quaternions stay at the reference's identity start: its whole-tensor renormalisation (quirk Q3,
        # fit.py:616-618) rescales every row by 1/sqrt(F), which only the identity survives unchanged

    # ------------------------------------------------------------------------------------------
    def weights(self):
        """Current blendshape activations [F,K] (prior mode): (M2 M1)^T."""
        with torch.no_grad():
            return torch.matmul(self.maps_intermediate['local'], self.maps['local']).t()

    # ------------------------------------------------------------------------------------------
    def state_dict(self):
        """Everything a resumed run needs to continue bit-identically (the reference has no checkpointing, SURVEY.md
        section 5): parameters, Adam moments, schedule position, iteration, minibatch RNG and the result buffer."""
        names = ("m1", "m2", "m3", "maps_local", "maps_intermediate_local", "t_opt", "q_opt", "per_frame_t", "per_frame_q", "tex_opt")
        # (the composite exposure table, present only when this rank's captures have been mapped: today's key sets stay as they are)
        exposure = {} if self._exposure_total is None else {"exposure_lut": torch.from_numpy(self._exposure_total.copy())}
        return {**exposure,
                "params": {n: p.detach().clone() for n, p in zip(names, self.params)},
                "requires_grad": [bool(p.requires_grad) for p in self.params],
                "optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(),
                "iteration": self.iteration, "rng": self.rng.bit_generator.state,
                "skipped_steps": self.skipped_steps,      # (device-side skips: the update kernel subtracts them from the step counters,
                "skipped_per_tensor": self.skipped_steps_per_tensor(),      # each tensor its own; the schedule the total)
                "result": self.result.clone(),      # this rank's rows (others zero): checkpoints are per rank
                "frame_range": (self.frame_lo, self.frame_hi),
                "config": dict(self.cfg.__dict__),
                # (the texture prior's anchor and its weights: None without the term; a checkpoint without the keys loads as before)
                "tex_anchor": None if self._tex_anchor is None else self._tex_anchor.clone(),
                "tex_anchor_weights": None if self._tex_anchor_w is None else self._tex_anchor_w.clone()}

    def load_state_dict(self, state):
        with torch.no_grad():
            for p, (_, v) in zip(self.params, state["params"].items()):
                p.copy_(v.to(p.device))
        for p, rg in zip(self.params, state["requires_grad"]):
            p.requires_grad = rg
        self._load_optimizer(state["optimizer"])
        self.scheduler.load_state_dict(state["scheduler"])
        self.iteration = int(state["iteration"])
        total = int(state.get("skipped_steps", 0))
        per = state.get("skipped_per_tensor")
        if per is None:      # (a checkpoint from before the per-tensor counts: the global count for every tensor with state, as the old kernel had it)
            per = [total if 'step' in self.optimizer.state.get(p, {}) else 0 for p in self.params]
        per = [int(v) for v in per]
        assert len(per) == len(self.params) and all(0 <= v <= total for v in per), (per, total)
        if getattr(self.optimizer, "skipped", None) is not None:
            self.optimizer.skipped.fill_(total)
            self.optimizer.skipped_per_tensor.zero_()
            self.optimizer.skipped_per_tensor[:len(per)].copy_(torch.tensor(per, dtype=torch.int32))
        elif total > 0:
            self._forget_skips(total, per)
        self.rng.bit_generator.state = state["rng"]
        self.result.copy_(state["result"].to(self.result.device))
        if self._tex_anchor is not None and state.get("tex_anchor") is not None:      # (without the key the anchor stays as constructed)
            self.set_texture_anchor(state["tex_anchor"], state.get("tex_anchor_weights"))
        if state.get("exposure_lut") is not None:      # the checkpoint's captures were mapped: map these the same way, once
            lut = np.ascontiguousarray(torch.as_tensor(state["exposure_lut"]).cpu().numpy())
            if lut.dtype != np.uint8 or lut.shape != (len(self.cam_idxs), 256):
                raise ValueError(f"load_state_dict: exposure_lut must be uint8 [{len(self.cam_idxs)},256] (got {lut.dtype} {lut.shape})")
            if self._exposure_total is None:
                self._apply_exposure(lut)
            elif not np.array_equal(self._exposure_total, lut):
                raise ValueError("load_state_dict: the checkpoint's exposure table differs from the one already applied to this Fitter's "
                                 "captures; load it into a Fitter whose captures are as read")
        elif self._exposure_total is not None:      # (a checkpoint without the key: its captures were as read, these are mapped)
            raise ValueError("load_state_dict: the checkpoint carries no exposure table, but this Fitter's captures have been mapped; load "
                             "it into a Fitter whose captures are as read")
        self._graphs, self._graph_key = None, None
        if self._levels is not None:
            self._set_level(self.pyramid_factor())

    def _load_optimizer(self, sd):
        """torch's Optimizer.load_state_dict replaces every param_group by the checkpoint's: a GroupedAdam checkpoint carries lr / betas /
        eps only, and torch.optim.Adam's groups also hold its implementation switches (fused, capturable, weight_decay, ...) -- a checkpoint
        of one kind left the other without them.  The groups keep this optimiser's own keys and take the checkpoint's values of the
        optimisation state (learning rates, betas, eps); a device learning rate (graph mode) stays the device tensor the update reads."""
        taken = ("lr", "initial_lr", "betas", "eps")
        groups = []
        for g, ng in zip(self.optimizer.param_groups, sd["param_groups"]):
            m = {k: v for k, v in g.items() if k != "params"}
            for k in taken:
                if k not in ng:
                    continue
                if torch.is_tensor(m.get(k)):
                    m[k].fill_(float(ng[k]))
                else:
                    m[k] = float(ng[k]) if torch.is_tensor(ng[k]) else ng[k]
            m["params"] = ng["params"]
            groups.append(m)
        assert len(groups) == len(sd["param_groups"]) == len(self.optimizer.param_groups)
        self.optimizer.load_state_dict({"state": sd["state"], "param_groups": groups})

    def _forget_skips(self, total, per):
        """A checkpoint of a run that skipped steps on the device, loaded into an optimiser that cannot (capturable GroupedAdam,
        torch.optim.Adam): its step counters and schedule become those of the run that never drew the skipped steps -- what the update
        kernel formed for them (include/fpcdr.h, fpcdr_adam_params.skipped).  Each tensor's step count loses its own skips, the scheduler's
        epoch the total, and the groups' current learning rates (device tensors in graph mode) follow the epoch."""
        for p, k in zip(self.params, per):
            st = self.optimizer.state.get(p, {})
            if k and 'step' in st:
                st['step'] = st['step'] - k
        sch = self.scheduler
        sch.last_epoch -= total
        lrs = [base * lmbda(sch.last_epoch) for base, lmbda in zip(sch.base_lrs, sch.lr_lambdas)]
        for g, lr in zip(self.optimizer.param_groups, lrs):
            if torch.is_tensor(g['lr']):
                g['lr'].fill_(float(lr))
            else:
                g['lr'] = lr
        sch._last_lr = [g['lr'].clone() if torch.is_tensor(g['lr']) else g['lr'] for g in self.optimizer.param_groups]

    def save_checkpoint(self, path):
        torch.save(self.state_dict(), path)

    def load_checkpoint(self, path):
        self.load_state_dict(torch.load(path, map_location=self.device, weights_only=False))

    def save_config(self, directory, extra=None):
        """config.txt in the reference's format (fit.py:651-657): one "key: 'value'" line per setting."""
        os.makedirs(directory, exist_ok=True)
        args = dict(self.cfg.__dict__)
        args.update(extra or {})
        with open(os.path.join(directory, "config.txt"), "w") as f:
            for k, v in args.items():
                f.write(f"{k}: '{v}'\n")

    def gather_result(self):
        """The per-frame final meshes [F,3V] of ALL ranks (every rank holds only its own frames' rows of self.result):
        one all-gather of the contiguous shards.  Collective: every rank must call it."""
        if self.world == 1:
            return self.result
        import torch.distributed as tdist
        assert tdist.is_initialized(), "world > 1 needs an initialised process group (dist.init)"
        shards = [torch.empty_like(self.result[self.frame_lo:self.frame_hi]) for _ in range(self.world)]
        tdist.all_gather(shards, self.result[self.frame_lo:self.frame_hi].contiguous())
        return torch.cat(shards, dim=0)       # contiguous, equal shards in rank order = frame order

    def save(self, directory):
        """Result files in the reference's layout (fit.py:235-286): result/{i}.obj, texture.png, pose.json.
        With several ranks the shards are gathered first (collective) and rank 0 writes."""
        result = self.gather_result()
        if self.rank != 0:
            return
        write_result(directory, result.cpu().numpy(), self.uv.cpu().numpy(), face_lines(self.sc.pos_idx, self.sc.uv_idx),
                     self.tex_opt.detach().cpu().numpy(), self.per_frame_t.detach().cpu().tolist(), self.per_frame_q.detach().cpu().tolist())
        if self._exposure_total is not None:      # (only then: the files of a fit that never equalised stay byte for byte what they were)
            self.save_exposure(directory)

    def save_exposure(self, directory):
        """<directory>/exposure.json: per camera name the composite table 'lut' (256 bytes: capture byte -> the byte the fit saw) and, of the
        last equalise_exposure call, 'gain' = g, 'offset' = b_common - g b (new byte ~ gain * byte + offset) and 'rho'; null where this
        Fitter made no fit of its own (a table loaded from a checkpoint) or the camera was not usable."""
        total = identity_lut(len(self.cam_idxs)) if self._exposure_total is None else self._exposure_total
        fitted = self._exposure_fit
        num = lambda v: float(v) if np.isfinite(v) else None
        rec = {}
        for j, c in enumerate(self.cam_idxs):
            gain = offset = rho = None
            if fitted is not None:
                rho = num(fitted['rho'][j])
                if fitted['usable'][j]:
                    gain = num(fitted['g'][j])
                    offset = num(fitted['b_common'] - fitted['g'][j] * fitted['b'][j])
            rec[str(self.sc.cams[c].get('cam', c))] = {'gain': gain, 'offset': offset, 'rho': rho, 'lut': [int(v) for v in total[j]]}
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "exposure.json"), "w", encoding="utf-8") as f:
            json.dump(rec, f, sort_keys=True, indent=1)


def face_lines(pos_idx, uv_idx):
    """The 'f v/vt v/vt v/vt' lines of an OBJ (1-based).  The reference copies them from a faces.txt it expects in the result directory
    (fit.py:252-257); the build writes them from the index buffers."""
    return ["f " + " ".join(f"{int(v) + 1}/{int(t) + 1}" for v, t in zip(fv, ft)) + "\n" for fv, ft in zip(pos_idx, uv_idx)]


def write_result(directory, meshes, uv, faces, texture, translation, rotation):
    """The files of the reference's save() (fit.py:235-286), byte for byte (tests/golden/save_golden.json holds what the reference's own
    function wrote): <directory>/result/{i}.obj -- 'v x y z' per vertex, 'vt u v' per uv vertex, then the face lines --, pose.json and
    texture.png.  meshes [F,3V] and uv [Vt,2] float32 arrays, translation / rotation nested lists.
    Numbers: the reference formats 0-dim torch tensors, i.e. Python floats -- the float32 value widened to double and printed with
    repr() ('0.10000000149011612', not numpy's shortest float32 form '0.1')."""
    from PIL import Image
    directory = os.path.join(directory, "result")
    os.makedirs(directory, exist_ok=True)
    uv_txt = "".join(f"vt {float(u[0])} {float(u[1])}\n" for u in np.asarray(uv, dtype=np.float32))
    for i, mesh in enumerate(np.asarray(meshes, dtype=np.float32)):
        with open(os.path.join(directory, f"{i}.obj"), "w") as f:
            for v in mesh.reshape(-1, 3):
                f.write(f"v {float(v[0])} {float(v[1])} {float(v[2])}\n")
            f.write(uv_txt)
            f.writelines(faces)
    tex = np.asarray(texture)
    # the reference casts (flip(tex) * 255) straight to uint8 (fit.py:268), which WRAPS values outside [0,255]
    # (an unconstrained Adam texture can leave the range): reproduced via int64 so the wrap is defined behaviour
    img = (np.flip(tex, 0) * 255).astype(np.int64).astype(np.uint8)
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(os.path.join(directory, "texture.png"))
    with open(os.path.join(directory, "pose.json"), "w", encoding="utf-8") as f:
        json.dump({'translation': translation, 'rotation': rotation}, f, separators=(',', ':'), sort_keys=True, indent=4)


# ----------------------------------------------------------------------------------------------
def smoke_step(sc, device='cuda:0', cams=(0, 4), mode='prior', m3_init=None):
    """One small forward + backward of the whole hot path (used by __graft_entry__.smoke and the tests).
    Starts from a perturbed state so that every gradient is non-trivial; `m3_init` [3V,F] fills the learned basis of the
    'free' / 'combined' modes (zero in the reference's start state, which would leave m1 / m2 without gradient)."""
    cfg = FitConfig(max_iter=100, cam_idxs=tuple(cams), mode=mode, weight_laplacian=0.0, fused_loss=True)
    targets = smoke_targets(sc, cams)
    ft = Fitter(sc, cfg, device=device, targets=targets.to(device))
    with torch.no_grad():
        K, F = ft.maps_intermediate['local'].shape
        ft.maps['local'].copy_(torch.eye(F, device=ft.device))
        ft.maps_intermediate['local'].copy_(0.5 * torch.tensor(sc.weights_gt, device=ft.device).t())
        ft.per_frame_t.copy_(0.5 * torch.tensor(sc.t_gt, device=ft.device))
        if m3_init is not None:
            ft.m3.copy_(m3_init.to(ft.device))
    if mode == 'combined':      # as after the switch of fit.py:603-608
        for m in (ft.m1, ft.m2, ft.m3):
            m.requires_grad = True
    frame_ids = torch.arange(0, F, device=ft.device)
    Nc = len(ft.cam_idxs)
    verts = ft.vertices(frame_ids).reshape(F, -1, 3)
    pos_clip = camera.transform_clip(ft.mvp(frame_ids), verts)
    pos_clip.retain_grad()
    colour, rast = render_from_clip(ft.glctx, pos_clip, ft.pos_idx, ft.uv, ft.uv_idx, ft.tex_opt, ft.resolution, False, 0)
    ref = ft.targets.reshape(F * Nc, *ft.resolution)
    sum_sq, g_colour = pixel_loss_fused(colour, rast, ref)
    ft.optimizer.zero_grad(set_to_none=False)
    torch.autograd.backward([colour], [g_colour])
    loss = sum_sq[0].to(torch.float32) / colour.numel()
    with torch.no_grad():
        image = torch.where(rast[..., 3:] > 0, colour, torch.tensor(BACKGROUND, device=ft.device))
    # the same clip positions through the fused objective, the form the fit loop runs (two C-ABI calls)
    pc = pos_clip.detach().clone().requires_grad_(True)
    tex_f = ft.tex_opt.detach().clone().requires_grad_(True)
    loss_f = dr.pixel_objective(ft.glctx, pc, ft.pos_idx, ft.uv, ft.uv_idx, tex_f, ref, ft.resolution)
    loss_f.backward()

    def g(t):
        return t.grad.clone() if t.grad is not None else None

    return {'loss': loss.detach(), 'ids': rast[..., 3].to(torch.int32), 'image': image.detach(),
            'loss_fused': loss_f.detach(), 'grad_pos_clip_fused': pc.grad.clone(), 'grad_tex_fused': tex_f.grad.clone(),
            'pos_clip': pos_clip.detach(), 'grad_pos_clip': pos_clip.grad.clone(),
            'grad_w': g(ft.maps_intermediate['local']), 'grad_M1': g(ft.maps['local']), 'grad_m1': g(ft.m1), 'grad_m2': g(ft.m2),
            'grad_m3': g(ft.m3), 'grad_tex': ft.tex_opt.grad.clone(),
            'grad_pose': torch.cat([ft.per_frame_t.grad.reshape(-1), ft.per_frame_q.grad.reshape(-1),
                                    ft.t_opt.grad.reshape(-1), ft.q_opt.grad.reshape(-1)])}


def smoke_targets(sc, cams):
    """Deterministic stand-in reference images for smoke_step: a smooth 8-bit pattern (no renderer involved,
    so the HIP path and the oracle are compared on identical targets)."""
    H, W = sc.resolution
    F = sc.n_frames
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    imgs = np.zeros((F, len(cams), H, W), dtype=np.uint8)
    for f in range(F):
        for c in range(len(cams)):
            imgs[f, c] = np.clip(70 + 60 * np.sin(0.05 * xx + 0.3 * f) * np.cos(0.07 * yy + 0.5 * c), 0, 140).astype(np.uint8)
    return torch.from_numpy(imgs)

"""
The texture's prior ("Texture prior rule"; device code csrc/tex_prior.hip): smoothness over neighbouring texels and a hold
to an anchor texture (texture_prior), the maps that weight them (load_texel_weights, chart_map) and the checks of FitConfig's options
that need no GPU.  fit.py imports these names: fit.texture_prior, fit.chart_map, ... are the documented spelling.
"""
import os

import numpy as np
import torch

from . import ops as dr
from .mesh_reg import _check_item_weights, _inv_scale, _penalty


def tex_prior_inv_scale(scale):
    """fpcdr_tex_prior's inv_c for a scale in texture units, 0..1 (mesh_reg._inv_scale: 0.0 for None, or ValueError; a bool is refused)."""
    return _inv_scale(scale, "the texture prior's", refuse_bool=True)


def _check_weight(name, w):
    try:
        v = float(w)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number (got {w!r})")
    if isinstance(w, bool) or not (np.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and not negative (got {w!r})")
    return v


class _texture_prior(_penalty):
    """w_smooth * smoothness + w_anchor * anchor with its gradient from ONE call (fpcdr_tex_prior): every texel gathers its four
    neighbours, so the gradient for a unit upstream is always made in forward(); backward() is _penalty's.  .part [2] on the returned
    value's grad_fn is not kept: ops.tex_prior_call returns it to callers that want the breakdown."""

    @staticmethod
    def forward(ctx, tex, anchor, smooth_w, anchor_w, inv_c, w_smooth, w_anchor, unit=False, acc=None):
        ctx.n_inputs, ctx.unit = 9, bool(unit)
        out, _, g = dr.tex_prior_call(tex, w_smooth, w_anchor, anchor, smooth_w, anchor_w, inv_c, want_grad=ctx.needs_input_grad[0], acc=acc)
        if g is not None:
            ctx.save_for_backward(g)
        return out


def _check_map(name, m, tex, live):
    Ht, Wt = int(tex.shape[0]), int(tex.shape[1])
    if not torch.is_tensor(m) or m.dtype != torch.float32 or tuple(m.shape) != (Ht, Wt) or m.device != tex.device:
        raise ValueError(f"texture_prior: {name} must be a float32 tensor [{Ht},{Wt}] on the device of tex")
    if live and not bool((torch.isfinite(m) & (m >= 0)).all()):
        raise ValueError(f"texture_prior: {name} must be finite and not negative")
    return m.detach().contiguous()


def texture_prior(tex, w_smooth, w_anchor, anchor=None, smooth_weights=None, anchor_weights=None, scale=None, eager_grad=False,
                  unit_upstream=False, acc=None, validate=True):
    """w_smooth * part[0] + w_anchor * part[1] of the texture tex [Ht,Wt,C] float32, C in 1..4 ("Texture prior rule"):
      part[0] = 1 / (Ht Wt) * sum over the pairs of horizontally and vertically neighbouring texels (none across the border) of
                min(smooth_weights[p], smooth_weights[q]) * rho(|t_p - t_q|^2), the channels sharing their edges; rho(s) = s, or with a
                scale c (texture units, 0..1) the Charbonnier form 2 c^2 (sqrt(1 + s / c^2) - 1): quadratic below c, linear above it
      part[1] = 1 / (Ht Wt) * sum over the texels of anchor_weights[p] * |t_p - anchor_p|^2   (0 without an anchor)
    anchor [Ht,Wt,C] and the maps [Ht,Wt]: float32 on the device of tex, the maps finite and >= 0 (None: 1); they are constants and get
    no gradient.  A pair or texel of weight 0 contributes exactly 0, whatever the texel holds.  The modes are stretch_penalty's: the
    one call makes the gradient with the value in every mode; eager_grad with unit_upstream hands the buffer over as it is (the caller
    guarantees d loss / d value = 1).  acc: two float64 zeros on the device, left zero again (None: a fresh buffer per call).
    validate: check the maps' values on the host (a read-back each; skipped while a stream is capturing)."""
    w_smooth, w_anchor = _check_weight("texture_prior: w_smooth", w_smooth), _check_weight("texture_prior: w_anchor", w_anchor)
    inv_c = tex_prior_inv_scale(scale)
    if not torch.is_tensor(tex) or tex.dim() != 3 or tex.dtype != torch.float32 or not 1 <= tex.shape[2] <= 4 or tex.shape[0] < 1 or tex.shape[1] < 1:
        raise ValueError(f"texture_prior: tex must be float32 [Ht,Wt,C] with C in 1..4 (got "
                         f"{getattr(tex, 'dtype', type(tex))} {tuple(getattr(tex, 'shape', ()))})")
    live = validate and not (tex.is_cuda and torch.cuda.is_current_stream_capturing())
    if anchor is not None:
        if not torch.is_tensor(anchor) or anchor.dtype != torch.float32 or tuple(anchor.shape) != tuple(tex.shape) or anchor.device != tex.device:
            raise ValueError(f"texture_prior: anchor must be a float32 tensor {tuple(tex.shape)} on the device of tex")
        anchor = anchor.detach().contiguous()
    elif anchor_weights is not None:
        raise ValueError("texture_prior: anchor_weights without an anchor")
    if smooth_weights is not None:
        smooth_weights = _check_map("smooth_weights", smooth_weights, tex, live)
    if anchor_weights is not None:
        anchor_weights = _check_map("anchor_weights", anchor_weights, tex, live)
    if not tex.is_cuda:
        raise RuntimeError("the texture prior runs on the GPU only (fpcdr_tex_prior); there is no CPU fallback")
    return _texture_prior.apply(tex.contiguous(), anchor, smooth_weights, anchor_weights, inv_c, w_smooth, w_anchor,
                                bool(eager_grad and unit_upstream), acc)


def load_texel_weights(weights, Ht, Wt, option):
    """FitConfig.<option> -- an array-like [Ht,Wt], or the path of an 8-bit image of Wt x Ht pixels read as byte / 255 (the first channel
    of a multi-channel file; its top row is the texture's LAST row, the orientation of the texture.png a fit writes) -- as a float32
    array [Ht,Wt], or ValueError: another shape, an entry that is not finite or is negative.  ('chart' is the Fitter's: it needs the mesh.)"""
    if isinstance(weights, (str, os.PathLike)):
        from .data import load_raw_image
        try:
            w = np.flip(load_raw_image(weights), 0).astype(np.float64) / 255.0
        except (OSError, ValueError) as e:
            raise ValueError(f"FitConfig.{option}: cannot read {weights}: {e}")
    else:
        try:
            w = np.asarray(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"FitConfig.{option} must be an array-like [{Ht},{Wt}], the path of an 8-bit image, or 'chart'")
    return _check_item_weights(w, (Ht, Wt), option, 'texel')


def dilate3(cover):
    """The 3 x 3 maximum of a [Ht,Wt] map (no wrap at the border), torch or numpy alike in meaning: a texel is on when it or one of its
    eight neighbours is."""
    c = cover[None, None].to(torch.float32)
    return torch.nn.functional.max_pool2d(c, 3, stride=1, padding=1)[0, 0]


def chart_map(uv, uv_idx, Ht, Wt):
    """The texels the render can read, float32 [Ht,Wt] of 0 / 1 on the device of uv: the UV triangles (uv [Vt,2] float32, uv_idx [T,3]
    int32) rasterised at the texture's own resolution -- positions (2u - 1, 2v - 1, 0, 1), so that a pixel centre is a texel centre: the
    sampler's x = u Wt - 0.5 against the rasteriser's (2 x + 1) / Wt - 1 -- and the coverage grown by one texel (dilate3), so that the
    bilinear taps of a chart's border pixels are inside.  Assumes UVs in [0,1] (the sampler wraps, the atlas does not); charts closer than
    two texels to each other become one region, and their texels are coupled by the smoothness term."""
    uv = uv.detach().to(torch.float32)
    pos = torch.stack([2.0 * uv[:, 0] - 1.0, 2.0 * uv[:, 1] - 1.0, torch.zeros_like(uv[:, 0]), torch.ones_like(uv[:, 0])], dim=1)
    glctx = dr.RasterizeGLContext(output_db=False, device=uv.device)
    with torch.no_grad():
        rast, _ = dr.rasterize(glctx, pos[None].contiguous(), uv_idx.to(torch.int32).contiguous(), resolution=(int(Ht), int(Wt)))
        return dilate3(rast[0, ..., 3] > 0).contiguous()


def check_tex_prior_options(cfg):
    """What FitConfig's texture-prior fields ask of each other (FitConfig.__post_init__), or ValueError.  Needs no GPU."""
    ws = _check_weight("FitConfig.weight_tex_smooth", cfg.weight_tex_smooth)
    wa = _check_weight("FitConfig.weight_tex_anchor", cfg.weight_tex_anchor)
    try:
        tex_prior_inv_scale(cfg.tex_smooth_scale)
    except ValueError as e:
        raise ValueError(f"FitConfig.tex_smooth_scale: {e}")
    if (ws > 0 or wa > 0) and not cfg.optimize_texture:
        raise ValueError("FitConfig.weight_tex_smooth / weight_tex_anchor > 0 need optimize_texture=True: the prior acts on the texture "
                         "being optimised")

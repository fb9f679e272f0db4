"""
nvdiffrast-compatible operator API over the gfx950 HIP kernels (C ABI: include/fpcdr.h).

The reference's fit loop calls exactly these names on `import nvdiffrast.torch as dr`
(reference src/torch/fit.py:13):

    dr.RasterizeGLContext(device='cuda')                                   fit.py:484
    dr.rasterize(glctx, pos_clip, pos_idx, resolution=(H, W))              fit.py:151
    dr.interpolate(uv[None], rast, uv_idx[, rast_db=..., diff_attrs='all']) fit.py:154, 157
    dr.texture(tex[None], texc[, texd], filter_mode=..., max_mip_level=..) fit.py:155, 158
    dr.antialias(colour, rast, pos_clip, pos_idx)                          fit.py:160

so `import fpc_diffrend_amd.ops as dr` lets the reference's render() (fit.py:134-162) run
unchanged.  Signatures, argument meaning, defaults and error behaviour follow nvdiffrast's
documented API; arguments the reference never passes are accepted with upstream defaults.
Instanced mode (pos [B,V,4]) and range mode (pos [V,4] + ranges [B,2]) are implemented.

PyTorch is plumbing here: it owns the HBM buffers (including kernel scratch, so lifetimes follow
autograd), supplies the stream, and runs autograd bookkeeping.  All pixel work happens in
libfpcdr.so; there is no CPU or eager-torch fallback.
"""
import ctypes
import functools
import weakref
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib

__all__ = ['RasterizeGLContext', 'RasterizeCudaContext', 'RasterizeHipContext', 'rasterize', 'interpolate', 'texture',
           'texture_construct_mip', 'antialias', 'antialias_construct_topology_hash', 'render_textured', 'pixel_objective', 'undistort_images', 'compare_images',
           'gaussian_taps', 'blurred_pixel_loss', 'normalised_pixel_loss', 'robust_pixel_loss', 'bake_accumulate', 'bake_resolve', 'downsample_images',
           'exposure_sums', 'apply_lut_u8']


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_tensor(name, t, dtype, dims=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor (got device {t.device}); the raster ops have no CPU path")
    if t.dtype != dtype:
        raise ValueError(f"{name} must have dtype {dtype} (got {t.dtype})")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name} must have {dims} dimensions (got shape {tuple(t.shape)})")


# ----------------------------------------------------------------------------------------------
# region hints (include/fpcdr.h): which 32 x 32-pixel bins of an image tensor are known to be empty
# ----------------------------------------------------------------------------------------------
# rasterize() leaves a byte map of the bins no triangle touches.  It rides with the tensors of the operator chain of the
# reference's render() (fit.py:151-160) -- rast ('rast': zero there), the interpolated texture coordinates ('zero') and the
# sampled colour ('const': one known value there) -- in this registry, keyed by the tensor OBJECT: a consumer that is handed
# the very tensor an operator returned, unmodified (same object, same version counter), does not read it in empty bins.
# Anything else (a clone, a slice, an in-place edit, a tensor from elsewhere) simply finds no hint and takes the dense path.
# Results are identical either way; set `region_hints = False` to switch the mechanism off.
region_hints = True
_hints = {}


def _tag(t, hint, kind, const=None):
    """Register the hint of a tensor THIS library has just produced (a fresh allocation that owns its storage)."""
    if len(_hints) > 256:
        for k in [k for k, e in _hints.items() if e[0]() is None]:
            del _hints[k]
    st = t.untyped_storage()
    _hints[t.data_ptr()] = (weakref.ref(t), t._version, tuple(t.shape), hint, kind, const, st.data_ptr(), st.nbytes())


def _hint_of(t, kind):
    """The hint of `t`, or None.  A hint is honoured only for the very tensor object an operator of this library returned, owning the
    storage the library allocated for it (not a view, not re-pointed with set_() / .data = ...), with an unchanged version counter --
    every in-place torch operation bumps it.  What no host-side check can see is a write that bypasses autograd's bookkeeping: a
    foreign kernel, or `t.data.copy_(...)`; such a caller must call ops.drop_hints(t) (or work under ops.no_region_hints())."""
    if not region_hints:
        return None
    e = _hints.get(t.data_ptr())
    if e is None:
        return None
    ref, version, shape, hint, k, const, st_ptr, st_bytes = e
    if ref() is not t or t._version != version or tuple(t.shape) != shape or k != kind:
        return None
    st = t.untyped_storage()
    if t._base is not None or st.data_ptr() != st_ptr or st.nbytes() != st_bytes or t.storage_offset() != 0 or not t.is_contiguous():
        return None
    return hint, const


def drop_hints(*tensors):
    """Forget the region hints of these tensors (call it after writing to one of them behind torch's back)."""
    for t in tensors:
        _hints.pop(t.data_ptr(), None)


class no_region_hints:
    """Context manager: the operators inside take the dense path (module switch `region_hints` restored on exit)."""

    def __enter__(self):
        global region_hints
        self._old, region_hints = region_hints, False

    def __exit__(self, *exc):
        global region_hints
        region_hints = self._old


def _n_bins(B, H, W):
    """32 x 32-pixel bins of a batch of B images."""
    return B * ((H + _lib.OCC_BIN - 1) // _lib.OCC_BIN) * ((W + _lib.OCC_BIN - 1) // _lib.OCC_BIN)


def _hint_bytes(B, H, W):
    return 2 * _n_bins(B, H, W)     # FPCDR_HINT_BYTES


# ----------------------------------------------------------------------------------------------
# contexts
# ----------------------------------------------------------------------------------------------

class RasterizeHipContext:
    """Rasteriser context.  Stateless on the device side (the library keeps no state between calls);
    holds the device and whether rast_db is produced.  `RasterizeGLContext` / `RasterizeCudaContext`
    are aliases so reference code constructing either keeps working (reference fit.py:484)."""

    def __init__(self, output_db=True, mode='automatic', device=None):
        assert output_db is True or output_db is False
        assert mode in ('automatic', 'manual')
        self.output_db = output_db
        self.mode = mode
        if device is None:
            self.device = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else None
        else:
            self.device = torch.device(device)
            if self.device.type == 'cuda' and self.device.index is None and torch.cuda.is_available():
                self.device = torch.device('cuda', torch.cuda.current_device())
        _lib.load()  # fail loudly here if the HIP extension is missing

    # nvdiffrast GL-context API surface (no-ops: there is no GL context to bind)
    def set_context(self):
        pass

    def release_context(self):
        pass


RasterizeGLContext = RasterizeHipContext
RasterizeCudaContext = RasterizeHipContext


# ----------------------------------------------------------------------------------------------
# rasterize
# ----------------------------------------------------------------------------------------------

class _rasterize_func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, H, W, output_db, grad_db, hint, ranges):
        lib = _lib.load()
        B, V, _ = pos.shape
        T = tri.shape[0]
        dev = pos.device
        rast = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev)
        rast_db = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev) if output_db else None
        scratch = torch.empty(lib.fpcdr_rasterize_scratch_bytes(B, T), dtype=torch.uint8, device=dev)
        p = _lib.RasterizeFwd(pos=_ptr(pos), tri=_ptr(tri), B=B, V=V, T=T, H=H, W=W, scratch=_ptr(scratch),
                              rast=_ptr(rast), rast_db=_ptr(rast_db), hint=_ptr(hint), ranges=_ptr(ranges))
        _lib.call("fpcdr_rasterize_fwd", ctypes.byref(p), _stream())
        ctx.save_for_backward(pos, tri, rast)
        ctx.hint = hint
        ctx.grad_db = bool(grad_db and output_db)
        if rast_db is None:
            rast_db = torch.zeros(B, H, W, 0, dtype=torch.float32, device=dev)
        return rast, rast_db

    @staticmethod
    def backward(ctx, dy, ddb):
        lib = _lib.load()
        pos, tri, rast = ctx.saved_tensors
        B, V, _ = pos.shape
        _, H, W, _ = rast.shape
        g_pos = torch.zeros_like(pos)
        dy = dy.contiguous()
        ddb = ddb.contiguous() if (ctx.grad_db and ddb is not None and ddb.numel() > 0) else None
        p = _lib.RasterizeBwd(pos=_ptr(pos), tri=_ptr(tri), rast=_ptr(rast), dy=_ptr(dy), ddb=_ptr(ddb), B=B, V=V,
                              T=tri.shape[0], H=H, W=W, grad_pos=_ptr(g_pos), hint=_ptr(ctx.hint))
        _lib.call("fpcdr_rasterize_bwd", ctypes.byref(p), _stream())
        return g_pos, None, None, None, None, None, None, None


def rasterize(glctx, pos, tri, resolution, ranges=None, grad_db=True):
    """Rasterize triangles.  pos [B,V,4] clip space f32, tri [T,3] i32, resolution (H, W).

    Returns (rast [B,H,W,4] = (u, v, z/w, triangle_id + 1), rast_db [B,H,W,4] = (du/dX, du/dY, dv/dX, dv/dY)).
    """
    assert isinstance(glctx, RasterizeHipContext), "glctx must be a Rasterize*Context"
    ranges_dev = None
    if isinstance(pos, torch.Tensor) and pos.dim() == 2:
        # range mode (nvdiffrast): one shared vertex array pos [V,4]; image b renders triangles ranges[b] = (first, count).
        # The vertex array is broadcast over the minibatch (its gradient is the sum over the images); the kernel only needs
        # to know which slice of `tri` each image draws.  Triangle ids in rast stay indices into `tri`.
        if ranges is None:
            raise ValueError("range mode (pos [V,4]) needs ranges [B,2]")
        ranges = torch.as_tensor(ranges)
        if ranges.dim() != 2 or ranges.shape[1] != 2 or ranges.shape[0] < 1 or ranges.dtype != torch.int32:
            raise ValueError("ranges must be an int32 tensor of shape [minibatch, 2]")
        r = ranges.cpu()
        if int(r.min()) < 0 or int((r[:, 0] + r[:, 1]).max()) > tri.shape[0]:
            raise ValueError("ranges reach outside the triangle tensor")
        ranges_dev = ranges.to(pos.device).contiguous()
        pos = pos[None].expand(ranges.shape[0], -1, -1)
    elif ranges is not None:
        raise ValueError("ranges is for range mode only (pos [V,4]); instanced mode takes pos [B,V,4]")
    assert grad_db is True or grad_db is False
    resolution = tuple(int(r) for r in resolution)
    assert len(resolution) == 2 and resolution[0] > 0 and resolution[1] > 0, "resolution must be (height, width)"
    _check_tensor('pos', pos, torch.float32, 3)
    _check_tensor('tri', tri, torch.int32, 2)
    if pos.shape[2] != 4 or pos.shape[0] < 1 or pos.shape[1] < 1:
        raise ValueError(f"pos must have shape [>0, >0, 4] (got {tuple(pos.shape)})")
    if tri.shape[1] != 3 or tri.shape[0] < 1:
        raise ValueError(f"tri must have shape [>0, 3] (got {tuple(tri.shape)})")
    if glctx.device is not None and pos.device != glctx.device:
        raise ValueError(f"pos is on {pos.device} but the context was created for {glctx.device}")
    hint = torch.empty(_hint_bytes(pos.shape[0], *resolution), dtype=torch.uint8, device=pos.device) if region_hints else None
    rast, rast_db = _rasterize_func.apply(pos.contiguous(), tri.contiguous(), resolution[0], resolution[1], glctx.output_db,
                                          grad_db, hint, ranges_dev)
    if hint is not None:
        _tag(rast, hint, 'rast')
    return rast, rast_db


# ----------------------------------------------------------------------------------------------
# fused render (extension; not part of the nvdiffrast surface)
# ----------------------------------------------------------------------------------------------

class _render_textured_func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, uv, uv_tri, tex, H, W, boundary):
        lib = _lib.load_twocall()      # (include/fpcdr_twocall.h: fpcdr_render_fwd / _bwd live in the second library)
        B, V, _ = pos.shape
        T = tri.shape[0]
        Ht, Wt, C = tex.shape
        dev = pos.device
        rast = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev)
        color = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
        scratch = torch.empty(lib.fpcdr_rasterize_scratch_bytes(B, T), dtype=torch.uint8, device=dev)
        tri_uv = uv[uv_tri.long()].contiguous()      # [T,3,2], static per mesh
        p = _lib.RenderFwd(pos=_ptr(pos), tri=_ptr(tri), B=B, V=V, T=T, H=H, W=W, scratch=_ptr(scratch), uv=_ptr(uv),
                           uv_tri=_ptr(uv_tri), Vt=uv.shape[0], tex=_ptr(tex), Ht=Ht, Wt=Wt, C=C, boundary_mode=boundary,
                           rast=_ptr(rast), color=_ptr(color), tri_uv=_ptr(tri_uv))
        _lib.call("fpcdr_render_fwd", ctypes.byref(p), _stream())
        ctx.save_for_backward(pos, tri, uv, uv_tri, tex, rast)
        ctx.boundary = boundary
        ctx.mark_non_differentiable(rast)
        return color, rast

    @staticmethod
    def backward(ctx, dy, _drast):
        pos, tri, uv, uv_tri, tex, rast = ctx.saved_tensors
        B, V, _ = pos.shape
        _, H, W, _ = rast.shape
        Ht, Wt, C = tex.shape
        g_pos = torch.zeros_like(pos) if ctx.needs_input_grad[0] else None
        g_tex = torch.zeros_like(tex) if ctx.needs_input_grad[4] else None
        if g_pos is None and g_tex is None:
            return (None,) * 8
        dy = dy.contiguous()
        p = _lib.RenderBwd(pos=_ptr(pos), tri=_ptr(tri), uv=_ptr(uv), uv_tri=_ptr(uv_tri), tex=_ptr(tex), rast=_ptr(rast),
                           dy=_ptr(dy), B=B, V=V, T=tri.shape[0], H=H, W=W, Vt=uv.shape[0], Ht=Ht, Wt=Wt, C=C,
                           boundary_mode=ctx.boundary, grad_pos=_ptr(g_pos), grad_tex=_ptr(g_tex), tri_uv=None)
        _lib.call("fpcdr_render_bwd", ctypes.byref(p), _stream())
        return g_pos, None, None, None, g_tex, None, None, None


def render_textured(glctx, pos, tri, uv, uv_tri, tex, resolution, boundary_mode='wrap'):
    """rasterize -> interpolate(uv) -> texture('linear') in one pass (the non-mip branch of the reference's render(),
    fit.py:151,157,158).  pos [B,V,4], tri [T,3], uv [Vt,2], uv_tri [T,3], tex [Ht,Wt,C].  Returns (colour [B,H,W,C],
    rast [B,H,W,4]); values equal the three separate calls, the texture-coordinate image never reaches HBM, and the
    backward pass scatters straight into grad_tex and grad_pos.  rast carries no gradient here (use `rasterize` for that)."""
    assert isinstance(glctx, RasterizeHipContext)
    _check_tensor('pos', pos, torch.float32, 3)
    _check_tensor('tri', tri, torch.int32, 2)
    _check_tensor('uv', uv, torch.float32, 2)
    _check_tensor('uv_tri', uv_tri, torch.int32, 2)
    _check_tensor('tex', tex, torch.float32, 3)
    if uv.shape[1] != 2 or uv_tri.shape != tri.shape or pos.shape[2] != 4 or tri.shape[1] != 3:
        raise ValueError("shapes: pos [B,V,4], tri [T,3], uv [Vt,2], uv_tri [T,3], tex [Ht,Wt,C]")
    if boundary_mode not in _lib.BOUNDARY:
        raise ValueError(f"unknown boundary_mode '{boundary_mode}'")
    H, W = int(resolution[0]), int(resolution[1])
    return _render_textured_func.apply(pos.contiguous(), tri.contiguous(), uv.contiguous(), uv_tri.contiguous(),
                                       tex.contiguous(), H, W, _lib.BOUNDARY[boundary_mode])


class _ListHints:
    """Launch-size hints for the list kernels of the sparse objective (include/fpcdr.h: cap_bins / cap_fix / cap_bwd).
    Every forward call leaves the number of bins each of its three list kernels visited in the occupancy buffer; they are
    copied to pinned host memory asynchronously and the NEXT call on a batch of the same shape sizes its launches from them
    (+ 12 % margin) -- never waiting: a copy that has not landed yet simply means "no hint".  Results do not depend on the
    hints (entries beyond one are swept up on the device)."""

    def __init__(self):
        self.host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.event = None
        self.caps = (0, 0, 0)       # bins, fix, bwd

    def poll(self):
        if self.event is not None and self.event.query():
            n_bwd, _, n_bins, n_fix = (int(v) for v in self.host.tolist())
            self.caps = tuple(n + max(256, n // 8) if n > 0 else 0 for n in (n_bins, n_fix, n_bwd))
            self.event = None
        return self.caps

    def update(self, counts_dev):
        if self.event is not None or torch.cuda.is_current_stream_capturing():
            return                  # a copy is still in flight / no host read-back from inside a HIP graph
        self.host.copy_(counts_dev, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()


class _MappedHints:
    """The same for the one-pass objective, without a copy in the stream: the call's last kernel writes the counters straight into
    pinned host memory (fpcdr_objective_params.counts_out) as a sequence lock -- the call's sequence number in front of AND behind them;
    poll() uses whatever has landed (a device-to-host copy per step was a blit kernel between two barriers: ~20 us of the step's serial tail)."""

    def __init__(self):
        self.host = torch.zeros(8, dtype=torch.int32)
        if torch.cuda.is_available():      # (device-writable host memory; without a GPU only the bookkeeping below can be exercised)
            self.host = self.host.pin_memory()
        self.seq = 0
        self.seen = 0
        self.caps = (0, 0, 0)       # live bins, occupied bins, bins with a deferred pixel
        self.frozen = False         # tests: keep `caps` as set
        self.sil_bins = -1          # bins that took a record slot in the last call seen (compact records; -1: none seen yet)
        self.slots = 0              # record slots the next call gets (tests may pin it with `frozen`)
        self.overflowed = None      # sequence number of the newest call seen at or before which a call ran out of record slots
        self.overflow_count = 0     # the device's cumulative count of such calls, as last read (host[5]: only clear_hints resets it)
        self.skipped_calls = 0      # ... of them, calls whose caller took the device-side flag (skip_out): handled, not raised

    def poll(self):
        if self.frozen:
            self._poll_overflow(int(self.host[4]))
            return self.caps
        # include/fpcdr.h, counts_out: the device writes [6] = seq, fences, the counters, fences, [4] = seq.  Read the other way round --
        # [4], the counters, [6] -- the counters are ONE call's iff both numbers agree: a later call that has started to write has
        # already changed [6], one that has not finished has not yet changed [4]
        end = int(self.host[4])
        n_def, n_sil, n_bins, n_occ = (int(v) for v in self.host[:4].tolist())
        slots_valid = int(self.host[7])
        begin = int(self.host[6])
        if begin == end and end != self.seen:
            self.seen = end
            self.caps = tuple(n + max(256, n // 8) if n > 0 else 0 for n in (n_bins, n_occ, n_def))
            if slots_valid:      # (a dense call takes no record slots: its zero says nothing about the demand)
                self.sil_bins = n_sil
                self.slots = n_sil + max(RECORD_SLOT_MARGIN, n_sil // 2)
        self._poll_overflow(end)
        return self.caps

    def _poll_overflow(self, seq):
        # cumulative on the device: an overflow in call N is still there when call N + 1 has finished before this poll
        n_over = int(self.host[5])
        if n_over != self.overflow_count:
            self.overflow_count = n_over
            self.overflowed = seq

    def next_seq(self):
        self.seq = self.seq % 0x7ffffff0 + 1
        return self.seq

    @staticmethod
    def plan(hints, nbins, capturing, has_skip_out, record_slots, n_pixels):
        """What a one-pass call on a batch of `nbins` bins and `n_pixels` pixels does with its launch sizes, its counters and its records
        of DEFERRED pixels (a pixel pair at a silhouette; a few per cent of the covered pixels -- nothing else of the image ever exists in
        HBM): a _CallPlan.  hints: the shape's record, or None (launch_hints=False, first use of a shape under capture) -- caps 0, nothing
        reported, records as the caller says or by pixel.  capturing: a graph replays fixed launch sizes and cannot be waited for --
        nothing is reported, a pending overflow stays pending, records by pixel.  Host logic only: no device, no stream."""
        given = record_slots is not None
        if hints is None:
            return _CallPlan((0, 0, 0), None, False, int(record_slots) if given else 0, n_pixels)
        # a batch of few bins -- one image of the reference's run shape has 1 900 -- is launched at its full size whatever the hint says: a
        # sized launch has a strided sweep launched behind it (four per call, 4.6 us each), and the dead workgroups of a full launch cost less
        caps = hints.poll()
        if nbins <= SMALL_BATCH_BINS and not hints.frozen:
            caps = (0, 0, 0)
        seq = None if capturing else hints.next_seq()
        if hints.overflowed is not None and not capturing:
            # an earlier call on this shape ran out of record slots: its value was NaN and its gradients incomplete.  A caller that hands
            # over skip_out had the device flag of that very call (Fitter: the update was skipped on the device) -- nothing to raise; the
            # demand the call counted (it keeps counting beyond the pool) has sized this call.  Anybody else learns it here.
            over, hints.overflowed = hints.overflowed, None
            if not has_skip_out:
                hints.sil_bins = -1      # (re-count in front of the next call)
                raise RuntimeError(f"pixel_objective: a call on this batch shape (sequence number <= {over}) ran out of record slots (the "
                                   "take's silhouette grew by more than half within one step); its value was NaN and its gradients "
                                   "incomplete -- repeat the step, or pass skip_out= and skip the update as Fitter does")
            hints.skipped_calls += 1
        # large batches: COMPACT, a slot of 1 024 records for every bin that shows a silhouette triangle, sized from the last call on the
        # batch shape (24 B per pixel of the batch otherwise: 14 GB at 288 full-HD images, for 0.2 % of them); the first call on a shape
        # asks the rasteriser for the count (one extra rasterisation and a host wait, once per shape)
        compact = not given and COMPACT_RECORDS and not capturing and nbins > SMALL_BATCH_BINS
        count = compact and hints.sil_bins < 0 and not hints.frozen
        slots = int(record_slots) if given else max(hints.slots, 1) if compact else 0
        return _CallPlan(caps, seq, count, slots, n_pixels)

    def counted(self, plan):
        """The plan of the call proper once the count-only call `plan` asked for has landed (the caller has waited for the stream)."""
        caps, seq = self.poll(), self.next_seq()
        if self.sil_bins < 0:
            raise RuntimeError("pixel_objective: the counting call reported nothing")
        return _CallPlan(caps, seq, False, max(self.slots, 1), plan.n_pixels)


class _CallPlan(namedtuple('_CallPlan', 'caps seq count slots n_pixels')):
    """_MappedHints.plan's answer: caps (cap_bins, cap_occ, cap_def); seq, the counts_seq with which counts_out is handed over, or None:
    nothing reported; count: a count-only call comes first, then _MappedHints.counted; slots: rec_slots, 0 = records by pixel."""
    __slots__ = ()

    @property
    def n_records(self):
        return self.slots * _lib.OCC_BIN * _lib.OCC_BIN if self.slots > 0 else self.n_pixels


_list_hints = {}
# Compact records (fpcdr_objective_params.rec_slots): a call gets 1.5 x the slots the last call on the batch shape used, at least this
# many more.  The slot demand is the number of occupied bins that show a silhouette triangle: it moves by a few per cent from one minibatch
# of a take to the next.  A call that runs out regardless says so itself -- NaN value, skip_out = 1 (include/fpcdr.h ABI v11): Fitter skips
# that update on the device --; a caller that did not hand over skip_out gets a RuntimeError at its next call on the shape.
RECORD_SLOT_MARGIN = 1024
COMPACT_RECORDS = True
SMALL_BATCH_BINS = 16384      # (eight full-HD images) batches up to this many 32 x 32 bins run their list kernels unhinted: see _pixel_objective_onepass


def _hints_for(key, cls):
    """The hint record of a batch shape, made on first use -- never under HIP-graph capture (its pinned allocation would be a
    hipHostMalloc inside the capture): a captured call simply runs unhinted then."""
    h = _list_hints.get(key)
    if h is None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return None
        h = _list_hints[key] = cls()
    return h


def clear_hints():
    """Forget every launch hint.  The objective's last kernel writes its counters into the records' pinned host memory through a raw
    pointer the allocator cannot see, so the device is drained first: dropping a record while a call is queued would return its block
    to the pinned cache with a write still in flight."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _list_hints.clear()


_objective_options = namedtuple('_objective_options', 'H W n_total bg boundary ref_bg_sumsq use_hints want_grad mip_levels sparse queued_backward '
                                'unit_upstream flags_out zero_extra bin_lists idp_out record_slots skip_out weights',
                                defaults=(True, False, False, None, None, True, None, None, None, None))
_objective_options.__doc__ = """What pixel_objective hands to either form's apply() beside its tensors, as ONE argument (nothing in it gets
a gradient).  Both forms read the first nine; sparse and queued_backward are the two-call form's, the rest the one-pass form's."""


def _background_share(ref, bg, ref_bg_sumsq, dev):
    """The plain objective's share of an all-background image, f64 []: the caller's ref_bg_sumsq, or computed here (it depends on ref alone)."""
    return (reference_background_sumsq(ref, bg).sum() if ref_bg_sumsq is None
            else torch.as_tensor(ref_bg_sumsq, device=dev)).to(torch.float64).contiguous()


def _wire_plan(p, hints, plan):
    """A _CallPlan's launch sizes and, when the call reports its counters, where to and under which number, into the struct p."""
    p.cap_bins, p.cap_occ, p.cap_def = plan.caps      # (live bins, occupied bins, bins with a deferred pixel)
    if plan.seq is not None:
        p.counts_out, p.counts_seq = hints.host.data_ptr(), plan.seq


def _mip_chain(p, tex, mip_levels, want_grad=False):
    """mip_levels = n: the reference's enable_mip branch inside the objective's kernels -- levels 1..n of tex [Ht,Wt,C] (built here, box
    filter as texture()) and, with want_grad, the buffers of their gradients, wired into the parameter struct p.  None: ([], [])."""
    if mip_levels is None:
        return [], []
    chain = _build_mips(tex[None], mip_levels)[1:]
    g_chain = [torch.empty_like(t) for t in chain] if want_grad else []
    _wire_mips(p, chain, g_chain)
    return chain, g_chain


class _pixel_objective_func(torch.autograd.Function):
    """The two-call form: mean over n_total of (ref - 255 * where(covered, antialias(render(pos, tex)), bg))^2 as three kernels."""

    @staticmethod
    def forward(ctx, pos, tex, *const):
        tri, adj, uv, uv_tri, ref, opt = const
        H, W, n_total, bg, boundary, sparse, mip_levels = opt.H, opt.W, opt.n_total, opt.bg, opt.boundary, opt.sparse, opt.mip_levels
        ctx.n_const = len(const)
        lib = _lib.load_twocall()      # (the two-call form: include/fpcdr_twocall.h, libfpcdr_twocall.so)
        B, V, _ = pos.shape
        T = tri.shape[0]
        Ht, Wt, C = tex.shape
        dev = pos.device
        rast = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev)
        color = torch.empty(B, H, W, C, dtype=torch.float32, device=dev)
        scratch = torch.empty(lib.fpcdr_rasterize_scratch_bytes(B, T), dtype=torch.uint8, device=dev)
        # sparse: 32x32-pixel bins that no triangle's bounding box touches are neither written nor read by the three
        # kernels; occ is the map of the others, ecol the colour of an empty pixel
        occ = torch.empty(lib.fpcdr_occ_bytes(B, H, W), dtype=torch.uint8, device=dev) if sparse else None
        ecol = torch.empty(4, dtype=torch.float32, device=dev) if sparse else None
        tri_uv = _cached_tri_uv(uv, uv_tri)          # [T,3,2], static per mesh: saves a dependent load per pixel
        p = _lib.RenderFwd(pos=_ptr(pos), tri=_ptr(tri), B=B, V=V, T=T, H=H, W=W, scratch=_ptr(scratch), uv=_ptr(uv),
                           uv_tri=_ptr(uv_tri), Vt=uv.shape[0], tex=_ptr(tex), Ht=Ht, Wt=Wt, C=C, boundary_mode=boundary,
                           rast=_ptr(rast), color=_ptr(color), tri_uv=_ptr(tri_uv), occ=_ptr(occ), empty_color=_ptr(ecol))
        chain, _ = _mip_chain(p, tex, mip_levels)
        g_aa = torch.empty_like(color)
        sil = torch.empty(B, T, dtype=torch.uint8, device=dev)
        nflag = lib.fpcdr_antialias_flags_bytes(B, H, W) // 8
        flags = torch.empty(nflag, dtype=torch.int64, device=dev)     # (sparse: zeroed by fpcdr_render_loss_fwd itself, inside its first kernel)
        acc = torch.zeros(_lib.LOSS_SLOTS, dtype=torch.float64, device=dev)
        q = _lib.AaLossFwd(color=_ptr(color), rast=_ptr(rast), pos=_ptr(pos), tri=_ptr(tri), adj=_ptr(adj), ref=_ptr(ref), B=B,
                           H=H, W=W, C=C, V=V, T=T, bg=bg, color_scale=255.0, grad_scale=1.0 / n_total, sil=_ptr(sil),
                           flags=_ptr(flags), grad_aa=_ptr(g_aa), occ=_ptr(occ), empty_color=_ptr(ecol), loss_sum=_ptr(acc))
        ctx.cap_bwd = 0
        ctx.hint_update = None
        if sparse:
            # one call: the rasteriser settles every pixel antialiasing cannot touch, a second kernel the candidates it marks
            cmask = torch.empty(lib.fpcdr_cmask_bytes(B, H, W), dtype=torch.uint8, device=dev)
            hints = _hints_for((dev.index, B, V, T, H, W), _ListHints) if opt.use_hints else None
            if hints is not None:
                q.cap_bins, q.cap_fix, ctx.cap_bwd = hints.poll()
            _lib.call("fpcdr_render_loss_fwd", ctypes.byref(p), ctypes.byref(q), _ptr(cmask), _stream())
            if hints is not None:
                # (the counts are read back after the BACKWARD call has been enqueued: the copy would otherwise sit between the
                # two large kernels on the stream)
                off = (4 * _n_bins(B, H, W) + 3) // 4 * 4                       # FPCDR_OCC_COUNTS_OFFSET
                ctx.hint_update = (hints, occ[off:off + 16].view(torch.int32))
        else:
            _lib.call("fpcdr_render_fwd", ctypes.byref(p), _stream())
            _lib.call("fpcdr_aa_loss_fwd", ctypes.byref(q), _stream())
        del scratch
        ctx.save_for_backward(pos, tex, tri, uv, uv_tri, rast, color, g_aa, sil, flags, occ, ecol, tri_uv, *chain)
        ctx.mip = mip_levels is not None
        ctx.boundary = boundary
        # the one-call sparse forward leaves the list of bins the backward visits in `occ`; measured at cfg3 the backward gains
        # nothing from it (2.69 vs 2.64 ms: its dead workgroups' dispatch hides behind the live ones' work), so the grid form is
        # the default and the list form stays selectable
        ctx.queued = 1 if (sparse and opt.queued_backward) else 0
        # (sparse => the one-call forward, which also leaves the per-bin summary of the antialias flags in `occ`); its kernel summed only
        # the difference to an all-background image: the rest depends on ref alone
        bg_sum = _background_share(ref, bg, opt.ref_bg_sumsq, dev) if sparse else None
        out = torch.empty((), dtype=torch.float32, device=dev)
        _lib.call("fpcdr_objective_value", _ptr(acc), _lib.LOSS_SLOTS, _ptr(bg_sum), float(C), float(n_total), _ptr(out), _stream())
        # forward only (no input wants a gradient, or the caller runs under no_grad -- needs_input_grad stays True there): read the
        # counts back now; otherwise after the backward call has been enqueued
        if not (opt.want_grad and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1])) and ctx.hint_update is not None:
            ctx.hint_update[0].update(ctx.hint_update[1])
            ctx.hint_update = None
        return out

    @staticmethod
    def backward(ctx, g):
        pos, tex, tri, uv, uv_tri, rast, color, g_aa, sil, flags, occ, ecol, tri_uv = ctx.saved_tensors[:13]
        chain = ctx.saved_tensors[13:]
        B, V, _ = pos.shape
        _, H, W, _ = rast.shape
        Ht, Wt, C = tex.shape
        g_pos = torch.zeros_like(pos)
        g_tex = torch.zeros_like(tex) if ctx.needs_input_grad[1] else None
        g_chain = [torch.zeros_like(t) for t in chain] if g_tex is not None else []
        g = g.to(torch.float32).contiguous()
        p = _lib.RenderAaBwd(pos=_ptr(pos), tri=_ptr(tri), uv=_ptr(uv), uv_tri=_ptr(uv_tri), tex=_ptr(tex), rast=_ptr(rast),
                             color=_ptr(color), grad_aa=_ptr(g_aa), sil=_ptr(sil), flags=_ptr(flags), occ=_ptr(occ), empty_color=_ptr(ecol), B=B, V=V,
                             T=tri.shape[0],
                             H=H, W=W, Vt=uv.shape[0], Ht=Ht, Wt=Wt, C=C, boundary_mode=ctx.boundary, grad_pos=_ptr(g_pos),
                             grad_tex=_ptr(g_tex), tri_uv=_ptr(tri_uv), upstream=_ptr(g),    # g: applied inside the kernel
                             queued=ctx.queued, cap_bwd=ctx.cap_bwd, binflags=1 if occ is not None else 0)
        if ctx.mip:
            _wire_mips(p, chain, g_chain)
        _lib.call("fpcdr_render_aa_bwd", ctypes.byref(p), _stream())
        if g_chain:
            _fold_mip_grads([g_tex[None]] + g_chain)
        if ctx.hint_update is not None:
            ctx.hint_update[0].update(ctx.hint_update[1])
            ctx.hint_update = None
        if not ctx.needs_input_grad[0]:
            g_pos = None
        return (g_pos, g_tex) + (None,) * ctx.n_const


class _pixel_objective_onepass(torch.autograd.Function):
    """The pixel objective with VALUE AND GRADIENT from one call (include/fpcdr.h, fpcdr_objective_fwd): the objective is a scalar, so
    its gradient is d(objective)/d(input) times the one upstream number -- it is accumulated by the kernel that shades a pixel, while
    barycentrics, taps, texels and vertices are in registers, and backward() only multiplies by what autograd hands over."""

    @staticmethod
    def forward(ctx, pos, tex, *const):
        tri, adj, uv, uv_tri, ref, opt = const
        H, W, weights, skip_out = opt.H, opt.W, opt.weights, opt.skip_out
        ctx.n_const = len(const)
        lib = _lib.load()
        B, V, _ = pos.shape
        T = tri.shape[0]
        Ht, Wt, C = tex.shape
        dev = pos.device
        want_pos = bool(opt.want_grad and ctx.needs_input_grad[0])
        want_tex = bool(opt.want_grad and ctx.needs_input_grad[1])
        # buffers
        u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
        scratch = u8(lib.fpcdr_rasterize_scratch_bytes(B, T))
        sil = u8(B * T)
        idp = opt.idp_out if opt.idp_out is not None else u8(lib.fpcdr_idplane_bytes(B, H, W))      # (tests / diagnostics: the caller keeps the id planes)
        binlist = u8(lib.fpcdr_binlist_bytes(B, H, W)) if opt.bin_lists else None      # per-bin triangle lists (set-up kernel -> rasteriser)
        occ, cmask = u8(lib.fpcdr_occ_bytes(B, H, W)), u8(lib.fpcdr_objective_cmask_bytes(B, H, W))
        ecol = torch.empty(4, dtype=torch.float32, device=dev)
        # (zero_outputs: the call's first kernel zero-fills its accumulators)
        acc = torch.empty(_lib.LOSS_SLOTS, dtype=torch.float64, device=dev)
        g_pos = torch.empty_like(pos) if want_pos else None
        g_tex = torch.empty_like(tex) if want_tex else None
        tri_uv = _cached_tri_uv(uv, uv_tri)
        p = _lib.Objective(pos=_ptr(pos), tri=_ptr(tri), adj=_ptr(adj), B=B, V=V, T=T, H=H, W=W, scratch=_ptr(scratch), uv=_ptr(uv),
                           uv_tri=_ptr(uv_tri), Vt=uv.shape[0], tri_uv=_ptr(tri_uv), tex=_ptr(tex), Ht=Ht, Wt=Wt, C=C,
                           boundary_mode=opt.boundary, ref=_ptr(ref), bg=opt.bg, color_scale=255.0, grad_scale=1.0 / opt.n_total, sil=_ptr(sil),
                           idp=_ptr(idp), occ=_ptr(occ), cmask=_ptr(cmask),
                           empty_color=_ptr(ecol), loss_sum=_ptr(acc), grad_pos=_ptr(g_pos), grad_tex=_ptr(g_tex), flags=_ptr(opt.flags_out),
                           binlist=_ptr(binlist), zero_outputs=1, skip_out=_ptr(skip_out))
        chain, g_chain = _mip_chain(p, tex, opt.mip_levels, want_tex)
        # plan (_MappedHints.plan: launch sizes, counters, records), and the count-only call when it asks for one
        hints = _hints_for(('onepass', dev.index, B, V, T, H, W), _MappedHints) if opt.use_hints else None
        nbins = _n_bins(B, H, W)
        plan = _MappedHints.plan(hints, nbins, torch.cuda.is_current_stream_capturing(), skip_out is not None, opt.record_slots, B * H * W)
        _wire_plan(p, hints, plan)
        if plan.count:
            p.count_only = 1
            _lib.call("fpcdr_objective_fwd", ctypes.byref(p), _stream())
            p.count_only = 0
            torch.cuda.current_stream(dev).synchronize()
            plan = hints.counted(plan)
            _wire_plan(p, hints, plan)
        # records of the deferred pixels: in slots, or by pixel
        if plan.slots > 0:
            slot_map = torch.empty(nbins, dtype=torch.int32, device=dev)
            p.rec_slots, p.slot_map = plan.slots, _ptr(slot_map)
        rec = torch.empty(plan.n_records, 4, dtype=torch.float32, device=dev)
        color = torch.empty(plan.n_records, C, dtype=torch.float32, device=dev)
        g_aa = torch.empty(plan.n_records, C, dtype=torch.float32, device=dev)
        p.rec, p.color, p.grad_aa = _ptr(rec), _ptr(color), _ptr(g_aa)
        # the value from the call's last kernel: (loss slots + C * background share) / n_total.  The weighted background share is [2] =
        # sum of w0 * rho(d0), sum of w0 over the call's images; the kernel reads [0]
        bg_sum = _background_share(ref, opt.bg, opt.ref_bg_sumsq, dev) if weights is None else weights['bg']
        out = torch.empty((), dtype=torch.float32, device=dev)
        p.bg_sumsq, p.bg_coeff, p.n_total, p.value_out = _ptr(bg_sum), float(C), float(opt.n_total), _ptr(out)
        if opt.zero_extra is not None:      # (a caller's own small accumulators, zero-filled by the call's first kernel)
            p.zero_extra, p.zero_extra_bytes = _ptr(opt.zero_extra), opt.zero_extra.numel() * opt.zero_extra.element_size()
        # launch, fold
        if weights is None:
            _lib.call("fpcdr_objective_fwd", ctypes.byref(p), _stream())
        else:
            # the weighted instantiations of the same kernels ("Weighted objective rule"); the counting call above is the plain one
            wslots = torch.empty(_lib.WSUM_SLOTS, dtype=torch.float64, device=dev)      # (zero-filled by the call's first kernel)
            face_w = weights['face_w']
            pw = _lib.ObjectiveWeighted(base=p, kind=weights['kind'], inv_c=weights['inv_c'], w_outside=weights['w_outside'], sat=weights['sat'],
                                        T_weights=0 if face_w is None else int(face_w.shape[0]), mask=_ptr(weights['mask']), face_w=_ptr(face_w),
                                        wsum=_ptr(wslots))
            _lib.call("fpcdr_objective_weighted_fwd", ctypes.byref(pw), _stream())
            if weights['wsum_out'] is not None:      # the sum of all weights: the covered pixels' w - w0 and the all-background share
                weights['wsum_out'].reshape(-1)[:1].copy_((wslots.sum() + float(C) * bg_sum[1]).reshape(1))
        if g_chain:
            _fold_mip_grads([g_tex[None]] + g_chain)
        ctx.save_for_backward(*(t for t in (g_pos, g_tex) if t is not None))
        ctx.have = (want_pos, want_tex)
        ctx.unit = bool(opt.unit_upstream)
        return out

    @staticmethod
    def backward(ctx, g):
        saved = list(ctx.saved_tensors)
        g_pos = saved.pop(0) if ctx.have[0] else None
        g_tex = saved.pop(0) if ctx.have[1] else None
        if (ctx.needs_input_grad[0] and g_pos is None) or (ctx.needs_input_grad[1] and g_tex is None):
            raise RuntimeError("pixel_objective: the forward pass ran with gradients disabled")
        if not ctx.unit:      # (unit_upstream: the caller guarantees d loss / d objective = 1, as the fit loop's `pix + reg` does)
            g = g.to(torch.float32)
            g_pos = g_pos * g if g_pos is not None else None
            g_tex = g_tex * g if g_tex is not None else None
        return (g_pos if ctx.needs_input_grad[0] else None, g_tex if ctx.needs_input_grad[1] else None) + (None,) * ctx.n_const


def reference_background_sumsq(ref_u8, background=45.0 / 255.0):
    """Per image sum over pixels of (ref - 255 * background)^2 (f64 [B]): the pixel loss (fit.py:579) of an image that
    shows nothing but background.  It depends on the reference images only, so a fit loop computes it once and hands it
    to pixel_objective(ref_bg_sumsq=...), which then reads reference pixels only where geometry is."""
    _check_tensor('ref_u8', ref_u8, torch.uint8, 3)
    ref_u8 = ref_u8.contiguous()
    out = torch.zeros(ref_u8.shape[0], dtype=torch.float64, device=ref_u8.device)
    _lib.call("fpcdr_ref_bg_sumsq", _ptr(ref_u8), ref_u8.shape[0], ref_u8.shape[1] * ref_u8.shape[2], float(background) * 255.0,
              _ptr(out), _stream())
    return out


def reference_background_weighted(ref_u8, mask=None, kind='l2', scale=None, weight_outside=1.0, saturation=0, background=45.0 / 255.0):
    """Per image (sum over pixels of w0 * rho(ref - 255 * background), sum of w0), w0 = wm * weight_outside with wm from the mask byte
    and the saturation level ("Weighted objective rule"; fpcdr_ref_bg_wsum): f64 [B,2].  The weighted one-pass objective's
    share of an image that shows nothing but background -- it depends on the captures and the masks alone, so a fit loop computes it once
    per kind and hands its sum over a call's images to pixel_objective(ref_bg_wsum=...).  mask: uint8 [B,H,W] or None."""
    kind_no, inv_c, weight_outside, saturation = robust_args(kind, scale, weight_outside, saturation)
    _check_tensor('ref_u8', ref_u8, torch.uint8, 3)
    ref_u8 = ref_u8.contiguous()
    if mask is not None:
        _check_tensor('mask', mask, torch.uint8, 3)
        if tuple(mask.shape) != tuple(ref_u8.shape) or mask.device != ref_u8.device:
            raise ValueError(f"mask must be [B,H,W] = {tuple(ref_u8.shape)} on the device of ref_u8 (got {tuple(mask.shape)})")
        mask = mask.contiguous()
    with torch.cuda.device(ref_u8.device):
        out = torch.zeros(ref_u8.shape[0], 2, dtype=torch.float64, device=ref_u8.device)
        _lib.call("fpcdr_ref_bg_wsum", _ptr(ref_u8), _ptr(mask), ref_u8.shape[0], ref_u8.shape[1] * ref_u8.shape[2], float(background) * 255.0,
                  kind_no, inv_c, weight_outside, saturation, _ptr(out), _stream())
    return out


def gaussian_taps(kernel_size, sigma):
    """The taps of the blurred pixel loss ("Blurred loss rule"): g_i = exp(-((i - r) / sigma)^2 / 2), r = (k - 1) / 2, in
    float64, divided by their sum, rounded to float32 -- a CPU tensor [k].  (torchvision's GaussianBlur kernel as recalled; torchvision
    draws sigma at random per call when none is given, here it is always explicit.  Parity with torchvision is not pinned by a test.)"""
    k = int(kernel_size)
    if k != kernel_size or k % 2 == 0 or not 3 <= k <= 63:
        raise ValueError(f"kernel_size must be odd and in 3 .. 63 (got {kernel_size})")
    if not float(sigma) > 0.0:
        raise ValueError(f"sigma must be positive (got {sigma})")
    x = (np.arange(k, dtype=np.float64) - (k - 1) // 2) / float(sigma)
    g = np.exp(-0.5 * x * x)
    return torch.from_numpy((g / g.sum()).astype(np.float32))


def _colour_shape(colour):
    """(B, H, W, C) of the colour a pixel-loss call is handed, or ValueError: what the checks that need no GPU read of it."""
    if not (torch.is_tensor(colour) and colour.dim() == 4):
        raise ValueError("colour must be a [B,H,W,C] tensor")
    return tuple(colour.shape)


def _pixel_tensors(colour, rast, ref_u8):
    """The tensor checks of every pixel-loss call: colour [B,H,W,C] float32, rast [B,H,W,4] float32, ref_u8 [B,H,W] uint8, all on the
    GPU -> the three detached and contiguous, or ValueError.  A call runs its checks that need no GPU before this one."""
    B, H, W, _ = _colour_shape(colour)
    _check_tensor('colour', colour, torch.float32, 4)
    _check_tensor('rast', rast, torch.float32, 4)
    _check_tensor('ref_u8', ref_u8, torch.uint8, 3)
    if tuple(rast.shape) != (B, H, W, 4) or tuple(ref_u8.shape) != (B, H, W):
        raise ValueError(f"rast must be [B,H,W,4] and ref_u8 [B,H,W] for colour {tuple(colour.shape)}")
    return colour.detach().contiguous(), rast.detach().contiguous(), ref_u8.contiguous()


def _pixel_head(colour, rast, ref_u8, background, grad_scale):
    """The ten fields every pixel-loss parameter struct begins with (fpcdr_pixel_loss_params and the three that follow its style)."""
    B, H, W, C = colour.shape
    return dict(color=_ptr(colour), rast=_ptr(rast), ref=_ptr(ref_u8), B=B, H=H, W=W, C=C, bg=float(background), color_scale=255.0,
                grad_scale=float(grad_scale))


def pixel_loss_call(colour, rast, ref_u8, grad_scale, background=45.0 / 255.0, want_grad=True):
    """One fpcdr_pixel_loss call, the plain L2: -> (sum (ref - 255 * (rast.w > 0 ? colour : background))^2 [1] f64, grad_scale * d sum /
    d colour [B,H,W,C] or None)."""
    colour, rast, ref_u8 = _pixel_tensors(colour, rast, ref_u8)
    with torch.cuda.device(colour.device):
        acc = torch.zeros(1, dtype=torch.float64, device=colour.device)
        grad = torch.empty_like(colour) if want_grad else None
        p = _lib.PixelLoss(**_pixel_head(colour, rast, ref_u8, background, grad_scale), loss_sum=_ptr(acc), grad_color=_ptr(grad))
        _lib.call("fpcdr_pixel_loss", ctypes.byref(p), _stream())
    return acc, grad


def _window_args(colour, taps, nonneg_taps=False):
    """The taps of a windowed-loss call as a CPU float32 tensor [k], checked against the image size, or ValueError.  Needs no GPU."""
    _, H, W, _ = _colour_shape(colour)
    taps = torch.as_tensor(taps, dtype=torch.float32).detach().cpu().reshape(-1)
    k = taps.numel()
    if k % 2 == 0 or not 3 <= k <= 63:
        raise ValueError(f"the number of taps must be odd and in 3 .. 63 (got {k})")
    if nonneg_taps and (bool((taps < 0).any()) or not bool(torch.isfinite(taps).all())):
        raise ValueError("the taps of the normalised loss must be finite and non-negative (m >= mu^2 rests on it)")
    if (k - 1) // 2 >= min(H, W):
        raise ValueError(f"reflected borders need (kernel_size - 1) / 2 < min(H, W) (got kernel size {k} for {H} x {W})")
    return taps


def _set_taps(p, taps):
    """taps [k] -> the radius and taps fields of a parameter struct (fpcdr_blur_loss_params / fpcdr_norm_loss_params)"""
    p.radius = (taps.numel() - 1) // 2
    for t in range(taps.numel()):
        p.taps[t] = float(taps[t])


def blur_loss_call(colour, rast, ref_u8, taps, grad_scale, background=45.0 / 255.0, want_grad=True):
    """One fpcdr_blur_loss call: -> (sum E^2 [1] f64, grad_scale * d sum / d colour [B,H,W,C] or None, E [B,H,W,C])."""
    taps = _window_args(colour, taps)
    colour, rast, ref_u8 = _pixel_tensors(colour, rast, ref_u8)
    with torch.cuda.device(colour.device):
        acc = torch.zeros(1, dtype=torch.float64, device=colour.device)
        tmp, blurred = torch.empty_like(colour), torch.empty_like(colour)
        grad = torch.empty_like(colour) if want_grad else None
        p = _lib.BlurLoss(**_pixel_head(colour, rast, ref_u8, background, grad_scale), tmp=_ptr(tmp), blurred=_ptr(blurred),
                          loss_sum=_ptr(acc), grad_color=_ptr(grad))
        _set_taps(p, taps)
        _lib.call("fpcdr_blur_loss", ctypes.byref(p), _stream())
    return acc, grad, blurred


def norm_loss_call(colour, rast, ref_u8, taps, grad_scale, eps=2.0, want_grad=True, background=45.0 / 255.0):
    """One fpcdr_norm_loss call ("Normalised loss rule"): -> (sum d^2 [1] f64, grad_scale * d sum / d colour [B,H,W,C] or
    None, planes), planes a dict of the float32 planes the kernels wrote: 'stats' [B,H,W,C,4] = (mu_a, m_a, mu_t, m_t), 'd' [B,H,W,C]
    and, with a gradient, 'pq' [B,H,W,C,2] = (P, q) and 'p' [B,H,W,C]."""
    eps = float(eps)
    if not (eps > 0.0 and eps < float('inf')):
        raise ValueError(f"eps must be finite and positive, in grey levels (got {eps})")
    taps = _window_args(colour, taps, nonneg_taps=True)
    colour, rast, ref_u8 = _pixel_tensors(colour, rast, ref_u8)
    B, H, W, C = colour.shape
    with torch.cuda.device(colour.device):
        f32 = dict(dtype=torch.float32, device=colour.device)
        acc = torch.zeros(1, dtype=torch.float64, device=colour.device)
        tmp, stats = torch.empty(B, H, W, C, 4, **f32), torch.empty(B, H, W, C, 4, **f32)
        planes = {'stats': stats, 'd': torch.empty_like(colour)}
        grad = None
        if want_grad:
            grad = torch.empty_like(colour)
            planes['pq'], planes['p'] = torch.empty(B, H, W, C, 2, **f32), torch.empty_like(colour)
        p = _lib.NormLoss(**_pixel_head(colour, rast, ref_u8, background, grad_scale), eps=eps, tmp=_ptr(tmp), stats=_ptr(stats),
                          d=_ptr(planes['d']), pq=_ptr(planes.get('pq')), p=_ptr(planes.get('p')), loss_sum=_ptr(acc), grad_color=_ptr(grad))
        _set_taps(p, taps)
        _lib.call("fpcdr_norm_loss", ctypes.byref(p), _stream())
    return acc, grad, planes


def robust_args(kind, scale, weight_outside=1.0, saturation=0):
    """The scalar arguments of the robust loss checked on the host: -> (kind number, inv_c as the float32 the kernel is handed,
    weight_outside, saturation), or ValueError.  Needs no GPU."""
    if kind not in _lib.ROBUST_KIND:
        raise ValueError(f"kind must be one of {sorted(_lib.ROBUST_KIND)} (got {kind!r})")
    inv_c = 0.0
    if kind != 'l2':
        if scale is None:
            raise ValueError(f"kind {kind!r} needs a scale in grey levels: there is no default")
        with np.errstate(over='ignore'):
            inv_c = float(np.float32(1.0 / float(scale))) if float(scale) > 0.0 else 0.0      # float32(1 / c): the statement's number too
        if not (float(scale) > 0.0 and float(scale) < float('inf') and 0.0 < inv_c < float('inf')):
            raise ValueError(f"scale must be finite and positive, in grey levels (got {scale})")
    weight_outside = float(weight_outside)
    if not (weight_outside >= 0.0 and weight_outside < float('inf')):
        raise ValueError(f"weight_outside must be finite and not negative (got {weight_outside})")
    if isinstance(saturation, bool) or not isinstance(saturation, (int, np.integer)) or not 0 <= int(saturation) <= 255:
        raise ValueError(f"saturation must be an integer in 0..255, 0 = off (got {saturation!r})")
    return _lib.ROBUST_KIND[kind], inv_c, weight_outside, int(saturation)


def _weight_tensors(ref_u8, mask, face_weights, check_weights, device=None, n_tri=None):
    """The per-pixel and per-face weights of a robust call, checked -> (mask, face_weights), contiguous, either None as given: mask uint8
    [B,H,W] like ref_u8; face_weights float32 [T], T > 0, finite and >= 0 (a read-back: check_weights=False skips it).  What only the
    objective knows: device, the device of pos, on which both must lie, and n_tri, the triangles of tri, one entry each."""
    where = "" if device is None else " on the device of pos"
    if mask is not None:
        _check_tensor('mask', mask, torch.uint8, 3)
        if tuple(mask.shape) != tuple(ref_u8.shape) or (device is not None and mask.device != device):
            raise ValueError(f"mask must be [B,H,W] = {tuple(ref_u8.shape)}{where} (got {tuple(mask.shape)})")
        mask = mask.contiguous()
    if face_weights is not None:
        _check_tensor('face_weights', face_weights, torch.float32, 1)
        T = int(face_weights.shape[0])
        if T == 0 or (n_tri is not None and T != n_tri) or (device is not None and face_weights.device != device):
            raise ValueError(f"face_weights must have one entry per triangle{'' if n_tri is None else f' ({n_tri})'}{where} (got {T})")
        face_weights = face_weights.detach().contiguous()
        if check_weights and not bool((torch.isfinite(face_weights) & (face_weights >= 0)).all()):
            raise ValueError("face_weights must be finite and not negative")
    return mask, face_weights


def _objective_weights(ref_u8, device, n_tri, background, plain_form, ref_bg_sumsq, robust, mask, face_weights, weight_outside, saturation,
                       ref_bg_wsum, wsum_out, check_weights):
    """pixel_objective's weighted keywords, checked -> what the weighted one-pass call reads (kind, inv_c, w_outside, sat, mask, face_w,
    bg: the background share f64 [2], wsum_out), or None when none of them is given: the plain call.  ref_u8 contiguous; device, n_tri:
    of pos and tri; plain_form: the call is not the one-pass sparse form without mip, which alone takes weights.  ValueError otherwise."""
    if (robust is None and mask is None and face_weights is None and float(weight_outside) == 1.0 and saturation == 0
            and ref_bg_wsum is None and wsum_out is None):
        return None
    if plain_form:
        raise ValueError("pixel_objective: robust / mask / face_weights / weight_outside / saturation / ref_bg_wsum / wsum_out belong to "
                         "the one-pass sparse form without mip (use the separate operators and robust_pixel_loss otherwise)")
    if ref_bg_sumsq is not None:
        raise ValueError("pixel_objective: a weighted call takes ref_bg_wsum (reference_background_weighted), not ref_bg_sumsq")
    if robust is not None and not (isinstance(robust, (tuple, list)) and len(robust) == 2):
        raise ValueError(f"robust must be (kind, scale) (got {robust!r})")
    kind, scale = robust if robust is not None else ('l2', None)
    kind_no, inv_c, weight_outside, saturation = robust_args(kind, scale, weight_outside, saturation)
    mask, face_weights = _weight_tensors(ref_u8, mask, face_weights, check_weights, device=device, n_tri=n_tri)
    if wsum_out is not None and not (torch.is_tensor(wsum_out) and wsum_out.dtype == torch.float64 and wsum_out.device == device
                                     and wsum_out.numel() >= 1 and wsum_out.is_contiguous()):
        raise ValueError("wsum_out must be a contiguous float64 tensor of at least one element on the device of pos")
    if ref_bg_wsum is None:
        bgw = reference_background_weighted(ref_u8, mask, kind, scale, weight_outside, saturation, background).sum(0)
    else:
        bgw = torch.as_tensor(ref_bg_wsum, device=device).to(torch.float64)
        if bgw.dim() == 2:
            bgw = bgw.sum(0)
        if tuple(bgw.shape) != (2,):
            raise ValueError(f"ref_bg_wsum must be [2] or [B,2] (got {tuple(bgw.shape)})")
    return dict(kind=kind_no, inv_c=inv_c, w_outside=weight_outside, sat=saturation, mask=mask, face_w=face_weights, bg=bgw.contiguous(),
                wsum_out=wsum_out)


def robust_loss_call(colour, rast, ref_u8, kind, scale, grad_scale, mask=None, face_weights=None, weight_outside=1.0, saturation=0,
                     background=45.0 / 255.0, want_grad=True, check_weights=True):
    """One fpcdr_robust_loss call ("Robust loss rule"): -> (sums [2] f64 = (sum of w * rho, sum of w), grad_scale * d sums[0] /
    d colour [B,H,W,C] or None).  kind 'l2' | 'charbonnier' | 'geman_mcclure', scale c in grey levels (ignored for 'l2'); mask uint8
    [B,H,W], 255 = trust, 0 = ignore; face_weights float32 [T], finite and >= 0, looked up through the triangle id of rast (the check
    of its values is a read-back; check_weights=False for a caller that has checked them once, as the Fitter has); weight_outside for
    uncovered pixels; saturation 1..255: capture pixels at or above it count nothing.  The weights are constants: they get no gradient."""
    kind_no, inv_c, weight_outside, saturation = robust_args(kind, scale, weight_outside, saturation)
    colour, rast, ref_u8 = _pixel_tensors(colour, rast, ref_u8)
    mask, face_weights = _weight_tensors(ref_u8, mask, face_weights, check_weights)
    T = 0 if face_weights is None else int(face_weights.shape[0])
    with torch.cuda.device(colour.device):
        sums = torch.zeros(2, dtype=torch.float64, device=colour.device)
        grad = torch.empty_like(colour) if want_grad else None
        p = _lib.RobustLoss(**_pixel_head(colour, rast, ref_u8, background, grad_scale), kind=kind_no, inv_c=inv_c, w_outside=weight_outside,
                            sat=saturation, mask=_ptr(mask), face_w=_ptr(face_weights), T=T, sums=_ptr(sums), grad_color=_ptr(grad))
        _lib.call("fpcdr_robust_loss", ctypes.byref(p), _stream())
    return sums, grad


def tex_prior_call(tex, w_smooth, w_anchor, anchor=None, smooth_weights=None, anchor_weights=None, inv_c=0.0, want_grad=True, acc=None):
    """One fpcdr_tex_prior call ("Texture prior rule") on tensors the caller has checked (fit.texture_prior does): tex, anchor
    [Ht,Wt,C] and the maps [Ht,Wt] float32, contiguous, on one GPU; inv_c the float32 inverse of the Charbonnier scale, 0.0 for L2.
    -> (value [] = w_smooth * part[0] + w_anchor * part[1], part [2] = (smoothness, anchor) / (Ht Wt), d value / d tex [Ht,Wt,C] for a
    unit upstream or None).  acc: two float64 zeros on the device (None: a fresh buffer); the call leaves them zero again."""
    Ht, Wt, C = tex.shape
    with torch.cuda.device(tex.device):
        if acc is None:
            acc = torch.zeros(2, dtype=torch.float64, device=tex.device)
        assert acc.dtype == torch.float64 and acc.numel() >= 2 and acc.is_contiguous() and acc.device == tex.device
        part = torch.empty(2, dtype=torch.float32, device=tex.device)
        out = torch.empty((), dtype=torch.float32, device=tex.device)
        grad = torch.empty_like(tex) if want_grad else None
        _lib.call("fpcdr_tex_prior", _ptr(tex), _ptr(anchor), _ptr(smooth_weights), _ptr(anchor_weights), float(inv_c), float(w_smooth),
                  float(w_anchor), _ptr(grad), _ptr(acc), _ptr(part), _ptr(out), int(Ht), int(Wt), int(C), _stream())
    return out, part, grad


class _pixel_loss_func(torch.autograd.Function):
    """call = a *_loss_call with its keyword arguments bound, args = its positional arguments between colour and grad_scale: the mean over
    n_total of the call's first sum, and the gradient the same call computed, times the upstream scalar, as the backward."""
    @staticmethod
    def forward(ctx, call, n_total, colour, *args):
        sums, grad = call(colour, *args, 1.0 / n_total)[:2]
        ctx.save_for_backward(grad)
        ctx.n_args = len(args)
        return (sums[0] / n_total).to(torch.float32)

    @staticmethod
    def backward(ctx, upstream):
        grad, = ctx.saved_tensors
        return (None, None, grad * upstream) + (None,) * ctx.n_args


def _mean_pixel_loss(call, colour, n_total, *args):
    _colour_shape(colour)
    return _pixel_loss_func.apply(call, float(n_total or colour.numel()), colour, *args)


def _taps_of(what, sigma, kernel_size, taps):
    """The "sigma or taps" of the windowed losses: taps= as given, else the Gaussian of (kernel_size, sigma)."""
    if taps is not None:
        return taps
    if sigma is None:
        raise ValueError(f"{what} needs sigma (or taps)")
    return gaussian_taps(kernel_size, sigma)


def blurred_pixel_loss(colour, rast, ref_u8, sigma=None, kernel_size=31, n_total=None, background=45.0 / 255.0, taps=None):
    """mean over n_total elements (default: all of colour) of E^2, E = the Gaussian-blurred residual ref - 255 * (rast.w > 0 ? colour :
    background) with reflected borders ("Blurred loss rule"; fpcdr_blur_loss) -- a float32 scalar whose backward is the
    closed-form gradient the same call computed, times the upstream scalar.  taps= (odd, 3 .. 63 entries) overrides sigma and kernel_size."""
    taps = _taps_of("blurred_pixel_loss", sigma, kernel_size, taps)
    return _mean_pixel_loss(functools.partial(blur_loss_call, background=background), colour, n_total, rast, ref_u8, taps)


def normalised_pixel_loss(colour, rast, ref_u8, sigma=None, kernel_size=31, eps=2.0, n_total=None, background=45.0 / 255.0, taps=None):
    """mean over n_total elements (default: all of colour) of (n_a - n_t)^2, the render a = 255 * (rast.w > 0 ? colour : background) and
    the capture t = ref each normalised by the mean and the deviation of its own Gaussian window, n = (x - G x) / sqrt(G x^2 - (G x)^2 +
    eps^2) ("Normalised loss rule"; fpcdr_norm_loss): a camera's gain and offset drop out.  A dimensionless float32 scalar
    whose backward is the closed-form gradient the same call computed, times the upstream scalar.  eps is in grey levels; taps= (odd,
    3 .. 63 non-negative entries) overrides sigma and kernel_size.  Within a window the loss sees neither the level nor the contrast of the
    texture: start from a baked or supplied texture, not from noise."""
    taps = _taps_of("normalised_pixel_loss", sigma, kernel_size, taps)
    return _mean_pixel_loss(functools.partial(norm_loss_call, eps=float(eps), background=background), colour, n_total, rast, ref_u8, taps)


def robust_pixel_loss(colour, rast, ref_u8, kind='charbonnier', scale=None, n_total=None, mask=None, face_weights=None, weight_outside=1.0,
                      saturation=0, background=45.0 / 255.0):
    """sum of w * rho(ref - 255 * (rast.w > 0 ? colour : background)) over n_total elements (default: all of colour), rho the robust
    function `kind` with scale c = `scale` in grey levels -- like d^2 for |d| << c, 2 c |d| ('charbonnier') or c^2 ('geman_mcclure') for
    |d| >> c -- and w the product of the weights given ("Robust loss rule"; fpcdr_robust_loss).  The division is by
    n_total, not by the sum of the weights.  A float32 scalar whose backward is the closed-form gradient the same call computed, times
    the upstream scalar.  There is no default scale: nobody has measured one."""
    call = functools.partial(robust_loss_call, mask=mask, face_weights=face_weights, weight_outside=weight_outside, saturation=saturation,
                             background=background)
    return _mean_pixel_loss(call, colour, n_total, rast, ref_u8, kind, scale)


def undistort_images(images, intr, dist, clip_max=255, flip_rows=False):
    """Lens undistortion of 8-bit images (the reference's src/undistort.py: cv2.undistort(image, intrinsic, dist), new camera matrix =
    old one), by the rule of DESIGN.md 3 "Undistortion rule" (fpcdr_undistort_u8): OpenCV's five-coefficient model in double precision,
    bilinear taps with a zero border, round half up, then min(., clip_max) and, with flip_rows, row i written to row H - 1 - i.

      images  uint8 GPU tensor [N,H,W] or [F,Nc,H,W], contiguous; image n belongs to camera n % Nc
      intr    [Nc,3,3] intrinsic matrices, dist [Nc,5] or [Nc,5,1] coefficients (k1, k2, p1, p2, k3): arrays or tensors; their values
              (data.load_calibration holds float32) are widened to double

    Returns a new uint8 tensor of the shape of `images`."""
    _check_tensor('images', images, torch.uint8)
    if images.dim() not in (3, 4):
        raise ValueError(f"images must be [N,H,W] or [F,Nc,H,W] (got shape {tuple(images.shape)})")
    if not images.is_contiguous():
        raise ValueError("images must be contiguous")
    intr = torch.as_tensor(intr).detach().to('cpu', torch.float64)
    dist = torch.as_tensor(dist).detach().to('cpu', torch.float64)
    if intr.dim() != 3 or tuple(intr.shape[1:]) != (3, 3):
        raise ValueError(f"intr must be [Nc,3,3] (got shape {tuple(intr.shape)})")
    Nc = intr.shape[0]
    if tuple(dist.shape) not in ((Nc, 5), (Nc, 5, 1)):
        raise ValueError(f"dist must be [Nc,5] or [Nc,5,1] with Nc = {Nc} (got shape {tuple(dist.shape)})")
    if images.dim() == 4 and images.shape[1] != Nc:
        raise ValueError(f"images [F,Nc,H,W] has {images.shape[1]} cameras, intr has {Nc}")
    if Nc == 0 or images.numel() == 0:
        raise ValueError("empty input")
    if not 0 <= int(clip_max) <= 255:
        raise ValueError("clip_max must be in [0, 255]")
    H, W = images.shape[-2:]
    table = torch.cat([torch.stack([intr[:, 0, 0], intr[:, 1, 1], intr[:, 0, 2], intr[:, 1, 2]], dim=1), dist.reshape(Nc, 5)], dim=1)
    out = torch.empty_like(images)
    with torch.cuda.device(images.device):
        table = table.contiguous().to(images.device)
        _lib.call("fpcdr_undistort_u8", _ptr(images), _ptr(out), _ptr(table), images.numel() // (H * W), H, W, Nc, int(clip_max),
                  1 if flip_rows else 0, _stream())
    return out


def _check_image_pair(what, img, ref, others=()):
    """The (render, capture) pair of compare_images / overlay_images (`what`: the operator's noun for the messages): img a float32 or
    uint8 GPU tensor [N,H,W] or [N,H,W,1], ref a uint8 one [N,H,W] on the same device, both contiguous and not empty.  others: further
    (name, tensor) inputs of the call, which must be tensors on that device too -- the rest about them is the caller's.  Returns img as
    [N,H,W]."""
    tensors = [('img', img), ('ref', ref)] + list(others)
    for name, t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    for name, t in tensors:
        if not t.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor (got {t.device}); the {what} has no CPU path")
        if t.device != img.device:
            raise ValueError(f"img and {name} are on different devices ({img.device}, {t.device})")
    if img.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"img must be float32 or uint8 (got {img.dtype})")
    if ref.dtype != torch.uint8:
        raise ValueError(f"ref must be uint8 (got {ref.dtype})")
    if img.dim() == 4:
        if img.shape[3] != 1:
            raise ValueError(f"img must have one channel (got shape {tuple(img.shape)})")
        img = img[..., 0]
    if img.dim() != 3 or ref.dim() != 3:
        raise ValueError(f"img must be [N,H,W] or [N,H,W,1] and ref [N,H,W] (got shapes {tuple(img.shape)}, {tuple(ref.shape)})")
    if img.shape != ref.shape:
        raise ValueError(f"img {tuple(img.shape)} and ref {tuple(ref.shape)} differ in shape")
    if not img.is_contiguous() or not ref.is_contiguous():
        raise ValueError("img and ref must be contiguous")
    if img.numel() == 0:
        raise ValueError("empty input")
    return img


def compare_images(img, ref, mode='colour', cols=(100, 1100), scale=255.0, flip_rows=False, want_rows=True):
    """Rendered images against captures (the reference's comparisons.py: compareSequence's heat map and the integer differences behind
    compareSequenceNumerical's row means), by the rule of DESIGN.md 3 "Comparison rule" (fpcdr_compare_u8).

      img        GPU tensor [N,H,W] or [N,H,W,1], contiguous: uint8, or float32 quantised as clip(rint(img * scale), 0, 255) (NaN -> 0)
      ref        uint8 GPU tensor [N,H,W], contiguous, top row first
      mode       'colour' (d >= 0: (255, s, s), d < 0: (s, s, 255), s = max(255 - 2 |d|, 0)), 'grey' ((s, s, s)), or None: no heat map
      cols       (col0, col1): the row sums run over the columns [col0, col1) inside the image
      flip_rows  output row i compares img's row H - 1 - i (a raster has row 0 at the bottom) with ref's row i
      want_rows  False: no row sums

    Returns (heat uint8 [N,H,W,3] or None, row_sums int32 [N,H] or None): sums of |d|, exact; the means are the caller's."""
    if mode not in ('colour', 'grey', None):
        raise ValueError(f"mode must be 'colour', 'grey' or None (got {mode!r})")
    if mode is None and not want_rows:
        raise ValueError("neither a heat map (mode) nor row sums (want_rows) requested")
    img = _check_image_pair('comparison', img, ref)
    N, H, W = img.shape
    if 255 * W >= 2 ** 31:
        raise ValueError("a row sum of 255 * W does not fit int32")
    col0, col1 = (int(c) for c in cols)
    lim = 2 ** 31 - 1
    col0, col1 = max(min(col0, lim), -lim), max(min(col1, lim), -lim)
    heat = torch.empty((N, H, W, 3), dtype=torch.uint8, device=img.device) if mode is not None else None
    rows = torch.zeros((N, H), dtype=torch.int32, device=img.device) if want_rows else None
    with torch.cuda.device(img.device):
        _lib.call("fpcdr_compare_u8", _ptr(img), 1 if img.dtype == torch.float32 else 0, float(scale), _ptr(ref), _ptr(heat), _ptr(rows),
                  N, H, W, col0, col1, 1 if mode == 'grey' else 0, 1 if flip_rows else 0, _stream())
    return heat, rows


def overlay_images(img, ref, rast=None, rast_db=None, weight=0.5, outside='render', wire=None, half_width=0.5, scale=255.0,
                   flip_rows=False):
    """Rendered images laid over the captures, optionally with the mesh's edges drawn (the reference's render_result_blended.py:149-154,
    ref * 0.5 + img * 0.5 rounded and clipped; its wireframe variant paints the lines into a texture instead), by the rule of DESIGN.md 3
    "Overlay rule" (fpcdr_overlay_u8).

      img         GPU tensor [N,H,W] or [N,H,W,1], contiguous: uint8, or float32 quantised as clip(rint(img * scale), 0, 255) (NaN -> 0)
      ref         uint8 GPU tensor [N,H,W], contiguous, top row first
      rast        float32 [N,H,W,4] as rasterize returns it (u, v, z/w, triangle + 1), or None
      rast_db     float32 [N,H,W,4], rasterize's second output (du/dX, du/dY, dv/dX, dv/dY), or None
      weight      the render's share of the blend in [0, 1], taken to the nearest 1/256; the blend is rounded half to even
      outside     'render': the blend everywhere, whatever background the caller put into img (the reference's behaviour);
                  'capture': the capture unchanged where rast shows no triangle (needs rast)
      wire        None, or the (r, g, b) bytes of the mesh lines (needs rast and rast_db): a covered pixel is painted where one of its
                  triangle's barycentrics b has b * b < half_width^2 * |grad b|^2, i.e. lies within half_width pixels of an edge to
                  first order; both triangles of a shared edge draw, so a line is 2 * half_width wide
      flip_rows   output row i takes row H - 1 - i of img, rast and rast_db (a raster has row 0 at the bottom) and row i of ref

    Returns uint8 [N,H,W,3].  rast is read only if outside='capture' or a wire asks for it, rast_db only for a wire."""
    if outside not in ('render', 'capture'):
        raise ValueError(f"outside must be 'render' or 'capture' (got {outside!r})")
    rasters = [(k, v) for k, v in (('rast', rast), ('rast_db', rast_db)) if v is not None]
    img = _check_image_pair('overlay', img, ref, rasters)
    for name, t in rasters:
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 (got {t.dtype})")
        if tuple(t.shape) != tuple(img.shape) + (4,):
            raise ValueError(f"{name} must be {tuple(img.shape) + (4,)} (got {tuple(t.shape)})")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    weight = float(weight)
    if not 0.0 <= weight <= 1.0:        # (false for a NaN)
        raise ValueError(f"weight must lie in [0, 1] (got {weight})")
    weight_256 = int(np.rint(weight * 256))
    hw2, rgb = 0.0, 0
    if wire is not None:
        wire = tuple(wire)
        if len(wire) != 3 or any(int(c) != c or not 0 <= int(c) <= 255 for c in wire):
            raise ValueError(f"wire must be None or three bytes (r, g, b) (got {wire!r})")
        if rast is None or rast_db is None:
            raise ValueError("wire needs rast and rast_db (rasterize's two outputs)")
        with np.errstate(over='ignore'):
            hw2 = np.float32(half_width) * np.float32(half_width)
        if not (np.isfinite(hw2) and float(half_width) >= 0.0):
            raise ValueError(f"half_width must be finite and >= 0 (got {half_width})")
        hw2 = float(hw2)
        rgb = int(wire[0]) | int(wire[1]) << 8 | int(wire[2]) << 16
    if outside == 'capture' and rast is None:
        raise ValueError("outside='capture' needs rast")
    N, H, W = img.shape
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=img.device)
    with torch.cuda.device(img.device):
        _lib.call("fpcdr_overlay_u8", _ptr(img), 1 if img.dtype == torch.float32 else 0, float(scale), _ptr(ref), _ptr(rast), _ptr(rast_db),
                  _ptr(out), N, H, W, weight_256, 1 if outside == 'capture' else 0, hw2, rgb, 1 if flip_rows else 0, _stream())
    return out


def bake_accumulate(texc, rast, ref_u8, acc, boundary_mode='wrap', interior_only=False, flip_rows=False):
    """Splat captures into a texture accumulator by the rule of DESIGN.md 3 "Bake rule" (fpcdr_bake_accumulate_u8): every covered pixel
    adds its capture into the four texels texture(filter_mode='linear') would read for it, with the bilinear weights in 1/256 per axis.

      texc           float32 GPU tensor [N,H,W,2], as interpolate returns it;  rast  float32 [N,H,W,4], only .w is read (> 0: covered)
      ref_u8         uint8 [N,H,W]; row i belongs to raster row i, or with flip_rows to raster row H - 1 - i
      acc            int64 [Ht,Wt,2], (num, den) per texel, the bits of unsigned 64-bit sums; ADDED to: torch.zeros for a new bake
      boundary_mode  'wrap' or 'clamp', as for texture
      interior_only  leave out covered pixels with an uncovered neighbour (up, down, left, right) inside the image: their capture
                     holds background the antialias operator blended in

    All contiguous, on one device.  Integer sums: the result does not depend on the order of the calls or on how the images are shared out
    over calls and ranks.  Returns acc."""
    tensors = [('texc', texc), ('rast', rast), ('ref_u8', ref_u8), ('acc', acc)]
    for name, t in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    for name, t in tensors:
        if not t.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor (got {t.device}); the bake has no CPU path")
        if t.device != texc.device:
            raise ValueError(f"texc and {name} are on different devices ({texc.device}, {t.device})")
    for name, t, dtype in (('texc', texc, torch.float32), ('rast', rast, torch.float32), ('ref_u8', ref_u8, torch.uint8), ('acc', acc, torch.int64)):
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if boundary_mode not in ('wrap', 'clamp'):
        raise ValueError(f"boundary_mode must be 'wrap' or 'clamp' (got {boundary_mode!r})")
    if texc.dim() != 4 or texc.shape[3] != 2:
        raise ValueError(f"texc must be [N,H,W,2] (got shape {tuple(texc.shape)})")
    N, H, W, _ = texc.shape
    if tuple(rast.shape) != (N, H, W, 4):
        raise ValueError(f"rast must be {(N, H, W, 4)} (got {tuple(rast.shape)})")
    if tuple(ref_u8.shape) != (N, H, W):
        raise ValueError(f"ref_u8 must be {(N, H, W)} (got {tuple(ref_u8.shape)})")
    if acc.dim() != 3 or acc.shape[2] != 2:
        raise ValueError(f"acc must be [Ht,Wt,2] (got shape {tuple(acc.shape)})")
    if not all(t.is_contiguous() for _, t in tensors):
        raise ValueError("texc, rast, ref_u8 and acc must be contiguous")
    if texc.numel() == 0 or acc.numel() == 0:
        raise ValueError("empty input")
    with torch.cuda.device(texc.device):
        _lib.call("fpcdr_bake_accumulate_u8", _ptr(texc), _ptr(rast), _ptr(ref_u8), _ptr(acc), N, H, W, acc.shape[0], acc.shape[1],
                  _lib.BOUNDARY[boundary_mode], 1 if interior_only else 0, 1 if flip_rows else 0, _stream())
    return acc


def bake_resolve(acc, color_scale=255.0, min_weight=0.0, dilate=8, hole_value=0.5):
    """The texture of an accumulator of bake_accumulate (DESIGN.md 3 "Bake rule": fpcdr_bake_resolve, fpcdr_bake_dilate).

      acc          int64 GPU tensor [Ht,Wt,2], contiguous
      color_scale  the captures' unit: tex = num / (den * color_scale), 255 as in the pixel loss
      min_weight   a texel is filled when its summed weight reaches it, in pixels (1 = one pixel centred on the texel); every texel
                   with any weight at all for 0: min_den = max(1, round(min_weight * 65536))
      dilate       passes that give an unfilled texel next to filled ones the mean of those neighbours: the gutter a UV chart needs,
                   because bilinear taps at its border read texels no pixel landed on
      hole_value   the value of the texels that are still unfilled afterwards

    Returns (tex [Ht,Wt] float32, filled [Ht,Wt] bool: which texels the captures reached, BEFORE the dilation)."""
    _check_tensor('acc', acc, torch.int64, 3)
    if acc.shape[2] != 2 or acc.numel() == 0:
        raise ValueError(f"acc must be [Ht,Wt,2] and not empty (got shape {tuple(acc.shape)})")
    if not acc.is_contiguous():
        raise ValueError("acc must be contiguous")
    color_scale, min_weight, dilate = float(color_scale), float(min_weight), int(dilate)
    if not (color_scale > 0.0 and np.isfinite(color_scale)):
        raise ValueError(f"color_scale must be positive and finite (got {color_scale})")
    if not 0.0 <= min_weight < 2.0 ** 40:       # (false for a NaN)
        raise ValueError(f"min_weight must lie in [0, 2^40) (got {min_weight})")
    if dilate < 0:
        raise ValueError(f"dilate must be >= 0 (got {dilate})")
    min_den = max(1, int(round(min_weight * 65536)))
    Ht, Wt = acc.shape[:2]
    dev = acc.device
    tex = torch.empty((Ht, Wt), dtype=torch.float32, device=dev)
    filled = torch.empty((Ht, Wt), dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        _lib.call("fpcdr_bake_resolve", _ptr(acc), _ptr(tex), _ptr(filled), Ht, Wt, color_scale, min_den, _stream())
        cur, cur_f = tex, filled
        if dilate > 0:
            cur_f = filled.clone()          # (the returned mask stays as the resolve left it)
            nxt, nxt_f = torch.empty_like(tex), torch.empty_like(filled)
            for _ in range(dilate):
                _lib.call("fpcdr_bake_dilate", _ptr(cur), _ptr(cur_f), _ptr(nxt), _ptr(nxt_f), Ht, Wt, _stream())
                cur, cur_f, nxt, nxt_f = nxt, nxt_f, cur, cur_f
    out = torch.where(cur_f, cur, torch.tensor(float(hole_value), dtype=torch.float32, device=dev))
    return out, filled


def downsample_images(images, factor):
    """Box reduction of 8-bit images by an integer factor, by the rule of DESIGN.md 3 "Downsample rule" (fpcdr_downsample_u8): every output
    pixel is the exact mean of its factor x factor block of `images`, rounded half up, once; rows are not flipped.  A level of a resolution
    pyramid (FitConfig.pyramid): the projection chain is pure NDC, so a render at (H / factor, W / factor) with the same matrices is aligned
    with this reduction of the capture.  Make every level from the full-size images: a cascade rounds twice and gives other bytes.

      images  uint8 GPU tensor [..., H, W] (made contiguous);  factor  an integer in 2..16 that divides H and W

    Runs on the current stream and allocates its result only.  Returns a new uint8 tensor [..., H / factor, W / factor]."""
    _check_tensor('images', images, torch.uint8)
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)):
        raise ValueError(f"factor must be an integer (got {factor!r})")
    factor = int(factor)
    if not 2 <= factor <= 16:
        raise ValueError(f"factor must lie in 2..16 (got {factor})")
    if images.dim() < 2:
        raise ValueError(f"images must be [..., H, W] (got shape {tuple(images.shape)})")
    H, W = int(images.shape[-2]), int(images.shape[-1])
    if H == 0 or W == 0 or H % factor or W % factor:
        raise ValueError(f"factor {factor} does not divide the image size {H} x {W}")
    images = images.contiguous()
    out = torch.empty(tuple(images.shape[:-2]) + (H // factor, W // factor), dtype=torch.uint8, device=images.device)
    with torch.cuda.device(images.device):
        _lib.call("fpcdr_downsample_u8", _ptr(images), _ptr(out), images.numel() // (H * W), H, W, factor, _stream())
    return out


def exposure_sums(colour, rast, ref_u8, sums=None, mask=None, face_weights=None, lo=1, hi=254):
    """The integer moments of render byte against capture byte over the interior covered pixels of every image, by the rule of DESIGN.md
    3 "Exposure rule" (fpcdr_exposure_sums): what exposure.fit_gains fits a camera's gain and offset from.

      colour        float32 GPU tensor [N,H,W,C], C in 1..4: the render, r = its byte at scale 255 (the Comparison rule's quantisation)
      rast          float32 [N,H,W,4], only .w is read (> 0: covered; the triangle id + 1 for face_weights)
      ref_u8        uint8 [N,H,W], t; row i belongs to raster row i
      sums          int64 [N,6] = (n, sum r, sum t, sum r^2, sum t^2, sum r t) per image, ADDED to; None: a new table of zeros
      mask          uint8 [N,H,W] or None: a pixel counts only where its byte is >= 128
      face_weights  float32 [T] or None: a pixel counts only where its triangle's weight is > 0 (an id past the table does not count)
      lo, hi        0 <= lo <= hi <= 255: a pixel counts only where lo <= t <= hi

    A pixel with an uncovered neighbour (up, down, left, right) inside the image does not count: silhouette pixels hold blended
    background.  All contiguous, on one device.  Integer sums: the result does not depend on the order of the calls or on how the images
    are shared out over calls and ranks.  Returns sums."""
    tensors = [('colour', colour, torch.float32), ('rast', rast, torch.float32), ('ref_u8', ref_u8, torch.uint8)]
    if sums is not None:
        tensors.append(('sums', sums, torch.int64))
    if mask is not None:
        tensors.append(('mask', mask, torch.uint8))
    if face_weights is not None:
        tensors.append(('face_weights', face_weights, torch.float32))
    for name, t, _ in tensors:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    for name, t, dtype in tensors:
        if not t.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor (got {t.device}); the exposure sums have no CPU path")
        if t.device != colour.device:
            raise ValueError(f"colour and {name} are on different devices ({colour.device}, {t.device})")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    for name, v in (('lo', lo), ('hi', hi)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer (got {v!r})")
    if not 0 <= lo <= hi <= 255:
        raise ValueError(f"0 <= lo <= hi <= 255 is required (got lo = {lo}, hi = {hi})")
    if colour.dim() != 4 or not 1 <= colour.shape[3] <= 4:
        raise ValueError(f"colour must be [N,H,W,C] with C in 1..4 (got shape {tuple(colour.shape)})")
    N, H, W, C = colour.shape
    if tuple(rast.shape) != (N, H, W, 4):
        raise ValueError(f"rast must be {(N, H, W, 4)} (got {tuple(rast.shape)})")
    if tuple(ref_u8.shape) != (N, H, W):
        raise ValueError(f"ref_u8 must be {(N, H, W)} (got {tuple(ref_u8.shape)})")
    if mask is not None and tuple(mask.shape) != (N, H, W):
        raise ValueError(f"mask must be {(N, H, W)} (got {tuple(mask.shape)})")
    if face_weights is not None and (face_weights.dim() != 1 or face_weights.numel() == 0):
        raise ValueError(f"face_weights must be [T] and not empty (got shape {tuple(face_weights.shape)})")
    if colour.numel() == 0:
        raise ValueError("empty input")
    if sums is None:
        sums = torch.zeros(N, 6, dtype=torch.int64, device=colour.device)
    elif tuple(sums.shape) != (N, 6):
        raise ValueError(f"sums must be {(N, 6)} (got {tuple(sums.shape)})")
    if not all(t.is_contiguous() for _, t, _ in tensors) or not sums.is_contiguous():
        raise ValueError("colour, rast, ref_u8, sums, mask and face_weights must be contiguous")
    with torch.cuda.device(colour.device):
        _lib.call("fpcdr_exposure_sums", _ptr(colour), _ptr(rast), _ptr(ref_u8), _ptr(mask), _ptr(face_weights),
                  0 if face_weights is None else int(face_weights.numel()), int(lo), int(hi), N, H, W, C, _ptr(sums), _stream())
    return sums


def apply_lut_u8(images, lut, cam_of_image):
    """images[b] <- lut[cam_of_image[b]][images[b]], IN PLACE (DESIGN.md 3 "Exposure rule": fpcdr_apply_lut_u8): a camera's 256-entry
    table applied to each of its 8-bit images, e.g. exposure.fit_gains' or a Fitter's composite table on captures read anew.

      images        uint8 GPU tensor [B, ...], contiguous (every trailing dimension is one image's bytes)
      lut           uint8 [Nl,256], contiguous, same device
      cam_of_image  int32 [B], same device: the table of each image

    An entry of cam_of_image outside [0, Nl) raises RuntimeError after the other images have been mapped; that image is left as it is.
    The call reads cam_of_image back first, so it waits for the stream and cannot be captured into a graph.  Returns images."""
    for name, t, dtype in (('images', images, torch.uint8), ('lut', lut, torch.uint8), ('cam_of_image', cam_of_image, torch.int32)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if not t.is_cuda:
            raise ValueError(f"{name} must be a GPU tensor (got {t.device}); apply_lut_u8 has no CPU path")
        if t.device != images.device:
            raise ValueError(f"images and {name} are on different devices ({images.device}, {t.device})")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous (the images are written in place)")
    if images.dim() < 2 or images.numel() == 0:
        raise ValueError(f"images must be [B, ...] and not empty (got shape {tuple(images.shape)})")
    if lut.dim() != 2 or lut.shape[1] != 256 or lut.shape[0] == 0:
        raise ValueError(f"lut must be [Nl,256] (got shape {tuple(lut.shape)})")
    B = int(images.shape[0])
    if tuple(cam_of_image.shape) != (B,):
        raise ValueError(f"cam_of_image must be {(B,)} (got {tuple(cam_of_image.shape)})")
    with torch.cuda.device(images.device):
        _lib.call("fpcdr_apply_lut_u8", _ptr(images), _ptr(lut), _ptr(cam_of_image), int(lut.shape[0]), B, images.numel() // B, _stream())
    return images


def pixel_objective(glctx, pos, tri, uv, uv_tri, tex, ref_u8, resolution, n_total=None, background=45.0 / 255.0,
                    boundary_mode='wrap', sparse=True, ref_bg_sumsq=None, launch_hints=True, queued_backward=False,
                    enable_mip=False, max_mip_level=None, one_pass=True, unit_upstream=False, aa_flags_out=None, zero_extra=None,
                    id_plane_out=None, record_slots=None, skip_out=None, robust=None, mask=None, face_weights=None, weight_outside=1.0,
                    saturation=0, ref_bg_wsum=None, wsum_out=None, check_weights=True):
    """The whole pixel term of the reference's loss (fit.py:151-161 + the first term of :579) for a minibatch:
    mean((ref - 255 * where(rast.w > 0, antialias(texture(interpolate(rasterize(pos)))), bg))^2) over n_total elements (default: all of
    this call's).  pos [B,V,4], tex [Ht,Wt,C] (C in 1,3,4), ref_u8 [B,H,W] uint8.  Differentiable w.r.t. pos and tex; equals the chain of
    separate operators + pixel loss.
    By default (one_pass and sparse) VALUE AND GRADIENT come from ONE call, fpcdr_objective_fwd: the kernel that shades a pixel also
    chains its gradient back; backward() multiplies by the upstream scalar, or returns the buffers as they are with unit_upstream=True
    (the caller guarantees d loss / d objective = 1).  The alternative, one_pass=False or sparse=False, is the two-call form: a forward
    call of three kernels that keeps the image, and a backward call.
    sparse=True: 32x32-pixel bins that no triangle's bounding box touches are skipped by every kernel (they can only
    contribute (ref - 255 bg)^2 to the loss, which is added from ref_bg_sumsq: a scalar f64 tensor, the sum of
    reference_background_sumsq(ref_u8, background) over this call's images; computed here when None); same result.
    launch_hints: size the sparse kernels' launches from the bin counts of the previous call on the same batch shape
    (never waited for; the result does not depend on them).  queued_backward (two-call form): the backward
    kernel also runs over the compact list of occupied bins instead of one workgroup per bin (same result).
    enable_mip (sparse mode, either form): the reference's other branch (fit.py:153-155) -- interpolate with the rasteriser's
    screen-space derivatives and texture 'linear-mipmap-linear' with max_mip_level -- inside the same kernels; equals the
    chain rasterize(output_db) -> interpolate(diff_attrs='all') -> texture(texd) -> antialias + pixel loss.
    aa_flags_out (one_pass; tests / diagnostics): a zero-filled int64 tensor of fpcdr_antialias_flags_bytes(B,H,W) / 8 words that
    receives the antialias flag planes (which pixel pairs were blended).  zero_extra (one_pass): a contiguous float32 / int32 tensor of the
    caller's that the call's first kernel zero-fills along with its own buffers (a fit step's small gradient accumulators).
    id_plane_out (one_pass; tests / diagnostics): a zero-filled tensor of fpcdr_idplane_bytes(B,H,W) bytes that is used as the call's id
    planes and so keeps them -- 1024 uint32 per 32 x 32 bin, bin-major, (triangle + 1) | silhouette bits << 24 (include/fpcdr.h).
    record_slots (one_pass): the records of deferred pixels in that many slots of 1 024 (fpcdr_objective_params.rec_slots) instead of the
    default -- by pixel for batches of up to SMALL_BATCH_BINS bins, compact and sized from the last call on the shape beyond; 0 = by pixel.
    skip_out (one_pass): a one-element float32 device tensor that receives 1.0 when the call ran out of record slots -- its value is then
    NaN and its gradients are incomplete -- and 0.0 otherwise, written by the call's last kernel: hand it to GroupedAdam.skip_flag (summed
    over the ranks under data parallelism) and the update of such a step does not happen, without a host read-back.  Without it the
    NEXT call on the batch shape raises.
    WEIGHTS (one_pass, sparse, no mip; DESIGN.md 3, "Weighted objective rule"): robust=(kind, scale) -- 'l2' | 'charbonnier' |
    'geman_mcclure', scale c in grey levels, None for 'l2' --, mask uint8 [B,H,W] (255 = trust, 0 = ignore), face_weights float32 [T]
    (finite, >= 0; check_weights=False for a caller that has checked them), weight_outside for uncovered pixels, saturation 1..255
    (capture pixels at or above it count nothing): the term of ops.robust_pixel_loss on the antialiased image, from the weighted
    instantiations of the same kernels (fpcdr_objective_weighted_fwd) -- the image never exists in memory.  The weights get no gradient;
    the mean's denominator stays n_total.  ref_bg_wsum: f64 [2] or [B,2], reference_background_weighted(...) of this call's images
    (summed over them when [B,2]; computed here when None).  wsum_out: a float64 device tensor whose first element receives the sum of
    all weights of the call (robust_loss_call's sums[1]).  Giving any of these without one_pass and sparse, or with enable_mip, raises
    ValueError; with none given the call is the plain one."""
    assert isinstance(glctx, RasterizeHipContext)
    _check_tensor('pos', pos, torch.float32, 3)
    _check_tensor('tri', tri, torch.int32, 2)
    _check_tensor('uv', uv, torch.float32, 2)
    _check_tensor('uv_tri', uv_tri, torch.int32, 2)
    _check_tensor('tex', tex, torch.float32, 3)
    _check_tensor('ref_u8', ref_u8, torch.uint8, 3)
    H, W = int(resolution[0]), int(resolution[1])
    if tex.shape[2] not in (1, 3, 4):
        raise ValueError("pixel_objective supports 1, 3 or 4 colour channels")
    if ref_u8.shape != (pos.shape[0], H, W):
        raise ValueError("ref_u8 must have shape [B,H,W]")
    if boundary_mode not in _lib.BOUNDARY:
        raise ValueError(f"unknown boundary_mode '{boundary_mode}'")
    tri, ref_u8 = tri.contiguous(), ref_u8.contiguous()
    adj = _cached_topology(tri)
    n_total = n_total or pos.shape[0] * H * W * tex.shape[2]
    one_pass = bool(one_pass and sparse)
    mip_levels = None
    if enable_mip:
        if not sparse:
            raise NotImplementedError("pixel_objective(enable_mip=True) runs in sparse mode (use the separate operators otherwise)")
        mip_levels = _num_mip_levels(tex.shape[0], tex.shape[1], max_mip_level)
    if skip_out is not None and not (torch.is_tensor(skip_out) and skip_out.dtype == torch.float32 and skip_out.device == pos.device
                                     and skip_out.numel() >= 1 and skip_out.is_contiguous()):
        raise ValueError("skip_out must be a contiguous float32 tensor of at least one element on the device of pos")
    if zero_extra is not None:
        # (the kernel zero-fills numel * itemsize bytes from data_ptr(): a view with gaps would have other storage overwritten)
        if not (zero_extra.is_contiguous() and zero_extra.dtype in (torch.float32, torch.int32) and zero_extra.device == pos.device):
            raise ValueError("zero_extra must be a contiguous float32 / int32 tensor on the device of pos")
        if not one_pass:
            zero_extra.zero_()
    weights = _objective_weights(ref_u8, pos.device, int(tri.shape[0]), background, not one_pass or enable_mip, ref_bg_sumsq, robust, mask,
                                 face_weights, weight_outside, saturation, ref_bg_wsum, wsum_out, check_weights)
    if not one_pass and skip_out is not None:      # (what else belongs to the one-pass form alone)
        raise ValueError("skip_out belongs to the one-pass form")
    if not one_pass and record_slots is not None:
        raise ValueError("record_slots belongs to the one-pass form")
    if not one_pass and id_plane_out is not None:
        raise ValueError("id_plane_out is an output of the one-pass form")
    if id_plane_out is not None and (id_plane_out.numel() * id_plane_out.element_size() != _lib.load().fpcdr_idplane_bytes(pos.shape[0], H, W)
                                     or not id_plane_out.is_contiguous() or id_plane_out.device != pos.device):
        raise ValueError("id_plane_out must be a contiguous device tensor of fpcdr_idplane_bytes(B, H, W) bytes")
    opt = _objective_options(H, W, n_total, background, _lib.BOUNDARY[boundary_mode], ref_bg_sumsq, bool(launch_hints), torch.is_grad_enabled(),
                             mip_levels, sparse=bool(sparse), queued_backward=bool(queued_backward), unit_upstream=bool(unit_upstream),
                             flags_out=aa_flags_out, zero_extra=zero_extra, idp_out=id_plane_out, record_slots=record_slots, skip_out=skip_out,
                             weights=weights)
    form = _pixel_objective_onepass if one_pass else _pixel_objective_func
    return form.apply(pos.contiguous(), tex.contiguous(), tri, adj, uv.contiguous(), uv_tri.contiguous(), ref_u8, opt)


# ----------------------------------------------------------------------------------------------
# interpolate
# ----------------------------------------------------------------------------------------------

def _diff_array(diff_list):
    arr = (ctypes.c_int32 * _lib.MAX_ATTR)()
    for i, k in enumerate(diff_list):
        arr[i] = k
    return arr


class _interpolate_func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri, rast_db, diff_list, hint):
        lib = _lib.load()
        B, H, W, _ = rast.shape
        Ba, Vt, A = attr.shape
        n_diff = len(diff_list)
        dev = rast.device
        out = torch.empty(B, H, W, A, dtype=torch.float32, device=dev)
        out_da = torch.empty(B, H, W, 2 * n_diff, dtype=torch.float32, device=dev)
        p = _lib.InterpolateFwd(attr=_ptr(attr), rast=_ptr(rast), tri=_ptr(tri), rast_db=_ptr(rast_db) if n_diff else None,
                                B=B, H=H, W=W, Ba=Ba, Vt=Vt, A=A, T=tri.shape[0], n_diff=n_diff,
                                diff_idx=_diff_array(diff_list), out=_ptr(out), out_da=_ptr(out_da) if n_diff else None,
                                hint=_ptr(hint))
        _lib.call("fpcdr_interpolate_fwd", ctypes.byref(p), _stream())
        ctx.save_for_backward(attr, rast, tri, rast_db if n_diff else None)
        ctx.diff_list = diff_list
        ctx.hint = hint
        return out, out_da

    @staticmethod
    def backward(ctx, dy, dda):
        lib = _lib.load()
        attr, rast, tri, rast_db = ctx.saved_tensors
        B, H, W, _ = rast.shape
        Ba, Vt, A = attr.shape
        diff_list = ctx.diff_list
        n_diff = len(diff_list)
        dev = rast.device
        need_attr = ctx.needs_input_grad[0]
        g_attr = torch.zeros_like(attr) if need_attr else None
        g_rast = torch.empty_like(rast)
        g_db = torch.empty_like(rast_db) if n_diff else None
        dy = dy.contiguous()
        if n_diff:
            dda = dda.contiguous() if dda is not None else torch.zeros(B, H, W, 2 * n_diff, dtype=torch.float32, device=dev)
        p = _lib.InterpolateBwd(attr=_ptr(attr), rast=_ptr(rast), tri=_ptr(tri), rast_db=_ptr(rast_db) if n_diff else None,
                                dy=_ptr(dy), dda=_ptr(dda) if n_diff else None, B=B, H=H, W=W, Ba=Ba, Vt=Vt, A=A,
                                T=tri.shape[0], n_diff=n_diff, diff_idx=_diff_array(diff_list), grad_attr=_ptr(g_attr),
                                grad_rast=_ptr(g_rast), grad_rast_db=_ptr(g_db), hint=_ptr(ctx.hint))
        _lib.call("fpcdr_interpolate_bwd", ctypes.byref(p), _stream())
        return g_attr, g_rast, None, g_db, None, None


def interpolate(attr, rast, tri, rast_db=None, diff_attrs=None):
    """Interpolate vertex attributes.  attr [1|B,Vt,A], rast [B,H,W,4], tri [T,3] -> (out [B,H,W,A], out_da [B,H,W,2D])."""
    _check_tensor('attr', attr, torch.float32)
    _check_tensor('rast', rast, torch.float32, 4)
    _check_tensor('tri', tri, torch.int32, 2)
    if attr.dim() == 2:     # range mode: one shared attribute array
        attr = attr[None]
    if attr.dim() != 3:
        raise ValueError(f"attr must have shape [1|B,Vt,A] (got {tuple(attr.shape)})")
    if rast.shape[3] != 4:
        raise ValueError("rast must have shape [B,H,W,4]")
    if attr.shape[0] not in (1, rast.shape[0]):
        raise ValueError(f"attr minibatch ({attr.shape[0]}) must be 1 or match rast ({rast.shape[0]})")
    if tri.shape[1] != 3:
        raise ValueError("tri must have shape [T,3]")
    A = attr.shape[2]
    if diff_attrs is None or rast_db is None:
        diff_list = []
        if diff_attrs is not None and rast_db is None:
            raise ValueError("diff_attrs given but rast_db is None")
    elif isinstance(diff_attrs, str):
        if diff_attrs != 'all':
            raise ValueError("diff_attrs must be None, 'all' or a list of attribute indices")
        diff_list = list(range(A))
    else:
        diff_list = [int(i) for i in diff_attrs]
        if any(i < 0 or i >= A for i in diff_list):
            raise ValueError("diff_attrs index out of range")
    if len(diff_list) > _lib.MAX_ATTR:
        raise ValueError(f"at most {_lib.MAX_ATTR} attributes may have pixel differentials")
    if diff_list:
        _check_tensor('rast_db', rast_db, torch.float32, 4)
        if rast_db.shape != rast.shape:
            raise ValueError("rast_db must have the same shape as rast")
        rast_db = rast_db.contiguous()
    else:
        rast_db = None
    h = _hint_of(rast, 'rast')
    out, out_da = _interpolate_func.apply(attr.contiguous(), rast.contiguous(), tri.contiguous(), rast_db, diff_list,
                                          h[0] if h else None)
    if h:
        _tag(out, h[0], 'zero')       # no triangle, no attribute: zeros in empty bins
    return out, out_da


# ----------------------------------------------------------------------------------------------
# texture
# ----------------------------------------------------------------------------------------------

def _num_mip_levels(Ht, Wt, max_mip_level):
    n = 0
    h, w = Ht, Wt
    while (max_mip_level is None or n < max_mip_level) and h % 2 == 0 and w % 2 == 0 and h >= 2 and w >= 2:
        h //= 2
        w //= 2
        n += 1
        if n >= _lib.MAX_MIP:
            break
    return n


def _build_mips(tex, n_levels):
    lib = _lib.load()
    chain = [tex]
    for _ in range(n_levels):
        src = chain[-1]
        N, h, w, C = src.shape
        dst = torch.empty(N, h // 2, w // 2, C, dtype=torch.float32, device=tex.device)
        _lib.call("fpcdr_mip_downsample", _ptr(src), _ptr(dst), N, h, w, C, _stream())
        chain.append(dst)
    return chain


class MipStack(list):
    """Levels 1..n of the box-filtered mip chain of `base`, as texture_construct_mip() returns it.  texture(base, ..., mip=stack)
    recognises the pairing (same tensor object, unmodified) and lets the levels' gradients flow back into `base`, as
    nvdiffrast's opaque mip wrapper does; any other list of tensors passed as `mip` is a CUSTOM stack."""

    def __init__(self, levels, base):
        super().__init__(levels)
        self._base = weakref.ref(base)
        self._version = base._version

    def built_from(self, tex):
        return self._base() is tex and tex._version == self._version

    def stale_for(self, tex):
        """Built from this very tensor, which has been modified in place since (an optimiser step): the levels no longer match it."""
        return self._base() is tex and tex._version != self._version


def texture_construct_mip(tex, max_mip_level=None, cube_mode=False):
    """Pre-build a mip stack for `texture(..., mip=...)`.  Returns a MipStack (a list of the level tensors 1..n)."""
    if cube_mode:
        raise NotImplementedError("cube maps are not implemented")
    _check_tensor('tex', tex, torch.float32, 4)
    n = _num_mip_levels(tex.shape[1], tex.shape[2], max_mip_level)
    with torch.no_grad():
        return MipStack(_build_mips(tex.contiguous(), n)[1:], tex)


def _wire_mips(p, chain, g_chain=()):
    """Levels 1..n of a texture's mip chain -- and the buffers of their gradients, when there are any -- into the tex_mip / grad_tex_mip
    tables of an objective's parameter struct."""
    p.mip, p.n_levels = 1, len(chain)
    for l, t in enumerate(chain):
        p.tex_mip[l] = _ptr(t)
        if g_chain:
            p.grad_tex_mip[l] = _ptr(g_chain[l])


def _fold_mip_grads(g_levels):
    """Fold the gradients of a mip chain's levels [N,h,w,C] (level 0 first) into level 0's: the box filter's backward, coarse to fine."""
    for l in range(len(g_levels) - 1, 0, -1):
        N, h, w, C = g_levels[l - 1].shape
        _lib.call("fpcdr_mip_downsample_bwd", _ptr(g_levels[l]), _ptr(g_levels[l - 1]), N, h, w, C, _stream())


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * (_lib.MAX_MIP + 1))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr() if t is not None else None
    return arr


class _texture_func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, uv_da, bias, filter_mode, boundary_mode, n_levels, hint, empty_color, custom, *mips):
        lib = _lib.load()
        B, H, W, _ = uv.shape
        Bt, Ht, Wt, C = tex.shape
        chain = [tex] + list(mips) if mips else _build_mips(tex, n_levels)
        out = torch.empty(B, H, W, C, dtype=torch.float32, device=uv.device)
        p = _lib.TextureFwd(tex=_ptr_array(chain), n_levels=n_levels, uv=_ptr(uv), uv_da=_ptr(uv_da),
                            mip_level_bias=_ptr(bias), B=B, H=H, W=W, Bt=Bt, Ht=Ht, Wt=Wt, C=C,
                            filter_mode=filter_mode, boundary_mode=boundary_mode, out=_ptr(out), hint=_ptr(hint),
                            empty_color=_ptr(empty_color))
        _lib.call("fpcdr_texture_fwd", ctypes.byref(p), _stream())
        ctx.save_for_backward(tex, uv, uv_da, bias, *chain[1:])
        ctx.cfg = (filter_mode, boundary_mode, n_levels)
        ctx.hint = hint
        ctx.custom = bool(custom)     # a caller's own mip tensors: each level keeps its gradient (nvdiffrast: not propagated to tex)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        tex, uv, uv_da, bias = ctx.saved_tensors[:4]
        chain = [tex] + list(ctx.saved_tensors[4:])
        filter_mode, boundary_mode, n_levels = ctx.cfg
        B, H, W, _ = uv.shape
        Bt, Ht, Wt, C = tex.shape
        need_tex = ctx.needs_input_grad[0]
        if ctx.custom:
            need = [need_tex] + [bool(ctx.needs_input_grad[10 + l]) for l in range(len(chain) - 1)]
        else:
            need = [need_tex] * len(chain)
        g_levels = [torch.zeros_like(t) if n else None for t, n in zip(chain, need)]
        g_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] else None
        g_da = torch.empty_like(uv_da) if (uv_da is not None and ctx.needs_input_grad[2]) else None
        g_bias = torch.empty_like(bias) if (bias is not None and ctx.needs_input_grad[3]) else None
        dy = dy.contiguous()
        p = _lib.TextureBwd(tex=_ptr_array(chain), n_levels=n_levels, uv=_ptr(uv), uv_da=_ptr(uv_da),
                            mip_level_bias=_ptr(bias), dy=_ptr(dy), B=B, H=H, W=W, Bt=Bt, Ht=Ht, Wt=Wt, C=C,
                            filter_mode=filter_mode, boundary_mode=boundary_mode, grad_tex=_ptr_array(g_levels),
                            grad_uv=_ptr(g_uv), grad_uv_da=_ptr(g_da), grad_mip_level_bias=_ptr(g_bias), hint=_ptr(ctx.hint))
        _lib.call("fpcdr_texture_bwd", ctypes.byref(p), _stream())
        if ctx.custom:
            return (g_levels[0], g_uv, g_da, g_bias, None, None, None, None, None, None) + tuple(g_levels[1:])
        if need_tex:
            _fold_mip_grads(g_levels)
        return (g_levels[0], g_uv, g_da, g_bias, None, None, None, None, None, None) + (None,) * (len(chain) - 1)


def texture(tex, uv, uv_da=None, mip_level_bias=None, mip=None, filter_mode='auto', boundary_mode='wrap',
            max_mip_level=None):
    """Texture lookup.  tex [1|B,Ht,Wt,C], uv [B,H,W,2], uv_da [B,H,W,4] -> [B,H,W,C]."""
    if filter_mode == 'auto':
        filter_mode = 'linear-mipmap-linear' if (uv_da is not None or mip_level_bias is not None) else 'linear'
    if filter_mode not in _lib.FILTER:
        raise ValueError(f"unknown filter_mode '{filter_mode}'")
    if boundary_mode == 'cube':
        raise NotImplementedError("cube maps are not implemented")
    if boundary_mode not in _lib.BOUNDARY:
        raise ValueError(f"unknown boundary_mode '{boundary_mode}'")
    _check_tensor('tex', tex, torch.float32, 4)
    _check_tensor('uv', uv, torch.float32, 4)
    if uv.shape[3] != 2:
        raise ValueError("uv must have shape [B,H,W,2]")
    if tex.shape[0] not in (1, uv.shape[0]):
        raise ValueError(f"tex minibatch ({tex.shape[0]}) must be 1 or match uv ({uv.shape[0]})")
    mipped = filter_mode in ('linear-mipmap-nearest', 'linear-mipmap-linear')
    n_levels = 0
    mips = ()
    custom = False
    if mipped:
        if uv_da is None and mip_level_bias is None:
            raise ValueError("mipmapped filter modes need uv_da and/or mip_level_bias")
        if uv_da is not None:
            _check_tensor('uv_da', uv_da, torch.float32, 4)
            if uv_da.shape != uv.shape[:3] + (4,):
                raise ValueError("uv_da must have shape [B,H,W,4]")
            uv_da = uv_da.contiguous()
        if mip_level_bias is not None:
            _check_tensor('mip_level_bias', mip_level_bias, torch.float32, 3)
            if mip_level_bias.shape != uv.shape[:3]:
                raise ValueError("mip_level_bias must have shape [B,H,W]")
            mip_level_bias = mip_level_bias.contiguous()
        if mip is not None:
            # a stack texture_construct_mip() built from this very tensor behaves like the internal chain (its gradient
            # collapses into tex); any other list of tensors is a custom stack whose levels receive their own gradients
            if isinstance(mip, MipStack) and mip.stale_for(tex):
                # (silently demoting it to a custom stack would sample stale levels AND cut their gradient off from tex, where
                # nvdiffrast's mip wrapper keeps propagating it)
                raise RuntimeError("texture(): `mip` was built by texture_construct_mip() from this tensor, which has been modified in "
                                   "place since (e.g. an optimiser step): rebuild the stack, or pass mip=None to build it per call")
            custom = not (isinstance(mip, MipStack) and mip.built_from(tex))
            mips = tuple(m.contiguous() for m in mip)
            n_levels = min(len(mips), _lib.MAX_MIP)
            if max_mip_level is not None:
                n_levels = min(n_levels, int(max_mip_level))
            mips = mips[:n_levels]
            h, w = tex.shape[1], tex.shape[2]
            for l, m in enumerate(mips):
                _check_tensor(f'mip[{l}]', m, torch.float32, 4)
                h, w = h // 2, w // 2
                if tuple(m.shape) != (tex.shape[0], h, w, tex.shape[3]):
                    raise ValueError(f"mip level {l + 1} must have shape {(tex.shape[0], h, w, tex.shape[3])} (got {tuple(m.shape)})")
        else:
            n_levels = _num_mip_levels(tex.shape[1], tex.shape[2], max_mip_level)
    else:
        uv_da = None
        mip_level_bias = None
    h = _hint_of(uv, 'zero') if (not mipped and tex.shape[0] == 1) else None
    empty_color = torch.empty(tex.shape[3], dtype=torch.float32, device=uv.device) if h else None
    out = _texture_func.apply(tex.contiguous(), uv.contiguous(), uv_da, mip_level_bias, _lib.FILTER[filter_mode],
                              _lib.BOUNDARY[boundary_mode], n_levels, h[0] if h else None, empty_color, custom, *mips)
    if h:
        _tag(out, h[0], 'const', empty_color)     # uv = (0,0) in empty bins: the texture's value there
    return out


# ----------------------------------------------------------------------------------------------
# antialias
# ----------------------------------------------------------------------------------------------

_topology_cache = OrderedDict()
_TOPOLOGY_CACHE_SIZE = 16


def antialias_construct_topology_hash(tri):
    """Edge adjacency of `tri` ([T,3] i32): adj [T,3] i32 (see include/fpcdr.h).  Built on the GPU."""
    _check_tensor('tri', tri, torch.int32, 2)
    lib = _lib.load()
    tri = tri.contiguous()
    T = tri.shape[0]
    scratch = torch.empty(lib.fpcdr_topology_scratch_bytes(T), dtype=torch.uint8, device=tri.device)
    adj = torch.empty(T, 3, dtype=torch.int32, device=tri.device)
    _lib.call("fpcdr_topology_build", _ptr(tri), T, _ptr(scratch), _ptr(adj), _stream())
    return adj


_tri_uv_cache = OrderedDict()


def _cached_tri_uv(uv, uv_tri):
    """uv[uv_tri] as [T,3,2], gathered once per (uv, uv_tri) pair: static per mesh, saves a dependent load per pixel."""
    key = (uv.data_ptr(), uv._version, uv_tri.data_ptr(), uv_tri._version, tuple(uv.shape), tuple(uv_tri.shape), str(uv.device))
    hit = _tri_uv_cache.get(key)
    if hit is not None:
        _tri_uv_cache.move_to_end(key)
        return hit[2]
    out = uv.detach()[uv_tri.long()].contiguous()
    _tri_uv_cache[key] = (uv, uv_tri, out)     # holding the tensors keeps their storage (and so the key) alive
    while len(_tri_uv_cache) > _TOPOLOGY_CACHE_SIZE:
        _tri_uv_cache.popitem(last=False)
    return out


def _cached_topology(tri):
    key = (tri.data_ptr(), tri._version, tuple(tri.shape), str(tri.device))
    hit = _topology_cache.get(key)
    if hit is not None:
        _topology_cache.move_to_end(key)
        return hit[1]
    adj = antialias_construct_topology_hash(tri)
    _topology_cache[key] = (tri, adj)  # holding `tri` keeps its storage (and so the key) alive
    while len(_topology_cache) > _TOPOLOGY_CACHE_SIZE:
        _topology_cache.popitem(last=False)
    return adj


class _antialias_func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, adj, boost, hint, empty_color):
        lib = _lib.load()
        B, H, W, C = color.shape
        V, T = pos.shape[1], tri.shape[0]
        dev = color.device
        out = torch.empty_like(color)
        sil = torch.empty(B, T, dtype=torch.uint8, device=dev)
        flags = torch.empty(lib.fpcdr_antialias_flags_bytes(B, H, W) // 8, dtype=torch.int64, device=dev)
        p = _lib.AntialiasFwd(color=_ptr(color), rast=_ptr(rast), pos=_ptr(pos), tri=_ptr(tri), adj=_ptr(adj), B=B, H=H,
                              W=W, C=C, V=V, T=T, sil=_ptr(sil), flags=_ptr(flags), out=_ptr(out), hint=_ptr(hint),
                              empty_color=_ptr(empty_color))
        _lib.call("fpcdr_antialias_fwd", ctypes.byref(p), _stream())
        ctx.save_for_backward(color, rast, pos, tri, adj, sil, flags)
        ctx.boost = float(boost)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        color, rast, pos, tri, adj, sil, flags = ctx.saved_tensors
        B, H, W, C = color.shape
        V, T = pos.shape[1], tri.shape[0]
        g_color = torch.empty_like(color)
        g_pos = torch.zeros_like(pos)
        dy = dy.contiguous()
        p = _lib.AntialiasBwd(color=_ptr(color), rast=_ptr(rast), pos=_ptr(pos), tri=_ptr(tri), adj=_ptr(adj), dy=_ptr(dy),
                              B=B, H=H, W=W, C=C, V=V, T=T, sil=_ptr(sil), flags=_ptr(flags),
                              pos_gradient_boost=ctx.boost, grad_color=_ptr(g_color), grad_pos=_ptr(g_pos))
        _lib.call("fpcdr_antialias_bwd", ctypes.byref(p), _stream())
        return g_color, None, g_pos, None, None, None, None, None


def antialias(color, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0):
    """Silhouette antialiasing.  color [B,H,W,C], rast [B,H,W,4], pos [B,V,4], tri [T,3] -> [B,H,W,C]."""
    _check_tensor('color', color, torch.float32, 4)
    _check_tensor('rast', rast, torch.float32, 4)
    _check_tensor('pos', pos, torch.float32)
    _check_tensor('tri', tri, torch.int32, 2)
    if pos.dim() == 2:      # range mode: one shared vertex array for the whole minibatch (its gradient sums over the images)
        pos = pos[None].expand(color.shape[0], -1, -1)
    if pos.dim() != 3 or pos.shape[2] != 4:
        raise ValueError("pos must have shape [B,V,4]")
    if color.shape[:3] != rast.shape[:3] or rast.shape[3] != 4:
        raise ValueError("color [B,H,W,C] and rast [B,H,W,4] must agree in B, H, W")
    if pos.shape[0] != color.shape[0]:
        raise ValueError("pos minibatch must match color")
    tri = tri.contiguous()
    if topology_hash is None:
        adj = _cached_topology(tri)
    else:
        adj = topology_hash
        _check_tensor('topology_hash', adj, torch.int32, 2)
        if adj.shape != tri.shape:
            raise ValueError("topology_hash does not belong to this tri tensor")
    hr = _hint_of(rast, 'rast')
    hc = _hint_of(color, 'const') if hr else None
    if hc is not None and hc[0] is not hr[0]:     # a colour image from another rasterisation
        hc = None
    return _antialias_func.apply(color.contiguous(), rast.contiguous(), pos.contiguous(), tri, adj, pos_gradient_boost,
                                 hr[0] if hr else None, hc[1] if hc else None)

"""
Mesh regularisers (pytorch3d in the reference: fit.py:16-19, 578-582): the static tables of a triangle list (MeshTopology, the hinge
tables, RestShape), the torch restatements of the reference's terms, and the penalties whose device code is csrc/mesh_reg.hip
(laplacian_penalty, stretch_penalty, bend_penalty within a mesh, motion_penalty across the frames).  fit.py imports these names:
fit.MeshTopology, fit.laplacian_penalty, ... remain the documented spelling.
"""
import numpy as np
import torch

from . import _lib
from .ops import _ptr, _stream


class MeshTopology:
    """Edges and uniform-Laplacian structure of a triangle list, built once (the reference rebuilds a
    pytorch3d Meshes object every iteration, fit.py:578)."""

    def __init__(self, faces, n_vertices, device):
        f = np.asarray(faces, dtype=np.int64)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
        e = np.unique(np.sort(e, axis=1), axis=0)
        self.edges = torch.tensor(e, dtype=torch.long, device=device)
        deg = np.bincount(e.reshape(-1), minlength=n_vertices).astype(np.int64)
        self.inv_deg = torch.tensor(np.where(deg > 0, 1.0 / np.maximum(deg, 1), 0.0), dtype=torch.float32, device=device)
        self.n_vertices = n_vertices
        # padded one-ring table [V, Dmax]; the pad index V points at an all-zero row appended to the vertex buffer
        dmax = int(deg.max()) if deg.size else 0
        nbr = np.full((n_vertices, max(dmax, 1)), n_vertices, dtype=np.int64)
        fill = np.zeros(n_vertices, dtype=np.int64)
        for a, b in e:
            nbr[a, fill[a]] = b; fill[a] += 1
            nbr[b, fill[b]] = a; fill[b] += 1
        # interior edges (exactly two incident faces) with those faces, for the normal-consistency term
        self.faces = torch.tensor(f, dtype=torch.long, device=device)
        fe = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0), axis=1)
        fid = np.tile(np.arange(f.shape[0]), 3)
        key = fe[:, 0] * (n_vertices + 1) + fe[:, 1]
        order = np.argsort(key, kind='stable')
        ks, fs = key[order], fid[order]
        first = np.concatenate([[True], ks[1:] != ks[:-1]])
        starts = np.nonzero(first)[0]
        counts = np.diff(np.concatenate([starts, [len(ks)]]))
        two = starts[counts == 2]
        self.edge_faces = (torch.tensor(fs[two], dtype=torch.long, device=device),
                           torch.tensor(fs[two + 1], dtype=torch.long, device=device))
        self.nbr = torch.tensor(nbr, dtype=torch.long, device=device)
        self.nbr32 = self.nbr.to(torch.int32).t().contiguous()      # [Dmax, V] slot-major for the gather kernel
        self._hinge_key, self._hinges = ks[two], None      # (the edges of edge_faces, for hinges())

    def hinges(self):
        """The bending term's tables ("Bend rule"), built on the first call and kept: (hinge_vtx [4,H] int32, hinge_inc [K,V]
        int32, H, K) on the topology's device.  The hinges are the edges of edge_faces, in that order."""
        if self._hinges is None:
            dev = self.faces.device
            f0, f1 = (t.cpu().numpy() for t in self.edge_faces)
            hv = hinge_vertices(self.faces.cpu().numpy(), f0, f1, self._hinge_key // (self.n_vertices + 1),
                                self._hinge_key % (self.n_vertices + 1))
            inc = hinge_incidence(hv, self.n_vertices)
            self._hinges = (torch.from_numpy(hv).to(dev), torch.from_numpy(inc).to(dev), int(hv.shape[1]), int(inc.shape[0]))
        return self._hinges


def hinge_vertices(faces, fa, fb, lo, hi):
    """hinge_vtx [4,H] int32 (role-major: p0, p1, q0, q1) for the hinges with faces (fa, fb) on the edges {lo, hi}: f0 = the lower face
    index, p0 -> p1 the edge in the direction f0 runs through it, q0 / q1 the third vertex of f0 / f1; a hinge whose f1 runs through the
    edge in the same direction (sigma = -1) stores -1 - q1.  numpy, no loop over the hinges."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    f0, f1 = np.minimum(fa, fb), np.maximum(fa, fb)
    ar = np.arange(f0.shape[0])

    def locate(tri):      # the corner k at which the face runs tri[k] -> tri[k + 1] along the edge, either way
        nxt = tri[:, [1, 2, 0]]
        on = ((tri == lo[:, None]) & (nxt == hi[:, None])) | ((tri == hi[:, None]) & (nxt == lo[:, None]))
        k = np.argmax(on, axis=1)
        return tri[ar, k], tri[ar, (k + 1) % 3], tri[ar, (k + 2) % 3]

    p0, p1, q0 = locate(f[f0])
    b0, _, q1 = locate(f[f1])
    q1 = np.where(b0 == p1, q1, -1 - q1)
    return np.stack([p0, p1, q0, q1]).astype(np.int32).reshape(4, -1)


def hinge_incidence(hinge_vtx, n_vertices):
    """hinge_inc [K,V] int32, slot-major: the hinge corners 4 h + role at every vertex, ascending; pads -1 trailing; K = the largest
    count over the vertices, at least 1."""
    hv = np.asarray(hinge_vtx, dtype=np.int64)
    hv = np.where(hv < 0, -1 - hv, hv)
    at = hv.T.reshape(-1)                                 # the vertex of corner 4 h + role
    order = np.argsort(at, kind='stable')
    counts = np.bincount(at, minlength=n_vertices)
    K = max(int(counts.max()) if counts.size else 0, 1)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    sorted_at = at[order]
    inc = np.full((K, n_vertices), -1, dtype=np.int32)
    inc[np.arange(order.shape[0]) - starts[sorted_at], sorted_at] = order
    return inc


def hinge_rest_cs(hinge_vtx, v_rest):
    """rest_cs [2,H] float32 = (cos, sin) of every hinge's dihedral angle in the rest shape, by the Bend rule's expressions in float64 from
    the float32 rest positions [V,3], rounded once; a hinge degenerate at rest gets (1, 0)."""
    hv = np.asarray(hinge_vtx, dtype=np.int64)
    x = v_rest.detach().to('cpu', torch.float32).reshape(-1, 3).numpy().astype(np.float64)
    sigma = np.where(hv[3] < 0, -1.0, 1.0)[:, None]
    p0, p1, q0, q1 = x[hv[0]], x[hv[1]], x[hv[2]], x[np.where(hv[3] < 0, -1 - hv[3], hv[3])]
    e = p1 - p0
    n0, n1 = np.cross(e, q0 - p0), sigma * np.cross(q1 - p0, e)
    e2, m0, m1 = (e * e).sum(1), (n0 * n0).sum(1), (n1 * n1).sum(1)
    live = (e2 > 0) & (m0 > 0) & (m1 > 0)
    safe = lambda a: np.sqrt(np.where(live, a, 1.0))[:, None]
    u0, u1, eh = n0 / safe(m0), n1 / safe(m1), e / safe(e2)
    c = np.where(live, (u0 * u1).sum(1), 1.0)
    s = np.where(live, (np.cross(u0, u1) * eh).sum(1), 0.0)
    return torch.from_numpy(np.stack([c, s]).astype(np.float32).reshape(2, -1))


def _require_gpu(verts, entry):
    if not verts.is_cuda:
        raise RuntimeError(f"the mesh regularisers run on the GPU only ({entry}); there is no CPU fallback")


class _uniform_laplacian(torch.autograd.Function):
    """L X with L = D^-1 A - I for a batch of vertex buffers [F,V,3].  Forward and backward are both GATHERS over the
    static one-ring table (L^T = A D^-1 - I), so no scatter / index_put runs in the step (fpcdr_laplacian_gather)."""

    @staticmethod
    def _apply(x, nbr, nbr32, inv_deg, transpose):
        _require_gpu(x, "fpcdr_laplacian_gather")
        x = x.contiguous()
        out = torch.empty_like(x)
        _lib.call("fpcdr_laplacian_gather", _ptr(x), _ptr(nbr32), _ptr(inv_deg), _ptr(out), x.shape[0], x.shape[1],
                  nbr32.shape[0], 1 if transpose else 0, _stream())
        return out

    @staticmethod
    def forward(ctx, verts, nbr, nbr32, inv_deg):
        ctx.save_for_backward(nbr, nbr32, inv_deg)
        return _uniform_laplacian._apply(verts, nbr, nbr32, inv_deg, False)

    @staticmethod
    def backward(ctx, g):
        nbr, nbr32, inv_deg = ctx.saved_tensors
        return _uniform_laplacian._apply(g, nbr, nbr32, inv_deg, True), None, None, None


def mesh_laplacian_smoothing(verts, topo, per_mesh=False, rest=None):
    """Uniform Laplacian smoothing (pytorch3d mesh_laplacian_smoothing(method='uniform'), reference fit.py:581):
    mean_v || mean_{n in N(v)} x_n - x_v || of every mesh of verts [F,V,3]; per_mesh=True returns the [F] values, else
    their mean.  rest (a RestShape): the differentials are measured against the rest shape's, || L x - L x_rest ||."""
    lap = _uniform_laplacian.apply(verts, topo.nbr, topo.nbr32, topo.inv_deg)
    if rest is not None:
        lap = lap - rest.lap[None]
    per = lap.norm(dim=2).mean(dim=1)
    return per if per_mesh else per.mean()


class _penalty(torch.autograd.Function):
    """The host path the penalties share.  Each is one C-ABI call that ends in the finish kernel (csrc/mesh_reg.hip), and each can
    make its gradient for a unit upstream in forward() already (the terms depend on the vertices only)."""

    @staticmethod
    def begin(ctx, n_inputs, entry, verts, acc, unit):
        """The device check and the buffers of the finish contract: (x, acc, per [F], out) for the vertices x [F,V,3], contiguous.
        acc: F + 1 doubles, zero on entry -- and the call leaves them zero again, so a caller that hands over its own buffer (the
        Fitter: one per instance) saves the fill launch of a fresh one per step."""
        _require_gpu(verts, entry)
        x = verts.contiguous()
        F = x.shape[0]
        if acc is None:
            acc = torch.zeros(F + 1, dtype=torch.float64, device=x.device)
        assert acc.dtype == torch.float64 and acc.numel() >= F + 1 and acc.is_contiguous()
        ctx.n_inputs, ctx.unit = n_inputs, bool(unit)
        return x, acc, torch.empty(F, dtype=torch.float32, device=x.device), torch.empty((), dtype=torch.float32, device=x.device)

    @staticmethod
    def backward(ctx, g):
        """The eager hand-over: the gradient buffer saved by forward() times the upstream scalar, or as it is with unit (the caller
        guarantees d loss / d value = 1)."""
        gx, = ctx.saved_tensors
        return ((gx if ctx.unit else gx * g.to(torch.float32)),) + (None,) * (ctx.n_inputs - 1)


class _laplacian_penalty(_penalty):
    """weight * mean_f (mean_v ||(L x_f)_v||)^2 in one launch each way (fpcdr_laplacian_penalty_fwd / _bwd).
    eager: the gradient kernel runs in forward() already, backward() is _penalty's.  Lazy (the one term with such a mode): the gradient
    kernel runs in backward() with the upstream scalar as its argument, which rounds differently from gradient * upstream."""

    @staticmethod
    def forward(ctx, verts, nbr32, inv_deg, weight, eager=False, unit=False, acc=None, rest_lap=None):
        x, acc, per, out = _penalty.begin(ctx, 8, "fpcdr_laplacian_penalty_fwd", verts, acc, unit)
        F, V, _ = x.shape
        eager = bool(eager and ctx.needs_input_grad[0])
        lap = torch.empty_like(x)
        if rest_lap is None:
            _lib.call("fpcdr_laplacian_penalty_fwd", _ptr(x), _ptr(nbr32), _ptr(inv_deg), _ptr(lap), _ptr(acc), _ptr(per), _ptr(out),
                      float(weight), F, V, nbr32.shape[0], _stream())
        else:      # lap = L x - L x_rest; the backward kernel takes it as it takes L x
            assert rest_lap.shape == (V, 3) and rest_lap.dtype == torch.float32 and rest_lap.is_contiguous() and rest_lap.device == x.device
            _lib.call("fpcdr_laplacian_penalty_rest_fwd", _ptr(x), _ptr(nbr32), _ptr(inv_deg), _ptr(rest_lap), _ptr(lap), _ptr(acc),
                      _ptr(per), _ptr(out), float(weight), F, V, nbr32.shape[0], _stream())
        ctx.weight, ctx.eager = float(weight), eager
        if eager:
            ctx.save_for_backward(_laplacian_penalty._grad(lap, nbr32, inv_deg, per, _unit_scalar(x.device), ctx.weight))
        else:
            ctx.save_for_backward(lap, nbr32, inv_deg, per)
        return out

    @staticmethod
    def _grad(lap, nbr32, inv_deg, per, upstream, weight):
        gx = torch.empty_like(lap)
        _lib.call("fpcdr_laplacian_penalty_bwd", _ptr(lap), _ptr(nbr32), _ptr(inv_deg), _ptr(per), _ptr(upstream), _ptr(gx), weight,
                  lap.shape[0], lap.shape[1], nbr32.shape[0], _stream())
        return gx

    @staticmethod
    def backward(ctx, g):
        if ctx.eager:
            return _penalty.backward(ctx, g)
        return (_laplacian_penalty._grad(*ctx.saved_tensors, g.to(torch.float32).contiguous(), ctx.weight),) + (None,) * 7


_unit_scalars = {}


def _unit_scalar(dev):
    """A device-resident 1.0f (the upstream of a gradient computed ahead of backward())."""
    t = _unit_scalars.get(dev)
    if t is None:
        t = _unit_scalars[dev] = torch.ones((), dtype=torch.float32, device=dev)
    return t


def laplacian_penalty(verts, topo, weight, eager_grad=False, unit_upstream=False, acc=None, rest=None):
    """weight * mean over the meshes of verts [F,V,3] of mesh_laplacian_smoothing(mesh)^2 -- the reference's term (fit.py:581 squares
    the value of the ONE mesh of its step) -- as two launches per step instead of a gather and fifteen torch kernels.
    eager_grad: the gradient is computed with the value (backward() only multiplies by the upstream scalar, or not at all with
    unit_upstream).  acc: see _penalty.begin.  rest (a RestShape): the term measures against the rest shape, L x - L x_rest
    in place of L x ("Rest Laplacian rule"): exactly 0, value and gradient, at the rest shape itself."""
    return _laplacian_penalty.apply(verts, topo.nbr32, topo.inv_deg, weight, eager_grad, unit_upstream, acc,
                                    None if rest is None else rest.lap)


def rest_edge_lengths(nbr32, v_rest):
    """rest_len [D,V] float32 for the slot-major one-ring table nbr32 [D,V] (MeshTopology.nbr32): || x_rest[nbr[d][v]] - x_rest[v] ||,
    formed in float64 on the host from the float32 rest positions [V,3] and rounded once -- both ends of an edge hold the same number;
    pads 0.  Also the number of edges (sum of the degrees / 2)."""
    nbr = nbr32.detach().cpu().numpy().astype(np.int64)
    x = v_rest.detach().to('cpu', torch.float32).reshape(-1, 3).numpy().astype(np.float64)
    V = x.shape[0]
    assert nbr.shape[1] == V
    real = nbr < V
    d = x[np.where(real, nbr, 0)] - x[None]
    length = np.where(real, np.sqrt((d * d).sum(axis=2)), 0.0)
    n_real = int(real.sum())
    assert n_real % 2 == 0
    return torch.from_numpy(length.astype(np.float32)), n_real // 2


class RestShape:
    """What the rest-shape regularisers need of a rest mesh, built once: .lap [V,3] = L x_rest, .len [D,V] the rest length of every slot of
    topo.nbr32, .n_edges, and .bend_cs [2,H] the rest dihedral angles of topo.hinges() (made when first asked for).  .lap comes from the
    device code that forms the term's own L x (fpcdr_laplacian_penalty_rest_fwd without a rest), so that L x - .lap is exactly 0 at the
    rest shape; on a CPU topology it is None (the Laplacian runs on the GPU only)."""

    def __init__(self, topo, v_rest):
        dev = topo.nbr32.device
        x = v_rest.detach().to(torch.float32).reshape(1, -1, 3).contiguous()
        V, D = x.shape[1], topo.nbr32.shape[0]
        assert V == topo.n_vertices
        length, self.n_edges = rest_edge_lengths(topo.nbr32, x)
        self.len = length.to(dev)
        self.lap = None
        self._topo, self._x_rest, self._bend_cs = topo, x, None      # (for bend_cs: nothing of it is built until somebody asks)
        if dev.type == 'cuda':
            x = x.to(dev)
            lap = torch.empty_like(x)
            acc = torch.zeros(2, dtype=torch.float64, device=dev)
            per, out = torch.empty(1, dtype=torch.float32, device=dev), torch.empty((), dtype=torch.float32, device=dev)
            _lib.call("fpcdr_laplacian_penalty_rest_fwd", _ptr(x), _ptr(topo.nbr32), _ptr(topo.inv_deg), None, _ptr(lap), _ptr(acc),
                      _ptr(per), _ptr(out), 0.0, 1, V, D, _stream())
            self.lap = lap[0]

    @property
    def bend_cs(self):
        """[2,H] float32 (cos, sin) of the rest dihedral angle of every hinge of topo.hinges(), built on first use."""
        if self._bend_cs is None:
            self._bend_cs = hinge_rest_cs(self._topo.hinges()[0].cpu().numpy(), self._x_rest).to(self._topo.nbr32.device)
        return self._bend_cs


class _stretch_penalty(_penalty):
    """weight * mean_f mean_edges (|e| - l)^2 with its gradient from ONE call (fpcdr_stretch_penalty): the kernel that walks a vertex's
    ring for the value has everything the gradient at that vertex needs, so the gradient for a unit upstream is always made in
    forward(); backward() is _penalty's."""

    @staticmethod
    def forward(ctx, verts, nbr32, rest_len, n_edges, target, weight, unit=False, acc=None):
        x, acc, per, out = _penalty.begin(ctx, 8, "fpcdr_stretch_penalty", verts, acc, unit)
        F, V, _ = x.shape
        if rest_len is not None:
            assert rest_len.shape == nbr32.shape and rest_len.dtype == torch.float32 and rest_len.is_contiguous() and rest_len.device == x.device
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _lib.call("fpcdr_stretch_penalty", _ptr(x), _ptr(nbr32), _ptr(rest_len), float(target), _ptr(gx), _ptr(acc), _ptr(per), _ptr(out),
                  float(weight), F, V, nbr32.shape[0], int(n_edges), _stream())
        if gx is not None:
            ctx.save_for_backward(gx)
        return out


def stretch_penalty(verts, topo, weight, rest=None, target=0.0, eager_grad=False, unit_upstream=False, acc=None):
    """weight * mean over the meshes of verts [F,V,3] and over the edges of (|e| - l)^2 ("Stretch rule"): l the edge's length
    in `rest` (a RestShape), or the constant `target` without one -- stretch_penalty(v, topo, w, target=0.1) is w * mesh_edge_loss(v, topo, 0.1),
    the reference's term (fit.py:580).  The modes are laplacian_penalty's: lazy, eager_grad, and eager_grad with unit_upstream (the caller
    guarantees d loss / d value = 1: backward() hands the gradient buffer over).  The one call makes the gradient with the value in every
    mode, so lazy and eager_grad differ in nothing but the name.  acc: see _penalty.begin."""
    if rest is None:
        rest_len, n_edges = None, int(topo.edges.shape[0])
    else:
        rest_len, n_edges = rest.len, rest.n_edges
    return _stretch_penalty.apply(verts, topo.nbr32, rest_len, n_edges, target, weight, bool(eager_grad and unit_upstream), acc)


class _bend_penalty(_penalty):
    """weight * mean_f mean_hinges (1 - cos(theta - theta_rest)) with its gradient from ONE call (fpcdr_bend_penalty): a pass over the
    hinges leaves every corner's gradient in a scratch, a gather sums them per vertex.  As with _stretch_penalty the gradient for a unit
    upstream is made in forward(); backward() is _penalty's."""

    @staticmethod
    def forward(ctx, verts, hinge_vtx, hinge_inc, rest_cs, weight, unit=False, acc=None, scratch=None):
        x, acc, per, out = _penalty.begin(ctx, 8, "fpcdr_bend_penalty", verts, acc, unit)
        F, V, _ = x.shape
        H, K = hinge_vtx.shape[1], hinge_inc.shape[0]
        assert hinge_vtx.dtype == torch.int32 and hinge_inc.dtype == torch.int32 and hinge_inc.shape[1] == V and hinge_vtx.device == x.device
        if rest_cs is not None:
            assert rest_cs.shape == (2, H) and rest_cs.dtype == torch.float32 and rest_cs.is_contiguous() and rest_cs.device == x.device
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            if scratch is None:      # the corners' gradients, F * H * 12 floats (a caller that keeps one saves the allocation per step)
                scratch = torch.empty(max(F * H * 12, 1), dtype=torch.float32, device=x.device)
            assert scratch.dtype == torch.float32 and scratch.numel() >= F * H * 12 and scratch.is_contiguous() and scratch.device == x.device
        _lib.call("fpcdr_bend_penalty", _ptr(x), _ptr(hinge_vtx), _ptr(rest_cs), _ptr(hinge_inc), _ptr(scratch) if gx is not None else None,
                  _ptr(gx), _ptr(acc), _ptr(per), _ptr(out), float(weight), F, V, H, K, _stream())
        if gx is not None:
            ctx.save_for_backward(gx)
        return out


def bend_penalty(verts, topo, weight, rest=None, eager_grad=False, unit_upstream=False, acc=None, scratch=None):
    """weight * mean over the meshes of verts [F,V,3] and over the hinges of 1 - cos(theta - theta_rest) ("Bend rule"):
    theta the signed dihedral angle, theta_rest the hinge's angle in `rest` (a RestShape), or 0 without one -- bend_penalty(v, topo, w) is
    w * mesh_normal_consistency(v, topo), the reference's term (fit.py:582).  The modes and `acc` are stretch_penalty's.  scratch: a float32
    buffer of at least F * H * 12 elements for the corners' gradients (None: one is allocated per call)."""
    hinge_vtx, hinge_inc, _, _ = topo.hinges()
    return _bend_penalty.apply(verts, hinge_vtx, hinge_inc, None if rest is None else rest.bend_cs, weight,
                               bool(eager_grad and unit_upstream), acc, scratch)


def _inv_scale(scale, whose, refuse_bool=False):
    """1 / scale as the float32 a kernel is handed as its Charbonnier inv_c, 0.0 for None (L2); ValueError ("<whose> scale ...") for a
    scale that is not finite and positive (refuse_bool: or is a bool), or whose inverse is not a finite positive float32."""
    if scale is None:
        return 0.0
    try:
        c = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"{whose} scale must be a number (got {scale!r})")
    if (refuse_bool and isinstance(scale, bool)) or not (np.isfinite(c) and c > 0.0):
        raise ValueError(f"{whose} scale must be finite and positive (got {scale!r})")
    with np.errstate(over='ignore'):
        inv = float(np.float32(1.0 / c))
    if not (np.isfinite(inv) and inv > 0.0):
        raise ValueError(f"{whose} scale {scale!r} has no finite positive inverse in float32")
    return inv


def _check_item_weights(w, shape, option, item):
    """How every loader of a per-<item> weight option of FitConfig ends: w (float64) as a contiguous float32 array of `shape`, or ValueError."""
    if w.shape != tuple(shape):
        raise ValueError(f"FitConfig.{option} holds one number per {item}: expected [{','.join(map(str, shape))}], got shape {tuple(w.shape)}")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError(f"FitConfig.{option} must be finite and not negative")
    return np.ascontiguousarray(w.astype(np.float32))


def motion_inv_scale(scale):
    """fpcdr_motion_penalty's inv_c for a scale in the length units of the vertices (_inv_scale: 0.0 for None, or ValueError)."""
    return _inv_scale(scale, "the motion term's")


def check_motion_options(cfg):
    """What FitConfig's motion fields ask of each other (FitConfig.__post_init__), or ValueError.  Needs no GPU; what needs the mesh and
    the shard is fit.motion_options."""
    if isinstance(cfg.motion_order, bool) or cfg.motion_order not in (1, 2):
        raise ValueError(f"FitConfig.motion_order must be 1 (velocity) or 2 (acceleration) (got {cfg.motion_order!r})")
    try:
        motion_inv_scale(cfg.motion_scale)
    except ValueError as e:
        raise ValueError(f"FitConfig.motion_scale: {e}")
    if cfg.weight_motion and 0 < cfg.frames_per_step < cfg.motion_order + 1:
        raise ValueError(f"FitConfig.weight_motion > 0 with motion_order={cfg.motion_order} needs frames_per_step = 0 or >= "
                         f"{cfg.motion_order + 1} (got {cfg.frames_per_step}): fewer frames hold no stencil")


def _check_motion_order(order):
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"the motion term's order must be 1 (velocity) or 2 (acceleration) (got {order!r})")
    return int(order)


class _motion_penalty(_penalty):
    """weight / F * sum_f m_f mean_v w_v rho(|a_{f,v}|^2) with its gradient from ONE call (fpcdr_motion_penalty): the lane of a (frame,
    vertex) reads the frames around its own, so the gradient for a unit upstream is always made in forward(); backward() is _penalty's."""

    @staticmethod
    def forward(ctx, verts, frame_ids, vertex_w, inv_c, order, weight, unit=False, acc=None):
        x, acc, per, out = _penalty.begin(ctx, 8, "fpcdr_motion_penalty", verts, acc, unit)
        F, V, _ = x.shape
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        _lib.call("fpcdr_motion_penalty", _ptr(x), _ptr(frame_ids), _ptr(vertex_w), float(inv_c), int(order), _ptr(gx), _ptr(acc),
                  _ptr(per), _ptr(out), float(weight), F, V, _stream())
        if gx is not None:
            ctx.save_for_backward(gx)
        return out


def motion_penalty(verts, weight, frame_ids=None, order=2, scale=None, vertex_weights=None, eager_grad=False, unit_upstream=False,
                   acc=None, validate=True):
    """weight / F * sum over the meshes of verts [F,V,3] of m_f * mean_v w_v rho(|a_{f,v}|^2) ("Motion rule"): a the
    acceleration x_{f-1} - 2 x_f + x_{f+1} (order 2) or the velocity x_{f+1} - x_f (order 1) of a vertex across the frames, m_f = 1 where
    the frames the difference needs are in the call and one frame number apart.  frame_ids: the meshes' frame numbers, int64 [F] on the
    device of verts, strictly increasing (None: consecutive); they are read on the device.  scale c (None: rho(s) = s): rho(s) =
    2 c^2 (sqrt(1 + s / c^2) - 1), quadratic below c and linear above it, in the length units of verts.  vertex_weights: float32 [V] on
    the device of verts, finite and >= 0 (None: 1).  Fewer than order + 1 meshes, or no valid stencil: value and gradient exactly 0.
    The modes and `acc` are stretch_penalty's.  validate: check frame_ids and vertex_weights on the host (two read-backs; skipped while
    a stream is capturing)."""
    order = _check_motion_order(order)
    inv_c = motion_inv_scale(scale)
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.dtype != torch.float32:
        raise ValueError(f"motion_penalty: verts must be float32 [F,V,3] (got {verts.dtype} {tuple(verts.shape)})")
    F, V = int(verts.shape[0]), int(verts.shape[1])
    if F < 1 or V < 1:
        raise ValueError(f"motion_penalty: verts must hold at least one mesh and one vertex (got {tuple(verts.shape)})")
    live = validate and not (verts.is_cuda and torch.cuda.is_current_stream_capturing())
    if frame_ids is not None:
        if not torch.is_tensor(frame_ids) or frame_ids.dtype != torch.int64 or tuple(frame_ids.shape) != (F,):
            raise ValueError(f"motion_penalty: frame_ids must be an int64 tensor [{F}], one frame number per mesh")
        if frame_ids.device != verts.device:
            raise ValueError(f"motion_penalty: frame_ids must be on the device of verts ({verts.device}), they are read there")
        if live and F > 1 and not bool((frame_ids[1:] > frame_ids[:-1]).all()):
            raise ValueError("motion_penalty: frame_ids must be strictly increasing")
        frame_ids = frame_ids.contiguous()
    if vertex_weights is not None:
        if (not torch.is_tensor(vertex_weights) or vertex_weights.dtype != torch.float32 or tuple(vertex_weights.shape) != (V,)
                or vertex_weights.device != verts.device):
            raise ValueError(f"motion_penalty: vertex_weights must be a float32 tensor [{V}] on the device of verts")
        if live and not bool((torch.isfinite(vertex_weights) & (vertex_weights >= 0)).all()):
            raise ValueError("motion_penalty: vertex_weights must be finite and not negative")
        vertex_weights = vertex_weights.contiguous()
    return _motion_penalty.apply(verts, frame_ids, vertex_weights, inv_c, order, weight, bool(eager_grad and unit_upstream), acc)


def mesh_normal_consistency(verts, topo):
    """pytorch3d.loss.mesh_normal_consistency restated (reference fit.py:582; weight 0 in main.py:40): for every edge
    shared by exactly two faces, 1 - cos of the angle between the two face normals (oriented by the faces' own vertex
    order, as pytorch3d does through the edge's two opposite vertices); mean over those edges and over the batch.
    verts [F,V,3]."""
    f0, f1 = topo.edge_faces
    if f0.numel() == 0:
        return verts.sum() * 0.0
    tri = topo.faces

    def normals(fid):
        a, b, c = verts[:, tri[fid, 0]], verts[:, tri[fid, 1]], verts[:, tri[fid, 2]]
        return torch.cross(b - a, c - a, dim=-1)

    n0, n1 = normals(f0), normals(f1)
    cos = torch.nn.functional.cosine_similarity(n0, n1, dim=-1, eps=1e-8)
    return (1.0 - cos).mean()


def mesh_edge_loss(verts, topo, target_length=0.0):
    """mean over edges (and meshes) of (|e| - target)^2."""
    d = verts[:, topo.edges[:, 0]] - verts[:, topo.edges[:, 1]]
    return ((d.norm(dim=2) - target_length) ** 2).mean()


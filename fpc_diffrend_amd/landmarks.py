"""
The landmark term ("Landmark rule"): named points of the mesh held to their detected 2D positions in the captures -- the
tables of a set of landmarks (LandmarkSet), the penalty whose device code is csrc/landmark.hip (landmark_penalty), the two closed-form
starts from the landmarks, every frame's rigid pose (solve_pose, csrc/landmark_pose.hip) and blend weights (solve_expression,
csrc/landmark_expr.hip), the float64 projection of a synthetic Scene's own landmarks (project_landmarks) and the landmark file of a take (read_landmarks / write_landmarks).
The reference has no such term.  fit.py imports these names: fit.LandmarkSet, fit.landmark_penalty, ... are the documented spelling.
"""
import json

import numpy as np
import torch

from . import _lib, camera
from .mesh_reg import _check_item_weights, _inv_scale, _penalty
from .ops import _ptr, _stream


def landmark_tables(points, n_vertices, faces):
    """The tables of the Landmark rule from a list of points, numpy: (lm_vtx [3,L] int32, lm_bary [3,L] float32, lm_w [L] float32,
    names [L]).  A point is {'vertex': i} -- stored as (i, i, i) with weights (1, 0, 0) -- or {'face': t, 'bary': (b0, b1, b2)} -- the
    face's three vertices with the weights formed in float64 and rounded once --, with optional 'name' (default: its index as text) and
    'weight' (default 1).  ValueError for an id out of range, a weight or barycentric that is not finite, a negative weight."""
    if points is None or len(points) == 0:
        raise ValueError("a landmark set needs at least one point")
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    L = len(points)
    vtx, bary, w, names = np.zeros((3, L), np.int64), np.zeros((3, L), np.float64), np.ones(L, np.float64), []
    for l, p in enumerate(points):
        if not isinstance(p, dict) or ('vertex' in p) == ('face' in p):
            raise ValueError(f"landmark {l}: a point is {{'vertex': i}} or {{'face': t, 'bary': (b0, b1, b2)}} (got {p!r})")
        if 'vertex' in p:
            i = p['vertex']
            if isinstance(i, bool) or int(i) != i or not 0 <= int(i) < n_vertices:
                raise ValueError(f"landmark {l}: vertex {i!r} is out of range (the mesh has {n_vertices} vertices)")
            vtx[:, l], bary[:, l] = int(i), (1.0, 0.0, 0.0)
        else:
            t = p['face']
            if isinstance(t, bool) or int(t) != t or not 0 <= int(t) < f.shape[0]:
                raise ValueError(f"landmark {l}: face {t!r} is out of range (the mesh has {f.shape[0]} faces)")
            b = np.asarray(p.get('bary', ()), dtype=np.float64).reshape(-1)
            if b.shape != (3,) or not np.isfinite(b).all():
                raise ValueError(f"landmark {l}: 'bary' must be three finite numbers (got {p.get('bary')!r})")
            if not (0 <= f[int(t)]).all() or not (f[int(t)] < n_vertices).all():
                raise ValueError(f"landmark {l}: face {t} names a vertex out of range")
            vtx[:, l], bary[:, l] = f[int(t)], b
        wl = float(p.get('weight', 1.0))
        if not np.isfinite(wl) or wl < 0.0:
            raise ValueError(f"landmark {l}: 'weight' must be finite and not negative (got {p.get('weight')!r})")
        w[l] = wl
        names.append(str(p.get('name', l)))
    return vtx.astype(np.int32), bary.astype(np.float32), w.astype(np.float32), names


def landmark_incidence(lm_vtx, lm_bary, n_vertices):
    """lm_inc [K,V] int32, slot-major: the landmark corners 3 l + k at every vertex, ascending; pads -1 trailing; K = the largest count
    over the vertices, at least 1 (built like mesh_reg.hinge_incidence).  A corner whose barycentric weight is 0 -- two of the three of a
    landmark at a vertex -- receives no gradient and has no slot."""
    vt, bw = np.asarray(lm_vtx, dtype=np.int64), np.asarray(lm_bary)
    corner = np.nonzero((bw != 0).T.reshape(-1))[0]             # 3 l + k, ascending
    at = vt.T.reshape(-1)[corner]                               # the vertex of that corner
    order = np.argsort(at, kind='stable')
    counts = np.bincount(at, minlength=n_vertices)
    K = max(int(counts.max()) if counts.size else 0, 1)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    sorted_at = at[order]
    inc = np.full((K, n_vertices), -1, dtype=np.int32)
    inc[np.arange(order.shape[0]) - starts[sorted_at], sorted_at] = corner[order]
    return inc


class LandmarkSet:
    """The mesh side of the Landmark rule, built once: .vtx [3,L] int32, .bary [3,L] float32, .w [L] float32, .inc [K,V] int32 on
    `device`, .names, .n (= L), .n_vertices, .K.  points: see landmark_tables."""

    def __init__(self, points, n_vertices, faces, device):
        vtx, bary, w, self.names = landmark_tables(points, int(n_vertices), faces)
        inc = landmark_incidence(vtx, bary, int(n_vertices))
        self.n, self.n_vertices, self.K = int(vtx.shape[1]), int(n_vertices), int(inc.shape[0])
        dev = torch.device(device)
        self.vtx, self.bary, self.w, self.inc = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (vtx, bary, w, inc))

    def with_weights(self, weights):
        """The same set with other per-landmark weights (float32 array-like [L], finite and >= 0): the tables are shared."""
        w = _check_item_weights(np.asarray(weights, dtype=np.float64), (self.n,), 'landmark_weights', 'landmark')
        other = object.__new__(LandmarkSet)
        other.__dict__.update(self.__dict__)
        other.w = torch.from_numpy(w).to(self.w.device)
        return other


def landmark_inv_scale(scale):
    """fpcdr_landmark_penalty's inv_c for a scale in pixels (mesh_reg._inv_scale: 0.0 for None, or ValueError)."""
    return _inv_scale(scale, "the landmark term's", refuse_bool=True)


def check_landmark_options(cfg):
    """What FitConfig's landmark fields ask (FitConfig.__post_init__), or ValueError.  Needs no GPU and no Scene."""
    w = cfg.weight_landmark
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not np.isfinite(w) or w < 0:
        raise ValueError(f"FitConfig.weight_landmark must be finite and not negative (got {w!r})")
    try:
        landmark_inv_scale(cfg.landmark_scale)
    except ValueError as e:
        raise ValueError(f"FitConfig.landmark_scale: {e}")
    n = cfg.landmark_iters
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"FitConfig.landmark_iters must be an integer >= 0 (got {n!r})")
    if not isinstance(cfg.use_landmarks, bool):
        raise ValueError(f"FitConfig.use_landmarks must be True or False (got {cfg.use_landmarks!r})")


class _landmark_penalty(_penalty):
    """weight / F * sum_f mean over the frame's images and landmarks of omega kappa rho(|residual|^2) with both gradients from ONE call
    (fpcdr_landmark_penalty): the pass over the landmarks leaves every point's gradient in a scratch and the matrices' gradients whole, a
    gather sums the points per vertex.  The gradients for a unit upstream are made in forward(); backward() hands them over."""

    @staticmethod
    def forward(ctx, verts, mvp, vtx, bary, w, inc, obs, inv_c, height, width, weight, unit=False, acc=None, scratch=None, residuals=None):
        x, acc, per, out = _penalty.begin(ctx, 15, "fpcdr_landmark_penalty", verts, acc, unit)
        m = mvp.contiguous()
        F, V, _ = x.shape
        Nc, L, K = m.shape[0] // F, vtx.shape[1], inc.shape[0]
        gx = gm = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx, gm = torch.empty_like(x), torch.empty_like(m)
            if scratch is None:      # the points' gradients, F * Nc * L * 3 floats (a caller that keeps one saves the allocation per step)
                scratch = torch.empty(F * Nc * L * 3, dtype=torch.float32, device=x.device)
            assert scratch.dtype == torch.float32 and scratch.numel() >= F * Nc * L * 3 and scratch.is_contiguous() and scratch.device == x.device
        _lib.call("fpcdr_landmark_penalty", _ptr(x), _ptr(m), _ptr(vtx), _ptr(bary), _ptr(w), _ptr(inc), _ptr(obs), float(inv_c), int(width),
                  int(height), _ptr(scratch) if gx is not None else None, _ptr(gx), _ptr(gm), _ptr(residuals), _ptr(acc), _ptr(per), _ptr(out),
                  float(weight), F, Nc, V, L, K, _stream())
        if gx is not None:
            ctx.save_for_backward(gx, gm)
        return out

    @staticmethod
    def backward(ctx, g):
        gx, gm = ctx.saved_tensors
        if not ctx.unit:
            g = g.to(torch.float32)
            gx, gm = gx * g, gm * g
        return (gx if ctx.needs_input_grad[0] else None, gm if ctx.needs_input_grad[1] else None) + (None,) * (ctx.n_inputs - 2)


def _check_entry_args(fn, lms, verts, own, obs, resolution, validate):
    """What landmark_penalty and solve_pose ask of the arguments they share, or ValueError in the name of `fn`: lms, verts, obs [n,L,3],
    resolution, the set's device and -- validate: one read-back, skipped while a stream is capturing -- the confidences.  own(F, device)
    -> n: the caller's checks of its own arguments, in their place between verts and obs; its matrices tell the image count n.
    -> (F, V, n, H, W)."""
    if not isinstance(lms, LandmarkSet):
        raise ValueError(f"{fn}: lms must be a LandmarkSet (got {type(lms).__name__})")
    if not torch.is_tensor(verts) or verts.dim() != 3 or verts.shape[2] != 3 or verts.dtype != torch.float32:
        raise ValueError(f"{fn}: verts must be float32 [F,V,3] (got {getattr(verts, 'dtype', None)} {tuple(getattr(verts, 'shape', ()))})")
    F, V = int(verts.shape[0]), int(verts.shape[1])
    if F < 1 or V != lms.n_vertices:
        raise ValueError(f"{fn}: verts must hold at least one mesh of the landmark set's {lms.n_vertices} vertices (got {tuple(verts.shape)})")
    n = own(F, verts.device)
    if not torch.is_tensor(obs) or obs.dtype != torch.float32 or tuple(obs.shape) != (n, lms.n, 3) or obs.device != verts.device:
        raise ValueError(f"{fn}: obs must be a float32 tensor [{n},{lms.n},3] on the device of verts")
    try:
        H, W = (int(v) for v in resolution)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: resolution must be (H, W) (got {resolution!r})")
    if H < 1 or W < 1:
        raise ValueError(f"{fn}: resolution must be (H, W), both positive (got {resolution!r})")
    if lms.vtx.device != verts.device:
        raise ValueError(f"{fn}: the landmark set must be on the device of verts ({verts.device})")
    if validate and not (verts.is_cuda and torch.cuda.is_current_stream_capturing()):
        k = obs[..., 2]
        if not bool((torch.isfinite(k) & (k >= 0)).all()):
            raise ValueError(f"{fn}: the confidences obs[..., 2] must be finite and not negative")
    return F, V, n, H, W


def landmark_penalty(verts, mvp, lms, obs, weight, resolution, scale=None, eager_grad=False, unit_upstream=False, acc=None, scratch=None,
                     residuals=None, validate=True):
    """weight / F * sum over the meshes of verts [F,V,3] of the mean over the frame's Nc images and the L landmarks of
    omega_l kappa rho(|(u, v) - (u*, v*)|^2) ("Landmark rule"): (u, v) the landmark's projection by mvp [F*Nc,4,4]
    (frame-major, as camera.transform_clip takes it) in raster pixels of a resolution = (H, W) capture -- pixel centres at integers, row
    0 at the bottom --, obs [F*Nc,L,3] float32 = (u*, v*, kappa >= 0) on the device of verts, lms a LandmarkSet there.  An entry counts
    when kappa > 0, omega_l > 0 and the point is in front of the camera (p.w > 1e-6).  scale c in pixels (None: rho(s) = s): rho(s) =
    2 c^2 (sqrt(1 + s / c^2) - 1), quadratic below c and linear above it, so one wrong detection does not outweigh the others.
    Differentiable in verts AND mvp; both gradients are made with the value (the modes and `acc` are stretch_penalty's: lazy and
    eager_grad differ in nothing but the name; with unit_upstream the caller guarantees d loss / d value = 1 and backward() hands the
    buffers over).  scratch: a float32 buffer of at least F * Nc * L * 3 elements (None: one is allocated per call).  residuals: a
    float32 tensor [F*Nc,L,2] that receives (u - u*, v - v*), NaN where the entry does not count.  validate: check obs on the host (one
    read-back; skipped while a stream is capturing)."""
    inv_c = landmark_inv_scale(scale)

    def own(F, dev):
        if (not torch.is_tensor(mvp) or mvp.dim() != 3 or tuple(mvp.shape[1:]) != (4, 4) or mvp.dtype != torch.float32 or mvp.shape[0] < F
                or mvp.shape[0] % F or mvp.device != dev):
            raise ValueError(f"landmark_penalty: mvp must be float32 [F*Nc,4,4] on the device of verts, frame-major (got {tuple(getattr(mvp, 'shape', ()))} "
                             f"for {F} meshes)")
        n = int(mvp.shape[0])
        if residuals is not None and (not torch.is_tensor(residuals) or residuals.dtype != torch.float32 or tuple(residuals.shape) != (n, lms.n, 2)
                                      or residuals.device != dev or not residuals.is_contiguous()):
            raise ValueError(f"landmark_penalty: residuals must be a contiguous float32 tensor [{n},{lms.n},2] on the device of verts")
        return n

    _, _, _, H, W = _check_entry_args("landmark_penalty", lms, verts, own, obs, resolution, validate)
    return _landmark_penalty.apply(verts, mvp, lms.vtx, lms.bary, lms.w, lms.inc, obs.contiguous(), inv_c, H, W, weight,
                                   bool(eager_grad and unit_upstream), acc, scratch, residuals)


def check_pose_options(cfg):
    """What FitConfig's init_pose / quat_renorm fields ask (FitConfig.__post_init__), or ValueError.  Needs no GPU and no Scene."""
    if cfg.init_pose not in ('keep', 'landmarks'):
        raise ValueError(f"FitConfig.init_pose must be 'keep' or 'landmarks' (got {cfg.init_pose!r})")
    if cfg.quat_renorm not in ('tensor', 'rows'):
        raise ValueError(f"FitConfig.quat_renorm must be 'tensor' or 'rows' (got {cfg.quat_renorm!r})")
    n = cfg.init_pose_iters
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"FitConfig.init_pose_iters must be an integer >= 0 (got {n!r})")
    if not isinstance(cfg.init_pose_rotation, bool):
        raise ValueError(f"FitConfig.init_pose_rotation must be True or False (got {cfg.init_pose_rotation!r})")


def solve_pose(verts, proj, base, lms, obs, q, t, resolution, scale=None, iters=20, rotation=True, damping=1e-3, normal_out=None):
    """Every frame's rigid pose (q [F,4] XYZW, t [F,3], float32, written IN PLACE) solved from its landmarks by damped Gauss-Newton on the
    Landmark rule's cost, one launch for all frames ("Pose solve rule"; fpcdr_landmark_pose): the chain is
    proj[c] . Rt(q_f / |q_f|, t_f) . base[c] on the meshes verts [F,V,3], proj and base [Nc,4,4] float32 (base = Rt(q_c, t_c) . MV_c .
    T(0,170,0)), lms a LandmarkSet, obs [F*Nc,L,3] = (u*, v*, kappa) in raster pixels of a resolution = (H, W) capture, scale the
    Charbonnier scale in pixels (None: L2).  iters trials from the damping `damping`; a trial is kept when it has at least as many live
    entries and a smaller cost.  rotation=False: the translation alone, q is not written.  A frame with fewer than 3 live entries stays
    bit for bit as it was.  normal_out: a contiguous float32 tensor [F,28] that receives A's upper triangle (21), b (6) and the cost at
    the INPUT pose (iters=0: nothing else happens).  -> info [F,4] float32 = (cost at the input pose, cost at the returned pose, live
    entries at the returned pose, accepted trials).  ValueError names what does not fit."""
    inv_c = landmark_inv_scale(scale)

    def own(F, dev):
        for name, m in (('proj', proj), ('base', base)):
            if not torch.is_tensor(m) or m.dim() != 3 or tuple(m.shape[1:]) != (4, 4) or m.dtype != torch.float32 or m.shape[0] < 1 or m.device != dev:
                raise ValueError(f"solve_pose: {name} must be float32 [Nc,4,4] on the device of verts (got {tuple(getattr(m, 'shape', ()))})")
        if int(base.shape[0]) != int(proj.shape[0]):
            raise ValueError(f"solve_pose: proj and base must hold the same cameras (got {int(proj.shape[0])} and {int(base.shape[0])})")
        for name, p, k in (('q', q, 4), ('t', t, 3)):
            if not torch.is_tensor(p) or p.dtype != torch.float32 or tuple(p.shape) != (F, k) or p.device != dev or not p.is_contiguous():
                raise ValueError(f"solve_pose: {name} must be a contiguous float32 tensor [{F},{k}] on the device of verts "
                                 f"(got {tuple(getattr(p, 'shape', ()))})")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise ValueError(f"solve_pose: iters must be an integer >= 0 (got {iters!r})")
        if isinstance(damping, bool) or not isinstance(damping, (int, float)) or not np.isfinite(damping) or not damping > 0:
            raise ValueError(f"solve_pose: damping must be finite and positive (got {damping!r})")
        if normal_out is not None and (not torch.is_tensor(normal_out) or normal_out.dtype != torch.float32 or tuple(normal_out.shape) != (F, 28)
                                       or normal_out.device != dev or not normal_out.is_contiguous()):
            raise ValueError(f"solve_pose: normal_out must be a contiguous float32 tensor [{F},28] on the device of verts")
        return F * int(proj.shape[0])

    F, V, n, H, W = _check_entry_args("solve_pose", lms, verts, own, obs, resolution, True)
    Nc, dev = n // F, verts.device
    if not (verts.is_cuda and torch.cuda.is_current_stream_capturing()):
        qn = q.detach().double().norm(dim=1)
        if not bool((torch.isfinite(qn) & (qn > 0)).all()):
            bad = int(torch.nonzero(~(torch.isfinite(qn) & (qn > 0)))[0])
            raise ValueError(f"solve_pose: the norm of q[{bad}] must be finite and positive (got {q[bad].tolist()})")
    info = torch.empty(F, 4, dtype=torch.float32, device=dev)
    x, pj, bs, ob = verts.detach().contiguous(), proj.detach().contiguous(), base.detach().contiguous(), obs.contiguous()
    _lib.call("fpcdr_landmark_pose", _ptr(x), _ptr(pj), _ptr(bs), _ptr(lms.vtx), _ptr(lms.bary), _ptr(lms.w), _ptr(ob), _ptr(q.detach()),
              _ptr(t.detach()), float(inv_c), W, H, int(iters), 1 if rotation else 0, float(damping), _ptr(info), _ptr(normal_out), F, Nc, V,
              lms.n, _stream())
    return info


EXPR_MAX_KB, EXPR_MAX_L = 160, 512      # what fpcdr_landmark_expr accepts (csrc/landmark_expr.hip)


def check_expression_options(cfg):
    """What FitConfig's init_expression / init_landmark_rounds fields ask (FitConfig.__post_init__), or ValueError.  Needs no GPU and no
    Scene."""
    if cfg.init_expression not in ('keep', 'landmarks'):
        raise ValueError(f"FitConfig.init_expression must be 'keep' or 'landmarks' (got {cfg.init_expression!r})")
    n = cfg.init_expression_iters
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"FitConfig.init_expression_iters must be an integer >= 0 (got {n!r})")
    r = cfg.init_expression_ridge
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not np.isfinite(r) or r < 0:
        raise ValueError(f"FitConfig.init_expression_ridge must be finite and not negative (got {r!r})")
    k = cfg.init_landmark_rounds
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"FitConfig.init_landmark_rounds must be an integer >= 1 (got {k!r})")
    if cfg.init_expression == 'landmarks' and cfg.mode == 'free':
        raise ValueError("FitConfig.init_expression='landmarks' needs mode='prior' or 'combined': mode='free' has no rig weights to solve")


def solve_expression(verts, mvp, basis, lms, obs, w, resolution, scale=None, ridge=0.0, iters=20, damping=1e-3, normal_out=None):
    """Every frame's blend weights (w [F,Kb] float32, written IN PLACE) solved from its landmarks by damped Gauss-Newton on the Landmark
    rule's cost plus a ridge, one launch for all frames and trials ("Expression solve rule"; fpcdr_landmark_expr): verts
    [F,V,3] are the meshes AT the weights w, mvp [F*Nc,4,4] the matrices as landmark_penalty takes them (the pose is fixed), basis
    [3V,Kb] float32 the blend basis (datasets['local']), lms a LandmarkSet, obs [F*Nc,L,3] = (u*, v*, kappa) in raster pixels of a
    resolution = (H, W) capture, scale the Charbonnier scale in pixels (None: L2).  The point of landmark l at the weights w' is its
    point on verts plus A_l (w' - w), A the basis at the landmark's corners.  ridge >= 0, in px^2 per unit weight^2 on the Landmark
    rule's per-entry scale, pulls towards neutral (the cost gains ridge * Nc * L * sum_k w_k^2).  iters trials from the damping
    `damping`; a trial is kept when it has at least as many live entries and a smaller cost.  A frame with fewer than 3 live entries,
    and a weight that no live landmark touches (without a ridge), stay bit for bit as they were.  Kb <= 160 and L <= 512.
    normal_out: a contiguous float64 tensor [F, Kb (Kb + 1) / 2 + Kb + 2] that receives the packed lower triangle of H, g, E and the
    live count at the INPUT weights (iters=0: nothing else happens).  -> info [F,4] float32 = (cost at the input weights, cost at the
    returned weights, live entries there, accepted trials).  ValueError names what does not fit."""
    inv_c = landmark_inv_scale(scale)

    def own(F, dev):
        if (not torch.is_tensor(mvp) or mvp.dim() != 3 or tuple(mvp.shape[1:]) != (4, 4) or mvp.dtype != torch.float32 or mvp.shape[0] < F
                or mvp.shape[0] % F or mvp.device != dev):
            raise ValueError(f"solve_expression: mvp must be float32 [F*Nc,4,4] on the device of verts, frame-major (got "
                             f"{tuple(getattr(mvp, 'shape', ()))} for {F} meshes)")
        V = int(verts.shape[1])
        if (not torch.is_tensor(basis) or basis.dim() != 2 or basis.shape[0] != 3 * V or basis.shape[1] < 1 or basis.dtype != torch.float32
                or basis.device != dev):
            raise ValueError(f"solve_expression: basis must be float32 [{3 * V},Kb] on the device of verts (got {tuple(getattr(basis, 'shape', ()))})")
        Kb = int(basis.shape[1])
        if Kb > EXPR_MAX_KB or lms.n > EXPR_MAX_L:
            raise ValueError(f"solve_expression: at most {EXPR_MAX_KB} blend weights and {EXPR_MAX_L} landmarks (got {Kb} and {lms.n})")
        if not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != (F, Kb) or w.device != dev or not w.is_contiguous():
            raise ValueError(f"solve_expression: w must be a contiguous float32 tensor [{F},{Kb}] on the device of verts "
                             f"(got {tuple(getattr(w, 'shape', ()))})")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise ValueError(f"solve_expression: iters must be an integer >= 0 (got {iters!r})")
        if isinstance(damping, bool) or not isinstance(damping, (int, float)) or not np.isfinite(damping) or not damping > 0:
            raise ValueError(f"solve_expression: damping must be finite and positive (got {damping!r})")
        if isinstance(ridge, bool) or not isinstance(ridge, (int, float)) or not np.isfinite(ridge) or ridge < 0:
            raise ValueError(f"solve_expression: ridge must be finite and not negative (got {ridge!r})")
        n_out = Kb * (Kb + 1) // 2 + Kb + 2
        if normal_out is not None and (not torch.is_tensor(normal_out) or normal_out.dtype != torch.float64 or tuple(normal_out.shape) != (F, n_out)
                                       or normal_out.device != dev or not normal_out.is_contiguous()):
            raise ValueError(f"solve_expression: normal_out must be a contiguous float64 tensor [{F},{n_out}] on the device of verts")
        return int(mvp.shape[0])

    F, V, n, H, W = _check_entry_args("solve_expression", lms, verts, own, obs, resolution, True)
    Nc, Kb, dev = n // F, int(basis.shape[1]), verts.device
    info = torch.empty(F, 4, dtype=torch.float32, device=dev)
    nbytes = int(_lib.load().fpcdr_landmark_expr_scratch_bytes(F, lms.n, Kb))
    scratch = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    x, m, b, ob = verts.detach().contiguous(), mvp.detach().contiguous(), basis.detach().contiguous(), obs.contiguous()
    _lib.call("fpcdr_landmark_expr", _ptr(x), _ptr(m), _ptr(b), _ptr(lms.vtx), _ptr(lms.bary), _ptr(lms.w), _ptr(ob), _ptr(w.detach()),
              float(inv_c), float(ridge), W, H, int(iters), float(damping), _ptr(info), _ptr(normal_out), _ptr(scratch), nbytes, F, Nc, V,
              lms.n, Kb, _stream())
    return info


def project_landmarks(sc, lms_points, cam_idxs=None):
    """The landmarks of a synthetic Scene at its hidden ground truth, float64 numpy through camera.py's own chain (fit.py:541-553 of the
    reference: P . Rt(q_f, t_f) . MV_c . T(0, 170, 0)): [F,Ncam,L,3] = (u, v, kappa) in raster pixels of sc.resolution, kappa = 1 (0 for a
    point that is not in front of its camera).  No occlusion reasoning: a landmark on the far side of the head projects like any other.
    cam_idxs: the cameras, in this order (None: every camera of the Scene).  For synthetic scenes and for the tests."""
    if sc.weights_gt is None:
        raise ValueError("project_landmarks needs a synthetic Scene (its hidden ground truth)")
    vtx, bary, _, _ = landmark_tables(lms_points, sc.n_vertices, sc.pos_idx)
    H, W = sc.resolution
    cams = list(range(len(sc.cams))) if cam_idxs is None else list(cam_idxs)
    F = sc.n_frames
    verts = (sc.v_base.astype(np.float64)[None] + sc.weights_gt.astype(np.float64) @ sc.blendshapes.astype(np.float64).T).reshape(F, -1, 3)
    b = bary.astype(np.float64)
    q = sum(b[k][None, :, None] * verts[:, vtx[k]] for k in range(3))               # [F,L,3]
    qw = np.concatenate([q, np.ones(q.shape[:2] + (1,))], axis=2)
    T = camera.translate(0.0, 170.0, 0.0).astype(np.float64)
    out = np.zeros((F, len(cams), vtx.shape[1], 3), dtype=np.float64)
    for f in range(F):
        Rt = np.eye(4)
        Rt[:3, :3] = camera.unitquat_to_rotmat(torch.tensor(sc.q_gt[f], dtype=torch.float64)).numpy()
        Rt[:3, 3] = sc.t_gt[f]
        for j, c in enumerate(cams):
            cam = sc.cams[c]
            P = camera.intrinsic_to_projection(cam['intr']).astype(np.float64)
            MV = camera.extrinsic_to_modelview(cam['rot'], cam['trans_calib']).astype(np.float64)
            p = qw[f] @ (P @ (Rt @ (MV @ T))).T
            front = p[:, 3] > 1e-6
            pw = np.where(front, p[:, 3], 1.0)
            out[f, j, :, 0] = (p[:, 0] / pw * 0.5 + 0.5) * W - 0.5
            out[f, j, :, 1] = (p[:, 1] / pw * 0.5 + 0.5) * H - 0.5
            out[f, j, :, 2] = front
    return out


def write_landmarks(path, points, landmarks, cam_names, height):
    """The landmark file of a take: {"points": [...], "observations": {camera name: [[[x, y, conf] x L] x F]}} with x, y in pixels of the
    images as they lie on disk -- x right, y DOWN, the top-left pixel's centre at (0, 0) --, from landmarks [F,Nc,L,3] in raster
    coordinates (row 0 at the bottom: y = height - 1 - v, formed in float64).  An entry of confidence 0 is written as null."""
    lm = np.asarray(landmarks, dtype=np.float32)
    if lm.ndim != 4 or lm.shape[1] != len(cam_names) or lm.shape[2] != len(points) or lm.shape[3] != 3:
        raise ValueError(f"landmarks must be [F,{len(cam_names)},{len(points)},3] (got {lm.shape})")
    obs = {}
    for j, name in enumerate(cam_names):      # (the flip in float64: exact, so that reading gives the float32 back)
        obs[str(name)] = [[None if not e[2] > 0 else [float(e[0]), float(height - 1) - float(e[1]), float(e[2])] for e in frame]
                          for frame in lm[:, j]]
    with open(path, "w") as f:
        json.dump({"points": [dict(p) for p in points], "observations": obs}, f)
    return path


def read_landmarks(path, cam_names, n_frames, height):
    """The landmark file of a take (write_landmarks) -> (points, landmarks [F,Nc,L,3] float32 in raster coordinates: v = height - 1 - y).
    cam_names: the take's cameras in order; each is looked up under its own name, then under the second '_' field of it (the
    calibration's key).  A null entry, or a camera the file does not hold, gives kappa = 0.  ValueError names what does not fit."""
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"{path}: cannot read the landmark file: {e}")
    if not isinstance(doc, dict) or not isinstance(doc.get("points"), list) or not isinstance(doc.get("observations"), dict):
        raise ValueError(f"{path}: a landmark file holds {{\"points\": [...], \"observations\": {{camera: ...}}}}")
    points, obs = doc["points"], doc["observations"]
    L = len(points)
    out = np.zeros((n_frames, len(cam_names), L, 3), dtype=np.float32)
    for j, name in enumerate(cam_names):
        parts = str(name).split("_")
        rows = obs.get(str(name), obs.get(parts[1]) if len(parts) > 1 else None)
        if rows is None:
            continue
        if len(rows) != n_frames:
            raise ValueError(f"{path}: camera {name} holds {len(rows)} frames, the take has {n_frames}")
        for fr, row in enumerate(rows):
            if row is None:
                continue
            if len(row) != L:
                raise ValueError(f"{path}: camera {name}, frame {fr} holds {len(row)} landmarks, 'points' has {L}")
            for l, e in enumerate(row):
                if e is None:
                    continue
                if len(e) != 3 or not all(isinstance(v, (int, float)) and np.isfinite(v) for v in e) or e[2] < 0:
                    raise ValueError(f"{path}: camera {name}, frame {fr}, landmark {l}: an entry is [x, y, conf >= 0] or null (got {e!r})")
                out[fr, j, l] = (e[0], float(height - 1) - float(e[1]), e[2])      # (the flip in float64, rounded once)
    return points, out

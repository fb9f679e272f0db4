"""float64 restatements on the CPU of the small kernels of a fit step (csrc/blend.hip, clip.hip, mesh_reg.hip, loss.hip): the yardstick of
tests/test_gpu_fitstep.py, itself checked on the CPU by tests/test_fitstep_ref.py.  Nothing here imports fpc_diffrend_amd.

Every function takes tensors of any float dtype and evaluates in `dtype` (float64 by default; float32 gives "the same formula in
float32 by torch", the yardstick of the long sums).  Besides each value it returns a scale S: the same formula with every input
replaced by its absolute value and every subtraction by an addition -- the sum of the absolute values of the terms of that entry.
An error is measured per entry in units of u = 2^-24 against S (measure()): a lost or doubled term of an entry shows at its own
size, however many other entries the tensor has.

The module also builds the inputs both test files share (meshes, camera-like matrices), so that the CPU file measures the float32
evaluation on the very inputs the GPU file hands to the kernels."""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of float32

# Rounded operations that reach one entry, n: the entry's error is then at most (n + 2) u of its scale S, for any order of summation, with
# or without fused multiply-add.  Rules: an input has n = 0; a product has n_a + n_b + 1; a sum of k terms has max n_i + (k - 1);
# a product with 2 or 4 is exact.
# MVP value: an entry of rigid(): 2 x exact, txx and tyy 1, their sum 2, 1 - sum 3.  B = rigid . MV: products 3 + 0 + 1 = 4, three adds: 7.
#            X = rigid . B: products 3 + 7 + 1 = 11, three adds: 14.  M = P . X: products 15, three adds: 18.
MVP_N_VALUE = 18
# MVP gradients: gX = P^T g: 1 + 3 = 4.  gA = gX B^T: products 4 + 7 + 1 = 12, three adds: 15; gC = (A^T gX) MV^T: A^T gX 3 + 4 + 1 + 3 = 11,
#            then 12 + 3 = 15 as well.  rigid_bwd: a sum of two entries 16, its product with a quaternion entry 17, the sum of three such 19
#            (times 2: exact), the 4 x (g + g) term 17, the subtraction: 20.  The translation's gradient is an entry of gA / gC itself (15).
#            One more add for every (frame, view) pair that sums into the row: added by the tests.
MVP_N_GRAD = 20
# L^T y: c_f = upstream * weight * 2 * per_f / (F V): three products and a quotient, 4.  ||lap||: squares 1, two adds 3, the root 4.
#            c_f / ||lap||: 4 + 4 + 1 = 9, its product with lap 10.  The float32 1 / degree of the neighbour (1) times y: 12.  Then degree - 1
#            adds and the subtraction of y_v: 12 + degree; the degree is added by the tests.
LAP_N_GRAD = 12
# value of the penalty from per_f: per_f rounded to float32 and squared (2), the sum in float64, the rounding of the result: 3
LAP_N_VALUE = 3
# d mean / d colour: 1 / n_total rounded to float32 (1), its product with -2 * 255 (2); 255 * colour (1), ref - that (2); their product: 5
PIXEL_N_GRAD = 5


def measure(x, r, S):
    """max_i |x_i - r_i| / S_i over the entries with S_i > 0, in units of u, and the number of entries with S_i = 0; those must
    be exactly 0 in x (asserted here).  A NaN or Inf in x gives nan / inf, which no bound admits."""
    x, r, S = (t.detach().to('cpu', torch.float64) for t in (x, r, S))
    assert x.shape == r.shape == S.shape, (x.shape, r.shape, S.shape)
    z = S == 0
    assert bool((x[z] == 0).all()), "an entry without any term is not exactly 0"
    if bool(z.all()):
        return 0.0, int(z.sum())
    q = (x - r).abs()[~z] / S[~z]
    e = float('nan') if bool(torch.isnan(q).any()) else float(q.max())
    return e / U, int(z.sum())


def rel_l2(x, r):
    x, r = x.detach().to('cpu', torch.float64), r.detach().to('cpu', torch.float64)
    return float((x - r).norm() / max(float(r.norm()), 1e-300))


def _c(t, dtype):
    return t.detach().to('cpu', dtype)


# ---------------------------------------------------------------------------------------------------------------------
# blend, rig weights
# ---------------------------------------------------------------------------------------------------------------------

def blend(v_base, Bmat, w, go=None, dtype=torch.float64):
    """out = v_base + w @ Bmat.T ([F,M]; v_base None = 0) and, with go = d loss / d out, the gradients for v_base, Bmat, w.
    -> dict name -> (value, S)."""
    Bm, ww = _c(Bmat, dtype), _c(w, dtype)
    vb = _c(v_base, dtype) if v_base is not None else torch.zeros(Bm.shape[0], dtype=dtype)
    res = {'out': (vb[None] + ww @ Bm.t(), vb.abs()[None] + ww.abs() @ Bm.abs().t())}
    if go is not None:
        g = _c(go, dtype)
        res['g_vb'] = (g.sum(0), g.abs().sum(0))
        res['g_B'] = (g.t() @ ww, g.abs().t() @ ww.abs())
        res['g_w'] = (g @ Bm, g.abs() @ Bm.abs())
    return res


def rig_columns(ids, Fc):
    """The columns maps[:, ids] takes: a slice or an index tensor, negative entries from the end."""
    if isinstance(ids, slice):
        return torch.arange(*ids.indices(Fc))
    c = ids.detach().cpu().to(torch.int64)
    return torch.where(c < 0, c + Fc, c)


def rig_weights(mi, maps, ids, go=None, dtype=torch.float64):
    """w = (mi @ maps[:, ids]).T ([Fb,K]) and the gradients for mi and maps (columns no index names get 0)."""
    a, m = _c(mi, dtype), _c(maps, dtype)
    cols = rig_columns(ids, m.shape[1])
    sel = m[:, cols]
    res = {'w': ((a @ sel).t(), (a.abs() @ sel.abs()).t())}
    if go is not None:
        g = _c(go, dtype)                                            # [Fb,K]
        res['g_mi'] = (g.t() @ sel.t(), g.abs().t() @ sel.abs().t())
        gs, gs_abs = a.t() @ g.t(), a.abs().t() @ g.abs().t()        # [Fr,Fb]: d / d maps[:, cols]
        res['g_maps'] = (torch.zeros_like(m).index_add_(1, cols, gs), torch.zeros_like(m).index_add_(1, cols, gs_abs))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# MVP chain: mvp[f,c] = P_c . Rt(q_f, t_f) . (Rt(q_c, t_c) . MV_c), quaternions XYZW, not normalised
# ---------------------------------------------------------------------------------------------------------------------

def rigid(q, t, scale=False):
    """[R(q) | t; 0 0 0 1] for q [...,4], t [...,3].  scale=True: q, t are absolute values and every subtraction adds."""
    s = 1.0 if scale else -1.0
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    rows = [one + s * (tyy + tzz), txy + s * twz, txz + twy, t[..., 0],
            txy + twz, one + s * (txx + tzz), tyz + s * twx, t[..., 1],
            txz + s * twy, tyz + twx, one + s * (txx + tyy), t[..., 2],
            zero, zero, zero, one]
    return torch.stack(rows, dim=-1).reshape(q.shape[:-1] + (4, 4))


def rigid_bwd(q, G, scale=False):
    """d loss / d (q, t) from G = d loss / d rigid(q, t) [...,4,4], written out by hand."""
    s = 1.0 if scale else -1.0
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    g = lambda i, j: G[..., i, j]
    gx = 2.0 * (y * (g(0, 1) + g(1, 0)) + z * (g(0, 2) + g(2, 0)) + w * (g(2, 1) + s * g(1, 2))) + s * 4.0 * x * (g(1, 1) + g(2, 2))
    gy = 2.0 * (x * (g(0, 1) + g(1, 0)) + z * (g(1, 2) + g(2, 1)) + w * (g(0, 2) + s * g(2, 0))) + s * 4.0 * y * (g(0, 0) + g(2, 2))
    gz = 2.0 * (x * (g(0, 2) + g(2, 0)) + y * (g(1, 2) + g(2, 1)) + w * (g(1, 0) + s * g(0, 1))) + s * 4.0 * z * (g(0, 0) + g(1, 1))
    gw = 2.0 * (z * (g(1, 0) + s * g(0, 1)) + y * (g(0, 2) + s * g(2, 0)) + x * (g(2, 1) + s * g(1, 2)))
    return torch.stack([gx, gy, gz, gw], dim=-1), G[..., :3, 3]


def mvp_chain(q_cam, t_cam, q_frame, t_frame, proj, t_mv, go=None, frame_idx=None, view_idx=None, cam_of_view=None, Fb=None, Nc=None,
              dtype=torch.float64):
    """The matrices [Fb*Nc,4,4] and, with go, the gradients for the FULL tables q_cam, t_cam, q_frame, t_frame.  frame_idx [Fb] / None
    (frames 0 .. Fb-1), view_idx [Nc] / None: rows of proj and t_mv, cam_of_view [views] / None: row of q_cam / t_cam of a view.
    Two entries that name one row add into it; a row no entry names gets 0."""
    qc, tc, qf, tf, P, MV = (_c(t, dtype) for t in (q_cam, t_cam, q_frame, t_frame, proj, t_mv))
    Fb = int(Fb if Fb is not None else (len(frame_idx) if frame_idx is not None else qf.shape[0]))
    Nc = int(Nc if Nc is not None else (len(view_idx) if view_idx is not None else P.shape[0]))
    fr = frame_idx.cpu().long() if frame_idx is not None else torch.arange(Fb)
    cv = view_idx.cpu().long() if view_idx is not None else torch.arange(Nc)
    cp = cam_of_view.cpu().long()[cv] if cam_of_view is not None else cv
    res = {}
    both = []
    for scale in (False, True):
        f = (lambda t: t.abs()) if scale else (lambda t: t)
        A = rigid(f(qf[fr]), f(tf[fr]), scale)                        # [Fb,4,4]
        B = rigid(f(qc[cp]), f(tc[cp]), scale) @ f(MV[cv])             # [Nc,4,4]
        X = A[:, None] @ B[None]                                       # [Fb,Nc,4,4]
        M = f(P[cv])[None] @ X
        out = [M.reshape(Fb * Nc, 4, 4)]
        if go is not None:
            g = f(_c(go, dtype)).reshape(Fb, Nc, 4, 4)
            gX = f(P[cv]).transpose(1, 2)[None] @ g                    # P^T dL/dM
            gA = (gX @ B.transpose(1, 2)[None]).sum(1)                 # dL/dX B^T, summed over the views of a frame
            gC = ((A.transpose(1, 2)[:, None] @ gX) @ f(MV[cv]).transpose(1, 2)[None]).sum(0)
            gqf, gtf = rigid_bwd(f(qf[fr]), gA, scale)
            gqc, gtc = rigid_bwd(f(qc[cp]), gC, scale)
            out += [torch.zeros_like(qc).index_add_(0, cp, gqc), torch.zeros_like(tc).index_add_(0, cp, gtc),
                    torch.zeros_like(qf).index_add_(0, fr, gqf), torch.zeros_like(tf).index_add_(0, fr, gtf)]
        both.append(out)
    for name, v, s in zip(('mvp', 'g_q_cam', 'g_t_cam', 'g_q_frame', 'g_t_frame'), *both):
        res[name] = (v, s)
    return res


def mvp_chain_plain(q_cam, t_cam, q_frame, t_frame, proj, t_mv, frame_idx=None, view_idx=None, cam_of_view=None):
    """The same value as a plain differentiable torch expression (for torch.autograd, in the dtype of its inputs)."""
    Fb = len(frame_idx) if frame_idx is not None else q_frame.shape[0]
    Nc = len(view_idx) if view_idx is not None else proj.shape[0]
    fr = frame_idx.long() if frame_idx is not None else torch.arange(Fb)
    cv = view_idx.long() if view_idx is not None else torch.arange(Nc)
    cp = cam_of_view.long()[cv] if cam_of_view is not None else cv
    A = rigid(q_frame[fr], t_frame[fr])
    B = rigid(q_cam[cp], t_cam[cp]) @ t_mv[cv]
    return (proj[cv][None] @ (A[:, None] @ B[None])).reshape(Fb * Nc, 4, 4)


# ---------------------------------------------------------------------------------------------------------------------
# clip transform
# ---------------------------------------------------------------------------------------------------------------------

def clip_transform(mvp, verts, go=None, dtype=torch.float64):
    """out[f * Nc + c, v] = mvp[f * Nc + c] @ (verts[f, v], 1) and both gradients."""
    m, x = _c(mvp, dtype), _c(verts, dtype)
    F, V = x.shape[0], x.shape[1]
    Nc = m.shape[0] // F
    m = m.reshape(F, Nc, 4, 4)
    pw = torch.cat([x, torch.ones(F, V, 1, dtype=dtype)], dim=-1)
    ev = lambda mm, pp: torch.einsum('fcij,fvj->fcvi', mm, pp).reshape(F * Nc, V, 4)
    res = {'out': (ev(m, pw), ev(m.abs(), pw.abs()))}
    if go is not None:
        g = _c(go, dtype).reshape(F, Nc, V, 4)
        gv = lambda gg, mm: torch.einsum('fcvi,fcij->fvj', gg, mm[..., :3])
        gm = lambda gg, pp: torch.einsum('fcvi,fvj->fcij', gg, pp).reshape(F * Nc, 4, 4)
        res['g_verts'] = (gv(g, m), gv(g.abs(), m.abs()))
        res['g_mvp'] = (gm(g, pw), gm(g.abs(), pw.abs()))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# uniform Laplacian from the FACE LIST, and the penalty in its stages
# ---------------------------------------------------------------------------------------------------------------------

class FaceLaplacian:
    """L = D^-1 A - I (sparse float64) of a triangle list: edges from the faces, each once; a vertex without an edge has a row
    of D^-1 A that is 0.  |L| = D^-1 A + I is the scale's operator."""

    def __init__(self, faces, n_vertices):
        f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        V = int(n_vertices)
        pairs = set()
        for a, b, c in f.tolist():
            for p, q in ((a, b), (b, c), (c, a)):
                if p != q:
                    pairs.add((min(p, q), max(p, q)))
        e = np.asarray(sorted(pairs), dtype=np.int64).reshape(-1, 2)
        rows = np.concatenate([e[:, 0], e[:, 1]])
        cols = np.concatenate([e[:, 1], e[:, 0]])
        self.V = V
        self.deg = np.bincount(rows, minlength=V)
        wgt = 1.0 / self.deg[rows]
        idx = torch.tensor(np.stack([np.concatenate([rows, np.arange(V)]), np.concatenate([cols, np.arange(V)])]))
        for name, diag in (('L', -1.0), ('Labs', 1.0)):
            val = torch.tensor(np.concatenate([wgt, np.full(V, diag)]), dtype=torch.float64)
            setattr(self, name, torch.sparse_coo_tensor(idx, val, (V, V)).coalesce())

    def dense(self):
        return self.L.to_dense()

    def _mm(self, Lm, x, transpose, dtype):
        x = _c(x, dtype)
        F, V = x.shape[0], x.shape[1]
        Lm = Lm.to(dtype)
        flat = x.permute(1, 0, 2).reshape(V, F * 3)
        out = torch.sparse.mm(Lm.t() if transpose else Lm, flat)
        return out.reshape(V, F, 3).permute(1, 0, 2).contiguous()

    def apply(self, x, transpose=False, dtype=torch.float64):
        """L x (or L^T x) for x [F,V,3] -> (value, S)."""
        return self._mm(self.L, x, transpose, dtype), self._mm(self.Labs, _c(x, dtype).abs(), transpose, dtype)


def penalty_value(lap, weight, dtype=torch.float64):
    """per_f = mean_v ||lap_v|| and value = weight / F * sum_f per_f^2 from a given lap [F,V,3].  Every term is positive: the scales
    are the values themselves."""
    l = _c(lap, dtype)
    per = l.norm(dim=2).mean(dim=1)
    return per, (weight / l.shape[0]) * (per ** 2).sum()


def penalty_value_from_per(per, weight, dtype=torch.float64):
    p = _c(per, dtype)
    return (weight / p.shape[0]) * (p ** 2).sum()


def penalty_grad(lap, per, fl, weight, upstream=1.0, dtype=torch.float64):
    """d value / d x = L^T y, y_v = c_f lap_v / ||lap_v|| (0 where lap_v = 0), c_f = upstream * weight * 2 per_f / (F V), from a
    given lap [F,V,3] and per [F] -> (value, S)."""
    l, p = _c(lap, dtype), _c(per, dtype)
    F, V = l.shape[0], l.shape[1]
    c = float(upstream) * float(weight) * 2.0 * p / (F * V)
    nr = l.norm(dim=2, keepdim=True)
    y = torch.where(nr > 0, c[:, None, None] * l / torch.where(nr > 0, nr, torch.ones_like(nr)), torch.zeros_like(l))
    return fl._mm(fl.L, y, True, dtype), fl._mm(fl.Labs, y.abs(), True, dtype)


def penalty_plain(x, Ldense, weight):
    """The whole term as one differentiable torch expression (for torch.autograd)."""
    lap = torch.matmul(Ldense[None], x)
    per = lap.norm(dim=2).mean(dim=1)
    return (weight / x.shape[0]) * (per ** 2).sum()


# ---------------------------------------------------------------------------------------------------------------------
# pixel loss, background sum of squares, objective value
# ---------------------------------------------------------------------------------------------------------------------

BACKGROUND = 45.0 / 255.0


def pixel_loss(colour, coverage, ref_u8, n_total=None, background=BACKGROUND, dtype=torch.float64):
    """Composite with the background where coverage <= 0, sum (ref - 255 colour)^2 and d mean / d colour (mean over n_total
    elements, default all).  The background and 1 / n_total are the float32 numbers the kernel is handed.
    -> dict: 'sum' (value, S) scalars, 'grad' (value, S) [B,H,W,C]."""
    col = _c(colour, dtype)
    cov = (coverage.detach().cpu() > 0)[..., None]
    ref = _c(ref_u8, dtype)[..., None]
    n_total = n_total or col.numel()
    bg = torch.tensor(float(np.float32(background)), dtype=dtype)
    gs = torch.tensor(float(np.float32(1.0 / n_total)), dtype=dtype)
    comp = torch.where(cov, col, bg)
    d = ref - 255.0 * comp
    dabs = ref + 255.0 * comp.abs()
    zero = torch.zeros((), dtype=dtype)
    return {'sum': ((d * d).sum(), (dabs * dabs).sum()),
            'grad': (torch.where(cov, -2.0 * 255.0 * gs * d, zero), torch.where(cov, 2.0 * 255.0 * gs * dabs, zero))}


def bg_sumsq_int(ref_u8, background_scaled):
    """Per image sum of (ref - b)^2 for an INTEGER b, in exact int64 arithmetic."""
    assert float(background_scaled) == int(background_scaled)
    r = ref_u8.detach().cpu().to(torch.int64).reshape(ref_u8.shape[0], -1)
    return ((r - int(background_scaled)) ** 2).sum(dim=1)


def bg_sumsq(ref_u8, background_scaled, dtype=torch.float64):
    """The same for any b (the float32 number the kernel is handed) -> (value, S) per image."""
    r = _c(ref_u8, dtype).reshape(ref_u8.shape[0], -1)
    b = torch.tensor(float(np.float32(background_scaled)), dtype=dtype)
    return ((r - b) ** 2).sum(dim=1), ((r + b.abs()) ** 2).sum(dim=1)


def objective_value(slots, bg=None, coeff=0.0, n_total=1.0):
    """(sum(slots) + coeff * bg) / n_total, summed exactly (math.fsum) -> (value, S)."""
    s = [float(v) for v in slots.detach().cpu().double().reshape(-1)]
    extra = [float(coeff) * float(bg)] if bg is not None else []
    return math.fsum(s + extra) / float(n_total), math.fsum(abs(v) for v in s + extra) / float(n_total)


# ---------------------------------------------------------------------------------------------------------------------
# inputs both test files use
# ---------------------------------------------------------------------------------------------------------------------

def fan(n):
    """Vertex 0 in the middle of an n-gon: hub degree n, rim degree 3; n + 1 vertices."""
    return np.asarray([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], dtype=np.int32), n + 1


def fan_positions(n, F, gen):
    ang = torch.arange(n, dtype=torch.float32) * (2 * math.pi / n)
    ring = torch.stack([torch.cos(ang), torch.sin(ang), torch.zeros(n)], dim=1)
    xyz = torch.cat([torch.tensor([[0.1, -0.2, 0.3]]), ring])[None].repeat(F, 1, 1)
    return xyz + 0.05 * torch.randn(xyz.shape, generator=gen)


def uv_sphere(n_lon=120, n_rings=125):
    """A closed UV sphere: two poles of degree n_lon, n_rings rings of n_lon vertices of degree 6; V = 2 + n_lon * n_rings."""
    vid = lambda r, l: 1 + r * n_lon + (l % n_lon)
    south = 1 + n_rings * n_lon
    faces = []
    for l in range(n_lon):
        faces.append([0, vid(0, l), vid(0, l + 1)])
        faces.append([south, vid(n_rings - 1, l + 1), vid(n_rings - 1, l)])
        for r in range(n_rings - 1):
            faces.append([vid(r, l), vid(r + 1, l), vid(r + 1, l + 1)])
            faces.append([vid(r, l), vid(r + 1, l + 1), vid(r, l + 1)])
    th = math.pi * (torch.arange(n_rings, dtype=torch.float64) + 1) / (n_rings + 1)
    ph = 2 * math.pi * torch.arange(n_lon, dtype=torch.float64) / n_lon
    ring = torch.stack([8.0 * torch.sin(th)[:, None] * torch.cos(ph)[None], 11.0 * torch.cos(th)[:, None].expand(-1, n_lon),
                        9.0 * torch.sin(th)[:, None] * torch.sin(ph)[None]], dim=-1).reshape(-1, 3)
    pos = torch.cat([torch.tensor([[0.0, 11.0, 0.0]], dtype=torch.float64), ring, torch.tensor([[0.0, -11.0, 0.0]], dtype=torch.float64)])
    return np.asarray(faces, dtype=np.int32), south + 1, pos.float()


def sheared_grid(n=5):
    """A flat n x n grid, sheared so that the six-ring of an interior vertex is centred: its Laplacian is exactly 0."""
    idx = lambda i, j: i * n + j
    faces = [[idx(i, j), idx(i + 1, j), idx(i, j + 1)] for i in range(n - 1) for j in range(n - 1)] + \
            [[idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)] for i in range(n - 1) for j in range(n - 1)]
    xy = torch.tensor([[float(i) + 0.5 * j, float(j), 0.0] for i in range(n) for j in range(n)])
    return np.asarray(faces, dtype=np.int32), n * n, xy


def closed_ring_zero_count(fl, t):
    """The number of entries (v, k) of t [F,V,3] for which t is exactly 0 at v and at every neighbour of v: the entries of L t, L^T t
    and their scales that have no term at all -- counted on the pattern of the mesh, without arithmetic on the values."""
    nz = (t.detach().cpu() != 0).to(torch.float64)
    return int((fl._mm(fl.Labs, nz, False, torch.float64) == 0).sum())


def camera_like(n_views, gen, t_scale=170.0):
    """proj / modelview matrices of the size a real camera gives (focal ratio ~ 4, distances ~ 170..450) without a scene:
    an OpenGL projection and [R | t] with a random rotation."""
    proj = torch.zeros(n_views, 4, 4)
    zn, zf = 0.01, 200.0
    proj[:, 0, 0] = 3.0 + 2.0 * torch.rand(n_views, generator=gen)
    proj[:, 1, 1] = 3.0 + 2.0 * torch.rand(n_views, generator=gen)
    proj[:, 2, 2] = -(zf + zn) / (zf - zn)
    proj[:, 2, 3] = -(2 * zf * zn) / (zf - zn)
    proj[:, 3, 2] = -1.0
    q = torch.randn(n_views, 4, generator=gen, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    mv = rigid(q, (torch.rand(n_views, 3, generator=gen, dtype=torch.float64) * 2 - 1) * 450.0).float()
    mv[:, 1:3, :] *= -1
    tr = torch.eye(4)
    tr[1, 3] = t_scale
    return proj, (mv @ tr).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_fitstep.py (the CPU file measures float32 torch on the same inputs)
# ---------------------------------------------------------------------------------------------------------------------

# (M, K, F): the path each takes is named in tests/test_gpu_fitstep.py
BLEND_SHAPES = [(45006, 150, 32), (45006, 150, 33), (999, 70, 70), (1542, 224, 8), (1542, 225, 8), (1541, 257, 5), (64, 1, 1), (31, 3, 2)]


def blend_inputs(M, K, F, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, generator=g), torch.randn(M, K, generator=g), torch.randn(F, K, generator=g), torch.randn(F, M, generator=g))


def rig_ids(F=32):
    return [slice(0, F), slice(8, 24), torch.tensor([5, 0, 31, 17]), torch.tensor([2, 9, 2, 2, 30]), torch.tensor([-1, 3, -32, -7])]


def rig_inputs(K, Fr, Fc, Fb, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(K, Fr, generator=g), torch.randn(Fr, Fc, generator=g), torch.randn(Fb, K, generator=g)


CLIP_SHAPES = [(32, 9, 15002), (2, 17, 15002), (1, 33, 2049), (3, 4, 1000), (2, 1, 1), (2, 3, 1024), (2, 3, 1025), (2, 3, 2048), (2, 3, 2049)]


def clip_inputs(F, Nc, V, kind, seed=0, zero_images=False):
    """kind 'randn', or 'real': matrix entries to 450, vertices to 100.  zero_images: view 0 of every frame and, with F > 1, every
    view of the last frame have a grad_out of zeros."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'randn':
        mvp, verts = torch.randn(F * Nc, 4, 4, generator=g), torch.randn(F, V, 3, generator=g)
    else:
        mvp = (torch.rand(F * Nc, 4, 4, generator=g) * 2 - 1) * 450.0
        verts = (torch.rand(F, V, 3, generator=g) * 2 - 1) * 100.0
    go = torch.randn(F * Nc, V, 4, generator=g)
    if zero_images:
        go.view(F, Nc, V, 4)[:, 0] = 0
        if F > 1:
            go.view(F, Nc, V, 4)[F - 1] = 0
    return mvp, verts, go


MVP_SHAPES = [(5, 3), (32, 9), (70, 3)]


def mvp_inputs(Fb, Nc, kind, seed=3, n_frames=None, n_cams=None, n_views=None):
    """Tables q_cam [n_cams,4], t_cam, q_frame [n_frames,4], t_frame, proj [n_views,4,4], t_mv and an upstream [Fb*Nc,4,4].  kind
    'randn' or 'camera' (camera_like matrices; small pose corrections around the identity, as a fit has them).  Quaternions are
    not normalised; frame 1's is near zero."""
    g = torch.Generator().manual_seed(seed)
    n_frames, n_views = n_frames or Fb, n_views or Nc
    n_cams = n_cams or n_views
    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == 'randn':
        proj, t_mv = rn(n_views, 4, 4), rn(n_views, 4, 4)
        q_cam, t_cam, q_frame, t_frame = rn(n_cams, 4), rn(n_cams, 3), rn(n_frames, 4), rn(n_frames, 3)
    else:
        proj, t_mv = camera_like(n_views, g)
        ident = torch.tensor([0.0, 0.0, 0.0, 1.0])
        q_cam, t_cam = ident + 0.01 * rn(n_cams, 4), 0.5 * rn(n_cams, 3)
        q_frame, t_frame = ident + 0.2 * rn(n_frames, 4), 5.0 * rn(n_frames, 3)
    if n_frames > 1:
        q_frame[1] = 1e-4 * rn(4)
    return q_cam, t_cam, q_frame, t_frame, proj, t_mv, rn(Fb * Nc, 4, 4)


def mvp_index_cases(gen):
    """(name, n_frames, n_cams, n_views, frame_idx, view_idx, cam_of_view): a repeated frame, a permuted subset of the views, two
    views on one camera row, and each of the three left out."""
    n_frames, n_cams, n_views = 9, 4, 6
    fi = torch.tensor([7, 2, 7, 0, 5])
    vi = torch.tensor([4, 0, 5, 2])
    cov = torch.tensor([0, 1, 2, 3, 0, 2])          # views 0 and 4 -> camera row 0; views 2 and 5 -> row 2
    return [('all', n_frames, n_cams, n_views, fi, vi, cov),
            ('no_frame_idx', n_frames, n_cams, n_views, None, vi, cov),
            ('no_view_idx', n_frames, n_cams, n_views, fi, None, cov),
            ('no_cam_of_view', n_frames, n_views, n_views, fi, vi, None),
            ('none', n_frames, n_views, n_views, None, None, None)]


def pixel_inputs(B, H, W, C, seed=2):
    g = torch.Generator().manual_seed(seed)
    colour = torch.rand(B, H, W, C, generator=g)
    cover = (torch.rand(B, H, W, generator=g) > 0.4).float() * 7
    ref = torch.randint(0, 141, (B, H, W), generator=g, dtype=torch.uint8)
    return colour, cover, ref


def lap_meshes(gen):
    """name -> (faces, V, positions [V,3] float32, {vertex: degree it must have}) for the small meshes (the cfg1 mesh and the sphere
    are added by the tests)."""
    out = {}
    for n in (8, 9, 72, 73, 200, 255, 256):
        f, V = fan(n)
        out[f'fan{n}'] = (f, V, fan_positions(n, 1, gen)[0], {0: n, 1: 3})
    f, V = fan(20)                                     # vertex V: no edge at all
    out['isolated'] = (f, V + 1, torch.cat([fan_positions(20, 1, gen)[0], torch.tensor([[0.3, 0.4, -0.5]])]), {0: 20, V: 0})
    f, V, xy = sheared_grid(5)
    out['grid'] = (f, V, xy, {12: 6, 0: 2})
    return out

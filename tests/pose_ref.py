"""float64 statement on the CPU of the per-frame pose solve ("Pose solve rule"; csrc/landmark_pose.hip k_landmark_pose): the
yardstick of tests/test_gpu_pose.py, itself checked on the CPU by tests/test_pose_ref.py.  Nothing here imports fpc_diffrend_amd.

The convention is tests/landmark_ref.py's: the sums of a pass are evaluated in `dtype` (float64 by default; float32 gives "the same
formula in float32 by torch", in the order the kernel evaluates an entry) and come as (value, S) pairs, S the same formula with every
input replaced by its absolute value and every subtraction by an addition.  Here S is carried by a small algebra (SV) instead of a second
copy of every line: S(a + b) = S(a - b) = S(a) + S(b), S(a b) = S(a) S(b), S(a / b) = S(a) / |b| + |a| S(b) / b^2 (a quotient's error has
a term from its divisor), S(sqrt a) = sqrt S(a); the divisor 1 + h of the Charbonnier value enters with its actual value, as
landmark_ref.py's does.  The trial itself -- the damped 6 x 6 solve, the quaternion update, the rounding of the trial pose to float32 --
is float64 in both statements, as it is in the kernel: only the sums differ."""
import math

import numpy as np
import torch

from fitstep_ref import _c

W_MIN = 1e-6      # a point counts when p.w > W_MIN
TRI = [(i, j) for i in range(6) for j in range(i, 6)]      # A's upper triangle, row-major: the order of normal_out


def _sqrt(t):
    """The correctly rounded square root in t's own format (numpy's is the hardware's; torch's float32 root on the CPU is a vector
    library's and misses the last bit of one value in 200, which is enough to send the float32 statement down another branch than the
    kernel, whose root is IEEE's)."""
    return torch.from_numpy(np.sqrt(t.contiguous().numpy())).reshape(t.shape)


class SV:
    """A value and its scale."""

    def __init__(self, v, s=None):
        self.v, self.s = v, (v.abs() if s is None else s)

    @staticmethod
    def of(o, like):
        return o if isinstance(o, SV) else SV(torch.as_tensor(float(o), dtype=like.v.dtype))

    def __add__(self, o):
        o = SV.of(o, self)
        return SV(self.v + o.v, self.s + o.s)

    def __sub__(self, o):
        o = SV.of(o, self)
        return SV(self.v - o.v, self.s + o.s)

    def __rsub__(self, o):
        return SV.of(o, self) - self

    def __mul__(self, o):
        o = SV.of(o, self)
        return SV(self.v * o.v, self.s * o.s)

    __rmul__ = __mul__
    __radd__ = __add__

    def __truediv__(self, o):
        o = SV.of(o, self)
        return SV(self.v / o.v, self.s / o.v.abs() + self.v.abs() * o.s / (o.v * o.v))

    def sqrt(self):
        return SV(_sqrt(self.v), torch.sqrt(self.s))


def rotation(q):
    """R(q / |q|) [...,3,3] entries as a 3 x 3 list of SV, roma's XYZW form in the order csrc/clip.hip's rigid() has it; q: four SV."""
    qn = ((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3])).sqrt()
    x, y, z, w = (c / qn for c in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def _ksum(t):
    """The sum over the last axis in the kernel's order: entry e goes to lane e mod 256, a lane adds its entries in ascending order, the
    64 lanes of a wave are summed as a balanced binary tree over neighbouring lanes (what the DPP steps of wave_sum_dpp come to: every
    step adds two partial sums, and a + b = b + a to the bit), then the four waves in wave order.  In float32 this is the kernel's sum
    bit for bit, so the float32 statement takes the kernel's branches."""
    n = t.shape[-1]
    pad = (-n) % 256
    if pad:
        t = torch.cat([t, torch.zeros(t.shape[:-1] + (pad,), dtype=t.dtype)], dim=-1)
    t = t.reshape(t.shape[:-1] + (-1, 256))
    lane = t[..., 0, :].clone()
    for k in range(1, t.shape[-2]):
        lane = lane + t[..., k, :]
    wave = lane.reshape(lane.shape[:-1] + (4, 64))
    while wave.shape[-1] > 1:
        wave = wave[..., 0::2] + wave[..., 1::2]
    wave = wave[..., 0]
    return ((wave[..., 0] + wave[..., 1]) + wave[..., 2]) + wave[..., 3]


def normal(x, proj, base, vtx, bary, w, obs, q, t, H, W, inv_c=0.0, dtype=torch.float64):
    """One pass at the poses (q [F,4], t [F,3]): x [F,V,3], proj / base [Nc,4,4], vtx / bary [3,L], w [L] or None, obs [F Nc,L,3];
    inv_c = 1 / c as the float32 the kernel is handed (0: L2).
      p = sum_k bary_k x[vtx_k],  y = base (p, 1),  a = R(q / |q|) y,  z = a + t,  (px, py, pw) = proj (z, 1),  u, v, live, r, rho, d as
      the Landmark rule;  g_u = (W / 2) / pw (P_x - (px / pw) P_w),  J_u = (a x g_u, g_u),  J_v alike;
      A = sum w (J_u^T J_u + J_v^T J_v),  b = sum w (J_u r_u + J_v r_v),  E = sum omega kappa rho  over the live entries, w = omega kappa d.
    -> dict 'A' [F,21], 'b' [F,6], 'E' [F] of (value, S); 'n' [F] the live counts; 'live' [F,Nc,L]; 'res' [F,Nc,L,2] (NaN where not
    live); 'y' [F,Nc,L,3] the points in front of the pose; 'J' [F,Nc,L,2,6]."""
    xx, pp, bb, oo = _c(x, dtype), _c(proj, dtype), _c(base, dtype), _c(obs, dtype)
    qq, tt = _c(q, dtype), _c(t, dtype)
    F, Nc, L = xx.shape[0], pp.shape[0], oo.shape[1]
    assert oo.shape[0] == F * Nc and bb.shape == (Nc, 4, 4) and qq.shape == (F, 4) and tt.shape == (F, 3)
    oo = oo.reshape(F, Nc, L, 3)
    br = torch.as_tensor(np.asarray(bary, dtype=np.float32)).to(dtype)
    om = torch.ones(L, dtype=dtype) if w is None else _c(torch.as_tensor(w), dtype)
    ic = float(np.float32(inv_c))
    sv = lambda v: SV(v)
    corner = [xx[:, torch.as_tensor(np.asarray(vtx[k], dtype=np.int64))] for k in range(3)]            # [F,L,3]
    p = [(sv(br[0][None, None, :]) * sv(corner[0][..., i][:, None]) + sv(br[1][None, None, :]) * sv(corner[1][..., i][:, None]))
         + sv(br[2][None, None, :]) * sv(corner[2][..., i][:, None]) for i in range(3)]                # [F,1,L]
    Bm = lambda r, k: sv(bb[:, r, k][None, :, None])
    Pm = lambda r, k: sv(pp[:, r, k][None, :, None])
    y = [((Bm(r, 0) * p[0] + Bm(r, 1) * p[1]) + Bm(r, 2) * p[2]) + Bm(r, 3) for r in range(3)]         # [F,Nc,L]
    R = rotation([sv(qq[:, i][:, None, None]) for i in range(4)])
    a = [(R[r][0] * y[0] + R[r][1] * y[1]) + R[r][2] * y[2] for r in range(3)]
    z = [a[r] + sv(tt[:, r][:, None, None]) for r in range(3)]
    px, py, pw = (((Pm(r, 0) * z[0] + Pm(r, 1) * z[1]) + Pm(r, 2) * z[2]) + Pm(r, 3) for r in (0, 1, 3))
    us, vs, kap = oo[..., 0], oo[..., 1], oo[..., 2]
    live = (kap > 0) & (om[None, None] > 0) & (pw.v > W_MIN)
    one = torch.ones_like(pw.v)
    sw = SV(torch.where(live, pw.v, one), torch.where(live, pw.s, one))
    hw, hh = 0.5 * W, 0.5 * H
    nx, ny = px / sw, py / sw
    zero = torch.zeros_like(pw.v)
    us0, vs0 = torch.where(live, us, zero), torch.where(live, vs, zero)                                # (what is not live is not read)
    ru = ((nx * 0.5 + 0.5) * (2.0 * hw) - 0.5) - sv(us0)
    rv = ((ny * 0.5 + 0.5) * (2.0 * hh) - 0.5) - sv(vs0)
    s = ru * ru + rv * rv
    if ic > 0.0:
        zu, zv = ru.v * ic, rv.v * ic
        h = _sqrt(1.0 + (zu * zu + zv * zv))
        rho = SV((2.0 * s.v) / (1.0 + h), (2.0 * s.s) / (1.0 + h))
        d = SV(1.0 / h, 1.0 / h + (ic * ic) * (ru.v.abs() * ru.s + rv.v.abs() * rv.s) / (h * h * h))
    else:
        rho, d = s, SV(torch.ones_like(s.v))
    wk = sv(om[None, None] * kap)
    wd = wk * d
    ku, kv = sv(torch.as_tensor(hw, dtype=dtype)) / sw, sv(torch.as_tensor(hh, dtype=dtype)) / sw
    gu = [ku * (Pm(0, i) - nx * Pm(3, i)) for i in range(3)]
    gv = [kv * (Pm(1, i) - ny * Pm(3, i)) for i in range(3)]
    cross = lambda g: [a[1] * g[2] - a[2] * g[1], a[2] * g[0] - a[0] * g[2], a[0] * g[1] - a[1] * g[0]]
    ju, jv = cross(gu) + gu, cross(gv) + gv

    def total(term):
        v = _ksum(torch.where(live, term.v, zero).reshape(F, -1))
        S = torch.where(live, term.s, zero).reshape(F, -1).sum(dim=1)
        return v, S

    A = [total(wd * (ju[i] * ju[j] + jv[i] * jv[j])) for i, j in TRI]
    b = [total(wd * (ju[i] * ru + jv[i] * rv)) for i in range(6)]
    nan = torch.full_like(zero, float('nan'))
    return {'A': (torch.stack([v for v, _ in A], dim=1), torch.stack([S for _, S in A], dim=1)),
            'b': (torch.stack([v for v, _ in b], dim=1), torch.stack([S for _, S in b], dim=1)),
            'E': total(wk * rho), 'n': live.reshape(F, -1).sum(dim=1), 'live': live,
            'res': torch.stack([torch.where(live, ru.v, nan), torch.where(live, rv.v, nan)], dim=-1),
            'y': torch.stack([c.v.expand(F, Nc, L) for c in y], dim=-1),
            'J': torch.stack([torch.stack([c.v for c in ju], dim=-1), torch.stack([c.v for c in jv], dim=-1)], dim=-2)}


def residuals_plain(q, t, y, proj, obs, H, W):
    """(u - u*, v - v*) [Nc,L,2] of ONE frame as a differentiable torch expression of its pose, straight from the rule's text (for
    torch.autograd): y [Nc,L,3] the points in front of the pose, proj [Nc,4,4], obs [Nc,L,3]."""
    qh = q / q.norm()
    x, yy, z, w = qh
    R = torch.stack([torch.stack([1 - 2 * (yy * yy + z * z), 2 * (x * yy - z * w), 2 * (x * z + yy * w)]),
                     torch.stack([2 * (x * yy + z * w), 1 - 2 * (x * x + z * z), 2 * (yy * z - x * w)]),
                     torch.stack([2 * (x * z - yy * w), 2 * (yy * z + x * w), 1 - 2 * (x * x + yy * yy)])])
    zz = y @ R.T + t
    p = torch.einsum('crk,clk->clr', proj[:, :, :3], zz) + proj[:, None, :, 3]
    u = (p[..., 0] / p[..., 3] * 0.5 + 0.5) * W - 0.5
    v = (p[..., 1] / p[..., 3] * 0.5 + 0.5) * H - 0.5
    return torch.stack([u - obs[..., 0], v - obs[..., 1]], dim=-1)


def sincos(h):
    """(sin h, cos h) for h >= 0 as the kernel's pose_sincos has them, operation for operation: h halved until it is at most 1/16, both
    series by Horner, the angle doubled back.  Within 2^6 roundings (7e-15; 1.1e-15 measured) of the library's up to h = pi (tests/test_pose_ref.py)."""
    k = 0
    while h > 0.0625 and k < 64:
        h *= 0.5
        k += 1
    x = h * h
    sc = 1.0 + x * (-1.0 / 6.0 + x * (1.0 / 120.0 + x * (-1.0 / 5040.0 + x * (1.0 / 362880.0 + x * (-1.0 / 39916800.0)))))
    c = 1.0 + x * (-0.5 + x * (1.0 / 24.0 + x * (-1.0 / 720.0 + x * (1.0 / 40320.0 + x * (-1.0 / 3628800.0 + x * (1.0 / 479001600.0))))))
    s = sc * h
    for _ in range(k):
        s, c = (2.0 * s) * c, 1.0 - 2.0 * (s * s)
    return s, c


def trial(A, b, lam, q, t, rotate=True, round32=True):
    """One damped step in float64 from the sums A [21], b [6] at the pose (q [4], t [3]) -> (q', t') rounded to float32, or None when a
    pivot of the Cholesky factorisation of A + lam diag A is not positive (a rejected trial).  round32=False keeps the pose in float64
    (the rule rounds it; scripts/pose_table.py shows what the iteration itself reaches)."""
    lo = 0 if rotate else 3      # (the translation block alone: the kernel's identity block in front of it changes no bit)
    n = 6 - lo
    M = [[0.0] * n for _ in range(n)]
    for k, (i, j) in enumerate(TRI):
        if i >= lo:
            v = float(A[k])
            M[i - lo][j - lo] = v + lam * v if i == j else v
    rhs = [-float(v) for v in b[lo:]]
    Lc = [[0.0] * n for _ in range(n)]
    for j in range(n):      # plain loops in the kernel's order: one rounding per operation, as its unrolled code has them
        dj = M[j][j]
        for m in range(j):
            dj -= Lc[j][m] * Lc[j][m]
        if not dj > 0.0:
            return None
        r = math.sqrt(dj)
        Lc[j][j] = r
        for i in range(j + 1, n):
            v = M[j][i]
            for m in range(j):
                v -= Lc[i][m] * Lc[j][m]
            Lc[i][j] = v / r
    y = [0.0] * n
    for i in range(n):
        v = rhs[i]
        for m in range(i):
            v -= Lc[i][m] * y[m]
        y[i] = v / Lc[i][i]
    delta = [0.0] * n
    for i in range(n - 1, -1, -1):
        v = y[i]
        for m in range(i + 1, n):
            v -= Lc[m][i] * delta[m]
        delta[i] = v / Lc[i][i]
    if not all(math.isfinite(v) for v in delta):
        return None
    qd = [float(v) for v in q]
    if rotate:
        d0, d1, d2 = delta[:3]
        th2 = (d0 * d0 + d1 * d1) + d2 * d2
        th = math.sqrt(th2)
        sn, cs = sincos(0.5 * th)
        sh = 0.5 if th2 < 1e-16 else sn / th
        ax, ay, az, aw = sh * d0, sh * d1, sh * d2, (1.0 if th2 < 1e-16 else cs)
        bn = math.sqrt((qd[0] * qd[0] + qd[1] * qd[1]) + (qd[2] * qd[2] + qd[3] * qd[3]))
        bx, by, bz, bw = (v / bn for v in qd)
        c = [((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by - ax * bz) + ay * bw) + az * bx,
             ((aw * bz + ax * by) - ay * bx) + az * bw, ((aw * bw - ax * bx) - ay * by) - az * bz]      # exp(delta / 2) (x) q / |q|
        cn = math.sqrt((c[0] * c[0] + c[1] * c[1]) + (c[2] * c[2] + c[3] * c[3]))
        qd, delta = [v / cn for v in c], delta[3:]
    out = np.asarray(qd, dtype=np.float64), np.asarray([float(a) + d for a, d in zip(t, delta)])
    return (out[0].astype(np.float32), out[1].astype(np.float32)) if round32 else out


def solve(x, proj, base, vtx, bary, w, obs, q, t, H, W, inv_c=0.0, iters=20, rotate=True, lambda0=1e-3, dtype=torch.float64, round32=True):
    """The solver loop of the rule on every frame: -> (q [F,4] float32, t [F,3] float32, info [F,4] float64 = (E at the input pose, E at
    the returned pose, live entries at the returned pose, accepted trials), trace: per frame the list of trials
    (E before, E of the trial or None, live before, live of the trial, accepted))."""
    pose_t = torch.float32 if round32 else torch.float64
    q_out, t_out = _c(q, pose_t).clone(), _c(t, pose_t).clone()
    F, Nc = q_out.shape[0], proj.shape[0]
    info, trace = torch.zeros(F, 4, dtype=torch.float64), []
    ob = obs.reshape(F, Nc, -1, 3)
    for f in range(F):
        def sums(qf, tf):
            r = normal(x[f:f + 1], proj, base, vtx, bary, w, ob[f], qf[None], tf[None], H, W, inv_c, dtype)
            return r['A'][0][0].numpy(), r['b'][0][0].numpy(), r['E'][0][0].item(), int(r['n'][0])
        qf, tf = q_out[f].clone(), t_out[f].clone()
        A, b, E, n = sums(qf, tf)
        info[f, 0], lam, accepted, tr = E, float(np.float32(lambda0)), 0, []      # (lambda0 as the float32 the kernel is handed)
        for _ in range(iters if n >= 3 else 0):
            new = trial(A, b, lam, qf.numpy(), tf.numpy(), rotate, round32)
            if new is None:
                tr.append((E, None, n, None, False))
                lam = min(lam * 10.0, 1e9)
                continue
            qn = torch.from_numpy(new[0]) if rotate else qf
            tn = torch.from_numpy(new[1])
            A2, b2, E2, n2 = sums(qn, tn)
            keep = n2 >= n and E2 < E
            tr.append((E, E2, n, n2, keep))
            if keep:
                qf, tf, A, b, E, n, accepted = qn, tn, A2, b2, E2, n2, accepted + 1
                lam = max(lam / 10.0, 1e-9)
            else:
                lam = min(lam * 10.0, 1e9)
        if accepted:
            q_out[f], t_out[f] = qf, tf
        info[f, 1], info[f, 2], info[f, 3] = E, n, accepted
        trace.append(tr)
    return q_out, t_out, info, trace


def mean_residual(x, proj, base, vtx, bary, w, obs, q, t, H, W):
    """The mean live |residual| in pixels at the poses (q, t), float64."""
    r = normal(x, proj, base, vtx, bary, w, obs, q, t, H, W)['res'].reshape(-1, 2)
    ok = ~torch.isnan(r[:, 0])
    return float(r[ok].norm(dim=1).mean())

"""GPU: the small kernels of a fit step (csrc/blend.hip, clip.hip, mesh_reg.hip, loss.hip) entry by entry against float64 (tests/fitstep_ref.py).

Each kernel is compared with float64 arithmetic on the float32 inputs that this kernel read (the Laplacian's backward from the
forward's own float32 lap and per).  The error of an output x with float64 reference r is e = max_i |x_i - r_i| / S_i in units of
u = 2^-24, S_i the sum of the absolute values of the terms of entry i; entries with S_i = 0 have no term, must be exactly 0, and
their number must be the one the construction predicts.
  short paths: an entry reached by at most n rounded operations must have e <= n + 2 (derived; n is counted beside each case);
  long sums:   e <= 8 * e32 + 4, e32 the error of float32 torch on the CPU for the same sum against the same reference.
Every line below is printed by a test as "FITSTEP case name e_gpu e32 bound" (pytest -s).

Measured on an MI355X (units of u; the largest over the cases of a row; e32 "-": the bound is n + 2, derived, no yardstick is
measured; the last column is the case of the row that came closest to its own bound).  Outputs that are finished by atomics (g_w, g_mvp, the MVP gradients)
move by a few tenths of u from run to run.  The whole file runs in 13 s there:

  kernel     output                                 cases max e_gpu  max e32   closest to its bound (e_gpu / bound)
  blend      out                                       13      6.09        -   1.04 / 4.0
  blend      g_B                                       13      5.65        -   3.04 / 7.0
  blend      g_w                                       13      1.02     3.61   0.94 / 10.2
  blend      g_vb                                      10      2.35        -   2.35 / 7.0
  blend      out[32:]                                   1      1.12        -   1.12 / 153.0
  rig        w                                          6      2.95        -   2.95 / 34.0
  rig        g_mi                                       6      2.41     3.42   2.34 / 22.3
  rig        g_maps                                     6      0.65     3.08   0.51 / 15.2
  mvp        mvp                                       18      4.65        -   4.65 / 20.0
  mvp        g_q_cam                                   18      1.01        -   0.77 / 27.0
  mvp        g_t_cam                                   18      0.75        -   0.75 / 27.0
  mvp        g_q_frame                                 18      2.44        -   2.44 / 25.0
  mvp        g_t_frame                                 18      1.77        -   1.77 / 25.0
  mvp_idx    mvp                                       12      4.26        -   4.26 / 20.0
  mvp_idx    g_q_cam                                   12      1.14        -   1.14 / 32.0
  mvp_idx    g_t_cam                                   12      1.05        -   1.05 / 27.0
  mvp_idx    g_q_frame                                 12      2.19        -   2.07 / 26.0
  mvp_idx    g_t_frame                                 12      1.56        -   1.47 / 26.0
  clip       out                                       82      3.51        -   3.51 / 6.0
  clip       g_verts                                   55      3.33        -   2.69 / 14.0
  clip       g_mvp                                     55      0.84     2.78   0.84 / 10.7
  lap        L x                                       23      2.83        -   1.32 / 13.0
  lap        L^T y                                     23      3.25        -   1.98 / 10.0
  lap        penalty lap                               23      2.83        -   1.32 / 13.0
  lap        per                                       23      1.86     2.73   1.02 / 7.0
  lap        value                                     23      2.58        -   2.58 / 5.0
  lap        penalty grad                              23      4.15        -   3.05 / 20.0
  lap        wrapper lazy value                        23      3.64     3.60   3.64 / 16.0
  lap        wrapper lazy grad                         23      4.15        -   3.05 / 20.0
  lap        wrapper eager_grad,unit_upstream value    23      3.64     3.60   3.64 / 16.0
  lap        wrapper eager_grad,unit_upstream grad     23      3.79        -   2.03 / 20.0
  lap        wrapper eager_grad value                  23      3.64     3.60   3.64 / 16.0
  lap        wrapper eager_grad grad                   23      4.05        -   2.65 / 23.0
  lap        wrapper acc value                         46      3.64     3.60   3.64 / 16.0
  lap        wrapper acc grad                          46      4.15        -   3.05 / 20.0
  pixel      sum                                        6      0.01     0.20   0.01 / 5.4
  pixel      grad                                       6      2.23        -   2.23 / 7.0
  bg_sumsq   sum                                        7      0.00     0.41   0.00 / 7.2
  objective  value                                      6      0.67        -   0.67 / 2.0
"""
import ctypes

import pytest
import torch

import fitstep_ref as R
from helpers import scene_cameras

pytestmark = pytest.mark.gpu


def _report(case, name, e, e32, bound):
    print(f"FITSTEP {case} {name} e_gpu={e:.3f} e32={'-' if e32 is None else format(e32, '.3f')} bound={bound:.1f}")


def short(case, name, x, ref, n, zeros=0):
    """e <= n + 2 for every entry; n a number or a tensor of the entries' shape (a bound per entry)."""
    r, S = ref
    e, nz = R.measure(x, r, S)
    nmax = float(n.max()) if torch.is_tensor(n) else float(n)
    _report(case, name, e, None, nmax + 2)
    assert nz == zeros, (case, name, nz, zeros)
    if torch.is_tensor(n):
        worst, _ = R.measure(x, r, S * (n.to(torch.float64) + 2.0))
        assert worst <= 1.0, (case, name, worst)
    assert e <= nmax + 2, (case, name, e)


def long_sum(case, name, x, ref, x32, zeros=0):
    r, S = ref
    e, nz = R.measure(x, r, S)
    e32, _ = R.measure(x32, r, S)
    _report(case, name, e, e32, 8 * e32 + 4)
    assert nz == zeros, (case, name, nz, zeros)
    assert e <= 8 * e32 + 4, (case, name, e, e32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _offset_view(t, n_floats):
    """A contiguous copy of t that starts n_floats floats into a larger buffer."""
    buf = torch.zeros(t.numel() + n_floats + 4, dtype=t.dtype, device='cuda')
    v = buf[n_floats:n_floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------------------------------

def _blend_case(case, vb, Bm, w, go, misalign=False):
    from fpc_diffrend_amd import fit
    M, K = Bm.shape
    F = w.shape[0]
    ref, ref32 = R.blend(vb, Bm, w, go), R.blend(vb, Bm, w, go, dtype=torch.float32)
    Bg, wg = (_offset_view(t, 1) if misalign else t.cuda() for t in (Bm, w))
    if misalign:
        assert Bg.data_ptr() % 16 == 4 and wg.data_ptr() % 16 == 4 and Bg.is_contiguous() and wg.is_contiguous()
    else:
        assert Bg.data_ptr() % 16 == 0 and wg.data_ptr() % 16 == 0
    Bg.requires_grad_(True); wg.requires_grad_(True)
    vg = vb.cuda().requires_grad_(True) if vb is not None else None
    out = fit.blend_batched(vg, Bg, wg)
    out.backward(go.cuda())
    short(case, 'out', out, ref['out'], K + 1)          # K products, K - 1 adds of them along one path at most, + v_base: <= K + 1
    short(case, 'g_B', Bg.grad, ref['g_B'], F)          # F products and their adds
    long_sum(case, 'g_w', wg.grad, ref['g_w'], ref32['g_w'][0])     # over M, by slabs of 512 rows and atomics
    assert R.rel_l2(out, ref['out'][0]) < 1e-6 and R.rel_l2(Bg.grad, ref['g_B'][0]) < 1e-6 and R.rel_l2(wg.grad, ref['g_w'][0]) < 1e-5
    if vb is not None:
        short(case, 'g_vb', vg.grad, ref['g_vb'], F)
        assert R.rel_l2(vg.grad, ref['g_vb'][0]) < 1e-6


# the path of each shape (csrc/blend.hip): K <= 224 and 16-byte aligned -> k_blend_fwd_lds, else the register kernel k_blend_fwd
#   (45006, 150, 32)  the benchmark's rig;  (45006, 150, 33), (999, 70, 70): a second and third frame tile of 32 (blockIdx.z of
#   k_blend_bwd_w, the re-staged weights of the LDS kernel);  (1542, 224, 8) / (1542, 225, 8): LDS_KMAX and one past it (register kernel,
#   odd K, a second 2 * KC round);  (1541, 257, 5): odd K, odd M, a third round;  (1542, 226, 8): the register kernel's even-K form;
#   (64, 1, 1), (31, 3, 2): less than one tile each way
@pytest.mark.parametrize("M,K,F", R.BLEND_SHAPES + [(1542, 226, 8)])
def test_blend_entries_against_float64(M, K, F):
    vb, Bm, w, go = R.blend_inputs(M, K, F)
    _blend_case(f"blend({M},{K},{F})", vb, Bm, w, go)


def test_blend_register_kernel_at_small_k_through_misaligned_views():
    """Bmat and w one float into a larger buffer: fpcdr_blend_fwd takes the register kernel at K <= 224 (its even-K form)."""
    vb, Bm, w, go = R.blend_inputs(4500, 150, 32, seed=1)
    _blend_case("blend(4500,150,32)+4B", vb, Bm, w, go, misalign=True)


@pytest.mark.parametrize("M,K,F", [(1542, 224, 8), (1541, 257, 5), (999, 70, 70)])
def test_blend_without_a_base_mesh(M, K, F):
    _, Bm, w, go = R.blend_inputs(M, K, F, seed=2)
    _blend_case(f"blend({M},{K},{F})-novb", None, Bm, w, go)


def test_blend_second_frame_tile_is_clean_after_a_tile_of_inf():
    """w is Inf in all of frames 0 .. 31: the partial sums the LDS kernel parks over the pad columns of the weights are Inf / NaN; the
    second tile's pads are zeroed again, so rows 32 .. 39 are finite and meet the bound (0 * x is 0 only for finite x)."""
    from fpc_diffrend_amd import fit
    M, K, F = 999, 150, 40
    vb, Bm, w, _ = R.blend_inputs(M, K, F, seed=3)
    w[:32] = float('inf')
    out = fit.blend_batched(vb.cuda(), Bm.cuda(), w.cuda())
    ref = R.blend(vb, Bm, w[32:])
    assert bool(torch.isfinite(out[32:]).all())
    short("blend(999,150,40)inf", 'out[32:]', out[32:], ref['out'], K + 1)
    assert not bool(torch.isfinite(out[:32]).any())


# ---------------------------------------------------------------------------------------------------------------------
# rig weights
# ---------------------------------------------------------------------------------------------------------------------

def _rig_case(case, K, Fr, Fc, ids):
    from fpc_diffrend_amd import fit
    cols = R.rig_columns(ids, Fc)
    mi, maps, go = R.rig_inputs(K, Fr, Fc, len(cols))
    ref, ref32 = R.rig_weights(mi, maps, ids, go), R.rig_weights(mi, maps, ids, go, dtype=torch.float32)
    a, m = mi.cuda().requires_grad_(True), maps.cuda().requires_grad_(True)
    w = fit.rig_weights(a, m, ids if isinstance(ids, slice) else ids.cuda())
    w.backward(go.cuda())
    assert w.shape == ref['w'][0].shape and w.is_contiguous()
    short(case, 'w', w, ref['w'], Fr)                   # Fr products and their adds
    long_sum(case, 'g_mi', a.grad, ref['g_mi'], ref32['g_mi'][0])        # over the Fb entries of the batch, 64 lanes + a wave sum
    unnamed = Fc - len(set(cols.tolist()))
    long_sum(case, 'g_maps', m.grad, ref['g_maps'], ref32['g_maps'][0], zeros=Fr * unnamed)     # over K (and the repeats of a column)
    for x, k in ((w, 'w'), (a.grad, 'g_mi'), (m.grad, 'g_maps')):
        assert R.rel_l2(x, ref[k][0]) < 1e-6, (case, k)


def test_rig_weights_entries_against_float64():
    for i, ids in enumerate(R.rig_ids(32)):
        _rig_case(f"rig(150,32,32)ids{i}", 150, 32, 32, ids)
    # 130 entries that draw 10 of 70 columns 13 times each: more than one trip of both 64-lane loops (Fb > 64, K > 128)
    _rig_case("rig(151,70,70)x130", 151, 70, 70, torch.arange(130) * 7 % 70)


# ---------------------------------------------------------------------------------------------------------------------
# MVP chain, plain and indexed
# ---------------------------------------------------------------------------------------------------------------------

def _mvp_tables(Fb, Nc, kind, **kw):
    from fpc_diffrend_amd import scene
    t = list(R.mvp_inputs(Fb, Nc, 'camera' if kind == 'cfg1' else kind, **kw))
    if kind == 'cfg1':          # the cameras of the cfg1 rig, as helpers.scene_mvps makes its matrices
        nv = t[4].shape[0]
        t[4], t[5] = scene_cameras(scene.cfg('cfg1', n_frames=2), [i % 9 for i in range(nv)])
    return t


def _mvp_check(case, got, ref, pairs_cam, pairs_frame, zeros):
    """pairs_*: the largest number of (frame, view) pairs that add into one row: one more rounded add each."""
    short(case, 'mvp', got[0], ref['mvp'], R.MVP_N_VALUE)
    short(case, 'g_q_cam', got[1], ref['g_q_cam'], R.MVP_N_GRAD + pairs_cam, zeros=zeros[0] * 4)
    short(case, 'g_t_cam', got[2], ref['g_t_cam'], R.MVP_N_GRAD + pairs_cam, zeros=zeros[0] * 3)
    short(case, 'g_q_frame', got[3], ref['g_q_frame'], R.MVP_N_GRAD + pairs_frame, zeros=zeros[1] * 4)
    short(case, 'g_t_frame', got[4], ref['g_t_frame'], R.MVP_N_GRAD + pairs_frame, zeros=zeros[1] * 3)


@pytest.mark.parametrize("Fb,Nc", R.MVP_SHAPES)          # (70, 3): 210 pairs, four blocks of 64 threads
@pytest.mark.parametrize("kind", ['randn', 'camera', 'cfg1'])
def test_mvp_chain_entries_against_float64(Fb, Nc, kind):
    from fpc_diffrend_amd import fit
    qc, tc, qf, tf, P, MV, go = _mvp_tables(Fb, Nc, kind)
    ref = R.mvp_chain(qc, tc, qf, tf, P, MV, go)
    for form in ('plain', 'indexed'):
        leaves = [t.cuda().requires_grad_(True) for t in (qc, tc, qf, tf)]
        if form == 'plain':
            out = fit._mvp_func.apply(*leaves, P.cuda(), MV.cuda())
        else:      # (an identity frame index: without any index tensor the call is the plain one)
            out = fit._mvp_indexed_func.apply(*leaves, P.cuda(), MV.cuda(), torch.arange(Fb).cuda(), None, None, Fb, Nc)
        out.backward(go.cuda())
        _mvp_check(f"mvp({Fb},{Nc}){kind}/{form}", [out] + [t.grad for t in leaves], ref, Fb, Nc, (0, 0))


@pytest.mark.parametrize("kind", ['randn', 'cfg1'])
def test_mvp_indexed_tables_against_float64(kind):
    """A repeated frame, a permuted subset of the views, two views on one camera row, each index left out in turn; then 70 frames drawn
    (with repeats) from a table of 80.  Rows no index names get a gradient of exactly 0."""
    from fpc_diffrend_amd import fit
    g = torch.Generator().manual_seed(7)
    cases = R.mvp_index_cases(g)
    big_fi = torch.randint(0, 80, (70,), generator=g)
    cases.append(('70_of_80', 80, 3, 3, big_fi, torch.tensor([2, 0, 1]), None))
    for name, nf, ncam, nv, fi, vi, cov in cases:
        Fb, Nc = (len(fi) if fi is not None else nf), (len(vi) if vi is not None else nv)
        qc, tc, qf, tf, P, MV, go = _mvp_tables(Fb, Nc, kind, n_frames=nf, n_cams=ncam, n_views=nv)
        ref = R.mvp_chain(qc, tc, qf, tf, P, MV, go, fi, vi, cov, Fb, Nc)
        leaves = [t.cuda().requires_grad_(True) for t in (qc, tc, qf, tf)]
        dev = lambda t: t.cuda() if t is not None else None
        out = fit._mvp_indexed_func.apply(*leaves, P.cuda(), MV.cuda(), dev(fi), dev(vi), dev(cov), Fb, Nc)
        out.backward(go.cuda())
        fr = fi.tolist() if fi is not None else list(range(Fb))
        cv = vi.tolist() if vi is not None else list(range(Nc))
        cp = [int(cov[v]) for v in cv] if cov is not None else cv
        rep_f, rep_c = max(fr.count(r) for r in set(fr)), max(cp.count(r) for r in set(cp))
        if name == 'all':
            assert rep_f == 2 and rep_c == 2 and sorted(cv) != cv
        zeros = (ncam - len(set(cp)), nf - len(set(fr)))
        _mvp_check(f"mvp_idx/{name}/{kind}", [out] + [t.grad for t in leaves], ref, Fb * rep_c, Nc * rep_f, zeros)


@pytest.mark.parametrize("Fb,Nc", [(1, 1), (2, 2)])
def test_mvp_plain_call_equals_the_indexed_call_with_identity_indices(Fb, Nc):
    """The two instantiations of k_mvp_fwd / k_mvp_bwd (csrc/clip.hip) run the same arithmetic: the matrices agree to the bit, and so do
    the four gradient tables -- at these sizes a gradient row receives at most two atomic adds into zero, and a + b = b + a."""
    from fpc_diffrend_amd import fit
    qc, tc, qf, tf, P, MV, go = _mvp_tables(Fb, Nc, 'randn')
    res = []
    for idx in ((None, None, None), (torch.arange(Fb).cuda(), torch.arange(Nc).cuda(), torch.arange(Nc).cuda())):
        leaves = [t.cuda().requires_grad_(True) for t in (qc, tc, qf, tf)]
        out = fit._mvp_func.apply(*leaves, P.cuda(), MV.cuda(), *idx, Fb, Nc)
        out.backward(go.cuda())
        res.append([out.detach()] + [t.grad for t in leaves])
    for name, a, b in zip(('mvp', 'g_q_cam', 'g_t_cam', 'g_q_frame', 'g_t_frame'), *res):
        assert torch.equal(a, b), (name, a, b)


# ---------------------------------------------------------------------------------------------------------------------
# clip transform
# ---------------------------------------------------------------------------------------------------------------------

# (32, 9, 15002): the benchmark's shape, 15 workgroups per frame add into grad_mvp by atomics;  (2, 17, 15002), (1, 33, 2049): a second
# and third round of CLIP_VIEWS = 16 views, the last one partial;  (3, 4, 1000): the shape of the older test;  (2, 1, 1): one vertex;
# V = 1024, 1025 (256 * CLIP_VPT and one more: a second workgroup of k_clip_bwd_both), 2048, 2049 (MVP_VPB and one more)
@pytest.mark.parametrize("F,Nc,V", R.CLIP_SHAPES)
@pytest.mark.parametrize("kind,zero_images", [('randn', False), ('real', False), ('randn', True)])
def test_clip_transform_entries_against_float64(F, Nc, V, kind, zero_images):
    from fpc_diffrend_amd import fit
    mvp, verts, go = R.clip_inputs(F, Nc, V, kind, zero_images=zero_images)
    ref, ref32 = R.clip_transform(mvp, verts, go), R.clip_transform(mvp, verts, go, dtype=torch.float32)
    # images without an upstream (view 0 of every frame; every view of the last frame when F > 1): no term in grad_mvp; a frame
    # all of whose views have none: no term in grad_verts
    z_img = (F + (Nc - 1 if F > 1 else 0)) if zero_images else 0
    z_frames = (F if Nc == 1 else (1 if F > 1 else 0)) if zero_images else 0
    case = f"clip({F},{Nc},{V}){kind}{'/zeros' if zero_images else ''}"
    for need_m, need_v in ((True, True), (False, True), (True, False)):       # k_clip_bwd_both, k_clip_bwd_verts, k_clip_bwd_mvp
        m, x = mvp.cuda().requires_grad_(need_m), verts.cuda().requires_grad_(need_v)
        out = fit.transform_clip_batched(m, x)
        out.backward(go.cuda())
        tag = case + ('/both' if need_m and need_v else '/verts' if need_v else '/mvp')
        short(tag, 'out', out, ref['out'], 4)                                 # a product and three adds
        assert R.rel_l2(out, ref['out'][0]) < 1e-6
        if need_v:
            short(tag, 'g_verts', x.grad, ref['g_verts'], 4 * Nc, zeros=z_frames * V * 3)       # per view a product and four adds
            assert R.rel_l2(x.grad, ref['g_verts'][0]) < 1e-6 or z_frames == F
        else:
            assert x.grad is None
        if need_m:
            long_sum(tag, 'g_mvp', m.grad, ref['g_mvp'], ref32['g_mvp'][0], zeros=z_img * 16)   # over V
            assert R.rel_l2(m.grad, ref['g_mvp'][0]) < 1e-5
        else:
            assert m.grad is None


def test_clip_transform_with_the_cfg1_rig():
    """Matrices and vertices of a real scene: the nine cameras of cfg1 on three frames of its mesh."""
    from fpc_diffrend_amd import fit, scene
    from helpers import clip_positions
    sc = scene.cfg('cfg1', n_frames=3)
    _, mvp = clip_positions(sc, list(range(9)), frames=[0, 1, 2])
    V = sc.n_vertices
    verts = (torch.tensor(sc.v_base)[None] + torch.tensor(sc.weights_gt[:3]) @ torch.tensor(sc.blendshapes).t()).reshape(3, V, 3)
    verts[..., 1] += 170.0
    go = torch.randn(27, V, 4, generator=torch.Generator().manual_seed(4))
    assert float(mvp.abs().max()) > 100 and float(verts.abs().max()) > 100
    ref, ref32 = R.clip_transform(mvp, verts, go), R.clip_transform(mvp, verts, go, dtype=torch.float32)
    m, x = mvp.cuda().requires_grad_(True), verts.cuda().requires_grad_(True)
    out = fit.transform_clip_batched(m, x)
    out.backward(go.cuda())
    short("clip(3,9,514)cfg1", 'out', out, ref['out'], 4)
    short("clip(3,9,514)cfg1", 'g_verts', x.grad, ref['g_verts'], 36)
    long_sum("clip(3,9,514)cfg1", 'g_mvp', m.grad, ref['g_mvp'], ref32['g_mvp'][0])


# ---------------------------------------------------------------------------------------------------------------------
# uniform Laplacian: the gather in both modes, the penalty and both forms of its backward
# ---------------------------------------------------------------------------------------------------------------------

def _lap_case(name, faces, V, pos, F, gen, degs=None, exact=False):
    from fpc_diffrend_amd import _lib, fit
    fl = R.FaceLaplacian(faces, V)
    topo = fit.MeshTopology(faces, V, 'cuda')
    D = topo.nbr32.shape[0]
    assert D == max(int(fl.deg.max()), 1)
    for v, d in (degs or {}).items():
        assert int(fl.deg[v]) == d and int((topo.nbr[v] < V).sum()) == d, (name, v, d)
    deg = torch.tensor(fl.deg, dtype=torch.float64)[None, :, None].expand(F, V, 3)
    if exact:       # positions that stay exact binary fractions: copies scaled by 1, 2, 3, ...
        x = pos[None] * torch.arange(1, F + 1, dtype=torch.float32)[:, None, None]
    else:
        x = pos[None].repeat(F, 1, 1) + 0.05 * torch.randn(F, V, 3, generator=gen)
    up = torch.randn(F, V, 3, generator=gen)
    case = f"lap/{name}/F{F}"
    weight, upstream = 7.5, 0.3
    zx = R.closed_ring_zero_count(fl, x)
    assert zx == (F * V if exact else 0)                  # the flat grid: z = 0 everywhere; nothing else is zero
    # (i) fpcdr_laplacian_gather, both modes: degree - 1 adds, the float32 1 / degree and its product, the subtraction: degree + 2
    xg = x.cuda().requires_grad_(True)
    lap = fit._uniform_laplacian.apply(xg, topo.nbr, topo.nbr32, topo.inv_deg)
    lap.backward(up.cuda())
    short(case, 'L x', lap, fl.apply(x), deg + 2, zeros=zx)
    short(case, 'L^T y', xg.grad, fl.apply(up, transpose=True), deg + 2)
    # (ii) fpcdr_laplacian_penalty_fwd: lap, per_f (a long sum over V of float32 norms), the value from per_f
    xc = x.cuda()
    lap2, gx = torch.empty_like(xc), torch.empty_like(xc)
    acc = torch.zeros(F + 1, dtype=torch.float64, device='cuda')
    per = torch.empty(F, dtype=torch.float32, device='cuda')
    val = torch.empty((), dtype=torch.float32, device='cuda')
    _lib.call("fpcdr_laplacian_penalty_fwd", _ptr(xc), _ptr(topo.nbr32), _ptr(topo.inv_deg), _ptr(lap2), _ptr(acc), _ptr(per), _ptr(val),
              weight, F, V, D, _stream())
    short(case, 'penalty lap', lap2, fl.apply(x), deg + 2, zeros=zx)
    per64, _ = R.penalty_value(lap2, weight)
    per32, _ = R.penalty_value(lap2, weight, dtype=torch.float32)
    long_sum(case, 'per', per, (per64, per64), per32)
    v64 = R.penalty_value_from_per(per, weight)
    short(case, 'value', val.reshape(1), (v64.reshape(1), v64.reshape(1)), R.LAP_N_VALUE)
    assert bool((acc == 0).all())                         # the call leaves its accumulators zeroed
    # (iii) fpcdr_laplacian_penalty_bwd from the forward's own lap and per: c_f, y and the transposed gather (LAP_N_GRAD + degree)
    ups = torch.full((1,), upstream, dtype=torch.float32, device='cuda')
    _lib.call("fpcdr_laplacian_penalty_bwd", _ptr(lap2), _ptr(topo.nbr32), _ptr(topo.inv_deg), _ptr(per), _ptr(ups), _ptr(gx), weight,
              F, V, D, _stream())
    gref = R.penalty_grad(lap2, per, fl, weight, float(ups[0]))
    zg = R.closed_ring_zero_count(fl, lap2)
    assert (zg >= F * V) if exact else (zg == 0)
    short(case, 'penalty grad', gx, gref, deg + R.LAP_N_GRAD, zeros=zg)
    # (iv) fit.laplacian_penalty: lazy, eager with a unit upstream, eager with a factor (one more product), twice on the caller's acc
    g1 = R.penalty_grad(lap2, per, fl, weight, 1.0)
    vref = R.penalty_value(lap2, weight)[1].reshape(1)
    v32 = R.penalty_value(lap2, weight, dtype=torch.float32)[1].reshape(1)
    for kw, upv, extra in ((dict(), upstream, 0), (dict(eager_grad=True, unit_upstream=True), 1.0, 0), (dict(eager_grad=True), upstream, 1),
                           (dict(acc=acc), upstream, 0), (dict(acc=acc), upstream, 0)):
        leaf = x.cuda().requires_grad_(True)
        value = fit.laplacian_penalty(leaf, topo, weight, **kw)
        (value * upv).backward() if upv != 1.0 else value.backward()
        tag = 'wrapper ' + ','.join(kw) if kw else 'wrapper lazy'
        long_sum(case, tag + ' value', value.reshape(1), (vref, vref), v32)
        short(case, tag + ' grad', leaf.grad, g1 if upv == 1.0 else gref, deg + R.LAP_N_GRAD + extra, zeros=zg)
        assert bool((acc == 0).all())


def test_laplacian_entries_against_float64_small_meshes():
    """Fans with 8 and 9 spokes (the table is 8 slots wide / the hub is the one ring the whole wave finishes), 72 and 73 (one round of
    64 slots / one slot of a second), 200, 255 and 256 (V = 256 and 257: one workgroup / one thread of a second), a vertex without an
    edge (inv_deg = 0), the sheared flat grid whose interior Laplacian is 0."""
    g = torch.Generator().manual_seed(5)
    for name, (faces, V, pos, degs) in R.lap_meshes(g).items():
        for F in (1, 3):
            _lap_case(name, faces, V, pos, F, g, degs, exact=(name == 'grid'))
    faces, V, pos, degs = R.lap_meshes(g)['fan73']
    _lap_case('fan73', faces, V, pos, 300, g, degs)       # more meshes than the 256 threads of k_penalty_finish


def test_laplacian_entries_against_float64_cfg1_and_sphere():
    from fpc_diffrend_amd import scene
    g = torch.Generator().manual_seed(6)
    sc = scene.cfg('cfg1', n_frames=3)
    pos = torch.tensor(sc.v_base).reshape(-1, 3)
    for F in (1, 3):
        _lap_case('cfg1', sc.pos_idx, sc.n_vertices, pos, F, g)
    faces, V, pos = R.uv_sphere()                         # the benchmark's kind of mesh: 15002 vertices, two poles of degree 120
    for F in (1, 3):
        _lap_case('sphere', faces, V, pos, F, g, {0: 120, V - 1: 120, 1: 5, 200: 6})


# ---------------------------------------------------------------------------------------------------------------------
# pixel loss, background sum of squares, objective value
# ---------------------------------------------------------------------------------------------------------------------

# (9, 1080, 1920, 1): 18.7 M pixels over 8192 x 256 threads: nine trips of the grid-stride loop
@pytest.mark.parametrize("B,H,W,C", [(3, 37, 53, 1), (2, 37, 53, 3), (9, 1080, 1920, 1)])
def test_pixel_loss_entries_against_float64(B, H, W, C):
    from fpc_diffrend_amd import fit
    colour, cover, ref_u8 = R.pixel_inputs(B, H, W, C)
    frac = float((cover > 0).float().mean())
    assert 0.3 <= frac <= 0.7
    uncovered = int((cover <= 0).sum())
    rast = torch.zeros(B, H, W, 4, device='cuda')
    rast[..., 3] = cover.cuda()
    cg, rg = colour.cuda(), ref_u8.cuda()
    for n_total in (None, 3 * colour.numel() + 1):
        ref = R.pixel_loss(colour, cover, ref_u8, n_total)
        ref32 = R.pixel_loss(colour, cover, ref_u8, n_total, dtype=torch.float32)
        s, grad = fit.pixel_loss_fused(cg, rast, rg, n_total=n_total)
        case = f"pixel({B},{H},{W},{C})" + ('' if n_total is None else '/n_total')
        long_sum(case, 'sum', s.reshape(()), ref['sum'], ref32['sum'][0])
        short(case, 'grad', grad, ref['grad'], R.PIXEL_N_GRAD, zeros=C * uncovered)
        assert R.rel_l2(grad, ref['grad'][0]) < 1e-6
        del s, grad, ref, ref32
    del rast, cg, rg
    torch.cuda.empty_cache()


def _bg_images():
    g = torch.Generator().manual_seed(9)
    rnd = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)
    out = [('(3,1080,1920)', rnd(3, 1080, 1920).cuda()),
           ('(3,37,53)', rnd(3, 37, 53).cuda()),                  # 1961 bytes per image: images 2 and 3 start misaligned (scalar path)
           ('(2,1,5)', rnd(2, 1, 5).cuda()),
           ('(1,600,1000)', rnd(1, 600, 1000).cuda()),
           ('(1,1,64*4096+19)', rnd(1, 1, 64 * 4096 + 16 + 3).cuda())]     # the 64-chunk cap, a second trip of the vector loop, a tail of 3
    for off in (16, 1):
        img = rnd(2, 37, 48)
        buf = torch.zeros(img.numel() + 32, dtype=torch.uint8, device='cuda')
        v = buf[off:off + img.numel()].view(img.shape)
        v.copy_(img)
        assert v.data_ptr() % 16 == off % 16 and v.is_contiguous()
        out.append((f'(2,37,48)+{off}B', v))
    return out


def test_background_sum_of_squares_is_exact():
    """Default background: 45 / 255 * 255 is 45.0 in float32, every term an integer below 2^16, a thread's float32 partial of 16
    terms below 2^24, the rest float64: the result EQUALS the int64 sum, per image."""
    from fpc_diffrend_amd import ops
    for name, img in _bg_images():
        got = ops.reference_background_sumsq(img).cpu()
        exact = R.bg_sumsq_int(img, 45.0)
        print(f"FITSTEP bg_sumsq{name} exact max|diff|={float((got - exact.double()).abs().max()):.1f}")
        assert got.dtype == torch.float64 and torch.equal(got, exact.double()), (name, got, exact)


def test_background_sum_of_squares_with_a_fractional_background():
    from fpc_diffrend_amd import ops
    for name, img in _bg_images():
        got = ops.reference_background_sumsq(img, background=0.3)
        ref = R.bg_sumsq(img, 0.3 * 255.0)
        ref32 = R.bg_sumsq(img, 0.3 * 255.0, dtype=torch.float32)
        long_sum(f"bg_sumsq{name}/0.3", 'sum', got, ref, ref32[0])


def test_objective_value_against_an_exact_sum():
    """float64 inside, one rounding to float32: relative error at most 2 u."""
    from fpc_diffrend_amd import _lib
    g = torch.Generator().manual_seed(10)
    for n in (_lib.LOSS_SLOTS, 100, 1):
        slots = torch.rand(n, generator=g, dtype=torch.float64) * 1e7
        bg = torch.rand(1, generator=g, dtype=torch.float64) * 1e9
        for with_bg in (False, True):
            out = torch.zeros(1, dtype=torch.float32, device='cuda')
            sg, bgg = slots.cuda(), bg.cuda()
            _lib.call("fpcdr_objective_value", _ptr(sg), n, _ptr(bgg) if with_bg else None, 0.75, 12345.0, _ptr(out), _stream())
            v, S = R.objective_value(slots, float(bg) if with_bg else None, 0.75, 12345.0)
            e = abs(float(out) - v) / S / R.U
            _report(f"objective(n={n},bg={with_bg})", 'value', e, None, 2.0)
            assert e <= 2.0

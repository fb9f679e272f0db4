"""CPU: the float64 yardstick of the rasterize operator (tests/rasterize_ref.py) is right, and what tests/test_gpu_rasterize.py asks of the
kernels is reachable and discriminates:
  1. the reference's values and hand-written gradient equal torch.autograd through oracle.ops.rasterize evaluated in float64 on the same
     ids to 1e-12 of the entry's scale, for every case and form (with and without the rast_db gradient, instanced and range mode);
  2. every case meets the condition it is there for (the branch, table, tile, bin and skip it reaches), float64 and float32 take the same
     clamp and renormalise branches at every covered pixel with a gradient, the gate margin holds without leaving a pixel out, and the
     entries without a term are as many as predicted;
  3. float32 reaches the bars: the float32 statement's g_pos summed in other orders than the e32 yardstick (pixels permuted; per bin in
     double and then added in float32, as k_grad does) lies within 8 e32 + 4;
  4. ten wrong restatements each miss a bar, a zero count or (one of them) only the bit-identity, on a named case.
Lines "RAST ..." are printed under pytest -s."""
import pytest
import torch

import rasterize_ref as R

F32, F64 = torch.float32, torch.float64
OUTPUTS = ('rast', 'rast_db', 'g_pos')


def _three(name, form, oracle_ops):
    inp = R.case_inputs(name, oracle_ops)
    return inp, R.reference(inp, form), R.reference(inp, form, F32)


def _go_db(inp, form):
    return None if form == 'no rast_db' else inp['go_db']


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference against float64 autograd through the oracle
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,form", [f for f in R.FORMS if f[1] != 'no rast_db'], ids=[i for i in R.FORM_IDS if 'no_rast_db' not in i])
def test_reference_equals_float64_autograd_through_the_oracle(name, form, oracle_ops):
    inp, ref, _ = _three(name, form, oracle_ops)
    pos = inp['pos'].double().requires_grad_(True)
    rast, db = oracle_ops.rasterize(pos, inp['tri'], inp['res'], grad_db=form == 'grad_db', ids=inp['ids'], ranges=inp['ranges'])
    ((rast * inp['go'].double()).sum() + (db * inp['go_db'].double()).sum()).backward()
    assert pos.grad.shape == inp['pos'].shape and (inp['pos'].dim() == 2) == (inp['ranges'] is not None)
    for k, got in (('rast', rast.detach()[..., :3]), ('rast_db', db.detach()), ('g_pos', pos.grad)):
        r, S = ref[k]
        assert bool((S[r != 0] > 0).all()), (name, k)
        worst = float(((r - got).abs() / S.clamp(min=1e-300)).max())
        assert worst <= 1e-12, (name, form, k, worst)
    assert torch.equal(rast.detach()[..., 3].int(), inp['ids'].int())


# ---------------------------------------------------------------------------------------------------------------------
# 2. the conditions of the cases
# ---------------------------------------------------------------------------------------------------------------------

def _pixel_coordinates(pos, res):
    H, W = res
    return torch.stack([(pos[..., 0].double() / pos[..., 3].double() + 1.0) * W / 2, (pos[..., 1].double() / pos[..., 3].double() + 1.0) * H / 2], -1)


def test_lattice_reaches_the_clamp_and_renormalise_branches(oracle_ops):
    inp, ref, r32 = _three('lattice', 'grad_db', oracle_ops)
    H, W = inp['res']
    assert tuple(inp['ids'].shape) == (1, 70, 100) and inp['tri'].shape == (48, 3) and inp['tri'].unique().numel() == 144
    X = _pixel_coordinates(inp['pos'][0], inp['res'])
    off = (X - (X.floor() + 0.5)).abs()            # every vertex on a pixel centre, nudged by less than 0.45 / 256 pixel (float32 pos: 1e-5 pixel)
    assert float(off.max()) < 0.45 / 256 + 1e-5 and float(off.min()) > 0.3 / 256
    w = inp['pos'][0, :, 3]
    assert float(w.min()) >= 0.5 and float(w.max()) <= 2.5
    C = (X.floor() + 0.5)[inp['tri'].long()]                                          # [48,3,2]: right triangles with legs along the axes
    ext = C.amax(1) - C.amin(1)
    assert float(ext.min()) >= 3 and float(ext.max()) <= 11
    right = torch.stack([((c[:, 0] == c[:, 0].roll(1)) | (c[:, 0] == c[:, 0].roll(-1))) & ((c[:, 1] == c[:, 1].roll(1)) | (c[:, 1] == c[:, 1].roll(-1)))
                         for c in C]).long().argmax(1)
    assert int(torch.bincount(right, minlength=3).min()) >= 8                          # the vertex order is permuted: the right angle at 0, 1 and 2
    p32, p64 = r32['px'], ref['px']
    n0, n1, nr = int((p32.b0.v < 0).sum()), int((p32.b1.v < 0).sum()), int(((p32.uc.v + p32.vc.v) > 1).sum())
    print(f"RAST lattice: {p32.n} covered pixels, float32 b0 < 0 at {n0}, b1 < 0 at {n1}, uc + vc > 1 at {nr}")
    assert min(n0, n1, nr) >= 16
    corner = R.corner_pixels(p32)            # beyond a vertex in both other barycentrics: (u, v) is (1, 0), (0, 1) or (0, 0) exactly
    assert int(corner.sum()) >= 4 and int(((p32.b0.v >= 1) | (p32.b1.v >= 1)).sum()) >= 3 and int(((p32.b0.v <= 0) & (p32.b1.v <= 0)).sum()) >= 1
    u, v = r32['rast'][0][p32.bi, p32.yy, p32.xx][:, 0], r32['rast'][0][p32.bi, p32.yy, p32.xx][:, 1]
    assert bool((((u == 0) | (u == 1)) & ((v == 0) | (v == 1)))[corner].all())
    assert not bool((inp['ids'][0, :, 96:] > 0).any())                               # the last bin column: empty in the hint


def test_soup_fills_partial_bins(oracle_ops):
    inp, ref, _ = _three('soup', 'grad_db', oracle_ops)
    B, H, W = inp['ids'].shape
    assert (B, H, W) == (2, 70, 100) and H % 32 and W % 32 and inp['tri'].shape == (400, 3) and inp['tri'].unique().numel() == 1200
    for b in range(B):
        assert int((inp['ids'][b, 64:, :] > 0).sum()) > 100 and int((inp['ids'][b, :, 96:] > 0).sum()) > 50
    assert bool((inp['go'] != 0).all()) and bool((inp['go_db'] != 0).all())
    shown = [inp['ids'][b].unique().numel() - 1 for b in range(B)]
    assert min(shown) > 60, shown                                                     # overlapping: most triangles are hidden or off screen


def test_confetti_overflows_the_vertex_table(oracle_ops):
    inp, ref, _ = _three('confetti', 'grad_db', oracle_ops)
    assert tuple(inp['ids'].shape) == (1, 70, 100) and inp['tri'].shape == (3000, 3) and inp['tri'].unique().numel() == 9000
    assert bool(ref['with_g'].all())
    counts = R.bin_vertex_counts(ref)
    print(f"RAST confetti: {ref['px'].n} covered pixels, distinct vertices with a gradient per bin {sorted(counts.values())}")
    assert max(counts.values()) > R.VT_SLOTS
    assert max(R.bin_vertex_counts(R.reference(inp, 'no grad_db')).values()) > R.VT_SLOTS


def test_grid_shares_vertices_between_triangles_and_bins(oracle_ops):
    inp, ref, _ = _three('grid', 'grad_db', oracle_ops)
    px = ref['px']
    named = torch.bincount(inp['tri'].reshape(-1).long(), minlength=R.GRID_NX * R.GRID_NY).reshape(R.GRID_NY, R.GRID_NX)
    assert bool((named[1:-1, 1:-1] == 6).all()) and tuple(inp['ids'].shape) == (2, 70, 100)
    w = inp['pos'][..., 3]
    assert float(w.max() / w.min()) > 2                                               # perspective
    bins = (px.bi * 100 + px.yy // R.BIN) * 100 + px.xx // R.BIN
    assert bins.unique().numel() >= 20                                                # the mesh spans (nearly) every bin of both images
    spans = 0
    for vtx in range(px.B * px.V):
        m = (px.rows[0] == vtx) | (px.rows[1] == vtx) | (px.rows[2] == vtx)
        spans += int(bins[m].unique().numel() > 1)
    assert spans > 40, spans                                                          # vertices summed by more than one workgroup


def test_big_takes_whole_waves_of_one_triangle(oracle_ops):
    inp, ref, _ = _three('big', 'grad_db', oracle_ops)
    H, W = inp['res']
    ids = inp['ids']
    assert tuple(ids.shape) == (1, 64, 96) and bool((ids > 0).all()) and set(ids.unique().tolist()) == {1, 2}
    X = _pixel_coordinates(inp['pos'][0], inp['res'])[inp['tri'].long()]
    assert bool(((X.amax(1) - X.amin(1)) > torch.tensor([W, H])).all())                # each triangle's box is larger than the frame
    passes = ids[0].reshape(H // 2, 2, W // 32, 32).permute(0, 2, 1, 3).reshape(-1, 64)   # a wave pass of k_grad: two rows of a bin
    whole = int((passes == passes[:, :1]).all(1).sum())
    assert whole > passes.shape[0] // 2, whole
    per_vertex = torch.bincount(torch.cat(ref['px'].rows), minlength=4)
    assert int(per_vertex.min()) > 2000, per_vertex


@pytest.mark.parametrize("name", ['lattice/one-per-triangle', 'soup/one-per-triangle'])
def test_one_per_triangle_gives_every_vertex_one_term(name, oracle_ops):
    for form in ('grad_db', 'no grad_db'):
        inp, ref, r32 = _three(name, form, oracle_ops)
        px, w = ref['px'], ref['with_g']
        live = (inp['go'] != 0).any(-1) | (inp['go_db'] != 0).any(-1)
        assert bool((inp['ids'][live] > 0).all())
        key = px.bi * inp['tri'].shape[0] + px.t
        assert torch.equal(key[w].sort().values, key.unique())                        # exactly one pixel of each visible triangle
        terms = torch.bincount(torch.cat([r[w] for r in px.rows]), minlength=px.B * px.V)
        assert int(terms.max()) == 1
        k32 = R.kernel_order(inp, form)
        assert torch.equal(k32['g_pos one term'], r32['g_pos'][0])
        # g_pos IS the nine components of the chosen pixels
        nine = k32['nine'][px.bi[w], px.yy[w], px.xx[w]]
        g = k32['g_pos one term'].reshape(-1, 4)
        for k in range(3):
            assert torch.equal(g[px.rows[k][w]][:, [0, 1, 3]], nine[:, 3 * k:3 * k + 3])
    if name.startswith('lattice'):
        p32 = r32['px']
        n0, n1, nr = int((p32.b0.v < 0)[w].sum()), int((p32.b1.v < 0)[w].sum()), int(p32.ren[w].sum())
        print(f"RAST {name}: of {int(w.sum())} pixels b0 < 0 at {n0}, b1 < 0 at {n1}, renormalised {nr}")
        assert min(n0, n1, nr) >= 4


def test_sparse_gradient_reaches_the_zero_gradient_exits(oracle_ops):
    inp, ref, _ = _three('soup/sparse-gradient', 'grad_db', oracle_ops)
    nod = R.reference(inp, 'no grad_db')
    go, go_db, ids = inp['go'], inp['go_db'], inp['ids']
    for b, by, bx in R.SPARSE_OFF_BINS:
        sl = (b, slice(by * R.BIN, (by + 1) * R.BIN), slice(bx * R.BIN, (bx + 1) * R.BIN))
        assert not bool(go[sl].any()) and not bool(go_db[sl].any()) and int((ids[sl] > 0).sum()) > 20
    assert {bx for _, _, bx in R.SPARSE_OFF_BINS} >= {0, 3} and {by for _, by, _ in R.SPARSE_OFF_BINS} >= {0, 2}      # full and partial bins
    px = ref['px']
    frac = float(ref['with_g'].float().mean())
    assert 0.3 < frac < 0.7, frac
    for (b, y), with_db, without_db in ((R.SPARSE_ROW_DB_ONLY, True, False), (R.SPARSE_ROW_ZW_ONLY, False, False)):
        row = (px.bi == b) & (px.yy == y)
        assert int(row.sum()) > 30
        assert bool((ref['with_g'][row] == with_db).all()) and bool((nod['with_g'][row] == without_db).all())
    b, y = R.SPARSE_ROW_ZW_ONLY
    assert bool((go[b, y, :, 2:] != 0).all()) and not bool(go[b, y, :, :2].any()) and not bool(go_db[b, y].any())
    b, y = R.SPARSE_ROW_DB_ONLY
    assert bool((go_db[b, y] != 0).all()) and not bool(go[b, y, :, :2].any())


def test_range_mode_sums_over_the_images(oracle_ops):
    inp, ref, _ = _three('range', 'grad_db', oracle_ops)
    T = inp['tri'].shape[0]
    assert inp['pos'].dim() == 2 and inp['ranges'].tolist() == [[0, T], [T // 3, T // 2], [5, 0], [T - 40, 40]] and inp['ranges'].dtype == torch.int32
    ids = inp['ids']
    assert tuple(ids.shape) == (4, 70, 100) and int(ids[2].max()) == 0 and int(ids[3].max()) > T - 40
    assert int(ids[1][ids[1] > 0].min()) > T // 3 and int(ids[1].max()) <= T // 3 + T // 2
    px = ref['px']
    images = torch.zeros(px.V, 4)
    images[px.rows[0], px.bi] = 1
    assert int((images.sum(1) > 1).sum()) > 50 and ref['g_pos'][0].shape == (px.V, 4)


@pytest.mark.parametrize("name,form", R.FORMS, ids=R.FORM_IDS)
def test_gates_are_safe_zeros_are_predicted_and_float32_reaches_the_bars(name, form, oracle_ops):
    inp, ref, r32 = _three(name, form, oracle_ops)
    px, p32, w = ref['px'], r32['px'], ref['with_g']
    B, H, W = inp['ids'].shape
    assert 1 <= B <= 4 and H <= 100 and W <= 100
    # gate safety: no pixel left out
    margin = R.gate_margin(ref)
    assert margin > R.GATE_MARGIN, (name, form, margin)
    assert torch.equal(ref['with_g'], r32['with_g'])
    for q64, q32 in zip(px.gates(), p32.gates()):
        assert torch.equal((q64.v > 0)[w], (q32.v > 0)[w])
    assert torch.equal(px.ren[w], p32.ren[w])
    # the entries without a term
    zeros = R.predicted_zeros(inp, grad_db=form == 'grad_db', output_db=form != 'no rast_db')
    k32 = R.kernel_order(inp, form)
    e32 = {}
    for k in OUTPUTS:
        e32[k], nz = R.measure(r32[k][0], *ref[k])
        assert nz == zeros[k], (name, form, k, nz, zeros[k])
        assert torch.equal(r32[k][0], k32['g_pos one term' if k == 'g_pos' else k])
    print(f"RAST {name} {form}: gate margin {margin:.1f}, e32 " + ", ".join(f"{k} {e32[k]:.3f}" for k in OUTPUTS) + f", zeros {zeros}")
    # g_pos from the float32 statement's nine components in other orders
    nine = k32['nine'][px.bi, px.yy, px.xx]
    Bp = 1 if px.range_mode else B
    gen = torch.Generator().manual_seed(11)
    perm = torch.nonzero(w, as_tuple=True)[0]
    perm = perm[torch.randperm(perm.numel(), generator=gen)]
    G = torch.zeros(Bp * px.V, 4)
    for k in range(3):
        for c, col in enumerate((0, 1, 3)):
            G[:, col].index_add_(0, px.rows[k][perm], nine[perm, 3 * k + c])
    # per (image, bin) in double, rounded once, then added in float32: k_grad's table and its flush
    bins = (px.bi * 100 + px.yy // R.BIN) * 100 + px.xx // R.BIN
    Gb = torch.zeros(B * px.V, 4)
    for bn in bins[w].unique().tolist():
        m = w & (bins == bn)
        part = torch.zeros(B * px.V, 4, dtype=F64)
        for k in range(3):
            rows = px.vi[:, k] + px.bi * px.V
            for c, col in enumerate((0, 1, 3)):
                part[:, col].index_add_(0, rows[m], nine[m, 3 * k + c].double())
        Gb = Gb + part.float()
    Gb = Gb.reshape(B, px.V, 4).sum(0) if px.range_mode else Gb
    for how, x in (('permuted', G), ('per bin', Gb)):
        e, nz = R.measure(x.reshape(ref['g_pos'][0].shape), *ref['g_pos'])
        print(f"RAST {name} {form}: g_pos {how} float32 e={e:.3f} e32={e32['g_pos']:.3f} bound={8 * e32['g_pos'] + 4:.1f}")
        assert nz == zeros['g_pos'] and e <= 8 * e32['g_pos'] + 4, (name, form, how, e)


# ---------------------------------------------------------------------------------------------------------------------
# 4. mutants: wrong float32 restatements must miss a check on their case
# ---------------------------------------------------------------------------------------------------------------------

def _failures(inp, form, ref, r32, got):
    """What of `got` (name -> tensor) misses a check test_gpu_rasterize.py makes: a term where there is none, a zero count, the bar
    8 * e32 + 4 with e32 from the unmutated r32."""
    zeros = R.predicted_zeros(inp, grad_db=form == 'grad_db', output_db=form != 'no rast_db')
    bad = []
    for k, x in got.items():
        r, S = ref[k]
        if not bool((x[S == 0] == 0).all()):
            bad.append((k, 'a term where there is none'))
            continue
        e, nz = R.measure(x, r, S)
        limit = 8 * R.measure(r32[k][0], r, S)[0] + 4
        if nz != zeros[k]:
            bad.append((k, 'zero count', nz, zeros[k]))
        if not e <= limit:
            bad.append((k, round(e, 1), round(limit, 1)))
    return bad


def _mutated(inp, form, mutant, monkeypatch):
    monkeypatch.setattr(R, 'MUTANT', mutant)
    r = R.rasterize(inp['pos'], inp['tri'], inp['ids'], inp['res'], inp['go'], _go_db(inp, form), grad_db=form == 'grad_db', dtype=F32)
    monkeypatch.setattr(R, 'MUTANT', None)
    return {k: r[k][0] for k in OUTPUTS}


@pytest.mark.parametrize("mutant,name,form,outputs", [
    ('clamp_gate_ignored', 'lattice', 'no grad_db', {'g_pos'}),
    ('clamp_gate_ignored', 'lattice/one-per-triangle', 'grad_db', {'g_pos'}),
    ('renormalise_backward_without_dot', 'lattice', 'grad_db', {'g_pos'}),
    ('renormalise_backward_without_dot', 'lattice/one-per-triangle', 'no grad_db', {'g_pos'}),
    ('renormalise_u_only', 'lattice', 'grad_db', {'rast'}),
    ('fy_formed_with_W', 'soup', 'grad_db', {'rast', 'rast_db', 'g_pos'}),
    ('sx_sy_swapped', 'soup', 'grad_db', {'rast_db', 'g_pos'}),
    ('rast_db_chained_without_grad_db', 'soup', 'no grad_db', {'g_pos'}),
    ('rast_db_chained_without_grad_db', 'soup/sparse-gradient', 'no grad_db', {'g_pos'}),
    ('one_pixel_dropped', 'confetti', 'grad_db', {'g_pos'}),
    ('one_pixel_dropped', 'grid', 'no grad_db', {'g_pos'}),
    ('range_gradient_not_summed', 'range', 'grad_db', {'g_pos'}),
    ('w_column_without_fx_fy', 'soup', 'no grad_db', {'g_pos'}),
    ('w_column_without_fx_fy', 'big', 'grad_db', {'g_pos'}),
])
def test_wrong_restatements_miss_the_bars(mutant, name, form, outputs, oracle_ops, monkeypatch):
    """The clamp gate ignored in the backward; the renormalise backward without its - dot term; renormalise applied to u only; fy formed
    with W; sx and sy swapped in rast_db; the rast_db gradient chained although grad_db is off; one pixel's contribution dropped from
    g_pos; the range-mode gradient taken from the first image only; the w column without - fx gpx - fy gpy."""
    inp, ref, r32 = _three(name, form, oracle_ops)
    assert not _failures(inp, form, ref, r32, {k: r32[k][0] for k in OUTPUTS})      # (the unmutated one passes)
    got = _mutated(inp, form, mutant, monkeypatch)
    hit = _failures(inp, form, ref, r32, got)
    print(f"RAST mutant {mutant} on {name} {form}: rel-L2 " + ", ".join(f"{k} {R.rel_l2(got[k], r32[k][0]):.1e}" for k in OUTPUTS) + f": {hit[:4]}")
    assert {h[0] for h in hit} == outputs, (mutant, name, hit)


@pytest.mark.parametrize("name", ['lattice', 'soup', 'big'])
def test_b0_by_division_breaks_bit_identity_and_not_the_bound(name, oracle_ops, monkeypatch):
    """b0 = a0 / at instead of a0 * (1 / at): another rounding of the same quantity.  It stays inside 8 e32 + 4; what catches it is the
    bit-identity with float32_in_kernel_order."""
    inp, ref, r32 = _three(name, 'grad_db', oracle_ops)
    got = _mutated(inp, 'grad_db', 'b0_by_division', monkeypatch)
    differ = int((got['rast'] != r32['rast'][0]).any(-1).sum())
    hit = _failures(inp, 'grad_db', ref, r32, got)
    print(f"RAST mutant b0_by_division on {name}: {differ} pixels of rast differ in a bit, rel-L2 {R.rel_l2(got['rast'], r32['rast'][0]):.1e}: {hit}")
    assert differ > 50 and not hit
    assert not torch.equal(got['rast_db'], r32['rast_db'][0]) and not torch.equal(got['g_pos'], r32['g_pos'][0])

"""CPU: the numpy statement of the overlay rule (tests/overlay_ref.py; DESIGN.md 3, "Overlay rule") against what it stands for -- the
reference's two expressions for the blend, exact rational rounding, and for the wire the true distance of a pixel centre from the
projected edges of its triangle on jittered, perspective-projected grids rasterised by the oracle."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import overlay_ref as R

F32 = np.float32


# ---- blend -----------------------------------------------------------------------------------------------------------------------------
def _all_pairs():
    c, q = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    return c, q


def test_half_weight_is_the_reference_blend_for_all_pairs():
    """w = 128 over all 65 536 (capture, render) pairs: np.clip(np.rint(ref * 0.5 + img * 0.5), 0, 255) in float64, the two
    expressions of render_result_blended.py:149, :154."""
    c, q = _all_pairs()
    want = np.clip(np.rint(c.astype(np.float64) * 0.5 + q.astype(np.float64) * 0.5), 0, 255).astype(np.uint8)
    assert np.array_equal(R.blend(q, c, 128), want)
    # and through the whole statement, as an image
    out = R.overlay(q[None], c[None], w=128)
    assert out.shape == (1, 256, 256, 3) and all(np.array_equal(out[0, ..., k], want) for k in range(3))


def _round_half_even(fr):
    """Round a non-negative Fraction to the nearest integer, ties to even: Python integers only."""
    fl = fr.numerator // fr.denominator
    rest = fr - fl
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl


@pytest.mark.parametrize("w", [0, 1, 77, 128, 200, 255, 256])
def test_blend_rounds_the_exact_rational_half_to_even(w):
    c, q = _all_pairs()
    got = R.blend(q, c, w)
    want = np.array([[_round_half_even(Fraction(w * qq + (256 - w) * cc, 256)) for qq in range(256)] for cc in range(256)])
    assert np.array_equal(got, want)
    if w == 0:
        assert np.array_equal(got, c)
    if w == 256:
        assert np.array_equal(got, q)


def test_outside_capture_keeps_the_capture_off_the_mesh():
    rng = np.random.default_rng(3)
    N, H, W = 2, 6, 9
    ref = rng.integers(0, 256, size=(N, H, W), dtype=np.uint8)
    rast, rast_db = R.raster_inputs(N, H, W, rng)
    cov = rast[..., 3] > 0
    assert 0 < cov.sum() < cov.size
    outs = []
    for img in (rng.integers(0, 256, size=(N, H, W), dtype=np.uint8), R.float_image(N, H, W, rng), np.full((N, H, W), np.nan, dtype=F32)):
        for flip in (False, True):
            out = R.overlay(img, ref, rast, rast_db, w=200, outside_capture=True, flip_rows=flip)
            cv = cov[:, ::-1] if flip else cov
            assert np.array_equal(out[~cv], np.repeat(ref[~cv][:, None], 3, axis=1))
            inside = R.overlay(img, ref, w=200, flip_rows=flip)
            assert np.array_equal(out[cv], inside[cv])
            outs.append(out)
    # without the flag the uncovered pixels are blended like any other
    out = R.overlay(np.zeros((N, H, W), dtype=np.uint8), ref, rast, rast_db, w=256)
    assert not out.any()


# ---- wire against geometry ---------------------------------------------------------------------------------------------------------------
def _grid_mesh(n, jitter, p, rng):
    """Jittered n x n vertex grid in clip space, each cell two triangles; x before y from the generator."""
    lin = np.linspace(-0.85, 0.85, n)
    x = np.tile(lin[None, :], (n, 1)) + rng.uniform(-jitter, jitter, size=(n, n))
    y = np.tile(lin[:, None], (1, n)) + rng.uniform(-jitter, jitter, size=(n, n))
    w = 1.0 + p * x + 0.5 * p * y
    pos = np.stack([x * w, y * w, np.zeros_like(x), w], axis=-1).reshape(-1, 4).astype(F32)
    tri = []
    for a in range(n - 1):
        for b in range(n - 1):
            v00, v01, v10, v11 = a * n + b, a * n + b + 1, (a + 1) * n + b, (a + 1) * n + b + 1
            tri += [(v00, v01, v11), (v00, v11, v10)]
    return pos, np.asarray(tri, dtype=np.int32)


def _edge_distance(pos, tri, rast, R_):
    """float64 distance of every covered pixel's centre to the nearest of its triangle's three projected edge lines; pixel units."""
    ids = rast[..., 3].astype(np.int64)
    yy, xx = np.nonzero(ids > 0)
    t = ids[yy, xx] - 1
    p = pos.astype(np.float64)
    sx = (p[:, 0] / p[:, 3] + 1.0) * R_ / 2.0
    sy = (p[:, 1] / p[:, 3] + 1.0) * R_ / 2.0
    cx, cy = xx + 0.5, yy + 0.5
    d = np.full(t.shape, np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ax, ay, bx, by = sx[tri[t, a]], sy[tri[t, a]], sx[tri[t, b]], sy[tri[t, b]]
        ex, ey = bx - ax, by - ay
        d = np.minimum(d, np.abs(ex * (cy - ay) - ey * (cx - ax)) / np.hypot(ex, ey))
    return yy, xx, d


GEOMETRY = [(6, 0.05, 0.0, 64), (6, 0.05, 0.4, 64), (12, 0.03, 0.4, 128), (24, 0.01, 0.4, 128)]


@pytest.fixture(scope="module")
def rasterised():
    """Every mesh rasterised once by the oracle (float32), generator seeded once, cases in order."""
    from oracle import ops as oracle_ops
    rng = np.random.default_rng(0)
    out = []
    for n, jitter, p, R_ in GEOMETRY:
        pos, tri = _grid_mesh(n, jitter, p, rng)
        rast, rast_db = oracle_ops.rasterize(torch.from_numpy(pos)[None], torch.from_numpy(tri), (R_, R_))
        out.append((pos, tri, rast[0].numpy(), rast_db[0].numpy(), R_))
    return out


@pytest.mark.parametrize("hw", [0.5, 0.75, 1.0])
@pytest.mark.parametrize("case", range(len(GEOMETRY)))
def test_wire_is_within_a_twentieth_of_a_pixel_of_the_true_edge_distance(rasterised, case, hw):
    """b / |grad b| is the first-order distance to the edge b = 0; under perspective it leaves the true distance to the projected edge
    line by a little (at eps = 0.01 two pixels of 3 005 were wrong in one case), so eps = 0.05 px is the margin the rule is held to:
    every covered pixel nearer than hw - eps to an edge of its triangle is wire, every one farther than hw + eps is not, without
    exception, and the undecided band in between holds at most 12 % of the covered pixels."""
    pos, tri, rast, rast_db, R_ = rasterised[case]
    eps = 0.05
    yy, xx, d = _edge_distance(pos, tri, rast, R_)
    wire = R.wire_mask(rast, rast_db, R.hw2_of(hw))[yy, xx]
    must, must_not = d < hw - eps, d > hw + eps
    undecided = 1.0 - (must.sum() + must_not.sum()) / d.size
    print(f"case {GEOMETRY[case]}, hw {hw}: {d.size} covered, wire {int(wire.sum())}, missing {int((must & ~wire).sum())}, "
          f"spurious {int((must_not & wire).sum())}, undecided share {undecided:.3f}")
    assert d.size > 1000
    assert not (must & ~wire).any()
    assert not (must_not & wire).any()
    assert undecided <= 0.12
    # through the whole statement: exactly these pixels carry the wire colour, and nothing off the mesh does
    img = np.zeros((1, R_, R_), dtype=np.uint8)
    out = R.overlay(img, img, rast[None], rast_db[None], w=128, hw2=R.hw2_of(hw), wire_rgb=(1, 2, 3))
    drawn = (out[0] == np.array([1, 2, 3], dtype=np.uint8)).all(axis=-1)
    want = np.zeros((R_, R_), dtype=bool)
    want[yy, xx] = wire
    assert np.array_equal(drawn, want)


# ---- special values ------------------------------------------------------------------------------------------------------------------------
def test_non_finite_values_follow_the_float32_comparison_and_never_raise():
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.25, 1.0, 2.0, 1e-30, 3e38], dtype=F32)
    g = np.stack(np.meshgrid(vals, vals, vals, vals, indexing='ij'), axis=-1).reshape(-1, 4)       # u, v, ux (= vy), uy (= vx)
    n = g.shape[0]
    rast = np.stack([g[:, 0], g[:, 1], np.zeros(n, dtype=F32), np.ones(n, dtype=F32)], axis=-1).reshape(1, 1, n, 4)
    rast_db = np.stack([g[:, 2], g[:, 3], g[:, 3], g[:, 2]], axis=-1).reshape(1, 1, n, 4)
    hw2 = R.hw2_of(0.5)
    with np.errstate(all='raise'):                      # the statement silences what it expects and nothing else is raised
        got = R.wire_mask(rast, rast_db, hw2)[0, 0]
    # the same comparison element by element on float32 scalars
    def on(b, x, y):
        with np.errstate(all='ignore'):
            return bool(F32(b * b) < F32(hw2 * F32(F32(x * x) + F32(y * y))))
    for k in range(0, n, 7):
        u, v, a, b = (F32(z) for z in g[k])
        with np.errstate(all='ignore'):
            s = F32(F32(F32(1.0) - u) - v)
            b2 = F32(0.0) if s < 0 else s
            want = on(u, a, b) or on(v, b, a) or on(b2, F32(a + b), F32(b + a))
        assert bool(got[k]) == want, (k, g[k])
    assert not got[np.isnan(g).all(axis=1)].any()
    # a NaN in every operand of a comparison makes it false; a NaN in u alone leaves the v test standing
    one = lambda u, v, d: bool(R.wire_mask(np.array([u, v, 0, 1], dtype=F32), np.array(d, dtype=F32), hw2))
    assert one(np.nan, 0.0, (1, 0, 1, 0)) and not one(np.nan, np.nan, (1, 0, 1, 0))
    assert not one(0.0, 0.0, (np.nan, np.nan, np.nan, np.nan))
    out = R.overlay(np.zeros((1, 1, n), dtype=np.uint8), np.zeros((1, 1, n), dtype=np.uint8), rast, rast_db, hw2=hw2, wire_rgb=(9, 9, 9))
    assert np.array_equal((out[0, 0] == 9).all(axis=-1), got)


def test_no_triangle_no_wire():
    """id <= 0 (and a NaN id) is never wire, whatever u, v and the derivatives hold -- u = 0 with a unit gradient would be."""
    ids = np.array([0.0, -1.0, -0.0, np.nan, -np.inf, 1.0], dtype=F32)
    n = ids.size
    rast = np.zeros((1, 1, n, 4), dtype=F32)
    rast[..., 3] = ids
    rast_db = np.ones((1, 1, n, 4), dtype=F32)
    ref = np.full((1, 1, n), 100, dtype=np.uint8)
    out = R.overlay(np.zeros((1, 1, n), dtype=np.uint8), ref, rast, rast_db, w=0, hw2=R.hw2_of(0.5), wire_rgb=(0, 255, 0))
    assert np.array_equal(out[0, 0, :5], np.full((5, 3), 100, dtype=np.uint8))
    assert np.array_equal(out[0, 0, 5], np.array([0, 255, 0], dtype=np.uint8))
    # hw2 = 0: no wire anywhere
    assert np.array_equal(R.overlay(np.zeros((1, 1, n), dtype=np.uint8), ref, rast, rast_db, w=0), np.full((1, 1, n, 3), 100, dtype=np.uint8))

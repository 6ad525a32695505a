"""The raster pass census's case table (tests/raster_pass_cases.py) without a GPU: the plan puts a strip in every class for both
window sizes, the models agree with the oracle, the overflow raster is what it is meant to be, and the route witness is wired."""
import ctypes

import numpy as np
import pytest

from oracle import xrs_oracle as orc
from tests import raster_pass_cases as rc


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("name", ['A', 'B'])
def test_the_plan_puts_a_strip_in_every_class(name, K):
    z = rc.census_raster(name)
    rows, cols = z.shape
    strips = rc.strip_classes(z, K, rows, cols)
    assert len(strips) == 12 * 5
    interior = [s for s in strips if s.interior]
    assert {(s.y0, s.x_tile) for s in interior} == {(y0, xt) for y0 in range(4, 44, 4) for xt in (256, 512, 768)}
    seen = {}
    for s in interior:
        for c in rc.class_of(s, K):
            seen.setdefault(c, []).append((s.y0, s.x_tile))
    assert set(seen) == set('abcdefghi'), sorted(seen)
    # the strips the plan names (PLAN's comments)
    for c, where in (('b', (12, 256)), ('c', (20, 256)), ('f', (12, 512)), ('g', (28, 512)), ('h', (40, 512)), ('h', (40, 768)),
                     ('e', (4, 512)), ('d', (20, 768)), ('i', (36, 256)), ('a', (16, 256))):
        assert where in seen[c], (c, where, seen[c])
    assert len(seen['a']) >= 8
    by = {(s.y0, s.x_tile): s for s in strips}
    # the row vote: nothing on a clean strip, nothing on the lone 1e20 (a finite cell it cannot see), the row of the 1e36 cell
    # (finite, reported: nothing to repair), and exactly the rows that hold a NaN / inf everywhere else on the interior
    for s in interior:
        if not s.big:
            assert s.probe == s.hit, (s.y0, s.x_tile, s.probe, s.hit)
    assert by[(40, 512)].probe == frozenset() and by[(40, 512)].hit == frozenset()
    assert by[(40, 768)].probe == frozenset({1 + K // 2}) and by[(40, 768)].hit == frozenset()
    # a dirty strip with an output row whose own K rows are clean (the `hit == 0u` shortcut), and one without
    assert rc.has_clean_row_in_dirty_strip(by[(8, 256)], K)
    assert not rc.has_clean_row_in_dirty_strip(by[(12, 512)], K)
    # j: edge strips, clean and dirty, on every side and in the corners; dirty = one of the raster's own cells is NaN
    edge = [s for s in strips if not s.interior]
    kinds = {(frozenset(rc.edge_sides(s, K, rows, cols)), bool(s.nan)) for s in edge}
    for sides in ({'top'}, {'bottom'}, {'left'}, {'right'}):
        assert (frozenset(sides), False) in kinds and (frozenset(sides), True) in kinds, (sides, kinds)
    corners = [k for k in kinds if len(k[0]) == 2]
    assert {k[0] for k in corners} == {frozenset(c) for c in ({'top', 'left'}, {'top', 'right'}, {'bottom', 'left'}, {'bottom', 'right'})}
    assert {k[1] for k in corners} == {False, True}
    # the last lane: 4 cells of its own on A, 2 on B (ragged), and a NaN among them
    last = by[(28, 1024)]
    assert np.isnan(z[30, 1037]) and (cols - 1036 == (4 if name == 'A' else 2)) and last.nan


def test_the_boundaries_of_strip_is_interior():
    """516 columns: the second tile column is interior, 515: it is not; 24 rows: strip row 16 is interior for K = 5, 21 rows: it is
    not (for K = 3 it still is)."""
    def interior(name, K):
        z = rc.census_raster(name)
        return {(s.y0, s.x_tile) for s in rc.strip_classes(z, K, *z.shape) if s.interior}
    for K in (3, 5):
        assert interior('516', K) == {(y0, 256) for y0 in (4, 8, 12, 16)}
        assert interior('515', K) == set()
    assert interior('21', 5) == {(y0, 256) for y0 in (4, 8, 12)}
    assert interior('21', 3) == {(y0, 256) for y0 in (4, 8, 12, 16)}
    # and each of them has clean interior strips and one dirty one
    z = rc.census_raster('516')
    clean = [s for s in rc.strip_classes(z, 5, *z.shape) if s.interior and not s.probe]
    assert len(clean) >= 2


def test_a_shard_whose_only_nan_is_in_a_halo_row():
    """Rows [16, 32) of A with halos (2, 2) for K = 5 and (1, 1) for K = 3: the strips that reach row 15 or 32 from inside."""
    z = rc.census_raster('A')
    z = z.copy()
    for K, h in ((5, 2), (3, 1)):
        strips = rc.strip_classes(z[16 - h:32 + h], K, 16, 1040, h, h)
        assert {s.y0 for s in strips if s.interior} == {0, 4, 8, 12}
    # rows [0, 16) with halos (0, 2): the NaN column of rows 10 .. 17 reaches the bottom halo rows 16, 17 and nothing else does
    strips = rc.strip_classes(z[0:18], 5, 16, 1040, 0, 2)
    s = {(s.y0, s.x_tile): s for s in strips}[(12, 768)]
    assert s.interior and not s.hit
    # rows [32, 48) with halos (2, 0): strip (0, 512) of the shard sees -inf at row 30 only through its top halo
    strips = rc.strip_classes(z[30:48], 5, 16, 1040, 2, 0)
    s = {(s.y0, s.x_tile): s for s in strips}[(0, 512)]
    assert s.interior and s.hit == frozenset({0}) and not s.nan and s.inf
    # rows [16, 32) with halos (5, 7): strip (8, 256) of the shard is rows 24 .. 27, whose only NaN ... is its own row 24;
    # strip (4, 256), rows 20 .. 23, has its only NaN in the bottom halo
    strips = rc.strip_classes(z[11:39], 5, 16, 1040, 5, 7)
    s = {(s.y0, s.x_tile): s for s in strips}[(4, 256)]
    assert s.interior and s.hit == frozenset({6}) and len(s.nan) == 1
    # rows [12, 28) of A with halos (2, 2): strip (0, 256) of the shard has its only NaN in the halo row above the shard
    strips = rc.strip_classes(z[10:30], 5, 16, 1040, 2, 2)
    s = {(s.y0, s.x_tile): s for s in strips}[(0, 256)]
    assert s.interior and s.hit == frozenset({1}) and s.nan == ((1, 300 - 256 + 2),)


@pytest.mark.parametrize("name", ['A', 'B'])
@pytest.mark.parametrize("mask", ['circle5', 'box3', 'box5'])
def test_the_mean_model_is_the_oracle(name, mask):
    """float32(sum / count) of the exact model == oracle.focal_apply(..., 'mean'): bit-equal where finite, same NaN / inf."""
    z = rc.census_raster(name)
    k = rc.masks()[mask][0]
    m = rc.mean_model(z, k)
    with np.errstate(all='ignore'):
        mine = (m.sum / m.count).astype(np.float32)
        want = orc.focal_apply(z, k, 'mean')
    np.testing.assert_array_equal(mine, want)
    assert want.dtype == np.float32 and np.isnan(want).any() and np.isinf(want).any()
    # windows that lose every tap, and windows with one tap left (the 7x7 hole under the circle); none of the second kind under a box
    assert (m.count == 0).sum() >= (9 if mask != 'box3' else 25)
    assert ((m.count == 1).sum() > 0) == (mask == 'circle5')
    # check_mean accepts the oracle's own plane wherever windows lost taps, and counts what it saw
    kinds = rc.check_mean(np.where(m.count == m.ntaps, (m.sum * (1.0 / m.ntaps)).astype(np.float32), want), m, mask)
    assert all(kinds[key] > 0 for key in ('whole', 'lost', 'empty', 'inf', 'huge')) and kinds['cancel'] == 0


def test_check_mean_bites():
    z = rc.census_raster('A')
    k = rc.masks()['circle5'][0]
    m = rc.mean_model(z, k)
    with np.errstate(all='ignore'):
        good = np.where(m.count == m.ntaps, (m.sum * (1.0 / m.ntaps)).astype(np.float32), (m.sum / m.count).astype(np.float32))
    rc.check_mean(good, m, 'good')
    for y, x, why in ((20, 500, 'whole'), (11, 301, 'lost'), (37, 383, 'empty'), (29, 621, 'inf')):
        bad = good.copy()
        bad[y, x] = np.nextafter(bad[y, x], np.float32(0)) if np.isfinite(bad[y, x]) else np.float32(1.0)
        if why == 'lost':
            bad[y, x] = np.nextafter(bad[y, x], np.float32(0))            # (1 ulp is allowed there; 2 are not)
        with pytest.raises(AssertionError):
            rc.check_mean(bad, m, why)


def test_the_overflow_raster():
    """Every cell finite, the row vote silent on the strips of the pairs, the gradient infinite at the cell between each pair --
    where the reference answers a finite hillshade."""
    z = rc.census_raster('overflow')
    assert np.isfinite(z).all()
    for K in (3, 5):
        strips = {(s.y0, s.x_tile): s for s in rc.strip_classes(z, K, *z.shape)}
        for where in ((8, 256), (12, 256)):
            assert strips[where].interior and not strips[where].probe and strips[where].big, where
    with np.errstate(all='ignore'):
        want = orc.hillshade(z, *rc.LIGHT)
        gy, gx = np.gradient(z)
    for y, x in rc.OVERFLOW_CELLS:
        assert np.isinf(gy[y, x]) or np.isinf(gx[y, x])
    assert np.isfinite(want[1:-1, 1:-1]).all()
    np.testing.assert_allclose([want[c] for c in rc.OVERFLOW_CELLS], [0.82043, 0.17957], rtol=2e-5)
    # the mean model on it: windows holding one huge cell, and windows whose two cancel
    m = rc.mean_model(z, rc.masks()['circle5'][0])
    with np.errstate(all='ignore'):
        good = np.where(m.count == m.ntaps, (m.sum * (1.0 / m.ntaps)).astype(np.float32), (m.sum / m.count).astype(np.float32))
        kinds = rc.check_mean(good, m, 'overflow', exact_huge=True)
    assert kinds['cancel'] > 0 and kinds['huge'] == 0 and kinds['lost'] > 0


def test_the_ulp_sentinel():
    """The window around rc.ULP_CELL: an exact sum whose float32 mean moves when 1 / 13 moves by one float64 ulp, in an output row
    of a dirty interior strip that loses no tap."""
    z = rc.census_raster('ulp')
    m = rc.mean_model(z, rc.masks()['circle5'][0])
    assert m.sum[rc.ULP_CELL] == rc.ULP_SUM and m.count[rc.ULP_CELL] == m.ntaps == 13
    inv = 1.0 / 13
    assert np.float32(rc.ULP_SUM * inv) == np.float32(1000.0)
    assert np.float32(rc.ULP_SUM * np.nextafter(inv, 1.0)) == np.nextafter(np.float32(1000.0), np.float32(2000.0))
    # any order of the 13 taps gives the same float64
    taps = [float(v) for v in z[8:13, 398:403][rc.masks()['circle5'][0] == 1]]
    rng = np.random.default_rng(0)
    for _ in range(50):
        acc = 0.0
        for v in rng.permutation(taps):
            acc += v
        assert acc == rc.ULP_SUM
    s = {(s.y0, s.x_tile): s for s in rc.strip_classes(z, 5, *z.shape)}[(8, 256)]
    assert s.interior and s.probe == frozenset({3})          # row 9: under the windows of all four output rows


def test_dispatch_table():
    assert len(rc.SUBSETS) == 16 and len(set(rc.SUBSETS)) == 16
    got = {rc.ops_text(s): rc.expected_ops(s) for s in rc.SUBSETS}
    assert got == {'-': '-', 'S': 'SH', 'A': 'A', 'SA': 'SACH', 'C': 'C', 'SC': 'SC', 'AC': 'SACH', 'SAC': 'SACH', 'H': 'H',
                   'SH': 'SH', 'AH': 'AH', 'SAH': 'SACH', 'CH': 'CH', 'SCH': 'SCH', 'ACH': 'SACH', 'SACH': 'SACH'}
    assert set(got.values()) == set(rc.INSTANTIATIONS)
    assert len(rc.reachable_combinations()) == 10 * 8 - 4
    assert rc.expected_route(('slope',), 5, True, True, 48, 1040) == "pass(ops=SH,K=5,nt=1,cmask=1,tiles=5x3,seg=0+0)"
    kinds = {(k.shape[0], ct) for k, ct in rc.masks().values()}
    assert kinds == {(3, True), (3, False), (5, True), (5, False)}


def test_fake_hip_answers_the_pass_witness(monkeypatch):
    from tests import fake_hip
    from xrspatial_amd import _lib
    fake_hip.install(monkeypatch)
    assert "xrs_debug_pass_route" in _lib.EXPORTED
    z = np.arange(48, dtype=np.float32).reshape(6, 8)
    out = np.zeros_like(z)
    k = np.ones((3, 3))
    window_route = _lib.window_route()
    args = (z.ctypes.data, out.ctypes.data, None, None, None, None, k.ctypes.data, 3, 3, None, 6, 8, 8, 8, 1.0, 1.0, 225.0, 25.0, 0, 0)
    _lib.call("xrs_raster_pass_f32", *args, None)
    assert _lib.pass_route() == "oracle:xrs_raster_pass_f32"
    _lib.call("xrs_raster_pass_edges_f32", *args, 2, None)
    assert _lib.pass_route() == "oracle:xrs_raster_pass_edges_f32"
    buf = ctypes.create_string_buffer(8)
    assert _lib.load().xrs_debug_pass_route(buf, 8) == len("oracle:xrs_raster_pass_edges_f32") and buf.value == b"oracle:"
    # the window route is another record
    assert _lib.window_route() == window_route

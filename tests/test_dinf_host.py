"""CPU checks of flow_direction(method='dinf') and flow_accumulation(method='dinf' | weights=..).  The reference
has neither, so there is nothing to execute: the rule's statement in NumPy (tests/dinf_oracle.py) is pinned to 3 x 3 literals
worked out by hand, the relaxer's schedule (as a NumPy model with random tile orders and a small CAP) is held to Kahn's order bit
for bit on random graphs, and the argument checks and the ABI's refusals run before any device work."""
import ctypes
import math

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import dinf_oracle as do
from tests import hydrology_oracle as ho

NAN, INF, PI = np.nan, np.inf, np.pi


def _agg(z, res=(1.0, 1.0), **kw):
    import xrspatial_amd as xa
    return xa.DataArray(z, dims=["y", "x"], attrs={"res": res}, **kw)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _centre(ring, centre=10.0, res=(1.0, 1.0)):
    """The angle of the centre of a 3 x 3 raster whose neighbours E, NE, N, NW, W, SW, S, SE are `ring`."""
    z = np.full((3, 3), centre, np.float64)
    for (dr, dc), v in zip(do.OFFSETS, ring):
        z[1 + dr, 1 + dc] = v
    return float(do.flow_direction(z, *res)[1, 1])


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("res", [(1.0, 1.0), (2.0, 0.5), (0.5, 2.0), (30.0, 30.0), (1.0, 1e-9), (1e6, 1.0)])
def test_table_for_several_cell_sizes(res):
    entry.build()
    from xrspatial_amd import hydrology as hy
    b = hy.angle_table(*res)
    td = np.arctan2(np.float64(res[1]), np.float64(res[0]))
    want = [0.0, td, PI / 2, PI - td, PI, PI + td, 3 * PI / 2, 2 * PI - td, 2 * PI]
    assert b.dtype == np.float64 and np.array_equal(_bits(b), _bits(want)) and np.array_equal(_bits(b), _bits(do.table(*res)))
    assert (np.diff(b) > 0).all()
    if res[0] == res[1]:
        assert b[1] == PI / 4


def test_table_that_does_not_increase_is_refused_for_dinf_only():
    entry.build()
    import xrspatial_amd as xa
    from xrspatial_amd import hydrology as hy
    for res in ((1.0, 1e-20), (1e-20, 1.0), (1e17, 1.0)):
        with pytest.raises(ValueError, match="dinf"):
            hy.angle_table(*res)
        with pytest.raises(ValueError):
            do.table(*res)
        z = _agg(np.zeros((3, 4), np.float32), res=res)
        with pytest.raises(ValueError, match="dinf"):
            xa.flow_direction(z, method='dinf')
        with pytest.raises(ValueError, match="dinf"):
            xa.flow_accumulation(_agg(np.zeros((3, 4)), res=res), method='dinf')
        hy.cell_distances(z)                                             # D8 takes these cell sizes


# ------------------------------------------------------------------ directions on literals
def test_cardinal_and_diagonal_winners_get_table_angles():
    b = do.table()
    for n in range(8):                                                   # one lower neighbour: its own angle, bit for bit
        ring = [10.0] * 8
        ring[n] = 7.0
        assert _centre(ring) == b[n], n
    b2 = do.table(2.0, 0.5)
    assert _centre([10, 5, 10, 10, 10, 10, 10, 10], res=(2.0, 0.5)) == b2[1] == np.arctan2(0.5, 2.0)
    assert _centre([10, 10, 10, 10, 10, 4, 10, 10], res=(2.0, 0.5)) == b2[5]


def test_interior_angles_at_square_and_oblong_cells():
    # E = 8, NE = 7: D8 takes NE (3 / sqrt 2 = 2.12 > 2), its square 4.5; facet 0 has s1 = 2, s2 = 1, 1 < 2, q = 5 > 4.5
    assert _centre([8, 7, 10, 10, 10, 10, 10, 10]) == math.atan2(1.0, 2.0) == 0.4636476090008061
    # the same two slopes in every facet: even facets add the turn to b[o], odd ones take it from b[o + 1]
    b = do.table()
    for o in range(8):
        card, diag = ((o + 1) & 7, o) if o & 1 else (o, o + 1)
        ring = [10.0] * 8
        ring[card], ring[diag] = 8.0, 7.0
        want = b[o + 1] - math.atan2(1.0, 2.0) if o & 1 else b[o] + math.atan2(1.0, 2.0)
        assert _centre(ring) == want and b[o] < want < b[o + 1], o
    # res = (2.0, 0.5), facet 0: d1 = 2, d2 = 0.5; s1 = (10 - 8) / 2 = 1, s2 = (8 - 7.9375) / 0.5 = 0.125; 0.125 * 2 < 1 * 0.5;
    # q = 1.015625 > (2.0625 / sqrt 4.25)^2 = 1.00092
    assert _centre([8, 7.9375, 10, 10, 10, 10, 10, 10], res=(2.0, 0.5)) == math.atan2(0.125, 1.0)
    # s2 * d1 == s1 * d2 is no interior candidate: NE = 7.875 gives s2 = 0.25 and 0.5 < 0.5 is false; D8's winner E stays
    # ((10 - 7.875) / sqrt 4.25 = 1.0308 > 1: NE)
    assert _centre([8, 7.875, 10, 10, 10, 10, 10, 10], res=(2.0, 0.5)) == do.table(2.0, 0.5)[1]
    # facet 1 (odd): the cardinal neighbour is N at d1 = 0.5, d2 = 2; s1 = 2, s2 = 0.25, q = 4.0625 > 4
    assert _centre([10, 8.5, 9, 10, 10, 10, 10, 10], res=(2.0, 0.5)) == PI / 2 - math.atan2(0.25, 2.0)


def test_pits_flats_nan_and_infinite_neighbours():
    assert _centre([5.0] * 8, centre=1.0) == -1.0                        # a pit
    assert _centre([10.0] * 8) == -1.0                                   # a flat
    assert _centre([NAN] * 8) == -1.0                                    # nothing to flow to
    assert math.isnan(_centre([5.0] * 8, centre=NAN))
    # E is NaN: facets 0 and 7 have no s1; facet 1 (N = 8, NE = 7) is interior
    assert _centre([NAN, 7, 8, 10, 10, 10, 10, 10]) == PI / 2 - math.atan2(1.0, 2.0)
    # a NaN diagonal: facet 0 has no s2; E stays
    assert _centre([8, NAN, 10, 10, 10, 10, 10, 10]) == 0.0
    # an infinite cell over finite neighbours: the first neighbour in D8's order keeps the infinite drop
    assert _centre([0.0] * 8, centre=INF) == 0.0
    assert _centre([INF] * 8, centre=INF) == -1.0                        # inf - inf is NaN: never taken
    # E = -inf: best = inf and no square is above inf
    assert _centre([-INF, 0, 10, 10, 10, 10, 10, 10]) == 0.0
    assert _centre([8, -INF, 10, 10, 10, 10, 10, 10]) == PI / 4         # s2 = inf: inf < 2 is false


def test_drops_whose_squares_underflow_keep_the_d8_winner():
    # NE's drop 1.5e-200 / sqrt 2 beats E's 1e-200; facet 0 is a candidate (0.5e-200 < 1e-200) with q = 0 + 0, not > 0
    assert _centre([-1e-200, -1.5e-200, 0, 0, 0, 0, 0, 0], centre=0.0) == PI / 4
    assert _centre([-1e-200, -1.2e-200, 0, 0, 0, 0, 0, 0], centre=0.0) == 0.0
    # and squares that overflow: best^2 = inf, q = inf
    assert _centre([-1e200, -1.2e200, 0, 0, 0, 0, 0, 0], centre=1e200) == 0.0


def test_a_cell_has_a_direction_exactly_where_d8_has_one_and_flats_take_the_resolved_code():
    for seed in range(20):
        z = ho.random_terrain(12, 15, seed, np.float64).round(0)         # rounding makes flats and ties
        z[seed % 12, 3] = NAN
        for res in ((1.0, 1.0), (2.0, 0.5)):
            code = ho.flow_direction(z, *res)
            ang = do.flow_direction(z, *res)
            assert np.array_equal(np.isnan(ang), np.isnan(code)) and np.array_equal(ang == -1.0, code == 0)
            assert ((ang[~np.isnan(ang)] == -1.0) | ((ang[~np.isnan(ang)] >= 0) & (ang[~np.isnan(ang)] < 2 * PI))).all()
            resolved = code.copy()
            resolved[code == 0] = 4.0                                    # any codes will do for the statement
            ang2 = do.flow_direction(z, *res, codes=resolved)
            assert np.array_equal(_bits(ang2[code != 0]), _bits(ang[code != 0]))
            assert (ang2[code == 0] == do.table(*res)[6]).all()


# ------------------------------------------------------------------ decoding
def test_share_decoding_at_every_table_entry():
    for res in ((1.0, 1.0), (2.0, 0.5)):
        b = do.table(*res)
        for o in range(8):
            d = np.full((3, 3), -1.0)
            d[1, 1] = b[o]                                               # exactly at a neighbour: one receiver, share 1.0
            _, out = do.edges(d, 'dinf', *res)
            r, q = 1 + do.OFFSETS[o][0], 1 + do.OFFSETS[o][1]
            assert out[4] == [(o, r * 3 + q, 1.0)]
            d[1, 1] = np.nextafter(b[o + 1], 0.0)                        # just below the next one: two receivers
            (n0, _, s0), (n1, _, s1) = do.edges(d, 'dinf', *res)[1][4]
            assert (n0, n1) == (o, (o + 1) & 7) and 0 < s0 < 1e-14 and 1.0 - 1e-14 < s1 <= 1.0
            d[1, 1] = (b[o] + b[o + 1]) / 2
            (_, _, s0), (_, _, s1) = do.edges(d, 'dinf', *res)[1][4]
            assert abs(s0 - 0.5) < 1e-14 and abs(s1 - 0.5) < 1e-14             # (a few ulp of 2 pi over the facet's width)
        for bad in (b[8], 7.0, -0.5, INF, -INF, -1.0000000000000002):
            d = np.full((3, 3), -1.0)
            d[0, 2] = bad
            with pytest.raises(ValueError, match="angle"):
                do.edges(d, 'dinf', *res)
    with pytest.raises(ValueError, match="code"):
        do.edges(np.array([[1, 3, 0]], np.float32), 'd8')
    # a receiver outside the raster or at a NaN cell loses the water
    d = np.array([[0.0, NAN, PI, 0.0]])
    assert [len(e) for e in do.edges(d)[1]] == [0, 0, 0, 0]


def test_accumulation_literals():
    b = do.table()
    # the middle of facet 0, pi / 8: both shares are exactly 0.5; E lies in the raster, NE outside it and its half is lost
    d = np.array([[b[1] / 2, -1.0]])
    got = do.flow_accumulation(d)
    assert got.tolist() == [[1.0, 1.5]]
    # weights, negative and NaN: ordinary values
    assert do.flow_accumulation(np.array([[0.0, 0.0, -1.0]]), weights=np.array([[0.5, -2.0, 4.0]])).tolist() == [[0.5, -1.5, 2.5]]
    got = do.flow_accumulation(np.array([[0.0, 0.0, -1.0], [PI, PI, -1.0]]), weights=np.array([[1.0, NAN, 1.0], [1.0, 1.0, INF]]))
    assert np.array_equal(np.isnan(got), [[False, True, True], [False, False, False]]) and got[1].tolist() == [2.0, 1.0, INF]
    # the order of the gather is E, SE, S, SW, W, NW, N, NE: 1e16 + 1 + 1 - 1e16 depends on it
    d = np.full((3, 3), -1.0)
    d[1, 2], d[2, 1], d[1, 0], d[0, 1] = b[4], b[2], b[0], b[6]          # E, S, W, N of the centre flow into it
    w = np.zeros((3, 3))
    w[1, 2], w[2, 1], w[1, 0], w[0, 1] = 1e16, 1.0, -1e16, 1.0
    assert do.flow_accumulation(d, weights=w)[1, 1] == ((((0.0 + 1e16) + 1.0) + -1e16) + 1.0) == 1.0
    # a NaN cell is outside the graph; a ring raises with its cells and the ones below it
    assert np.isnan(do.flow_accumulation(np.array([[0.0, NAN, PI]]))[0, 1])
    ring = do.codes_to_angles(ho.ring(4, 5, 1, 1, 2, 2))                # four cells in a ring
    ring[0, 0] = b[7]                                                    # a tributary into it: final, not counted
    with pytest.raises(ValueError, match="cycle: 4 cells"):
        do.flow_accumulation(ring)


def test_d8_codes_as_table_angles_give_the_d8_counts():
    for seed in range(6):
        d = ho.random_directions(23, 31, seed)
        want = ho.flow_accumulation(d)
        for res in ((1.0, 1.0), (2.0, 0.5)):
            got = do.flow_accumulation(do.codes_to_angles(d, *res), 'dinf', *res)
            assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(do.flow_accumulation(d, 'd8')), _bits(want))
        w = np.random.default_rng(seed).normal(size=d.shape)
        assert np.array_equal(_bits(do.flow_accumulation(d, 'd8', weights=w)),
                              _bits(do.flow_accumulation(do.codes_to_angles(d), 'dinf', weights=w)))
    d = ho.serpentine(5, 7)
    assert do.flow_accumulation(do.codes_to_angles(d)).max() == 35


# ------------------------------------------------------------------ the schedule
def test_tile_schedule_model_equals_kahn_bit_for_bit_for_any_tile_order():
    capped = splits = 0
    for seed in range(150):
        res = ((1.0, 1.0), (2.0, 0.5))[seed & 1]
        d = do.random_dag(9, 11, seed, res)
        w = np.random.default_rng(seed).normal(size=d.shape) if seed % 3 == 0 else None
        want = do.flow_accumulation(d, 'dinf', *res, weights=w)
        splits += sum(len(e) == 2 for e in do.edges(d, 'dinf', *res)[1])
        for order in range(3):
            got, rounds, cap = do.tile_model(d, 'dinf', *res, weights=w, tile=4, cap=2, rng=np.random.default_rng(1000 * order + seed))
            assert np.array_equal(_bits(got), _bits(want)), (seed, order)
            assert rounds >= 1
            capped += cap
    assert capped > 100 and splits > 1000                               # CAP was reached, and the graphs do split water
    d = do.codes_to_angles(ho.serpentine(9, 10))                         # a path far longer than CAP iterations in one tile
    got, rounds, cap = do.tile_model(d, tile=4, cap=3)
    assert cap and rounds > 3 and np.array_equal(_bits(got), _bits(do.flow_accumulation(d)))


def test_tile_schedule_model_finds_cycles_with_their_cells():
    b = do.table()
    d = do.codes_to_angles(ho.ring(9, 9, 2, 2, 4, 5))                    # 14 cells on the ring, across four tiles of the model
    d[1, 2] = b[6]                                                       # a tributary: (1, 2) -> (2, 2), on the ring
    d[0, 2] = b[6]
    for fn in (do.flow_accumulation, do.tile_model):
        with pytest.raises(ValueError, match="cycle: 14 cells"):
            fn(d)
    two = np.array([[0.0, PI, -1.0]])
    for fn in (do.flow_accumulation, do.tile_model):
        with pytest.raises(ValueError, match="cycle: 2 cells"):
            fn(two)
    # (0, 1) splits between W = (0, 0), its partner in the ring, and SW = (1, 0), which flows on to (1, 1): both lie below the ring
    fed = np.array([[0.0, (b[4] + b[5]) / 2, -1.0], [b[0], -1.0, -1.0]])
    for fn in (do.flow_accumulation, do.tile_model):
        with pytest.raises(ValueError, match="cycle: 4 cells"):
            fn(fed)
    fed[0, 1] = b[5]                                                     # the ring is cut: nothing is left
    assert do.flow_accumulation(fed).tolist() == [[1.0, 2.0, 1.0], [3.0, 4.0, 1.0]]
    assert np.array_equal(do.tile_model(fed)[0], do.flow_accumulation(fed))


# ------------------------------------------------------------------ the package's host side
def test_signatures_and_docstrings():
    import inspect
    entry.build()
    import xrspatial_amd as xa
    from xrspatial_amd import hydrology as hy
    sig = inspect.signature(xa.flow_direction)
    assert list(sig.parameters) == ['agg', 'name', 'resolve_flats', 'method'] and sig.parameters['method'].default == 'd8'
    sig = inspect.signature(xa.flow_accumulation)
    assert list(sig.parameters) == ['flow_dir', 'name', 'method', 'weights']
    assert sig.parameters['method'].default == 'd8' and sig.parameters['weights'].default is None
    assert hy.NEIGHBOUR_CODES == do.CODES and (hy.D8, hy.DINF) == (0, 1)
    assert "D-infinity" in hy.__doc__ and "Not built" in hy.__doc__
    tail = hy.__doc__[hy.__doc__.index("Not built"):]
    assert "float-weighted" not in tail and "D-infinity" not in tail


def test_argument_checks_come_before_device_work():
    entry.build()
    import xrspatial_amd as xa
    ok = _agg(np.zeros((3, 4), np.float32))
    cube = xa.DataArray(np.zeros((2, 3, 4), np.float32), dims=["b", "y", "x"])
    for method in ('D8', 'mfd', None, 8):
        with pytest.raises(ValueError, match="method"):
            xa.flow_direction(ok, method=method)
        with pytest.raises(ValueError, match="method"):
            xa.flow_accumulation(ok, method=method)
    for kw in (dict(method='dinf'), dict(weights=ok), dict(method='dinf', weights=ok)):
        with pytest.raises(ValueError, match="2D"):
            xa.flow_accumulation(cube, **kw)
        with pytest.raises(TypeError, match="dtype"):
            xa.flow_accumulation(_agg(np.zeros((3, 4), np.complex64)), **kw)
    with pytest.raises(ValueError, match="2D"):
        xa.flow_direction(cube, method='dinf')
    with pytest.raises(TypeError, match="dtype"):
        xa.flow_direction(_agg(np.zeros((3, 4), np.complex64)), method='dinf')
    for method in ('d8', 'dinf'):
        with pytest.raises(ValueError, match="differ in shape"):
            xa.flow_accumulation(ok, method=method, weights=_agg(np.zeros((4, 3), np.float32)))
        with pytest.raises(ValueError, match="2D"):
            xa.flow_accumulation(ok, method=method, weights=cube)
        with pytest.raises(TypeError, match="dtype"):
            xa.flow_accumulation(ok, method=method, weights=_agg(np.zeros((3, 4), np.complex64)))
    for res in ((0.0, 1.0), (np.inf, 1.0)):
        with pytest.raises(ValueError, match="cell size"):
            xa.flow_direction(_agg(np.zeros((3, 4), np.float32), res=res), method='dinf')
        with pytest.raises(ValueError, match="cell size"):
            xa.flow_accumulation(_agg(np.zeros((3, 4)), res=res), method='dinf')


def test_dask_and_sharded_rasters_are_refused(monkeypatch):
    entry.build()
    import xrspatial_amd as xa
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.zeros((8, 8), np.float32), (4, 4)))
    shard = object.__new__(xa.ShardedArray)                              # (its constructor wants a device; the refusal does not)
    shard.local = np.zeros((8, 8), np.float32)
    ok = _agg(np.zeros((8, 8), np.float32))
    for bad, kind, err in ((lazy, "dask", NotImplementedError), (_agg(shard), "sharded", NotImplementedError)):
        with pytest.raises(err, match=kind):
            xa.flow_direction(bad, method='dinf')
        with pytest.raises(err, match=kind):
            xa.flow_accumulation(bad, method='dinf')
        with pytest.raises(err, match=kind):
            xa.flow_accumulation(bad, weights=ok)
        with pytest.raises(err, match=kind):
            xa.flow_accumulation(ok, weights=bad)


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xa
    if xa.has_hip():
        pytest.skip("a GPU is present")
    z = _agg(np.zeros((4, 4), np.float32))
    for call in (lambda: xa.flow_direction(z, method='dinf'), lambda: xa.flow_direction(z, method='dinf', resolve_flats=True),
                 lambda: xa.flow_accumulation(_agg(np.zeros((4, 4))), method='dinf'),
                 lambda: xa.flow_accumulation(z, weights=_agg(np.ones((4, 4), np.int16))),
                 lambda: xa.flow_accumulation(xa.Dataset({"a": _agg(np.zeros((4, 4)))}), method='dinf')):
        with pytest.raises(xa.XrsError):
            call()
    with xa.fuse():                                                      # eager inside a scope: the same error, at the call
        with pytest.raises(xa.XrsError):
            xa.flow_accumulation(_agg(np.zeros((4, 4))), method='dinf')


def workspace_layout(rows, cols):
    """The written layout of xrs_flow_accumulate_frac's workspace: the rounds' part (4160 head words, a flag and a list word a
    tile), 256 bytes of counters, one byte a cell; every part on a 256-byte boundary."""
    up = lambda v: (v + 255) & ~255                                      # noqa: E731
    tiles = -(-rows // 64) * -(-cols // 64)
    return up(4160 * 4) + 2 * up(4 * tiles) + 256 + up(rows * cols)


def test_abi_refuses_bad_arguments_before_device_work():
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    assert {"xrs_flow_direction_dinf", "xrs_flow_accumulate_frac_workspace_size", "xrs_flow_accumulate_frac"} <= set(_lib.EXPORTED)
    fake, other, third = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(768)
    nan, inf = float("nan"), float("inf")
    good = (ctypes.c_double * 9)(*do.table())
    for shape in ((0, 5), (5, -1), (1 << 16, 1 << 16), (1, (1 << 32) - 1)):
        assert _lib.workspace_bytes("flow_accumulate_frac", *shape) == 0, shape
    for shape in ((1, 1), (64, 64), (65, 130), (1, 4097), (257, 513), (1, (1 << 32) - 2)):
        assert _lib.workspace_bytes("flow_accumulate_frac", *shape) == workspace_layout(*shape), shape
    assert lib.xrs_flow_accumulate_frac_workspace_size(4, 4, None) != 0 and "null" in _lib.last_error()

    def tab(*values):
        return (ctypes.c_double * 9)(*values)

    bad_tables = (tab(*([0.0] * 9)), tab(0, 1, 2, 3, 3, 4, 5, 6, 7), tab(0.5, 1, 2, 3, 4, 5, 6, 7, 8), tab(0, 1, 2, 3, 4, 5, 6, 7, inf),
                  tab(0, 1, 2, nan, 4, 5, 6, 7, 8))

    def direction(data=fake, dtype=9, rows=4, cols=5, cx=1.0, cy=1.0, dg=2.0 ** 0.5, table=good, codes=None, out=other):
        return lib.xrs_flow_direction_dinf(data, dtype, rows, cols, cx, cy, dg, table, codes, out, None)

    for kw, text in ((dict(rows=-1), "negative shape"), (dict(dtype=4), "dtype"), (dict(dtype=10), "dtype"), (dict(cx=0.0), "positive"),
                     (dict(cy=-1.0), "positive"), (dict(dg=nan), "positive"), (dict(cx=inf), "positive"), (dict(table=None), "null table"),
                     (dict(data=None), "null"), (dict(out=None), "null"), (dict(out=fake), "overwrite"),
                     (dict(codes=other), "overwrite"), (dict(rows=1 << 31), "too large")):
        assert direction(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    for table in bad_tables:
        assert direction(table=table) != 0 and "table" in _lib.last_error()
    assert direction(rows=0, data=None, out=None) == 0                   # nothing to do

    status = (ctypes.c_int64 * 256)()

    def frac(d=fake, method=1, table=good, wts=None, wdt=8, rows=4, cols=5, work=third, out=other, st=status, flags=0):
        return lib.xrs_flow_accumulate_frac(d, method, table, wts, wdt, rows, cols, work, out, st, flags, None)

    for kw, text in ((dict(cols=-1), "negative shape"), (dict(method=2), "method"), (dict(method=-1), "method"),
                     (dict(wts=ctypes.c_void_p(1024), wdt=4), "weights dtype"), (dict(wts=ctypes.c_void_p(1024), wdt=11), "weights dtype"),
                     (dict(flags=2), "flags"), (dict(table=None), "null table"), (dict(st=None), "null"), (dict(d=None), "null"),
                     (dict(work=None), "null"), (dict(out=None), "null"), (dict(out=fake), "overwrite"),
                     (dict(wts=other), "overwrite"), (dict(rows=1 << 16, cols=1 << 16), "2^32 - 2"),
                     (dict(rows=1, cols=(1 << 32) - 1), "2^32 - 2")):
        assert frac(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    for table in bad_tables:
        assert frac(table=table) != 0 and "table" in _lib.last_error()
        status[0] = 7
        assert frac(method=0, table=table, rows=0) == 0 and status[0] == 0      # D8 reads no table; the words are cleared
    assert frac(method=0, table=None, cols=0, d=None, work=None, out=None) == 0

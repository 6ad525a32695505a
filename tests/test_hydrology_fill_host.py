"""CPU checks of fill and flow_direction(resolve_flats=True).  There is no reference to execute: the NumPy
statement of the two rules (tests/hydrology_fill_oracle.py) is pinned to small literals worked out by hand; its priority flood is
held against the definition (every path, on tiny rasters) and against the Jacobi fixed point; "every path drains" and "no cycle"
are shown on the rasters the GPU test uses, with tests/hydrology_oracle.py's flow_accumulation and basins; and the argument
checks, the refusals and the ABI's validation run before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import hydrology_fill_oracle as fo
from tests import hydrology_oracle as ho

NAN, INF = np.nan, np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _agg(z, res=(1.0, 1.0), **kw):
    import xrspatial_amd as xa
    return xa.DataArray(z, dims=["y", "x"], attrs={"res": res}, **kw)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want, np.asarray(got).dtype)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), (got, want)


def _fill_all_ways(z, want=None):
    """The flood, the Jacobi fixed point and (small rasters) the definition agree; returns the flood's result."""
    z = np.asarray(z)
    got = fo.fill(z)
    _same(fo.fill_fixed_point(z)[0], got)
    if z.size <= 25:                                                     # at most nine interior cells: every path is affordable
        _same(fo.fill_brute_force(z), got)
    if want is not None:
        _same(got, want)
    return got


# ------------------------------------------------------------------ fill: the rule on literals
def test_rim_mask():
    z = np.zeros((5, 6))
    z[2, 3] = NAN
    want = np.ones((5, 6), bool)
    want[1:4, 1] = False                                                 # the only cells with eight non-NaN neighbours
    want[2, 3] = False                                                   # a NaN cell is no rim cell
    assert np.array_equal(fo.rim_mask(z), want)
    assert fo.rim_mask(np.zeros((2, 9))).all() and fo.rim_mask(np.zeros((1, 1))).all()
    assert not fo.rim_mask(np.full((3, 3), INF))[1, 1]                   # an infinite neighbour is a neighbour


def test_bowl_with_one_notch_rises_to_the_notch():
    z = [[9, 9, 4, 9, 9],
         [9, 1, 2, 1, 9],
         [9, 2, 0, 2, 9],
         [9, 1, 2, 5, 9],
         [6, 9, 9, 9, 9]]
    want = [[9, 9, 4, 9, 9],
            [9, 4, 4, 4, 9],                                             # not 6, the other low rim cell, and not 9
            [9, 4, 4, 4, 9],
            [9, 4, 4, 5, 9],                                             # a cell above the level keeps its value
            [6, 9, 9, 9, 9]]
    for dt in (np.float32, np.float64):
        got = _fill_all_ways(np.array(z, dt), want)
        assert got.dtype == dt


def test_pits_joined_by_a_diagonal_share_a_spill_level():
    z = np.array([[9, 9, 9, 9, 9, 9],
                  [9, 1, 8, 8, 8, 9],
                  [9, 8, 2, 3, 3, 3],                                    # pit B = 2 spills at 3 along the channel to the rim
                  [9, 8, 8, 8, 8, 9],
                  [9, 8, 8, 8, 8, 9],
                  [9, 9, 9, 9, 9, 9]], np.float32)
    want = z.copy()
    want[1, 1] = 3                                                       # pit A = 1 touches B only diagonally; edge-connected it would rise to 8
    want[2, 2] = 3
    _fill_all_ways(z, want)


def test_a_nan_cell_drains_the_pit_beside_it():
    z = np.array([[9, 9, 9, 9, 9],
                  [9, 8, 8, 8, 9],
                  [9, 8, 1, NAN, 9],
                  [9, 8, 8, 8, 9],
                  [9, 9, 9, 9, 9]], np.float64)
    _fill_all_ways(z, z)                                                 # the pit is a rim cell: nothing rises


def test_a_pit_nested_in_a_larger_depression():
    z = np.array([[9, 9, 9, 9, 9, 9, 9],
                  [9, 3, 3, 3, 3, 3, 9],
                  [9, 3, 7, 7, 7, 3, 9],
                  [9, 3, 7, 1, 7, 3, 6],                                 # the raster's outlet: 6
                  [9, 3, 7, 7, 7, 3, 9],
                  [9, 3, 3, 3, 3, 3, 9],
                  [9, 9, 9, 9, 9, 9, 9]], np.float32)
    want = z.copy()
    want[1:6, 1:6] = 6                                                   # the moat rises to the outlet
    want[2:5, 2:5] = 7                                                   # the inner ring stands above it; its pit rises to the ring
    _fill_all_ways(z, want)


def test_infinities_are_ordinary_values():
    z = np.full((5, 5), INF)
    z[1:4, 1:4] = [[1, 2, 3], [4, -INF, 6], [7, 8, 9]]
    want = z.copy()
    want[1:4, 1:4] = INF                                                 # every way out leads over +inf
    _fill_all_ways(z, want)
    z[0, 0] = -INF                                                       # a rim cell at -inf beside (1, 1)
    want = z.copy()
    want[2, 2] = 1                                                       # the centre drains over (1, 1)
    _fill_all_ways(z, want)


def test_rasters_without_an_interior_are_returned_as_they_are():
    for z in (np.array([[3, 1, 4, 1, 5]], np.float32), np.array([[2, 0], [0, 2]], np.float64), np.array([[7]], np.float32),
              np.array([[5], [1], [5]], np.float64), np.zeros((0, 4), np.float32)):
        got = _fill_all_ways(z, z)
        assert got.dtype == z.dtype and got.shape == z.shape


def test_an_integer_raster_gives_float64():
    z = np.array([[9, 9, 4, 9, 9], [9, 1, 2, 1, 9], [9, 2, 0, 2, 9], [9, 1, 2, 5, 9], [6, 9, 9, 9, 9]], np.int16)
    got = _fill_all_ways(z)
    assert got.dtype == np.float64 and got[1:4, 1:4].tolist() == [[4, 4, 4], [4, 4, 4], [4, 4, 5]]
    assert fo.fill(z.astype(np.uint8)).dtype == np.float64 and fo.fill(z.astype(bool)).dtype == np.float64


def test_flood_definition_and_fixed_point_agree_on_tiny_rasters():
    """3000 random rasters of at most 4 x 4 and 1000 of 5 x 5 (values 0 .. 3: ties everywhere; one cell in ten NaN)."""
    rng = np.random.default_rng(17)
    raised = 0
    for k in range(4000):
        rows, cols = (int(rng.integers(1, 5)), int(rng.integers(1, 5))) if k < 3000 else (5, 5)
        if k % 7 == 0:
            rows, cols = (4, 4) if k < 3000 else (5, 5)
        z = rng.integers(0, 4, (rows, cols)).astype(np.float64)
        z[rng.random((rows, cols)) < 0.1] = NAN
        if k % 5 == 0:
            z[rng.random((rows, cols)) < 0.1] = INF
        got = _fill_all_ways(z)
        raised += int((got[~np.isnan(z)] != z[~np.isnan(z)]).sum())
        assert (got[~np.isnan(z)] >= z[~np.isnan(z)]).all() and np.isin(got[~np.isnan(z)], z[~np.isnan(z)]).all()
    assert raised > 100                                                  # the rasters do hold depressions


# ------------------------------------------------------------------ flats: the rule on literals
def test_a_flat_with_one_drained_end():
    z = np.full((3, 7), 9.0, np.float32)
    z[1, :6] = 5                                                         # a ledge of 5 between walls; (1, 0) is its rim cell
    code, d = fo.resolve_flats(z)
    assert ho.flow_direction(z)[1, 1:6].tolist() == [0, 0, 0, 0, 0]
    assert d[1].tolist() == [0, 1, 2, 3, 4, 5, 0] and code[1, 1:6].tolist() == [16] * 5
    code, d = fo.resolve_flats(z[:, ::-1])
    assert d[1].tolist() == [0, 5, 4, 3, 2, 1, 0] and code[1, 1:6].tolist() == [1] * 5
    assert np.array_equal(code[[0, 2]], ho.flow_direction(z[:, ::-1])[[0, 2]])           # drained cells keep their codes


def test_two_outlets_at_equal_distance_the_order_decides():
    z = np.full((3, 7), 9.0)
    z[1, :] = 5
    code, d = fo.resolve_flats(z)
    assert d[1].tolist() == [0, 1, 2, 3, 2, 1, 0]
    assert code[1].tolist() == [0, 16, 16, 1, 1, 1, 0]                   # (1, 3): E comes before W; the two rim cells are outlets
    z = np.full((5, 5), 5.0)                                             # all level: every interior cell beside the rim takes E or SE first
    code, d = fo.resolve_flats(z)
    assert d[1:4, 1:4].tolist() == [[1, 1, 1], [1, 2, 1], [1, 1, 1]]
    assert code[1:4, 1:4].tolist() == [[8, 32, 1], [8, 1, 1], [2, 2, 1]]


def test_a_closed_flat_of_an_unfilled_dem_keeps_0():
    z = np.full((5, 5), 9.0, np.float32)
    z[1:4, 1:4] = 5
    code, d = fo.resolve_flats(z)
    assert (d[1:4, 1:4] == fo.INFINITE).all() and (code[1:4, 1:4] == 0).all()
    assert np.array_equal(code, ho.flow_direction(z))
    z[2, 2] = NAN                                                        # NaN stays NaN, and makes its neighbours rim cells
    code, d = fo.resolve_flats(z)
    assert np.isnan(code[2, 2]) and d[2, 2] == fo.INFINITE and (d[1:4, 1:4][~np.isnan(z[1:4, 1:4])] == 0).all()
    filled = fo.fill(np.where(np.isnan(z), 5, z).astype(np.float32))     # filled, the flat has the rim as its drain
    assert (filled == 9).all() and fo.drains(fo.resolve_flats(filled)[0], filled) == (0, 0, 0)


def test_elevations_are_compared_in_their_own_dtype():
    z = np.full((3, 5), 9.0, np.float64)
    z[1, :4] = [1.0, 1.0, 1.0 + 2.0 ** -40, 1.0]                         # equal as float32 only
    assert fo.resolve_flats(z)[1][1].tolist() == [0, 1, 0, fo.INFINITE, 0]            # (1, 2) has a lower neighbour: drained
    assert fo.resolve_flats(z.astype(np.float32))[1][1].tolist() == [0, 1, 2, 3, 0]


# ------------------------------------------------------------------ the two properties on the GPU test's rasters
@pytest.mark.parametrize("name", list(fo.cases(np.float32)))
def test_every_path_drains_and_no_cycle(name):
    z, filled, codes_unfilled, codes_filled = fo.expected(name, np.float32)
    _same(fo.fill_fixed_point(z)[0], filled)                             # the flood against the Jacobi form
    assert fo.drains(codes_filled, filled) == (0, 0, 0)
    ho.flow_accumulation(codes_unfilled)                                 # an unfilled raster: paths may end inside, none cycles
    ho.basins(codes_unfilled)
    plain = ho.flow_direction(z)
    drained = fo.drained_mask(z, plain)
    assert np.array_equal(codes_unfilled[drained], plain[drained])       # drained cells keep code0
    if name == "featured_129x257":
        rim = fo.rim_mask(filled)
        assert int(((plain == 0) & ~rim).sum()) == 842 and int(((codes_filled == 0) & ~rim).sum()) == 0
        assert np.nanmax(ho.flow_accumulation(codes_filled)) == 13385


def test_the_featured_rasters_are_what_their_names_say():
    w = fo.fill(fo.lake_four_tiles(np.float32))
    assert (w[1:-1, 1:-1] == 7).all() and fo.lake_four_tiles(np.float32).shape == (2 * fo.TILE + 2,) * 2
    z = fo.diagonal_pits(np.float32)
    w = fo.fill(z)
    assert w[fo.TILE - 1, fo.TILE - 1] == 3 == w[fo.TILE, fo.TILE] and (w >= z).all()
    z, length = fo.serpentine_corridor(np.float32)
    w, rounds = fo.fill_fixed_point(z)
    assert length == 8450 and int((w == 0).sum()) == length and rounds > 8000     # plain global rounds are not an option
    assert fo.resolve_flats(w)[1].max() > 8000
    z = fo.signed_zeros(np.float32)
    assert np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()


# ------------------------------------------------------------------ the package's host side
def test_fill_is_exported_and_the_constants_agree_with_the_header():
    import xrspatial_amd as xa
    from xrspatial_amd import hydrology
    assert xa.fill is hydrology.fill
    header = open(os.path.join(ROOT, "include", "xrs_hip.h")).read()
    value = lambda name: int(re.search(r"\b%s = (\d+)" % name, header).group(1))    # noqa: E731
    assert hydrology.TILE == fo.TILE == value("XRS_FILL_TILE")
    assert hydrology.FILL_STATUS_WORDS == value("XRS_FILL_STATUS_WORDS") and hydrology.FILL_STATUS_ROUNDS == value("XRS_FILL_STATUS_ROUNDS")
    assert hydrology.TIMED == value("XRS_FILL_TIMED")
    words = [0] * hydrology.FILL_STATUS_WORDS
    words[0], words[1], words[8], words[9], words[88], words[168] = 2, 13, 5, 0, 9, 777
    assert hydrology.relax_rounds(words) == {"rounds": 2, "tiles_launched": 13, "changed": [5, 0], "tiles": [9, 0], "ns": [777, 0]}


def test_argument_checks_come_before_device_work():
    import xrspatial_amd as xa
    for fn in (xa.fill, lambda a: xa.flow_direction(a, resolve_flats=True)):
        with pytest.raises(ValueError, match="2D"):
            fn(xa.DataArray(np.zeros((2, 3, 4), np.float32), dims=["b", "y", "x"]))
        with pytest.raises(TypeError, match="dtype"):
            fn(_agg(np.zeros((3, 4), np.complex64)))
    with pytest.raises(ValueError, match="cell size"):
        xa.flow_direction(_agg(np.zeros((3, 4), np.float32), res=(0.0, 1.0)), resolve_flats=True)


def test_dask_and_sharded_rasters_are_refused(monkeypatch):
    import xrspatial_amd as xa
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.zeros((8, 8), np.float32), (4, 4)))
    shard = object.__new__(xa.ShardedArray)                              # (its constructor wants a device; the refusal does not)
    shard.local = np.zeros((8, 8), np.float32)
    for fn in (xa.fill, lambda a: xa.flow_direction(a, resolve_flats=True)):
        with pytest.raises(NotImplementedError, match="dask"):
            fn(lazy)
        with pytest.raises(NotImplementedError, match="sharded"):
            fn(_agg(shard))


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xa
    if xa.has_hip():
        pytest.skip("a GPU is present")
    for dt in (np.float32, np.float64, np.int64, np.bool_):
        with pytest.raises(xa.XrsError):
            xa.fill(_agg(np.zeros((4, 4), dt)))
        with pytest.raises(xa.XrsError):
            xa.flow_direction(_agg(np.zeros((4, 4), dt)), resolve_flats=True)
    with xa.fuse():                                                      # eager inside a scope: the same error, at the call
        with pytest.raises(xa.XrsError):
            xa.fill(_agg(np.zeros((4, 4), np.float32)))
    with pytest.raises(xa.XrsError):
        xa.fill(xa.Dataset({"a": _agg(np.zeros((4, 4), np.float32))}))


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_fill / xrs_flow_flats validate on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    names = {"xrs_fill_workspace_size", "xrs_fill", "xrs_flow_flats_workspace_size", "xrs_flow_flats"}
    assert names <= set(_lib.EXPORTED)
    fake, other = ctypes.c_void_p(256), ctypes.c_void_p(4096)
    up = lambda v: (v + 255) // 256 * 256                                # noqa: E731
    head = (64 * 64 + 64) * 4                                            # the count slots, the round's total and four list lengths
    tiles = 5 * 7                                                        # 300 x 400 in tiles of 64
    size = _lib.workspace_bytes                                          # (the status-returning entries, the bytes through a pointer)
    assert size("fill", 300, 400) == head + 2 * up(tiles * 4) == 17152   # flags and lists
    assert size("flow_flats", 300, 400) == 17152 + up(300 * 400 * 4)     # and the step counts
    assert size("fill", 1, (1 << 32) - 2) == head + 2 * up((1 << 26) * 4)
    assert size("flow_flats", 1 << 16, (1 << 16) - 1) == head + 2 * up((1 << 20) * 4) + up(((1 << 32) - (1 << 16)) * 4)    # beyond 2^32 bytes
    for name in ("fill", "flow_flats"):
        for args in ((0, 5), (5, -1), (1 << 16, 1 << 16), (1, (1 << 32) - 1)):
            assert size(name, *args) == 0, args
        assert getattr(lib, f"xrs_{name}_workspace_size")(4, 5, None) != 0 and "null" in _lib.last_error()

    status = (ctypes.c_int64 * 256)()
    for fn in (lib.xrs_fill, lib.xrs_flow_flats):
        def call(z=fake, dtype=9, rows=4, cols=5, plane=other, work=other, st=status, flags=0):
            return fn(z, dtype, rows, cols, plane, work, st, flags, None)

        for kw, text in ((dict(rows=-1), "negative shape"), (dict(cols=-3), "negative shape"), (dict(dtype=4), "dtype"),
                         (dict(dtype=10), "dtype"), (dict(flags=2), "flags"), (dict(st=None), "null"), (dict(z=None), "null"),
                         (dict(plane=None), "null"), (dict(work=None), "null"), (dict(plane=fake), "overwrite"),
                         (dict(rows=1 << 16, cols=1 << 16), "2^32 - 2"), (dict(rows=1, cols=(1 << 32) - 1), "2^32 - 2")):
            assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
        status[0], status[255] = 7, 7
        assert call(rows=0, z=None, plane=None, work=None) == 0 and status[0] == 0 and status[255] == 0   # nothing to do; words cleared
        assert call(cols=0, dtype=8) == 0

"""CPU checks of flow_direction / flow_accumulation / basins.  The reference has no hydrology code, so there is
nothing to execute: the rule's NumPy statement (tests/hydrology_oracle.py) is pinned to small literals worked out by hand, the
kernels' doubling recurrence (as a NumPy model) is held against Kahn's order on the rasters the GPU test uses, with the round
counts those rasters are meant to reach, and the argument checks and refusals run before any device work."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import hydrology_oracle as ho

NAN = np.nan
RAMP_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 1025)


def _agg(z, res=(1.0, 1.0), **kw):
    import xrspatial_amd as xa
    return xa.DataArray(z, dims=["y", "x"], attrs={"res": res}, **kw)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want, got.dtype)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), (got, want)


# ------------------------------------------------------------------ flow_direction: the rule on literals
def test_pit_in_a_3x3_gives_all_eight_codes():
    z = [[1, 1, 1], [1, 0, 1], [1, 1, 1]]
    want = [[2, 4, 8], [1, 0, 16], [128, 64, 32]]
    for dt in (np.float32, np.float64, np.int16):
        got = ho.flow_direction(np.array(z, dt))
        assert got.dtype == np.float32
        _same(got, want)


def test_peak_in_a_3x3_prefers_the_steeper_diagonal():
    # the peak drops 1 to its four edge neighbours and 2 / sqrt(2) = 1.41 to its corners: SE, the first corner in the order
    _same(ho.flow_direction(np.array([[0, 1, 0], [1, 2, 1], [0, 1, 0]], np.float32)), [[0, 1, 0], [4, 2, 4], [0, 1, 0]])


def test_a_tie_between_e_and_se_gives_e():
    # cx = 3, cy = 4, diagonal exactly 5: E drops (10 - 7) / 3 = 1, SE (10 - 5) / 5 = 1
    z = np.array([[10, 7], [10, 5]], np.float64)
    assert ho.cell_distances(3, 4)[2] == 5.0
    _same(ho.flow_direction(z, 3, 4), [[1, 4], [1, 0]])
    _same(ho.flow_direction(z, -3, -4), [[1, 4], [1, 0]])                # |cell size|


def test_anisotropic_cells_change_the_steepest_neighbour():
    z = np.array([[10, 10, 10], [10, 10, 8], [10, 5, 10]], np.float32)
    assert ho.flow_direction(z, 1, 1)[1, 1] == 4                          # S drops 5, E 2
    assert ho.flow_direction(z, 1, 3)[1, 1] == 1                          # S drops 5 / 3, E 2


def test_flats_nan_and_infinities():
    _same(ho.flow_direction(np.full((3, 4), 7.0)), np.zeros((3, 4)))
    _same(ho.flow_direction(np.array([[5, NAN, 1]])), [[0, NAN, 0]])      # a NaN neighbour is never taken
    _same(ho.flow_direction(np.array([[5, NAN], [5, 1]])), [[2, NAN], [1, 0]])
    inf = np.inf
    _same(ho.flow_direction(np.array([[inf, inf, 1, -inf]])), [[0, 1, 1, 0]])   # inf - inf is not taken
    _same(ho.flow_direction(np.zeros((1, 1))), [[0]])
    assert ho.flow_direction(np.zeros((0, 5))).shape == (0, 5)


# ------------------------------------------------------------------ accumulation and basins: the rule on literals
def test_ramp_of_five():
    d = np.array([[1, 1, 1, 1, 0]], np.float32)
    _same(ho.flow_accumulation(d), [[1, 2, 3, 4, 5]])
    _same(ho.basins(d), [[4, 4, 4, 4, 4]])
    d = np.array([[16, 16, 16, 16, 16]], np.float32)                      # the first cell points out of the raster: an outlet
    _same(ho.flow_accumulation(d), [[5, 4, 3, 2, 1]])
    _same(ho.basins(d), [[0, 0, 0, 0, 0]])


def test_y_shaped_confluence():
    d = np.array([[2, 0, 8], [0, 4, 0], [0, 0, 0]], np.float32)
    _same(ho.flow_accumulation(d), [[1, 1, 1], [1, 3, 1], [1, 4, 1]])
    _same(ho.basins(d), [[7, 1, 7], [3, 7, 5], [6, 7, 8]])


def test_nan_cells_are_outside_the_graph():
    d = np.array([[1, NAN, 16], [64, 32, 64]], np.float32)               # (0, 0) and (0, 2) point into NaN: outlets
    _same(ho.flow_accumulation(d), [[3, NAN, 2], [1, 1, 1]])
    _same(ho.basins(d), [[0, NAN, 2], [0, 0, 2]])


def test_pit_cone_literal_through_both_stages():
    d = ho.flow_direction(np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], np.float32))
    _same(ho.flow_accumulation(d), [[1, 1, 1], [1, 9, 1], [1, 1, 1]])
    _same(ho.basins(d), np.full((3, 3), 4.0))


@pytest.mark.parametrize("d", [[[1, 16]], [[1, 4], [64, 16]]], ids=["two_cells", "four_cycle"])
def test_cycles_raise(d):
    d = np.array(d, np.float32)
    for fn in (ho.flow_accumulation, ho.basins, ho.doubling_model):
        with pytest.raises(ValueError, match="cycle"):
            fn(d)


def test_code_3_raises():
    for fn in (ho.flow_accumulation, ho.basins, ho.doubling_model):
        with pytest.raises(ValueError, match="code"):
            fn(np.array([[1, 3, 0]], np.float32))


# ------------------------------------------------------------------ the kernels' recurrence on the GPU test's rasters
def _model_equals_kahn(d):
    acc, bas, rounds = ho.doubling_model(d)
    _same(acc, ho.flow_accumulation(d))
    _same(bas, ho.basins(d))
    return acc, rounds


@pytest.mark.parametrize("n", RAMP_LENGTHS)
def test_model_on_ramps_reaches_every_round_count(n):
    for code in (1, 16):
        acc, rounds = _model_equals_kahn(ho.ramp(n, code))
        want = np.arange(1, n + 1, dtype=np.float64)
        _same(acc, [want if code == 1 else want[::-1]])
        # the longest path has n - 1 steps: rounds 0 .. floor(log2(n - 1)); one below n.bit_length() at a power of two only
        assert rounds == (n - 1).bit_length()
        assert rounds == n.bit_length() - (1 if n & (n - 1) == 0 else 0)


def test_model_on_the_serpentine_takes_12_rounds():
    d = ho.serpentine(33, 65)
    acc, rounds = _model_equals_kahn(d)
    assert rounds == 12 and acc.max() == 33 * 65 == 2145
    assert sorted(acc.ravel().tolist()) == list(range(1, 2146))           # one path through every cell


def test_model_on_the_fan_the_random_raster_and_all_zeros():
    fan = ho.flow_direction(ho.pit_cone(129, 257))
    acc, rounds = _model_equals_kahn(fan)
    assert acc.max() == 129 * 257 == 33153 and rounds == 8                # every cell drains to the centre
    d = ho.random_directions(129, 257, 5)
    acc, rounds = _model_equals_kahn(d)
    assert np.isnan(d).sum() > 500 and rounds >= 3
    acc, rounds = _model_equals_kahn(np.zeros((7, 9), np.float32))
    assert rounds == 0 and (acc == 1).all()


def test_a_cycle_trips_the_bit_length_bound():
    for d in (ho.ring(4, 5, 1, 1, 2, 2), ho.ring(80, 300, 3, 100, 70, 82), np.array([[1, 16]], np.float32)):
        with pytest.raises(ValueError, match="cycle"):
            ho.doubling_model(d)
    assert int((ho.ring(80, 300, 3, 100, 70, 82) != 0).sum()) == 300      # the GPU test's 300-cell cycle
    assert not (ho.break_cycles(ho.ring(80, 300, 3, 100, 70, 82)) == ho.ring(80, 300, 3, 100, 70, 82)).all()
    ho.flow_accumulation(ho.break_cycles(ho.ring(80, 300, 3, 100, 70, 82)))


# ------------------------------------------------------------------ the package's host side
def test_the_new_names_are_exported():
    import xrspatial_amd as xa
    from xrspatial_amd import hydrology
    assert xa.flow_direction is hydrology.flow_direction and xa.flow_accumulation is hydrology.flow_accumulation
    assert xa.basins is hydrology.basins
    assert hydrology.CODES == ho.CODES
    assert hydrology.cell_distances(_agg(np.zeros((2, 2)), res=(-3, 4))) == (3.0, 4.0, 5.0)


def test_argument_checks_come_before_device_work():
    import xrspatial_amd as xa
    fns = (xa.flow_direction, xa.flow_accumulation, xa.basins)
    for fn in fns:
        with pytest.raises(ValueError, match="2D"):
            fn(xa.DataArray(np.zeros((2, 3, 4), np.float32), dims=["b", "y", "x"]))
        with pytest.raises(TypeError, match="dtype"):
            fn(_agg(np.zeros((3, 4), np.complex64)))
    for res in ((0.0, 1.0), (1.0, 0.0), (np.inf, 1.0), (1e-200, 1e-200), (1e200, 1.0)):      # the last two: the diagonal is 0 / inf
        with pytest.raises(ValueError, match="cell size"):
            xa.flow_direction(_agg(np.zeros((3, 4), np.float32), res=res))


def test_dask_and_sharded_rasters_are_refused(monkeypatch):
    import xrspatial_amd as xa
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.zeros((8, 8), np.float32), (4, 4)))
    shard = object.__new__(xa.ShardedArray)                              # (its constructor wants a device; the refusal does not)
    shard.local = np.zeros((8, 8), np.float32)
    for fn in (xa.flow_direction, xa.flow_accumulation, xa.basins):
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
        for fn in (xa.flow_direction, xa.flow_accumulation, xa.basins):
            with pytest.raises(xa.XrsError):
                fn(_agg(np.zeros((4, 4), dt)))
    with xa.fuse():                                                      # eager inside a scope: the same error, at the call
        with pytest.raises(xa.XrsError):
            xa.flow_direction(_agg(np.zeros((4, 4), np.float32)))
    with pytest.raises(xa.XrsError):
        xa.flow_direction(xa.Dataset({"a": _agg(np.zeros((4, 4), np.float32))}))


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_flow_direction / xrs_flow_accumulate validate on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    assert {"xrs_flow_direction", "xrs_flow_workspace_bytes", "xrs_flow_accumulate"} <= set(_lib.EXPORTED)
    fake = ctypes.c_void_p(256)
    up = lambda v: (v + 255) // 256 * 256                                # noqa: E731
    plane = up(300 * 400 * 4)
    assert lib.xrs_flow_workspace_bytes(300, 400, 1) == 540928 + 5 * plane  # head, two pointer planes, the count and two increments
    assert lib.xrs_flow_workspace_bytes(300, 400, 2) == 540928 + 4 * plane  # head, two pointer planes, two root planes
    assert lib.xrs_flow_workspace_bytes(300, 400, 3) == 540928 + 7 * plane
    for args in ((0, 5, 3), (5, -1, 3), (5, 5, 0), (5, 5, 4), (1 << 16, 1 << 16, 3), (1, (1 << 32) - 1, 3)):
        assert lib.xrs_flow_workspace_bytes(*args) == 0, args
    assert lib.xrs_flow_workspace_bytes(1, (1 << 32) - 2, 2) == 540928 + 4 * up(((1 << 32) - 2) * 4)

    def direction(data=fake, dtype=9, rows=4, cols=5, cx=1.0, cy=1.0, dg=2.0 ** 0.5, out=fake):
        return lib.xrs_flow_direction(data, dtype, rows, cols, cx, cy, dg, out, None)

    nan = float("nan")
    for kw, text in ((dict(rows=-1), "negative shape"), (dict(dtype=4), "dtype"), (dict(dtype=10), "dtype"), (dict(cx=0.0), "positive"),
                     (dict(cy=-1.0), "positive"), (dict(dg=0.0), "positive"), (dict(cx=nan), "positive"), (dict(cy=float("inf")), "positive"),
                     (dict(data=None), "null"), (dict(out=None), "null"), (dict(cols=1 << 31), "too large"),
                     (dict(rows=1 << 30, cols=1 << 12), "too large")):
        assert direction(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    assert direction(rows=0) == 0 and direction(cols=0, data=None, out=None) == 0        # nothing to do

    status = (ctypes.c_int64 * 80)()

    def accumulate(d=fake, rows=4, cols=5, work=fake, acc=fake, basin=fake, st=status, flags=0):
        return lib.xrs_flow_accumulate(d, rows, cols, work, acc, basin, st, flags, None)

    for kw, text in ((dict(cols=-1), "negative shape"), (dict(flags=2), "flags"), (dict(st=None), "null"), (dict(d=None), "null"),
                     (dict(work=None), "null"), (dict(acc=None, basin=None), "no product"), (dict(rows=1 << 16, cols=1 << 16), "2^32 - 2"),
                     (dict(rows=1, cols=(1 << 32) - 1), "2^32 - 2")):
        assert accumulate(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    status[0] = 7
    assert accumulate(rows=0, d=None, work=None) == 0 and status[0] == 0                  # nothing to do; the words are cleared

"""bump on the MI355X against what the reference's own loop produced (tests/golden/bump_exec.npz) and, for live cases, against
the restated loop of tests/bump_oracle.py, which tests/test_bump_host.py pins to the same fixture.

Equality is exact: a cell that is NaN in one is NaN in the other (sign and payload of a NaN are free), every other cell has
identical bits, compared as uint64.  Nothing is tolerated: the kernel's arithmetic is the reference's, operation by operation.

The status words are deterministic -- a centre's value can be read only in a pass after the one that published it -- so events,
passes, chunks and touched cells are compared with the NumPy model of the scheme (bump_oracle.fold_model), which witnesses that
a case reached the path it is meant for: 301 passes for the forward chain, 2 for the reversed one, several chunks where the
capacity is forced down.

Shapes, the smallest at which each part can go wrong (the generator's): rasters of one cell, one row and one column; bumps on
every corner and edge of 9 x 7; a spread larger than the raster; 40 bumps on one cell with cancelling heights; chains of 300;
8 x 8 and 6 x 6 dense enough to reach 1e115 and to overflow; 130 x 70 and 257 x 33 (more than one workgroup of cells and of
events, widths that are no multiple of the wave) with spreads 1, 2, 3, 5, 9; spread 0 and -2; four height dtypes."""
import numpy as np
import pytest

from tests import bump_oracle as orc
from tests.golden import make_bump_exec as gen

pytestmark = pytest.mark.gpu

FIX = gen.load()
CASES = gen.names(FIX)
MODEL_EVENTS_MAX = 140_000          # the model is plain Python: the two largest seam cases are compared for their result alone
_model_status = {}


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def finish(xs, *args, **kw):
    return xs.bump.finish_bump(*args, **kw)


def model_status(name):
    if name not in _model_status:
        width, height, spread, locs, heights, _ = gen.case_of(FIX, name)
        _model_status[name] = orc.fold_model(width, height, locs, heights, spread)[1]
    return _model_status[name]


def assert_same(got, want, what=""):
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape, what
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{what}: NaN cells")
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got.view(np.uint64)[ok], want.view(np.uint64)[ok], err_msg=f"{what}: bits")


# ------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("name", CASES)
def test_finish_bump_equals_the_reference(xs, name):
    width, height, spread, locs, heights, want = gen.case_of(FIX, name)
    status = {}
    got = finish(xs, width, height, locs, heights, spread, status=status)
    print(name, status)
    assert_same(got, want, name)
    assert status["chunks"] == 1 and status["events"] >= len(heights)
    if status["events"] <= MODEL_EVENTS_MAX:
        model = model_status(name)
        assert {k: status[k] for k in model} == model, name


def test_the_overflowing_case_overflows_and_the_dense_one_does_not():
    assert not np.isfinite(FIX["dense_6x6_n8000_s3/out"]).all()
    dense = FIX["dense_8x8_n2000_s3/out"]
    assert np.isfinite(dense).all() and np.abs(dense).max() > 1e100
    for name in ("inf_height_7x7_s2", "overflow_7x7_s2"):
        out = FIX[f"{name}/out"]
        assert np.isinf(out).any() and np.isnan(out).any() and np.isfinite(out).any()


def test_chains_take_the_passes_their_depth_asks_for(xs):
    for name, check in (("chain_forward_300", lambda p: p >= 300 // 2), ("chain_reverse_300", lambda p: p <= 4)):
        width, height, spread, locs, heights, want = gen.case_of(FIX, name)
        status = {}
        assert_same(finish(xs, width, height, locs, heights, spread, status=status), want, name)
        print(name, status)
        assert check(status["passes"]), (name, status)


def test_order_on_one_cell(xs):
    width, height, spread, locs, heights, want = gen.case_of(FIX, "one_cell_5x5_s1")
    assert want[2, 2] != heights.sum()                                  # another order of the adds gives another centre
    assert_same(finish(xs, width, height, locs, heights, spread), want)


@pytest.mark.parametrize("max_events", [660, 11, 100])
def test_chunks_carry_the_state(xs, max_events):
    width, height, spread, locs, heights, want = gen.case_of(FIX, "r64x48_n307_s2")
    status = {}
    got = finish(xs, width, height, locs, heights, spread, max_events=max_events, status=status)
    print(max_events, status)
    assert status["chunks"] == -(-307 // (max_events // 11)) >= 5       # (a spread-2 bump has at most 11 events)
    assert_same(got, want)
    model = orc.fold_model(width, height, locs, heights, spread, max_events=max_events)[1]
    assert {k: status[k] for k in model} == model
    assert_same(got, finish(xs, width, height, locs, heights, spread))


def test_chunks_of_a_dense_raster(xs):
    """every chunk starts from what the chunks before it left on the raster: 2000 bumps on 8 x 8, 23 chunks"""
    width, height, spread, locs, heights, want = gen.case_of(FIX, "dense_8x8_n2000_s3")
    status = {}
    got = finish(xs, width, height, locs, heights, spread, max_events=27 * 90, status=status)
    assert status["chunks"] == 23
    assert_same(got, want)


# ------------------------------------------------------------------ live cases against the oracle
@pytest.mark.parametrize("spread", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("shape", [(130, 70), (257, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_seams(xs, shape, spread):
    width, height = shape
    rng = np.random.default_rng(1000 * width + spread)
    locs = np.stack([rng.integers(0, width, 2000), rng.integers(0, height, 2000)], axis=1).astype(np.uint16)
    heights = rng.normal(scale=2.0, size=2000)
    want = orc.finish_bump(width, height, locs, heights, spread)
    status = {}
    assert_same(finish(xs, width, height, locs, heights, spread, status=status), want)
    print(shape, spread, status)
    # ... and in several chunks, which end somewhere inside a workgroup of bumps
    bound = orc.footprint_bound(width, height, spread)
    assert_same(finish(xs, width, height, locs, heights, spread, max_events=bound * 300, status=status), want)
    assert status["chunks"] == 7


def test_spread_larger_than_the_raster(xs):
    rng = np.random.default_rng(5)
    for width, height, spread in ((3, 2, 40), (1, 1, 1000), (4, 6, 5000)):          # (5000: the bounding box stands for the disc)
        locs = np.stack([rng.integers(0, width, 12), rng.integers(0, height, 12)], axis=1).astype(np.uint16)
        heights = rng.normal(size=12)
        assert_same(finish(xs, width, height, locs, heights, spread), orc.finish_bump(width, height, locs, heights, spread))


def test_device_output_and_other_spellings_of_the_arguments(xs):
    width, height, spread, locs, heights, want = gen.case_of(FIX, "r37x29_n500_s3")
    dev = finish(xs, width, height, locs, heights, spread, device=True)
    assert isinstance(dev, xs.DeviceArray) and dev.shape == (height, width) and dev.dtype == np.float64
    assert_same(dev.get(), want)
    assert_same(finish(xs, np.int64(width), np.int32(height), locs.astype(np.int64), list(heights), np.int64(spread)), want)


def test_no_bumps(xs):
    got = finish(xs, 7, 3, np.empty((0, 2), np.uint16), np.empty(0), 2)
    assert got.shape == (3, 7) and got.dtype == np.float64 and not got.any()


def test_a_location_outside_the_raster_is_reported_not_written(xs):
    locs = np.array([[1, 1], [9, 2], [2, 2]], np.uint16)
    with pytest.raises(xs.XrsError, match="outside"):
        finish(xs, 9, 7, locs, np.ones(3), 2)
    with pytest.raises(xs.XrsError, match="outside"):
        finish(xs, 9, 7, locs[:, ::-1], np.ones(3), 0)
    # the next call is served as usual
    width, height, spread, locs, heights, want = gen.case_of(FIX, "border_9x7_s2")
    assert_same(finish(xs, width, height, locs, heights, spread), want)


def test_a_capacity_below_one_footprint_is_refused(xs):
    width, height, spread, locs, heights, _ = gen.case_of(FIX, "r64x48_n307_s2")
    with pytest.raises(xs.XrsError, match="capacity"):
        finish(xs, width, height, locs, heights, spread, max_events=10)


# ------------------------------------------------------------------ bump itself
def reference_draws(seed, width, height, count):
    """the locations of the reference's two draws for this seed, and NumPy's global state after them"""
    np.random.seed(seed)
    locs = np.empty((count, 2), dtype=np.uint16)
    locs[:, 0] = np.random.choice(range(width), count)
    locs[:, 1] = np.random.choice(range(height), count)
    return locs, np.random.get_state()


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("seed", [0, 7, 2024])
def test_bump_draws_what_the_reference_draws(xs, seed):
    locs, state = reference_draws(seed, 20, 20, 40)
    np.random.seed(seed)
    agg = xs.bump(20, 20)
    assert same_state(np.random.get_state(), state)
    assert isinstance(agg, xs.DataArray) and list(agg.dims) == ['y', 'x'] and dict(agg.attrs) == {'res': 1}
    assert isinstance(agg.data, np.ndarray)
    assert_same(agg.data, orc.finish_bump(20, 20, locs, np.ones(40), 1))
    assert agg.data.any()


def test_bump_hands_the_locations_to_the_height_function(xs):
    locs, state = reference_draws(3, 31, 17, 25)
    seen = []

    def heights(bumps):
        seen.append(bumps)
        return (np.arange(len(bumps)) % 5).astype(np.uint16)

    np.random.seed(3)
    agg = xs.bump(31, 17, count=25, height_func=heights, spread=3)
    assert same_state(np.random.get_state(), state)
    assert len(seen) == 1 and seen[0].dtype == np.uint16 and seen[0].shape == (25, 2)
    np.testing.assert_array_equal(seen[0], locs)
    assert agg.shape == (17, 31)
    assert_same(agg.data, orc.finish_bump(31, 17, locs, np.arange(25) % 5, 3))


def test_bump_wraps_locations_beyond_uint16_as_the_reference_does(xs):
    locs, _ = reference_draws(11, 70000, 2, 64)
    np.random.seed(11)
    drawn = np.random.choice(range(70000), 64)
    assert (drawn > 65535).any() and np.array_equal(locs[:, 0], drawn % 65536)
    np.random.seed(11)
    agg = xs.bump(70000, 2, count=64, spread=2)
    assert_same(agg.data, orc.finish_bump(70000, 2, locs, np.ones(64), 2))


def test_bump_refuses_heights_that_do_not_fit(xs):
    with pytest.raises(ValueError):
        xs.bump(8, 8, count=5, height_func=lambda b: np.ones(4))
    with pytest.raises(ValueError):
        xs.bump(8, 8, count=5, height_func=lambda b: ["a"] * 5)

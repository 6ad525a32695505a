"""zonal.regions on the MI355X: bit for bit against the reference's own outputs (tests/golden/regions_exec.npz), against
the restatement of DESIGN.md §6b (tests/regions_oracle.py) where the reference cannot be run (float32, large rasters),
and on the shapes that stress the tile seams of csrc/regions.hip."""
import numpy as np
import pytest

from tests import regions_oracle as ro
from tests.golden import make_regions_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = gen.case_names(FIXTURE)


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xs, a, **kw):
    return xs.DataArray(a, dims=["y", "x"], **kw)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if want.dtype.kind == "f":                    # bit for bit, NaN payloads included
        iv = np.dtype("u%d" % want.dtype.itemsize)
        assert np.array_equal(got.view(iv), want.view(iv))
    else:
        assert np.array_equal(got, want)


def _labels(xs, a, n):
    return np.asarray(xs.regions(_agg(xs, a), neighborhood=n).data)


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("case", CASES)
def test_equals_the_reference(xs, case, n):
    a = FIXTURE[f"{case}/in"]
    _same(_labels(xs, a, n), FIXTURE[f"{case}/n{n}"])


def _check_restated(xs, a, n, typing="numba"):
    lab, _ = ro.restated(a, n, typing)
    _same(_labels(xs, a, n), ro.as_output(lab, a))


def _typing_pairs():
    from tests.test_regions_host import TYPING_PAIRS
    return TYPING_PAIRS


@pytest.mark.parametrize("n", [4, 8])
def test_float32_follows_the_numba_typing(xs, n):
    rng = np.random.default_rng(5)
    for v, w in _typing_pairs():
        _check_restated(xs, np.array([[v, w]], np.float32), n)
        a = np.full((5, 70), v, np.float32)                  # the pair at a tile seam (column 63 | 64)
        a[2, 64] = w
        a[rng.random(a.shape) < 0.3] = w
        _check_restated(xs, a, n)
    for shape in ((9, 13), (40, 70), (33, 129)):
        base = np.float32(rng.choice([1000.0, -3.0, 7470.702]))
        t = np.float32(1e-05 * abs(float(base)) + 1e-08)
        a = (base + rng.integers(-2, 3, shape) * t * np.float32(rng.choice([0.5, 0.999, 1.0, 1.001]))).astype(np.float32)
        a[rng.random(shape) < 0.05] = np.nan
        _check_restated(xs, a, n)


@pytest.mark.parametrize("n", [4, 8])
def test_seeded_random_against_the_restatement(xs, n):
    rng = np.random.default_rng(100 + n)
    dtypes = (np.float64, np.float32, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)
    for t in range(30):
        dt = dtypes[t % len(dtypes)]
        shape = tuple(int(s) for s in rng.integers(1, 80, 2))
        if np.dtype(dt).kind == "f":
            a = rng.choice(np.array([0.0, -0.0, 1.0, 1.000005, np.inf, -np.inf, np.nan, 2.0]), shape).astype(dt)
        else:
            info = np.iinfo(dt)
            a = rng.choice(np.array([info.min, info.max, 0, 1, 2], dtype=dt), shape)
        if np.dtype(dt).itemsize == 1:
            a = a[:11, :11]                                  # within the 8-bit label limits
        _check_restated(xs, a, n)


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("shape", [(200, 300), (1000, 777), (65, 129), (1, 5000), (5000, 1), (3, 2000), (2000, 3),
                                   (97, 64), (32, 65)])
def test_many_tiles_against_the_fast_oracle(xs, shape, n):
    rng = np.random.default_rng(shape[0] * 7 + shape[1] + n)
    a = (rng.random(shape) < 0.55).astype(np.float64) + (rng.random(shape) < 0.2)
    a[rng.random(shape) < 0.02] = np.nan
    lab, _ = ro.fast_exact(a, n)
    _same(_labels(xs, a, n), ro.as_output(lab, a))
    ai = np.nan_to_num(a, nan=7).astype(np.int32)
    lab, _ = ro.fast_exact(ai, n)
    _same(_labels(xs, ai, n), ro.as_output(lab, ai))


def _serpentine(rows, cols):
    """1 on a path that fills every even row and turns at alternate ends through the odd rows; 0 elsewhere"""
    a = np.zeros((rows, cols), np.float32)
    a[0::2, :] = 1
    a[1::4, -1] = 1
    a[3::4, 0] = 1
    return a


@pytest.mark.parametrize("n", [4, 8])
def test_serpentine_threads_every_tile(xs, n):
    a = _serpentine(1027, 1000)
    out = _labels(xs, a, n)
    assert np.all(out[a == 1] == 1)                          # one region through every tile
    lab, _ = ro.fast_exact(a, n)
    _same(out, ro.as_output(lab, a))
    b = _serpentine(999, 70).T.copy()                        # and column-wise
    lab, _ = ro.fast_exact(b, n)
    _same(_labels(xs, b, n), ro.as_output(lab, b))


def _checker(rows, cols, dtype):
    y, x = np.mgrid[0:rows, 0:cols]
    return ((x + y) % 2).astype(dtype)


def test_checkerboards(xs):
    a = _checker(100, 130, np.float32)
    out8 = _labels(xs, a, 8)
    assert np.array_equal(out8, np.where(a == 0, 1, 2).astype(np.float32))
    out4 = _labels(xs, a, 4)
    assert np.array_equal(out4, np.arange(1, a.size + 1, dtype=np.float32).reshape(a.shape))


def test_all_nan_and_all_equal(xs):
    a = np.full((70, 90), np.nan)
    a.view(np.uint64)[3, 5] |= 1                             # a NaN payload survives
    for n in (4, 8):
        _same(_labels(xs, a, n), a)
        for dt in (np.float32, np.int8, np.uint64):
            b = np.full((70, 90), 3, dt)
            _same(_labels(xs, b, n), np.ones_like(b))


def test_every_cell_distinct_float64_4096(xs):
    rows = cols = 4096
    i = np.arange(rows * cols, dtype=np.float64)
    sign = np.where((np.arange(rows)[:, None] + np.arange(cols)[None, :]) % 2 == 0, 1.0, -1.0).reshape(-1)
    a = (i * sign).reshape(rows, cols)                       # every neighbour far outside the tolerance
    want = (i + 1).reshape(rows, cols)
    for n in (4, 8):
        assert np.array_equal(_labels(xs, a, n), want)


def test_refusal_at_the_label_limit(xs):
    ok = _labels(xs, _checker(15, 17, np.uint8), 4)          # 255 regions: the last label uint8 holds
    assert ok.max() == 255 and ok.dtype == np.uint8
    with pytest.raises(ValueError, match=r"up to 256, .*uint8.*uint16"):
        xs.regions(_agg(xs, _checker(16, 16, np.uint8)), neighborhood=4)
    with pytest.raises(ValueError, match=r"up to 128, .*int8.*int16"):
        xs.regions(_agg(xs, _checker(8, 16, np.int8)), neighborhood=4)
    assert _labels(xs, _checker(8, 16, np.int8), 8).max() == 2
    dev = xs.DeviceArray.from_numpy(_checker(4096, 4096, np.float32))
    out = xs.regions(_agg(xs, dev), neighborhood=4).data.get()
    assert out[-1, -1] == 2.0 ** 24 and out[0, 0] == 1.0
    with pytest.raises(ValueError, match=r"up to 16781312, .*float32.*float64"):
        xs.regions(_agg(xs, xs.DeviceArray.from_numpy(_checker(4097, 4096, np.float32))), neighborhood=4)


def test_device_array_in_and_out_keeps_metadata(xs):
    a = FIXTURE["shape_4/in"]
    coords = {"y": np.arange(a.shape[0]) * 2.0, "x": np.arange(a.shape[1]) * 3.0}
    agg = xs.DataArray(xs.DeviceArray.from_numpy(a), dims=["lat", "lon"], coords={"lat": coords["y"], "lon": coords["x"]},
                       attrs={"res": (2.0, 3.0), "crs": "EPSG:4326"}, name="dem")
    out = xs.regions(agg, neighborhood=8, name="patches")
    assert isinstance(out.data, xs.DeviceArray)
    assert out.name == "patches" and out.dims == ("lat", "lon") and out.attrs == agg.attrs
    assert np.array_equal(np.asarray(out["lat"]), coords["y"])
    _same(out.data.get(), FIXTURE["shape_4/n8"])
    assert xs.regions(_agg(xs, a)).name == "regions"


def test_two_runs_are_identical(xs):
    rng = np.random.default_rng(3)
    a = (rng.random((777, 1111)) < 0.5).astype(np.uint32) * 3
    for n in (4, 8):
        assert np.array_equal(_labels(xs, a, n), _labels(xs, a, n))


def test_sharded_raster_is_refused(xs):
    from xrspatial_amd import ShardedArray
    sh = ShardedArray(8, 8, np.float32)
    with pytest.raises(NotImplementedError, match="sharded"):
        xs.regions(xs.DataArray(sh, dims=["y", "x"]))


def test_patch_statistics_pipeline(xs):
    rng = np.random.default_rng(9)
    cls = rng.integers(0, 4, (300, 410)).astype(np.int32)
    cls = np.repeat(np.repeat(cls[::6, ::5], 6, axis=0), 5, axis=1)[:300, :410]
    values = rng.normal(100, 10, cls.shape)
    patches = xs.regions(_agg(xs, cls), neighborhood=8)
    lab, _ = ro.fast_exact(cls, 8)
    want_lab = ro.as_output(lab, cls)
    _same(np.asarray(patches.data), want_lab)
    got = xs.zonal_stats(patches, _agg(xs, values), stats_funcs=["mean", "count", "max"])
    want = xs.zonal_stats(_agg(xs, want_lab), _agg(xs, values), stats_funcs=["mean", "count", "max"])
    import pandas as pd
    pd.testing.assert_frame_equal(got, want, check_exact=False, rtol=1e-12)   # (float sums: atomics, any order)
    assert len(got) == len(np.unique(want_lab))


@pytest.mark.parametrize("n", [4, 8])
def test_threshold_is_multiply_then_add(xs, n):
    """pairs on which a fused multiply-add threshold would join what the reference keeps apart, or the reverse"""
    for v, w in ro.fma_sensitive_pairs():
        a = np.array([[v, w]])
        _check_restated(xs, a, n)
        b = np.full((3, 66), v)                              # at the 63 | 64 tile seam, and inside a tile
        b[1, 64] = w
        b[2, 10] = w
        _check_restated(xs, b, n)

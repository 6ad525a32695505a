"""idw on the MI355X, bit for bit against the written rule (tests/idw_oracle.py): the result and both neighbour
planes, with tolerance 0, at three bin sizes (1 cell, the planned one, one bin over the whole raster) that must agree with each
other.  The cases are the smallest that reach each path of csrc/idw.hip: tiles and waves cut on both axes, every capacity tier
of the k-best list at its last k and the next one, rings that grow to the whole grid, the apron, a bin of more than one staging
chunk, exact ties by the thousand, the radius at an exact d2, every power, values whose order of summation shows, and the three
entries at the C ABI.  Every comparison records its cell count (tests/parity_log.py)."""
import ctypes

import numpy as np
import pytest

from tests import idw_oracle as io
from tests import parity_log
from tests.golden import make_idw_witness as wit

pytestmark = pytest.mark.gpu

TIER_KS = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64)                  # capacities 1, 4, 8, 16 (registers), 32, 64 (LDS)


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _like(xs, shape):
    return xs.DataArray(np.zeros(shape, np.float32), dims=["y", "x"])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(config, op, got, want):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (config, op, got.dtype, want.dtype, got.shape, want.shape)
    parity_log.record(config, op, got, want, tol=0)
    ok = (_bits(got) == _bits(want)) | ((got != got) & (want != want))
    assert ok.all(), (config, op, np.argwhere(~ok)[:5].tolist(), got[~ok][:5].tolist(), want[~ok][:5].tolist())


def _bin_sizes(xs, shape):
    return (1, None, xs.idw.plan_bins(0, *shape))                # one cell, the plan, one bin over the whole raster


def _check(xs, config, points, values, shape, k, planes=True, **kw):
    """idw and neighbors at the three bin sizes against the oracle; returns the oracle's result."""
    points, values = np.asarray(points, np.float64).reshape(-1, 2), np.asarray(values, np.float64)
    want = io.idw(points, values, shape, k=k, **kw)
    radius = {key: kw[key] for key in ("max_distance", "transform") if key in kw}
    kept = points[~np.isnan(values)]
    want_index, want_d2 = io.neighbors(kept, shape, k, **radius)
    for b in _bin_sizes(xs, shape):
        stats = {}
        got = xs.idw(points, values, _like(xs, shape), k=k, bin_cells=b, stats=stats, **kw)
        assert stats["points"] == len(kept) and stats["bin_cells"] == (b or xs.idw.plan_bins(len(kept), *shape))
        _same(f"{config}_b{b}", "idw", got.data, want)
        if planes:
            index, d2 = xs.idw.neighbors(kept, _like(xs, shape), k=k, bin_cells=b, **radius)
            _same(f"{config}_b{b}", "idw_index", index, want_index)
            _same(f"{config}_b{b}", "idw_d2", d2, want_d2)
    return want


def _scatter(seed, n, shape, margin=4.0):
    rng = np.random.default_rng(seed)
    rows, cols = shape
    pts = np.stack([rng.uniform(-margin, cols + margin, n), rng.uniform(-margin, rows + margin, n)], axis=1)
    return pts, rng.normal(100.0, 30.0, n)


# ------------------------------------------------------------------ tiles and waves cut on both axes
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (17, 33), (33, 17)])
def test_shapes(xs, shape):
    pts, vals = _scatter(sum(shape), 60, shape)
    _check(xs, f"shape_{shape[0]}x{shape[1]}", pts, vals, shape, k=6)


# ------------------------------------------------------------------ the capacity tiers of the k-best list
@pytest.mark.parametrize("k", TIER_KS)
def test_k_tiers(xs, k):
    shape = (17, 33)
    pts, vals = _scatter(k, 150, shape)
    _check(xs, f"k{k}", pts, vals, shape, k=k)


def test_k_greater_than_n(xs):
    pts, vals = _scatter(3, 5, (9, 20))
    for k in (12, 40):
        want = _check(xs, f"k{k}_of_5", pts, vals, (9, 20), k=k)
        assert np.isfinite(want).all()
    _check(xs, "k12_of_5_min_points_6", pts, vals, (9, 20), k=12, min_points=6, fill=-1.0)      # never enough: all fill


# ------------------------------------------------------------------ rings that grow to the whole grid
def test_no_points_and_one_point_in_the_far_apron(xs):
    want = _check(xs, "n0", np.empty((0, 2)), np.empty(0), (20, 35), k=3, fill=-5.0)
    assert np.all(want == -5.0)
    want = _check(xs, "all_nan_values", [[1.0, 2.0], [3.0, 4.0]], [np.nan, np.nan], (20, 35), k=3)
    assert np.isnan(want).all()
    want = _check(xs, "far_corner", [[75.5, 80.25]], [8.0], (70, 70), k=4)
    assert np.all(want == 8.0)
    # empty rectangles of more bin rows than a workgroup has threads (256, and 128 for k > 32), skipped in one step
    far = [[1.25, 299.5], [0.5, 298.0], [7.0, 330.0]]
    for k in (2, 40):
        _check(xs, f"tall_empty_k{k}", far, [1.0, 2.0, 4.0], (300, 2), k=k)
        _check(xs, f"tall_empty_radius_k{k}", far, [1.0, 2.0, 4.0], (300, 2), k=k, max_distance=40.0, fill=0.0)


def test_all_points_outside(xs):
    shape = (40, 30)
    rng = np.random.default_rng(5)
    left = np.stack([rng.uniform(-20.0, -0.01, 80), rng.uniform(-5.0, 45.0, 80)], axis=1)
    _check(xs, "outside_left", left, rng.normal(0, 1, 80), shape, k=7)
    t = rng.uniform(0, 2 * np.pi, 120)
    around = np.stack([15.0 + 40.0 * np.cos(t), 20.0 + 45.0 * np.sin(t)], axis=1)
    _check(xs, "outside_around", around, rng.normal(0, 1, 120), shape, k=7)
    _check(xs, "outside_around_radius", around, rng.normal(0, 1, 120), shape, k=7, max_distance=30.0, min_points=2)


def test_one_bin_of_more_than_a_staging_chunk(xs):
    rng = np.random.default_rng(6)
    pts = np.stack([rng.uniform(8.0, 9.0, 700), rng.uniform(11.0, 12.0, 700)], axis=1)      # one cell: one bin at every size
    for k in (12, 64):
        _check(xs, f"one_bin_k{k}", pts, rng.normal(5, 1, 700), (20, 24), k=k)


# ------------------------------------------------------------------ exact ties
def test_lattices_and_duplicates(xs):
    shape = (12, 20)
    jj, ii = np.mgrid[0:12, 0:20]
    rng = np.random.default_rng(7)
    centres = np.stack([ii.ravel() + 0.5, jj.ravel() + 0.5], axis=1)
    corners = np.stack([ii.ravel() + 0.0, jj.ravel() + 0.0], axis=1)
    for name, pts in (("centres", centres), ("corners", corners)):
        order = rng.permutation(len(pts))                         # the index, not the position, breaks the ties
        vals = rng.normal(10, 3, len(pts))
        want = _check(xs, f"lattice_{name}", pts[order], vals, shape, k=9)
        if name == "centres":
            got_first = vals[np.argsort(order)].reshape(shape)    # every centre holds a point: its value
            assert np.array_equal(want, got_first)
        _check(xs, f"lattice_{name}_k1", pts[order], vals, shape, k=1)
    twice = np.concatenate([centres[::3], centres[::3], corners[::5]])
    _check(xs, "duplicates", twice, rng.normal(10, 3, len(twice)), shape, k=5)
    _check(xs, "duplicates_k20", twice, rng.normal(10, 3, len(twice)), shape, k=20, power=3)


# ------------------------------------------------------------------ the radius
def test_max_distance(xs):
    shape = (24, 40)
    pts, vals = _scatter(8, 40, shape)
    far = pts + np.array([100.0, 0.0])
    want = _check(xs, "radius_none_in_reach", far, vals, shape, k=4, max_distance=50.0, fill=-2.0)
    assert np.all(want == -2.0)
    jj, ii = np.mgrid[0:8, 0:14]
    lattice = np.stack([3.0 * ii.ravel() + 0.5, 3.0 * jj.ravel() + 0.5], axis=1)       # centres 3 cells apart: d2 == 9 exactly
    lv = np.arange(len(lattice), dtype=np.float64)
    want = _check(xs, "radius_at_a_d2", lattice, lv, shape, k=6, max_distance=3.0)
    index, _ = io.neighbors(lattice, shape, 6, 3.0)
    assert (index[1:5, 3, 3] >= 0).all() and index[5, 3, 3] == -1                      # the four at distance 3 are in
    _check(xs, "radius_below_a_d2", lattice, lv, shape, k=6, max_distance=np.nextafter(3.0, 0))
    for mp in (1, 5):
        want = _check(xs, f"radius_short_min{mp}", pts, vals, shape, k=5, max_distance=6.0, min_points=mp, fill=-9.0)
        assert np.any(want == -9.0) and np.any(want != -9.0)
    short, _ = io.neighbors(pts, shape, 5, 6.0)
    assert np.any((short[0] >= 0) & (short[4] < 0))                                    # some cells have some, not all five


# ------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize("power", range(1, 9))
def test_powers(xs, power):
    shape = (17, 33)
    pts, vals = _scatter(40 + power, 90, shape)
    pts[:6] = np.floor(pts[:6]) + 0.5                            # some on cell centres: d2 == 0
    _check(xs, f"power{power}", pts, vals, shape, k=12, power=power, planes=False)


def test_values_whose_summation_order_shows(xs):
    shape = (17, 33)
    pts, _ = _scatter(9, 120, shape)
    rng = np.random.default_rng(9)
    vals = rng.choice([-1.0, 1.0], 120) * 10.0 ** rng.uniform(-300, 300, 120)
    for k, power in ((12, 2), (33, 1), (64, 3)):
        want = _check(xs, f"wide_values_k{k}_p{power}", pts, vals, shape, k=k, power=power, planes=False)
        assert np.isfinite(want).all()
    # the sums are not symmetric in the neighbours: another order gives other bits somewhere
    index, d2 = io.neighbors(pts, shape, 12)
    w = io.weight(d2.reshape(12, -1), 2)
    v = vals[index.reshape(12, -1)]
    rev = sum((w[r] * v[r] for r in reversed(range(12))), np.zeros(w.shape[1])) / sum((w[r] for r in reversed(range(12))), np.zeros(w.shape[1]))
    assert np.any(rev != io.idw(pts, vals, shape, k=12).ravel())


def test_dtypes_backends_and_names(xs):
    shape = (33, 65)
    pts, vals = _scatter(10, 200, shape)
    vals[::17] = np.nan
    for dtype in (np.float64, np.float32):
        want = _check(xs, f"dtype_{np.dtype(dtype).name}", pts, vals, shape, k=12, dtype=dtype, planes=False)
        assert want.dtype == dtype
    want = io.idw(pts, vals, shape, k=12)
    kept = pts[~np.isnan(vals)]
    dev_like = xs.DataArray(xs.DeviceArray.from_numpy(np.zeros(shape, np.uint8)), dims=["lat", "lon"], attrs={"res": 2})
    got = xs.idw(pts, vals, dev_like, name="rain")
    assert isinstance(got.data, xs.DeviceArray) and got.dims == ("lat", "lon") and got.attrs == {"res": 2} and got.name == "rain"
    _same("device_like", "idw", got.data.get(), want)
    index, d2 = xs.idw.neighbors(kept, dev_like, k=3)
    assert isinstance(index, xs.DeviceArray) and isinstance(d2, xs.DeviceArray)
    want_index, want_d2 = io.neighbors(kept, shape, 3)
    _same("device_like", "idw_index", index.get(), want_index)
    _same("device_like", "idw_d2", d2.get(), want_d2)
    host = xs.idw(pts, vals, _like(xs, shape))
    assert isinstance(host.data, np.ndarray) and host.name == "idw"
    _same("host_like", "idw", host.data, want)
    _same("two_runs", "idw", xs.idw(pts, vals, _like(xs, shape)).data, host.data)
    with pytest.raises(NotImplementedError, match="idw\\(\\) does not support row-sharded"):
        xs.idw(pts, vals, xs.DataArray(xs.ShardedArray(8, 8, np.float32), dims=["y", "x"]))
    huge = np.array([[1e308, 0.0], [3.0, 4.0]])                   # finite as given, not after the transform
    with pytest.raises(ValueError, match="not finite"):
        xs.idw(huge, [1.0, 2.0], _like(xs, shape), transform=(1e-3, 0.0, -1e308, 0.0, 1e-3, 0.0))


def test_transform_with_a_negative_dy_and_a_world_radius(xs):
    shape = (23, 31)
    T = (25.0, 0.0, 300.0, 0.0, -25.0, 5000.0)
    pts, vals = _scatter(11, 70, shape)
    world = np.stack([T[0] * pts[:, 0] + T[2], T[4] * pts[:, 1] + T[5]], axis=1)
    _check(xs, "transform", world, vals, shape, k=8, transform=T)
    want = _check(xs, "transform_world_radius", world, vals, shape, k=8, transform=T, max_distance=125.0, min_points=2)
    assert np.isnan(want).any() and np.isfinite(want).any()
    like = xs.DataArray(np.zeros(shape, np.int16), dims=["y", "x"], coords={"y": 5000.0 - 12.5 - 25.0 * np.arange(23), "x": 300.0 + 12.5 + 25.0 * np.arange(31)})
    assert xs.transform_from_coords(like) == T
    got = xs.idw(world, vals, like, k=8, transform=xs.transform_from_coords(like))
    _same("transform_from_coords", "idw", got.data, io.idw(world, vals, shape, k=8, transform=T))
    assert np.array_equal(got.coords["y"].values, like.coords["y"].values)


# ------------------------------------------------------------------ the independent witness
def test_witness_cases_on_the_gpu(xs):
    for i, points, shape, k, radius, want in wit.cases(wit.load()):
        for b in _bin_sizes(xs, shape):
            index, _ = xs.idw.neighbors(points, _like(xs, shape), k=k, max_distance=radius, bin_cells=b)
            _same(f"witness_{i}_b{b}", "idw_index_vs_ckdtree", index, want)


# ------------------------------------------------------------------ at the C ABI
def test_abi_calls_and_refusals(xs):
    from xrspatial_amd import _lib
    lib = _lib.load()
    shape = rows, cols = (33, 47)
    pts, vals = _scatter(12, 300, shape)
    n, B, k = len(pts), 4, 10
    size = ctypes.c_uint64(0)
    _lib.call("xrs_idw_workspace_size", n, rows, cols, B, ctypes.byref(size))
    assert size.value > n * 20 and size.value % 256 == 0
    work = xs.DeviceArray((size.value,), np.uint8)
    dev_pts, dev_vals = xs.DeviceArray.from_numpy(pts), xs.DeviceArray.from_numpy(vals)
    flags = ctypes.c_int(-1)
    _lib.call("xrs_idw_bin", dev_pts.ptr, n, rows, cols, B, None, work.ptr, ctypes.byref(flags), None)
    assert flags.value == 0
    out32, out64 = xs.DeviceArray(shape, np.float32), xs.DeviceArray(shape, np.float64)
    index, d2 = xs.DeviceArray((k,) + shape, np.int32), xs.DeviceArray((k,) + shape, np.float64)
    md2 = 7.5 * 7.5
    _lib.call("xrs_idw_search", work.ptr, dev_vals.ptr, n, rows, cols, B, k, 3, md2, 2, -1.0, 9, out32.ptr, index.ptr, d2.ptr, None)
    _lib.call("xrs_idw_search", work.ptr, dev_vals.ptr, n, rows, cols, B, k, 3, -1.0, 1, -1.0, 8, out64.ptr, None, None, None)
    _lib.call("xrs_device_sync")
    _same("abi", "idw", out32.get(), io.idw(pts, vals, shape, k=k, power=3, max_distance=7.5, min_points=2, fill=-1.0, dtype=np.float32))
    _same("abi", "idw", out64.get(), io.idw(pts, vals, shape, k=k, power=3, fill=-1.0))
    want_index, want_d2 = io.neighbors(pts, shape, k, 7.5)
    _same("abi", "idw_index", index.get(), want_index)
    _same("abi", "idw_d2", d2.get(), want_d2)
    # a coordinate that is not finite raises the flag
    bad = pts.copy()
    bad[17, 1] = np.nan
    _lib.call("xrs_idw_bin", xs.DeviceArray.from_numpy(bad).ptr, n, rows, cols, B, None, work.ptr, ctypes.byref(flags), None)
    assert flags.value == 1
    # refused before any launch
    search = (work.ptr, dev_vals.ptr, n, rows, cols, B)
    tail = (out64.ptr, None, None, None)
    refusals = [
        (lambda: lib.xrs_idw_workspace_size(n, rows, cols, B, None), "null pointer"),
        (lambda: lib.xrs_idw_workspace_size(n, rows, cols, 3, ctypes.byref(size)), "not a power of two"),
        (lambda: lib.xrs_idw_workspace_size(n, 0, cols, B, ctypes.byref(size)), "at least \\(1, 1\\)"),
        (lambda: lib.xrs_idw_workspace_size(n, 2**17, 2**15, 64, ctypes.byref(size)), "exceed the 32-bit cell index"),
        (lambda: lib.xrs_idw_workspace_size(2**31, rows, cols, B, ctypes.byref(size)), "points, more than"),
        (lambda: lib.xrs_idw_workspace_size(n, 2**15, 2**15, 1, ctypes.byref(size)), "use larger bins"),
        (lambda: lib.xrs_idw_bin(None, n, rows, cols, B, None, work.ptr, ctypes.byref(flags), None), "null pointer"),
        (lambda: lib.xrs_idw_bin(dev_pts.ptr, n, rows, cols, B, None, None, ctypes.byref(flags), None), "null pointer"),
        (lambda: lib.xrs_idw_bin(dev_pts.ptr, n, rows, cols, B, None, work.ptr, None, None), "null pointer"),
        (lambda: lib.xrs_idw_bin(dev_pts.ptr, n, rows, cols, 0, None, work.ptr, ctypes.byref(flags), None), "not a power of two"),
        (lambda: lib.xrs_idw_search(*search, 0, 2, -1.0, 1, 0.0, 8, *tail), "k 0 outside"),
        (lambda: lib.xrs_idw_search(*search, 65, 2, -1.0, 1, 0.0, 8, *tail), "k 65 outside"),
        (lambda: lib.xrs_idw_search(*search, k, 0, -1.0, 1, 0.0, 8, *tail), "power 0 outside"),
        (lambda: lib.xrs_idw_search(*search, k, 9, -1.0, 1, 0.0, 8, *tail), "power 9 outside"),
        (lambda: lib.xrs_idw_search(*search, k, 2, -1.0, k + 1, 0.0, 8, *tail), "min_points"),
        (lambda: lib.xrs_idw_search(*search, k, 2, float("nan"), 1, 0.0, 8, *tail), "max_d2 is NaN"),
        (lambda: lib.xrs_idw_search(*search, k, 2, -1.0, 1, 0.0, 4, *tail), "dtype code 4"),
        (lambda: lib.xrs_idw_search(*search, k, 2, -1.0, 1, 0.0, 8, None, None, None, None), "null pointer"),
        (lambda: lib.xrs_idw_search(None, dev_vals.ptr, n, rows, cols, B, k, 2, -1.0, 1, 0.0, 8, *tail), "null pointer"),
        (lambda: lib.xrs_idw_search(work.ptr, None, n, rows, cols, B, k, 2, -1.0, 1, 0.0, 8, *tail), "null pointer"),
    ]
    import re
    for call, text in refusals:
        assert call() != 0
        assert re.search(text, _lib.last_error()), (text, _lib.last_error())
    with pytest.raises(_lib.XrsError, match="use larger bins"):
        _lib.call("xrs_idw_workspace_size", n, 1, 2**27, 1, ctypes.byref(size))

"""The kernel paths of xrspatial_amd.classify that the reference fixture does not reach, against the NumPy reference
of tests/classify_oracle.py (float64 comparisons, np.percentile / np.unique; never the package's own bin builders).

* the bin kernel's three searches (count up to 64 sorted bins, bisection above, the reference's loop for any others) on
  all ten raster dtypes, NumPy and DeviceArray input, cells on every edge and on its neighbours, tails of 1..3 cells;
* `binary` on all ten dtypes;
* the banded host pipeline of NumPy float32 rasters of >= 32 MiB;
* quantile / percentiles / box_plot / maximum_breaks beyond the fixture's k and dtypes, the finite reductions at 8192^2;
* 64-bit integer rasters that hold their dtype's extremes (the saturation rule);
* row-sharded binary / reclassify at world 1.

Comparisons are bit for bit (NaN equal) unless a test states a tolerance."""
import math
import warnings

import numpy as np
import pytest

import xrspatial_amd as xs
from tests import classify_oracle as orc
from xrspatial_amd import classify as cl

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]
LENGTHS = (1, 2, 3, 5, 1023, 1025, 4097)
ODD_2D = {1023: (3, 341), 1025: (5, 205), 4097: (17, 241)}


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def _agg(a):
    return xs.DataArray(a, dims=["y", "x"], attrs={"res": (1.0, 1.0)}, name="r")


def _host(x):
    return x.get() if isinstance(x, xs.DeviceArray) else np.asarray(x)


def _domain(dtype):
    """The value range the tests use for a dtype: the whole range up to 32 bits, +-2^53 for 64-bit integers."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return -1e3, 1e3
    info = np.iinfo(dtype)
    return float(max(info.min, -2 ** 53)), float(min(info.max, 2 ** 53))


def _neighbours(v, dtype):
    """v in the raster's dtype and the values just below / above it there."""
    dtype = np.dtype(dtype)
    if not np.isfinite(v):
        return []
    if dtype.kind == "f":
        x = dtype.type(v)
        if not np.isfinite(x):
            return []
        return [np.nextafter(x, dtype.type(-np.inf)), x, np.nextafter(x, dtype.type(np.inf))]
    lo, hi = _domain(dtype)
    out = []
    for c in (math.floor(v) - 1, math.floor(v), math.ceil(v), math.ceil(v) + 1):
        if lo <= c <= hi:
            out.append(c)
    return out


def _cells(bins, dtype, rng, extra=()):
    """Every edge and its neighbours, the dtype's specials, a few random cells: distinct values in `dtype`, shuffled."""
    dtype = np.dtype(dtype)
    vals = []
    for b in list(bins) + list(extra):
        vals += _neighbours(float(b), dtype)
    lo, hi = _domain(dtype)
    if dtype.kind == "f":
        tiny = np.finfo(dtype).smallest_subnormal
        vals += [np.nan, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, np.finfo(dtype).max, -np.finfo(dtype).max]
        vals += list(rng.uniform(lo * 1.1, hi * 1.1, 64))
    else:
        vals += [lo, hi, 0]
        vals += list(rng.integers(int(lo), int(hi), 64, endpoint=True))
    arr = np.array([dtype.type(v) for v in vals], dtype=dtype)
    return arr[rng.permutation(arr.size)]


def _shapes(vals):
    """(raster, label): the whole set as an odd-width 2-D raster, then every LENGTH as 1 x N, N x 1 and odd-width 2-D."""
    n = vals.size
    w = 127
    rows = -(-n // w)
    full = np.resize(vals, rows * w).reshape(rows, w)
    yield full, f"{rows}x{w}"
    for L in LENGTHS:
        seg = np.resize(np.roll(vals, L), L)
        yield seg.reshape(1, L), f"1x{L}"
        yield seg.reshape(L, 1), f"{L}x1"
        if L in ODD_2D:
            yield seg.reshape(ODD_2D[L]), f"{ODD_2D[L][0]}x{ODD_2D[L][1]}"


def _sorted_bins(n, dtype, rng, dup_runs=True, inf_last=False):
    """n non-decreasing bins in the dtype's range (its limits among them for integers; for floats bins that float32
    cannot hold, -0.0 and subnormals), optionally with runs of equal bins and +inf last."""
    lo, hi = _domain(dtype)
    if np.dtype(dtype).kind == "f":
        b = rng.uniform(lo, hi, n)
        special = [0.1, 1.0 / 3.0, -0.0, float(np.finfo(np.float32).smallest_subnormal), 1e-300]
        b[:min(n, 5)] = special[:min(n, 5)]
    else:
        b = rng.integers(int(lo), int(hi), n, endpoint=True).astype(np.float64)
        b[:min(n, 2)] = [lo, hi][:min(n, 2)]
    b = np.sort(b)
    if dup_runs and n >= 8:
        for s in rng.choice(n - 4, 3, replace=False):     # runs of equal bins
            b[s:s + 3] = b[s]
    if inf_last:
        b[-1] = np.inf
    return b


def _unsorted(b, rng):
    """The largest bin first, the others shuffled: never non-decreasing (the bins hold two distinct values)."""
    b = np.roll(b, 1)
    b[1:] = b[1:][rng.permutation(b.size - 1)]
    return b


def _new_values(n, rng, wide_int=False):
    if wide_int:                                   # int64 new_values above 2^24: rounded to float32 on the way
        nv = rng.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)
        nv[:min(n, 3)] = [2 ** 24 + 1, -(2 ** 24) - 3, 2 ** 53 - 1][:min(n, 3)]
        return nv
    nv = rng.normal(0, 100, n)
    nv[:min(n, 4)] = [16777217.0, 1e39, 1e-46, -1e39][:min(n, 4)]
    return nv


def _bin_cases(dtype, rng):
    """(label, bins, new_values, the mode bin_mode must choose)."""
    C, S, L = cl.BIN_COUNT, cl.BIN_SEARCH, cl.BIN_LITERAL
    cases = [("count1", _sorted_bins(1, dtype, rng), _new_values(1, rng), C),
             ("count63", _sorted_bins(63, dtype, rng), _new_values(63, rng), C),
             ("count64", _sorted_bins(64, dtype, rng, inf_last=True), _new_values(64, rng, wide_int=True), C),
             ("search65", _sorted_bins(65, dtype, rng, inf_last=True), _new_values(65, rng), S),
             ("search200", _sorted_bins(200, dtype, rng), _new_values(200, rng, wide_int=True), S),
             ("search4097", _sorted_bins(4097, dtype, rng, inf_last=True), _new_values(4097, rng), S)]
    for n in (3, 65, 200):
        b = _sorted_bins(n, dtype, rng, dup_runs=False)
        cases.append((f"literal{n}", _unsorted(b, rng), _new_values(n, rng), L))
    cases.append(("descending", _sorted_bins(9, dtype, rng)[::-1].copy(), _new_values(9, rng), L))
    for where in (0, 4, 8):
        b = _sorted_bins(9, dtype, rng)
        b[where] = np.nan
        cases.append((f"nan@{where}", b, _new_values(9, rng), L))
    return cases


@pytest.mark.parametrize("backend", ["numpy", "device"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_bin_kernel_modes_dtypes_and_tails(dtype, backend):
    rng = np.random.default_rng(100 + DTYPES.index(dtype))
    for label, bins, nv, mode in _bin_cases(dtype, rng):
        assert cl.bin_mode(np.asarray(bins, np.float64)) == mode, label
        vals = _cells(bins, dtype, rng)
        for a, shape in _shapes(vals):
            before = a.copy()
            data = a if backend == "numpy" else xs.DeviceArray.from_numpy(a)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)     # 1e39 -> float32 inf, as the reference's store
                got = _host(xs.classify.reclassify(_agg(data), bins=bins, new_values=nv).data)
                want = orc.bin_values(a, bins, nv)
            assert got.dtype == np.float32 and got.shape == a.shape
            np.testing.assert_array_equal(got, want, err_msg=f"{np.dtype(dtype).name} {label} {shape}")
            np.testing.assert_array_equal(_host(data), before)


@pytest.mark.parametrize("backend", ["numpy", "device"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_binary_all_dtypes(dtype, backend):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(200 + DTYPES.index(dtype.type))
    lo, hi = _domain(dtype)
    if dtype.kind == "f":
        f01 = float(dtype.type(0.1))
        base = np.concatenate([rng.normal(0, 10, 5000).round(1), [0.1, f01, 0.0, -0.0, np.nan, np.inf, -np.inf, 3.0]])
        lists = [[], [np.nan], [np.inf], [-0.0], [0.1], [f01, 3.0], [-np.inf, np.inf, 2.5]]
    else:
        base = np.concatenate([rng.integers(int(lo), int(hi), 5000, endpoint=True), [lo, hi, lo + 1, hi - 1, 0, 1, 3]])
        lists = [[], [np.nan], [np.inf], [-0.0], [lo, hi], [lo - 1, hi + 1], [3, 0.5, hi]]
        if dtype == np.uint8:
            lists.append([-1, 256])
    a = np.array([dtype.type(v) for v in base], dtype=dtype)[rng.permutation(base.size)]
    for values in lists:
        for shape in ((1, a.size), (a.size, 1), (83, a.size // 83)):
            r = np.ascontiguousarray(np.resize(a, shape))
            before = r.copy()
            data = r if backend == "numpy" else xs.DeviceArray.from_numpy(r)
            got = _host(xs.classify.binary(_agg(data), values).data)
            want = orc.binary(r, values)
            assert got.dtype == dtype and got.shape == r.shape, (values, shape)
            np.testing.assert_array_equal(got, want, err_msg=f"{dtype.name} {values} {shape}")
            np.testing.assert_array_equal(_host(data), before)
    if dtype == np.float32:                         # 0.1 is not float32(0.1): the compare is in float64
        hit = _host(xs.classify.binary(_agg(np.full((2, 3), np.float32(0.1))), [0.1]).data)
        np.testing.assert_array_equal(hit, np.zeros((2, 3), np.float32))


# ------------------------------------------------------------------ the banded pipeline of NumPy float32 rasters
def test_banded_pipeline_equals_device_path(monkeypatch):
    """4099 x 4097 float32 (three 8 Mi-cell chunks, the last one ragged) through binary and reclassify in all three
    modes: the pipeline must be taken, and equal the DeviceArray path and the NumPy reference."""
    taken = []
    real = cl.percell_pipelined

    def spy(fn, hosts, extra):
        out = real(fn, hosts, extra)
        taken.append((fn, out is not None))
        return out

    monkeypatch.setattr(cl, "percell_pipelined", spy)
    rng = np.random.default_rng(9)
    a = rng.normal(0, 50, (4099, 4097)).astype(np.float32)
    a[rng.random(a.shape) < 1e-3] = np.nan
    a[0, 0], a[-1, -1], a[2048, 7] = np.inf, -np.inf, 12.5
    q = (np.round(a / 0.25) * 0.25).astype(np.float32)           # <= 1000 distinct values for the literal oracle
    q = np.clip(q, -124.75, 124.75)
    dev_a, dev_q = xs.DeviceArray.from_numpy(a), xs.DeviceArray.from_numpy(q)
    count_bins = [-50.0, -0.1, 0.0, 0.1, 12.5, 80.0]
    search_bins = list(np.sort(rng.uniform(-150, 150, 99))) + [np.inf]
    literal_bins = [20.0, -5.0, 100.0, np.nan, 0.0, 55.0]
    values = [12.5, float(a[1, 1]), float(a[4098, 4096]), float(a[3000, 5]), np.inf]
    held = xs.classify.binary(_agg(a), values).data
    kept = held.copy()
    runs = [("binary", a, dev_a, {"values": values}, lambda r: orc.binary(r, values))]
    for bins in (count_bins, search_bins, literal_bins):
        nv = np.arange(len(bins), dtype=np.float64) * 1.5 - 3
        r = q if bins is literal_bins else a
        d = dev_q if bins is literal_bins else dev_a
        runs.append(("reclassify", r, d, {"bins": bins, "new_values": nv}, lambda r, b=bins, v=nv: orc.bin_values(r, b, v)))
    for fn, host, dev, kw, ref in runs:
        n_before = len(taken)
        got = getattr(xs.classify, fn)(_agg(host), **kw).data
        assert taken[n_before:] and taken[-1][1], f"{fn}: the banded pipeline was not taken"
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == host.shape
        np.testing.assert_array_equal(got, getattr(xs.classify, fn)(_agg(dev), **kw).data.get(), err_msg=fn)
        np.testing.assert_array_equal(got, ref(host), err_msg=f"{fn} {kw.get('bins', '')}")
    np.testing.assert_array_equal(held, kept)                     # a held result survives the later pipelined calls
    assert {m for m in (cl.bin_mode(np.asarray(b, np.float64)) for b in (count_bins, search_bins, literal_bins))} == \
        {cl.BIN_COUNT, cl.BIN_SEARCH, cl.BIN_LITERAL}


# ------------------------------------------------------------------ statistic classifiers: bins against NumPy
@pytest.fixture
def bins_seen(monkeypatch):
    """The bins every statistic classifier hands to the bin pass."""
    seen = []
    real = cl._bin_device

    def spy(dev, bins, new_values):
        seen.append(np.asarray(bins))
        return real(dev, bins, new_values)

    monkeypatch.setattr(cl, "_bin_device", spy)
    return seen


def _stat_rasters():
    rng = np.random.default_rng(31)
    f32 = rng.gamma(2.0, 10.0, (301, 257)).astype(np.float32)
    f32.ravel()[rng.choice(f32.size, 600, replace=False)] = [np.nan, np.inf, -np.inf] * 200
    f64 = rng.normal(-3.0, 1e3, (256, 311))
    f64.ravel()[rng.choice(f64.size, 300, replace=False)] = [np.nan, np.inf, -np.inf] * 100
    i16 = rng.integers(-32768, 32768, (129, 255)).astype(np.int16)
    i16[0, :4] = [-32768, 32767, -32768, 32767]
    yield "f32", f32
    yield "f64", f64
    yield "i8", rng.integers(-128, 128, (97, 101)).astype(np.int8)
    yield "i16_full_range", i16
    yield "u16", rng.integers(0, 65536, (123, 77)).astype(np.uint16)
    yield "u32", rng.integers(0, 2 ** 32, (111, 99), dtype=np.uint64).astype(np.uint32)
    yield "i64", rng.integers(-2 ** 53, 2 ** 53, (64, 127)).astype(np.int64)
    yield "u64", rng.integers(0, 2 ** 53, (65, 63)).astype(np.uint64)


STAT_CALLS = ([("quantile", {"k": k}) for k in (2, 33, 64, 100)]
              + [("percentiles", {"pct": sorted(set([0.0, 100.0, 33.3] + list(np.round(np.linspace(0.5, 99.5, 67), 3))))}),
                 ("box_plot", {"hinge": 0}), ("box_plot", {"hinge": 1.5}), ("box_plot", {"hinge": 3})])


@pytest.mark.parametrize("name,a", list(_stat_rasters()), ids=[n for n, _ in _stat_rasters()])
def test_percentile_classifiers_beyond_the_fixture(name, a, bins_seen, capsys):
    assert len(STAT_CALLS[4][1]["pct"]) == 70
    for fn, kw in STAT_CALLS:
        bins_seen.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = np.asarray(getattr(xs.classify, fn)(_agg(a), **kw).data)
            want = orc.bins_of(fn, a, **kw)
        capsys.readouterr()
        assert len(bins_seen) == 1, fn
        b = bins_seen[0]
        assert b.dtype == want.dtype, (fn, kw, b.dtype, want.dtype)
        np.testing.assert_array_equal(b.astype(np.float64) + 0.0, want.astype(np.float64) + 0.0, err_msg=f"{name} {fn} {kw}")
        np.testing.assert_array_equal(got, orc.bin_values(a, want, np.arange(len(want))), err_msg=f"{name} {fn} {kw}")


def _breaks_rasters():
    rng = np.random.default_rng(41)
    grid = (np.arange(3000, dtype=np.float32) * np.float32(0.5))            # every gap equal: ties resolved by index
    yield "f32_equal_gaps", grid[rng.permutation(grid.size)].reshape(50, 60)
    z = rng.normal(0, 1, (80, 90)).astype(np.float32)
    z.ravel()[:400] = [0.0, -0.0] * 200
    z.ravel()[400:430] = [np.nan, np.inf, -np.inf] * 10
    yield "f32_signed_zeros", z
    # float32 gaps (-3e38 .. 2e38) and midpoint sums (above 2e38) that overflow to inf
    big = np.concatenate([-3e38 - np.arange(60) * 5e35, 2e38 + np.arange(60) * 2.3e36]).astype(np.float32)
    yield "f32_overflowing_gaps", np.resize(big[rng.permutation(big.size)], (30, 50))
    yield "f64", np.round(rng.normal(0, 100, (70, 71)), 2)
    yield "i16", rng.integers(-32768, 32768, (90, 91)).astype(np.int16)
    yield "u8", rng.integers(0, 256, (33, 35)).astype(np.uint8)
    yield "i64", rng.integers(-2 ** 40, 2 ** 40, (60, 61)).astype(np.int64)


@pytest.mark.parametrize("name,a", list(_breaks_rasters()), ids=[n for n, _ in _breaks_rasters()])
def test_maximum_breaks_beyond_the_fixture(name, a, bins_seen):
    for k in (2, 64, 65, 66, 100, 1000):
        bins_seen.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            got = np.asarray(xs.classify.maximum_breaks(_agg(a), k=k).data)
            want = orc.maximum_breaks_bins(a, k)
        b = bins_seen[0]
        assert b.dtype == want.dtype, (name, k, b.dtype, want.dtype)
        np.testing.assert_array_equal(b.astype(np.float64) + 0.0, want.astype(np.float64) + 0.0, err_msg=f"{name} k={k}")
        np.testing.assert_array_equal(got, orc.bin_values(a, want, np.arange(len(want))), err_msg=f"{name} k={k}")


def test_maximum_breaks_a_million_distinct_values(bins_seen):
    rng = np.random.default_rng(43)
    pool = rng.standard_cauchy(10 ** 6).astype(np.float32)
    a = pool[rng.integers(0, pool.size, (4097, 4099))]
    assert 9e5 < np.unique(a).size <= 10 ** 6
    dev = xs.DeviceArray.from_numpy(a)
    for k in (2, 65, 66, 1000):
        bins_seen.clear()
        got = xs.classify.maximum_breaks(_agg(dev), k=k).data.get()
        want = orc.maximum_breaks_bins(a, k)
        assert bins_seen[0].dtype == want.dtype
        np.testing.assert_array_equal(bins_seen[0].astype(np.float64), want.astype(np.float64), err_msg=f"k={k}")
        np.testing.assert_array_equal(got, orc.bin_values(a, want, np.arange(len(want))), err_msg=f"k={k}")


def test_finite_reductions_at_8192_squared():
    """count / min / max exact; sum and the sum of squared deviations within the float64 rounding bound of a
    correctly rounded sum (math.fsum): (n - 1) * 2^-53 * sum of |terms|.  std_mean and head_tail_breaks keep the
    edge-only tolerance of tests/test_gpu_classify.py."""
    rng = np.random.default_rng(47)
    a = (rng.lognormal(3.0, 2.0, (8192, 8192)) * np.where(rng.random((8192, 8192)) < 0.1, -1, 1)).astype(np.float32)
    a[rng.random(a.shape) < 1e-3] = np.nan
    a[::4093, ::911] = np.inf
    dev = xs.DeviceArray.from_numpy(a)
    fin = a[np.isfinite(a)].astype(np.float64)
    st = cl._Stats(dev)
    n, mn, mx, s = st.moments()
    assert n == fin.size and mn == fin.min() and mx == fin.max()
    exact = math.fsum(memoryview(fin))
    bound = (n - 1) * 2.0 ** -53 * math.fsum(memoryview(np.abs(fin)))
    assert abs(s - exact) <= bound, (s, exact, bound)
    mean = s / n
    terms = (fin - mean) ** 2
    sq_exact = math.fsum(memoryview(terms))
    assert abs(st.sqdev(mean) - sq_exact) <= (n + 2) * 2.0 ** -53 * sq_exact
    del fin, terms
    for fn in ("std_mean", "head_tail_breaks"):
        ref = orc.bins_of(fn, a)
        got = getattr(xs.classify, fn)(_agg(dev)).data.get()
        want = orc.bin_values(a, ref, np.arange(len(ref)))
        diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        if diff.any():
            x = a.astype(np.float64)[diff]
            edge = ref[np.minimum(got[diff], want[diff]).astype(np.int64)]
            assert np.all(np.abs(got[diff] - want[diff]) == 1), fn
            assert np.all(np.abs(x - edge) <= 1e-5 * np.maximum(np.abs(edge), float(np.nanstd(a[np.isfinite(a)])))), fn


# ------------------------------------------------------------------ 64-bit integer extremes
def _extreme_rasters():
    i64, u64 = np.iinfo(np.int64), np.iinfo(np.uint64)
    rng = np.random.default_rng(53)
    mid = rng.integers(-3000, 3000, 4000)
    a = np.concatenate([mid, np.array([i64.max, i64.max - 1, 2 ** 62, i64.min, i64.min + 1, -2 ** 61], np.int64)])
    yield "i64_max_min", a.astype(np.int64)[rng.permutation(a.size)].reshape(2, 2003)
    b = np.concatenate([(mid + 5000).astype(np.uint64), np.array([u64.max, u64.max - 1, 2 ** 63, 2 ** 64 - 2 ** 12], np.uint64)])
    yield "u64_max", b[rng.permutation(b.size)].reshape(4, 1001)


EXTREME_CALLS = [("quantile", {"k": 4}), ("quantile", {"k": 100}), ("percentiles", {"pct": [0, 0.01, 1, 50, 99.99, 100]}),
                 ("box_plot", {"hinge": 1.5}), ("maximum_breaks", {"k": 3}), ("maximum_breaks", {"k": 70})]


@pytest.mark.parametrize("name,a", list(_extreme_rasters()), ids=[n for n, _ in _extreme_rasters()])
def test_64_bit_extremes_saturate(name, a, bins_seen):
    """No exception, no bin with a flipped sign, every bin within 4 ulp of the largest |cell| of the NumPy reference's,
    the exact min and max where the reference has them, and a cell off the reference only that close to an edge."""
    x = a.astype(np.float64)
    tol = 4 * np.spacing(np.max(np.abs(x)))
    for fn, kw in EXTREME_CALLS:
        bins_seen.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("error")                        # no wrapped cast, no scalar overflow
            got = getattr(xs.classify, fn)(_agg(a), **kw).data
        want = orc.bins_of(fn, a, **kw).astype(np.float64)
        b = bins_seen[0].astype(np.float64)
        assert b.size == want.size, (fn, kw, b, want)
        assert np.all(np.sign(b) == np.sign(want)), (fn, kw, b, want)
        assert np.all(np.abs(b - want) <= tol), (fn, kw, b - want)
        for extreme in (x.min(), x.max()):
            if extreme in want:
                assert extreme in b, (fn, kw, extreme)
        ref_out = orc.bin_values(a, want, np.arange(len(want)))
        off = ~((got == ref_out) | (np.isnan(got) & np.isnan(ref_out)))
        if off.any():
            near = np.min(np.abs(x[off][:, None] - want[None, :]), axis=1)
            assert np.all(near <= tol), (fn, kw, int(off.sum()))


# ------------------------------------------------------------------ row-sharded binary / reclassify at world 1
def test_sharded_world1_binary_and_reclassify():
    from xrspatial_amd import ShardedArray
    rng = np.random.default_rng(61)
    rasters = {np.float32: rng.normal(0, 10, (97, 130)).astype(np.float32), np.float64: rng.normal(0, 10, (97, 130)),
               np.int32: rng.integers(-50, 50, (97, 130)).astype(np.int32), np.int8: rng.integers(-50, 50, (97, 130)).astype(np.int8)}
    rasters[np.float32][3, 4], rasters[np.float64][5, 6] = np.nan, -np.inf
    bins_list = ([-5.0, 0.0, 5.0, np.inf], list(np.linspace(-40, 40, 80)), [5.0, -5.0, np.nan, 20.0])
    for dtype, a in rasters.items():
        sh = xs.DataArray(ShardedArray.from_numpy(a), dims=["y", "x"])
        dev = xs.DataArray(xs.DeviceArray.from_numpy(a), dims=["y", "x"])
        values = [float(a[0, 0]), float(a[50, 50]), 3]
        out = xs.classify.binary(sh, values).data
        assert isinstance(out, ShardedArray) and out.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(out.get(), xs.classify.binary(dev, values).data.get())
        np.testing.assert_array_equal(out.get(), orc.binary(a, values))
        for bins in bins_list:
            nv = np.arange(len(bins)) + 0.5
            if dtype == np.int8:
                with pytest.raises(NotImplementedError):
                    xs.classify.reclassify(sh, bins, nv)
                continue
            out = xs.classify.reclassify(sh, bins, nv).data
            assert isinstance(out, ShardedArray) and out.dtype == np.float32
            np.testing.assert_array_equal(out.get(), xs.classify.reclassify(dev, bins, nv).data.get())
            np.testing.assert_array_equal(out.get(), orc.bin_values(a, bins, nv))
    sh = xs.DataArray(ShardedArray.from_numpy(rasters[np.float32]), dims=["y", "x"])
    for fn in ("quantile", "equal_interval", "percentiles", "box_plot", "std_mean", "head_tail_breaks", "maximum_breaks"):
        with pytest.raises(NotImplementedError):
            getattr(xs.classify, fn)(sh)

"""Zone-id discovery and pair counting at the C ABI (xrspatial_amd/csrc/zonal_index.hip), and 64-bit ids through the
public zonal functions, against NumPy on the host: np.unique / np.searchsorted / np.bincount, never a function of the
package.

* xrs_crosstab_counts: the three launch tiers and their edges, the grid caps, indices outside the table, one address
  taking every atomic, planes of which only one is 16-byte aligned, accumulation into what the table held;
* xrs_zonal_scan / _presence / _index on int32 / int64 / float32 / float64: the 16-byte path and the element path, tails,
  chunks beyond the data, the capped grid, ids at the dtypes' ends and at the limits of what a float holds, NaN / inf /
  -0.0, non-integral ids, a window that covers part of the ids;
* xrs_zonal_scan_presence_i32: ids on both sides of the window's ends, guard bytes around the map;
* zonal.stats / crosstab / majority / trim / crop with int64 and uint64 ids a double cannot tell apart.

Everything is integer-valued and every comparison is exact; the one tolerance is crosstab's `percentage` (rtol 1e-6, as
test_zonal_crosstab).  The crosstab tests come first: run on its own, this module calls the 1024-thread tier (which
raises its LDS limit once per process) before any other tier."""
import numpy as np
import pytest

import xrspatial_amd as xs
from oracle import xrs_oracle as orc
from tests import zonal_id_cases as zc
from xrspatial_amd import _lib, zonal
from xrspatial_amd._launch import get_stream

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 4097, 2_200_003)      # the last: grid cap reached, not a multiple of 4
BIG = LENGTHS[-1]
ZDTYPES = [np.int32, np.int64, np.float32, np.float64]
I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def _agg(a, backend="numpy"):
    return xs.DataArray(xs.DeviceArray.from_numpy(a) if backend == "hip" else a, dims=["y", "x"])


def _place(arr, shift):
    """`arr` in HBM at a 16-byte aligned base (shift 0) or `shift` elements past one (the `shifted()` construction of
    test_unaligned_device_views)."""
    flat = np.zeros(arr.size + 8, dtype=arr.dtype)
    flat[shift:shift + arr.size] = arr.ravel()
    base = xs.DeviceArray.from_numpy(flat)
    view = xs.DeviceArray(arr.shape, arr.dtype, _ptr=base.ptr + shift * arr.dtype.itemsize, _base=base)
    assert base.ptr % 16 == 0 and (view.ptr % 16 == 0) == (shift == 0)
    return view


# ------------------------------------------------------------------------------------------ xrs_crosstab_counts
SMALL, MIDDLE = 16384, 36864                                          # table cells: LDS / 256 threads, LDS / 1024, global
TABLES = [(1, 1), (128, 128), (127, 127), (5, 3277), (192, 192), (181, 191), (365, 101), (211, 211)]
ALIGN = [(0, 0), (1, 0), (0, 1)]                                      # (zone plane shift, category plane shift)


def _tier(nz, nc):
    return "small" if nz * nc <= SMALL else "middle" if nz * nc <= MIDDLE else "global"


def _big_n(nz, nc):
    return 1_000_003 if _tier(nz, nc) == "middle" else BIG            # above the grid caps: 256 x 1024 x 4, 2048 x 256 x 4


def _index_planes(n, nz, nc, rng):
    """Two int32 index planes with 1 % of -1 and 1 % of nz / nc (one too large) in each."""
    zi, ci = rng.integers(0, nz, n).astype(np.int32), rng.integers(0, nc, n).astype(np.int32)
    for plane, top in ((zi, nz), (ci, nc)):
        u = rng.random(n)
        plane[u < 0.01] = -1
        plane[u > 0.99] = top
    return zi, ci


def _want_counts(zi, ci, nz, nc):
    ok = (zi >= 0) & (zi < nz) & (ci >= 0) & (ci < nc)
    return np.bincount(zi[ok].astype(np.int64) * nc + ci[ok], minlength=nz * nc).astype(np.uint64)


def _check_counts(zi, ci, nz, nc, shifts, label):
    """The table of one call, and of a second call on the same buffer (the ABI adds to what `counts` holds)."""
    zd, cd = _place(zi, shifts[0]), _place(ci, shifts[1])
    counts = xs.DeviceArray.from_numpy(np.zeros(nz * nc, np.uint64))
    want = _want_counts(zi, ci, nz, nc)
    for k in (1, 2):
        _lib.call("xrs_crosstab_counts", zd.ptr, cd.ptr, zi.size, nz, nc, counts.ptr, get_stream())
        np.testing.assert_array_equal(counts.get(get_stream()), want * np.uint64(k), err_msg=f"{label} call {k}")
    return want


def test_crosstab_counts_middle_tier_first():
    rng = np.random.default_rng(101)
    nz, nc = 181, 191
    zi, ci = _index_planes(70_001, nz, nc, rng)
    _check_counts(zi, ci, nz, nc, (0, 0), "middle tier, first")
    zi, ci = _index_planes(70_001, 127, 127, rng)
    _check_counts(zi, ci, 127, 127, (0, 0), "small tier after the middle one")


def test_crosstab_counts_middle_tier_after_the_small_one():
    rng = np.random.default_rng(102)
    for nz, nc in ((128, 128), (192, 192), (5, 3277), (365, 101), (192, 192)):
        zi, ci = _index_planes(50_003, nz, nc, rng)
        _check_counts(zi, ci, nz, nc, (0, 0), f"{nz}x{nc}")


@pytest.mark.parametrize("nz,nc", TABLES, ids=[f"{a}x{b}-{_tier(a, b)}" for a, b in TABLES])
def test_crosstab_counts_vs_bincount(nz, nc):
    rng = np.random.default_rng(nz * 7 + nc)
    for n in (0, 1, 3, 5, 1025, _big_n(nz, nc)):
        zi, ci = _index_planes(n, nz, nc, rng)
        for shifts in ALIGN:
            want = _check_counts(zi, ci, nz, nc, shifts, f"{nz}x{nc} n={n} shifts={shifts}")
        assert int(want.sum()) <= n and (n < 1025 or 0 < int(want.sum()) < n)        # (some pairs were skipped)


@pytest.mark.parametrize("nz,nc", [(1, 1), (128, 128), (192, 192), (211, 211)])
def test_crosstab_counts_every_pair_on_one_cell(nz, nc):
    for n in (1025, _big_n(nz, nc)):
        zi, ci = np.full(n, nz - 1, np.int32), np.full(n, nc - 1, np.int32)
        for shifts in ALIGN:
            want = _check_counts(zi, ci, nz, nc, shifts, f"{nz}x{nc} n={n} shifts={shifts}")
        assert int(want[-1]) == n and int(want.sum()) == n


# ------------------------------------------------------------------------ xrs_zonal_scan / _presence / _index
def _id_sets(dtype):
    """name -> ids (in `dtype`) whose span stays small enough for a presence map."""
    dtype = np.dtype(dtype)
    sets = {"dense_small": np.arange(0, 40), "gaps_negative": np.array([-300, -299, -17, -1, 0, 3, 4, 250, 1999]),
            "single": np.array([7])}
    if dtype == np.int32:
        sets["int32_min"] = I32.min + np.arange(6)
        sets["int32_max"] = I32.max - np.arange(6)[::-1]
    if dtype == np.int64:
        sets["around_2p31"] = (1 << 31) + np.arange(-3, 4)
        sets["around_m2p31"] = -(1 << 31) + np.arange(-3, 4)
        sets["below_2p53"] = zc.P53 - np.arange(1, 9)[::-1]
        sets["above_m2p53"] = -(zc.P53 - np.arange(1, 9))
    if dtype == np.float32:
        sets["around_2p24"] = np.array([2 ** 24 - 3, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 2, 2 ** 24 + 4, 2 ** 24 + 16])
        sets["around_m2p24"] = -sets["around_2p24"][::-1]
    if dtype == np.float64:
        sets["around_2p53"] = np.array([2.0 ** 53 - 3, 2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 53 + 4, 2.0 ** 53 + 16])
        sets["at_2p60"] = 2.0 ** 60 + 256.0 * np.array([0, 1, 2, 4, 9])
    if dtype.kind == "f":
        sets["signed_zero"] = np.array([-2.0, -0.0, 0.0, 1.0, 5.0])
    out = {}
    for name, ids in sets.items():
        cast = ids.astype(dtype)
        assert [int(c) for c in cast] == [int(i) for i in ids], name          # (the dtype holds every id as written)
        out[name] = cast
    return out


def _fill(ids, n, rng, specials=False):
    """n cells drawn from `ids`: runs of 1..16 equal cells with single cells strewn over them, every id present when n
    allows; `specials` (float dtypes): 2 % NaN, one +inf, one -inf."""
    if n == 0:
        return ids[:0].copy()
    n_runs = n // 8 + 1
    flat = np.resize(np.repeat(rng.integers(0, len(ids), n_runs), rng.integers(1, 17, n_runs)), n)
    strewn = rng.integers(0, n, n // 16 + 1)
    flat[strewn] = rng.integers(0, len(ids), strewn.size)
    k = min(n, len(ids))
    flat[:k] = np.arange(k)
    z = ids[rng.permutation(len(ids))][flat] if n < len(ids) else ids[flat]
    if specials:
        z[rng.random(n) < 0.02] = np.nan
        if n >= 3:
            where = rng.choice(n, 2, replace=False)
            z[where[0]], z[where[1]] = np.inf, -np.inf
    return z


def _call_scan(dev):
    res = xs.DeviceArray.from_numpy(np.full(4, -123.0))
    _lib.call("xrs_zonal_scan", dev.ptr, zonal._ZONE_DTYPE_CODE[dev.dtype], dev.size, res.ptr, get_stream())
    raw = res.get(get_stream())
    return float(raw[0]), float(raw[1]), int(raw[2:3].view(np.uint64)[0]), int(raw[3:4].view(np.int32)[0])


def _want_scan(z):
    fin = z[np.isfinite(z)] if z.dtype.kind == "f" else z
    if fin.size == 0:
        return np.inf, -np.inf, 0, 1
    integral = 1 if z.dtype.kind != "f" else int(bool(np.all(fin == np.floor(fin))))
    return float(fin.min()), float(fin.max()), int(fin.size), integral


def _lut(ids, lo, span):
    """(presence bytes, int32 LUT) over [lo, lo + span) of the ascending `ids` inside it, in exact integer arithmetic."""
    offs = np.array([int(u) - lo for u in ids], dtype=np.int64)
    present = np.zeros(span, np.uint8)
    present[offs] = 1
    lut = np.where(present > 0, np.cumsum(present, dtype=np.int64) - 1, -1).astype(np.int32)
    return present, lut


def _call_index(dev, lo, span, lut):
    lut_dev = xs.DeviceArray.from_numpy(lut)
    idx = xs.DeviceArray.from_numpy(np.full(dev.shape, -7, np.int32))
    _lib.call("xrs_zonal_index", dev.ptr, zonal._ZONE_DTYPE_CODE[dev.dtype], dev.size, float(lo), span, lut_dev.ptr, idx.ptr,
              get_stream())
    return idx.get(get_stream())


def _check_id_kernels(z, label):
    """scan, presence map, index plane and a partly covering index window of one raster, at both alignments."""
    finite = np.isfinite(z) if z.dtype.kind == "f" else np.ones(z.shape, bool)
    uniq = np.unique(z[finite])
    want = _want_scan(z)
    lo, hi = (int(want[0]), int(want[1])) if want[2] else (0, 0)
    span = hi - lo + 1
    present, lut = _lut(uniq, lo, span)
    np.testing.assert_array_equal(present, np.isin(np.arange(span, dtype=object) + lo, [int(u) for u in uniq]).astype(np.uint8))
    want_idx = np.full(z.shape, -1, np.int32)
    want_idx[finite] = np.searchsorted(uniq, z[finite])
    inner = uniq[1:-1]                                                 # a window that leaves ids out on both sides
    if inner.size:
        lo2, span2 = int(inner[0]), int(inner[-1]) - int(inner[0]) + 1
        _, lut2 = _lut(inner, lo2, span2)
        covered = finite & (z >= inner[0]) & (z <= inner[-1])
        want_idx2 = np.full(z.shape, -1, np.int32)
        want_idx2[covered] = np.searchsorted(inner, z[covered])
    for shift in (0, 1):
        tag = f"{label} shift={shift}"
        dev = _place(z, shift)
        got = _call_scan(dev)
        assert got == want, (tag, got, want)
        seen = xs.DeviceArray.from_numpy(np.full(span, 0xAA, np.uint8))
        _lib.call("xrs_zonal_presence", dev.ptr, zonal._ZONE_DTYPE_CODE[dev.dtype], dev.size, float(lo), span, seen.ptr, get_stream())
        np.testing.assert_array_equal(seen.get(get_stream()), present, err_msg=f"{tag} presence")
        np.testing.assert_array_equal(_call_index(dev, lo, span, lut), want_idx, err_msg=f"{tag} index")
        if inner.size:
            np.testing.assert_array_equal(_call_index(dev, lo2, span2, lut2), want_idx2, err_msg=f"{tag} partial window")


@pytest.mark.parametrize("dtype", ZDTYPES, ids=lambda d: np.dtype(d).name)
def test_id_kernels_vs_numpy(dtype):
    rng = np.random.default_rng(7)
    cases = 0
    for name, ids in _id_sets(dtype).items():
        for n in LENGTHS:
            _check_id_kernels(_fill(ids, n, rng), f"{np.dtype(dtype).name} {name} n={n}")
            cases += 1
            if np.dtype(dtype).kind == "f" and n:
                _check_id_kernels(_fill(ids, n, rng, specials=True), f"{np.dtype(dtype).name} {name} n={n} NaN/inf")
                cases += 1
    print(f"{np.dtype(dtype).name}: {cases} rasters x 2 alignments")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_scan_flags_non_integral_ids_and_rasters_without_ids(dtype):
    rng = np.random.default_rng(8)
    ids = _id_sets(dtype)["dense_small"]
    tiny = np.finfo(dtype).smallest_subnormal
    for n in (1, 5, 1025, 4097, BIG):
        for frac in (dtype(0.5), tiny, dtype(-2.5)):
            for where in sorted({n - 1, min(5, n - 1), n // 2}):     # the tail after the last 16-byte slot; the 16-byte body
                z = _fill(ids, n, rng)
                z[where] = frac
                want = _want_scan(z)
                assert want[3] == 0
                for shift in (0, 1):
                    got = _call_scan(_place(z, shift))
                    assert got == want, (np.dtype(dtype).name, n, float(frac), where, shift, got, want)
        z = np.full(n, np.nan, dtype=dtype)
        z[::3], z[1::5] = np.inf, -np.inf
        _check_id_kernels(z, f"{np.dtype(dtype).name} no finite id n={n}")
    # the public functions on such a raster (the host maps it): the oracle's frame
    zones = _fill(ids, 37 * 61, rng).reshape(37, 61)
    zones[5, 7], zones[20, 3] = 0.5, tiny
    vals = zc.small_values(zones.shape, seed=9)
    for backend in ("numpy", "hip"):
        got = zonal.stats(_agg(zones, backend), _agg(vals, backend), stats_funcs=["count", "max"])
        zc.assert_stats_frame(got, orc.zonal_stats(zones, vals, stats_funcs=["count", "max"]), ["count", "max"], zone_dtype=dtype)


@pytest.mark.parametrize("window", [1, 256, zonal._OPTIMISTIC_WINDOW])
def test_scan_presence_i32_window(window):
    rng = np.random.default_rng(9)
    guard = 64
    edges = np.array([-1, 0, window - 1, window, I32.min, window + 5, -7, I32.max], dtype=np.int64)
    ids = np.unique(np.concatenate([edges, rng.integers(-3, window + 3, 50)])).astype(np.int32)
    for n in LENGTHS:
        z = _fill(ids, n, rng)
        want_map = np.zeros(window, np.uint8)
        want_map[z[(z >= 0) & (z < window)]] = 1
        want = _want_scan(z)
        for shift in (0, 1):
            dev = _place(z, shift)
            buf = xs.DeviceArray.from_numpy(np.full(window + 2 * guard, 0xAA, np.uint8))
            res = xs.DeviceArray.from_numpy(np.full(4, -123.0))
            _lib.call("xrs_zonal_scan_presence_i32", dev.ptr, dev.size, res.ptr, buf.ptr + guard, window, get_stream())
            raw, out = res.get(get_stream()), buf.get(get_stream())
            got = float(raw[0]), float(raw[1]), int(raw[2:3].view(np.uint64)[0]), int(raw[3:4].view(np.int32)[0])
            assert got == want, (window, n, shift, got, want)
            np.testing.assert_array_equal(out[guard:guard + window], want_map, err_msg=f"window={window} n={n} shift={shift}")
            assert (out[:guard] == 0xAA).all() and (out[guard + window:] == 0xAA).all(), (window, n, shift)


# ------------------------------------------------------------------------------------- through the public API
STATS = ["count", "min", "max", "majority"]


@pytest.mark.parametrize("backend", ["numpy", "hip"])
@pytest.mark.parametrize("name", list(zc.INT64_ID_SETS))
def test_stats_of_int64_zones_a_double_merges(monkeypatch, name, backend):
    monkeypatch.delenv("XRS_ZONAL_MAJORITY", raising=False)
    ids = zc.INT64_ID_SETS[name]
    z = zc.id_raster(ids, seed=3)
    v = zc.small_values(z.shape, seed=3)
    got = zonal.stats(_agg(z, backend), _agg(v, backend), stats_funcs=STATS)
    zc.assert_stats_frame(got, orc.zonal_stats(z, v, stats_funcs=STATS), STATS, zone_dtype=np.int64, label=name)
    assert got["zone"].tolist() == ids
    picked = [ids[-1], ids[0], 12345]                                   # Python ints, one of them absent
    got = zonal.stats(_agg(z, backend), _agg(v, backend), zone_ids=picked, stats_funcs=["count"])
    zc.assert_stats_frame(got, orc.zonal_stats(z, v, zone_ids=picked, stats_funcs=["count"]), ["count"], label=name)
    assert got["zone"].tolist() == [ids[0], ids[-1]]
    plane = zonal.stats(_agg(z, backend), _agg(v, backend), stats_funcs=["count", "max"], return_type="xarray.DataArray")
    data = plane.data.get() if isinstance(plane.data, xs.DeviceArray) else np.asarray(plane.data)
    np.testing.assert_array_equal(data, orc.zonal_stats(z, v, stats_funcs=["count", "max"], return_type="array"))


@pytest.mark.parametrize("backend", ["numpy", "hip"])
@pytest.mark.parametrize("name", list(zc.INT64_ID_SETS))
def test_crosstab_of_int64_zones_and_categories_a_double_merges(name, backend):
    ids = zc.INT64_ID_SETS[name]
    z = zc.id_raster(ids, seed=5)
    small = zc.small_zones(z.shape, seed=5)
    cats = zc.id_raster(ids, seed=6)
    for zones, values in ((z, small), (small, cats), (z, cats)):
        for agg in ("count", "percentage"):
            got = zonal.crosstab(_agg(zones, backend), _agg(values, backend), agg=agg)
            zc.assert_crosstab_frame(got, orc.crosstab_2d(zones, values, agg=agg), agg, zone_dtype=zones.dtype,
                                     label=f"{name} {backend} {agg}")
    kw = dict(zone_ids=[ids[-1], ids[0]], cat_ids=[ids[0], ids[-1]])
    got = zonal.crosstab(_agg(z, backend), _agg(cats, backend), **kw)
    zc.assert_crosstab_frame(got, orc.crosstab_2d(z, cats, **kw), label=f"{name} {backend} selection")


WIDE_VALUES = {
    "int64_2p52": np.array([2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 52 + 3], np.int64),
    "int64_m2p52": -np.array([2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, 2 ** 52 + 3], np.int64)[::-1],
    "float64_2p52": np.array([2.0 ** 52 - 1, 2.0 ** 52, 2.0 ** 52 + 1, 2.0 ** 52 + 3]),
    "float64_2p60": 2.0 ** 60 + 256.0 * np.array([0, 1, 2, 4]),
}


@pytest.mark.parametrize("route", ["", "sort", "hash"], ids=["counting_first", "sort", "hash"])
@pytest.mark.parametrize("name", list(WIDE_VALUES))
def test_majority_of_wide_values(monkeypatch, name, route):
    """Values are reduced on their float64 image, which holds every value used here."""
    if route:
        monkeypatch.setenv("XRS_ZONAL_MAJORITY", route)
    else:
        monkeypatch.delenv("XRS_ZONAL_MAJORITY", raising=False)
    rng = np.random.default_rng(13)
    pool = WIDE_VALUES[name]
    zones = zc.small_zones((64, 97), n_zones=5, seed=13)
    # every zone prefers another value; zone 4 has a tie (the smaller value wins)
    vals = pool[rng.integers(0, len(pool), zones.shape)]
    for zid in range(4):
        pick = (zones == zid) & (rng.random(zones.shape) < 0.4)
        vals[pick] = pool[zid]
    four = np.flatnonzero(zones.ravel() == 4)
    vals.ravel()[four] = pool[np.arange(four.size) % 2 + 1][: four.size]
    if four.size % 2:
        vals.ravel()[four[-1]] = pool[3]
    want = orc.zonal_stats(zones, vals, stats_funcs=["majority", "count"])
    assert want["majority"][4] == float(pool[1])
    for backend in ("numpy", "hip"):
        got = zonal.stats(_agg(zones, backend), _agg(vals, backend), stats_funcs=["majority", "count"])
        zc.assert_stats_frame(got, want, ["majority", "count"], label=f"{name} {route or 'default'} {backend}")


@pytest.mark.parametrize("vtype", [np.int32, np.float64], ids=lambda d: np.dtype(d).name)
def test_majority_value_span_at_the_counting_limit(monkeypatch, vtype):
    """Values whose span is one below _MAJORITY_TABLE_LIMIT // n_zones (counted) and at it (hashed): the oracle's column."""
    monkeypatch.delenv("XRS_ZONAL_MAJORITY", raising=False)
    rng = np.random.default_rng(23)
    zones = zc.small_zones((48, 75), n_zones=4, seed=23)
    limit = zonal._MAJORITY_TABLE_LIMIT // 4
    for span, counted in ((limit - 1, True), (limit, False)):
        vals = np.where(rng.random(zones.shape) < 0.3 + 0.1 * zones, span - 40, -40).astype(vtype)
        staged = xs.DeviceArray.from_numpy(vals.astype(np.float64))
        assert (zonal._device_ids(staged, get_stream(), max_range=limit) is not None) == counted
        want = orc.zonal_stats(zones, vals, stats_funcs=["majority"])
        assert set(want["majority"]) == {-40.0, span - 40.0}
        for backend in ("numpy", "hip"):
            got = zonal.stats(_agg(zones, backend), _agg(vals, backend), stats_funcs=["majority"])
            zc.assert_stats_frame(got, want, ["majority"], label=f"span {span} {backend}")


def test_sharded_ids_spanning_the_sharded_range_limit():
    """World-1 row-sharded int32 zones whose ids span one below _SHARDED_RANGE_LIMIT values (mapped) and exactly that many
    (mapped: the limit is on the number of values) and one more (refused)."""
    rng = np.random.default_rng(29)
    vals = zc.small_values((40, 64), seed=29, nan_frac=0)
    for top, mapped in ((zonal._SHARDED_RANGE_LIMIT - 2, True), (zonal._SHARDED_RANGE_LIMIT - 1, True), (zonal._SHARDED_RANGE_LIMIT, False)):
        z = np.where(rng.random(vals.shape) < 0.5, top - 9, -9).astype(np.int32)
        zs, vs = xs.ShardedArray.from_numpy(z), xs.ShardedArray.from_numpy(vals)
        call = lambda: zonal.stats(xs.DataArray(zs, dims=["y", "x"]), xs.DataArray(vs, dims=["y", "x"]), stats_funcs=["count", "max"])  # noqa: E731
        if mapped:
            zc.assert_stats_frame(call(), orc.zonal_stats(z, vals, stats_funcs=["count", "max"]), ["count", "max"],
                                  zone_dtype=np.int32, label=str(top))
        else:
            with pytest.raises(NotImplementedError, match="span"):
                call()


OTHER_ZONE_DTYPES = {
    np.uint8: [0, 3, 255], np.int16: [-32768, -1, 0, 32767], np.uint32: [0, 1 << 31, (1 << 32) - 1],
    np.uint64: [0, zc.P53 + 1, 1 << 63, (1 << 63) + 1, (1 << 64) - 1],
}


@pytest.mark.parametrize("dtype", list(OTHER_ZONE_DTYPES), ids=lambda d: np.dtype(d).name)
def test_zone_dtypes_the_kernels_do_not_read(dtype):
    """Device-resident zones of a dtype outside _ZONE_DTYPE_CODE are mapped on the host, in their own dtype."""
    ids = OTHER_ZONE_DTYPES[dtype]
    z = zc.id_raster(ids, dtype=dtype, seed=17)
    v = zc.small_values(z.shape, seed=17)
    cats = zc.small_zones(z.shape, seed=17)
    got = zonal.stats(_agg(z, "hip"), _agg(v, "hip"), stats_funcs=STATS)
    zc.assert_stats_frame(got, orc.zonal_stats(z, v, stats_funcs=STATS), STATS, zone_dtype=dtype)
    assert got["zone"].tolist() == ids
    picked = np.array([ids[-1], ids[0]], dtype=dtype)
    got = zonal.stats(_agg(z, "hip"), _agg(v, "hip"), zone_ids=picked, stats_funcs=["count"])
    zc.assert_stats_frame(got, orc.zonal_stats(z, v, zone_ids=picked, stats_funcs=["count"]), ["count"])
    for zones, values in ((z, cats), (cats, z)):
        got = zonal.crosstab(_agg(zones, "hip"), _agg(values, "hip"))
        zc.assert_crosstab_frame(got, orc.crosstab_2d(zones, values), zone_dtype=zones.dtype, label=np.dtype(dtype).name)


@pytest.mark.parametrize("dtype", [np.int64, np.float64], ids=lambda d: np.dtype(d).name)
def test_ids_spanning_the_dense_range_limit(dtype):
    """Two ids whose span is one below the limit (mapped on the device) and at it (mapped on the host): the same frame."""
    rng = np.random.default_rng(19)
    for top, on_device in ((zonal._DENSE_RANGE_LIMIT - 1, True), (zonal._DENSE_RANGE_LIMIT, False)):
        z = np.where(rng.random((24, 35)) < 0.4, top - 5, -5).astype(dtype)
        v = zc.small_values(z.shape, seed=19)
        assert (zonal._device_ids(xs.DeviceArray.from_numpy(z), get_stream()) is not None) == on_device
        for backend in ("numpy", "hip"):
            got = zonal.stats(_agg(z, backend), _agg(v, backend), stats_funcs=STATS)
            zc.assert_stats_frame(got, orc.zonal_stats(z, v, stats_funcs=STATS), STATS, zone_dtype=dtype, label=f"{top} {backend}")
            assert got["zone"].tolist() == [-5, top - 5]


# ------------------------------------------------------------------------------------------------ trim / crop
@pytest.mark.parametrize("dtype", [np.int64, np.uint64], ids=lambda d: np.dtype(d).name)
def test_trim_crop_compare_64_bit_integers_as_integers(dtype):
    pairs = [(zc.P53, zc.P53 + 1)] + ([(1 << 63, (1 << 63) + 1)] if dtype == np.uint64 else [(-zc.P53, -zc.P53 - 1)])
    for even, odd in pairs:
        z = np.full((70, 300), even, dtype=dtype)
        z[12:31, 40:260] = odd
        z[60, 290] = 7
        for data in (z, xs.DeviceArray.from_numpy(z)):
            for wanted in ((odd,), (even,), (odd, 7), (7,), (7, 9), (float(7),)):
                assert zonal._match_bounds(data, wanted, False) == orc.crop_bounds(z, wanted), (dtype, wanted)
                assert zonal._match_bounds(data, wanted, True) == orc.trim_bounds(z, wanted), (dtype, wanted)
            # a wanted value given as a float is compared in float64 by NumPy too: odd and even cells both match
            wanted = (float(even),)
            assert zonal._match_bounds(data, wanted, False) == orc.crop_bounds(z, wanted) == (0, 69, 0, 299)
            assert zonal._match_bounds(data, wanted, True) == orc.trim_bounds(z, wanted) == (60, 60, 290, 290)
        assert zonal._match_bounds(z, (odd,), False) == (12, 30, 40, 259)
        for backend in ("numpy", "hip"):
            agg = _agg(z, backend)
            assert zonal.trim(agg, values=(even,)).shape == (49, 251)
            out = zonal.crop(agg, agg, zones_ids=(odd,))
            assert out.shape == (19, 220)
            data = out.data.get() if isinstance(out.data, xs.DeviceArray) else np.asarray(out.data)
            assert data.dtype == np.dtype(dtype) and (data == odd).all()

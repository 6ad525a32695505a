"""The zonal reduction kernels at the C ABI (xrspatial_amd/csrc/zonal.hip: xrs_zonal_init*, xrs_zonal_partials_*, _lut_*,
_window_*, xrs_zonal_sample_*; zonal_majority.hip: xrs_zonal_backproject_f64), one wave path at a time, against the NumPy
references of tests/zonal_partial_cases.py -- never a function of the package.

zonal_kernel picks a path per wave from the zone layout under it: the whole trip in one zone (wave_reduce, one lane adds),
rows of 16 lanes in one zone (row16_reduce), rows that straddle zones in the same wave, lane by lane, slots of more than 8
runs, a zone boundary inside a lane's 4 cells, the scalar tail.  tests/test_zonal_partials_host.py shows with a CPU model of
those paths that every case used here reaches the ones it is named for, for U = 2 and U = 4 slots per lane.

Values are multiples of 1/4 of a few thousand at most and the shift is an integer, so every partial sum of (x - shift) and
(x - shift)^2 is exact in float64 in any order, with or without a fused multiply-add: count, sum, sumsq, min and max are
compared with assert_array_equal.  The one tolerance is test_large_offset_small_spread's: m * 2^-52 * sum |t| for a zone of m
terms t, against math.fsum (derived in zonal_partial_cases.reference_fsum)."""
import numpy as np
import pytest

import xrspatial_amd as xs
from tests import zonal_partial_cases as pc
from tests.test_gpu_zonal_ids import _place
from xrspatial_amd import _lib
from xrspatial_amd._launch import get_stream

pytestmark = pytest.mark.gpu

VTYPES = [np.float32, np.float64]
vt_ids = lambda d: np.dtype(d).name  # noqa: E731
KEYS = ("count", "sum", "sumsq", "min", "max")
GUARD = 8                                             # elements in front of and behind every table


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def _sfx(dtype, init=False):
    f64 = np.dtype(dtype) == np.float64
    return ("_f64" if f64 else "") if init else ("f64" if f64 else "f32")


class Tables:
    """count u64 | sum f64 | sumsq f64 | min | max of `n_zones` zones, each in a buffer of its own with GUARD elements of a
    sentinel on either side."""
    SENTINEL = {"count": 0xABABABABABABABAB, "sum": -777.25, "sumsq": -778.25, "min": -779.25, "max": 780.25}

    def __init__(self, n_zones, dtype, init=True):
        self.n, self.dtype = n_zones, np.dtype(dtype)
        self.types = {"count": np.dtype(np.uint64), "sum": np.dtype(np.float64), "sumsq": np.dtype(np.float64),
                      "min": self.dtype, "max": self.dtype}
        self.bufs = {k: xs.DeviceArray.from_numpy(np.full(n_zones + 2 * GUARD, self.SENTINEL[k], dtype=t))
                     for k, t in self.types.items()}
        if init:
            _lib.call("xrs_zonal_init" + _sfx(dtype, init=True), *self.ptrs(), n_zones, get_stream())

    def ptrs(self, offset=0):
        return [self.bufs[k].ptr + (GUARD + offset) * self.types[k].itemsize for k in KEYS]

    def get(self):
        """The tables; the guards are checked on the way."""
        out = {}
        for k in KEYS:
            host = self.bufs[k].get(get_stream())
            want = np.array(self.SENTINEL[k], dtype=self.types[k])
            assert (host[:GUARD] == want).all() and (host[GUARD + self.n:] == want).all(), f"guard of {k} overwritten"
            out[k] = host[GUARD:GUARD + self.n]
        return out


def _nodata_args(nodata):
    return (0.0, 0) if nodata is None else (float(nodata), 1)


def _dense(z, v, n_zones, nodata, shift, tables, shifts=(0, 0)):
    zd, vd = _place(np.ascontiguousarray(z, np.int32), shifts[0]), _place(v, shifts[1])
    _lib.call("xrs_zonal_partials_" + _sfx(v.dtype), zd.ptr, vd.ptr, z.size, n_zones, *_nodata_args(nodata), float(shift),
              *tables.ptrs(), get_stream())
    return tables.get()


def _assert_tables(got, want, label, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype, (label, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{label} {k}")


def _want(case):
    return pc.reference(case.idx, case.v, case.n_zones, case.shift, case.nodata)


# ---------------------------------------------------------------------------------------------- dense partials
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_dense_partials_every_wave_path(dtype):
    """The segment layout for U = 2 (40 zones) and U = 4 (3000 / 2000 zones), without nodata, with a nodata value, with NaN
    and with +inf as the nodata value; the zone without a valid cell keeps count 0, min +inf, max -inf."""
    for case in pc.dense_cases(dtype):
        want = _want(case)
        got = _dense(case.z, case.v, case.n_zones, case.nodata, case.shift, Tables(case.n_zones, dtype))
        _assert_tables(got, want, case.name)
        dead = case.extra["dead"]
        assert got["count"][dead] == 0 and got["sum"][dead] == 0 and got["sumsq"][dead] == 0, case.name
        assert got["min"][dead] == np.inf and got["max"][dead] == -np.inf, case.name
        assert int(got["count"].sum()) < case.z.size - 1000, case.name           # (cells were left out)


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_init_guards_and_accumulation(dtype):
    """xrs_zonal_init* on zone counts that are no multiple of 256, the elements around the tables, and two calls on the two
    halves of a raster against one call on the whole."""
    for n_zones in (1, 255, 257, 3000):
        t = Tables(n_zones, dtype)
        got = t.get()
        assert (got["count"] == 0).all() and (got["sum"] == 0).all() and (got["sumsq"] == 0).all(), n_zones
        assert (got["min"] == np.inf).all() and (got["max"] == -np.inf).all(), n_zones
    for case in (pc.dense_cases(dtype)[1], pc.dense_cases(dtype)[5]):              # U = 2 and U = 4, nodata 17
        assert case.nodata == 17.0
        want = _want(case)
        whole = _dense(case.z, case.v, case.n_zones, case.nodata, case.shift, Tables(case.n_zones, dtype))
        for cut in (case.z.size // 2 // 4 * 4, 3 * pc.RUN_LONG + 100, 7):
            t = Tables(case.n_zones, dtype)
            _dense(case.z[:cut], case.v[:cut], case.n_zones, case.nodata, case.shift, t)
            halves = _dense(case.z[cut:], case.v[cut:], case.n_zones, case.nodata, case.shift, t)
            _assert_tables(halves, whole, f"{case.name} cut at {cut}")
        _assert_tables(whole, want, case.name)
        # a second call on the same tables adds the same again
        t = Tables(case.n_zones, dtype)
        _dense(case.z, case.v, case.n_zones, case.nodata, case.shift, t)
        twice = _dense(case.z, case.v, case.n_zones, case.nodata, case.shift, t)
        np.testing.assert_array_equal(twice["count"], 2 * want["count"])
        np.testing.assert_array_equal(twice["sum"], 2 * want["sum"])
        np.testing.assert_array_equal(twice["sumsq"], 2 * want["sumsq"])
        _assert_tables(twice, want, case.name, keys=("min", "max"))


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_alignment_and_tails(dtype):
    """Both planes 16-byte aligned, only the zone plane, only the value plane (the last two: every cell through the scalar
    tail), at lengths around the 16-byte slot, the wave and the trip."""
    for case in pc.tail_cases(dtype):
        want = _want(case)
        for shifts in pc.ALIGN:
            got = _dense(case.z, case.v, case.n_zones, case.nodata, case.shift, Tables(case.n_zones, dtype), shifts)
            _assert_tables(got, want, f"{case.name} shifts={shifts}")
    # a table of more than 64 KiB with a plane that is not aligned: the scalar kernel again
    case = pc.dense_cases(dtype)[5]
    want = _want(case)
    for shifts in pc.ALIGN[1:]:
        got = _dense(case.z, case.v, case.n_zones, case.nodata, case.shift, Tables(case.n_zones, dtype), shifts)
        _assert_tables(got, want, f"{case.name} shifts={shifts}")


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_several_zone_windows(dtype):
    """12 000 / 9 000 zones: three launches with zbase 0, w, 2 w; long runs of the indices on both sides of every window
    boundary.  Every zone lands in its own slice, nothing lands twice."""
    case = pc.windows_case(dtype)
    want = _want(case)
    for shifts in pc.ALIGN[:2]:
        got = _dense(case.z, case.v, case.n_zones, case.nodata, case.shift, Tables(case.n_zones, dtype), shifts)
        _assert_tables(got, want, f"{case.name} shifts={shifts}")
        w = pc.launch_window(dtype)
        for zone in (w - 1, w, 2 * w - 1, 2 * w, case.n_zones - 2, 0):
            assert got["count"][zone] > 1900, zone                                 # (a 2048-cell run, a few invalid)
        assert got["count"][case.extra["dead"]] == 0
        assert int(got["count"].sum()) == int((case.ok & (case.idx >= 0) & (case.idx < case.n_zones)).sum())


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_min_max_at_the_ends_of_the_format(dtype):
    """Zones of +-0.0 only, of subnormals, of +-FLT_MAX / +-DBL_MAX / 2: through the wave and row folds, the LDS float atomics
    and the CAS loop of the flush unchanged.  Compared with ==, so -0.0 equals +0.0."""
    case = pc.edge_cases(dtype)
    want = _want_min_max(case)
    for shifts in pc.ALIGN[:2]:
        got = _dense(case.z, case.v, case.n_zones, None, 0.0, Tables(case.n_zones, dtype), shifts)
        _assert_tables(got, want, f"{case.name} shifts={shifts}", keys=("count", "min", "max"))
    fi = np.finfo(dtype)
    big = fi.max if dtype == np.float32 else fi.max / 2
    assert want["min"].tolist() == [0.0, -fi.smallest_subnormal, fi.smallest_subnormal, -1.0, -big, 2.0, -big]
    assert want["max"].tolist() == [0.0, 3 * fi.smallest_subnormal, 1.0, -fi.smallest_subnormal, big, big, -2.0]


def _want_min_max(case):
    """count, min and max only (the sums of such values are not exact): np.bincount / np.minimum.at / np.maximum.at."""
    zi = case.idx.astype(np.int64)
    mn, mx = np.full(case.n_zones, np.inf, case.v.dtype), np.full(case.n_zones, -np.inf, case.v.dtype)
    np.minimum.at(mn, zi, case.v)
    np.maximum.at(mx, zi, case.v)
    return {"count": np.bincount(zi, minlength=case.n_zones).astype(np.uint64), "min": mn, "max": mx}


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_large_offset_small_spread(dtype):
    """3e5 +- 0.05 (float32) / 1e7 +- 1e-3 (float64) with the shift near the mean: sum and sumsq within m * 2^-52 * sum |t| of
    math.fsum of the float64 terms."""
    case = pc.conditioning_case(dtype)
    got = _dense(case.z, case.v, case.n_zones, None, case.shift, Tables(case.n_zones, dtype))
    s, q, bound_s, bound_q = pc.reference_fsum(case.idx, case.v, case.n_zones, case.shift)
    err_s, err_q = np.abs(got["sum"] - s), np.abs(got["sumsq"] - q)
    drawn = got["count"] > 0                                         # (the layout's last zone is drawn nowhere: 0 <= 0 there)
    print(f"{np.dtype(dtype).name}: max |sum - fsum| / bound = {np.max(err_s[drawn] / bound_s[drawn]):.3g}, "
          f"max |sumsq - fsum| / bound = {np.max(err_q[drawn] / bound_q[drawn]):.3g}")
    assert drawn.sum() == case.n_zones - 1 and (bound_s[drawn] > 0).all()
    assert (err_s <= bound_s).all() and (err_q <= bound_q).all()
    _assert_tables(got, _want_min_max_valid(case), case.name, keys=("count", "min", "max"))


def _want_min_max_valid(case):
    ok = case.ok & (case.idx >= 0) & (case.idx < case.n_zones)
    zi, x = case.idx[ok].astype(np.int64), case.v[ok]
    mn, mx = np.full(case.n_zones, np.inf, case.v.dtype), np.full(case.n_zones, -np.inf, case.v.dtype)
    np.minimum.at(mn, zi, x)
    np.maximum.at(mx, zi, x)
    return {"count": np.bincount(zi, minlength=case.n_zones).astype(np.uint64), "min": mn, "max": mx}


# ------------------------------------------------------------------------------------------------- LUT variant
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_lut_variant_equals_the_dense_call_on_host_mapped_indices(dtype):
    """Raw ids with gaps through the table: zone_min positive, negative and INT32_MIN, ids below and above the table's window
    (INT32_MAX with a negative zone_min among them), table entries of -1, more zones than one launch holds."""
    for case in pc.lut_cases(dtype):
        e = case.extra
        lut = xs.DeviceArray.from_numpy(e["lut"])
        want = _want(case)
        for shifts in pc.ALIGN[:2]:
            t = Tables(case.n_zones, dtype)
            zd, vd = _place(case.z, shifts[0]), _place(case.v, shifts[1])
            _lib.call("xrs_zonal_partials_lut_" + _sfx(dtype), zd.ptr, int(e["zone_min"]), int(e["zone_range"]), lut.ptr, vd.ptr,
                      case.z.size, case.n_zones, *_nodata_args(case.nodata), float(case.shift), *t.ptrs(), get_stream())
            got = t.get()
            dense = _dense(case.idx, case.v, case.n_zones, case.nodata, case.shift, Tables(case.n_zones, dtype), shifts)
            _assert_tables(got, dense, f"{case.name} shifts={shifts} against the dense call")
            _assert_tables(got, want, f"{case.name} shifts={shifts}")
        assert got["count"][e["dead"]] == 0 and (got["count"] > 0).sum() >= min(case.n_zones - 1, 39), case.name


# ---------------------------------------------------------------------------------------------- window variant
class WindowBuffers(Tables):
    """Tables that hold garbage (the ABI overwrites them), the present bytes between guards, the overflow flag."""

    def __init__(self, window, dtype):
        super().__init__(window, dtype, init=False)
        self.present = xs.DeviceArray.from_numpy(np.full(window + 2 * GUARD, 0xAA, np.uint8))
        self.overflow = xs.DeviceArray.from_numpy(np.array([-7, -7], np.int32))

    def call(self, case, shifts=(0, 0), window=None, base=None):
        e = case.extra
        zd, vd = _place(case.z, shifts[0]), _place(case.v, shifts[1])
        _lib.call("xrs_zonal_partials_window_" + _sfx(self.dtype), zd.ptr, int(e["base"] if base is None else base),
                  int(e["window"] if window is None else window), vd.ptr, case.z.size, *_nodata_args(case.nodata), float(case.shift),
                  *self.ptrs(), self.present.ptr + GUARD, self.overflow.ptr, get_stream())
        present = self.present.get(get_stream())
        assert (present[:GUARD] == 0xAA).all() and (present[GUARD + self.n:] == 0xAA).all(), "guard of present overwritten"
        flag = self.overflow.get(get_stream())
        assert flag[1] == -7
        return self.get(), present[GUARD:GUARD + self.n], int(flag[0])


def _check_window(case, shifts):
    e = case.extra
    window = e["window"]
    want = _want(case)
    inside = case.idx >= 0
    ids_seen = np.isin(np.arange(window), np.unique(case.idx[inside]))
    some_invalid = np.isin(np.arange(window), np.unique(case.idx[inside & ~case.ok]))
    all_invalid = ids_seen & (want["count"] == 0)
    assert all_invalid[e["dead"]]                                    # (a large window has a few more by chance)
    buffers = WindowBuffers(window, case.dtype)
    for call in (1, 2):                                              # (overwritten, not accumulated)
        label = f"{case.name} shifts={shifts} call {call}"
        got, present, overflow = buffers.call(case, shifts)
        assert overflow == int("stray" in e), label
        _assert_tables(got, want, label)
        assert set(np.unique(present)) <= {0, 1}, label
        assert (present[all_invalid] == 1).all(), label
        assert not (present.astype(bool) & ~some_invalid).any(), label
        if "stray" not in e:
            np.testing.assert_array_equal((got["count"] > 0) | (present > 0), ids_seen, err_msg=label)


@pytest.mark.parametrize("window", pc.WINDOW_SIZES)
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_window_variant_all_ids_inside(dtype, window):
    """Bases 0, far from 0, negative, -2^31 and 2^31 - window; one id whose cells are all invalid in a 2048-cell run, in a
    100-cell run, in the n % 4 tail: overflow stays 0, the tables equal the reference, present | count > 0 is np.unique."""
    for case in pc.window_cases(dtype):
        if case.extra["window"] != window:
            continue
        _check_window(case, (0, 0))
        if case.extra["dead_at"] != "long" or case.extra["base"] < 0:
            _check_window(case, (1, 0))


@pytest.mark.parametrize("window", pc.WINDOW_SIZES)
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_window_variant_one_stray_id(dtype, window):
    """ONE cell with an id outside the window -- inside a long run of one id, among scattered ids, as the last cell of the
    scalar tail, at the other end of int32 for the two extreme bases: overflow is 1 and the cell is counted nowhere."""
    for case in pc.stray_cases(dtype):
        if case.extra["window"] != window:
            continue
        for shifts in pc.ALIGN[:2]:
            _check_window(case, shifts)


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_window_above_the_launch_limit_is_refused_without_a_launch(dtype):
    case = pc.window_case(dtype, "zero", 256)
    limit = pc.launch_window(dtype)
    buffers = WindowBuffers(limit + 1, dtype)
    with pytest.raises(_lib.XrsError, match="at most %d ids" % limit):
        buffers.call(case, window=limit + 1)
    for k in KEYS:                                                   # nothing ran: the tables hold what they held
        host = buffers.bufs[k].get(get_stream())
        assert (host == np.array(Tables.SENTINEL[k], dtype=host.dtype)).all(), k
    assert (buffers.present.get(get_stream()) == 0xAA).all() and buffers.overflow.get(get_stream()).tolist() == [-7, -7]
    with pytest.raises(_lib.XrsError, match="empty window"):
        buffers.call(case, window=0)
    # the limit itself is a window like any other
    buffers = WindowBuffers(limit, dtype)
    got, present, overflow = buffers.call(case, window=limit)
    assert overflow == 0
    want = pc.reference(case.idx, case.v, limit, case.shift, case.nodata)
    _assert_tables(got, want, "window at the limit")


# ------------------------------------------------------------------------------------------------------- sample
SAMPLE_N = (1, 5, 1000, 65_536, 65_537, 100_000, 131_072, 200_003)
N_SAMPLES = 65_536


def _sample(zones, vals, nodata=None, shifts=(0, 0)):
    res = xs.DeviceArray.from_numpy(np.full(4, -123.0))
    zd, vd = _place(zones, shifts[0]), _place(vals, shifts[1])
    _lib.call("xrs_zonal_sample_" + _sfx(vals.dtype), zd.ptr, vd.ptr, zones.size, N_SAMPLES, *_nodata_args(nodata), res.ptr,
              get_stream())
    raw = res.get(get_stream())
    assert raw[3] == -123.0                                          # (24 bytes, not 32)
    zmin, zmax = (int(x) for x in raw[:1].view(np.int32))
    return zmin, zmax, float(raw[1]), int(raw[2:3].view(np.uint64)[0])


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_sample_reaches_both_ends_of_the_raster(dtype):
    """zones[i] = i: zmin and zmax are the lowest and highest sampled positions.  (A sample that divided n by n_samples
    rounding down looked at the first n_samples cells only when 64 K < n < 128 K.)"""
    for n in SAMPLE_N:
        zones = np.arange(n, dtype=np.int32)
        stride = -(-n // N_SAMPLES) | 1
        taken = min(n, N_SAMPLES)
        for shifts in ((0, 0), (1, 1)):
            zmin, zmax, total, n_valid = _sample(zones, np.ones(n, dtype), shifts=shifts)
            assert 0 <= zmin < 2 * stride and n - 2 * stride <= zmax < n, (n, stride, zmin, zmax)
            assert n_valid == taken and total == float(taken), (n, n_valid, total)
        for vals, nodata in ((np.full(n, np.nan, dtype), None), (np.full(n, 17.0, dtype), 17.0), (np.full(n, np.inf, dtype), 3.0)):
            zmin, zmax, total, n_valid = _sample(zones, vals, nodata)
            assert (n_valid, total) == (0, 0.0) and 0 <= zmin < 2 * stride and n - 2 * stride <= zmax < n, (n, nodata)
        # values 17 with nodata 17 given but switched off are values
        assert _sample(zones, np.full(n, 17.0, dtype))[2:] == (17.0 * taken, taken)


# -------------------------------------------------------------------------------------------------- backproject
@pytest.mark.parametrize("n_stats", [1, 8])
def test_backproject(n_stats):
    """out[s, i] = table[s, idx[i]], NaN where the cell has no zone; the output plane one element past a 16-byte boundary."""
    rng = np.random.default_rng(91)
    n_zones = 37
    table = rng.integers(-1000, 1000, (n_stats, n_zones)) * 0.25
    table[0, 3], table[-1, 5], table[0, 7] = np.nan, np.inf, -0.0
    tdev = xs.DeviceArray.from_numpy(table)
    for n in pc.TAILS:
        idx = rng.integers(-1, n_zones + 1, n).astype(np.int32)
        idx[0] = n_zones if n % 2 else -1
        no_zone = (idx < 0) | (idx >= n_zones)
        want = np.where(no_zone[None, :], np.nan, table[:, np.clip(idx, 0, n_zones - 1)])
        for shift in (0, 1):
            out = xs.DeviceArray.from_numpy(np.full(n_stats * n + 2 + GUARD, -5.5))
            idev = _place(idx, shift)
            _lib.call("xrs_zonal_backproject_f64", idev.ptr, n, tdev.ptr, n_stats, n_zones, out.ptr + 8, get_stream())
            host = out.get(get_stream())
            np.testing.assert_array_equal(host[1:1 + n_stats * n].reshape(n_stats, n), want, err_msg=f"n={n} shift={shift}")
            assert host[0] == -5.5 and (host[1 + n_stats * n:] == -5.5).all(), (n, shift)

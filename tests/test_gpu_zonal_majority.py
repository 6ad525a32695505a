"""zonal `majority` on continuous data at the C ABI, path by path: xrs_zonal_mode_* (xrspatial_amd/csrc/zonal_mode.hip: cells
routed by zone, then by a hash of the value, counted in LDS hash tables) and xrs_zonal_majority_* (zonal_majority.hip: two
radix sorts and run voting) on the cases of tests/zonal_majority_cases.py, against np.unique + the first argmax per zone --
never a function of the package.  The entry points xrs_zonal_group_* and xrs_zonal_backproject_f64 of the same file too.

There is no tolerance: the winner is selected, not computed.  Every result equals the reference value for value with NaN in
the same places, and the two device paths equal each other bit for bit (a zero that wins is +0.0 on both).  After every
xrs_zonal_mode_* call the first five words of the workspace (n_valid, n_parts, n_chunks, overflow, n_direct: include/xrs_hip.h)
must equal what the CPU model of the plan says for the case: that is how a case proves which kernels it went through.
tests/test_zonal_majority_host.py shows without a GPU that the model puts every case on the path it is named for."""
import functools

import numpy as np
import pytest

import xrspatial_amd as xs
from tests import parity_log
from tests import zonal_majority_cases as mc
from xrspatial_amd import _lib, zonal
from xrspatial_amd._launch import get_stream

pytestmark = pytest.mark.gpu

VTYPES = [np.float32, np.float64]
vt_ids = lambda d: np.dtype(d).name  # noqa: E731
GUARD = 4                                             # doubles in front of and behind the results
SENTINEL = -4242.5
GARBAGE_LIMIT = 64 << 20                              # workspaces up to this size are filled with 0xA5 before the call


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def _sfx(dtype):
    return "f64" if np.dtype(dtype) == np.float64 else "f32"


def _nodata_args(nodata):
    return (0.0, 0) if nodata is None else (float(nodata), 1)


def _workspace(nbytes):
    if nbytes <= GARBAGE_LIMIT:
        return xs.DeviceArray.from_numpy(np.full(nbytes, 0xA5, np.uint8))
    return xs.DeviceArray((nbytes,), np.uint8)


def _results(out, n):
    """The `n` doubles between the guards."""
    host = out.get(get_stream())
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "guard of the results overwritten"
    return host[GUARD:GUARD + n]


class Staged:
    """A case's planes in HBM, staged once for all the calls on them."""

    def __init__(self, case):
        self.case, self.dtype = case, case.v.dtype
        self.z = xs.DeviceArray.from_numpy(np.ascontiguousarray(case.z.ravel()))
        self.v = xs.DeviceArray.from_numpy(np.ascontiguousarray(case.v.ravel()))

    def mode(self, counts=None, nz=None, short=0, out_ptr=True):
        """xrs_zonal_mode_*: (results, the double behind them, the five header words); self.zone_count: the valid cells per
        zone as the workspace holds them (behind the 256-byte header: Plan::off_zone_count)."""
        case = self.case
        nz = case.nz if nz is None else nz
        f64 = int(self.dtype == np.float64)
        nbytes = int(_lib.load().xrs_zonal_mode_workspace_bytes(case.n, nz, f64))
        work = _workspace(nbytes)
        out = xs.DeviceArray.from_numpy(np.full(nz + 1 + 2 * GUARD, SENTINEL))
        cdev = None if counts is None else xs.DeviceArray.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32))
        _lib.call("xrs_zonal_mode_" + _sfx(self.dtype), self.z.ptr, self.v.ptr, case.n, nz, *_nodata_args(case.nodata),
                  None if cdev is None else cdev.ptr, work.ptr, nbytes - short, out.ptr + 8 * GUARD if out_ptr else None,
                  get_stream())
        res = _results(out, nz + 1)
        hdr = np.zeros(5, np.uint32)
        _lib.call("xrs_memcpy_d2h", hdr.ctypes.data, work.ptr, hdr.nbytes, get_stream())
        self.zone_count = np.zeros(nz, np.uint32)
        if nz:
            _lib.call("xrs_memcpy_d2h", self.zone_count.ctypes.data, work.ptr + 256, self.zone_count.nbytes, get_stream())
        _lib.call("xrs_stream_sync", get_stream())
        return res[:nz], float(res[nz]), [int(x) for x in hdr]

    def sort(self, nz=None, short=0, out_ptr=True):
        case = self.case
        nz = case.nz if nz is None else nz
        nbytes = int(_lib.load().xrs_zonal_majority_workspace_bytes(case.n, nz, int(self.dtype == np.float64)))
        work = _workspace(nbytes)
        out = xs.DeviceArray.from_numpy(np.full(nz + 2 * GUARD, SENTINEL))
        _lib.call("xrs_zonal_majority_" + _sfx(self.dtype), self.z.ptr, self.v.ptr, case.n, nz, *_nodata_args(case.nodata),
                  work.ptr, nbytes - short, out.ptr + 8 * GUARD if out_ptr else None, get_stream())
        return _results(out, nz)


def _same_bits(a, b, label):
    """Bit for bit, NaN where NaN is (whatever its payload); a zero is +0.0."""
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=label)
    fin = ~np.isnan(a)
    np.testing.assert_array_equal(a[fin].view(np.uint64), b[fin].view(np.uint64), err_msg=label)
    assert not np.signbit(a[fin][a[fin] == 0]).any(), label


def _check(case, both_counts=True):
    """Both device paths on `case` against the reference and the model; returns the model."""
    m = mc.model(case)
    assert not m.overflow, case.name
    want = case.want()
    st = Staged(case)
    sfx = _sfx(case.v.dtype)
    got_sort = st.sort()
    parity_log.record("zonal_majority/" + case.name, "sort_" + sfx, got_sort, want, tol=0.0)
    np.testing.assert_array_equal(got_sort, want, err_msg=f"{case.name}: sort against np.unique")
    first = None
    for counts in ((None, m.counts) if both_counts else (None,)):
        label = f"{case.name}: hash, counts {'given' if counts is not None else 'counted'}"
        got, overflow, hdr = st.mode(counts)
        print(f"{label}: header {hdr}, model {m.header}")
        parity_log.record("zonal_majority/" + case.name, "mode_" + sfx, got, want, tol=0.0)
        assert (hdr[0], hdr[1], hdr[2], hdr[4]) == m.header, label
        np.testing.assert_array_equal(st.zone_count, m.counts, err_msg=label)      # (before they are handed back in)
        assert hdr[3] == 0 and overflow == 0.0, label
        np.testing.assert_array_equal(got, want, err_msg=label + " against np.unique")
        _same_bits(got, got_sort, label + " against the sort")
        first = got if first is None else first
        _same_bits(got, first, label + " against counts counted")
    for zone, w in case.winners.items():
        np.testing.assert_array_equal(got_sort[zone], w, err_msg=f"{case.name} zone {zone}")
    return m


# ---------------------------------------------------------------------------------------------------- the paths
@functools.lru_cache(maxsize=None)
def _small(dtype):
    return {case.name: case for case in mc.small_cases(dtype)}


@pytest.mark.parametrize("name", mc.SMALL_NAMES)
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_small_case_on_both_paths(dtype, name):
    """Uncut zones of one and two batches, the B boundaries, many chunks with a partial one, 512 parts, 16 384 zones, a
    dominated part, the table filled to its last slot, ties at every level, the wave paths of the zone passes at n = 1 ..
    4097, the zone bits of the second sort, run votes across zone changes and workgroups."""
    _check(_small(dtype)[name])


@pytest.mark.parametrize("nz", mc.SCAN_NZ)
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_plan_scans_carry_across_trips(dtype, nz):
    """nz = 1, 1024, 1025, 2049 zones of 1281 / 0 / 1 cells in turn: key offsets, part bases and chunk bases."""
    _check(mc.scan_carry_case(dtype, nz))


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_lds_histogram_against_direct_kernels(dtype, direct):
    """A zone of exactly 2 097 152 valid cells (2^11 parts: n_direct == 0, the DIRECT kernels launch and leave) and one of
    2 097 153 (2^12 parts: n_direct == 1), each beside small zones."""
    m = _check(mc.lds_b_case(dtype, direct), both_counts=False)
    assert m.n_direct == direct


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_persistent_count_loop(dtype):
    """4096 * 4096 + 4097 cells: every workgroup of zone_count_kernel takes a second tile; counted here and supplied."""
    m = _check(mc.persistent_case(dtype))
    assert m.n_direct == 3


# ----------------------------------------------------------------------------------------------------- overflow
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_overflow_is_reported_and_python_sorts(dtype, monkeypatch):
    """SLOTS + 1 keys for the table of one part, and 6000 distinct values that all hash to one part of a 6001-cell zone: the
    double behind the zones is the header's overflow word and at least 1; the sort answers; zonal_majority forced onto the
    hash path and zonal.stats (which hands its counts over) both return the reference."""
    for case in mc.overflow_cases(dtype):
        m = mc.model(case)
        assert m.overflow, case.name
        want = case.want()
        st = Staged(case)
        for counts in (None, m.counts):
            got, overflow, hdr = st.mode(counts)
            print(f"{case.name}: header {hdr}, model {m.header}, double behind the zones {overflow}")
            assert (hdr[0], hdr[1], hdr[2], hdr[4]) == m.header, case.name
            np.testing.assert_array_equal(st.zone_count, m.counts, err_msg=case.name)
            assert overflow >= 1 and overflow == hdr[3], case.name
            base = np.cumsum(np.concatenate([[0], 1 << m.B]))
            fits = np.array([(m.table_keys[base[i]:base[i + 1]] <= mc.SLOTS).all() for i in range(case.nz)])
            assert not fits.all(), case.name
            np.testing.assert_array_equal(got[fits], want[fits], err_msg=case.name + ": zones that did not overflow")
        got_sort = st.sort()
        parity_log.record("zonal_majority/" + case.name, "sort_" + _sfx(dtype), got_sort, want, tol=0.0)
        np.testing.assert_array_equal(got_sort, want, err_msg=case.name)
        monkeypatch.setenv("XRS_ZONAL_MAJORITY", "hash")
        for counts in (None, m.counts):
            got = zonal.zonal_majority(case.z, case.v, case.nz, case.nodata, counts=counts)
            np.testing.assert_array_equal(got, want, err_msg=case.name + ": zonal_majority")
            _same_bits(got, got_sort, case.name)
        monkeypatch.delenv("XRS_ZONAL_MAJORITY")
        with np.errstate(all="ignore"):
            frame = zonal.stats(xs.DataArray(xs.DeviceArray.from_numpy(case.z.reshape(1, -1)), dims=["y", "x"]),
                                xs.DataArray(xs.DeviceArray.from_numpy(case.v.reshape(1, -1)), dims=["y", "x"]),
                                stats_funcs=["majority", "count"])
        assert list(frame["zone"]) == list(range(case.nz)), case.name
        np.testing.assert_array_equal(np.asarray(frame["majority"], dtype=np.float64), want, err_msg=case.name + ": zonal.stats")
        np.testing.assert_array_equal(np.asarray(frame["count"]), m.counts, err_msg=case.name)
        parity_log.record("zonal_majority/" + case.name, "stats_" + _sfx(dtype), np.asarray(frame["majority"], dtype=np.float64),
                          want, tol=0.0)


# ------------------------------------------------------------------------------------------- refusals and edges
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_refusals_and_edges(dtype, monkeypatch):
    assert int(_lib.load().xrs_zonal_mode_max_zones()) == mc.MAX_ZONES
    case = mc.lds_limit_case(dtype, mc.MAX_ZONES + 1)
    st = Staged(case)
    with pytest.raises(_lib.XrsError, match="at most %d zones" % mc.MAX_ZONES):
        st.mode()
    monkeypatch.setenv("XRS_ZONAL_MAJORITY", "hash")                 # ... and Python takes the sort without asking
    want = case.want()
    np.testing.assert_array_equal(zonal.zonal_majority(case.z, case.v, case.nz), want)
    np.testing.assert_array_equal(st.sort(), want)
    small = Staged(mc.wave_case(dtype, 65))
    with pytest.raises(_lib.XrsError, match="workspace too small"):
        small.mode(short=1)
    with pytest.raises(_lib.XrsError, match="xrs_zonal_majority: workspace too small"):
        small.sort(short=1)
    with pytest.raises(_lib.XrsError, match="xrs_zonal_mode: null output"):
        small.mode(out_ptr=False)
    with pytest.raises(_lib.XrsError, match="xrs_zonal_majority: null output"):
        small.sort(out_ptr=False)
    # no zone: the single double (the overflow count) is 0, nothing else is written
    got, overflow, _ = small.mode(nz=0)
    assert got.size == 0 and overflow == 0.0
    assert small.sort(nz=0).size == 0
    # no cell: every zone NaN, overflow 0
    empty = Staged(mc.Case("no cell", np.zeros(0, np.int32), np.zeros(0, dtype), 7))
    got, overflow, hdr = empty.mode()
    assert np.isnan(got).all() and got.size == 7 and overflow == 0.0 and hdr == [0, 7, 0, 0, 0]
    got = empty.sort()
    assert np.isnan(got).all() and got.size == 7


# ------------------------------------------------------------------------------------------------------ grouping
@pytest.mark.parametrize("n", [1, 257, 10_000])
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_group_orders_by_zone_then_value(dtype, n):
    """xrs_zonal_group_*: the valid cells by (zone, value) with -0.0 before +0.0, then NaN for every invalid cell."""
    rng = np.random.default_rng(n)
    for nz in (1, 4, 300):
        z = rng.integers(-1, nz + 1, n).astype(np.int32)
        v = (rng.integers(-6, 7, n) * 0.25).astype(dtype)
        v[rng.random(n) < 0.3] *= -1                                 # (-0.0 among them)
        u = rng.random(n)
        v[u < 0.05] = np.nan
        v[(u >= 0.05) & (u < 0.08)] = np.inf
        v[(u >= 0.08) & (u < 0.1)] = 1.25
        if n > 1:
            z[:2], v[:2] = 0, [0.0, -0.0]
        ok = mc.valid_mask(z, v, nz, 1.25)
        order = np.lexsort((mc.enc(v[ok]), z[ok]))
        want = np.concatenate([v[ok][order], np.full(n - int(ok.sum()), np.nan, dtype)])
        nbytes = int(_lib.load().xrs_zonal_majority_workspace_bytes(n, nz, int(dtype == np.float64)))
        work = _workspace(nbytes)
        out = xs.DeviceArray.from_numpy(np.full(n + 2 * GUARD, SENTINEL, dtype))
        zd, vd = xs.DeviceArray.from_numpy(z), xs.DeviceArray.from_numpy(v)
        _lib.call("xrs_zonal_group_" + _sfx(dtype), zd.ptr, vd.ptr, n, nz, 1.25, 1, work.ptr, nbytes,
                  out.ptr + GUARD * np.dtype(dtype).itemsize, get_stream())
        host = out.get(get_stream())
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
        got = host[GUARD:GUARD + n]
        U = np.uint32 if dtype == np.float32 else np.uint64
        valid = int(ok.sum())
        np.testing.assert_array_equal(got[:valid].view(U), want[:valid].view(U), err_msg=f"n={n} nz={nz}")
        assert np.isnan(got[valid:]).all(), (n, nz)
        parity_log.record(f"zonal_group/n={n} nz={nz}", "group_" + _sfx(dtype), got, want, tol=0.0)
        if n > 1:                                                    # (zone 0 holds both zeros: -0.0 comes first)
            zeros = np.flatnonzero(got[:int((z[ok] == 0).sum())] == 0)
            assert np.signbit(got[zeros[0]]) and not np.signbit(got[zeros[-1]]), (n, nz)


@pytest.mark.parametrize("n_stats", [1, 3])
def test_backproject_on_its_own(n_stats):
    """out[s, i] = table[s, idx[i]]; NaN where the cell lies outside the table."""
    rng = np.random.default_rng(7)
    nz = 11
    table = rng.integers(-50, 50, (n_stats, nz)) * 0.5
    table[0, 2], table[-1, 4] = -0.0, np.inf
    tdev = xs.DeviceArray.from_numpy(table)
    for n in (1, 255, 256, 1031):
        idx = rng.integers(-2, nz + 2, n).astype(np.int32)
        idx[0] = nz
        outside = (idx < 0) | (idx >= nz)
        want = np.where(outside[None, :], np.nan, table[:, np.clip(idx, 0, nz - 1)])
        out = xs.DeviceArray.from_numpy(np.full(n_stats * n + 2 * GUARD, SENTINEL))
        idev = xs.DeviceArray.from_numpy(idx)
        _lib.call("xrs_zonal_backproject_f64", idev.ptr, n, tdev.ptr, n_stats, nz, out.ptr + 8 * GUARD, get_stream())
        got = _results(out, n_stats * n).reshape(n_stats, n)
        np.testing.assert_array_equal(got, want, err_msg=f"n={n}")
        np.testing.assert_array_equal(np.signbit(got), np.signbit(want), err_msg=f"n={n}")
        parity_log.record(f"zonal_backproject/n={n}", f"backproject_{n_stats}", got, want, tol=0.0)

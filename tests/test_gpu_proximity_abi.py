"""xrs_proximity at the C ABI (xrspatial_amd/csrc/proximity.hip) -- never a function of the package: the scan's planes read
back from the workspace, the row list, the half calls, the three-plane mode, and the search against the rule
(tests/proximity_oracle.py) on the cases of tests/proximity_cases.py.  tests/test_proximity_cases_host.py shows on the CPU
that every case reaches what it is named for.

The workspace layout is documented ABI (include/xrs_hip.h); `proximity_cases.layout` mirrors it and its total
is held against xrs_proximity_workspace_bytes in every call.  The workspace and every output plane lie between GUARD elements
of a sentinel, checked after every call.  `list` is compared up to `count` only.

Tolerances are those derived in tests/test_gpu_proximity.py, unchanged (its `_check`): EUCLIDEAN / MANHATTAN `proximity` and
`allocation` bit for bit, `direction` within 1 float32 ulp and exactly 0 at targets; GREAT_CIRCLE `proximity` within 1 ulp,
`allocation` / `direction` where the rule's best and second-best target are more than 2 ulp apart, at most 0.5 % of a case's
cells left out.  The scan is integer work: assert_array_equal."""
import numpy as np
import pytest

import xrspatial_amd as xs
from tests import parity_log
from tests import proximity_cases as pc
from tests import proximity_oracle as po
from tests.test_gpu_proximity import GC_GAP_ULP, _check
from xrspatial_amd import _lib
from xrspatial_amd._launch import get_stream

pytestmark = pytest.mark.gpu

GUARD = 64                                            # elements in front of and behind the workspace and every output
WORK_SENTINEL = 0x5A5A5A5A
OUT_SENTINEL = np.float32(-777.25)
PRODUCTS = ("proximity", "allocation", "direction")   # modes 0, 1, 2; mode 3: the three planes in this order
ALL_THREE = 3


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Call:
    """One raster on the device with its coordinates (degrees, radians and cosines, as the host uploads them), its target
    values and a workspace between guards."""

    def __init__(self, z, xc, yc, tv=None):
        self.z = np.ascontiguousarray(z)
        self.rows, self.cols = self.z.shape
        self.cells = self.rows * self.cols
        xc, yc = np.asarray(xc, np.float64), np.asarray(yc, np.float64)
        tv = np.zeros(0, np.float64) if tv is None else np.asarray(tv)
        self.n_values, self.kind = int(tv.size), pc.VALUES_KIND[tv.dtype]
        lat = np.radians(yc)
        self.aux = xs.DeviceArray.from_numpy(np.concatenate([xc, yc, np.radians(xc), lat, np.cos(lat), tv.view(np.float64)]))
        self.data = xs.DeviceArray.from_numpy(self.z)
        self.lay = pc.layout(self.rows, self.cols)
        assert self.lay["total"] == _lib.workspace_bytes("proximity", self.rows, self.cols)
        self.work = xs.DeviceArray.from_numpy(np.full(self.lay["total"] // 4 + 2 * GUARD, WORK_SENTINEL, np.int32))

    def run(self, mode, metric="EUCLIDEAN", md=np.inf, with_out=True):
        """One call of xrs_proximity; the output planes (None without an output buffer).  Both guards are checked."""
        planes = 3 if mode & 3 == ALL_THREE else 1
        out = xs.DeviceArray.from_numpy(np.full(planes * self.cells + 2 * GUARD, OUT_SENTINEL, np.float32)) if with_out else None
        a, r, c = self.aux.ptr, self.rows, self.cols
        _lib.call("xrs_proximity", self.data.ptr, pc.DTYPE_CODE[self.z.dtype], r, c, a, a + 8 * c, a + 8 * (c + r),
                  a + 8 * (2 * c + 3 * r) if self.n_values else None, self.kind, self.n_values, float(md), po.METRICS[metric], mode,
                  self.work.ptr + 4 * GUARD, out.ptr + 4 * GUARD if with_out else None, get_stream())
        self.workspace()
        if not with_out:
            return None
        host = out.get(get_stream())
        assert (host[:GUARD] == OUT_SENTINEL).all() and (host[GUARD + planes * self.cells:] == OUT_SENTINEL).all(), "guard of out overwritten"
        return host[GUARD:GUARD + planes * self.cells].reshape(planes, r, c)

    def workspace(self):
        """The workspace as int32 words; its guards are checked on the way."""
        host = self.work.get(get_stream())
        assert (host[:GUARD] == WORK_SENTINEL).all() and (host[-GUARD:] == WORK_SENTINEL).all(), "guard of the workspace overwritten"
        return host[GUARD:-GUARD]

    def scan(self):
        """`mode | XRS_PROX_SCAN_ONLY` without an output buffer, then the five parts of the workspace."""
        self.run(pc.SCAN_ONLY, with_out=False)
        w, lay, cells = self.workspace(), self.lay, self.cells
        count = int(w[lay["count"] // 4])
        assert 0 <= count <= self.rows
        return {"left": w[lay["left"] // 4:][:cells].reshape(self.rows, self.cols),
                "right": w[lay["right"] // 4:][:cells].reshape(self.rows, self.cols),
                "flag": w[lay["flag"] // 4:][:self.rows], "list": w[lay["list"] // 4:][:count], "count": count}

    def products(self, metric, md=np.inf):
        """The three planes of mode 3, held bit for bit against modes 0, 1 and 2 on the way."""
        three = self.run(ALL_THREE, metric, md)
        for mode, p in enumerate(PRODUCTS):
            single = self.run(mode, metric, md)
            np.testing.assert_array_equal(_bits(single[0]), _bits(three[mode]), err_msg=f"{metric} mode {mode} against mode 3")
        return dict(zip(PRODUCTS, three))


def _assert_scan(got, targets, label):
    want = pc.scan_reference(targets)
    assert got["count"] == want["count"], (label, got["count"], want["count"])
    for k in ("left", "right", "flag", "list"):
        assert got[k].dtype == np.int32, (label, k)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{label} {k}")
        parity_log.record(label, k, got[k], want[k], tol=0)


_ORACLE = {}


def _oracle(case, metric):
    key = (case.name, metric)
    if key not in _ORACLE:
        with np.errstate(over="ignore"):                                 # (one tie-run case overflows float32 on purpose)
            _ORACLE[key] = po.run(case.z, case.xs, case.ys, case.tv, case.md, metric)
    return _ORACLE[key]


def _against_the_rule(case, metrics=None):
    call = Call(case.z, case.xs, case.ys, case.tv if case.tv.size else None)
    for metric in metrics or case.metrics:
        got = call.products(metric, case.md)
        _check(got, _oracle(case, metric), case.z, case.tv, metric, f"abi_{case.name}_{metric}")
    return call


# ------------------------------------------------------------------------------------------------ the scan
@pytest.mark.parametrize("cols", pc.WIDTHS)
def test_scan_planes_at_every_width(cols):
    """1 .. 769 columns: below a wave, a wave, a span and one past it, two spans and one past them, and 769: four steps, so
    both LDS slots are used twice and the right-to-left pass cuts the row at columns 1, 257, 513 where the other cuts at 256,
    512, 768.  Eight rows, one of each kind (proximity_cases.width_raster)."""
    z = pc.width_raster(cols)
    xc, yc = pc.unit_coords(*z.shape)
    _assert_scan(Call(z, xc, yc).scan(), z != 0, f"abi_scan_width_{cols}")


@pytest.mark.parametrize("rows", pc.HEIGHTS)
def test_row_list_at_every_height(rows):
    """1 .. 700 rows of 3 columns: the compaction's carry, the second use of an LDS slot (rows > 512), lists of 0, 1, 255, 256,
    257, 512, 513 and about 600 rows among them."""
    xc, yc = pc.unit_coords(rows, 3)
    for pattern in pc.FLAG_PATTERNS:
        z = pc.flag_raster(rows, 3, pattern)
        got = Call(z, xc, yc).scan()
        _assert_scan(got, z != 0, f"abi_scan_rows_{rows}_{pattern}")
        assert got["count"] == int(pc.flag_rows(rows, pattern).sum())


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_scan_reads_every_dtype(dtype):
    """the ten instantiations at 5 x 300 with n_values == 0: non-zero and finite"""
    z = pc.dtype_raster(dtype)
    xc, yc = pc.unit_coords(*z.shape)
    _assert_scan(Call(z, xc, yc).scan(), po.targets(z), f"abi_scan_dtype_{np.dtype(dtype).name}")


@pytest.mark.parametrize("name,z,tv", pc.value_cases(), ids=[c[0] for c in pc.value_cases()])
def test_scan_matches_target_values_as_numpy_does(name, z, tv):
    """value_match.h branch by branch: float rasters against float64 values (inf, NaN, +-0, 0.1), int64 values beyond 2^53,
    negative int64 values against unsigned rasters, uint64 values from 2^63 on against signed rasters and against uint64,
    float64 values against an int32 raster"""
    xc, yc = pc.unit_coords(*z.shape)
    _assert_scan(Call(z, xc, yc, tv).scan(), po.targets(z, tv), f"abi_scan_values_{name}")


# ------------------------------------------------------------------------------------------------ half calls, three planes
def test_scan_then_search_equals_one_call():
    """SCAN_ONLY then SEARCH_ONLY on the same workspace, bit for bit, three metrics, four modes.  The scan writes no output,
    the search leaves the workspace as it found it, and mode 3 is modes 0, 1, 2 (`products`)."""
    case = pc.roundtrip_case()
    for metric in case.metrics:
        whole, halves = Call(case.z, case.xs, case.ys), Call(case.z, case.xs, case.ys)
        whole.products(metric)
        for mode in (0, 1, 2, ALL_THREE):
            want = whole.run(mode, metric)
            untouched = halves.run(mode | pc.SCAN_ONLY, metric)
            assert (untouched == OUT_SENTINEL).all(), (metric, mode)
            before = halves.workspace().copy()
            got = halves.run(mode | pc.SEARCH_ONLY, metric)
            np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{metric} mode {mode}")
            np.testing.assert_array_equal(halves.workspace(), before, err_msg=f"{metric} mode {mode}: the search wrote to the workspace")
            assert not np.isnan(got).all()
        np.testing.assert_array_equal(whole.workspace(), halves.workspace())


def test_a_cut_in_the_half_calls_and_the_three_planes():
    """the same with max_distance set, which only the search reads"""
    case = pc.roundtrip_case()
    xc, yc = pc.unit_coords(*case.z.shape)
    for metric in ("EUCLIDEAN", "MANHATTAN"):
        whole, halves = Call(case.z, xc, yc), Call(case.z, xc, yc)
        want = whole.products(metric, 7.0)
        halves.scan()
        got = halves.run(ALL_THREE | pc.SEARCH_ONLY, metric, 7.0)
        for k, p in enumerate(PRODUCTS):
            np.testing.assert_array_equal(_bits(got[k]), _bits(want[p]), err_msg=f"{metric} {p}")
        assert np.isnan(got[0]).any() and not np.isnan(got[0]).all()


# ------------------------------------------------------------------------------------------------ the search against the rule
SEARCH = pc.search_cases()


@pytest.mark.parametrize("case", SEARCH, ids=[c.name for c in SEARCH])
def test_search_equals_the_rule(case):
    """EUCLIDEAN and MANHATTAN on every case of proximity_cases.search_cases: long row lists with cells above and below every
    non-empty row, a walk past 30 losing rows, lanes of one block closing far apart, the four coordinate orders, 2-, 4- and
    12-way ties, max_distance at equality and 0, uneven steps, a last block of one lane, int8 / uint16 / uint32 allocation."""
    call = _against_the_rule(case)
    if case.name == "ring_max5":
        for metric in case.metrics:
            prox = call.run(0, metric, case.md)[0]
            below = (pc.LONE[0] + 5, pc.LONE[1])
            assert prox[below] == 5.0 and prox[pc.LONE[0], pc.LONE[1] + 5] == 5.0 and np.isnan(prox[pc.LONE[0] + 6, pc.LONE[1]])
            if metric == "EUCLIDEAN":
                assert all(prox[c] == 5.0 for c in pc.RING_CENTRES)
    if case.name == "ring_max0":
        assert np.array_equal(~np.isnan(call.run(0, "EUCLIDEAN", 0.0)[0]), case.z != 0)
    if case.name.endswith("_none"):
        assert np.isnan(call.run(ALL_THREE, "EUCLIDEAN")).all()


@pytest.mark.parametrize("case", pc.tie_run_cases() + pc.margin_cases(), ids=lambda c: c.name)
def test_tie_runs_name_the_rules_target(case):
    """Long thin cells (0.01 x 100, 0.001 x 1000, 1e-6 x 1000), coordinates whose every d32 underflows to 0 (1e-46) or
    overflows to inf from row to row (1e30 x 1e39) or from cell to cell (1e39 x 1e39), and two targets at the widest ratio that still ties (`margin`): the
    targets of one side of a row share a float32 distance, and rule 3 names the far end of the run.  `allocation` and
    `direction` equal the oracle at every cell, EUCLIDEAN and MANHATTAN.

    These fail on the parent commit (0df363e), whose search looked at the nearest target on each side only: EUCLIDEAN
    allocation differed at 10 of 320 cells at 0.01 x 100 and at 114 at 0.001 x 1000 (the model of
    tests/test_proximity_cases_host.py: 11 and 118 winners).  `proximity` was right there, too."""
    call = Call(case.z, case.xs, case.ys)
    for metric in ("EUCLIDEAN", "MANHATTAN"):
        got, want = call.products(metric), _oracle(case, metric)
        what = f"abi_{case.name}_{metric}"
        for p in PRODUCTS:                                               # (`_check` minus its last line: where every d32 is 0
            off = po.ulps(got[p], want[p])                               #  a target's nearest target need not be itself)
            assert not np.isnan(got[p]).any(), (what, p)
            note = f"{int(np.count_nonzero(off))} of {off.size} cells not bit-equal, largest difference {int(off.max())} ulp"
            print(f"{what} {p}: {note}")
            parity_log.record(what, p, got[p], want[p], tol=2.0 ** -23 if p == "direction" else 0, note=note)
            assert (off <= (1 if p == "direction" else 0)).all(), (what, p, note)
        named = case.z[want["row"], want["col"]].astype(np.float32)      # every target has a value of its own:
        np.testing.assert_array_equal(got["allocation"], named, err_msg=what)   # allocation is the winner's identity


def test_great_circle_names_a_nearest_target_on_tie_runs():
    """The limit that is left (proximity.hip): GREAT_CIRCLE does not extend tie runs.  On longitudes 1e-9
    degrees apart `proximity` is within 1 ulp of the rule, and the target that `allocation` names (every target has a value
    of its own) is within 2 ulp of the nearest in the rule's arithmetic -- one of the float32-equidistant ones, not
    necessarily the one rule 3 names."""
    case = pc.great_circle_tie_case()
    want = po.run(case.z, case.xs, case.ys, (), np.inf, "GREAT_CIRCLE")
    got = Call(case.z, case.xs, case.ys).products("GREAT_CIRCLE")
    assert (po.ulps(got["proximity"], want["proximity"]) <= 1).all()
    tr, tc = np.nonzero(case.z)
    where = {int(case.z[r, c]): (r, c) for r, c in zip(tr, tc)}
    named = np.array([[where[int(v)] for v in row] for row in got["allocation"]])
    rows, cols = case.z.shape
    i, j = np.mgrid[0:rows, 0:cols]
    d_named = po.distance(case.xs[named[..., 1]], case.xs[j], case.ys[named[..., 0]], case.ys[i], po.METRICS["GREAT_CIRCLE"])
    off = po.ulps(d_named, want["d32"])
    print(f"gc_tie_run: the named target differs from the rule's at {int((named[..., 0] != want['row']).sum() + ((named[..., 0] == want['row']) & (named[..., 1] != want['col'])).sum())} "
          f"of {rows * cols} cells; its distance is within {int(off.max())} ulp of the nearest")
    parity_log.record("abi_gc_tie_run", "distance_of_named_target", d_named, want["d32"], tol=2.0 ** -22)
    assert (off <= GC_GAP_ULP).all()


@pytest.mark.parametrize("case", pc.great_circle_cases(), ids=lambda c: c.name)
def test_great_circle_long_row_lists(case):
    """300 rows under haversine, once on uneven degrees and once reaching round the back of the sphere (the row's first and
    last target as candidates); the existing rules, the share of cells left out asserted by `_check`."""
    want = _oracle(case, "GREAT_CIRCLE")
    if "wrap" in case.name:
        assert (np.abs(case.xs[want["col"]] - case.xs[None, :]) > 180.0).sum() >= 10
    _against_the_rule(case)

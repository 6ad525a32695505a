"""xrs_local_cells, xrs_local_combine (both calls) and xrs_local_gather at the C ABI (xrspatial_amd/csrc/local.hip) -- never a
function of the package -- on the cases of tests/local_cases.py, against the rule (tests/local_oracle.py).
tests/test_local_cases_host.py shows on the CPU that every case reaches the path it is named for.

The kernels use +, -, *, /, sqrt (correctly rounded, no contraction) and comparisons only, in the order the rule writes down, so
every cell is compared at tolerance 0: NaN equals NaN, -0.0 equals 0.0, as `same` of tests/test_gpu_local.py does.  A result
plane written with out_is_i64 = 1 is read as int64 and compared as integers.  The gathered key values are compared as 8-byte
bit patterns, except that a zero may carry either sign.  Every output lies between GUARD elements of a sentinel, checked after
every call; a case with `offset` = 1 passes plane, ref and output pointers one element past their allocation's start."""
import ctypes

import numpy as np
import pytest

import xrspatial_amd as xs
from tests import local_cases as lc
from xrspatial_amd import _lib
from xrspatial_amd._launch import get_stream

pytestmark = pytest.mark.gpu

GUARD = 8                                               # elements of 0x5A bytes: as float64 1.3e127, as int64 6.5e18 -- no case expects either
CASES = lc.by_name()
CELL_CASES = [name for name, c in CASES.items() if c["ops"] != ("combine",)]
COMBINE_CASES = [name for name, c in CASES.items() if c["ops"] == ("combine",)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")
    _lib.require_device()


class Planes:
    """the planes (and the ref plane) of a case on the device, `offset` elements past the start of their allocations"""

    def __init__(self, c):
        self.n, self.count, off = c["planes"][0].size, len(c["planes"]), c["offset"]
        arrays = c["planes"] + ([c["ref"]] if c["ref"] is not None else [])
        self.keep = [xs.DeviceArray.from_numpy(np.concatenate([np.ones(off, a.dtype), a])) for a in arrays]
        at = [d.ptr + off * a.dtype.itemsize for d, a in zip(self.keep, arrays)]
        self.ptrs = (ctypes.c_void_p * self.count)(*at[:self.count])
        self.codes = (ctypes.c_int * self.count)(*[lc.DTYPE_CODE[p.dtype] for p in c["planes"]])
        self.ref = at[self.count] if c["ref"] is not None else None
        self.ref_code = lc.DTYPE_CODE[c["ref"].dtype] if c["ref"] is not None else 0


class Guarded:
    """`count` 8-byte (or 4-byte) elements on the device between two guards, `offset` elements past the first guard"""

    def __init__(self, count, dtype=np.uint64, offset=0, guard=GUARD):
        self.count, self.dtype, self.lead = count, np.dtype(dtype), guard + offset
        fill = np.full((self.lead + count + guard) * self.dtype.itemsize, 0x5A, np.uint8)
        self.dev = xs.DeviceArray.from_numpy(fill.view(self.dtype))
        self.ptr = self.dev.ptr + self.lead * self.dtype.itemsize

    def get(self):
        host = self.dev.get(get_stream())
        sentinel = np.full(8, 0x5A, np.uint8).view(self.dtype)[0]
        assert (host[:self.lead] == sentinel).all() and (host[self.lead + self.count:] == sentinel).all(), "a guard was overwritten"
        return host[self.lead:self.lead + self.count]


def differing(got, want, planes, ref):
    """'' if every cell agrees, else the first five cells that do not, with their plane values"""
    if got.dtype.kind == "f":
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    else:
        bad = got != want
    lines = [f"{int(bad.sum())} of {bad.size} cells differ"]
    for i in np.flatnonzero(bad)[:5].tolist():
        lines.append(f"cell {i}: got {got[i]!r}, want {want[i]!r}; planes {[p[i].item() for p in planes]}"
                     + (f", ref {ref[i].item()!r}" if ref is not None else ""))
    return "\n".join(lines) if bad.any() else ""


@pytest.mark.parametrize("name", CELL_CASES)
def test_cells(name):
    c = CASES[name]
    dev = Planes(c)
    failures = []
    for op in c["ops"]:
        want = lc.expected(c, op)
        as_i64 = lc.out_i64(c, op)
        assert want.dtype == (np.int64 if as_i64 else np.float64)
        out = Guarded(dev.n, offset=c["offset"])
        needs_ref = op in lc.NEEDS_REF
        _lib.call("xrs_local_cells", lc.OPS[op], dev.ptrs, dev.codes, dev.count, dev.ref if needs_ref else None,
                  dev.ref_code if needs_ref else 0, dev.n, out.ptr, as_i64, get_stream())
        got = out.get().view(want.dtype)
        what = differing(got, want, c["planes"], c["ref"] if needs_ref else None)
        if what:
            failures.append(f"{op} (out_is_i64 = {as_i64}): {what}")
    assert not failures, f"{name} [{c['reaches']}]\n" + "\n".join(failures)


@pytest.mark.parametrize("pair", [("B_big_n05_out0", "B_big_n05_out1"), ("B_small_n03_out0", "B_small_n03_out1"),
                                  ("B_small_n09_out0", "B_small_n09_out1")], ids=lambda p: p[0][:-5])
def test_float64_result_is_the_int64_result_converted(pair):
    """the two result forms of the same call against each other: (double)r of the very integers out_is_i64 = 1 writes"""
    c = CASES[pair[0]]
    assert all(np.array_equal(p, q) for p, q in zip(c["planes"], CASES[pair[1]]["planes"]))
    dev = Planes(c)
    for op in c["ops"]:
        got = []
        for as_i64 in (0, 1):
            out = Guarded(dev.n)
            _lib.call("xrs_local_cells", lc.OPS[op], dev.ptrs, dev.codes, dev.count, dev.ref, dev.ref_code, dev.n, out.ptr, as_i64,
                      get_stream())
            got.append(out.get())
        as_f64, exact = got[0].view(np.float64), got[1].view(np.int64)
        assert np.array_equal(as_f64.view(np.uint64), exact.astype(np.float64).view(np.uint64)), op


@pytest.mark.parametrize("name", COMBINE_CASES)
def test_combine(name):
    c = CASES[name]
    want_ids, want_classes, want_first, want_values = lc.expected_combine(c)
    dev = Planes(c)
    n, count, stream = dev.n, dev.count, get_stream()
    nbytes = _lib.workspace_bytes("local_combine", n, count)
    assert nbytes >= 256
    work = Guarded((nbytes + 7) // 8, guard=32)                          # (256 bytes: the workspace stays 256-byte aligned)
    out = Guarded(n)
    classes = ctypes.c_int64(-1)
    _lib.call("xrs_local_combine", dev.ptrs, dev.codes, count, n, work.ptr, nbytes, out.ptr, None, 0, ctypes.byref(classes), stream)
    ids = out.get().view(np.float64)
    what = differing(ids, want_ids, c["planes"], None)
    assert not what, f"{name} [{c['reaches']}]\nids: {what}"
    assert classes.value == want_classes
    first = Guarded(want_classes, np.uint32)
    _lib.call("xrs_local_combine", dev.ptrs, dev.codes, count, n, work.ptr, nbytes, out.ptr, first.ptr, want_classes,
              ctypes.byref(classes), stream)
    assert classes.value == want_classes
    got_first = first.get()
    assert np.array_equal(got_first, want_first), (name, "first cells", got_first[:8], want_first[:8])
    work.get()                                                           # (its guards)
    assert np.array_equal(out.get().view(np.float64), ids, equal_nan=True)       # the second call leaves the ids alone
    values = Guarded(want_classes * count)
    _lib.call("xrs_local_gather", dev.ptrs, dev.codes, count, n, first.ptr, want_classes, values.ptr, stream)
    got_values = values.get().reshape(want_classes, count)
    for j, p in enumerate(c["planes"]):
        g, w = got_values[:, j], want_values[:, j]
        agree = g == w
        if p.dtype.kind == "f":                                          # -0.0 == 0.0: either zero stands for the class
            agree |= (g.view(np.float64) == 0) & (w.view(np.float64) == 0)
        view = np.float64 if p.dtype.kind == "f" else np.int64
        rows = np.flatnonzero(~agree)[:5]
        assert agree.all(), (name, f"key values of plane {j} ({p.dtype})", [(int(r), g.view(view)[r], w.view(view)[r]) for r in rows])

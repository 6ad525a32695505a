"""natural_breaks on the MI355X against what the reference's own code produced (tests/golden/natural_breaks_exec.npz).

Everything is exact: both tables of the dynamic programme are compared as uint32 words at every entry, the initial zeros and
infinities included; the classified rasters by digest and, where the fixture holds them, cell by cell.  There is no tolerance
to choose: the only arithmetic outside the reference's own NumPy lines is the kernel, which is specified operation by operation
(csrc/jenks.hip), and tests/test_natural_breaks_host.py holds a NumPy model of that specification against the same tables.

Sizes (the generator's): n = 1, 2, 3 (nothing / one row to launch), 63, 64, 65 and 129 (one thread short of a wave, exactly one
and two, one over), 600 and 2049 (many blocks, the longest rows first), k from 1 to 9 and k = n; ties, float32-subnormal squares
and mixed signs."""
import ctypes
import hashlib
import warnings

import numpy as np
import pytest

from tests.golden import make_classify_exec as cx
from tests.golden import make_natural_breaks_exec as gen

pytestmark = pytest.mark.gpu

FIX = gen.load()
MATRIX = sorted({k.split("/")[1] for k in FIX if k.startswith("m/")})
E2E = {name: (a, kw) for name, a, kw in gen.e2e_cases()}
for _a, _ in E2E.values():
    _a.setflags(write=False)


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _agg(xs, data, **kw):
    return xs.DataArray(data, dims=["y", "x"], attrs={"res": (1, 1), "tag": "kept"}, **kw)


# ------------------------------------------------------------------ the kernels at the ABI
@pytest.mark.parametrize("case", MATRIX)
def test_tables_at_the_abi(xs, case):
    from xrspatial_amd import _lib
    sample, k = FIX[f"m/{case}/sample"], int(FIX[f"m/{case}/k"])
    n = sample.size
    lib = _lib.load()
    data_d = xs.DeviceArray.from_numpy(sample)
    # poisoned outputs: the call must write every entry, the initial values too
    limits_d = xs.DeviceArray.from_numpy(np.full((n + 1, k + 1), np.nan, np.float32))
    var_d = xs.DeviceArray.from_numpy(np.full((n + 1, k + 1), np.nan, np.float32))
    work = xs.DeviceArray((int(lib.xrs_jenks_workspace_bytes(n, k)),), np.uint8)
    _lib.call("xrs_jenks_matrices_f32", data_d.ptr, n, k, limits_d.ptr, var_d.ptr, work.ptr, work.nbytes, None)
    limits, var = limits_d.get(), var_d.get()
    if f"m/{case}/limits" in FIX:
        np.testing.assert_array_equal(limits.view(np.uint32), FIX[f"m/{case}/limits"].view(np.uint32), err_msg=case)
        np.testing.assert_array_equal(var.view(np.uint32), FIX[f"m/{case}/var"].view(np.uint32), err_msg=case)
    else:
        assert _sha(limits) == str(FIX[f"m/{case}/limits_sha"]), case
        assert _sha(var) == str(FIX[f"m/{case}/var_sha"]), case
    from xrspatial_amd import jenks
    got = jenks.kclass_from_limits(limits, sample, k)
    np.testing.assert_array_equal(got.view(np.uint32), FIX[f"m/{case}/kclass"].view(np.uint32), err_msg=case)
    np.testing.assert_array_equal(data_d.get().view(np.uint32), sample.view(np.uint32))          # the sample is only read


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64, np.int64])
def test_gather_copies_elements_unconverted(xs, dtype):
    from xrspatial_amd import _lib
    rng = np.random.default_rng(7)
    n = 1000
    src = rng.integers(0, 256, n * np.dtype(dtype).itemsize, dtype=np.uint8).view(dtype)        # any bit pattern, NaNs included
    idx = np.concatenate([rng.integers(0, n, 700), [0, n - 1, n - 1, 0]]).astype(np.uint32)      # > 2 blocks, repeats, both ends
    src_d, idx_d = xs.DeviceArray.from_numpy(src), xs.DeviceArray.from_numpy(idx)
    out_d = xs.DeviceArray((idx.size,), dtype)
    _lib.call("xrs_gather_elems", src_d.ptr, src.itemsize, n, idx_d.ptr, idx.size, out_d.ptr, None)
    assert out_d.get().tobytes() == src[idx].tobytes()


def test_argument_errors_launch_nothing(xs):
    from xrspatial_amd import _lib
    lib = _lib.load()
    sample = np.arange(10, dtype=np.float32)
    data_d = xs.DeviceArray.from_numpy(sample)
    poison = np.full((11, 4), np.nan, np.float32)
    limits_d, var_d = xs.DeviceArray.from_numpy(poison), xs.DeviceArray.from_numpy(poison)
    work = xs.DeviceArray((int(lib.xrs_jenks_workspace_bytes(10, 3)),), np.uint8)
    none = ctypes.c_void_p(0)
    for args, text in (((data_d.ptr, 0, 3, limits_d.ptr, var_d.ptr, work.ptr, work.nbytes), "at least 1 value"),
                       ((data_d.ptr, 10, 0, limits_d.ptr, var_d.ptr, work.ptr, work.nbytes), "at least 1 class"),
                       ((data_d.ptr, 1 << 24, 3, limits_d.ptr, var_d.ptr, work.ptr, work.nbytes), "2^24"),
                       ((none, 10, 3, limits_d.ptr, var_d.ptr, work.ptr, work.nbytes), "null pointer"),
                       ((data_d.ptr, 10, 3, limits_d.ptr, var_d.ptr, none, work.nbytes), "null pointer"),
                       ((data_d.ptr, 10, 3, limits_d.ptr, var_d.ptr, work.ptr, work.nbytes - 1), "workspace")):
        assert lib.xrs_jenks_matrices_f32(*args, None) != 0 and text in _lib.last_error(), (text, _lib.last_error())
    out_d = xs.DeviceArray.from_numpy(poison)
    idx_d = xs.DeviceArray.from_numpy(np.arange(4, dtype=np.uint32))
    for args, text in (((data_d.ptr, 3, 10, idx_d.ptr, 4, out_d.ptr), "1, 2, 4 or 8 bytes"),
                       ((data_d.ptr, 4, 10, idx_d.ptr, -1, out_d.ptr), "negative size"),
                       ((data_d.ptr, 4, 10, none, 4, out_d.ptr), "null pointer")):
        assert lib.xrs_gather_elems(*args, None) != 0 and text in _lib.last_error(), (text, _lib.last_error())
    xs.synchronize()
    for d in (limits_d, var_d, out_d):
        assert np.isnan(d.get()).all()


# ------------------------------------------------------------------ the public function
def _call(xs, agg, kw):
    """(result or None, exception type name or None, ['Category: text'] of the plain `Warning`s raised)."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            res, exc = xs.natural_breaks(agg, **kw), None
        except Exception as e:                 # noqa: BLE001  (the exception type is the expected outcome)
            res, exc = None, type(e).__name__
    return res, exc, [f"{w.category.__name__}: {w.message}" for w in caught if w.category is Warning]


@pytest.mark.parametrize("case", sorted(E2E))
def test_public_function_equals_the_reference(xs, case):
    a, kw = E2E[case]
    key = f"e/{case}"
    before = a.copy()
    res, exc, warned = _call(xs, _agg(xs, a), kw)
    np.testing.assert_array_equal(a.view(np.uint8), before.view(np.uint8))                        # the input is left as it was
    if f"{key}/exc" in FIX:
        assert exc == str(FIX[f"{key}/exc"])
        assert _call(xs, _agg(xs, xs.DeviceArray.from_numpy(a)), kw)[1] == exc
        return
    assert exc is None
    assert warned == FIX[f"{key}/warn"].tolist()
    assert isinstance(res.data, np.ndarray) and res.data.dtype.str == str(FIX[f"{key}/dtype"])
    assert res.name == "natural_breaks" and res.dims == ("y", "x") and res.attrs == {"res": (1, 1), "tag": "kept"}
    if f"{key}/out" in FIX:
        np.testing.assert_array_equal(res.data, FIX[f"{key}/out"], err_msg=case)
    assert cx.digest(res.data) == str(FIX[f"{key}/sha"]), case
    # DeviceArray in, DeviceArray out, the same cells, the same warnings; the resident raster is left as it was
    dev = xs.DeviceArray.from_numpy(a)
    res_d, exc_d, warned_d = _call(xs, _agg(xs, dev), {**kw, "name": "other"})
    assert exc_d is None and warned_d == warned
    assert isinstance(res_d.data, xs.DeviceArray) and res_d.name == "other"
    assert cx.digest(res_d.data.get()) == str(FIX[f"{key}/sha"]), case
    assert dev.get().tobytes() == a.tobytes()


def test_the_long_sample_warning(xs):
    """The reference warns from 40 000 sample points on, before anything is computed; k = 1 keeps the call short (the backtrack
    reads no table for one class)."""
    a = np.random.default_rng(3).normal(0.0, 1.0, (200, 200)).astype(np.float32)
    res, exc, warned = _call(xs, _agg(xs, a), {"num_sample": None, "k": 1})
    assert exc is None
    assert warned == ["Warning: natural_breaks Warning: Natural break classification (Jenks) has a complexity of O(n^2), "
                      "your classification with 40000 data points may take a long time."]
    np.testing.assert_array_equal(res.data, np.zeros((200, 200), np.float32))


def test_dataset_is_classified_variable_by_variable(xs):
    a, kw = E2E["f32_12x17_sample_above_size"]
    b, _ = E2E["f32_16x16_k1"]
    ds = xs.Dataset({"first": _agg(xs, a), "second": _agg(xs, b[:12, :])}, attrs={"title": "both"})
    out = xs.natural_breaks(ds, **kw)
    assert isinstance(out, xs.Dataset) and list(out.data_vars) == ["first", "second"] and out.attrs == {"title": "both"}
    assert out["first"].name == "first"
    np.testing.assert_array_equal(out["first"].data, FIX["e/f32_12x17_sample_above_size/out"])
    np.testing.assert_array_equal(out["second"].data, xs.natural_breaks(_agg(xs, b[:12, :]), **kw).data)


@pytest.mark.parametrize("vec", ["natural_breaks", "natural_breaks_num_sample"])
def test_reference_vectors(xs, vec):
    agg = _agg(xs, FIX["vec/input"])
    if vec == "natural_breaks":
        k, want = int(FIX[f"vec/{vec}/0"]), FIX[f"vec/{vec}/1"]
        got = xs.natural_breaks(agg, k=k)
    else:
        k, num_sample, want = int(FIX[f"vec/{vec}/0"]), int(FIX[f"vec/{vec}/1"]), FIX[f"vec/{vec}/2"]
        got = xs.natural_breaks(agg, num_sample=num_sample, k=k)
    assert got.data.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.data, want)

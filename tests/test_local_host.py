"""CPU checks of xrspatial_amd.local: the rule (tests/local_oracle.py) against the reference's own outputs
(tests/golden/local_exec.npz) at every cell of every case -- NaN equals NaN, -0.0 equals 0.0, no tolerance --, the result
dtype of the rule, the reference's argument errors word for word, this backend's own errors and refusals, which all come
before any device work, and the argument validation of the C ABI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import local_oracle as lo
from tests.golden import make_local_exec as gen

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want):
    """equal at every cell: NaN equals NaN, -0.0 equals 0.0"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got.astype(np.float64), want.astype(np.float64), equal_nan=True)


def oracle_outputs(name):
    """{function: result} of the rule for the functions the fixture holds of a case"""
    planes = gen.planes_of(FIXTURE, name)
    out = {}
    for f in gen.functions_of(gen.stored(FIXTURE, name)):
        if f in lo.STATS:
            out[f] = lo.cell_stats(planes, f)
        elif f.endswith("_frequency"):
            out[f] = lo.frequency(planes, FIXTURE[f"{name}/ref_freq"], f.split("_")[0])
        elif f.endswith("_position"):
            out[f] = lo.position(planes, f.split("_")[0])
        elif f == "rank":
            out[f] = lo.rank(planes, FIXTURE[f"{name}/ref_rank"])
        else:
            out[f] = lo.popularity(planes, FIXTURE[f"{name}/ref_pop"])
    return out


def key_arrays(key, n_vars):
    return (np.array(list(key.keys()), np.int64),
            np.array([list(v) for v in key.values()], np.float64).reshape(len(key), n_vars))


# ------------------------------------------------------------------ the rule against the executed reference
@pytest.mark.parametrize("case", CASES)
def test_rule_equals_the_reference(case):
    got = oracle_outputs(case)
    funcs = gen.functions_of(gen.stored(FIXTURE, case))
    for row, f in enumerate(funcs):
        want = FIXTURE[f"{case}/outputs"][row]
        assert same(got[f], want), (f, np.argwhere(~((got[f] == want) | (np.isnan(got[f]) & np.isnan(want))))[:5].tolist())
    n_vars = FIXTURE[f"{case}/combine_key_values"].shape[1]
    ids, key = lo.combine(gen.planes_of(FIXTURE, case)[:n_vars])
    assert same(ids, FIXTURE[f"{case}/combine"])
    kid, kval = key_arrays(key, n_vars)
    assert kid.tolist() == list(range(1, len(kid) + 1)) and same(kval, FIXTURE[f"{case}/combine_key_values"])


@pytest.mark.parametrize("case", CASES)
def test_result_dtype_of_the_rule(case):
    planes = gen.planes_of(FIXTURE, case)
    floating = any(p.dtype.kind == "f" for p in planes)
    for f, res in oracle_outputs(case).items():
        ref = FIXTURE[f"{case}/ref_freq"] if f.endswith("_frequency") else None
        is_float = floating or f in ("mean", "median", "std", "rank", "popularity") or (ref is not None and ref.dtype.kind == "f")
        assert res.dtype == (np.float64 if is_float else np.int64), f


def test_fixture_covers_what_the_spec_lists():
    shapes = {gen.planes_of(FIXTURE, c)[0].shape for c in CASES}
    assert {(2, 2), (4, 4), (1, 1), (1, 7), (9, 1), (3, 5), (37, 53)} <= shapes
    counts = {len(gen.planes_of(FIXTURE, c)) for c in CASES}
    assert set(gen.N_LIST) <= counts
    kinds = {tuple(sorted({p.dtype.name for p in gen.planes_of(FIXTURE, c)})) for c in CASES}
    assert {("float32",), ("float64",), ("int32",), ("int64",), ("float32", "float64", "int16")} <= kinds
    assert FIXTURE["f32_ref_below_resolution/ref_freq"].dtype == np.float32
    row = gen.functions_of(gen.stored(FIXTURE, "f32_ref_below_resolution")).index("equal_frequency")
    assert (FIXTURE["f32_ref_below_resolution/outputs"][row] >= 3).all()          # equal in float32, not in float64
    for c in CASES:
        funcs = gen.functions_of(gen.stored(FIXTURE, c))
        if "popularity" in funcs and gen.planes_of(FIXTURE, c)[0].size > 1:
            assert np.isfinite(FIXTURE[f"{c}/outputs"][funcs.index("popularity")]).mean() >= 0.25, c
        n = len(gen.planes_of(FIXTURE, c))
        r = FIXTURE[f"{c}/ref_rank"]
        assert r.min() >= 1 - n and r.max() <= n + 2
    assert os.path.getsize(gen.OUT) < gen.MAX_BYTES
    assert any(np.isnan(FIXTURE[f"{c}/combine"]).any() for c in CASES)


@pytest.mark.skipif(not gen.rx.have_reference(), reason="the reference is not present here")
def test_fixture_reproduces():
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_local_exec.py"), "--check"],
                         capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr


def test_pairwise_is_numpys_sum():
    rng = np.random.default_rng(5)
    for n in range(1, 40):
        v = rng.normal(scale=1e3, size=(n, 50))
        want = np.array([np.sum(tuple(col.tolist())) for col in v.T])
        assert np.array_equal(lo.pairwise(v), want), n


# ------------------------------------------------------------------ the host side of the public functions
def _ds(**variables):
    import xrspatial_amd as xa
    return xa.Dataset({k: xa.DataArray(v) for k, v in variables.items()})


PLAIN = ("cell_stats", "combine", "lowest_position", "highest_position")
WITH_REF = ("lesser_frequency", "equal_frequency", "greater_frequency", "popularity", "rank")


def test_module_is_imported_and_nothing_is_exported_at_package_level():
    import xrspatial_amd as xa
    for name in PLAIN + WITH_REF:
        assert callable(getattr(xa.local, name)), name
        assert not hasattr(xa, name), name                       # the reference's __init__ exports none of them
    assert xa.local.XRS_LOCAL_MAX_PLANES == 64


def test_argument_errors_of_the_reference():
    import xrspatial_amd as xa
    z = np.zeros((2, 3))
    ds = _ds(a=z, b=z, r=z.astype(np.int32))
    for name in PLAIN + WITH_REF:
        fn = getattr(xa.local, name)
        args = ("r",) if name in WITH_REF else ()
        with pytest.raises(TypeError, match=r"^Expected raster to be a 'xarray.Dataset'. Received 'DataArray' instead.$"):
            fn(xa.DataArray(z), *args)
        with pytest.raises(TypeError, match="^Expected data_vars to be a list of string.$"):
            fn(ds, *args, data_vars=("a", "b"))
        with pytest.raises(TypeError, match="^Expected data_vars to be a list of string.$"):
            fn(ds, *args, data_vars=["a", 1])
        with pytest.raises(ValueError, match=r"^raster must contain all the variables of data_vars. The variables available are "
                                             r"'\['a', 'b', 'r'\]'.$"):
            fn(ds, *args, data_vars=["a", "nope"])
    with pytest.raises(ValueError, match=r"^mode is not supported. The supported types are "
                                         r"'\['max', 'mean', 'median', 'min', 'std', 'sum'\]'.$"):
        xa.local.cell_stats(ds, func="mode")
    for name in WITH_REF:
        fn = getattr(xa.local, name)
        with pytest.raises(TypeError, match=r"^Expected ref_var to be a 'str'. Received 'int' instead.$"):
            fn(ds, 3)
        with pytest.raises(ValueError, match="^raster must contain ref_var.$"):
            fn(ds, "nope")
        with pytest.raises(ValueError, match="^ref_var must not be an element of data_vars.$"):
            fn(ds, "r", data_vars=["a", "r"])


def test_errors_of_this_backend_come_before_device_work():
    import xrspatial_amd as xa
    z = np.zeros((2, 3))
    with pytest.raises(ValueError, match="shape"):
        xa.local.cell_stats(_ds(a=z, b=np.zeros((3, 2))))
    with pytest.raises(ValueError, match="2-D"):
        xa.local.combine(_ds(a=np.zeros(6), b=np.zeros(6)))
    with pytest.raises(ValueError, match="shape"):
        xa.local.rank(_ds(a=z, b=z, r=np.zeros((1, 3), np.int32)), "r")
    many = {f"v{j:02d}": z for j in range(65)}
    with pytest.raises(ValueError, match="at most 64"):
        xa.local.lowest_position(_ds(**many))
    many["r"] = z
    with pytest.raises(ValueError, match="at most 64"):
        xa.local.equal_frequency(_ds(**many), "r")
    for dtype in (np.uint64, np.bool_, np.float16):
        with pytest.raises(TypeError, match="unsupported dtype"):
            xa.local.cell_stats(_ds(a=z, b=z.astype(dtype)))
        with pytest.raises(TypeError, match="unsupported dtype"):
            xa.local.lesser_frequency(_ds(a=z, r=z.astype(dtype)), "r")
    for name in ("rank", "popularity"):
        with pytest.raises(TypeError, match="integer dtype"):
            getattr(xa.local, name)(_ds(a=z, b=z, r=z.astype(np.float32)), "r")


def test_dask_and_sharded_variables_are_refused(monkeypatch):
    import xrspatial_amd as xa
    from xrspatial_amd import utils
    from tests import fake_dask, fake_hip
    z = np.zeros((8, 8), np.float32)
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _ds(a=z, b=fake_dask.from_array(z, (4, 4)), r=z.astype(np.int32))
    for name in PLAIN + WITH_REF:
        with pytest.raises(NotImplementedError, match="dask"):
            getattr(xa.local, name)(lazy, *(("r",) if name in WITH_REF else ()))
    fake_hip.install(monkeypatch)
    split = _ds(a=z, b=z, r=xa.ShardedArray.from_numpy(z.astype(np.int32)))
    for name in WITH_REF:
        with pytest.raises(NotImplementedError, match="sharded"):
            getattr(xa.local, name)(split, "r")
    with pytest.raises(NotImplementedError, match="sharded"):
        xa.local.cell_stats(_ds(a=z, b=xa.ShardedArray.from_numpy(z)))


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xa
    if xa.has_hip():
        pytest.skip("a GPU is present")
    z = np.ones((4, 4), np.float32)
    with pytest.raises(xa.XrsError):
        xa.local.cell_stats(_ds(a=z, b=z))
    with pytest.raises(xa.XrsError):
        xa.local.combine(_ds(a=z, b=z))


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_local_* validate on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    F64, F32, I32, U64 = 8, 9, 4, 7
    MAX, MEAN, EQUAL, RANK = 0, 3, 7, 11
    some = ctypes.c_void_p(256)

    def table(n, code, ptr=256):
        return (ctypes.c_void_p * n)(*[ptr] * n), (ctypes.c_int * n)(*[code] * n)

    def cells(op, ptrs, codes, n_planes, ref=None, ref_dtype=0, n=16, out=some, out_i64=0):
        return lib.xrs_local_cells(op, ptrs, codes, n_planes, ref, ref_dtype, n, out, out_i64, None)

    p, c = table(3, F32)
    assert cells(MAX, None, c, 3) != 0 and "null pointer" in _lib.last_error()
    assert cells(MAX, p, None, 3) != 0 and "null pointer" in _lib.last_error()
    assert cells(MAX, p, c, 3, out=None) != 0 and "null pointer" in _lib.last_error()
    assert cells(EQUAL, p, c, 3) != 0 and "null pointer (ref)" in _lib.last_error()
    hole = (ctypes.c_void_p * 3)(256, None, 256)
    assert cells(MAX, hole, c, 3) != 0 and "null pointer (plane 1)" in _lib.last_error()
    for n_planes in (0, 65, -1):
        assert cells(MAX, p, c, n_planes) != 0 and "outside 1 .. 64" in _lib.last_error()
    for op in (-1, 13):
        assert cells(op, p, c, 3) != 0 and "unknown op" in _lib.last_error()
    pu, cu = table(2, U64)
    assert cells(MAX, pu, cu, 2) != 0 and "unsupported dtype" in _lib.last_error()
    assert cells(MAX, p, c, 3, out_i64=1) != 0 and "int64 result needs integer planes" in _lib.last_error()
    pi, ci = table(2, I32)
    assert cells(MEAN, pi, ci, 2, out_i64=1) != 0 and "int64 result needs integer planes" in _lib.last_error()
    assert cells(EQUAL, pi, ci, 2, ref=some, ref_dtype=F64, out_i64=1) != 0 and "int64 result" in _lib.last_error()
    assert cells(RANK, pi, ci, 2, ref=some, ref_dtype=F32) != 0 and "integer ref" in _lib.last_error()
    assert cells(RANK, pi, ci, 2, ref=some, ref_dtype=I32, out_i64=1) != 0 and "can give NaN" in _lib.last_error()
    assert cells(MAX, p, c, 3, n=-1) != 0 and "negative size" in _lib.last_error()
    assert cells(MAX, p, c, 3, n=0) == 0

    classes = ctypes.c_int64(-1)

    def combine(ptrs, codes, n_planes, n=16, work=some, work_bytes=1 << 40, out=some, count=ctypes.byref(classes)):
        return lib.xrs_local_combine(ptrs, codes, n_planes, n, work, work_bytes, out, None, 0, count, None)

    assert combine(None, c, 3) != 0 and "null pointer" in _lib.last_error()
    assert combine(p, c, 65) != 0 and "outside 1 .. 64" in _lib.last_error()
    assert combine(p, c, 3, count=None) != 0 and "null pointer" in _lib.last_error()
    assert combine(p, c, 3, n=2 ** 31) != 0 and "2^31-1 cells" in _lib.last_error()
    assert combine(p, c, 3, work=None) != 0 and "null pointer (workspace)" in _lib.last_error()
    assert combine(p, c, 3, work_bytes=16) != 0 and "workspace too small" in _lib.last_error()
    assert combine(p, c, 3, out=None) != 0 and "null pointer (out)" in _lib.last_error()
    assert combine(p, c, 3, n=0) == 0 and classes.value == 0
    assert lib.xrs_local_combine_workspace_bytes(0, 3) == 256
    assert lib.xrs_local_combine_workspace_bytes(1000, 3) >= 1000 * 33
    assert lib.xrs_local_gather(p, c, 3, 16, None, 4, some, None) != 0 and "null pointer" in _lib.last_error()
    assert lib.xrs_local_gather(p, c, 3, 16, None, 0, None, None) == 0

"""CPU checks of xrspatial_amd.natural_breaks (jenks.py) against what the reference's own code produced
(tests/golden/natural_breaks_exec.npz): the sample indices and their cache, the backtrack over the class limits, the NumPy
model of the kernel's walk (tests/natural_breaks_oracle.py) bit for bit against every stored table -- which pins the
algorithm csrc/jenks.hip implements independently of a GPU --, the C ABI's argument checks, and the public surface."""
import ctypes
import hashlib
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import xrspatial_amd as xs
from xrspatial_amd import _lib, jenks
from tests import natural_breaks_oracle as orc
from tests.golden import make_natural_breaks_exec as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = gen.load()
MATRIX = sorted({k.split("/")[1] for k in FIX if k.startswith("m/")})
_tables = {}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def model_tables(case):
    """The model's tables of a matrix case, computed once and left unchanged."""
    if case not in _tables:
        limits, var = orc.jenks_tables(FIX[f"m/{case}/sample"], int(FIX[f"m/{case}/k"]))
        limits.setflags(write=False)
        var.setflags(write=False)
        _tables[case] = (limits, var)
    return _tables[case]


def test_the_fixture_holds_every_case_of_the_generator():
    assert MATRIX == sorted(name for name, _, _ in gen.matrix_cases())
    for name, sample, k in gen.matrix_cases():
        np.testing.assert_array_equal(FIX[f"m/{name}/sample"].view(np.uint32), sample.view(np.uint32), err_msg=name)
        assert int(FIX[f"m/{name}/k"]) == k
        stored_whole = f"m/{name}/limits" in FIX
        assert stored_whole == ((sample.size + 1) * (k + 1) <= gen.SMALL) and (stored_whole or f"m/{name}/limits_sha" in FIX)
    assert sorted({k.split("/")[1] for k in FIX if k.startswith("e/")}) == sorted(name for name, _, _ in gen.e2e_cases())
    # the cases the arithmetic hinges on are really in there
    tied = FIX["m/ties_n90_k4/sample"]
    assert np.unique(tied).size <= 7 < tied.size
    tiny = FIX["m/tiny_n70_k3/sample"]
    squares = tiny * tiny
    assert ((squares != 0) & (np.abs(squares) < np.finfo(np.float32).tiny)).any()
    assert (FIX["m/both_signs_n100_k5/sample"] < 0).any() and (FIX["m/both_signs_n100_k5/sample"] > 0).any()


@pytest.mark.parametrize("pair", gen.INDEX_PAIRS, ids=lambda p: f"{p[0]}_{p[1]}")
def test_sample_indices_are_the_reference_s(pair):
    got = jenks.sample_indices(*pair)
    want = FIX[f"idx/{pair[0]}_{pair[1]}"]
    assert got.dtype == want.dtype == np.uint32
    np.testing.assert_array_equal(got, want)


def test_sample_indices_cache_keeps_the_last_two():
    a = jenks.sample_indices(3000, 100)
    assert jenks.sample_indices(3000, 100) is a and not a.flags.writeable
    b = jenks.sample_indices(3001, 100)
    assert jenks.sample_indices(3000, 100) is a and jenks.sample_indices(3001, 100) is b
    jenks.sample_indices(3002, 7)
    jenks.sample_indices(3003, 7)
    assert len(jenks._index_cache) == 2
    again = jenks.sample_indices(3000, 100)
    assert again is not a
    np.testing.assert_array_equal(again, a)


@pytest.mark.parametrize("case", MATRIX)
def test_model_of_the_kernel_reproduces_the_reference_s_tables(case):
    limits, var = model_tables(case)
    assert limits.dtype == var.dtype == np.float32
    if f"m/{case}/limits" in FIX:
        np.testing.assert_array_equal(limits.view(np.uint32), FIX[f"m/{case}/limits"].view(np.uint32), err_msg=case)
        np.testing.assert_array_equal(var.view(np.uint32), FIX[f"m/{case}/var"].view(np.uint32), err_msg=case)
    else:
        assert _sha(limits) == str(FIX[f"m/{case}/limits_sha"]), case
        assert _sha(var) == str(FIX[f"m/{case}/var_sha"]), case


@pytest.mark.parametrize("case", MATRIX)
def test_kclass_from_limits(case):
    k = int(FIX[f"m/{case}/k"])
    limits = FIX[f"m/{case}/limits"] if f"m/{case}/limits" in FIX else model_tables(case)[0]   # (the latter checked above)
    got = jenks.kclass_from_limits(limits, FIX[f"m/{case}/sample"], k)
    assert got.dtype == np.float32 and got.shape == (k + 1,)
    np.testing.assert_array_equal(got.view(np.uint32), FIX[f"m/{case}/kclass"].view(np.uint32), err_msg=case)


def test_the_two_warning_paths_are_covered():
    texts = {c: FIX[f"e/{c}/warn"].tolist() for c, _, _ in gen.e2e_cases() if f"e/{c}/warn" in FIX}
    assert texts["f32_three_values_k5"] == ["Warning: natural_breaks Warning: Not enough unique values in data array for 5 classes. "
                                            "n_samples=3 should be >= n_clusters=5. Using k=3 instead."]
    assert all(not t for c, t in texts.items() if c != "f32_three_values_k5")


def test_public_surface():
    sig = inspect.signature(xs.natural_breaks)
    assert list(sig.parameters) == ["agg", "num_sample", "name", "k"]
    assert [p.default for p in sig.parameters.values()][1:] == [20000, "natural_breaks", 5]
    assert xs.natural_breaks is jenks.natural_breaks
    assert not hasattr(xs.classify, "natural_breaks")
    if gen.rx.have_reference():
        import ast
        tree = ast.parse(open(os.path.join(gen.rx.REF_PKG, "classify.py")).read())
        ref = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "natural_breaks")
        assert [a.arg for a in ref.args.args] == list(sig.parameters)
        assert [ast.literal_eval(d) for d in ref.args.defaults] == [20000, "natural_breaks", 5]


def test_no_cpu_fallback():
    if xs.has_hip():
        pytest.skip("a GPU is present")
    agg = xs.DataArray(np.arange(12, dtype=np.float32).reshape(3, 4))
    with pytest.raises(xs.XrsError):
        xs.natural_breaks(agg, k=2)
    with pytest.raises(xs.XrsError):
        jenks.jenks_matrices(np.arange(5, dtype=np.float32), 2)


def test_dask_and_sharded_rasters_are_refused(monkeypatch):
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = xs.DataArray(fake_dask.from_array(np.zeros((8, 8)), (4, 4)), dims=("y", "x"))
    with pytest.raises(NotImplementedError, match="dask"):
        xs.natural_breaks(lazy)


def test_abi_argument_checks_come_before_any_device_work():
    lib = _lib.load()
    p = ctypes.c_void_p(256)

    def refused(rc, text):
        assert rc != 0 and text in _lib.last_error(), _lib.last_error()

    up = lambda v: (v + 255) & ~255                                                   # noqa: E731
    assert lib.xrs_jenks_workspace_bytes(1000, 5) == 2 * up(1001 * 4)
    assert lib.xrs_jenks_workspace_bytes(0, 5) == lib.xrs_jenks_workspace_bytes(10, 0) == lib.xrs_jenks_workspace_bytes(1 << 24, 2) == 0
    big = 1 << 20
    refused(lib.xrs_jenks_matrices_f32(p, 0, 3, p, p, p, big, None), "at least 1 value")
    refused(lib.xrs_jenks_matrices_f32(p, 10, 0, p, p, p, big, None), "at least 1 class")
    refused(lib.xrs_jenks_matrices_f32(p, 1 << 24, 3, p, p, p, 1 << 30, None), "2^24")
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        refused(lib.xrs_jenks_matrices_f32(args[0], 10, 3, args[1], args[2], args[3], big, None), "null pointer")
    refused(lib.xrs_jenks_matrices_f32(p, 1000, 5, p, p, p, 2 * up(1001 * 4) - 1, None), "workspace")
    refused(lib.xrs_gather_elems(p, 3, 10, p, 4, p, None), "1, 2, 4 or 8 bytes")
    refused(lib.xrs_gather_elems(p, 4, -1, p, 4, p, None), "negative size")
    refused(lib.xrs_gather_elems(p, 4, 10, p, -4, p, None), "negative size")
    refused(lib.xrs_gather_elems(p, 4, (1 << 32) + 1, p, 4, p, None), "2^32")
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        refused(lib.xrs_gather_elems(args[0], 4, 10, args[1], 4, args[2], None), "null pointer")
    assert lib.xrs_gather_elems(None, 4, 10, None, 0, None, None) == 0                # nothing to gather, nothing launched


@pytest.mark.skipif(not gen.rx.have_reference(), reason="the reference is not present here")
def test_fixture_reproduces():
    run = subprocess.run([sys.executable, gen.__file__, "--check"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr

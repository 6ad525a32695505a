"""Outputs of the reference's OWN natural_breaks code, executed here: tests/golden/natural_breaks_exec.npz.

Test infrastructure only, built like make_classify_exec.py (whose stand-ins it imports): _run_numpy_jenks_matrices, _run_jenks,
_compute_natural_break_bins, _run_natural_break, natural_breaks and _cpu_bin / _run_numpy_bin / _bin are lifted with `ast` from
the reference where it lies, decorators stripped, and RUN.  Nothing of the reference is copied: the fixture holds tables,
digests, bins and small outputs only; samples and rasters are regenerated from their seeds.

The typing trap.  _run_numpy_jenks_matrices is a Numba function, and as plain Python under NumPy 2 it does NOT compute what
Numba computes: `sum = 0.0; sum += np.float32(x)` stays float32 under NEP 50, where Numba types `sum` as float64.  So every
float literal of that one function is wrapped in `np.float64(...)` by an `ast` pass before it is compiled: the accumulators
are float64 then, `val * val` stays a float32 product, `variance + var_combinations[...]` is a float64 sum, the comparison
promotes the float32 minimum to float64, and the stores round to float32 -- Numba's typing of the same lines.

What is stored:
  m/<case>/sample, k        a sorted float32 sample and the class count
  m/<case>/limits, var      both tables, for up to 4096 entries each; else m/<case>/limits_sha, var_sha (sha256 of the bytes)
  m/<case>/kclass           the k + 1 class boundaries of _run_jenks on that sample
  idx/<num_data>_<num_sample>   the sample indices of _compute_natural_break_bins' own sampling lines
  e/<case>/kwargs, and bins + bins_dtype (what _cpu_bin received), sha, dtype, out (<= 4096 cells), warn (category and text
                            of the warnings raised) -- or exc, the exception type
  vec/...                   result_natural_breaks and result_natural_breaks_num_sample of the reference's tests/test_classify.py
                            with their input raster

Usage:  python tests/golden/make_natural_breaks_exec.py            (writes tests/golden/natural_breaks_exec.npz)
        python tests/golden/make_natural_breaks_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import ast
import hashlib
import os
import sys
import warnings
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_classify_exec as cx  # noqa: E402
from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "natural_breaks_exec.npz")
SMALL = 4096
LIFTED = ["_run_jenks", "_compute_natural_break_bins", "_run_natural_break", "natural_breaks", "_cpu_bin", "_run_numpy_bin", "_bin"]
INDEX_PAIRS = [(5, 3), (20, 8), (1000, 1), (77100, 600), (77100, 20000), (100001, 0)]


class _Float64Literals(ast.NodeTransformer):
    """0.0 -> np.float64(0.0): Numba's type for a float literal, which NumPy 2 gives a Python float no longer."""

    def visit_Constant(self, node):
        if isinstance(node.value, float):
            return ast.copy_location(ast.Call(func=ast.Attribute(value=ast.Name(id="np", ctx=ast.Load()), attr="float64", ctx=ast.Load()),
                                              args=[node], keywords=[]), node)
        return node


def _reference_function(name):
    with open(os.path.join(rx.REF_PKG, "classify.py")) as fh:
        tree = ast.parse(fh.read())
    return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)


def ref_jenks_matrices():
    """The reference's _run_numpy_jenks_matrices with Numba's typing restored (module docstring)."""
    fn = _reference_function("_run_numpy_jenks_matrices")
    fn.decorator_list = []
    mod = ast.Module(body=[_Float64Literals().visit(fn)], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"np": np}
    exec(compile(mod, os.path.join(rx.REF_PKG, "classify.py"), "exec"), ns)
    return ns["_run_numpy_jenks_matrices"]


def ref_sampling():
    """The sampling lines of _compute_natural_break_bins (the body of its first `if`) as f(num_data, num_sample) -> indices."""
    fn = _reference_function("_compute_natural_break_bins")
    branch = next(n for n in fn.body if isinstance(n, ast.If))
    mod = ast.Module(body=branch.body, type_ignores=[])
    code = compile(mod, os.path.join(rx.REF_PKG, "classify.py"), "exec")

    def run(num_data, num_sample):
        ns = {"np": np, "num_data": num_data, "num_sample": num_sample, "data_flat_np": np.zeros(num_data, np.int8)}
        exec(code, ns)
        return np.array(ns["sample_idx"])
    return run


def ref_natural_breaks():
    """Namespace of the lifted functions; `ns['_bins_seen']` collects the bins every _cpu_bin call received."""
    import types
    xr_stub = types.SimpleNamespace(DataArray=lambda data, **_: data)
    with open(os.path.join(rx.REF_PKG, "classify.py")) as fh:       # the other backends' runners: named, never called
        others = {n.name: None for n in ast.parse(fh.read()).body if isinstance(n, ast.FunctionDef) and n.name not in LIFTED}
    ns = rx.lift("classify.py", LIFTED, {**others, "xr": xr_stub, "ArrayTypeFunctionMapping": cx._Mapping, "partial": partial,
                                         "warnings": warnings, "dask": None})
    ns["_run_numpy_jenks_matrices"] = ref_jenks_matrices()
    cpu_bin = ns["_cpu_bin"]
    seen = ns["_bins_seen"] = []

    def fast_bin(data, bins, new_values):                   # every cell's output depends on its value alone
        seen.append(np.array(bins, copy=True))
        u, inv = np.unique(data.ravel(), return_inverse=True)
        return cpu_bin(u.reshape(1, -1), bins, new_values)[0][inv.ravel()].reshape(data.shape)

    ns["_cpu_bin"] = fast_bin
    return ns


# ---------------------------------------------------------------------------------------------------------------------
# seeded samples and rasters
# ---------------------------------------------------------------------------------------------------------------------
def matrix_cases():
    """[(name, sorted float32 sample, k)] -- regenerated bit for bit from their seeds."""
    rng = np.random.default_rng(20261019)
    out = []

    def add(name, values, k):
        out.append((name, np.sort(np.asarray(values).astype(np.float32)), int(k)))

    for n in (1, 2, 3, 63, 64, 65, 129, 600):
        values = rng.lognormal(1.0, 0.8, n)
        for k in (1, 2, 5, 9):
            if k <= n:
                add(f"lognorm_n{n}_k{k}", values, k)
    add("normal_n2049_k3", rng.normal(50.0, 12.0, 2049), 3)            # many blocks, the longest rows first
    add("ties_n90_k4", rng.integers(0, 7, 90) * 0.25, 4)               # ~7 distinct values: `>=` decides
    add("k_equals_n_n12", rng.normal(0.0, 1.0, 12), 12)
    add("tiny_n70_k3", rng.normal(0.0, 1.0, 70) * 1e-20, 3)            # squares are float32 subnormals
    add("both_signs_n100_k5", rng.normal(0.0, 300.0, 100), 5)
    return out


def e2e_cases():
    """[(name, raster, kwargs)] -- regenerated bit for bit from their seeds."""
    rng = np.random.default_rng(20261020)
    out = []
    a = rng.lognormal(2.0, 1.0, (300, 257)).astype(np.float32)
    out.append(("f32_lognorm_300x257_shuffle", cx._special(a, rng), {"num_sample": 600, "k": 5}))
    out.append(("f64_normal_40x50_all", rng.normal(100.0, 15.0, (40, 50)), {"num_sample": None, "k": 4}))
    out.append(("i32_70x30", rng.integers(-5000, 5000, (70, 30)).astype(np.int32), {"k": 3}))
    out.append(("f32_three_values_k5", np.array([[1, 1, 2, 2, 3]] * 4, dtype=np.float32), {"k": 5}))
    b = rng.normal(10.0, 3.0, (12, 17)).astype(np.float32)
    out.append(("f32_12x17_sample_above_size", cx._special(b, rng, 0.05), {"num_sample": 1000, "k": 4}))
    out.append(("f32_16x16_k1", rng.normal(0.0, 1.0, (16, 16)).astype(np.float32), {"k": 1}))
    out.append(("f32_1x1", np.array([[3.25]], np.float32), {"k": 1}))
    out.append(("f32_all_nan", np.full((9, 11), np.nan, np.float32), {}))
    return out


# ---------------------------------------------------------------------------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_all():
    ns = ref_natural_breaks()
    matrices, store = ns["_run_numpy_jenks_matrices"], {}
    for name, sample, k in matrix_cases():
        key = f"m/{name}"
        limits, var = matrices(sample, k)
        assert limits.dtype == var.dtype == np.float32
        store[f"{key}/sample"], store[f"{key}/k"] = sample, np.int64(k)
        if limits.size <= SMALL:
            store[f"{key}/limits"], store[f"{key}/var"] = limits, var
        else:
            store[f"{key}/limits_sha"], store[f"{key}/var_sha"] = np.array(_sha(limits)), np.array(_sha(var))
        store[f"{key}/kclass"] = ns["_run_jenks"](sample.copy(), k)
    sampling = ref_sampling()
    for num_data, num_sample in INDEX_PAIRS:
        store[f"idx/{num_data}_{num_sample}"] = sampling(num_data, num_sample)
    for name, a, kw in e2e_cases():
        key = f"e/{name}"
        store[f"{key}/kwargs"] = np.array(repr(kw))
        ns["_bins_seen"].clear()
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                res = np.asarray(ns["natural_breaks"](cx._agg(a.copy()), **kw))
        except NameError:
            raise
        except Exception as exc:               # noqa: BLE001  (the exception type is the expected outcome)
            store[f"{key}/exc"] = np.array(type(exc).__name__)
            continue
        store[f"{key}/warn"] = np.array([f"{w.category.__name__}: {w.message}" for w in caught if w.category is Warning], dtype=str)
        bins = ns["_bins_seen"][-1]
        store[f"{key}/bins"] = np.asarray(bins, dtype=np.float64)
        store[f"{key}/bins_dtype"] = np.array(np.asarray(bins).dtype.str)
        store[f"{key}/sha"] = np.array(cx.digest(res))
        store[f"{key}/dtype"] = np.array(res.dtype.str)
        if a.size <= SMALL:
            store[f"{key}/out"] = res
    tns = rx.lift("tests/test_classify.py", ["input_data", "result_natural_breaks", "result_natural_breaks_num_sample"],
                  {"create_test_raster": lambda data, backend='numpy': cx._agg(data)})
    store["vec/input"] = np.asarray(tns["input_data"]().data)
    for f in ("natural_breaks", "natural_breaks_num_sample"):
        for i, v in enumerate(tns[f"result_{f}"]()):
            store[f"vec/{f}/{i}"] = np.asarray(v)
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def check():
    want, got = load(), run_all()
    bad = sorted(set(want) ^ set(got))
    for k in set(want) & set(got):
        a, b = want[k], got[k]
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            bad.append(k)
    for k in sorted(bad)[:20]:
        print("MISMATCH", k)
    return not bad


if __name__ == "__main__":
    if not rx.have_reference():
        sys.exit("the reference is not present here")
    if sys.argv[1:] == ["--check"]:
        ok = check()
        print("natural_breaks_exec.npz reproduces" if ok else "natural_breaks_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")

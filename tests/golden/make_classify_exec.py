"""Outputs of the reference's OWN classify code, executed here: tests/golden/classify_exec.npz.

Test infrastructure only, built like make_reference_exec.py: the functions of xrspatial/classify.py (binary, reclassify,
equal_interval, quantile, percentiles, box_plot, std_mean, head_tail_breaks, maximum_breaks and the runners / helpers
they call) are lifted with `ast` from the reference where it lies, decorators stripped, and RUN on the seeded rasters of
`cases()`.  Nothing of the reference is copied: the fixture holds bins, output digests and small outputs only; the
rasters are regenerated from their seeds by `cases()`.

Stand-ins: xarray.DataArray returns its data, ArrayTypeFunctionMapping picks the numpy runner, cupy / dask are absent.
The two Numba loops run as plain Python, which is the same arithmetic here: _cpu_bin compares a cell with float64 bins
(NumPy promotes a float32 / integer scalar to float64, as Numba does) and assigns into a float32 array; _cpu_binary
compares with `np.any(values == cell)`.  For speed both run on the distinct values of a raster (np.unique, NaN once)
and the result is scattered back -- every cell's output depends on its value alone.  _cpu_binary pre-fills an array of
the input dtype with NaN, which NumPy refuses for an integer dtype (Numba stores an undefined integer that no cell keeps,
since every integer cell is finite): integer rasters run on their float64 image and the 0 / 1 result is cast back.

Per case and function the fixture stores the bins _cpu_bin received (`<case>/<fn>/bins`, with their dtype), the output's
sha256 (`.../sha`), the full output for rasters of <= 4096 cells (`.../out`), or the exception type (`.../exc`).  Per case
it also stores what the host bin builders consume: the finite count / min / max, numpy's nanmean / nanstd of the
inf-cleaned raster, and the head/tail means.  `vec/...` holds the expected arrays of the reference's
tests/test_classify.py fixtures and their input raster.

Usage:  python tests/golden/make_classify_exec.py            (writes tests/golden/classify_exec.npz)
        python tests/golden/make_classify_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import ast
import contextlib
import hashlib
import io
import os
import sys
import types
import warnings
from functools import partial

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "classify_exec.npz")
SMALL = 4096
FUNCS = ("binary", "reclassify", "equal_interval", "quantile", "percentiles", "box_plot", "std_mean", "head_tail_breaks",
         "maximum_breaks")
LIFTED = ["_cpu_binary", "_run_numpy_binary", "binary", "_cpu_bin", "_run_numpy_bin", "_bin", "reclassify", "_run_quantile",
          "_quantile", "quantile", "_run_equal_interval", "equal_interval", "_run_std_mean", "std_mean",
          "_compute_head_tail_bins", "_run_head_tail_breaks", "head_tail_breaks", "_run_percentiles", "percentiles",
          "_compute_maximum_break_bins", "_run_maximum_breaks", "maximum_breaks", "_run_box_plot", "box_plot"]


class _Mapping:
    def __init__(self, numpy_func=None, **_):
        self.numpy_func = numpy_func

    def __call__(self, agg):
        return self.numpy_func


def _agg(data):
    return types.SimpleNamespace(data=data, dims=("y", "x"), coords={}, attrs={}, name=None)


def ref_classify():
    """Namespace of the lifted functions; `ns['_bins_seen']` collects the bins every _cpu_bin call received."""
    xr_stub = types.SimpleNamespace(DataArray=lambda data, **_: data)
    with open(os.path.join(rx.REF_PKG, "classify.py")) as fh:       # the other backends' runners: named, never called
        others = {n.name: None for n in ast.parse(fh.read()).body if isinstance(n, ast.FunctionDef) and n.name not in LIFTED}
    ns = rx.lift("classify.py", LIFTED, {**others, "xr": xr_stub, "ArrayTypeFunctionMapping": _Mapping, "partial": partial,
                                         "warnings": warnings, "dask": None})
    cpu_bin, cpu_binary = ns["_cpu_bin"], ns["_cpu_binary"]
    seen = ns["_bins_seen"] = []

    def by_value(data, fn):
        u, inv = np.unique(data.ravel(), return_inverse=True)
        return fn(u.reshape(1, -1))[0][inv.ravel()].reshape(data.shape)

    def fast_bin(data, bins, new_values):
        seen.append(np.array(bins, copy=True))
        return by_value(data, lambda u: cpu_bin(u, bins, new_values))

    def fast_binary(data, values):
        if data.dtype.kind != "f":
            return by_value(data, lambda u: cpu_binary(u.astype(np.float64), values).astype(data.dtype))
        return by_value(data, lambda u: cpu_binary(u, values))

    ns["_cpu_bin"], ns["_cpu_binary"] = fast_bin, fast_binary
    return ns


# ---------------------------------------------------------------------------------------------------------------------
# seeded rasters
# ---------------------------------------------------------------------------------------------------------------------
def _special(a, rng, frac=0.02):
    """NaN, +-inf, +-0.0 and subnormal cells sprinkled over a float raster."""
    a = a.copy()
    n = a.size
    flat = a.reshape(-1)
    tiny = np.finfo(a.dtype).smallest_subnormal
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, 3 * tiny]
    idx = rng.choice(n, size=max(len(specials), int(n * frac)), replace=False)
    for j, i in enumerate(idx):
        flat[i] = specials[j % len(specials)]
    return a


def cases():
    """[(name, raster, {function: kwargs})] -- regenerated bit for bit from their seeds."""
    out = []
    rng = np.random.default_rng(20261015)
    default = {"binary": {"values": [1, 2, 3]}, "reclassify": {"bins": [10, 15, np.inf], "new_values": [1, 2, 3]},
               "equal_interval": {}, "quantile": {}, "percentiles": {}, "box_plot": {}, "std_mean": {},
               "head_tail_breaks": {}, "maximum_breaks": {}}

    def add(name, a, **over):
        kw = {f: dict(v) for f, v in default.items()}
        for f, v in over.items():
            kw[f] = v
        out.append((name, a, kw))

    # float32 with every special value, heavy-tailed
    a = (rng.lognormal(2.0, 1.0, (1010, 1000))).astype(np.float32)
    add("f32_lognorm_1010x1000", _special(a, rng),
        binary={"values": [0.0, np.inf, float(a[3, 3]), float(a[7, 9])]},
        reclassify={"bins": [1.0, 5.0, 5.0, 20.0, np.inf], "new_values": [1.5, 2, 3, 4.25, 1e10]},
        quantile={"k": 7}, equal_interval={"k": 6}, maximum_breaks={"k": 6}, percentiles={"pct": [5, 25, 50, 75, 95]})
    # float64 normal with specials, 1024 x 1024
    b = rng.normal(100.0, 15.0, (1024, 1024))
    add("f64_normal_1024", _special(b, rng),
        reclassify={"bins": [120.0, 80.0, np.nan, 100.0], "new_values": [1, 2, 3, 4]},
        quantile={"k": 10}, box_plot={"hinge": 0.75})
    # heavy ties: few distinct float32 values
    c = rng.integers(0, 9, (512, 700)).astype(np.float32) * np.float32(0.5)
    c[rng.random(c.shape) < 0.01] = np.nan
    add("f32_ties_512x700", c, quantile={"k": 12}, maximum_breaks={"k": 8},
        reclassify={"bins": [3.0, 1.0, 2.0, 2.0, 4.0], "new_values": [10, 20, 30, 40, 50]},
        binary={"values": [0.5, 1.0, 99]})
    # int32 and uint8 rasters
    d = rng.integers(-5000, 5000, (300, 257)).astype(np.int32)
    add("i32_300x257", d, binary={"values": [0, 17, -3]}, reclassify={"bins": [-1000, 0, 2500, 5000], "new_values": [0, 1, 2, 3]},
        quantile={"k": 5}, maximum_breaks={"k": 4})
    e = rng.integers(0, 256, (200, 180)).astype(np.uint8)
    add("u8_200x180", e, binary={"values": [0, 255, 7]}, reclassify={"bins": [50, 100, 200, 255], "new_values": [1, 2, 3, 4]},
        maximum_breaks={"k": 5})
    # fewer unique values than k; all-equal; all-NaN; k = 1
    f = np.array([[1, 1, 2, 2, 3]] * 4, dtype=np.float32)
    add("f32_three_values", f, quantile={"k": 5}, maximum_breaks={"k": 5}, equal_interval={"k": 4})
    add("f32_all_equal", np.full((33, 17), 2.5, np.float32))
    add("f32_all_nan", np.full((9, 11), np.nan, np.float32))
    g = rng.normal(0.0, 1.0, (64, 48)).astype(np.float32)
    add("f32_k1", _special(g, rng, 0.05), quantile={"k": 1}, equal_interval={"k": 1}, maximum_breaks={"k": 1})
    # shapes
    add("f32_1x1", np.array([[3.25]], np.float32))
    h = rng.normal(10.0, 3.0, (1, 777)).astype(np.float32)
    add("f32_1xN", _special(h, rng, 0.02))
    add("f64_Nx1", _special(rng.uniform(-1e3, 1e3, (901, 1)), rng, 0.02), maximum_breaks={"k": 3})
    return out


# ---------------------------------------------------------------------------------------------------------------------
def _digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def host_inputs(a):
    """What the host bin builders consume, computed by NumPy the way the reference computes it."""
    fin = a[np.isfinite(a)]
    clean = np.where(np.isinf(a), np.nan, a)
    r = {"count": np.int64(fin.size)}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        r["min"] = np.float64(float(np.nanmin(clean)) if clean.size else np.nan)
        r["max"] = np.float64(float(np.nanmax(clean)) if clean.size else np.nan)
        r["mean"] = np.float64(float(np.nanmean(clean)))
        r["std"] = np.float64(float(np.nanstd(clean)))
    means, data = [], fin.copy()
    while len(data) > 1:                      # the head means of _compute_head_tail_bins, and the head sizes
        mv = float(np.nanmean(data))
        head = data[data > mv]
        means.append((mv, len(data), len(head)))
        if len(head) == 0 or len(head) / len(data) > 0.40:
            break
        data = head
    r["ht"] = np.array(means, dtype=np.float64).reshape(-1, 3)
    return r


def run_all():
    ns = ref_classify()
    store = {}
    for name, a, kw in cases():
        for k, v in host_inputs(a).items():
            store[f"{name}/in/{k}"] = v
        for fn in FUNCS:
            key = f"{name}/{fn}"
            store[f"{key}/kwargs"] = np.array(repr(kw[fn]))
            ns["_bins_seen"].clear()
            try:
                with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()) as so:
                    warnings.simplefilter("ignore")
                    res = np.asarray(ns[fn](_agg(a.copy()), **kw[fn]))
            except NameError:
                raise
            except Exception as exc:           # noqa: BLE001  (the exception type is the expected outcome)
                store[f"{key}/exc"] = np.array(type(exc).__name__)
                continue
            if so.getvalue():
                store[f"{key}/stdout"] = np.array(so.getvalue())
            if ns["_bins_seen"]:
                bins = ns["_bins_seen"][-1]
                store[f"{key}/bins"] = np.asarray(bins, dtype=np.float64)
                store[f"{key}/bins_dtype"] = np.array(np.asarray(bins).dtype.str)
            store[f"{key}/sha"] = np.array(_digest(res))
            store[f"{key}/dtype"] = np.array(res.dtype.str)
            if a.size <= SMALL:
                store[f"{key}/out"] = res
    # the reference's own test vectors (tests/test_classify.py fixtures)
    tns = rx.lift("tests/test_classify.py", ["input_data", "result_binary", "result_reclassify", "result_quantile",
                                             "result_equal_interval", "result_std_mean", "result_head_tail_breaks",
                                             "result_percentiles", "result_maximum_breaks", "result_box_plot"],
                  {"create_test_raster": lambda data, backend='numpy': _agg(data)})
    store["vec/input"] = np.asarray(tns["input_data"]().data)
    for f in ("binary", "reclassify", "quantile", "equal_interval", "std_mean", "head_tail_breaks", "percentiles",
              "maximum_breaks", "box_plot"):
        r = tns[f"result_{f}"]()
        r = r if isinstance(r, tuple) else (r,)
        for i, v in enumerate(r):
            store[f"vec/{f}/{i}"] = np.asarray(v)
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def digest(a):
    return _digest(a)


def check():
    want = load()
    got = run_all()
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
        print("classify_exec.npz reproduces" if ok else "classify_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")

"""Outputs of the reference's OWN local code, executed here: tests/golden/local_exec.npz.

Test infrastructure only, built like make_proximity_exec.py: the nine functions of xrspatial/local.py and its `funcs` table are
lifted with `ast` from the reference where it lies and RUN as plain Python on the cases of `cases()`, with a small stand-in for
`xr.Dataset` / `xr.DataArray` (`.data_vars`, `[name].data`, `DataArray(data, attrs)`).  Nothing of the reference is copied: the
fixture holds the inputs of `cases()` and the outputs.

Keys of a case: `<case>/planes` ((N, h, w), one dtype) or `<case>/plane<j>` (mixed dtypes); `<case>/ref_freq`, `<case>/ref_rank`
and, where popularity runs, `<case>/ref_pop`; `<case>/outputs` ((F, h, w) float64: the reference's values, NaN included, one row
for each of `functions_of(case)`); `<case>/combine` and `<case>/combine_key_values` ((classes, planes) float64: the key's tuples
in the order of its ids 1 .. classes; combine was given as many leading planes as this has columns).

`ref_rank` holds 1 .. n, n + 1 .. n + 2 and 1 - n .. 0, for which `ref - 1` is -n .. -1 and Python's indexing wraps; `ref_pop`
the same around u, the cell's number of distinct values: 1 - u .. u + 2.  Values below, where the reference raises IndexError,
are kept out.

Usage:  python tests/golden/make_local_exec.py            (writes tests/golden/local_exec.npz; a few seconds)
        python tests/golden/make_local_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import os
import sys
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "local_exec.npz")
MAX_BYTES = 200_000
STATS = ("max", "mean", "median", "min", "std", "sum")
FREQUENCIES = ("lesser_frequency", "equal_frequency", "greater_frequency")
POSITIONS = ("lowest_position", "highest_position")
LIFTED = ["funcs", "cell_stats", "combine", "lesser_frequency", "equal_frequency", "greater_frequency", "lowest_position",
          "highest_position", "popularity", "rank"]
N_LIST = (2, 3, 7, 8, 9, 15, 16, 17, 24, 33, 64)       # (one variable: the reference fails, `np.nditer` of one array yields no tuples)


# ------------------------------------------------------------------ the stand-in for xarray
class _DataArray:
    def __init__(self, data=None, attrs=None):
        self.data = data
        self.attrs = attrs or {}


class _Dataset:
    def __init__(self, variables):
        self.data_vars = dict(variables)

    def __getitem__(self, name):
        return self.data_vars[name]


class _Xr:
    Dataset = _Dataset
    DataArray = _DataArray


def ref_functions():
    return rx.lift("local.py", LIFTED, {"xr": _Xr, "Counter": Counter})


# ------------------------------------------------------------------ cases
def _nan(planes, rng, share):
    """NaN in about `share` of the cells (one plane each), at least one cell where the raster has ten or more"""
    if not share or planes[0].dtype.kind != "f":
        return
    h, w = planes[0].shape
    hit = rng.random((h, w)) < share
    if h * w >= 10 and not hit.any():
        hit[h // 2, w // 2] = True
    which = rng.integers(0, len(planes), (h, w))
    for j, p in enumerate(planes):
        if p.dtype.kind == "f":
            p[hit & (which == j)] = np.nan
    first_float = next(p for p in planes if p.dtype.kind == "f")
    first_float[hit & ~np.isin(which, [j for j, p in enumerate(planes) if p.dtype.kind == "f"])] = np.nan


def _distinct(planes):
    v = np.stack([p.astype(np.float64) for p in planes])
    s = np.sort(v, axis=0)
    return 1 + (s[1:] != s[:-1]).sum(axis=0)


def _case(planes, rng, nan_share=0.0, popular=False, combine_vars=None, ref_freq=None, ref_dtype=np.int32):
    planes = [np.ascontiguousarray(p) for p in planes]
    _nan(planes, rng, nan_share)
    n, shape = len(planes), planes[0].shape
    lo = 0 if np.dtype(ref_dtype).kind == "u" else 1 - n
    c = dict(planes=planes, popular=popular, combine_vars=n if combine_vars is None else combine_vars)
    c["ref_rank"] = rng.integers(lo, n + 3, shape).astype(ref_dtype)
    if popular:
        u = _distinct([np.where(np.isnan(p), 0, p) if p.dtype.kind == "f" else p for p in planes])
        span = rng.random(shape)
        low = 0 if np.dtype(ref_dtype).kind == "u" else 1 - u
        c["ref_pop"] = np.floor(low + span * (u + 3 - low)).astype(np.int64).astype(ref_dtype)      # 1 - u .. u + 2
    if ref_freq is None:
        pick = rng.integers(0, n, shape)
        ref_freq = np.choose(pick, planes) if n <= 32 else np.where(pick % 2 == 0, planes[0], planes[-1])
        if ref_freq.dtype.kind == "f":
            ref_freq = np.where(rng.random(shape) < 0.1, np.nan, ref_freq).astype(ref_freq.dtype)
    c["ref_freq"] = np.ascontiguousarray(ref_freq)
    return c


def cases():
    """[(name, case)], deterministic"""
    out = []
    rng = np.random.default_rng(2024)
    # the sizes of the docstring examples
    out.append(("doc_2x2", _case([np.array([[1, 2], [3, 4]], np.float64), np.array([[4, 2], [1, 4]], np.float64),
                                  np.array([[2, 2], [0, 1]], np.float64)], rng, popular=True)))
    a = np.arange(16, dtype=np.float64).reshape(4, 4) % 5
    out.append(("doc_4x4", _case([a, a.T.copy(), (a * 2) % 3, a[::-1].copy()], rng, nan_share=0.05, popular=True)))
    for shape in ((1, 1), (1, 7), (9, 1)):
        out.append((f"shape_{shape[0]}x{shape[1]}", _case([rng.normal(size=shape) for _ in range(3)], rng)))
        out.append((f"sets_{shape[0]}x{shape[1]}", _case([rng.integers(1, 3, shape).astype(np.float32) for _ in range(3)], rng,
                                                         popular=shape != (1, 1))))
    # 3 x 5, every N: full-mantissa values (the pairwise order shows), NaN in 0 and 5 % of the cells
    for n in N_LIST:
        out.append((f"f64_n{n}", _case([rng.normal(scale=100.0, size=(3, 5)) for _ in range(n)], rng, nan_share=0.05 * (n % 2),
                                       combine_vars=min(n, 3))))
    for n in (2, 7, 8, 9, 16, 17, 33):
        out.append((f"f32_n{n}", _case([rng.normal(scale=100.0, size=(3, 5)).astype(np.float32) for _ in range(n)], rng,
                                       nan_share=0.05 * (1 - n % 2), combine_vars=min(n, 3))))
    # values from small sets: equal_frequency, popularity, combine
    for n in N_LIST:
        hi = 3 if n <= 3 else 5
        out.append((f"sets_f64_n{n}", _case([rng.integers(1, hi, (3, 5)).astype(np.float64) for _ in range(n)], rng,
                                            nan_share=0.05 * (n % 2), popular=True)))
    for n in (2, 8, 17, 64):
        out.append((f"sets_i32_n{n}", _case([rng.integers(-2 if n > 3 else 0, 3 if n > 3 else 2, (3, 5)).astype(np.int32) for _ in range(n)], rng,
                                            popular=True)))
    out.append(("sets_i64_n9", _case([rng.integers(1, 5, (3, 5)).astype(np.int64) * 3_000_000_000 for _ in range(9)], rng,
                                     popular=True, ref_dtype=np.int64)))
    out.append(("sets_i64_n3_u8ref", _case([rng.integers(1, 3, (3, 5)).astype(np.int64) for _ in range(3)], rng, popular=True,
                                           ref_dtype=np.uint8)))
    mix = lambda shape: [rng.integers(1, 4, shape).astype(np.float32), rng.integers(1, 4, shape).astype(np.float64),      # noqa: E731
                         rng.integers(1, 4, shape).astype(np.int16)]
    out.append(("mixed_3x5", _case(mix((3, 5)), rng, nan_share=0.05, popular=True)))
    # more than a row, odd widths; few distinct values, so that the outputs compress
    out.append(("mixed_9x11", _case(mix((9, 11)), rng, nan_share=0.05, popular=True)))
    out.append(("sets_f32_37x53_n3", _case([rng.integers(1, 5, (37, 53)).astype(np.float32) * 0.1 for _ in range(3)], rng,
                                           nan_share=0.05, popular=True)))
    out.append(("sets_i32_9x11_n9", _case([rng.integers(1, 5, (9, 11)).astype(np.int32) for _ in range(9)], rng, popular=True,
                                          combine_vars=3)))
    out.append(("sets_f64_9x11_n17", _case([rng.integers(1, 5, (9, 11)).astype(np.float64) for _ in range(17)], rng, popular=True,
                                           combine_vars=4)))
    # a float32 ref_var against float64 data that differ below float32 resolution
    base = rng.integers(1, 4, (3, 5)).astype(np.float32) + np.float32(0.1)
    data = [base.astype(np.float64) + e for e in (0.0, 1e-9, -1e-9)] + [rng.integers(1, 4, (3, 5)).astype(np.float64)]
    out.append(("f32_ref_below_resolution", _case(data, rng, ref_freq=base)))
    out.append(("f32_ref_int_data", _case([rng.integers(16777215, 16777219, (3, 5)).astype(np.int32) for _ in range(3)], rng,
                                          ref_freq=np.full((3, 5), 16777216, np.float32), popular=True)))
    return out


# ------------------------------------------------------------------ running the reference
def reference(ns, c):
    """{key: array} of one case"""
    planes = c["planes"]
    n = len(planes)
    names = [f"v{j:02d}" for j in range(n)]
    variables = {name: _DataArray(p.copy()) for name, p in zip(names, planes)}
    for r in ("ref_freq", "ref_rank", "ref_pop"):
        if r in c:
            variables[r] = _DataArray(c[r].copy())
    ds = _Dataset(variables)
    shape = planes[0].shape
    rows, funcs = [], []

    def keep(name, res):
        assert isinstance(res, _DataArray) and res.data.shape == shape, name
        funcs.append(name)
        rows.append(np.asarray(res.data, np.float64))

    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for f in STATS:
                keep(f, ns["cell_stats"](ds, names, f))
            for f in FREQUENCIES:
                keep(f, ns[f](ds, "ref_freq", names))
            for f in POSITIONS:
                keep(f, ns[f](ds, names))
            keep("rank", ns["rank"](ds, "ref_rank", names))
            if c["popular"]:
                keep("popularity", ns["popularity"](ds, "ref_pop", names))
            comb = ns["combine"](ds, names[:c["combine_vars"]])
    assert funcs == functions_of(c), funcs
    out = {"outputs": np.stack(rows), "combine": np.asarray(comb.data, np.float64)}
    key = comb.attrs["key"]
    assert list(key.keys()) == list(range(1, len(key) + 1)), "the ids of the key are 1 .. classes, in this order"
    out["combine_key_values"] = np.array([list(v) for v in key.values()], np.float64).reshape(len(key), c["combine_vars"])
    return out


def functions_of(case):
    """the names of the rows of `outputs`; `case`: of cases(), or {key: array} of a stored case"""
    return list(STATS + FREQUENCIES + POSITIONS) + ["rank"] + (["popularity"] if "ref_pop" in case else [])


def stored(store, name):
    """{key: array} of one case of a loaded fixture"""
    return {k.split("/", 1)[1]: v for k, v in store.items() if k.startswith(name + "/")}


def complaints(name, c, got):
    bad = []
    if c["popular"] and c["planes"][0].size > 1:
        share = np.isfinite(got["outputs"][functions_of(c).index("popularity")]).mean()
        if share < 0.25:
            bad.append(f"{name}: popularity is a number at {share:.0%} of the cells only")
    classes = len(got["combine_key_values"])
    if c["planes"][0].size > 1 and not 2 <= classes <= 400:
        bad.append(f"{name}: combine finds {classes} classes")
    return bad


def run_all():
    ns = ref_functions()
    store, bad = {}, []
    for name, c in cases():
        planes = c["planes"]
        if len({p.dtype for p in planes}) == 1:
            store[f"{name}/planes"] = np.stack(planes)
        else:
            for j, p in enumerate(planes):
                store[f"{name}/plane{j}"] = p
        for r in ("ref_freq", "ref_rank", "ref_pop"):
            if r in c:
                store[f"{name}/{r}"] = c[r]
        got = reference(ns, c)
        bad += complaints(name, c, got)
        for k, v in got.items():
            store[f"{name}/{k}"] = v
    return store, bad


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def names(store):
    return sorted({k.split("/")[0] for k in store})


def planes_of(store, name):
    if f"{name}/planes" in store:
        return list(store[f"{name}/planes"])
    out = []
    while f"{name}/plane{len(out)}" in store:
        out.append(store[f"{name}/plane{len(out)}"])
    return out


def check():
    want = load()
    got, _ = run_all()
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
        print("local_exec.npz reproduces" if ok else "local_exec.npz differs")
        sys.exit(0 if ok else 1)
    st, bad = run_all()
    for line in bad:
        print("REFUSED", line)
    if bad:
        sys.exit(1)
    np.savez_compressed(OUT, **st)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {len(st)} arrays of {len(names(st))} cases, {size} bytes")
    if size > MAX_BYTES:
        sys.exit(f"{size} bytes is above the {MAX_BYTES} allowed")

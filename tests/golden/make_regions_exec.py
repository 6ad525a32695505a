"""Outputs of the reference's OWN regions code, executed here: tests/golden/regions_exec.npz.

Test infrastructure only, built like make_reference_exec.py: `_area_connectivity` (xrspatial/zonal.py:1406-1549) is
lifted with `ast` from the reference where it lies, its `@ngjit` decorator stripped, and RUN as plain Python on the
seeded rasters of `cases()`, with both neighbourhoods.  Nothing of the reference is copied: the fixture holds inputs and
outputs only.

Which dtypes: float64 and the eight integer dtypes -- those on which the plain-Python run and the reference's Numba run
compute the same thing, each raster within its dtype's label limit.  For float64 both type every step
in float64.  For the integer dtypes Numba types `src_window - val` and `np.abs(...)` in the array's own dtype with
wrap-around (no overflow checks in nopython mode), promotes `rtol * np.abs(val)` to float64 and compares in float64;
NumPy 2 does the same (array - scalar of one dtype stays in it and wraps silently; `np.abs` of an integer array keeps its
dtype, so abs(int8(-128)) == -128; the float64 scalar threshold is a strong type, so `<=` promotes to float64).  That
agreement is argued from the two typing rules, as make_reference_exec.py argues its own cases; Numba is not installed
in the build image, so it is not executed.  float32 is left out: NumPy 2 keeps `1e-05 * abs(v)` in float32, where Numba
computes it in float64; tests/regions_oracle.py restates the Numba typing and the tests check float32 against that.

Cases: the reference's docstring arrays and those of its tests/test_zonal.py regions tests; NaN, +-inf and +-0.0;
values near the tolerance (the match is relative to the centre, so not symmetric); integer extremes (int8 -128 never
matches itself; differences that wrap to T_min match); 1x1, 1xN and Nx1; odd shapes up to 97x101.
Keys: `<case>/in` (the raster), `<case>/n4`, `<case>/n8` (the reference's output, in the raster's dtype).

Usage:  python tests/golden/make_regions_exec.py            (writes tests/golden/regions_exec.npz)
        python tests/golden/make_regions_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "regions_exec.npz")
INT_DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)
LIMIT = {np.dtype(np.int8): 127, np.dtype(np.uint8): 255}


def cases():
    """[(name, raster)], deterministic."""
    out = []
    add = lambda name, a: out.append((name, np.ascontiguousarray(a)))  # noqa: E731
    # the reference's docstring examples and its tests/test_zonal.py regions arrays
    add("doc_cross", np.array([[1, 1, 0, 2, 2], [1, 1, 0, 2, 2], [0, 0, 0, 0, 0], [3, 3, 0, 3, 3], [3, 3, 0, 3, 3]],
                              dtype=np.float64))
    add("doc_diag", np.array([[1, 0, 1], [0, 1, 0], [1, 0, 1]], dtype=np.float64))
    t4 = [[0, 0, 0, 0], [0, 4, 0, 0], [1, 4, 4, 0], [1, 1, 1, 0], [0, 0, 0, 0]]
    t8 = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1]]
    add("t4_int", np.array(t4, dtype=np.int64))
    f = np.array(t4, dtype=np.float64)
    f[0, 3] = np.nan
    add("t4_float", f)
    add("t8_int", np.array(t8, dtype=np.int64))
    f = np.array(t8, dtype=np.float64)
    f[0, 3] = np.nan
    add("t8_float", f)

    rng = np.random.default_rng(20261016)
    # NaN, +-inf, +-0.0
    for i, (r, c) in enumerate(((7, 9), (13, 6), (1, 17), (17, 1))):
        a = rng.choice(np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan]), (r, c))
        add(f"special_{i}", a)
    add("all_nan", np.full((5, 7), np.nan))
    add("all_inf", np.full((4, 5), np.inf))
    # near the tolerance: 1e-05 * |v| + 1e-08 relative to the centre, steps of about half of it
    for i, (r, c) in enumerate(((9, 11), (23, 19), (31, 8))):
        base = rng.choice(np.array([1000.0, -3.0, 1e-3, 0.0]))
        step = 1e-05 * abs(base) + 1e-08
        add(f"near_{i}", base + rng.integers(-2, 3, (r, c)) * step * rng.choice(np.array([0.55, 0.999, 1.0, 1.001])))
    # exact-tolerance pairs: w = v +- thr(v), and the next doubles around it
    v = 7470.702
    t = 1e-08 + 1e-05 * abs(v)
    w = np.array([v, v + t, np.nextafter(v + t, np.inf), np.nextafter(v + t, -np.inf), v - t, v, v + 2 * t])
    add("tol_edge_row", w.reshape(1, -1))
    add("tol_edge_grid", np.resize(w, (6, 7)))
    # integer extremes and small values
    for dt in INT_DTYPES:
        info = np.iinfo(dt)
        pool = np.array(sorted({info.min, info.min + 1, info.max, info.max - 1, 0, 1, -1 % (info.max + 1) if info.min == 0
                                else -1}), dtype=dt)
        for i, (r, c) in enumerate(((1, 1), (1, 13), (11, 1), (9, 11))):
            add(f"{np.dtype(dt).name}_ext_{i}", rng.choice(pool, (r, c)))
        add(f"{np.dtype(dt).name}_small", rng.integers(0, 3, (11, 11)).astype(dt))
    # wrapped differences that land on T_min: int8 centre -1, neighbour 127 (127 - -1 wraps to -128 <= thr)
    add("int8_wrap", np.array([[-1, 127, -1], [127, -1, 127], [-1, -1, 0]], dtype=np.int8))
    add("int16_wrap", np.array([[-1, 32767, -1, 5], [32767, -1, 32767, 5]], dtype=np.int16))
    # large-magnitude integers, where a difference of 1 is within the tolerance
    add("int64_big", (np.int64(2) ** 60 + rng.integers(-3, 4, (9, 10))).astype(np.int64))
    add("uint64_big", (np.uint64(2) ** 62 + rng.integers(0, 5, (9, 10)).astype(np.uint64)).astype(np.uint64))
    add("int32_big", (2 ** 30 + rng.integers(-30000, 30000, (10, 9))).astype(np.int32))
    # odd shapes, larger
    for i, (r, c) in enumerate(((1, 1), (1, 2), (2, 1), (37, 41), (97, 101), (64, 65), (33, 64))):
        a = rng.integers(0, 3, (r, c)).astype(np.float64)
        a[rng.random(a.shape) < 0.05] = np.nan
        add(f"shape_{i}", a)
    add("shape_i32", rng.integers(0, 2, (61, 67)).astype(np.int32))
    add("shape_u16", (rng.random((45, 80)) < 0.6).astype(np.uint16))
    return out


def ref_area_connectivity():
    return rx.lift("zonal.py", ["_area_connectivity"])["_area_connectivity"]


def run_all():
    fn = ref_area_connectivity()
    store = {}
    for name, a in cases():
        store[f"{name}/in"] = a
        for n in (4, 8):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                out = np.asarray(fn(a.copy(), n))
            assert out.dtype == a.dtype, name
            lim = LIMIT.get(a.dtype)
            assert lim is None or out.max() <= lim, (name, "beyond the dtype's label limit")
            store[f"{name}/n{n}"] = out
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def case_names(store):
    return sorted({k.rsplit("/", 1)[0] for k in store})


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
        print("regions_exec.npz reproduces" if ok else "regions_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")

"""Outputs of the reference's OWN polygonize code, executed here: tests/golden/polygonize_exec.npz.

Test infrastructure only, built like make_regions_exec.py: `_calculate_regions`, `_merge_regions`, `_follow`, `_scan`,
`_transform_points`, `_diff_row`, `_outside_domain`, `_min_and_max` and `_polygonize_numpy`
(xrspatial/experimental/polygonize.py) are lifted with `ast` from the reference where it lies, their `@ngjit` decorators
stripped, and RUN as plain Python on the rasters of `cases()`, with both connectivities.  Nothing of the reference is copied:
the fixture holds inputs and flat outputs only.

`_is_close` is a Numba type-dispatch generator (it returns one of two lambdas by the argument TYPES) and cannot run as plain
Python; `is_close` below is a stand-in written for this file with its two branches: `==` when both are integers, else
`abs(value - reference) <= 1e-08 + 1e-05 * abs(reference)`.  `Turn` is an Enum class, which `lift` does not carry; it is
restated here as three names.

Which dtypes: float64 and the eight integer dtypes.  For float64 plain Python on NumPy scalars and Numba both type every
step in float64; for integers both compare with `==`.  float32 is left out: NumPy 2 keeps `1e-05 * abs(v)` in float32 where
Numba computes it in float64; tests/polygonize_oracle.py restates the Numba typing and the tests check
float32 against that.

Keys: `<case>/in`, optional `<case>/mask` and `<case>/transform`, and for c in (4, 8) `<case>/c<c>/column`, `/points`
(float64 [total, 2]), `/ring_offsets`, `/polygon_offsets` (int64): the reference's lists, flattened.

Usage:  python tests/golden/make_polygonize_exec.py            (writes tests/golden/polygonize_exec.npz)
        python tests/golden/make_polygonize_exec.py --check    (exit 1 unless it equals what the reference computes today)
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

OUT = os.path.join(HERE, "polygonize_exec.npz")
INT_DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64)
LIFTED = ["_regions_dtype", "_visited_dtype", "_diff_row", "_outside_domain", "_min_and_max", "_follow", "_calculate_regions",
          "_merge_regions", "_transform_points", "_scan", "_polygonize_numpy"]
FMA_TRANSFORM = (0.1, 0.3, -0.7, 0.3, -0.7, 0.1)


def serpentine(rows, cols):
    """1 on a path that fills every even row and turns at alternate ends through the odd rows; 0 elsewhere"""
    a = np.zeros((rows, cols), np.float64)
    a[0::2, :] = 1
    a[1::4, -1] = 1
    a[3::4, 0] = 1
    return a


def spiral(rows, cols):
    """1 on a one-cell-wide path that winds inwards from a corner, keeping a one-cell gap to itself; 0 elsewhere"""
    a = np.zeros((rows, cols), np.int32)
    y, x, dy, dx = 0, 0, 0, 1
    a[0, 0] = 1
    inside = lambda r, c: 0 <= r < rows and 0 <= c < cols  # noqa: E731
    while True:
        for _ in range(2):
            y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(y1, x1) and a[y1, x1] == 0 and (not inside(y2, x2) or a[y2, x2] == 0):
                y, x = y1, x1
                a[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return a


def nested(n):
    """concentric square bands of alternating value: holes in holes, islands in holes"""
    y, x = np.mgrid[0:n, 0:n]
    ring = np.minimum(np.minimum(y, x), np.minimum(n - 1 - y, n - 1 - x))
    return (ring % 2).astype(np.float64)


def cases():
    """[(name, raster, mask or None, transform or None)], deterministic."""
    out = []

    def add(name, a, mask=None, transform=None):
        out.append((name, np.ascontiguousarray(a), None if mask is None else np.ascontiguousarray(mask), transform))

    rng = np.random.default_rng(20261019)
    # the arrays of the reference's tests/test_polygonize.py, retyped as data
    for dt in (np.int64, np.float64):
        add(f"ref_2x2_{np.dtype(dt).name}", np.asarray([[0, 1], [1, 0]], dtype=dt))
    for dt in INT_DTYPES + (np.float64,):
        add(f"ref_3x3_{np.dtype(dt).name}", np.asarray([[0, 0, 1], [0, 4, 0], [0, 0, 0]], dtype=dt))
    for dt in (np.int64, np.float64):
        r = np.random.default_rng(28403)
        raster = r.integers(low=0, high=2, size=(40, 50), dtype=dt) if np.issubdtype(dt, np.integer) else \
            r.integers(low=0, high=2, size=(40, 50)).astype(dt)
        mask = np.random.default_rng(384182).uniform(0, 1, size=(40, 50)) < 0.9
        add(f"ref_big_masked_{np.dtype(dt).name}", raster, mask)
    r33 = np.asarray([[0, 0, 1], [0, 4, 0], [0, 0, 0]], dtype=np.int32)
    add("ref_transform_identity", r33, None, (1, 0, 0, 0, 1, 0))
    add("ref_transform_affine", r33, None, (1.2, -0.3, 0.2, 1.4, 0.7, 0.1))
    # 1x1, 1xN (rings of 2N + 2 states: lengths on and beside powers of two and across a wave) and Nx1 (the nx == 1 path)
    for n in (1, 2, 3, 4, 7, 8, 15, 31, 63, 64):
        add(f"row_1x{n}", np.ones((1, n), np.float64))
        add(f"col_{n}x1", np.ones((n, 1), np.int32))
    add("row_1x9_mixed", np.array([[1, 1, 2, 2, 2, 1, 3, 3, 1]], np.int16))
    add("col_9x1_mixed", np.array([[1, 1, 2, 2, 2, 1, 3, 3, 1]], np.float64).T)
    add("col_7x1_masked", np.ones((7, 1), np.float64), np.array([[1, 1, 0, 1, 0, 0, 1]], bool).T)
    # a ring with a collinear start: a hole whose lowest row is two or more pixels wide
    a = np.ones((5, 7), np.int32)
    a[2:4, 2:5] = 0
    add("hole_wide_bottom", a)
    a = np.ones((6, 8), np.float64)
    a[1, 2:4] = 0
    a[2, 1:6] = 0
    a[3:5, 5] = 3
    add("hole_two_wide_irregular", a)
    add("hole_wide_bottom_tf", np.pad(np.zeros((2, 4)), 2, constant_values=7.0), None, FMA_TRANSFORM)
    # nested holes, and islands inside holes
    add("nested_9", nested(9))
    add("nested_12", nested(12).astype(np.uint8))
    a = nested(11)
    a[5, 5] = 4
    a[3, 3:8] = 1
    add("nested_bridge", a)
    # diagonal pinches
    add("pinch_2x2", np.array([[1, 0], [0, 1]], np.float64))
    add("pinch_anti", np.array([[0, 1], [1, 0]], np.int8))
    add("pinch_chain", np.array([[1, 0, 0, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 1, 0, 1]], np.float64))
    add("pinch_diamond", np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], np.uint16))
    add("pinch_diamond_big", np.array([[0, 0, 1, 0, 0], [0, 1, 0, 1, 0], [1, 0, 2, 0, 1], [0, 1, 0, 1, 0], [0, 0, 1, 0, 0]],
                                      np.float64))
    # checkerboards
    y, x = np.mgrid[0:6, 0:7]
    add("checker_6x7", ((x + y) % 2).astype(np.float64))
    y, x = np.mgrid[0:8, 0:8]
    add("checker_8x8", ((x + y) % 2).astype(np.uint32))
    # masks: all false, random, one that cuts a region in two (none: most other cases)
    add("mask_all_false", np.ones((4, 5), np.float64), np.zeros((4, 5), bool))
    a = rng.integers(0, 3, (13, 17)).astype(np.float64)
    add("mask_random_bool", a, rng.random(a.shape) < 0.7)
    add("mask_random_int", a.astype(np.int32), (rng.integers(-1, 2, a.shape)).astype(np.int16))
    m = rng.choice(np.array([0.0, -0.0, 1.0, np.nan, 0.5]), a.shape)
    add("mask_random_float", a, m)
    m = np.ones((5, 9), bool)
    m[:, 4] = False
    add("mask_cuts_region", np.ones((5, 9), np.float64), m)
    m = np.ones((7, 7), np.uint8)
    m[3, 3] = 0
    m[1, 1:3] = 0
    add("mask_makes_holes", np.full((7, 7), 2, np.int64), m)
    # NaN and +-inf cells
    for k, shape in enumerate(((7, 9), (1, 17), (17, 1), (12, 5))):
        add(f"special_{k}", rng.choice(np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan]), shape))
    add("all_nan", np.full((3, 4), np.nan))
    add("all_inf", np.full((3, 4), np.inf))
    # float values near the tolerance (relative to the later cell, so not symmetric)
    for k, shape in enumerate(((9, 11), (23, 19))):
        base = rng.choice(np.array([1000.0, -3.0, 1e-3]))
        step = 1e-05 * abs(base) + 1e-08
        add(f"near_{k}", base + rng.integers(-2, 3, shape) * step * rng.choice(np.array([0.55, 0.999, 1.0, 1.001])))
    v = 7470.702
    t = 1e-08 + 1e-05 * abs(v)
    w = np.array([v, v + t, np.nextafter(v + t, np.inf), np.nextafter(v + t, -np.inf), v - t, v, v + 2 * t])
    add("tol_edge_row", w.reshape(1, -1))
    add("tol_edge_grid", np.resize(w, (6, 7)))
    # within the larger value's tolerance but not the smaller's: linked only when the larger is the later cell
    d = 1000.0 + 0.01000006
    add("tol_asymmetric", np.array([[1000.0, d, 1000.0], [d, 1000.0, d], [5.0, d, 1000.0]]))
    # a W-close, SW-close, W-SW-not-close triple: under connectivity 8 the SW link must not be made where the W link is
    add("tol_triple", np.array([[1.0 - 0.9e-5, 5.0], [1.0 + 0.9e-5, 1.0]]))
    add("tol_triple_wide", np.array([[9.0, 1.0 - 0.9e-5, 5.0, 1.0 + 0.9e-5], [9.0, 1.0 + 0.9e-5, 1.0, 7.0],
                                     [1.0 - 0.9e-5, 3.0, 1.0 + 0.9e-5, 1.0]]))
    # integers: == and nothing else (2^60 and 2^60 + 1 are different values)
    for dt in INT_DTYPES:
        info = np.iinfo(dt)
        pool = np.array(sorted({info.min, info.min + 1, info.max, info.max - 1, 0, 1}), dtype=dt)
        add(f"{np.dtype(dt).name}_ext", rng.choice(pool, (7, 9)))
        add(f"{np.dtype(dt).name}_small", rng.integers(0, 3, (11, 12)).astype(dt))
    add("int64_big", (np.int64(2) ** 60 + rng.integers(0, 2, (8, 9))).astype(np.int64))
    # a transform whose products round differently when fused
    a = rng.integers(0, 3, (21, 23)).astype(np.float64)
    add("transform_fma", a, None, FMA_TRANSFORM)
    add("transform_fma_masked", a.astype(np.int32), rng.random(a.shape) < 0.8, (0.3, 0.1, 0.7, -0.7, 0.3, -0.1))
    # random 3-valued rasters
    for shape in ((37, 41), (33, 65), (70, 130)):
        add(f"random_{shape[0]}x{shape[1]}", rng.integers(0, 3, shape).astype(np.float64))
    add("random_33x65_i32", rng.integers(0, 3, (33, 65)).astype(np.int32), rng.random((33, 65)) < 0.9, FMA_TRANSFORM)
    # one ring of a few thousand states each
    add("serpentine_40x70", serpentine(40, 70))
    add("spiral_40x70", spiral(40, 70))
    return out


def is_close(reference, value):
    """stand-in for the reference's `_is_close` type dispatch (polygonize.py:213-225)"""
    if isinstance(reference, (int, np.integer)) and isinstance(value, (int, np.integer)):
        return value == reference
    atol = 1e-8
    rtol = 1e-5
    return abs(value - reference) <= (atol + rtol * abs(reference))


class Turn:
    Left = -1
    Straight = 0
    Right = 1


def ref_polygonize_numpy():
    ns = rx.lift(os.path.join("experimental", "polygonize.py"), LIFTED, extra={"_is_close": is_close, "Turn": Turn})
    return ns["_polygonize_numpy"]


def flatten(column, polygons, dtype):
    rings = [ring for poly in polygons for ring in poly]
    points = np.concatenate(rings).astype(np.float64) if rings else np.empty((0, 2))
    ring_offsets = np.concatenate([[0], np.cumsum([len(ring) for ring in rings])]).astype(np.int64)
    polygon_offsets = np.concatenate([[0], np.cumsum([len(poly) for poly in polygons])]).astype(np.int64)
    return np.array(column, dtype=dtype).reshape(-1), points.reshape(-1, 2), ring_offsets, polygon_offsets


def run_all():
    fn = ref_polygonize_numpy()
    store = {}
    for name, a, mask, transform in cases():
        store[f"{name}/in"] = a
        if mask is not None:
            store[f"{name}/mask"] = mask
        if transform is not None:
            store[f"{name}/transform"] = np.asarray(transform)
        for c in (4, 8):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                column, polygons = fn(a.copy(), None if mask is None else mask.copy(), c == 8,
                                      None if transform is None else np.asarray(transform))
            for key, arr in zip(("column", "points", "ring_offsets", "polygon_offsets"), flatten(column, polygons, a.dtype)):
                store[f"{name}/c{c}/{key}"] = arr
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def case_names(store):
    return sorted({k.split("/", 1)[0] for k in store})


def same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":                                   # bit for bit
        iv = np.dtype("u%d" % a.dtype.itemsize)
        return np.array_equal(np.ascontiguousarray(a).view(iv), np.ascontiguousarray(b).view(iv))
    return np.array_equal(a, b)


def check():
    want = load()
    got = run_all()
    bad = sorted(set(want) ^ set(got))
    for k in set(want) & set(got):
        if not same(want[k], got[k]):
            bad.append(k)
    for k in sorted(bad)[:20]:
        print("MISMATCH", k)
    return not bad


if __name__ == "__main__":
    if not rx.have_reference():
        sys.exit("the reference is not present here")
    if sys.argv[1:] == ["--check"]:
        ok = check()
        print("polygonize_exec.npz reproduces" if ok else "polygonize_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")

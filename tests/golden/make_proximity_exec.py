"""Outputs of the reference's OWN proximity code, executed here: tests/golden/proximity_exec.npz.

Test infrastructure only, built like make_viewshed_exec.py: `_process` of xrspatial/proximity.py and everything it calls
(the metric codes, the three distance functions, `_distance`, `_calc_direction`, `_process_proximity_line`) are lifted with
`ast` from the reference where it lies, `ngjit` supplied as the identity and `prange` as `range`, and RUN as plain Python on
the cases of `cases()`: GDAL's four-pass line sweep, once per product.  The raster it is given is a small stand-in that has
`.data`, `.dims`, `.shape` and `[name].data`.  Nothing of the reference is copied: the fixture holds the inputs of `cases()`
and the three outputs.

The sweep is a heuristic and misses the nearest target at a few cells; the rule (tests/proximity_oracle.py)
gives a strictly smaller distance there.  A fixture in which more than 0.5 % of one case's cells or more than 0.05 % of all
cells are such misses, or in which any cell differs in another way, is not written.

Keys: `<case>/z`, `<case>/xs`, `<case>/ys`, `<case>/target_values`, `<case>/max_distance`, `<case>/metric` (the name) and
`<case>/proximity`, `<case>/allocation`, `<case>/direction` (float32).

Usage:  python tests/golden/make_proximity_exec.py            (writes tests/golden/proximity_exec.npz; about a minute)
        python tests/golden/make_proximity_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "proximity_exec.npz")
PRODUCTS = ("proximity", "allocation", "direction")
CASE_CAP, TOTAL_CAP = 0.005, 0.0005                    # share of cells the reference's sweep may miss: one case, all cases
TARGET_VALUES = [2, 3, 7]
LIFTED = ["EUCLIDEAN", "GREAT_CIRCLE", "MANHATTAN", "PROXIMITY", "ALLOCATION", "DIRECTION", "_distance_metric_mapping",
          "DISTANCE_METRICS", "euclidean_distance", "manhattan_distance", "great_circle_distance", "_distance", "_calc_direction",
          "_process_proximity_line", "_process"]


def scatter(shape, seed, density, dtype, nan_share=0.0):
    """zeros with `density` of the cells holding a value in 1 .. 9 (and `nan_share` of them NaN)"""
    rng = np.random.default_rng(seed)
    z = np.where(rng.random(shape) < density, rng.integers(1, 10, shape), 0).astype(dtype)
    if nan_share:
        z[rng.random(shape) < nan_share] = np.nan
    return z


def geo(h, w, lon0=-7.3, lat0=51.2):
    """degrees of longitude and latitude in non-integer, slightly uneven steps: on an even grid the targets k columns left
    and k columns right of a cell are equidistant under GREAT_CIRCLE, which is what the GPU test has to leave out"""
    return lon0 + 0.0137 * np.arange(w) + 0.0011 * np.sin(1.7 * np.arange(w)), lat0 - 0.0093 * np.arange(h) + 0.0008 * np.sin(2.3 * np.arange(h))


def _case(z, xs=None, ys=None, target_values=(), max_distance=np.inf, metric="EUCLIDEAN"):
    h, w = z.shape
    xs = np.arange(w, dtype=np.float64) if xs is None else np.asarray(xs)
    ys = np.arange(h, dtype=np.float64)[::-1].copy() if ys is None else np.asarray(ys)
    return dict(z=z, xs=xs, ys=ys, target_values=np.asarray(target_values, np.int64 if len(target_values) else np.float64),
                max_distance=float(max_distance), metric=metric)


def cases():
    """[(name, dict(z, xs, ys, target_values, max_distance, metric))], deterministic"""
    out = []
    doc = {"proximity": [(1, 3, 1.)], "allocation": [(1, 1, 1.), (1, 3, 2.), (2, 2, 3.)], "direction": [(2, 2, 1.), (4, 0, 1.)]}
    for name, cells in doc.items():                                  # the docstring examples: y = 4 .. 0, x = 0 .. 4, integers
        z = np.zeros((5, 5))
        for r, c, v in cells:
            z[r, c] = v
        out.append((f"doc_{name}", _case(z, np.arange(5), np.arange(5)[::-1].copy())))
    out.append(("line_1x9", _case(np.array([[0, 0, 4, 0, 0, 0, 0, 1, 0]], np.int32))))
    out.append(("line_9x1", _case(np.array([[0, 5, 0, 0, 0, 0, 0, 2, 0]], np.float32).T.copy())))
    out.append(("no_targets", _case(np.zeros((6, 7), np.float32))))
    out.append(("all_targets", _case(np.random.default_rng(1).integers(1, 10, (6, 7)).astype(np.int32))))
    out.append(("ascending_y_20x25", _case(scatter((20, 25), 11, 0.03, np.float64), ys=100.0 + 2.0 * np.arange(20))))
    out.append(("descending_x_20x25", _case(scatter((20, 25), 12, 0.04, np.int32), xs=50.0 - 1.5 * np.arange(25))))
    rng = np.random.default_rng(13)
    xs, ys = np.cumsum(rng.uniform(0.2, 3.0, 25)), -np.cumsum(rng.uniform(0.5, 2.0, 20))
    out.append(("nonuniform_20x25", _case(scatter((20, 25), 14, 0.03, np.float32), xs, ys)))
    out.append(("nonuniform_20x25_max6", _case(scatter((20, 25), 15, 0.03, np.float32), xs, ys, max_distance=6.0)))
    # 37 x 53 and 64 x 96: the three metrics, four dtypes, NaN cells, target_values empty and given, max_distance set or not
    plane = lambda h, w: (3.0 + 0.1 * np.arange(w), 9.0 - 0.1 * np.arange(h))            # noqa: E731
    wide = lambda h, w: (100.0 + 2.5 * np.arange(w), 7000.0 - 70.0 * np.arange(h))      # noqa: E731
    table = [
        ("euclidean_37x53_i32_values", (37, 53), 21, 0.10, np.int32, 0.0, plane, TARGET_VALUES, np.inf, "EUCLIDEAN"),
        ("great_circle_37x53_f32_nan", (37, 53), 22, 0.02, np.float32, 0.03, geo, (), np.inf, "GREAT_CIRCLE"),
        ("manhattan_37x53_f64_nan_values", (37, 53), 23, 0.15, np.float64, 0.03, wide, TARGET_VALUES, np.inf, "MANHATTAN"),
        ("euclidean_37x53_i64", (37, 53), 24, 0.004, np.int64, 0.0, wide, (), np.inf, "EUCLIDEAN"),
        ("euclidean_64x96_f64_nan_max", (64, 96), 25, 0.01, np.float64, 0.02, None, (), 9.5, "EUCLIDEAN"),
        ("great_circle_64x96_i64_values", (64, 96), 26, 0.08, np.int64, 0.0, geo, TARGET_VALUES, 9000.0, "GREAT_CIRCLE"),
        ("manhattan_64x96_i32_max", (64, 96), 27, 0.02, np.int32, 0.0, None, (), 14.0, "MANHATTAN"),
        ("euclidean_64x96_f32_dense", (64, 96), 28, 0.40, np.float32, 0.0, plane, (), np.inf, "EUCLIDEAN"),
    ]
    for name, shape, seed, density, dtype, nan_share, coords, tv, md, metric in table:
        xs, ys = coords(*shape) if coords else (None, None)
        out.append((name, _case(scatter(shape, seed, density, dtype, nan_share), xs, ys, tv, md, metric)))
    # rows wider than a scan block, empty rows, targets at the two ends of a row only
    z = np.zeros((70, 300), np.float32)
    z[::7, 0] = np.arange(1, 11)
    z[::7, -1] = np.arange(11, 21)
    out.append(("comb_70x300", _case(z)))
    return out


class _Coord:
    def __init__(self, data):
        self.data = data


class _Raster:
    """what `_process` touches of a DataArray"""

    def __init__(self, z, xs, ys):
        self.data, self.dims, self.shape = z, ("y", "x"), z.shape
        self._coords = {"x": _Coord(xs), "y": _Coord(ys)}

    def __getitem__(self, name):
        return self._coords[name]


def ref_functions():
    return rx.lift("proximity.py", LIFTED, {"ngjit": lambda f: f, "prange": range})


def reference(ns, c):
    """the three products of the reference for one case"""
    out = {}
    for mode, product in enumerate(PRODUCTS):
        raster = _Raster(c["z"].copy(), c["xs"], c["ys"])
        with np.errstate(all="ignore"):
            res = ns["_process"](raster, "x", "y", c["target_values"], c["max_distance"], c["metric"], mode)
        assert res.dtype == np.float32 and res.shape == c["z"].shape, product
        out[product] = res
    return out


def misses(store, name):
    """(mask of the cells where the rule and the stored reference differ, None or a complaint)"""
    from tests import proximity_oracle as po
    z, xs, ys, tv, md, metric = call_args(store, name)
    got = po.run(z, xs, ys, tv, md, metric)
    differ = np.zeros(z.shape, bool)
    for p in PRODUCTS:
        differ |= got[p].view(np.uint32) != store[f"{name}/{p}"].view(np.uint32)
    with np.errstate(invalid="ignore"):
        below = got["proximity"] < store[f"{name}/proximity"]
    if (differ & ~below).any():
        return differ, f"{name}: {int((differ & ~below).sum())} cells differ without the rule's distance being the smaller one"
    if differ.mean() > CASE_CAP:
        return differ, f"{name}: the sweep misses {int(differ.sum())} of {differ.size} cells, above {CASE_CAP:.1%}"
    return differ, None


def complaints(store):
    bad, missed, cells = [], 0, 0
    for name in names(store):
        differ, why = misses(store, name)
        if why:
            bad.append(why)
        missed, cells = missed + int(differ.sum()), cells + differ.size
    if missed > TOTAL_CAP * cells:
        bad.append(f"the sweep misses {missed} of {cells} cells over all cases, above {TOTAL_CAP:.2%}")
    return bad, missed, cells


def run_all():
    ns = ref_functions()
    store = {}
    for name, c in cases():
        for k in ("z", "xs", "ys", "target_values"):
            store[f"{name}/{k}"] = np.asarray(c[k])
        store[f"{name}/max_distance"] = np.array(c["max_distance"], np.float64)
        store[f"{name}/metric"] = np.array(c["metric"])
        for product, res in reference(ns, c).items():
            store[f"{name}/{product}"] = res
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def names(store):
    return sorted({k.split("/")[0] for k in store})


def call_args(store, name):
    """(z, xs, ys, target_values as a list, max_distance, metric) of a stored case"""
    return (store[f"{name}/z"], store[f"{name}/xs"], store[f"{name}/ys"], store[f"{name}/target_values"].tolist(),
            float(store[f"{name}/max_distance"]), str(store[f"{name}/metric"]))


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
        print("proximity_exec.npz reproduces" if ok else "proximity_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    bad, missed, cells = complaints(st)
    for line in bad:
        print("REFUSED", line)
    if bad:
        sys.exit(1)
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes; the sweep misses {missed} of {cells} cells")

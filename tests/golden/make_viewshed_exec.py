"""Outputs of the reference's OWN viewshed code, executed here: tests/golden/viewshed_exec.npz.

Test infrastructure only, built like make_terrain_exec.py: every top-level function and constant of xrspatial/viewshed.py
except `viewshed` and `_viewshed_cpu` is lifted with `ast` from the reference where it lies, the `@ngjit` decorators stripped
(`fabs` and `PI` supplied), and RUN as plain Python on the cases of `cases()`: the radial sweep over the sorted events with
its red-black status tree.  Nothing of the reference is copied: the fixture holds the inputs of `cases()` and the outputs.

`_viewshed_cpu` (viewshed.py:1505-1586) needs xarray; its few lines around `_init_event_list`, the `lexsort` and
`_viewshed_cpu_sweep` are rebuilt in `reference_viewshed()`: the range checks, the nearest coordinate through pandas (what
`raster.sel(..., method='nearest')` asks), `np.where(coords == v)[0][0]`, the two resolutions, the event list and the sweep.
One line is NOT taken as it stands: the reference adds `observer_elev` to `raster.values[row, col]` before it casts the
raster to float64, so for a float32 raster the viewpoint's elevation is float64 under NumPy 1 promotion (float32 scalar +
Python number) and float32 under NumPy 2 (NEP 50).  Here it is the float64 sum on every NumPy: DESIGN.md §6d.

Undecorated, the lifted functions are the same arithmetic as under Numba: float64 `math.atan` / `math.sqrt` and IEEE
operations on float64 operands.

Keys: `<case>/z`, `<case>/xs`, `<case>/ys` (raster and coordinates), `<case>/args` = [x, y, observer_elev, target_elev] and
`<case>/out` (the visibility grid: 180 at the viewpoint, -1 where invisible, else the vertical angle).

Usage:  python tests/golden/make_viewshed_exec.py            (writes tests/golden/viewshed_exec.npz; about a minute)
        python tests/golden/make_viewshed_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import ast
import contextlib
import io
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "viewshed_exec.npz")
RESOLUTIONS = [(1.0, 1.0), (30.0, 30.0), (2.5, 70.0), (10.0, 0.3), (30.0, -30.0)]      # (ew, ns); the last: a descending y
EXACT = ("ramp", "stairs")                                       # exact ties: host only (tests/test_gpu_viewshed.py)


def relief(shape, seed, dtype):
    """non-integer random relief: a few smooth hills plus noise"""
    rng = np.random.default_rng(seed)
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    z = 40.0 * np.sin(xx / 5.3 + rng.uniform(0, 6)) * np.cos(yy / 4.1 + rng.uniform(0, 6)) + rng.normal(0, 6.0, shape)
    return (z + 100.0 * rng.random()).astype(dtype)


def _case(z, res=(1.0, 1.0), view=(0, 0), x0=0.0, y0=0.0, observer_elev=0, target_elev=0, nudge=0.0):
    """coordinates x0 + ew * j, y0 + ns * i; the viewpoint is asked for at cell `view` (row, col), `nudge` cells off it"""
    h, w = z.shape
    xs = x0 + res[0] * np.arange(w)
    ys = y0 + res[1] * np.arange(h)
    return dict(z=z, xs=xs, ys=ys, x=float(xs[view[1]] + nudge * res[0]), y=float(ys[view[0]] - nudge * res[1]),
                observer_elev=observer_elev, target_elev=target_elev)


def cases():
    """[(name, dict(z, xs, ys, x, y, observer_elev, target_elev))], deterministic and NaN-free unless named `nan_*`"""
    out = []
    doc = np.array([[0, 0, 1, 0, 0], [1, 3, 0, 0, 0], [10, 2, 5, 2, -1], [11, 1, 2, 9, 0]])       # the docstring example
    out.append(("doc", dict(z=doc, xs=np.linspace(1, 5, 5), ys=np.linspace(1, 4, 4), x=3, y=2, observer_elev=0, target_elev=0)))
    for obs in (5, 2):                                               # test_viewshed_flat of the reference's tests
        for tgt in (0, 1):
            out.append((f"flat_obs{obs}_tgt{tgt}", dict(z=np.full((5, 4), 1.3), xs=np.arange(4) * 0.5, ys=np.arange(5) * 1.5,
                                                       x=0, y=0, observer_elev=obs, target_elev=tgt)))
    out.append(("plane_obs0", _case(np.full((11, 13), 7.25), (30.0, 30.0), (4, 7))))   # every gradient is exactly 0
    yy, xx = np.mgrid[0:12, 0:15]
    out.append(("ramp", _case(2.0 * xx + 0.5 * yy, (1.0, 1.0), (5, 6), observer_elev=1)))
    out.append(("stairs", _case(np.floor(xx / 5.0) * 3.0 + 0.0 * yy, (2.5, 70.0), (6, 2), observer_elev=2, target_elev=1)))
    # viewpoints in the four corners, on the four edges and inside, at 20 x 30, cycling through dtypes and resolutions
    h, w = 20, 30
    views = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, 11), (h - 1, 17), (8, 0), (13, w - 1), (9, 14)]
    for i, view in enumerate(views):
        dtype = (np.float32, np.float64)[i % 2]
        res = RESOLUTIONS[i % len(RESOLUTIONS)]
        out.append((f"relief_20x30_v{i}", _case(relief((h, w), 100 + i, dtype), res, view, x0=500.0, y0=-20.0,
                                                 observer_elev=(3, 12.5, 0)[i % 3], target_elev=(0, 1.5)[i % 2],
                                                 nudge=(0.0, 0.3, -0.4)[i % 3] if 0 < view[0] < h - 1 and 0 < view[1] < w - 1 else 0.0)))
    for i, (shape, view) in enumerate([((37, 53), (20, 9)), ((64, 96), (30, 50))]):
        for j, dtype in enumerate((np.float32, np.float64)):
            res = RESOLUTIONS[(2 * i + j + 1) % len(RESOLUTIONS)]
            name = f"relief_{shape[0]}x{shape[1]}_{'f32' if dtype == np.float32 else 'f64'}"
            out.append((name, _case(relief(shape, 200 + 2 * i + j, dtype), res, view, x0=-3.0, y0=1000.0,
                                    observer_elev=(10, 4.5)[j], target_elev=(0, 2)[i])))
    for i, seed in enumerate(NAN_SEEDS):                             # NaN rasters on which the reference returns
        z = relief((20, 30), seed, np.float64)
        z[np.random.default_rng(seed).random(z.shape) < 0.04] = np.nan
        z[9 + i, :] = np.where(np.isnan(z[9 + i, :]), 50.0, z[9 + i, :])          # (the viewpoint's row holds no NaN)
        out.append((f"nan_{i}", _case(z, RESOLUTIONS[i], (9 + i, 12), observer_elev=5)))
    return out


NAN_SEEDS = (300, 301)


def ref_functions():
    """every top-level function and constant of viewshed.py except `viewshed` and `_viewshed_cpu`"""
    with open(os.path.join(rx.REF_PKG, "viewshed.py")) as fh:
        tree = ast.parse(fh.read())
    names = [n.name for n in tree.body if isinstance(n, ast.FunctionDef)]
    names += [n.targets[0].id for n in tree.body
              if isinstance(n, ast.Assign) and len(n.targets) == 1 and isinstance(n.targets[0], ast.Name)]
    names = [n for n in names if n not in ("viewshed", "_viewshed_cpu")]
    return rx.lift("viewshed.py", names, {"fabs": math.fabs, "PI": math.pi})


def reference_viewshed(ns, z, xs, ys, x, y, observer_elev, target_elev):
    """`_viewshed_cpu` without xarray (module docstring)"""
    import pandas as pd
    z, x_coords, y_coords = np.asarray(z), np.asarray(xs), np.asarray(ys)
    height, width = z.shape
    if not (x_coords.min() <= x <= x_coords.max()):
        raise ValueError("x argument outside of raster x_range")
    if not (y_coords.min() <= y <= y_coords.max()):
        raise ValueError("y argument outside of raster y_range")
    x = x_coords[pd.Index(x_coords).get_indexer([x], method="nearest")[0]]
    y = y_coords[pd.Index(y_coords).get_indexer([y], method="nearest")[0]]
    y_view = np.where(y_coords == y)[0][0]
    x_view = np.where(x_coords == x)[0][0]
    viewpoint_elev = np.float64(z[y_view, x_view]) + observer_elev
    viewpoint_target = 0.0
    if abs(target_elev) > 0:
        viewpoint_target = target_elev
    ew_res = (x_coords[-1] - x_coords[0]) / (width - 1)
    ns_res = (y_coords[-1] - y_coords[0]) / (height - 1)
    visibility_grid = np.empty(shape=z.shape, dtype=np.float64)
    visibility_grid.fill(ns["INVISIBLE"])
    data = np.zeros(shape=(3, width), dtype=np.float64)
    event_list = np.zeros((3 * (height * width - 1), 7), dtype=np.float64)
    z64 = z.astype(np.float64)
    with contextlib.redirect_stdout(io.StringIO()):                  # (the sweep prints a remark per out-of-span node)
        ns["_init_event_list"](event_list=event_list, raster=z64, vp_row=y_view, vp_col=x_view, data=data,
                               visibility_grid=visibility_grid)
        event_list = event_list[np.lexsort((event_list[:, ns["E_TYPE_ID"]], event_list[:, ns["E_ANG_ID"]]))]
        event_rcts = np.array(event_list[:, :3], dtype=np.int64)
        event_aes = np.array(event_list[:, 3:], dtype=np.float64)
        return ns["_viewshed_cpu_sweep"](z64, y_view, x_view, viewpoint_elev, viewpoint_target, ew_res, ns_res, event_rcts,
                                         event_aes, data, visibility_grid)


def run_all():
    ns = ref_functions()
    store = {}
    for name, c in cases():
        with np.errstate(all="ignore"):
            out = reference_viewshed(ns, c["z"], c["xs"], c["ys"], c["x"], c["y"], c["observer_elev"], c["target_elev"])
        assert out.dtype == np.float64 and out.shape == c["z"].shape, name
        store[f"{name}/z"], store[f"{name}/xs"], store[f"{name}/ys"] = c["z"], np.asarray(c["xs"]), np.asarray(c["ys"])
        store[f"{name}/args"] = np.array([c["x"], c["y"], c["observer_elev"], c["target_elev"]], np.float64)
        store[f"{name}/out"] = out
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def names(store):
    return sorted({k.split("/")[0] for k in store})


def call_args(store, name):
    """(z, xs, ys, x, y, observer_elev, target_elev) of a stored case"""
    x, y, obs, tgt = (float(v) for v in store[f"{name}/args"])
    return store[f"{name}/z"], store[f"{name}/xs"], store[f"{name}/ys"], x, y, obs, tgt


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
        print("viewshed_exec.npz reproduces" if ok else "viewshed_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")

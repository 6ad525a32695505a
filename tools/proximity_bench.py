"""Time proximity / allocation / direction (float32 DeviceArray in, the result stays in HBM).

Shapes of the reference's own benchmark (benchmarks/benchmarks/proximity.py): nx = 100 and 1000 with ny = nx // 2, the raster
rng.integers(-nx, nx) as float32 over longitudes -180 .. 180 and latitudes -90 .. 90, the first 1, 10 and 100 of its unique
values as target_values, all three metrics.  Beside them one large raster, 8192 x 8192 with unit cells, EUCLIDEAN, at 1 % and
at 0.001 % target density: the sparse one shows what the list of non-empty rows buys (most rows are never visited).

For each it prints, in ms (median of --reps after --warmup):
  the row scan (left / right nearest target columns, row flags, the list of non-empty rows) between two events;
  the search for `proximity` on that scan, and for all three products at once, between two events;
  the whole API call of `proximity` (coordinate checks and upload on the host, workspace, the launches, a stream sync).
Next to them the number of targets and of non-empty rows.  No threshold is applied to any of it.

    python tools/proximity_bench.py [--reps 5] [--warmup 1] [--large 8192] [--log profiles/proximity/proximity_bench.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402
from tools.terrain_bench import call_ms, kernel_ms  # noqa: E402

px = importlib.import_module("xrspatial_amd.proximity")          # (the package's attribute of that name is the function)

SCAN_ONLY, SEARCH_ONLY, ALL = px.SCAN_ONLY, px.SEARCH_ONLY, px.ALL_THREE
METRICS = ("EUCLIDEAN", "GREAT_CIRCLE", "MANHATTAN")


def asv_raster(nx):
    """`get_xr_dataarray((nx // 2, nx), 'numpy', is_int=True)` of the reference's benchmarks"""
    ny = nx // 2
    z = np.random.default_rng(71942).integers(-nx, nx, size=(ny, nx)).astype(np.float32)
    return z, np.linspace(-180, 180, nx), np.linspace(-90, 90, ny)


def measure(z, xc, yc, target_values, metric, reps, warmup):
    rows, cols = z.shape
    dev = xs.DeviceArray.from_numpy(z)
    agg = xs.DataArray(dev, dims=["y", "x"], coords={"y": yc, "x": xc})
    code = px.DISTANCE_METRICS[metric]
    values, kind = px.target_array(target_values, z.dtype)
    lat = np.radians(yc)
    aux = xs.DeviceArray.from_numpy(np.concatenate([xc, yc, np.radians(xc), lat, np.cos(lat), values.view(np.float64)]).astype(np.float64))
    gc, vals = aux.ptr + 8 * (cols + rows), (aux.ptr + 8 * (2 * cols + 3 * rows) if values.size else None)
    work = xs.DeviceArray((int(_lib.load().xrs_proximity_workspace_bytes(rows, cols)),), np.uint8)
    out = xs.DeviceArray((3, rows, cols), np.float32)

    def launch(mode):
        return lambda: _lib.call("xrs_proximity", dev.ptr, 9, rows, cols, aux.ptr, aux.ptr + 8 * cols, gc, vals, kind, int(values.size),
                                 float("inf"), code, mode, work.ptr, out.ptr, None)

    scan = kernel_ms(launch(SCAN_ONLY), reps, warmup)
    search = kernel_ms(launch(SEARCH_ONLY), reps, warmup)
    search_all = kernel_ms(launch(SEARCH_ONLY | ALL), reps, warmup)
    api = call_ms(lambda: xs.proximity(agg, target_values=target_values, distance_metric=metric), reps, warmup)
    mask = np.isin(z, target_values) if len(target_values) else (z != 0)
    return {"rows": rows, "cols": cols, "metric": metric, "n_target_values": len(target_values), "targets": int(mask.sum()),
            "nonempty_rows": int(mask.any(axis=1).sum()), "scan_ms": scan, "search_proximity_ms": search, "search_all_three_ms": search_all,
            "api_call_ms": api}


def show(r):
    print(f"{r['rows']:6d} x {r['cols']:<6d} {r['metric']:<12s} {r['n_target_values']:4d} values {r['targets']:9d} targets in "
          f"{r['nonempty_rows']:5d} rows   scan {r['scan_ms']:9.3f} ms   search {r['search_proximity_ms']:9.3f} ms   "
          f"all three {r['search_all_three_ms']:9.3f} ms   API call {r['api_call_ms']:9.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--large", type=int, default=8192)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "proximity", "proximity_bench.json"))
    a = ap.parse_args()
    _lib.require_device()
    rows = []
    for nx in (100, 1000):
        z, xc, yc = asv_raster(nx)
        unique = np.unique(z)
        for n_values in (1, 10, 100):
            for metric in METRICS:
                rows.append(measure(z, xc, yc, unique[:n_values].tolist(), metric, a.reps, a.warmup))
                show(rows[-1])
    if a.large:
        n = a.large
        coords = np.arange(n, dtype=np.float64)
        for density in (1e-2, 1e-5):
            z = (np.random.default_rng(5).random((n, n)) < density).astype(np.float32)
            rows.append(dict(measure(z, coords, coords[::-1].copy(), [], "EUCLIDEAN", a.reps, a.warmup), density=density))
            show(rows[-1])
    res = {"dtype": "float32", "build_id": _lib.build_id(), "reps": a.reps, "rows": rows}
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Time rasterize with a DeviceArray-backed `like` (the result stays in HBM; the polygons go up from the host every call).

Inputs: the polygons `polygonize` returns (flat form) for three rasters of tools/polygonize_bench.py -- the classified DEM, the
land cover and the serpentine -- at every --n (default 8192 and 16384), one rectangle covering the whole raster, and 1000 random
overlapping triangles.  Prints per input: ms per `rasterize` call (median of --reps after --warmup), the crossing, span and
work-item counts, the four ABI calls timed one by one with the polygons already resident (census, spans, burn, gather; each
followed by a device sync, so each figure holds one sync), beside them in the same process `polygonize` on the source raster
and a plain device fill of the 4 B/cell plane (`xrs_memset`), the floor of a burn that touches every cell.  Per-kernel times
come from a separate run:
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/rasterize_bench.py --n 8192 --reps 3 --warmup 1 --no-polygonize`.

    python tools/rasterize_bench.py [--n 8192 16384] [--reps 10] [--warmup 3] [--only NAME] [--no-polygonize] [--json out.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import xrspatial_amd as xs  # noqa: E402
from tools.polygonize_bench import raster  # noqa: E402
from tools.regions_bench import timed  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402
from xrspatial_amd.experimental.polygonize import flat  # noqa: E402

rz = importlib.import_module("xrspatial_amd.rasterize")
SOURCES = ("classified_dem_f32_n8", "landcover_u8_n4", "serpentine_f32_n4")
NAMES = SOURCES + ("one_rectangle", "triangles_1000")


def stages(shapes, n, column, reps, warmup):
    """ms of the four ABI calls, one by one, the polygons resident"""
    points, ring_off, poly_off = shapes
    n_points, n_rings, n_polys = len(points), len(ring_off) - 1, len(poly_off) - 1
    values, priority, order, dtype = rz.plan_merge("last", column, n_polys, None)
    dev = [xs.DeviceArray.from_numpy(v) for v in (points, ring_off, poly_off, priority, order, values)]
    work = xs.DeviceArray((_lib.workspace_bytes("rasterize", n_points),), np.uint8)
    args = (dev[0].ptr, dev[1].ptr, dev[2].ptr, n_points, n_rings, n_polys, n, n, None)
    c, flags, ns, ni = ctypes.c_uint64(0), ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    out = {}
    out["census_ms"], _ = timed(lambda: _lib.call("xrs_rasterize_census", *args, work.ptr, ctypes.byref(c), ctypes.byref(flags), None),
                                reps, warmup)
    spans = xs.DeviceArray((_lib.workspace_bytes("rasterize_spans", c.value),), np.uint8)
    out["spans_ms"], _ = timed(lambda: _lib.call("xrs_rasterize_spans", *args, work.ptr, spans.ptr, c.value, ctypes.byref(ns),
                                                 ctypes.byref(ni), None), reps, warmup)
    plane = xs.DeviceArray((n, n), np.uint32)
    out["burn_ms"], _ = timed(lambda: _lib.call("xrs_rasterize_burn", n, n, spans.ptr, c.value, n_polys, ni.value, dev[3].ptr, 0,
                                                plane.ptr, None), reps, warmup)
    result = xs.DeviceArray((n, n), dtype)
    fill = np.zeros(1, dtype)
    out["gather_ms"], _ = timed(lambda: _lib.call("xrs_rasterize_gather", plane.ptr, n, n, dev[5].ptr, dev[4].ptr,
                                                  xs.device.DTYPE_CODE[dtype], fill.ctypes.data, 0, result.ptr, None), reps, warmup)
    covered = int(np.count_nonzero(plane.get())) if n <= 8192 else None
    out["fill_ms"], _ = timed(lambda: _lib.call("xrs_memset", plane.ptr, 0, n * n * 4, None), reps, warmup)
    return {k: round(v, 3) for k, v in out.items()}, dict(crossings=c.value, spans=ns.value, items=ni.value, covered_cells=covered)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8192, 16384])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-polygonize", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.require_device()
    rows = []
    for n in a.n:
        for name in NAMES:
            if a.only and a.only not in name:
                continue
            row = {"input": name, "shape": [n, n]}
            if name in SOURCES:
                host, conn = raster(name, n)
                dev = xs.DeviceArray.from_numpy(host)
                agg = xs.DataArray(dev, dims=["y", "x"])
                column, points, ring_off, poly_off = flat(dev, None, conn == 8, None)
                if not a.no_polygonize:
                    pmed, _ = timed(lambda: xs.polygonize(agg, connectivity=conn, return_type="flat"), a.reps, a.warmup)
                    row["polygonize_ms_median"] = round(pmed, 3)
                shapes = (points, ring_off, poly_off)
                like = xs.DataArray(xs.DeviceArray((n, n), np.uint8), dims=["y", "x"])
                back = xs.rasterize(shapes, like, column)
                if n <= 8192:                                   # the round trip, checked where a host copy is cheap
                    row["round_trip_equal"] = bool(np.array_equal(back.data.get(), host))
                del dev, agg, back
            else:
                rng = np.random.default_rng(n)
                if name == "one_rectangle":
                    polys = [[np.array([[-1.0, -1.0], [n + 1.0, -1.0], [n + 1.0, n + 1.0], [-1.0, n + 1.0]])]]
                else:
                    polys = [[rng.uniform(0, n, 2) + rng.uniform(-0.1 * n, 0.1 * n, (3, 2))] for _ in range(1000)]
                shapes = rz.flatten(polys)
                column = None
                like = xs.DataArray(xs.DeviceArray((n, n), np.uint8), dims=["y", "x"])
            row.update(points=len(shapes[0]), rings=len(shapes[1]) - 1, polygons=len(shapes[2]) - 1)
            med, best = timed(lambda: xs.rasterize(shapes, like, column), a.reps, a.warmup)
            row.update(ms_median=round(med, 3), ms_min=round(best, 3))
            ms, counts = stages(shapes, n, column, a.reps, a.warmup)
            row.update(counts)
            row.update(ms)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del like, shapes, column
            xs.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"build_id": _lib.build_id(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

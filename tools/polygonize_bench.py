"""Time polygonize on DeviceArrays (HBM-resident in, `return_type="flat"`: four NumPy arrays out).

Rasters: those of tools/regions_bench.py -- a classified synthetic DEM (float32, 8-connectivity), categorical uint8 "land
cover" (240 rectangular patches, 4-connectivity), a serpentine that threads every tile (float32, 4-connectivity) and every
cell distinct (float64, 4-connectivity) -- at --n (default 16384), except that "distinct" runs at --distinct-n (default
4096): with 4 boundary states per cell its 16384^2 version has 2^30 states and 1.3 * 2^30 points, 21 GB of float64 that the
call would copy to the host.  Prints per raster: ms per call (median of --reps after --warmup, the whole call: census, rings,
scatter, the four device-to-host copies), regions, boundary states E, rings, points, the pointer-doubling rounds of the leader
and rank stages, and `zonal.regions`' ms on the same raster (csrc/regions.hip's device code is the parent commit's, byte for
byte).  Per-kernel times come from separate runs, one per raster:
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/polygonize_bench.py --reps 3 --warmup 1 --no-regions --only NAME`.

    python tools/polygonize_bench.py [--n 16384] [--distinct-n 4096] [--reps 10] [--warmup 3] [--only NAME] [--no-regions] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import xrspatial_amd as xs  # noqa: E402
from tools.regions_bench import timed  # noqa: E402
from xrspatial_amd.experimental.polygonize import flat  # noqa: E402


def raster(name, n):
    """one raster of tools/regions_bench.py: rasters(), built on its own"""
    if name == "classified_dem_f32_n8":
        y = np.arange(n, dtype=np.float32)[:, None]
        x = np.arange(n, dtype=np.float32)[None, :]
        dem = 1500 + 700 * np.sin(x / 1100.0) * np.cos(y / 1700.0) + 120 * np.sin((x + 2 * y) / 233.0)
        return np.floor(dem / 150.0).astype(np.float32), 8                 # 10 elevation classes
    if name == "landcover_u8_n4":
        by, bx = np.minimum(np.arange(n) * 15 // n, 14), np.minimum(np.arange(n) * 16 // n, 15)
        return ((by[:, None] * 7 + bx[None, :] * 3) % 11).astype(np.uint8), 4    # 15 x 16 rectangular patches
    if name == "serpentine_f32_n4":
        serp = np.zeros((n, n), np.float32)
        serp[0::2, :] = 1
        serp[1::4, -1] = 1
        serp[3::4, 0] = 1
        return serp, 4
    i = np.arange(n * n, dtype=np.float64).reshape(n, n)                         # distinct_f64_n4
    return np.where((np.arange(n)[:, None] + np.arange(n)[None, :]) % 2 == 0, i, -i), 4


NAMES = ("classified_dem_f32_n8", "landcover_u8_n4", "serpentine_f32_n4", "distinct_f64_n4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--distinct-n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-regions", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from xrspatial_amd import _lib
    _lib.require_device()
    rows = []
    for name in NAMES:
        if a.only and a.only not in name:
            continue
        host, n = raster(name, a.distinct_n if name.startswith("distinct") else a.n)
        dev = xs.DeviceArray.from_numpy(host)
        agg = xs.DataArray(dev, dims=["y", "x"])
        stats = {}
        flat(dev, None, n == 8, None, stats=stats)
        med, best = timed(lambda: xs.polygonize(agg, connectivity=n, return_type="flat"), a.reps, a.warmup)
        row = {"raster": name, "shape": list(host.shape), "dtype": host.dtype.name, "connectivity": n,
               "ms_median": round(med, 3), "ms_min": round(best, 3), **stats}
        if not a.no_regions:
            rmed, _ = timed(lambda: xs.regions(agg, neighborhood=n), a.reps, a.warmup)
            row["zonal_regions_ms_median"] = round(rmed, 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del dev, agg
        xs.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump({"build_id": _lib.build_id(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

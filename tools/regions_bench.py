"""Time zonal.regions on 16384 x 16384 DeviceArrays (HBM-resident in and out).

Rasters: a classified synthetic DEM (float32, 8-connectivity), categorical uint8 "land cover" (240 rectangular patches,
4-connectivity), a serpentine that threads every tile (float32, 4-connectivity: the union-find worst case) and every cell
distinct (float64, 4-connectivity).  Prints ms per call (median of --reps after --warmup, the whole call: link + count +
host check + merge + label) and the fraction of 8 TB/s at algorithmic bytes: the raster read twice and written once,
parent[] written once and read once -- 3 * itemsize + 8 B/cell.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/regions_bench.py --reps 3` run.

If scipy imports, `--scipy` also times scipy.ndimage.label on the host copy of the uint8 raster: a CPU yardstick for plain
connected-component labelling, not the reference (whose serial two-pass scan does not finish at this size).

    python tools/regions_bench.py [--n 16384] [--reps 10] [--warmup 3] [--only NAME] [--scipy] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import xrspatial_amd as xs  # noqa: E402

PEAK = 8e12


def rasters(n):
    y = np.arange(n, dtype=np.float32)[:, None]
    x = np.arange(n, dtype=np.float32)[None, :]
    dem = 1500 + 700 * np.sin(x / 1100.0) * np.cos(y / 1700.0) + 120 * np.sin((x + 2 * y) / 233.0)
    classified = np.floor(dem / 150.0).astype(np.float32)                     # 10 elevation classes
    del dem
    by, bx = np.minimum(np.arange(n) * 15 // n, 14), np.minimum(np.arange(n) * 16 // n, 15)
    cover = ((by[:, None] * 7 + bx[None, :] * 3) % 11).astype(np.uint8)       # 15 x 16 rectangular patches
    serp = np.zeros((n, n), np.float32)
    serp[0::2, :] = 1
    serp[1::4, -1] = 1
    serp[3::4, 0] = 1
    i = np.arange(n * n, dtype=np.float64).reshape(n, n)
    distinct = np.where((np.arange(n)[:, None] + np.arange(n)[None, :]) % 2 == 0, i, -i)
    return [("classified_dem_f32_n8", classified, 8), ("landcover_u8_n4", cover, 4), ("serpentine_f32_n4", serp, 4),
            ("distinct_f64_n4", distinct, 4)]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    xs.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        xs.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from xrspatial_amd import _lib
    _lib.require_device()
    rows = []
    for name, host, n in rasters(a.n):
        if a.only and a.only not in name:
            continue
        dev = xs.DeviceArray.from_numpy(host)
        agg = xs.DataArray(dev, dims=["y", "x"])
        out = xs.regions(agg, neighborhood=n)
        top = int(out.data.get().max())
        del out
        med, best = timed(lambda: xs.regions(agg, neighborhood=n), a.reps, a.warmup)
        cells = host.size
        bytes_ = cells * (3 * host.dtype.itemsize + 8)
        row = {"raster": name, "shape": list(host.shape), "dtype": host.dtype.name, "neighborhood": n,
               "largest_label": top, "ms_median": round(med, 3), "ms_min": round(best, 3),
               "algorithmic_bytes_per_cell": 3 * host.dtype.itemsize + 8,
               "fraction_of_8TBps": round(bytes_ / (med * 1e-3) / PEAK, 3)}
        if a.scipy and host.dtype == np.uint8:
            try:
                from scipy import ndimage
                t0 = time.perf_counter()
                for v in np.unique(host):
                    ndimage.label(host == v)
                row["scipy_ndimage_label_cpu_ms (yardstick, not the reference)"] = round((time.perf_counter() - t0) * 1e3, 1)
            except ImportError:
                pass
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

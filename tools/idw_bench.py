"""Time idw's two ABI calls with everything resident in HBM: `xrs_idw_bin` (transform, flag, counting sort; the figure holds
the call's one wait for the stream) and `xrs_idw_search` (followed by a device sync), one after the other, and beside them in
the same run a plain device fill of the output plane (`xrs_memset`), the floor of anything that writes every cell once.

Inputs: a --n x --n float64 result (default 8192 and 4096) from 10^4, 10^6 and 10^7 uniformly random points and one clustered
set (10^6 points, all in 1 % of the area), at k = 1, 12 and 64, at the planned bin size; with --sweep also the bin sizes a
factor 4 either side of the plan: the sweep against which `plan_bins`' target of 2 - 4 points per bin, set by reasoning before
any measurement, is to be read (DESIGN.md §6t quotes it).  Prints one JSON row per
(input, k, bin size): ms per call (median of --reps after --warmup), ns per cell of the search and its ratio to the fill.
Writes <out>/idw_bench.json after every row and <out>/idw_bench.log (the same rows as text).

    python tools/idw_bench.py [--n 8192 4096] [--k 1 12 64] [--sets u1e4 u1e6 u1e7 clustered] [--sweep] [--reps 5] [--warmup 1]
                              [--out profiles/idw]
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
from tools.regions_bench import timed  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402

idw = importlib.import_module("xrspatial_amd.idw")
SETS = {"u1e4": 10**4, "u1e6": 10**6, "u1e7": 10**7, "clustered": 10**6}


def points_of(name, n):
    rng = np.random.default_rng(len(name) + n)
    count = SETS[name]
    if name == "clustered":                                      # all points in a square of 1 % of the area
        side = 0.1 * n
        x0, y0 = 0.6 * n, 0.3 * n
        return np.stack([rng.uniform(x0, x0 + side, count), rng.uniform(y0, y0 + side, count)], axis=1)
    return np.stack([rng.uniform(0, n, count), rng.uniform(0, n, count)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8192, 4096])
    ap.add_argument("--k", type=int, nargs="+", default=[1, 12, 64])
    ap.add_argument("--sets", nargs="+", default=list(SETS), choices=list(SETS))
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "idw"))
    a = ap.parse_args()
    _lib.require_device()
    os.makedirs(a.out, exist_ok=True)
    rows = []
    log = open(os.path.join(a.out, "idw_bench.log"), "w")
    for n in a.n:
        out = xs.DeviceArray((n, n), np.float64)
        fill_ms, _ = timed(lambda: _lib.call("xrs_memset", out.ptr, 0, n * n * 8, None), a.reps, a.warmup)
        for name in a.sets:
            host = points_of(name, n)
            count = len(host)
            pts = xs.DeviceArray.from_numpy(host)
            vals = xs.DeviceArray.from_numpy(np.random.default_rng(1).normal(100.0, 30.0, count))
            plan = idw.plan_bins(count, n, n)
            sizes = [plan] if not a.sweep else sorted({max(plan // 4, 1), max(plan // 2, 1), plan, plan * 2, plan * 4})
            for b in sizes:
                if idw.n_bins(n, n, b) > idw.MAX_BINS:
                    continue
                work = xs.DeviceArray((_lib.workspace_bytes("idw", count, n, n, b),), np.uint8)
                flags = ctypes.c_int(0)
                bin_ms, _ = timed(lambda: _lib.call("xrs_idw_bin", pts.ptr, count, n, n, b, None, work.ptr, ctypes.byref(flags), None),
                                  a.reps, a.warmup)
                for k in a.k:
                    ms, best = timed(lambda: _lib.call("xrs_idw_search", work.ptr, vals.ptr, count, n, n, b, k, 2, -1.0, 1, float("nan"),
                                                       8, out.ptr, None, None, None), a.reps, a.warmup)
                    row = {"shape": [n, n], "input": name, "points": count, "k": k, "bin_cells": b, "planned": b == plan,
                           "points_per_bin": round(count * b * b / (n * n), 2), "bin_ms": round(bin_ms, 3),
                           "search_ms": round(ms, 3), "search_ms_min": round(best, 3), "fill_ms": round(fill_ms, 3),
                           "search_ns_per_cell": round(ms * 1e6 / (n * n), 3), "search_over_fill": round(ms / fill_ms, 1)}
                    print(json.dumps(row), flush=True)
                    log.write(json.dumps(row) + "\n")
                    log.flush()
                    rows.append(row)
                    with open(os.path.join(a.out, "idw_bench.json"), "w") as fh:
                        json.dump({"build_id": _lib.build_id(), "rows": rows}, fh, indent=1)
                del work
            del pts, vals
            xs.empty_cache()
        del out
        xs.empty_cache()


if __name__ == "__main__":
    main()

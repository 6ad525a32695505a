"""Time every classifier on a 16384 x 16384 float32 DeviceArray (HBM-resident in and out).

Prints ms per call (median of --reps after --warmup) and, for the kernels, the fraction of 8 TB/s at algorithmic bytes:
the bin pass moves 8 B/cell (4 read, 4 written), a radix-select digit pass and the finite-count pass 4 B/cell.

    python tools/classify_bench.py [--n 16384] [--reps 10] [--warmup 3] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402
from xrspatial_amd.classify import BIN_COUNT, _Stats  # noqa: E402

PEAK = 8e12


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
    return float(np.median(ts))


def kernel_ms(launch, reps, warmup):
    """Device time of `launch()` between two events on the null stream."""
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        _lib.call("xrs_event_create", ctypes.byref(e))
    for _ in range(warmup):
        launch()
    ts = []
    for _ in range(reps):
        _lib.call("xrs_event_record", ev[0], None)
        launch()
        _lib.call("xrs_event_record", ev[1], None)
        _lib.call("xrs_event_sync", ev[1])
        ms = ctypes.c_float()
        _lib.call("xrs_event_elapsed_ms", ev[0], ev[1], ctypes.byref(ms))
        ts.append(ms.value)
    for e in ev:
        _lib.call("xrs_event_destroy", e)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json")
    args = ap.parse_args()
    _lib.require_device()
    n = args.n
    rng = np.random.default_rng(0)
    host = rng.gamma(2.0, 50.0, (n, n)).astype(np.float32)
    host[rng.random((n, n)) < 1e-4] = np.nan
    dev = xs.DeviceArray.from_numpy(host)
    del host
    agg = xs.DataArray(dev, dims=["y", "x"])
    cells = n * n
    rows = []

    # kernels alone
    bins = xs.DeviceArray.from_numpy(np.array([20.0, 60.0, 100.0, 150.0, 1e30]))
    nv = xs.DeviceArray.from_numpy(np.arange(5, dtype=np.float64))
    out = xs.DeviceArray((n, n), np.float32)
    ms = kernel_ms(lambda: _lib.call("xrs_classify_bin_f32", dev.ptr, out.ptr, cells, bins.ptr, nv.ptr, 5, BIN_COUNT, None),
                   args.reps, args.warmup)
    rows.append({"what": "kernel: bin (5 sorted bins)", "ms": ms, "frac_peak": 8 * cells / (ms * 1e-3) / PEAK})
    st = _Stats(dev)
    ms = kernel_ms(lambda: _lib.call("xrs_classify_finite_stats_f32", dev.ptr, cells, st.work.ptr, st.out.ptr, None),
                   args.reps, args.warmup)
    rows.append({"what": "kernel: finite count/min/max/sum", "ms": ms, "frac_peak": 4 * cells / (ms * 1e-3) / PEAK})
    cnt = st.count
    ranks = xs.DeviceArray.from_numpy(np.array([cnt // 4, cnt // 4 + 1, cnt // 2, cnt // 2 + 1, 3 * cnt // 4, cnt - 1],
                                               dtype=np.int64))
    vals = xs.DeviceArray((6,), np.float64)
    ms = kernel_ms(lambda: _lib.call("xrs_classify_select_f32", dev.ptr, cells, ranks.ptr, 6, st.work.ptr, st.work.nbytes,
                                     vals.ptr, None), args.reps, args.warmup)
    rows.append({"what": "kernel: radix select, 6 ranks (3 digit passes)", "ms": ms,
                 "frac_peak": 3 * 4 * cells / (ms * 1e-3) / PEAK})

    # public calls, DeviceArray in / out
    calls = [("binary", lambda: xs.classify.binary(agg, [100.0, 101.0])),
             ("reclassify", lambda: xs.classify.reclassify(agg, [20, 60, 100, 150, np.inf], [1, 2, 3, 4, 5])),
             ("equal_interval", lambda: xs.classify.equal_interval(agg)),
             ("quantile", lambda: xs.classify.quantile(agg)),
             ("percentiles", lambda: xs.classify.percentiles(agg)),
             ("box_plot", lambda: xs.classify.box_plot(agg)),
             ("std_mean", lambda: xs.classify.std_mean(agg)),
             ("head_tail_breaks", lambda: xs.classify.head_tail_breaks(agg)),
             ("maximum_breaks", lambda: xs.classify.maximum_breaks(agg))]
    for name, fn in calls:
        rows.append({"what": f"call: {name}", "ms": timed(fn, args.reps, args.warmup)})
    for r in rows:
        frac = f"  {r['frac_peak']:.2f} of 8 TB/s" if "frac_peak" in r else ""
        print(f"{r['what']:<48s} {r['ms']:9.3f} ms{frac}")
    res = {"n": n, "cells": cells, "build_id": _lib.build_id(), "rows": rows}
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

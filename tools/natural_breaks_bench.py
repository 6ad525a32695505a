"""Time natural_breaks: the default call on generate_terrain output, stage by stage, and the dynamic programme alone.

Workload 1, per --sizes n (an n x n float32 DeviceArray from generate_terrain, the result stays in HBM), num_sample = 20 000, k = 5:
  index shuffle   the reference's seeded shuffle of n * n uint32 indices, NumPy on the host (cache emptied first); O(num_data)
                  by the reference's definition, and skipped by a second call on a raster of the same size
  gather          xrs_gather_elems of the 20 000 sample cells (device events)
  host sort       the finite filter, np.unique, the sort and the float32 cast of the sample, NumPy
  DP              xrs_jenks_matrices_f32 on that sample: the whole call, and column j as the difference of the calls with j and
                  j - 1 classes (the call with j classes runs the initial tables and columns 1 .. j)
  bin pass        classify's bin kernel over the raster with the resulting bins
  call            the whole public call, wall clock with a device sync: first with the index cache emptied, then with it warm
Workload 2: the DP alone on a sorted float32 normal sample of --dp-n values for every k of --dp-k, with its rate in steps per
second, a step being one (row, m) pair of one column: k * n * (n + 1) / 2 per call.

Medians of --reps after --warmup.  No threshold is applied to any of it.  Writes --out (JSON) and the printed lines next to it
(.log).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib, classify, jenks  # noqa: E402
from tools.terrain_bench import call_ms, kernel_ms  # noqa: E402

CELL = 30.0
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def dp_ms(sample_d, n, k, reps, warmup):
    lib = _lib.load()
    limits = xs.DeviceArray((n + 1, k + 1), np.float32)
    var = xs.DeviceArray((n + 1, k + 1), np.float32)
    work = xs.DeviceArray((int(lib.xrs_jenks_workspace_bytes(n, k)),), np.uint8)
    return kernel_ms(lambda: _lib.call("xrs_jenks_matrices_f32", sample_d.ptr, n, k, limits.ptr, var.ptr, work.ptr, work.nbytes, None),
                     reps, warmup)


def dp_columns(sorted_f32, k, reps, warmup):
    """(ms of the call with k classes, [ms of column 1 .. k as differences of the calls with j and j - 1 classes])"""
    n = sorted_f32.size
    sample_d = xs.DeviceArray.from_numpy(sorted_f32)
    totals = [dp_ms(sample_d, n, j, reps, warmup) for j in range(1, k + 1)]
    return totals[-1], [totals[0]] + [totals[j] - totals[j - 1] for j in range(1, k)]


def default_call(n, num_sample, k, reps, warmup):
    agg = xs.DataArray(xs.DeviceArray((n, n), np.float32), dims=["y", "x"])
    dem = xs.generate_terrain(agg, x_range=(0, CELL * n), y_range=(0, CELL * n))
    dev = dem.data
    row = {"n": n, "cells": n * n, "num_sample": num_sample, "k": k}

    def shuffle():
        del jenks._index_cache[:]
        return jenks.sample_indices(n * n, num_sample)
    row["index_shuffle_host_ms"] = host_ms(shuffle, max(1, min(reps, 3)))
    idx = jenks.sample_indices(n * n, num_sample)
    idx_d = xs.DeviceArray.from_numpy(idx)
    out = xs.DeviceArray((idx.size,), np.float32)
    row["gather_ms"] = kernel_ms(lambda: _lib.call("xrs_gather_elems", dev.ptr, 4, n * n, idx_d.ptr, idx.size, out.ptr, None), reps, warmup)
    sample = out.get()

    def prepare():
        fin = sample[np.isfinite(sample)]
        np.unique(fin)
        fin.sort()
        return fin.astype(np.float32)
    row["host_sort_ms"] = host_ms(prepare, reps)
    sorted_f32 = prepare()
    row["dp_ms"], row["dp_column_ms"] = dp_columns(sorted_f32, k, reps, warmup)
    row["dp_steps_per_s"] = k * sorted_f32.size * (sorted_f32.size + 1) / 2 / (row["dp_ms"] * 1e-3)
    st = classify._Stats(dev)
    bins, uvk = jenks.natural_break_bins(sample, k, st.moments()[2])
    row["bins"] = [float(b) for b in bins]
    row["bin_pass_ms"] = call_ms(lambda: classify._bin_device(dev, bins, np.arange(uvk)), reps, warmup)
    row["call_cold_ms"] = call_ms(lambda: xs.natural_breaks(dem, num_sample=num_sample, k=k), max(1, min(reps, 3)), 0,
                                  before=lambda: jenks._index_cache.clear())
    row["call_warm_ms"] = call_ms(lambda: xs.natural_breaks(dem, num_sample=num_sample, k=k), reps, 1)
    say(f"{n} x {n}, num_sample {num_sample}, k {k}: shuffle (host) {row['index_shuffle_host_ms']:9.1f} ms  gather {row['gather_ms']:7.3f}  "
        f"host sort {row['host_sort_ms']:7.3f}  DP {row['dp_ms']:9.3f} (columns {' '.join('%.3f' % c for c in row['dp_column_ms'])}; "
        f"{row['dp_steps_per_s']:.3e} steps/s)  bin pass {row['bin_pass_ms']:8.3f}  |  call, cache empty {row['call_cold_ms']:9.1f}  "
        f"cache warm {row['call_warm_ms']:9.1f}")
    return row


def dp_alone(n, k, reps, warmup):
    sample = np.sort(np.random.default_rng(1).normal(1000.0, 250.0, n).astype(np.float32))
    total, columns = dp_columns(sample, k, reps, warmup)
    row = {"n": n, "k": k, "dp_ms": total, "dp_column_ms": columns, "dp_steps_per_s": k * n * (n + 1) / 2 / (total * 1e-3)}
    say(f"DP alone n {n} k {k}: {total:9.3f} ms (columns {' '.join('%.3f' % c for c in columns)}); {row['dp_steps_per_s']:.3e} steps/s")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 16384])
    ap.add_argument("--num-sample", type=int, default=20000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--dp-n", type=int, default=20000)
    ap.add_argument("--dp-k", type=int, nargs="*", default=[5, 10])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "natural_breaks", "natural_breaks_bench.json"))
    a = ap.parse_args()
    _lib.require_device()
    result = {"build_id": _lib.build_id(), "reps": a.reps, "warmup": a.warmup, "dp_alone": [], "default_call": []}
    say(f"build {result['build_id']}, medians of {a.reps} after {a.warmup}")
    for k in a.dp_k:
        result["dp_alone"].append(dp_alone(a.dp_n, k, a.reps, a.warmup))
    for n in a.sizes:
        result["default_call"].append(default_call(n, a.num_sample, a.k, a.reps, a.warmup))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        with open(os.path.splitext(a.out)[0] + ".log", "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

"""Time `contours` on `generate_terrain` rasters resident in HBM (default 4096^2 and 8192^2, float32) at `levels=10` and `levels=100`.

Per --sizes n and per level count:
  stages      the three ABI calls one by one, wall clock with a device sync behind each (census and lines wait for the stream
              themselves), and the census once more between two events: segments, lines, points and the doubling rounds beside them
  call        `contours(agg, levels, return_type="flat")`, wall clock: the three calls, the workspaces, and the download of the
              points and offsets to the host
  yardsticks  in the same run: xrs_copy_f32 between two events (4 B read + 4 B written per cell), and `polygonize` (flat) on the
              10-class `equal_interval` of the same raster, wall clock
and the two ratios that say whether the raster is read once for all levels: census / copy, and the 100-level census and call over
the 10-level ones.  Medians of --reps after --warmup.  No threshold is applied to any of it.  Writes --out (JSON) and the printed
lines next to it (.log).
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402
from xrspatial_amd.device import DTYPE_CODE  # noqa: E402
from hydrology_bench import LINES, kernel_ms, say, wall_ms  # noqa: E402

ct = importlib.import_module("xrspatial_amd.contours")                  # (the package's attribute of that name is the function)
LEVEL_COUNTS = (10, 100)


def stages(z, levels, reps, warmup):
    """ms of the three ABI calls and the counts they report"""
    n = z.shape[0]
    code, K = DTYPE_CODE[np.dtype(z.dtype)], len(levels)
    work = xs.DeviceArray((_lib.workspace_bytes("contours", n, n, K),), np.uint8)
    ns, nl, npts = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rounds = (ctypes.c_int * 2)()

    def census():
        _lib.call("xrs_contours_census", z.ptr, code, n, n, levels.ctypes.data, K, work.ptr, ctypes.byref(ns), None)

    out = {"census_ms": wall_ms(census, reps, warmup), "census_event_ms": kernel_ms(census, reps, warmup)}
    out["workspace_bytes"] = int(work.nbytes)
    out["segments"] = int(ns.value)
    lines = xs.DeviceArray((_lib.workspace_bytes("contours_lines", ns.value),), np.uint8)
    out["lines_workspace_bytes"] = int(lines.nbytes)

    def chain():
        _lib.call("xrs_contours_lines", z.ptr, code, n, n, K, work.ptr, lines.ptr, ns.value, ctypes.byref(nl), ctypes.byref(npts), rounds, None)

    out["lines_ms"] = wall_ms(chain, reps, warmup)
    out.update(lines=int(nl.value), points=int(npts.value), leader_rounds=int(rounds[0]), rank_rounds=int(rounds[1]))
    sort = xs.DeviceArray((_lib.workspace_bytes("contours_scatter", nl.value),), np.uint8)
    points = xs.DeviceArray((npts.value, 2), np.float64)
    line_off, level_off = xs.DeviceArray((nl.value + 1,), np.int64), xs.DeviceArray((K + 1,), np.int64)
    closed = xs.DeviceArray((nl.value,), np.uint8)

    def scatter():
        _lib.call("xrs_contours_scatter", z.ptr, code, n, n, K, work.ptr, lines.ptr, sort.ptr, ns.value, nl.value, None, points.ptr,
                  line_off.ptr, level_off.ptr, closed.ptr, None)

    out["scatter_ms"] = wall_ms(scatter, reps, warmup)
    out["closed_lines"] = int(closed.get().sum())
    out["longest_line_points"] = int(np.diff(line_off.get()).max())
    return out


def one_size(n, reps, warmup):
    cells = n * n
    row = {"n": n, "cells": cells}
    terrain = xs.generate_terrain(xs.DataArray(xs.DeviceArray((n, n), np.float32), dims=["y", "x"]))
    z = terrain.data
    other = xs.DeviceArray((n, n), np.float32)
    row["yardstick_copy_8B_ms"] = kernel_ms(lambda: _lib.call("xrs_copy_f32", z.ptr, other.ptr, cells, None), reps, warmup)
    del other
    classes = xs.equal_interval(terrain, k=10)
    row["yardstick_polygonize_10_classes_ms"] = wall_ms(lambda: xs.polygonize(classes, return_type="flat"), reps, warmup)
    del classes
    say(f"{n} x {n}: yardsticks  xrs_copy_f32 {row['yardstick_copy_8B_ms']:.3f} ms, polygonize of 10 equal_interval classes "
        f"{row['yardstick_polygonize_10_classes_ms']:.3f} ms")
    count, lo, hi = ct._finite_range(z)
    for K in LEVEL_COUNTS:
        levels = ct.interior_levels(lo, hi, K)
        info = stages(z, levels, reps, warmup)
        info["call_ms"] = wall_ms(lambda: xs.contours(terrain, K, return_type="flat"), max(1, reps // 2), 1)
        info["census_over_copy"] = info["census_event_ms"] / row["yardstick_copy_8B_ms"]
        row[f"levels_{K}"] = info
        say(f"{n} x {n}: levels={K}  census {info['census_ms']:.3f} ms ({info['census_event_ms']:.3f} ms between events, "
            f"{info['census_over_copy']:.2f} x the copy), lines {info['lines_ms']:.3f} ms in {info['leader_rounds']} + {info['rank_rounds']} "
            f"rounds, scatter {info['scatter_ms']:.3f} ms; call with download {info['call_ms']:.3f} ms; {info['segments']} segments, "
            f"{info['lines']} lines ({info['closed_lines']} closed, the longest {info['longest_line_points']} points), {info['points']} points")
        xs.empty_cache()
    a, b = row[f"levels_{LEVEL_COUNTS[0]}"], row[f"levels_{LEVEL_COUNTS[1]}"]
    row["census_100_over_10"] = b["census_event_ms"] / a["census_event_ms"]
    row["call_100_over_10"] = b["call_ms"] / a["call_ms"]
    row["segments_100_over_10"] = b["segments"] / max(a["segments"], 1)
    say(f"{n} x {n}: 100 levels over 10 levels  census {row['census_100_over_10']:.2f} x, call {row['call_100_over_10']:.2f} x, "
        f"segments {row['segments_100_over_10']:.2f} x")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours", "contours_bench.json"))
    a = ap.parse_args()
    _lib.require_device()
    result = {"build_id": _lib.build_id(), "reps": a.reps, "warmup": a.warmup, "sizes": []}
    say(f"build {result['build_id']}, medians of {a.reps} after {a.warmup}")
    for n in a.sizes:
        result["sizes"].append(one_size(n, a.reps, a.warmup))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        with open(os.path.splitext(a.out)[0] + ".log", "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

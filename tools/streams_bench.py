"""Time stream_order, stream_link, watershed and flow_length on the filled, flat-resolved `generate_terrain` raster, resident in
HBM (default 4096^2 and 8192^2), at the accumulation thresholds 100 and 1000.

Per --sizes n, in one process:
  yardsticks   taken in the same run: xrs_copy_f32 between two events (8 B/cell), and `flow_accumulation` and `basins` through the
               public functions on the same direction raster
  stream_order (both methods), stream_link    the public functions on DeviceArrays, wall clock with a device sync; and from the
               status words of one xrs_stream_network call: stream cells, sources, heads, Strahler levels, the rounds of every
               level, the cells of every J_k; with XRS_STREAM_TIMED the milliseconds of its five phases
  watershed    at the five cells of largest accumulation; flow_length: wall clock, rounds from the status words
Medians of --reps after --warmup.  Every step runs under --limit seconds: a watchdog thread ends the process when a step
takes longer.  No threshold is applied to any of it.  Writes --out (JSON) and the printed lines next to it (.log).
"""
import argparse
import ctypes
import faulthandler
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib, hydrology as hy  # noqa: E402

LINES = []
LIMIT = 120


def say(text):
    print(text, flush=True)
    LINES.append(text)


def step(fn):
    """fn() under the time limit."""
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    try:
        return fn()
    finally:
        faulthandler.cancel_dump_traceback_later()


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


def wall_ms(fn, reps, warmup):
    def run():
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
    return step(run)


def one_size(n, thresholds, reps, warmup):
    cells = n * n
    row = {"n": n, "cells": cells, "thresholds": []}
    terrain = step(lambda: xs.generate_terrain(xs.DataArray(xs.DeviceArray((n, n), np.float32), dims=["y", "x"])))
    fd = step(lambda: xs.flow_direction(xs.fill(terrain), resolve_flats=True))
    fa = step(lambda: xs.flow_accumulation(fd))
    other = xs.DeviceArray((n, n), np.float32)
    row["yardstick_copy_8B_ms"] = step(lambda: kernel_ms(lambda: _lib.call("xrs_copy_f32", fd.data.ptr, other.ptr, cells, None), reps, warmup))
    del other
    row["flow_accumulation_ms"] = wall_ms(lambda: xs.flow_accumulation(fd), reps, warmup)
    row["basins_ms"] = wall_ms(lambda: xs.basins(fd), reps, warmup)
    say(f"{n} x {n}: yardsticks  xrs_copy_f32 {row['yardstick_copy_8B_ms']:.3f} ms, flow_accumulation {row['flow_accumulation_ms']:.3f} ms, "
        f"basins {row['basins_ms']:.3f} ms (public functions on a DeviceArray)")
    for thr in thresholds:
        part = {"threshold": thr}
        part["stream_order_strahler_ms"] = wall_ms(lambda: xs.stream_order(fd, fa, thr), reps, warmup)
        part["stream_order_shreve_ms"] = wall_ms(lambda: xs.stream_order(fd, fa, thr, method='shreve'), reps, warmup)
        part["stream_link_ms"] = wall_ms(lambda: xs.stream_link(fd, fa, thr), reps, warmup)
        words = step(lambda: hy.stream_network(fd.data, fa.data, thr, hy.STRAHLER | hy.SHREVE | hy.LINK, flags=hy.TIMED)[-1])
        levels = words[hy.STREAM_LEVELS]
        part.update(stream_cells=words[hy.STREAM_CELLS], stream_share=words[hy.STREAM_CELLS] / cells, sources=words[hy.STREAM_SOURCES],
                    heads=words[hy.STREAM_HEADS], levels=levels, source_count_rounds=words[0], head_rounds=words[hy.STREAM_HEAD_ROUNDS],
                    joints=[words[hy.STREAM_JOINTS + k] for k in range(1, levels + 1)],
                    level_rounds=[words[hy.STREAM_LEVEL_ROUNDS + k] for k in range(1, levels + 1)],
                    timed_ms=dict(zip(("mark_scan_compact", "source_count", "strahler_levels", "heads", "finish"),
                                      (w / 1e6 for w in words[hy.STREAM_NS:hy.STREAM_NS + 5]))))
        row["thresholds"].append(part)
        say(f"{n} x {n} threshold {thr}: stream_order strahler {part['stream_order_strahler_ms']:.3f} ms, shreve "
            f"{part['stream_order_shreve_ms']:.3f} ms, stream_link {part['stream_link_ms']:.3f} ms")
        say(f"{n} x {n} threshold {thr}: {part['stream_cells']} stream cells ({100 * part['stream_share']:.3f} % of the raster), "
            f"{part['sources']} sources, {part['heads']} heads, {levels} levels; rounds: source count {words[0]}, heads "
            f"{part['head_rounds']}, levels {part['level_rounds']}; |J_k| {part['joints']}")
        say(f"{n} x {n} threshold {thr}: one call for all three, timed phases (ms): "
            + ", ".join(f"{k} {v:.3f}" for k, v in part["timed_ms"].items()))
    acc = step(lambda: fa.data.get())
    pour = np.zeros((n, n), np.int32)
    pour.ravel()[np.argsort(acc.ravel())[::-1][:5]] = [1, 2, 3, 4, 5]
    row["max_accumulation"] = float(acc.max())
    del acc
    pp = xs.DataArray(xs.DeviceArray.from_numpy(pour), dims=["y", "x"])
    row["watershed_ms"] = wall_ms(lambda: xs.watershed(fd, pp), reps, warmup)
    row["flow_length_ms"] = wall_ms(lambda: xs.flow_length(fd), reps, warmup)
    shed_words = step(lambda: hy.watershed_plane(fd.data, pp.data, np.zeros(0), 0)[1])
    len_words = step(lambda: hy.length_plane(fd.data, *hy.cell_distances(fd))[1])
    row["watershed_rounds"], row["flow_length_rounds"] = shed_words[0], len_words[0]
    say(f"{n} x {n}: watershed (five pour points) {row['watershed_ms']:.3f} ms, {shed_words[0]} rounds; flow_length "
        f"{row['flow_length_ms']:.3f} ms, {len_words[0]} rounds; largest accumulation {row['max_accumulation']:.0f}")
    return row


def main():
    global LIMIT
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[4096, 8192])
    ap.add_argument("--thresholds", nargs="*", type=float, default=[100, 1000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams", "streams_bench.json"))
    a = ap.parse_args()
    LIMIT = a.limit
    _lib.require_device()
    result = {"build_id": _lib.build_id(), "reps": a.reps, "warmup": a.warmup, "sizes": []}
    say(f"build {result['build_id']}, medians of {a.reps} after {a.warmup}")
    for n in a.sizes:
        result["sizes"].append(one_size(n, a.thresholds, a.reps, a.warmup))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        with open(os.path.splitext(a.out)[0] + ".log", "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

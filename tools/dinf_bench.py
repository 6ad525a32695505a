"""Time flow_direction(method='dinf') and flow_accumulation(method='dinf' | weights=..) on the filled, flat-resolved
`generate_terrain` raster, resident in HBM (default 4096^2 and 8192^2).

Per --sizes n, in one process:
  yardsticks   taken in the same run: xrs_copy_f32 between two events (8 B/cell), and `cost_distance` from one source in a corner
               over the friction 1 + slope (the same tile relaxer, min-plus: its call and its rounds)
  direction    `flow_direction(resolve_flats=True)` with method 'd8' and with 'dinf', the public functions on DeviceArrays, wall
               clock with a device sync
  accumulation with 'dinf', with 'd8' + weights (ones, float64) and plain 'd8'; and from the status words of one
               xrs_flow_accumulate_frac call with XRS_FRAC_TIMED: the rounds, the tiles launched per round, the cells that became
               final per round and the milliseconds of the first rounds
Medians of --reps after --warmup.  Every step runs under --limit seconds: a watchdog ends the process when a step takes longer.
No threshold is applied to any of it.  Writes --out (JSON) and the printed lines next to it (.log).
"""
import argparse
import ctypes
import faulthandler
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib, hydrology as hy  # noqa: E402

cd = importlib.import_module("xrspatial_amd.cost_distance")             # (the package's attribute of that name is the function)

LINES = []
LIMIT = 150


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


def rounds_of(words):
    info = hy.relax_rounds(words)
    kept = len(info["tiles"])
    return {"rounds": info["rounds"], "tiles_launched": info["tiles_launched"],
            "tiles_per_round": info["tiles_launched"] / max(info["rounds"], 1), "tiles_first_rounds": info["tiles"],
            "final_first_rounds": info["changed"], "round_ms_first_rounds": [ns / 1e6 for ns in info["ns"]],
            "rounds_kept": kept, "init_ms": words[2] / 1e6, "left_ms": words[3] / 1e6}


def one_size(n, reps, warmup):
    cells = n * n
    row = {"n": n, "cells": cells, "tiles": ((n + hy.TILE - 1) // hy.TILE) ** 2}
    terrain = step(lambda: xs.generate_terrain(xs.DataArray(xs.DeviceArray((n, n), np.float32), dims=["y", "x"])))
    cx, cy, dg = hy.cell_distances(terrain)
    filled = step(lambda: xs.fill(terrain))
    other = xs.DeviceArray((n, n), np.float32)
    row["yardstick_copy_8B_ms"] = step(lambda: kernel_ms(lambda: _lib.call("xrs_copy_f32", filled.data.ptr, other.ptr, cells, None), reps, warmup))
    del other

    friction = xs.DeviceArray.from_numpy((1.0 + xs.slope(terrain).data.get()).astype(np.float32))    # NaN on the raster's edge
    corner = np.zeros((n, n), np.uint8)
    corner[1, 1] = 1
    src = xs.DeviceArray.from_numpy(corner)
    none = np.zeros(0, np.float64)

    def cost(flags=0):
        return cd.cost_planes(src, friction, none, 0, cx, cy, dg, backlink=False, flags=flags)[2]

    row["yardstick_cost_distance_corner_ms"] = wall_ms(cost, reps, warmup)
    words = step(cost)
    row["yardstick_cost_distance_corner_rounds"], row["yardstick_cost_distance_corner_tiles"] = words[0], words[1]
    say(f"{n} x {n}: yardsticks  xrs_copy_f32 {row['yardstick_copy_8B_ms']:.3f} ms; cost_distance from a corner source "
        f"{row['yardstick_cost_distance_corner_ms']:.3f} ms in {words[0]} rounds, {words[1]} tiles launched ({row['tiles']} tiles of {hy.TILE}^2)")
    del friction, src

    row["direction_d8_ms"] = wall_ms(lambda: xs.flow_direction(filled, resolve_flats=True), reps, warmup)
    row["direction_dinf_ms"] = wall_ms(lambda: xs.flow_direction(filled, resolve_flats=True, method='dinf'), reps, warmup)
    row["direction_d8_plain_ms"] = wall_ms(lambda: xs.flow_direction(filled), reps, warmup)
    row["direction_dinf_plain_ms"] = wall_ms(lambda: xs.flow_direction(filled, method='dinf'), reps, warmup)
    say(f"{n} x {n}: flow_direction(resolve_flats=True)  d8 {row['direction_d8_ms']:.3f} ms, dinf {row['direction_dinf_ms']:.3f} ms; without "
        f"the flats  d8 {row['direction_d8_plain_ms']:.3f} ms, dinf {row['direction_dinf_plain_ms']:.3f} ms")

    codes = step(lambda: xs.flow_direction(filled, resolve_flats=True))
    angles = step(lambda: xs.flow_direction(filled, resolve_flats=True, method='dinf'))
    ones = xs.DataArray(xs.DeviceArray.from_numpy(np.ones((n, n), np.float64)), dims=["y", "x"])
    row["accumulation_d8_ms"] = wall_ms(lambda: xs.flow_accumulation(codes), reps, warmup)
    row["accumulation_d8_weights_ms"] = wall_ms(lambda: xs.flow_accumulation(codes, weights=ones), reps, warmup)
    row["accumulation_dinf_ms"] = wall_ms(lambda: xs.flow_accumulation(angles, method='dinf'), reps, warmup)
    say(f"{n} x {n}: flow_accumulation  d8 {row['accumulation_d8_ms']:.3f} ms, d8 + weights {row['accumulation_d8_weights_ms']:.3f} ms, "
        f"dinf {row['accumulation_dinf_ms']:.3f} ms")
    table = hy.angle_table(cx, cy)
    for label, plane, method in (("dinf", angles.data, hy.DINF), ("d8_weights", codes.data, hy.D8)):
        info = rounds_of(step(lambda: hy.frac_plane(plane, method, table, ones.data if method == hy.D8 else None, flags=hy.TIMED)[1]))
        row[f"rounds_{label}"] = info
        say(f"{n} x {n}: {label}  {info['rounds']} rounds, {info['tiles_launched']} tiles launched ({info['tiles_per_round']:.1f} a round); "
            f"init {info['init_ms']:.3f} ms, count of cells left {info['left_ms']:.3f} ms")
        for k in range(0, info["rounds_kept"], 8):
            say(f"{n} x {n}: {label}  round {k:3d}: {info['final_first_rounds'][k]:10d} cells final, {info['tiles_first_rounds'][k]:6d} tiles, "
                f"{info['round_ms_first_rounds'][k]:.3f} ms")
    acc = step(lambda: xs.flow_accumulation(angles, method='dinf').data.get())
    row["max_accumulation_dinf"] = float(acc.max())
    row["workspace_bytes"] = _lib.workspace_bytes("flow_accumulate_frac", n, n)
    say(f"{n} x {n}: largest dinf accumulation {row['max_accumulation_dinf']:.1f}; workspace {row['workspace_bytes']} bytes")
    return row


def main():
    global LIMIT
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=150, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dinf", "dinf_bench.json"))
    a = ap.parse_args()
    LIMIT = a.limit
    _lib.require_device()
    result = {"build_id": _lib.build_id(), "reps": a.reps, "warmup": a.warmup, "tile": hy.TILE, "sizes": []}
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

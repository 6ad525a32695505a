"""Time `cost_distance` on `generate_terrain` rasters resident in HBM (default 4096^2 and 8192^2; friction 1 + slope, float32).

Per --sizes n and per source layout (one source in a corner; 1000 random sources):
  timed       the status words of one xrs_cost_distance call with XRS_COST_TIMED (a stream sync around every launch, host clock):
              rounds, and per round the cells that fell, the tiles launched and the milliseconds (four colour launches and the
              launch that builds the next lists); the first launch (init) and the last two (links, mask)
  call        the same entry untimed (it syncs once a round), wall clock, with and without the back-link plane
  yardsticks  in the same run: xrs_copy_f32 between two events, and the `fill` call (fill_plane, wall clock) on the terrain
Medians of --reps after --warmup.  No threshold is applied to any of it.  Writes --out (JSON) and the printed lines next to it
(.log).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib, hydrology  # noqa: E402
from hydrology_bench import LINES, kernel_ms, say, wall_ms  # noqa: E402
from hydrology_fill_bench import timed_rounds  # noqa: E402

cd = importlib.import_module("xrspatial_amd.cost_distance")             # (the package's attribute of that name is the function)


def report(n, label, info):
    say(f"{n} x {n}: {label}  call {info['call_ms']:.3f} ms untimed ({info['call_distance_only_ms']:.3f} ms without the links); timed: "
        f"init {info['first_launch_ms']:.3f} ms, {info['rounds']} rounds {sum(info['round_ms']):.3f} ms (the first "
        f"{len(info['round_ms'])}), links + mask {info['last_launch_ms']:.3f} ms; {info['tiles_launched']} tiles launched in all; "
        f"{info['sources']} sources, {info['reached']} cells reached, {info['absorbed']} absorbed")
    kept = len(info["round_ms"])
    shown = sorted(set(range(min(4, kept))) | {kept // 2, kept - 1})
    for k in shown:
        say(f"{n} x {n}: {label}  round {k:3d}: {info['changed'][k]:10d} cells fell, {info['tiles'][k]:6d} tiles, {info['round_ms'][k]:.3f} ms")


def one_size(n, reps, warmup):
    cells = n * n
    row = {"n": n, "cells": cells, "tiles": ((n + hydrology.TILE - 1) // hydrology.TILE) ** 2}
    terrain = xs.generate_terrain(xs.DataArray(xs.DeviceArray((n, n), np.float32), dims=["y", "x"]))
    cx, cy, dg = hydrology.cell_distances(terrain)
    z = terrain.data
    other = xs.DeviceArray((n, n), np.float32)
    row["yardstick_copy_8B_ms"] = kernel_ms(lambda: _lib.call("xrs_copy_f32", z.ptr, other.ptr, cells, None), reps, warmup)
    del other
    row["yardstick_fill_call_ms"] = wall_ms(lambda: hydrology.fill_plane(z), reps, warmup)
    row["yardstick_fill_rounds"] = hydrology.fill_plane(z)[1][0]
    say(f"{n} x {n}: yardsticks  xrs_copy_f32 {row['yardstick_copy_8B_ms']:.3f} ms, fill {row['yardstick_fill_call_ms']:.3f} ms in "
        f"{row['yardstick_fill_rounds']} rounds; {row['tiles']} tiles of {hydrology.TILE}^2")
    friction = xs.DeviceArray.from_numpy((1.0 + xs.slope(terrain).data.get()).astype(np.float32))    # NaN on the raster's edge
    none = np.zeros(0, np.float64)

    layouts = {}
    corner = np.zeros((n, n), np.uint8)
    corner[1, 1] = 1                                                     # (row 0 and column 0 are impassable)
    layouts["corner_source"] = corner
    many = np.zeros((n, n), np.uint8)
    rng = np.random.default_rng(5)
    many[rng.integers(1, n - 1, 1000), rng.integers(1, n - 1, 1000)] = 1
    layouts["1000_random_sources"] = many
    for label, host in layouts.items():
        src = xs.DeviceArray.from_numpy(host)

        def run(flags=0, backlink=True):
            return cd.cost_planes(src, friction, none, 0, cx, cy, dg, backlink=backlink, flags=flags)[2]

        info = timed_rounds(lambda: run(cd.TIMED), reps, warmup)
        words = run()
        info["sources"], info["absorbed"], info["reached"] = words[cd.SOURCES], words[cd.ABSORBED], words[cd.REACHED]
        info["call_ms"] = wall_ms(run, reps, warmup)
        info["call_distance_only_ms"] = wall_ms(lambda: run(backlink=False), reps, warmup)
        info["workspace_bytes"] = _lib.workspace_bytes("cost_distance", n, n)
        row[label] = info
        report(n, label, info)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_distance", "cost_distance_bench.json"))
    a = ap.parse_args()
    _lib.require_device()
    result = {"build_id": _lib.build_id(), "reps": a.reps, "warmup": a.warmup, "tile": hydrology.TILE, "sizes": []}
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

"""Time `fill` and the flat resolution on `generate_terrain` rasters resident in HBM (default 4096^2 and 8192^2, float32).

Per --sizes n:
  fill, flats  the status words of one xrs_fill / xrs_flow_flats call with XRS_FILL_TIMED (a stream sync around every launch,
               host clock): rounds, and per round the cells that changed, the tiles launched and the milliseconds (four colour
               launches and the launch that builds the next lists); the flats run on flow_direction of the filled raster
  call         the same entry untimed (it syncs once a round), wall clock
  yardsticks   in the same run: xrs_copy_f32 between two events, and the flow_accumulation call (flow_graph, wall clock) on the
               resolved direction raster
  effect       outlets, largest accumulation and pointer-doubling rounds of the resolved raster, beside the unfilled one's
Medians of --reps after --warmup.  No threshold is applied to any of it.  Writes --out (JSON) and the printed lines next to it
(.log).
"""
import argparse
import ctypes
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


def timed_rounds(run, reps, warmup):
    """Medians over `reps` runs of the status words `run()` returns, as a dict with per-round lists."""
    runs = [run() for _ in range(warmup + reps)][warmup:]
    info = hydrology.relax_rounds(runs[-1])
    med = np.median(np.array(runs, np.float64), axis=0)
    kept = len(info["changed"])
    info["round_ms"] = [float(v) / 1e6 for v in med[8 + 2 * hydrology.FILL_STATUS_ROUNDS:8 + 2 * hydrology.FILL_STATUS_ROUNDS + kept]]
    info["first_launch_ms"], info["last_launch_ms"] = float(med[2]) / 1e6, float(med[3]) / 1e6
    del info["ns"]
    return info


def report(n, label, info):
    say(f"{n} x {n}: {label}  call {info['call_ms']:.3f} ms untimed; timed: first launch {info['first_launch_ms']:.3f} ms, "
        f"{info['rounds']} rounds {sum(info['round_ms']):.3f} ms (the first {len(info['round_ms'])}), last launch "
        f"{info['last_launch_ms']:.3f} ms; {info['tiles_launched']} tiles launched in all")
    for k, ms in enumerate(info["round_ms"]):
        say(f"{n} x {n}: {label}  round {k:2d}: {info['changed'][k]:10d} cells changed, {info['tiles'][k]:6d} tiles, {ms:.3f} ms")


def one_size(n, reps, warmup):
    cells = n * n
    row = {"n": n, "cells": cells, "tiles": ((n + hydrology.TILE - 1) // hydrology.TILE) ** 2}
    terrain = xs.generate_terrain(xs.DataArray(xs.DeviceArray((n, n), np.float32), dims=["y", "x"]))
    cx, cy, dg = hydrology.cell_distances(terrain)
    z = terrain.data
    other = xs.DeviceArray((n, n), np.float32)
    row["yardstick_copy_8B_ms"] = kernel_ms(lambda: _lib.call("xrs_copy_f32", z.ptr, other.ptr, cells, None), reps, warmup)
    say(f"{n} x {n}: yardstick xrs_copy_f32 {row['yardstick_copy_8B_ms']:.3f} ms, {row['tiles']} tiles of {hydrology.TILE}^2")
    del other

    info = timed_rounds(lambda: hydrology.fill_plane(z, flags=hydrology.TIMED)[1], reps, warmup)
    info["call_ms"] = wall_ms(lambda: hydrology.fill_plane(z), reps, warmup)
    info["workspace_bytes"] = _lib.workspace_bytes("fill", n, n)
    row["fill"] = info
    report(n, "fill", info)
    filled = hydrology.fill_plane(z)[0]
    xs.synchronize()
    row["cells_raised"] = int(np.count_nonzero(filled.get() != z.get()))

    codes = xs.DeviceArray((n, n), np.float32)

    def flats(flags=0):
        _lib.call("xrs_flow_direction", filled.ptr, 9, n, n, cx, cy, dg, codes.ptr, None)
        return hydrology.resolve_flats_plane(filled, codes, flags=flags)

    info = timed_rounds(lambda: flats(hydrology.TIMED), reps, warmup)
    info["call_ms"] = wall_ms(flats, reps, warmup)                       # (with the plain direction launch in front: + ~0.3 ms at 8192^2)
    info["workspace_bytes"] = _lib.workspace_bytes("flow_flats", n, n)
    row["flats"] = info
    report(n, "flats", info)

    flats()
    xs.synchronize()
    plain = xs.flow_direction(terrain).data
    for label, d in (("resolved", codes), ("unfilled", plain)):
        acc, bas, words = hydrology.flow_graph(d, hydrology.ACCUMULATION | hydrology.BASINS)
        part = {"doubling_rounds": words[0], "max_accumulation": float(np.nanmax(acc.get())), "outlets": int(np.unique(bas.get()).size)}
        part["accumulation_call_ms"] = wall_ms(lambda: hydrology.flow_graph(d, hydrology.ACCUMULATION), reps, warmup)
        row[label] = part
        say(f"{n} x {n}: {label} direction raster  {part['outlets']} outlets, largest accumulation {part['max_accumulation']:.0f}, "
            f"{part['doubling_rounds']} doubling rounds, flow_accumulation call {part['accumulation_call_ms']:.3f} ms")
    say(f"{n} x {n}: fill raised {row['cells_raised']} cells; fill {row['fill']['call_ms']:.3f} ms + flats {row['flats']['call_ms']:.3f} ms "
        f"against flow_accumulation {row['resolved']['accumulation_call_ms']:.3f} ms on the resolved raster")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hydrology_fill", "hydrology_fill_bench.json"))
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

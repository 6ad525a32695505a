"""Time bump's device work: xrs_bump_f64 on resident locations and heights, result left in HBM.

Per --cases n:spread (an n x n raster at the default density, count = n * n // 10, unit heights, locations from a seeded generator):
  call      the whole entry, wall clock (it ends with a stream sync of its own), median of --reps after --warmup
  events, chunks, passes, touched cells    the call's status words
  expand / sort / fold    the entry's own split: count + scan + emit, radix sort + segment heads, the passes of the fold
  finish_bump             the Python entry with device=True: the same plus the upload of locations and heights

No threshold is applied to any of it.  Writes --out (JSON) and the printed lines next to it (.log).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402
from xrspatial_amd.bump import DEFAULT_MAX_EVENTS, STATUS_WORDS, finish_bump  # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def one_case(n, spread, reps, warmup, max_events):
    count = n * n // 10
    rng = np.random.default_rng(n + spread)
    locs = rng.integers(0, n, (count, 2)).astype(np.uint16)
    heights = np.ones(count)
    lib = _lib.load()
    nbytes = int(lib.xrs_bump_workspace_bytes(count, n, n, spread, max_events))
    if not nbytes:
        raise SystemExit(f"{n}:{spread}: the arguments are refused")
    locs_d, z_d = xs.DeviceArray.from_numpy(locs), xs.DeviceArray.from_numpy(heights)
    out = xs.DeviceArray((n, n), np.float64)
    work = xs.DeviceArray((nbytes,), np.uint8)
    words = (ctypes.c_int64 * 8)()
    rows = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        _lib.call("xrs_bump_f64", locs_d.ptr, z_d.ptr, count, n, n, spread, out.ptr, work.ptr, nbytes, max_events, words, None)
        ms = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            rows.append([ms] + [int(w) for w in words][:len(STATUS_WORDS)])
    med = np.median(np.array(rows, np.float64), axis=0)
    row = {"n": n, "spread": spread, "count": count, "workspace_bytes": nbytes, "call_ms": float(med[0])}
    row.update({k: int(v) for k, v in zip(STATUS_WORDS, rows[-1][1:])})
    for k, v in zip(STATUS_WORDS[4:], med[5:]):
        row[k.replace("_ns", "_ms")] = float(v) / 1e6
        del row[k]
    del work, locs_d, z_d
    ts = []
    for _ in range(max(1, min(reps, 2))):
        t0 = time.perf_counter()
        finish_bump(n, n, locs, heights, spread, device=True, max_events=max_events)
        xs.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    row["finish_bump_ms"] = float(np.median(ts))
    row["checksum"] = float(out.get().sum())
    say(f"{n} x {n}, spread {spread}, {count} bumps: call {row['call_ms']:9.2f} ms = expand {row['expand_ms']:8.2f} + sort "
        f"{row['sort_ms']:8.2f} + fold {row['fold_ms']:8.2f}  |  {row['events']} events, {row['touched_cells']} touched cells, "
        f"{row['chunks']} chunks, {row['passes']} passes ({row['fold_ms'] / row['passes']:.3f} ms each), workspace "
        f"{nbytes / 2**30:.2f} GiB  |  finish_bump(device=True) {row['finish_bump_ms']:9.2f} ms")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["4096:1", "4096:3", "4096:8", "16384:1"])
    ap.add_argument("--max-events", type=int, default=DEFAULT_MAX_EVENTS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bump", "bump_bench.json"))
    a = ap.parse_args()
    _lib.require_device()
    result = {"build_id": _lib.build_id(), "reps": a.reps, "warmup": a.warmup, "max_events": a.max_events, "cases": []}
    say(f"build {result['build_id']}, medians of {a.reps} after {a.warmup}, at most {a.max_events} events a chunk")
    for case in a.cases:
        n, spread = (int(v) for v in case.split(":"))
        result["cases"].append(one_case(n, spread, a.reps, a.warmup, a.max_events))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
        with open(os.path.splitext(a.out)[0] + ".log", "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()

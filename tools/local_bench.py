"""Time the functions of xrspatial_amd.local (float32 DeviceArray planes in, the result stays in HBM).

--planes (8) float32 planes of --n x --n (8192) cells.  For each of the eight per-cell entry points (cell_stats with its six
functions counted one by one, a frequency, a position, rank, popularity) it prints the device time of `xrs_local_cells`
between two events (median of --reps after --warmup) and the rate in GB/s of ALGORITHMIC bytes: N x itemsize read plus 8
written per cell (std reads its planes twice; that is not counted).  `combine` runs on planes of the values 1 .. 4 and is
timed as the whole `xrs_local_combine` call (it synchronises after every plane), at the same byte count.  The yardstick is a
device-to-device copy that moves the same number of bytes (half of them read, half written), measured in the same run, before
and after the functions.  No threshold is applied to any of it; the reference has no usable time at this size.

    python tools/local_bench.py [--n 8192] [--planes 8] [--reps 5] [--warmup 2] [--log profiles/local/local_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib, local  # noqa: E402
from tools.terrain_bench import call_ms, kernel_ms  # noqa: E402

OPS = [("max", local.MAX), ("min", local.MIN), ("sum", local.SUM), ("mean", local.MEAN), ("std", local.STD), ("median", local.MEDIAN),
       ("equal_frequency", local.EQUAL), ("lowest_position", local.LOWEST), ("rank", local.RANK), ("popularity", local.POPULARITY)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "local", "local_bench.json"))
    a = ap.parse_args()
    _lib.require_device()
    n, count = a.n, a.planes
    cells = n * n
    nbytes = cells * (count * 4 + 8)                                   # algorithmic bytes of one call
    rng = np.random.default_rng(11)
    base = rng.normal(scale=50.0, size=cells).astype(np.float32)
    sets = rng.integers(1, 5, cells).astype(np.float32)
    planes = [xs.DeviceArray.from_numpy(np.roll(base, 977 * j).reshape(n, n)) for j in range(count)]
    small = [xs.DeviceArray.from_numpy(np.roll(sets, 977 * j).reshape(n, n)) for j in range(count)]
    ref = xs.DeviceArray.from_numpy(rng.integers(1, count + 1, (n, n)).astype(np.int32))
    out = xs.DeviceArray((n, n), np.float64)
    src, dst = xs.DeviceArray((nbytes // 2,), np.uint8), xs.DeviceArray((nbytes // 2,), np.uint8)
    _lib.call("xrs_memset", src.ptr, 1, nbytes // 2, None)

    def copy_ms():
        return kernel_ms(lambda: _lib.call("xrs_memcpy_d2d", dst.ptr, src.ptr, nbytes // 2, None), a.reps, a.warmup)

    def gbs(ms):
        return nbytes / ms / 1e6

    rows = []
    copy_before = copy_ms()
    print(f"{n} x {n} cells, {count} float32 planes, {nbytes / 1e9:.3f} GB per call; copy of the same bytes {copy_before:.3f} ms "
          f"{gbs(copy_before):7.0f} GB/s", flush=True)
    for name, op in OPS:
        for label, dev in (("normal", planes), ("1..4", small)) if name in ("median", "rank", "popularity", "equal_frequency") else (("normal", planes),):
            ptrs, codes = local._plane_table(dev)
            ref_dev = dev[0] if op == local.EQUAL else ref
            ms = kernel_ms(lambda: _lib.call("xrs_local_cells", op, ptrs, codes, count, ref_dev.ptr, xs.device.DTYPE_CODE[ref_dev.dtype],
                                             cells, out.ptr, 0, None), a.reps, a.warmup)
            rows.append({"function": name, "values": label, "ms": ms, "GB_per_s": gbs(ms)})
            print(f"{name:18s} {label:7s} {ms:9.3f} ms {gbs(ms):7.0f} GB/s", flush=True)
    ptrs, codes = local._plane_table(small)
    lib = _lib.load()
    work_bytes = int(lib.xrs_local_combine_workspace_bytes(cells, count))
    work = xs.DeviceArray((work_bytes,), np.uint8)
    classes = ctypes.c_int64(0)
    ms = call_ms(lambda: _lib.call("xrs_local_combine", ptrs, codes, count, cells, work.ptr, work_bytes, out.ptr, None, 0,
                                   ctypes.byref(classes), None), max(1, a.reps // 2), 1)
    rows.append({"function": "combine", "values": "1..4", "ms": ms, "GB_per_s": gbs(ms), "classes": int(classes.value),
                 "workspace_bytes": work_bytes})
    print(f"{'combine':18s} {'1..4':7s} {ms:9.3f} ms {gbs(ms):7.0f} GB/s   {classes.value} classes, workspace {work_bytes / 1e9:.2f} GB", flush=True)
    copy_after = copy_ms()
    print(f"copy of the same bytes, after: {copy_after:.3f} ms {gbs(copy_after):7.0f} GB/s", flush=True)
    res = {"n": n, "planes": count, "dtype": "float32", "algorithmic_bytes": nbytes, "build_id": _lib.build_id(), "reps": a.reps,
           "copy_ms_before": copy_before, "copy_ms_after": copy_after, "copy_GB_per_s": [gbs(copy_before), gbs(copy_after)], "rows": rows}
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

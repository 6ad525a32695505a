"""Time resample's three ABI calls with everything resident in HBM -- the source plane, the tables and the result -- each next to
its yardstick measured in the same run: a plain device fill of the destination plane (`xrs_memset`) for the upsampling cases,
the floor of anything that writes every cell once, and a plain device copy of the source plane (`xrs_memcpy_d2d`) for the
downsampling cases, the floor of anything that reads every cell once.  A figure is a call followed by a device sync, by the
host's clock; median of --reps after --warmup.

Cases: --up x --up float32 -> twice that by nearest, bilinear, cubic and lanczos; --down x --down float32 -> a quarter by
average (the LDS tile kernel) and -> 1/128 by average (one wave per cell); --down x --down uint8 land cover (12 classes in
patches) -> a quarter by mode and max.  The tables are built by `resample.tables` once per case and are not part of the figure
(`tables_ms` says what they cost on the host).  Prints one JSON row per case; writes <out>/resample_bench.json after every row
and <out>/resample_bench.log (the same rows as text).

    python tools/resample_bench.py [--up 8192] [--down 16384] [--only nearest bilinear ...] [--reps 5] [--warmup 2]
                                   [--out profiles/resample]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import xrspatial_amd as xs  # noqa: E402
from tools.regions_bench import timed  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402
from xrspatial_amd.device import DTYPE_CODE  # noqa: E402

R = xs.resample
SELECT_OP = {"min": 0, "max": 1, "mode": 2}


def dem(n):
    """A smooth float32 surface with relief, generated in row bands to keep the host's peak memory low."""
    out = np.empty((n, n), np.float32)
    x = np.arange(n, dtype=np.float32)[None, :]
    for r0 in range(0, n, 1024):
        y = np.arange(r0, min(r0 + 1024, n), dtype=np.float32)[:, None]
        out[r0:r0 + 1024] = 2000.0 + 800.0 * np.sin(x / 300.0) * np.cos(y / 400.0) + 5.0 * np.sin(x * 0.7 + y * 1.3)
    return out


def land_cover(n):
    """uint8 classes 0 .. 11 in patches of 8 x 8 cells with a speckle of single cells, so a 4 x 4 window holds 1 - 3 classes."""
    rng = np.random.default_rng(5)
    out = np.repeat(np.repeat(rng.integers(0, 12, (n // 8, n // 8), dtype=np.uint8), 8, axis=0), 8, axis=1)
    speckle = rng.integers(0, n, (n * n // 16, 2))
    out[speckle[:, 0], speckle[:, 1]] = rng.integers(0, 12, len(speckle), dtype=np.uint8)
    return out


def launch_of(method, src, dst_shape, tab, dev, out):
    """A callable that makes the one ABI call of `method`."""
    code = DTYPE_CODE[np.dtype(src.dtype)]
    head = (src.ptr, code, src.shape[0], src.shape[1], None, dst_shape[0], dst_shape[1])
    fill = np.zeros(1, src.dtype)
    ptr = lambda key: dev[key].ptr if key in dev else None  # noqa: E731
    if method == "nearest":
        return lambda: _lib.call("xrs_resample_gather", *head, ptr("near_y"), ptr("near_x"), fill.ctypes.data, out.ptr, None)
    taps = (ptr("first_y"), ptr("w_y"), tab["w_y"].shape[1], ptr("first_x"), ptr("w_x"), tab["w_x"].shape[1])
    if method in SELECT_OP:
        return lambda: _lib.call("xrs_resample_select", *head, *taps, SELECT_OP[method], fill.ctypes.data, out.ptr, None)
    fb = 2 if "fb_w_y" in tab else 0
    return lambda: _lib.call("xrs_resample_weighted", *head, *taps, ptr("near_y"), ptr("near_x"), ptr("fb_first_y"), ptr("fb_w_y"),
                             fb, ptr("fb_first_x"), ptr("fb_w_x"), fb, int(method != "sum"), DTYPE_CODE[np.dtype(out.dtype)],
                             float("nan"), out.ptr, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--up", type=int, default=8192)
    ap.add_argument("--down", type=int, default=16384)
    ap.add_argument("--only", nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample"))
    a = ap.parse_args()
    _lib.require_device()
    os.makedirs(a.out, exist_ok=True)
    up, down = a.up, a.down
    cases = [("up", m, np.float32, (up, up), (2 * up, 2 * up)) for m in ("nearest", "bilinear", "cubic", "lanczos")]
    cases += [("down", "average", np.float32, (down, down), (down // 4, down // 4)),
              ("down", "average", np.float32, (down, down), (down // 128, down // 128)),
              ("down", "mode", np.uint8, (down, down), (down // 4, down // 4)),
              ("down", "max", np.uint8, (down, down), (down // 4, down // 4))]
    rows = []
    log = open(os.path.join(a.out, "resample_bench.log"), "w")
    held = {}
    for kind, method, dtype, src_shape, dst_shape in cases:
        if a.only and method not in a.only:
            continue
        key = (np.dtype(dtype).name, src_shape)
        if key not in held:
            held.clear()
            xs.empty_cache()
            held[key] = xs.DeviceArray.from_numpy(dem(src_shape[0]) if dtype == np.float32 else land_cover(src_shape[0]))
        src = held[key]
        out_dtype = np.dtype(dtype)
        out = xs.DeviceArray(dst_shape, out_dtype)
        t0 = time.perf_counter()
        tab = R.tables(method, src_shape, dst_shape, None, R.shape_transform(src_shape, dst_shape))
        tables_ms = (time.perf_counter() - t0) * 1e3
        dev = {k: xs.DeviceArray.from_numpy(v) for k, v in tab.items()}
        if kind == "up":
            yard_name, yard_bytes = "fill_dst", out.nbytes
            yard_ms, _ = timed(lambda: _lib.call("xrs_memset", out.ptr, 0, out.nbytes, None), a.reps, a.warmup)
        else:
            spare = xs.DeviceArray(src_shape, dtype)
            yard_name, yard_bytes = "copy_src", 2 * src.nbytes
            yard_ms, _ = timed(lambda: _lib.call("xrs_memcpy_d2d", spare.ptr, src.ptr, src.nbytes, None), a.reps, a.warmup)
            del spare
        ms, best = timed(launch_of(method, src, dst_shape, tab, dev, out), a.reps, a.warmup)
        cells = dst_shape[0] * dst_shape[1]
        row = {"case": f"{src_shape[0]}^2 {np.dtype(dtype).name} -> {dst_shape[0]}^2", "method": method,
               "taps": [int(tab["w_y"].shape[1]), int(tab["w_x"].shape[1])] if "w_y" in tab else None,
               "ms": round(ms, 3), "ms_min": round(best, 3), "yardstick": yard_name, "yardstick_ms": round(yard_ms, 3),
               "yardstick_gb_s": round(yard_bytes / yard_ms / 1e6, 1), "over_yardstick": round(ms / yard_ms, 2),
               "ns_per_dst_cell": round(ms * 1e6 / cells, 4), "gb_s_src_plus_dst": round((src.nbytes + out.nbytes) / ms / 1e6, 1),
               "tables_ms": round(tables_ms, 1)}
        print(json.dumps(row), flush=True)
        log.write(json.dumps(row) + "\n")
        log.flush()
        rows.append(row)
        with open(os.path.join(a.out, "resample_bench.json"), "w") as fh:
            json.dump({"build_id": _lib.build_id(), "rows": rows}, fh, indent=1)
        del dev, out
    held.clear()
    xs.empty_cache()


if __name__ == "__main__":
    main()

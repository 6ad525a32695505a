"""Time hillshade(shadows=True) on generate_terrain output (float32 DeviceArray, the result stays in HBM).

For every sun altitude asked for (azimuth 225) at n x n cells it prints, in ms (median of --reps after --warmup, device
events around both launches of the entry point: the prepare pass and the walk):
  the walk with the block level over 32 x 32 cells (what the API runs), over 16 x 16 and 8 x 8, and the plain cell walk
  without a block level (xrs_hillshade_shadow_probe_f32), Mcells/s of the first;
  the whole API call (the finite-cell reduction, the workspace, both kernels, a stream sync);
  the plain `hillshade` kernel and a device-to-device copy of the same float32 plane, for scale.
The mean and maximum number of cells and blocks a ray visits come from the counting build of the walk on the top-left
--crop x --crop cells of the same terrain (its atomics would distort a timing: it is never timed).  The share of shadowed
cells is read off the result, and the four variants must return the same plane.  No threshold is applied to any of it.

One altitude per process keeps every GPU step short enough for a time limit of its own:
    for alt in 5 25 60; do timeout -k 10 300 python tools/hillshade_shadow_bench.py --altitudes $alt || break; done
Results are appended to --log (JSON lines) and printed as a table row.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import xrspatial_amd as xs  # noqa: E402
from xrspatial_amd import _lib  # noqa: E402
from xrspatial_amd.hillshade import sun_vector  # noqa: E402
from tools.terrain_bench import call_ms, kernel_ms  # noqa: E402

CELL = 30.0
AZIMUTH = 225
BLOCKS = (32, 16, 8, 0)                        # the API's first


def terrain(n):
    agg = xs.DataArray(xs.DeviceArray((n, n), np.float32), dims=["y", "x"])
    return xs.generate_terrain(agg, x_range=(0, CELL * n), y_range=(0, CELL * n))


def bounds(dev):
    """(min, max) of a float32 DeviceArray through the one-pass reduction the API uses"""
    stats = xs.DeviceArray((4,), np.float64)
    work = xs.DeviceArray((int(_lib.load().xrs_classify_workspace_bytes(1, 0)),), np.uint8)
    _lib.call("xrs_classify_finite_stats_f32", dev.ptr, dev.size, work.ptr, stats.ptr, None)
    count, zmin, zmax, _ = (float(v) for v in stats.get())
    assert int(count) == dev.size and zmax > 0
    return zmin, zmax


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--crop", type=int, default=1024)
    ap.add_argument("--altitudes", type=float, nargs="+", default=[5, 25, 60])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "hillshade_shadows", "hillshade_shadow_bench.jsonl"))
    a = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    n = a.n
    dem = terrain(n)
    src = dem.data
    zmin, zmax = bounds(src)
    out = xs.DeviceArray((n, n), np.float32)
    work = xs.DeviceArray((int(lib.xrs_hillshade_shadow_workspace_bytes(n, n)),), np.uint8)
    crop = min(a.crop, n)
    small = xs.DeviceArray.from_numpy(np.ascontiguousarray(src.get()[:crop, :crop]))
    smin, smax = bounds(small)
    small_out = xs.DeviceArray((crop, crop), np.float32)
    small_work = xs.DeviceArray((int(lib.xrs_hillshade_shadow_workspace_bytes(crop, crop)),), np.uint8)

    plain_ms = call_ms(lambda: xs.hillshade(dem, azimuth=AZIMUTH, angle_altitude=25), a.reps, a.warmup)
    copy_ms = kernel_ms(lambda: _lib.call("xrs_memcpy_d2d", out.ptr, src.ptr, n * n * 4, None), a.reps, a.warmup)
    for alt in a.altitudes:
        sun = sun_vector(AZIMUTH, alt)
        row = {"n": n, "azimuth": AZIMUTH, "altitude": alt, "reps": a.reps, "build_id": _lib.build_id(),
               "plain_hillshade_call_ms": plain_ms, "d2d_copy_ms": copy_ms}
        for block in BLOCKS:
            launch = lambda: _lib.call("xrs_hillshade_shadow_probe_f32", src.ptr, n, n, float(n) / zmax, zmin, zmax, sun[0], sun[1],  # noqa: E731
                                       sun[2], block, work.ptr, out.ptr, None, None)
            row[f"kernels_ms_block{block}"] = kernel_ms(launch, a.reps, a.warmup)
            if block != BLOCKS[0]:                                  # every variant must give the same plane
                assert np.array_equal(out.get()[1:-1, 1:-1], shade), f"block {block} differs from block {BLOCKS[0]}"
            else:
                shade = out.get()[1:-1, 1:-1]
                flag_off = xs.DeviceArray((n, n), np.float32)
                _lib.call("xrs_hillshade_shadow_f32", src.ptr, n, n, float(n) / zmax, zmin, zmax, sun[0], sun[1], sun[2], 0, work.ptr,
                          flag_off.ptr, None)
                _lib.call("xrs_device_sync")
                row["shadow_share"] = float(np.mean(shade != flag_off.get()[1:-1, 1:-1]))
                del flag_off
            counts = xs.DeviceArray.from_numpy(np.zeros(4, np.uint64))
            _lib.call("xrs_hillshade_shadow_probe_f32", small.ptr, crop, crop, float(crop) / smax, smin, smax, sun[0], sun[1], sun[2],
                      block, small_work.ptr, small_out.ptr, counts.ptr, None)
            _lib.call("xrs_device_sync")
            c = counts.get().astype(np.float64)
            rays = float((crop - 2) * (crop - 2))
            row[f"crop_cells_mean_block{block}"], row[f"crop_cells_max_block{block}"] = c[0] / rays, c[1]
            row[f"crop_blocks_mean_block{block}"], row[f"crop_blocks_max_block{block}"] = c[2] / rays, c[3]
        row["mcells_per_s"] = n * n / row[f"kernels_ms_block{BLOCKS[0]}"] / 1e3
        row["api_call_ms"] = call_ms(lambda: xs.hillshade(dem, azimuth=AZIMUTH, angle_altitude=alt, shadows=True), a.reps, a.warmup)
        print(f"{n} x {n} alt {alt:4.0f}: B32 {row['kernels_ms_block32']:9.3f} ms ({row['mcells_per_s']:8.0f} Mcells/s)  B16 "
              f"{row['kernels_ms_block16']:9.3f}  B8 {row['kernels_ms_block8']:9.3f}  plain walk {row['kernels_ms_block0']:9.3f}  API call "
              f"{row['api_call_ms']:9.3f}  |  hillshade {plain_ms:7.3f}  d2d copy {copy_ms:7.3f}  |  shadow {row['shadow_share']:6.2%}  |  "
              f"{crop}^2 crop, per ray: cells mean {row['crop_cells_mean_block32']:.1f} max {row['crop_cells_max_block32']:.0f}, blocks mean "
              f"{row['crop_blocks_mean_block32']:.1f} max {row['crop_blocks_max_block32']:.0f}; plain walk cells mean "
              f"{row['crop_cells_mean_block0']:.1f} max {row['crop_cells_max_block0']:.0f}", flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, "a") as fh:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()

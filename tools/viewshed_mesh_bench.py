"""Time viewshed(method='mesh') on generate_terrain output (float32 DeviceArray, the result stays in HBM).

For n x n cells, the observer at the raster's centre and at a corner, observer_elev 10 and 100, it prints, in ms (median of
--reps after --warmup, device events around both launches of the entry point: the prepare pass and the walk):
  the walk with the block level over 32 x 32 cells (what the API runs), over 16 x 16 and 8 x 8 (xrs_viewshed_mesh_probe_f32),
  Mcells/s of the first;
  the whole API call (the finite-cell reduction, the workspace, both kernels, a stream sync);
  the existing sweep `viewshed` call from the same observer and a device-to-device copy of the float32 plane, for scale.
The plain cell walk without a block level is timed on the top-left --crop x --crop cells only (observer at that crop's centre
or corner): at full size a sight line is thousands of cells long, and that walk is what the block level is there to avoid.  The
mean and maximum number of cells and blocks a ray visits come from the counting build of the walk on the same crop (its
atomics would distort a timing: it is never timed).  The share of visible cells is read off the result, and the variants must
return the same plane.  No threshold is applied to any of it.

One size per process keeps every GPU step short enough for a time limit of its own:
    for n in 4096 8192; do timeout -k 10 600 python tools/viewshed_mesh_bench.py --n $n || break; done
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
from tools.hillshade_shadow_bench import bounds, terrain  # noqa: E402
from tools.terrain_bench import call_ms, kernel_ms  # noqa: E402

BLOCKS = (32, 16, 8)                           # the API's first
ELEVS = (10.0, 100.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--crop", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-sweep", action="store_true", help="leave the sweep viewshed yardstick out")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "viewshed_mesh", "viewshed_mesh_bench.jsonl"))
    a = ap.parse_args()
    _lib.require_device()
    lib = _lib.load()
    n = a.n
    dem = terrain(n)
    src = dem.data
    xc, yc = np.asarray(dem["x"].data), np.asarray(dem["y"].data)
    ew_res, ns_res = float(xc[-1] - xc[0]) / (n - 1), float(yc[-1] - yc[0]) / (n - 1)
    zmin, zmax = bounds(src)
    out = xs.DeviceArray((n, n), np.float32)
    work = xs.DeviceArray((int(lib.xrs_viewshed_mesh_workspace_bytes(n, n)),), np.uint8)
    crop = min(a.crop, n)
    small = xs.DeviceArray.from_numpy(np.ascontiguousarray(src.get()[:crop, :crop]))
    smin, smax = bounds(small)
    small_out = xs.DeviceArray((crop, crop), np.float32)
    small_work = xs.DeviceArray((int(lib.xrs_viewshed_mesh_workspace_bytes(crop, crop)),), np.uint8)
    copy_ms = kernel_ms(lambda: _lib.call("xrs_memcpy_d2d", out.ptr, src.ptr, n * n * 4, None), a.reps, a.warmup)

    for where, at in (("centre", lambda m: (m // 2, m // 2)), ("corner", lambda m: (0, 0))):
        (row, col), (srow, scol) = at(n), at(crop)
        sweep_ms = None
        if not a.no_sweep:
            sweep_ms = call_ms(lambda: xs.viewshed(dem, x=float(xc[col]), y=float(yc[row]), observer_elev=ELEVS[0]), a.reps, a.warmup)
        for oe in ELEVS:
            rec = {"n": n, "viewpoint": where, "observer_elev": oe, "reps": a.reps, "build_id": _lib.build_id(), "d2d_copy_ms": copy_ms,
                   "sweep_viewshed_call_ms": sweep_ms, "sweep_observer_elev": ELEVS[0]}
            full = (src.ptr, n, n, float(n) / zmax, zmin, zmax, row, col, oe, 0.0, ew_res, ns_res)
            part = (small.ptr, crop, crop, float(crop) / smax, smin, smax, srow, scol, oe, 0.0, ew_res, ns_res)
            for block in BLOCKS + (0,):
                if block:
                    launch = lambda: _lib.call("xrs_viewshed_mesh_probe_f32", *full, block, work.ptr, out.ptr, None, None)  # noqa: E731
                    rec[f"kernels_ms_block{block}"] = kernel_ms(launch, a.reps, a.warmup)
                    if block != BLOCKS[0]:                          # every variant must give the same plane
                        assert np.array_equal(out.get(), plane), f"block {block} differs from block {BLOCKS[0]}"
                    else:
                        plane = out.get()
                        rec["visible_share"] = float(np.mean(plane != -1))
                launch = lambda: _lib.call("xrs_viewshed_mesh_probe_f32", *part, block, small_work.ptr, small_out.ptr, None, None)  # noqa: E731
                rec[f"crop_kernels_ms_block{block}"] = kernel_ms(launch, a.reps, a.warmup)
                if block != BLOCKS[0]:
                    assert np.array_equal(small_out.get(), small_plane), f"crop: block {block} differs from block {BLOCKS[0]}"
                else:
                    small_plane = small_out.get()
                    rec["crop_visible_share"] = float(np.mean(small_plane != -1))
                counts = xs.DeviceArray.from_numpy(np.zeros(4, np.uint64))
                _lib.call("xrs_viewshed_mesh_probe_f32", *part, block, small_work.ptr, small_out.ptr, counts.ptr, None)
                _lib.call("xrs_device_sync")
                c = counts.get().astype(np.float64)
                rays = float(crop * crop - 1)
                rec[f"crop_cells_mean_block{block}"], rec[f"crop_cells_max_block{block}"] = c[0] / rays, c[1]
                rec[f"crop_blocks_mean_block{block}"], rec[f"crop_blocks_max_block{block}"] = c[2] / rays, c[3]
            rec["mcells_per_s"] = n * n / rec[f"kernels_ms_block{BLOCKS[0]}"] / 1e3
            rec["api_call_ms"] = call_ms(lambda: xs.viewshed(dem, x=float(xc[col]), y=float(yc[row]), observer_elev=oe, method="mesh"),
                                         a.reps, a.warmup)
            sweep = "      n/a" if sweep_ms is None else f"{sweep_ms:9.3f}"
            print(f"{n} x {n} {where:<6s} oe {oe:5.0f}: B32 {rec['kernels_ms_block32']:9.3f} ms ({rec['mcells_per_s']:8.0f} Mcells/s)  B16 "
                  f"{rec['kernels_ms_block16']:9.3f}  B8 {rec['kernels_ms_block8']:9.3f}  API call {rec['api_call_ms']:9.3f}  |  sweep viewshed "
                  f"{sweep}  d2d copy {copy_ms:7.3f}  |  visible {rec['visible_share']:6.2%}  |  {crop}^2 crop (visible "
                  f"{rec['crop_visible_share']:6.2%}): B32 {rec['crop_kernels_ms_block32']:8.3f} ms  B16 {rec['crop_kernels_ms_block16']:8.3f}  B8 "
                  f"{rec['crop_kernels_ms_block8']:8.3f}  plain walk {rec['crop_kernels_ms_block0']:8.3f}; per ray with B32: cells mean "
                  f"{rec['crop_cells_mean_block32']:.1f} max {rec['crop_cells_max_block32']:.0f}, blocks mean {rec['crop_blocks_mean_block32']:.1f} max "
                  f"{rec['crop_blocks_max_block32']:.0f}; plain walk cells mean {rec['crop_cells_mean_block0']:.1f} max "
                  f"{rec['crop_cells_max_block0']:.0f}", flush=True)
            if a.log:
                os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
                with open(a.log, "a") as fh:
                    fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

"""Outputs of the reference's OWN ray-traced viewshed code, executed here: tests/golden/viewshed_mesh_exec.npz.

Test infrastructure only, built like make_hillshade_shadow_exec.py.  The OptiX trace itself cannot run anywhere without NVIDIA
RT cores; everything around it can.  The functions below are lifted with `ast` from the reference where it lies (decorators
stripped), and RUN as plain Python on small inputs; nothing of the reference is copied, the fixture holds inputs and outputs
only:

  gpu_rtx/viewshed.py    `_generate_primary_rays_kernel`, `_generate_viewshed_rays_kernel`, `_calc_viewshed_kernel`,
                         `_get_vertical_ang` (and the constants they name) -- the three CUDA kernels run once per (i, j):
                         `nb.cuda.grid` is replaced by a stub that hands out each cell in turn
  gpu_rtx/cuda_utils.py  `float3`, `make_float3`, `add`, `diff`, `mul`, `invert`, `dot`: np.float32 tuples, as on the device

The hits handed to `_generate_viewshed_rays_kernel` are what the first trace would return for the rule's surface points
(tests/viewshed_mesh_oracle.py) at EVERY cell, the border rows and columns included: the distance to the camera and the hit
triangle's own normal, which for the mesh's winding points down (the kernel flips it).  The camera of these rays is lowered
from 10000 to twice the float32 hit height, as make_hillshade_shadow_exec.py explains: from 10000 a float32 distance is good to
6e-4 only, more than the 1e-3 offsets it is there to carry (why the rule computes the hit).
`_calc_viewshed_kernel` gets seeded hit flags (a distance of exactly 0 among them, which counts as a hit), the viewpoint and
one cell level with the observer (where the case has one) kept visible; the viewpoint's own viewshed ray is left as zeros
where it has no length (the rule traces none there); the raster goes in widened to float64 (exact): Numba
types `hmap[v] + oe` as float64 whatever the raster's dtype, plain NumPy 2 would keep a float32 sum.

Keys, per case `<k>`: `data`, `view` (row, col), `elev` (observer_elev, target_elev), `res` (ew_res, ns_res), `scale`,
`primary` (H, W, 8), `hits` (H, W, 4), `camera` (H, W, 8: the rays the second kernel reads), `vsrays` (H, W, 8: what it writes),
`flags` (H, W, 4) and `visgrid` (H, W float32).

Usage:  python tests/golden/make_viewshed_mesh_exec.py            (writes the fixture)
        python tests/golden/make_viewshed_mesh_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402
from tests.golden.make_hillshade_shadow_exec import _Grid  # noqa: E402

OUT = os.path.join(HERE, "viewshed_mesh_exec.npz")


def cases():
    """[(name, raster, (row, col), (observer_elev, target_elev), (ew_res, ns_res))]: rasters of at most 9 x 11, float32 /
    float64 / int16; viewpoints inside, in a corner, on the last row and on the last column"""
    rng = np.random.default_rng(20261019)
    yy, xx = np.mgrid[0:9, 0:11]
    hills = 40.0 * np.sin(xx / 2.3) * np.cos(yy / 1.7) + 55.0
    steps = rng.integers(1, 60, (7, 4)).astype(np.int16)
    steps[1, 1] = steps[3, 3] + 1                                    # level with the observer at (3, 3) for (2, 1): diff == 0
    return [("rough_9x11_f32", (rng.random((9, 11)) * 100 + 1).astype(np.float32), (4, 5), (5.0, 0.0), (1.0, 1.0)),
            ("hills_9x11_f64", hills + rng.normal(0, 1.5, (9, 11)), (0, 0), (0.0, 0.0), (30.0, 25.0)),
            ("rough_5x7_f64", rng.random((5, 7)) * 30 + 2, (4, 3), (2.0, 1.0), (2.0, 3.0)),
            ("steps_7x4_i16", steps, (3, 3), (2.0, 1.0), (1.0, 1.0)),
            ("plane_5x4_f32", np.full((5, 4), 1.3, np.float32), (4, 3), (0.0, 0.0), (0.5, 1.5))]


def ref_functions():
    grid = _Grid()
    names = ["float3", "make_float3", "add", "diff", "mul", "invert", "dot"]
    vec = rx.lift(os.path.join("gpu_rtx", "cuda_utils.py"), names)
    extra = {k: vec[k] for k in names}
    extra["nb"] = grid
    vs = rx.lift(os.path.join("gpu_rtx", "viewshed.py"), ["INVISIBLE", "CAMERA_HEIGHT", "_generate_primary_rays_kernel", "_get_vertical_ang",
                                                         "_calc_viewshed_kernel", "_generate_viewshed_rays_kernel"], extra)
    return grid, vs


def level_cells(data, view, elev):
    """cells other than the viewpoint that stand level with the observer (rule 6's diff == 0)"""
    z = np.asarray(data).astype(np.float64)
    level = (z[view] + elev[0]) - (z + elev[1]) == 0
    level[view] = False
    return level


def run_all():
    from tests import hillshade_shadow_oracle as ho
    from tests import viewshed_mesh_oracle as vo
    grid, vs = ref_functions()
    store = {}
    rng = np.random.default_rng(11)
    for name, data, view, elev, res in cases():
        H, W = data.shape
        scale, zv, _, _ = ho.mesh(data)
        rays = np.empty((H, W, 8), np.float32)
        grid.launch(vs["_generate_primary_rays_kernel"], H, W, rays, H, W)
        primary = rays.copy()
        # what the first trace would return for the rule's surface points: distance from the camera, the triangle's own normal
        S, n = vo.surface_points(zv)
        zh32 = S[..., 2].astype(np.float32)
        rays[..., 2] = 2 * zh32                                      # (module docstring: the camera is lowered)
        hits = np.empty((H, W, 4), np.float32)
        hits[..., 0] = zh32
        hits[..., 1:] = -n
        vsrays = np.zeros((H, W, 8), np.float32)
        vp = (view[1], view[0], elev[0] * scale, elev[1] * scale)
        for i in range(H):
            for j in range(W):
                grid.at = (i, j)
                try:
                    vs["_generate_viewshed_rays_kernel"](rays, hits, vsrays, H, W, vp)
                except ZeroDivisionError:                            # the viewpoint's own ray without an observer height has no
                    assert (i, j) == view and elev[0] == 0           # length: CUDA divides to inf, Python raises.  Left as zeros
                    vsrays[i, j] = 0
        # rule 6 on seeded hit flags
        flags = np.zeros((H, W, 4), np.float32)
        flags[..., 0] = np.where(rng.random((H, W)) < 0.6, -1.0, rng.random((H, W)) * 50)
        flags[..., 0][level_cells(data, view, elev)] = -1.0
        flags[0, 1, 0] = 0.0                                         # a distance of exactly 0 counts as a hit (`>= 0`)
        flags[view][0] = -1.0
        visgrid = np.full((H, W), np.nan, np.float32)
        grid.launch(vs["_calc_viewshed_kernel"], H, W, flags, visgrid, H, W, np.asarray(data).astype(np.float64), (view[0], view[1]), elev[0],
                    elev[1], res[0], res[1])
        for key, value in (("data", data), ("view", np.array(view, np.int64)), ("elev", np.array(elev, np.float64)),
                           ("res", np.array(res, np.float64)), ("scale", np.float64(scale)), ("primary", primary), ("hits", hits),
                           ("camera", rays), ("vsrays", vsrays), ("flags", flags), ("visgrid", visgrid)):
            store[f"{name}/{key}"] = np.asarray(value)
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def names(store):
    return sorted({k.split("/")[0] for k in store})


def check():
    want = load()
    got = run_all()
    bad = sorted(set(want) ^ set(got))
    for k in set(want) & set(got):
        a, b = want[k], got[k]
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            bad.append(k)
    for k in sorted(bad)[:20]:
        print("MISMATCH", k)
    return not bad


if __name__ == "__main__":
    if not rx.have_reference():
        sys.exit("the reference is not present here")
    if sys.argv[1:] == ["--check"]:
        ok = check()
        print("viewshed_mesh_exec.npz reproduces" if ok else "viewshed_mesh_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")

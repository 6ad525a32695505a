"""Outputs of the reference's OWN ray-traced hillshade code, executed here: tests/golden/hillshade_shadow_exec.npz.

Test infrastructure only, built like make_viewshed_exec.py.  The OptiX trace itself cannot run anywhere without NVIDIA RT
cores; everything around it can.  The functions below are lifted with `ast` from the reference where it lies (decorators
stripped), and RUN as plain Python on small seeded inputs; nothing of the reference is copied, the fixture holds inputs and
outputs only:

  gpu_rtx/hillshade.py   `_get_sun_dir` (scipy's rotations), `_generate_primary_rays_kernel`, `_generate_shadow_rays_kernel`,
                         `_shade_lambert_kernel` -- the three CUDA kernels run once per (i, j): `nb.cuda.grid` is replaced by
                         a stub that hands out each cell in turn
  gpu_rtx/mesh_utils.py  `_triangulate_cpu` (`nb.prange` = range): the vertex and index buffers
  gpu_rtx/cuda_utils.py  `float3`, `make_float3`, `add`, `mul`, `invert`, `dot`: np.float32 tuples, as on the device

The hits handed to `_generate_shadow_rays_kernel` are what the first trace would return for the rule's camera hit
(tests/hillshade_shadow_oracle.py): the distance to the camera and the hit triangle's own normal, which for the mesh's
winding points down (the kernel flips it).  The camera of these rays is lowered from 10000 to twice the float32 hit height, so
that the kernel's float32 `origin + direction * distance` returns the hit height exactly: from 10000 a float32 distance is
good to 2^-24 * 10000 = 6e-4 only, more than the 1e-3 offsets it is there to carry (why the rule computes the hit).
`_shade_lambert_kernel` gets seeded unit normals and hit flags, with both values of `cast_shadows`; two normals are too long
on purpose, so that both clamps are taken.  The unit normals lie within 90 degrees of the sun: the kernel's float32
`(cos_theta + 1) / 2` carries 2^-24 of 1 absolutely, which is the 1e-6 relative of tests/test_hillshade_shadow_host.py only
where the shade is not close to 0.

Keys: `sun/args` (n, 2: altitude, azimuth) and `sun/out` (n, 3); per raster `<k>/data`, `<k>/scale`, `<k>/verts`,
`<k>/triangles`, `<k>/primary` (H, W, 8), `<k>/sun`, `<k>/hits` (H, W, 4), `<k>/shadow_in` and `<k>/shadow_rays` (H, W, 8: the
kernel's rays before and after), `<k>/normals` (H, W, 3), `<k>/shade_normals`, `<k>/shade_hits`, `<k>/shade_plain`,
`<k>/shade_cast` (H, W).

Usage:  python tests/golden/make_hillshade_shadow_exec.py            (writes the fixture)
        python tests/golden/make_hillshade_shadow_exec.py --check    (exit 1 unless it equals what the reference computes today)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_reference_exec as rx  # noqa: E402

OUT = os.path.join(HERE, "hillshade_shadow_exec.npz")
SUNS = [(25, 225), (5, 90), (60, 0), (-10, 135), (90, 45)]           # (altitude, azimuth), the order `_get_sun_dir` takes


def cases():
    """[(name, raster, (altitude, azimuth))]: a few rasters of at most 9 x 11, float32 / float64 / int16"""
    rng = np.random.default_rng(20261019)
    yy, xx = np.mgrid[0:9, 0:11]
    hills = 40.0 * np.sin(xx / 2.3) * np.cos(yy / 1.7) + 55.0
    return [("rough_9x11_f32", (rng.random((9, 11)) * 100 + 1).astype(np.float32), SUNS[0]),
            ("hills_9x11_f64", hills + rng.normal(0, 1.5, (9, 11)), SUNS[1]),
            ("rough_5x7_f64", rng.random((5, 7)) * 30 + 2, SUNS[2]),
            ("steps_7x4_i16", rng.integers(1, 60, (7, 4)).astype(np.int16), SUNS[3]),
            ("rough_3x3_f32", (rng.random((3, 3)) * 9 + 1).astype(np.float32), SUNS[4])]


class _Grid:
    """stand-in for `nb`: `nb.cuda.grid(2)` gives the cell the driver is at, `nb.prange` is range"""

    def __init__(self):
        self.at = (0, 0)
        self.cuda = types.SimpleNamespace(grid=lambda ndim: self.at)
        self.prange = range

    def launch(self, kernel, H, W, *args):
        for i in range(H):
            for j in range(W):
                self.at = (i, j)
                kernel(*args)


def ref_functions():
    from scipy.spatial.transform import Rotation as R
    grid = _Grid()
    vec = rx.lift(os.path.join("gpu_rtx", "cuda_utils.py"), ["float3", "make_float3", "add", "mul", "invert", "dot"])
    extra = {k: vec[k] for k in ("float3", "make_float3", "add", "mul", "invert", "dot")}
    extra.update(nb=grid, R=R)
    hs = rx.lift(os.path.join("gpu_rtx", "hillshade.py"), ["_get_sun_dir", "_generate_primary_rays_kernel", "_generate_shadow_rays_kernel",
                                                          "_shade_lambert_kernel"], extra)
    mesh = rx.lift(os.path.join("gpu_rtx", "mesh_utils.py"), ["_triangulate_cpu"], {"nb": grid})
    return grid, hs, mesh


def run_all():
    from tests import hillshade_shadow_oracle as ho
    grid, hs, mesh = ref_functions()
    store = {"sun/args": np.array(SUNS, np.float64),
             "sun/out": np.array([hs["_get_sun_dir"](alt, az) for alt, az in SUNS], np.float64)}
    rng = np.random.default_rng(7)
    for name, data, (alt, az) in cases():
        H, W = data.shape
        scale = max(H, W) / float(data.max())                        # mesh_utils.py:17-19
        verts = np.empty(H * W * 3, np.float32)
        triangles = np.empty((H - 1) * (W - 1) * 6, np.int32)
        # float32 cells are widened first (exact): Numba types `val * scale` as float32 * float64 -> float64, plain NumPy 2
        # would keep a float32 product (make_reference_exec.py, "what is deliberately NOT executed")
        mesh["_triangulate_cpu"](verts, triangles, data.astype(np.float64) if data.dtype == np.float32 else data, H, W, scale)
        rays = np.empty((H, W, 8), np.float32)
        grid.launch(hs["_generate_primary_rays_kernel"], H, W, rays, H, W)
        primary = rays.copy()
        # what the first trace would return for the rule's camera hit: distance from the camera, the triangle's own normal
        hit = ho.camera_hits(verts.reshape(H, W, 3)[..., 2])
        inner = ~np.isnan(hit["zh"])
        zh32 = np.where(inner, hit["zh"], 0.0).astype(np.float32)
        rays[..., 2] = np.where(inner, 2 * zh32, rays[..., 2])       # (module docstring: the camera is lowered)
        hits = np.full((H, W, 4), -1.0, np.float32)
        hits[..., 0] = np.where(inner, zh32, -1.0)
        hits[..., 1:] = np.where(inner[..., None], -hit["n"], 0.0)
        shadow_in = rays.copy()
        sun = np.asarray(hs["_get_sun_dir"](alt, az), np.float64)
        normals = np.zeros((H, W, 3), np.float32)
        grid.launch(hs["_generate_shadow_rays_kernel"], H, W, rays, hits, normals, H, W, sun)
        # Lambert on seeded unit normals and hit flags
        nrm = rng.normal(0, 1, (H, W, 3))
        nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
        nrm = np.where((nrm @ sun < 0)[..., None], -nrm, nrm).astype(np.float32)       # (module docstring: within 90 degrees of the sun)
        flags = np.where(rng.random((H, W)) < 0.5, -1.0, rng.random((H, W)) * 50).astype(np.float32)
        flags[0, 0] = 0.0                                            # a distance of exactly 0 counts as a hit (`>= 0`)
        nrm[0, 1], flags[0, 1] = (-3 * sun).astype(np.float32), -1.0      # (1 - 3) / 2 < 0
        nrm[1, 1], flags[1, 1] = (5 * sun).astype(np.float32), 1.0        # (1 + 5) / 2 / 2 > 1
        shade_hits = np.zeros((H, W, 4), np.float32)
        shade_hits[..., 0] = flags
        shade = []
        for cast in (False, True):
            out = np.full((H, W), np.nan, np.float32)
            grid.launch(hs["_shade_lambert_kernel"], H, W, shade_hits, nrm, out, H, W, sun, cast)
            shade.append(out)
        for key, value in (("data", data), ("scale", np.float64(scale)), ("verts", verts), ("triangles", triangles), ("primary", primary),
                           ("sun", sun), ("hits", hits), ("shadow_in", shadow_in), ("shadow_rays", rays), ("normals", normals),
                           ("shade_normals", nrm), ("shade_hits", shade_hits), ("shade_plain", shade[0]), ("shade_cast", shade[1])):
            store[f"{name}/{key}"] = np.asarray(value)
    return store


def load(path=OUT):
    z = np.load(path, allow_pickle=False)
    return {k: z[k] for k in z.files}


def names(store):
    return sorted({k.split("/")[0] for k in store} - {"sun"})


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
        print("hillshade_shadow_exec.npz reproduces" if ok else "hillshade_shadow_exec.npz differs")
        sys.exit(0 if ok else 1)
    st = run_all()
    np.savez_compressed(OUT, **st)
    print(f"wrote {OUT}: {len(st)} arrays, {os.path.getsize(OUT)} bytes")

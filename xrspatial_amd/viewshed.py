"""viewshed: the cells of a raster that are seen from one observer.  Reference: xrspatial/viewshed.py, its CPU path.

The reference sweeps a line around the viewpoint over 3 (N - 1) sorted events and keeps the cells the line crosses in a
red-black tree; what it computes per cell is a predicate of that cell and the raster alone, and csrc/viewshed.hip
evaluates it with one ray walk per cell.  Visible cells hold the vertical angle in degrees (0 straight below the observer,
90 level, towards 180 above), invisible ones -1, the viewpoint 180; the result is float64.

What the host adds is the reference's lookup of the viewpoint: the coordinate nearest to `x` / `y` (of two equally near ones the
larger, as `raster.sel(..., method='nearest')` picks), then the first index holding that value, and the two resolutions
(last - first coordinate) / (cells - 1).  The raster's values never cross to the host: the kernel reads the viewpoint's
elevation itself.  float32 and float64 rasters are read in place, every other dtype is converted to float64 first.

Two departures from the reference, both on purpose: the input is not overwritten with a float64 copy, and NaN cells follow
the predicate (never visible, never hiding a cell) where the reference's sweep raises ValueError('node not found') for some
NaN layouts.  There is no CPU fallback; dask- and ShardedArray-backed rasters raise NotImplementedError.

`method='mesh'` (and `viewshed_mesh`, the reference's `viewshed_gpu` signature) is the reference's OTHER viewshed, the one a CuPy
raster gets (gpu_rtx/viewshed.py: one ray per cell traced through OptiX over the triangle mesh of gpu_rtx/mesh_utils.py), as a
rule evaluated by csrc/viewshed_mesh.hip with one bounded ray walk per cell.  Float64 unless marked; only
+ - * /, sqrt, atan and comparisons, every sum left to right:
  1 mesh      hillshade's rule 2: scale = max(H, W) / max of the raster, zv = (float32)((double)value * scale), T0 and T1 per cell.
  2 surface   every cell (i, j): x0 = (double)(float)(j + 1e-3), (j - 1e-3) when j == W - 1, y0 likewise; the point lies in cell
              (min(i, H - 2), min(j, W - 2)) at fx, fy = x0 - cj, y0 - ci; from there hillshade's rule 3 (T0 when fy >= fx, the
              gradient, zh, the unit normal n with n_z > 0).  S(i, j) = (x0, y0, zh).  Computed, not traced.
  3 observer  P = S(viewpoint) + (0, 0, observer_elev * scale).
  4 ray       origin S + n * 1e-3 + (0, 0, target_elev * scale); d = P - S (from S, not from the origin); L = sqrt(d . d);
              direction d * (1 / L).
  5 verdict   invisible iff some triangle of the mesh is hit, Moller-Trumbore in hillshade's rule 4 order, accepted iff
              det != 0, u >= 0, v >= 0, u + v <= 1, 0 <= t <= L.  The viewpoint is 180 without a ray.
  6 value     -1 where invisible; else with diff = (z[v] + observer_elev) - (z[t] + target_elev) on the UNSCALED raster and
              dist = sqrt(dx^2 + dy^2), dx = (vc - j) ew_res, dy = (vr - i) ns_res: 90 if diff == 0, atan(dist / diff) 180 / pi if
              diff > 0, else atan(-diff / dist) 180 / pi + 90; stored as float32.  The mesh is in index space: the resolutions
              move the angles, never the verdicts (reproduced as found).
Departures: the camera hit is computed; the viewpoint gets no ray (the reference traces a zero-length one); the rays are float64
on float32 vertices (single cells on an occluder's silhouette may differ from an RTX run, which nothing here can execute); a
non-finite cell or a maximum <= 0 raises ValueError before any device walk, as hillshade(shadows=True) does.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, resident, settle, workspace
from ._xr import DataArray
from .device import FLOAT_SUFFIX, DeviceArray

OBS_ELEV = 0
TARGET_ELEV = 0
INVISIBLE = -1


# ------------------------------------------------------------------ argument checks and the viewpoint (before any device work)
def check_raster(raster):
    if len(raster.shape) != 2:
        raise ValueError(f"viewshed: a 2-D raster is needed, got {len(raster.shape)} dimensions")
    if min(raster.shape) < 2:
        raise ValueError(f"viewshed: at least two cells along each dimension are needed, got {tuple(raster.shape)}")


def nearest_index(coords, v, axis):
    """Index of the cell whose coordinate is nearest to `v`, as the reference finds it (viewshed.py:1518-1533)."""
    coords = np.asarray(coords)
    if not (coords.min() <= v <= coords.max()):
        raise ValueError(f"{axis} argument outside of raster {axis}_range")
    dist = np.abs(coords.astype(np.float64) - float(v))
    value = coords[dist == dist.min()].max()                 # pandas' `nearest`: of two equally near labels the larger
    return int(np.where(coords == value)[0][0])


def viewpoint(raster, x, y):
    """(row, col, ew_res, ns_res) of the observer at data-space (x, y): viewshed.py:1513-1546"""
    ydim, xdim = raster.dims[-2], raster.dims[-1]
    x_coords, y_coords = np.asarray(raster[xdim].data), np.asarray(raster[ydim].data)
    height, width = raster.shape
    if x_coords.shape != (width,) or y_coords.shape != (height,):
        raise ValueError("viewshed: one coordinate per column and per row is needed")
    col = nearest_index(x_coords, x, "x")
    row = nearest_index(y_coords, y, "y")
    ew_res = float(x_coords[-1] - x_coords[0]) / (width - 1)
    ns_res = float(y_coords[-1] - y_coords[0]) / (height - 1)
    return row, col, ew_res, ns_res


# ------------------------------------------------------------------ the launch
def _run(data, row, col, observer_elev, target_elev, ew_res, ns_res):
    """A NumPy raster gets NumPy back, a DeviceArray a DeviceArray."""
    _lib.require_device()
    stream = get_stream()
    src, like_numpy = resident(data, stream, FLOAT_SUFFIX, np.float64)      # integers, bool, float16: float64, as the reference casts
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float64)
    work = workspace("viewshed", rows, cols)
    _lib.call("xrs_viewshed_" + FLOAT_SUFFIX[src.dtype], src.ptr, rows, cols, row, col, float(observer_elev), float(target_elev),
              float(ew_res), float(ns_res), work.ptr, out.ptr, stream)
    settle(stream, like_numpy)
    return finish(out, like_numpy)


def _run_mesh(data, row, col, observer_elev, target_elev, ew_res, ns_res):
    """method='mesh': a NumPy raster gets NumPy back, a DeviceArray a DeviceArray; float32 either way."""
    from .hillshade import mesh_source
    like_numpy = isinstance(data, np.ndarray)
    rows, cols = data.shape
    stream = get_stream()
    src, scale, zmin, zmax = mesh_source(data, stream, "viewshed(method='mesh')")
    if not (np.isfinite(observer_elev * scale) and np.isfinite(target_elev * scale)):
        raise ValueError("viewshed(method='mesh'): observer_elev and target_elev overflow the mesh's height scale")
    out = DeviceArray((rows, cols), np.float32)
    work = workspace("viewshed_mesh", rows, cols)
    _lib.call("xrs_viewshed_mesh_" + FLOAT_SUFFIX[src.dtype], src.ptr, rows, cols, scale, zmin, zmax, row, col,
              float(observer_elev), float(target_elev), float(ew_res), float(ns_res), work.ptr, out.ptr, stream)
    settle(stream, like_numpy)
    return finish(out, like_numpy)


def viewshed_mesh(raster, x, y, observer_elev, target_elev):
    """`viewshed(..., method='mesh')` under the signature of the reference's `xrspatial.gpu_rtx.viewshed.viewshed_gpu`."""
    return viewshed(raster, x, y, observer_elev, target_elev, method="mesh")


def viewshed(raster, x, y, observer_elev=OBS_ELEV, target_elev=TARGET_ELEV, method="sweep"):
    """The cells of `raster` visible from the observer at data-space (x, y).

    raster: 2-D DataArray of elevations, at least 2 x 2, NumPy- or DeviceArray-backed (the result's backend).  x, y: the
    observer's position, inside the raster's coordinate ranges; the nearest cell is the viewpoint.  observer_elev: the
    observer's height above that cell.  target_elev: height added to every cell when it is looked at (not when it hides
    another).  Returns a float64 DataArray with raster's dims, coords and attrs: 180 at the viewpoint, -1 where invisible,
    else the vertical angle in degrees.  Same signature and results as `xrspatial.viewshed` (CPU path); `raster` is left
    as it is.

    method: 'sweep' (the default) is the above.  'mesh' gives what the reference computes for a CuPy raster instead (its
    ray-traced `viewshed_gpu`; the rule is in this module's docstring): line of sight over the raster's triangle mesh, float32,
    named 'viewshed', for rasters without non-finite cells and with a positive maximum."""
    if method not in ("sweep", "mesh"):
        raise ValueError(f"viewshed: method must be 'sweep' or 'mesh', got {method!r}")
    check_raster(raster)
    observer_elev, target_elev = float(observer_elev), float(target_elev)
    if not (np.isfinite(observer_elev) and np.isfinite(target_elev)):
        raise ValueError("viewshed: observer_elev and target_elev must be finite")
    row, col, ew_res, ns_res = viewpoint(raster, x, y)
    if not (np.isfinite(ew_res) and np.isfinite(ns_res)):
        raise ValueError("viewshed: the raster's coordinates are not finite")
    run = _run_mesh if method == "mesh" else _run
    refuse_split_backends(raster, 'viewshed')
    out = run(raster.data, row, col, observer_elev, target_elev, ew_res, ns_res)
    if method == "mesh":
        return DataArray(out, name="viewshed", coords=raster.coords, dims=raster.dims, attrs=raster.attrs)
    return DataArray(out, coords=raster.coords, dims=raster.dims, attrs=raster.attrs)

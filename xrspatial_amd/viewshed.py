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
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._launch import finish, get_stream
from ._xr import DataArray
from .device import DeviceArray
from .utils import ArrayTypeFunctionMapping, not_implemented_func

OBS_ELEV = 0
TARGET_ELEV = 0
INVISIBLE = -1
_SUFFIX = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}


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
    like_numpy = isinstance(data, np.ndarray)
    stream = get_stream()
    if np.dtype(data.dtype) not in _SUFFIX:                  # integers, bool, float16: float64, as the reference casts
        data = (data if like_numpy else data.get(stream)).astype(np.float64)
    src = DeviceArray.from_numpy(data, stream=stream) if isinstance(data, np.ndarray) else data
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float64)
    work = DeviceArray((int(_lib.load().xrs_viewshed_workspace_bytes(rows, cols)),), np.uint8)
    _lib.call("xrs_viewshed_" + _SUFFIX[src.dtype], src.ptr, rows, cols, row, col, float(observer_elev), float(target_elev),
              float(ew_res), float(ns_res), work.ptr, out.ptr, stream)
    if not like_numpy:
        _lib.call("xrs_stream_sync", stream)                 # the workspace goes back to the pool when this returns
    return finish(out, like_numpy)


def viewshed(raster, x, y, observer_elev=OBS_ELEV, target_elev=TARGET_ELEV):
    """The cells of `raster` visible from the observer at data-space (x, y).

    raster: 2-D DataArray of elevations, at least 2 x 2, NumPy- or DeviceArray-backed (the result's backend).  x, y: the
    observer's position, inside the raster's coordinate ranges; the nearest cell is the viewpoint.  observer_elev: the
    observer's height above that cell.  target_elev: height added to every cell when it is looked at (not when it hides
    another).  Returns a float64 DataArray with raster's dims, coords and attrs: 180 at the viewpoint, -1 where invisible,
    else the vertical angle in degrees.  Same signature and results as `xrspatial.viewshed` (CPU path); `raster` is left
    as it is."""
    check_raster(raster)
    observer_elev, target_elev = float(observer_elev), float(target_elev)
    if not (np.isfinite(observer_elev) and np.isfinite(target_elev)):
        raise ValueError("viewshed: observer_elev and target_elev must be finite")
    row, col, ew_res, ns_res = viewpoint(raster, x, y)
    if not (np.isfinite(ew_res) and np.isfinite(ns_res)):
        raise ValueError("viewshed: the raster's coordinates are not finite")
    mapper = ArrayTypeFunctionMapping(
        numpy_func=_run, hip_func=_run,
        sharded_func=lambda *args: not_implemented_func(
            *args, messages='viewshed() does not support row-sharded (multi-GPU) DataArray'),
        dask_func=lambda *args: not_implemented_func(*args, messages='viewshed() does not support dask backed DataArray'))
    out = mapper(raster)(raster.data, row, col, observer_elev, target_elev, ew_res, ns_res)
    return DataArray(out, coords=raster.coords, dims=raster.dims, attrs=raster.attrs)

"""a_star_search: the shortest path between two points over the crossable cells of a raster.  Reference:
xrspatial/pathfinding.py.

The reference runs A* with a Euclidean heuristic, and every pop of its open list scans the whole raster.  The heuristic is
admissible, so what it returns is a shortest path.  This backend computes the shortest-distance field of the grid graph from the
goal and walks along it once from the start (csrc/pathfinding.hip), by this rule:

  1. a cell is crossable when it is not NaN and equals none of `barriers` under NumPy's `==` (compared as `proximity` compares
     `target_values`: integers with an integer raster as integers, everything else as float64); +-inf is crossable;
  2. D(c) = (a, b) is the exact shortest distance from the goal to the crossable cell c over 4- or 8-connected crossable cells:
     a steps of 1.0 along rows and columns and b diagonal steps of sqrt(2) (8-connectivity only), kept and compared as integers;
  3. if the start or the goal is not crossable, or the start cannot be reached, every cell of the result is NaN;
  4. otherwise the path goes from the start, at every cell to the first neighbour n, in the order of the reference's
     `_neighborhood_structure`, with D(n) + step == D(cell) exactly; it takes a + b steps; the start holds 0.0, every further
     cell of the path the float64 running sum g = g + (1.0 or 1.4142135623730951) in walk order (the arithmetic of the
     reference's `d_from_start`), every other cell NaN; the result is float64 whatever the raster's dtype;
  5. `snap_start` / `snap_goal` follow `_find_nearest_pixel`: a crossable cell is kept; otherwise the crossable cell with the
     smallest squared pixel distance, the first in row-major order among equals, and only if that is strictly below
     (rows - 1)**2 + (cols - 1)**2; if there is none the result is all NaN;
  6. "Start at a non crossable location" / "End at a non crossable location" are warned as the reference warns, after snapping.

The rule always gives a shortest path.  Where the shortest path is unique it gives the reference's own image bit for bit.
Elsewhere it gives one of the equally short paths, the one fixed by (4), with the goal's cost within rounding of the
reference's (the same a ones and b sqrt(2)s, added in another order); the reference's choice among equally short paths
follows the order of its pops and is not reproduced.

Every dtype the kernels read (the ten XRS_DT_* codes) is read in place; bool and float16 rasters are widened on the host first.
The warnings come from the call's status words, so no raster value crosses to the host.  There is no CPU fallback; dask- and
ShardedArray-backed surfaces raise NotImplementedError.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import Optional, Union

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, resident, widened, workspace
from ._xr import DataArray
from .device import DTYPE_CODE, DeviceArray
from .proximity import target_array, widen
from .utils import get_dataarray_resolution

SNAP_START, SNAP_GOAL, NO_WALK, GROUP_SHIFT = 1, 2, 4, 8                 # XRS_ASTAR_*: bits of `snap_flags`
START_CROSSABLE, GOAL_CROSSABLE, PATH_FOUND = 1, 2, 4                    # XRS_ASTAR_*: bits of the status flags


def _get_pixel_id(point, raster, xdim=None, ydim=None):
    """(row, column) of the (y, x) coordinate pair `point`, as the reference's `_get_pixel_id`."""
    if ydim is None:
        ydim = raster.dims[-2]
    if xdim is None:
        xdim = raster.dims[-1]
    y_coords = np.asarray(raster[ydim].data)
    x_coords = np.asarray(raster[xdim].data)
    cellsize_x, cellsize_y = get_dataarray_resolution(raster, xdim, ydim)
    py = int(abs(point[0] - y_coords[0]) / cellsize_y)
    px = int(abs(point[1] - x_coords[0]) / cellsize_x)
    return py, px


def _is_inside(py, px, h, w):
    return 0 <= px < w and 0 <= py < h


def search(data, start, goal, barriers, connectivity, snap_flags=0, walk=True, group=0):
    """One xrs_astar call: (float64 path image on the device, the 8 status words).  `data`: NumPy raster or DeviceArray."""
    _lib.require_device()
    stream = get_stream()
    data = widened(data, stream, DTYPE_CODE, widen("a_star_search"))
    values, kind = target_array(barriers, data.dtype)                    # (its TypeError comes before the upload)
    src, _ = resident(data, stream)
    rows, cols = src.shape
    work = workspace("astar", rows, cols, at_least=1)                    # (a raster beyond 2^30 cells is refused by the call)
    out = DeviceArray((rows, cols), np.float64)
    vals = DeviceArray.from_numpy(values.view(np.float64), stream=stream) if values.size else None
    status = (ctypes.c_int64 * 8)()
    flags = snap_flags | (0 if walk else NO_WALK) | (group << GROUP_SHIFT)
    _lib.call("xrs_astar", src.ptr, DTYPE_CODE[src.dtype], rows, cols, start[0], start[1], goal[0], goal[1],
              vals.ptr if vals is not None else None, kind, int(values.size), connectivity, flags, work.ptr, out.ptr, status, stream)
    return out, [int(v) for v in status]                                 # (the call has waited for the stream)


def _run(data, start, goal, barriers, connectivity, snap_flags):
    """A NumPy raster gets NumPy back, a DeviceArray a DeviceArray."""
    out, status = search(data, start, goal, barriers, connectivity, snap_flags)
    if not status[4] & START_CROSSABLE:
        warnings.warn("Start at a non crossable location", Warning)
    if not status[4] & GOAL_CROSSABLE:
        warnings.warn("End at a non crossable location", Warning)
    return finish(out, isinstance(data, np.ndarray))


def a_star_search(surface: DataArray,
                  start: Union[tuple, list, np.array],
                  goal: Union[tuple, list, np.array],
                  barriers: list = [],
                  x: Optional[str] = 'x',
                  y: Optional[str] = 'y',
                  connectivity: int = 8,
                  snap_start: bool = False,
                  snap_goal: bool = False) -> DataArray:
    """The shortest path from `start` to `goal` over the crossable cells of `surface`.

    surface: 2-D DataArray with dims (y, x); NumPy- or DeviceArray-backed (the result's backend).  start, goal: (y, x)
    coordinate pairs inside the raster.  barriers: the cell values that cannot be crossed; NaN cells never can.  connectivity:
    4 or 8; steps cost 1.0 along rows and columns and sqrt(2) diagonally.  snap_start / snap_goal: move a start / goal that is
    not crossable to the nearest crossable cell first.  Returns a float64 DataArray with surface's coords, dims and attrs: 0.0
    at the start, the cost so far at every further cell of the path, NaN everywhere else; all NaN when there is no path.  Same
    signature as `xrspatial.a_star_search`; the path is a shortest one and equals the reference's wherever the shortest path is
    unique (module docstring)."""
    if surface.ndim != 2:
        raise ValueError("input `surface` must be 2D")
    if tuple(surface.dims) != (y, x):
        raise ValueError("`surface.coords` should be named as coordinates:"
                         "({}, {})".format(y, x))
    if connectivity != 4 and connectivity != 8:
        raise ValueError("Use either 4 or 8-connectivity.")
    refuse_split_backends(surface, 'a_star_search')

    start_py, start_px = _get_pixel_id(start, surface, x, y)
    goal_py, goal_px = _get_pixel_id(goal, surface, x, y)
    h, w = surface.shape
    if not _is_inside(start_py, start_px, h, w):
        raise ValueError("start location outside the surface graph.")
    if not _is_inside(goal_py, goal_px, h, w):
        raise ValueError("goal location outside the surface graph.")

    snap_flags = (SNAP_START if snap_start else 0) | (SNAP_GOAL if snap_goal else 0)
    out = _run(surface.data, (start_py, start_px), (goal_py, goal_px), np.array(barriers), connectivity, snap_flags)
    return DataArray(out, coords=surface.coords, dims=surface.dims, attrs=surface.attrs)

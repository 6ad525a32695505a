"""flow_direction, flow_accumulation, basins: D8 hydrology.  The reference (0.5.3) has no hydrology code, so the result is a
written rule (csrc/hydrology.hip; stated in NumPy by tests/hydrology_oracle.py), and every output is an integer
code or a count: the tests compare bit for bit.

flow_direction.  ESRI's codes, the neighbours (drow, dcol) in this fixed order: E 1 (0, +1), SE 2 (+1, +1), S 4 (+1, 0),
SW 8 (+1, -1), W 16 (0, -1), NW 32 (-1, -1), N 64 (-1, 0), NE 128 (-1, +1).
  1. cx, cy = |get_dataarray_resolution(agg)| as float64; the host computes dg = np.sqrt(cx * cx + cy * cy);
  2. a neighbour's distance is cx (E, W), cy (N, S) or dg (the diagonals);
  3. drop_k = (float64(z) - float64(zk)) / dist_k: one IEEE subtraction, one IEEE division;
  4. best = 0.0, code = 0; in the order above neighbour k is taken only if drop_k > best (strict, false on NaN): ties keep the
     earlier neighbour; a NaN neighbour, one outside the raster and inf - inf are never taken; a flat, a pit and an edge cell
     with no lower neighbour get 0;
  5. a NaN cell gives NaN.  The result is float32.
float32 and float64 rasters are read in place; every other numeric dtype is cast to float64 on the host.

flow_accumulation, basins.  The input is a raster of such codes, staged as float32.
  1. a NaN cell is outside the graph: both results are NaN there;
  2. any other value that is not one of 0, 1, 2, 4, 8, 16, 32, 64, 128 raises ValueError (found on the device, raised before a
     result is returned);
  3. the downstream cell of u is the neighbour its code names; a code 0, a neighbour outside the raster or a NaN neighbour make
     u an outlet;
  4. flow_accumulation[v] = the number of non-NaN cells whose path reaches v, v included (float64, exact below 2^32);
  5. basins[v] = row * W + col of the outlet v's path ends in (float64);
  6. a raster from flow_direction descends strictly and holds no cycle; a user's raster can: a pointer that is still live after
     (H * W).bit_length() doubling rounds lies on or above a cycle, and the call raises ValueError;
  7. more than 2^32 - 2 cells raise ValueError (the all-ones word is the null pointer).

Flow paths cross chunks and shards: dask- and ShardedArray-backed rasters raise NotImplementedError.  Inside a `fuse()` scope
the calls run eagerly.  There is no CPU fallback.  Weighted accumulation, flow length and watersheds from given pour points
are not built.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, resident, settle, workspace
from ._xr import DataArray
from .dataset_support import supports_dataset
from .device import DTYPE_CODE, FLOAT_SUFFIX, DeviceArray, to_device_f32
from .utils import get_dataarray_resolution

ACCUMULATION, BASINS = 1, 2             # XRS_FLOW_ACCUMULATION / XRS_FLOW_BASINS
INVALID_CODE, CYCLE = 1, 2              # XRS_FLOW_INVALID_CODE / XRS_FLOW_CYCLE (status word 1)
TIMED = 1                               # XRS_FLOW_TIMED
STATUS_WORDS = 80
MAX_CELLS = 2 ** 32 - 2
CODES = (0, 1, 2, 4, 8, 16, 32, 64, 128)


def _check_raster(data, what):
    if len(data.shape) != 2:
        raise ValueError(f"{what}: expected a 2D raster, got shape {tuple(data.shape)}")
    if np.dtype(data.dtype).kind not in "iufb":
        raise TypeError(f"{what}: unsupported raster dtype {data.dtype}")
    rows, cols = (int(s) for s in data.shape)
    if rows * cols > MAX_CELLS:
        raise ValueError(f"{what}: more than 2**32 - 2 cells ({rows} x {cols})")
    return rows, cols


def cell_distances(agg):
    """(cx, cy, dg) of rule 1, as float64."""
    cellsize_x, cellsize_y = get_dataarray_resolution(agg)
    cx, cy = np.abs(np.float64(cellsize_x)), np.abs(np.float64(cellsize_y))
    with np.errstate(over='ignore', under='ignore'):
        dg = np.sqrt(cx * cx + cy * cy)
    if not (np.isfinite(cx) and np.isfinite(cy) and np.isfinite(dg) and cx > 0 and cy > 0 and dg > 0):
        raise ValueError(f"flow_direction: cell sizes must be positive and finite, and so their diagonal, got ({cellsize_x}, {cellsize_y})")
    return float(cx), float(cy), float(dg)


# ------------------------------------------------------------------ flow_direction
def _run_direction(data, cx, cy, dg):
    _lib.require_device()
    stream = get_stream()
    src, like_numpy = resident(data, stream, FLOAT_SUFFIX, np.float64)
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float32)
    if rows * cols:
        _lib.call("xrs_flow_direction", src.ptr, DTYPE_CODE[src.dtype], rows, cols, cx, cy, dg, out.ptr, stream)
        if src is not data:
            settle(stream, like_numpy)                                   # the widened copy goes back to the pool
    return finish(out, like_numpy)


@supports_dataset
def flow_direction(agg: DataArray, name: str = 'flow_direction') -> DataArray:
    """D8 flow direction: for every cell the ESRI code (E 1, SE 2, S 4, SW 8, W 16, NW 32, N 64, NE 128) of the neighbour with
    the steepest drop, 0 where no neighbour lies lower, NaN at NaN cells (the rule: module docstring).

    agg: 2-D DataArray of elevations (or a Dataset: every variable on its own), NumPy- or DeviceArray-backed (the result's
    backend); the cell size comes from `attrs['res']` or the coordinates, as for `slope`.  Returns a float32 DataArray with
    agg's coords, dims and attrs."""
    refuse_split_backends(agg, 'flow_direction')
    rows, cols = _check_raster(agg.data, 'flow_direction')
    cx, cy, dg = cell_distances(agg) if rows * cols else (1.0, 1.0, float(np.sqrt(2.0)))
    out = _run_direction(agg.data, cx, cy, dg)
    return DataArray(out, name=name, coords=agg.coords, dims=agg.dims, attrs=agg.attrs)


# ------------------------------------------------------------------ flow_accumulation, basins
def flow_graph(src: DeviceArray, want: int, flags: int = 0, stream=None):
    """xrs_flow_accumulate on a resident float32 plane of codes: (accumulation or None, basins or None, status words).
    Raises ValueError for an invalid code or a cycle."""
    rows, cols = src.shape
    acc = DeviceArray((rows, cols), np.float64) if want & ACCUMULATION else None
    basin = DeviceArray((rows, cols), np.float64) if want & BASINS else None
    status = (ctypes.c_int64 * STATUS_WORDS)()
    if rows * cols:
        work = workspace("flow", rows, cols, want)
        _lib.call("xrs_flow_accumulate", src.ptr, rows, cols, work.ptr, acc.ptr if acc else None, basin.ptr if basin else None,
                  status, flags, stream)
        settle(stream)
    words = [int(w) for w in status]
    if words[1] & INVALID_CODE:
        raise ValueError("flow direction raster holds a value that is not one of the D8 codes 0, 1, 2, 4, 8, 16, 32, 64, 128")
    if words[1] & CYCLE:
        raise ValueError(f"flow direction raster contains a cycle (pointers still live after {words[0]} doubling rounds)")
    return acc, basin, words


def _run_graph(data, want):
    _lib.require_device()
    like_numpy = isinstance(data, np.ndarray)
    src = to_device_f32(data)
    acc, basin, _ = flow_graph(src, want, stream=get_stream())
    return finish(acc if want == ACCUMULATION else basin, like_numpy)


def _graph_product(flow_dir, name, what, want):
    refuse_split_backends(flow_dir, what)
    _check_raster(flow_dir.data, what)
    out = _run_graph(flow_dir.data, want)
    return DataArray(out, name=name, coords=flow_dir.coords, dims=flow_dir.dims, attrs=flow_dir.attrs)


@supports_dataset
def flow_accumulation(flow_dir: DataArray, name: str = 'flow_accumulation') -> DataArray:
    """For every cell the number of cells whose D8 flow path reaches it, itself included; NaN at NaN cells.

    flow_dir: 2-D DataArray of D8 codes as `flow_direction` returns them (or a Dataset: every variable on its own), NumPy- or
    DeviceArray-backed (the result's backend).  A value that is no code, or a cycle, raises ValueError.  Returns a float64
    DataArray with flow_dir's coords, dims and attrs."""
    return _graph_product(flow_dir, name, 'flow_accumulation', ACCUMULATION)


@supports_dataset
def basins(flow_dir: DataArray, name: str = 'basins') -> DataArray:
    """For every cell the linear index `row * W + col` of the outlet its D8 flow path ends in (an outlet: a cell with code 0,
    or whose code names a neighbour outside the raster or a NaN neighbour); NaN at NaN cells.  Arguments and errors as for
    `flow_accumulation`.  Returns a float64 DataArray."""
    return _graph_product(flow_dir, name, 'basins', BASINS)

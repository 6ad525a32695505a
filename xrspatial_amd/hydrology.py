"""fill, flow_direction, flow_accumulation, basins: D8 hydrology.  The reference (0.5.3) has no hydrology code, so the result is a
written rule (csrc/hydrology.hip and csrc/hydrology_fill.hip; stated in NumPy by tests/hydrology_oracle.py
and tests/hydrology_fill_oracle.py), and every output is an input value, an integer code or a count: the tests compare bit for bit.

fill.  The neighbours are the eight below.  A rim cell is a non-NaN cell with a neighbour outside the raster or NaN: water leaves
the raster there.
  1. a NaN cell gives NaN;
  2. a rim cell keeps its value;
  3. every other cell gets W(c) = the minimum, over all 8-connected paths of non-NaN cells from c to a rim cell, of the largest z
     on the path (both ends included): the fixed point of W(c) = max(z(c), min_n W(n)) reached from +inf at non-rim cells;
  4. only comparisons are made: every output value is an input value, +-inf are ordinary values, and which of -0.0 / +0.0
     comes out is not specified;
  5. float32 gives float32, float64 float64 (read in place); every other numeric dtype is cast to float64 on the host;
  6. with fewer than 3 rows or columns every cell is a rim cell: the result equals the input.

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

flow_direction(resolve_flats=True).  code0 = the result above.  A cell is drained if it is a rim cell or code0 != 0; every other
non-NaN cell is a flat cell.
  1. d(c) = 0 at drained cells;
  2. at a flat cell d(c) = 1 + min d(n) over the neighbours with z(n) == z(c), compared in the raster's dtype: the 8-connected
     step count, through cells of equal elevation, to the nearest drained cell of that elevation; infinite without one;
  3. a flat cell with finite d gets the code of the first neighbour, in the order above, with z(n) == z(c) and d(n) == d(c) - 1;
  4. a flat cell with infinite d (a closed pit or flat of an unfilled DEM) keeps 0;
  5. drained cells keep code0 (a rim cell with code 0 is an outlet); NaN cells stay NaN.
Along a path z never rises and among equal z the count d falls strictly: no cycle.  On W = fill(z) every flat cell has a finite d,
so every path of flow_direction(W, resolve_flats=True) ends in a rim cell.

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
TILE = 64                               # XRS_FILL_TILE: the tile edge of the fill / flat relaxer
FILL_STATUS_WORDS, FILL_STATUS_ROUNDS = 256, 80     # XRS_FILL_STATUS_WORDS / XRS_FILL_STATUS_ROUNDS


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


def relax_rounds(words):
    """The per-round part of xrs_fill's / xrs_flow_flats' status words: rounds run, then for the first FILL_STATUS_ROUNDS of them
    the cells that changed, the tiles launched and (with TIMED) the nanoseconds."""
    kept = min(words[0], FILL_STATUS_ROUNDS)
    return {"rounds": words[0], "tiles_launched": words[1], "changed": words[8:8 + kept],
            "tiles": words[8 + FILL_STATUS_ROUNDS:8 + FILL_STATUS_ROUNDS + kept],
            "ns": words[8 + 2 * FILL_STATUS_ROUNDS:8 + 2 * FILL_STATUS_ROUNDS + kept]}


# ------------------------------------------------------------------ fill
def fill_plane(src: DeviceArray, flags: int = 0, stream=None):
    """xrs_fill on a resident float32 / float64 plane: (the filled plane, status words)."""
    rows, cols = src.shape
    out = DeviceArray((rows, cols), src.dtype)
    status = (ctypes.c_int64 * FILL_STATUS_WORDS)()
    if rows * cols:
        work = workspace("fill", rows, cols)
        _lib.call("xrs_fill", src.ptr, DTYPE_CODE[src.dtype], rows, cols, out.ptr, work.ptr, status, flags, stream)
    return out, [int(w) for w in status]


def _run_fill(data):
    _lib.require_device()
    stream = get_stream()
    src, like_numpy = resident(data, stream, FLOAT_SUFFIX, np.float64)
    out, _ = fill_plane(src, stream=stream)
    settle(stream, like_numpy)                                           # the workspace goes back to the pool
    return finish(out, like_numpy)


@supports_dataset
def fill(agg: DataArray, name: str = 'fill') -> DataArray:
    """Depression fill: every cell raised to the level at which its water reaches the rim of the raster (a cell with a neighbour
    outside the raster or NaN); NaN at NaN cells.  Every output value is an input value (the rule: module docstring).

    agg: 2-D DataArray of elevations (or a Dataset: every variable on its own), NumPy- or DeviceArray-backed (the result's
    backend).  Returns a DataArray of agg's dtype (float32 or float64; any other numeric dtype gives float64) with agg's coords,
    dims and attrs."""
    refuse_split_backends(agg, 'fill')
    _check_raster(agg.data, 'fill')
    return DataArray(_run_fill(agg.data), name=name, coords=agg.coords, dims=agg.dims, attrs=agg.attrs)


# ------------------------------------------------------------------ flow_direction
def resolve_flats_plane(src: DeviceArray, codes: DeviceArray, flags: int = 0, stream=None):
    """xrs_flow_flats: the codes of xrs_flow_direction for the resident plane `src`, updated in place; the status words."""
    rows, cols = src.shape
    status = (ctypes.c_int64 * FILL_STATUS_WORDS)()
    if rows * cols:
        work = workspace("flow_flats", rows, cols)
        _lib.call("xrs_flow_flats", src.ptr, DTYPE_CODE[src.dtype], rows, cols, codes.ptr, work.ptr, status, flags, stream)
    return [int(w) for w in status]


def _run_direction(data, cx, cy, dg, resolve_flats=False):
    _lib.require_device()
    stream = get_stream()
    src, like_numpy = resident(data, stream, FLOAT_SUFFIX, np.float64)
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float32)
    if rows * cols:
        _lib.call("xrs_flow_direction", src.ptr, DTYPE_CODE[src.dtype], rows, cols, cx, cy, dg, out.ptr, stream)
        if resolve_flats:
            resolve_flats_plane(src, out, stream=stream)
        if src is not data or resolve_flats:
            settle(stream, like_numpy)                                   # the widened copy and the workspace go back to the pool
    return finish(out, like_numpy)


@supports_dataset
def flow_direction(agg: DataArray, name: str = 'flow_direction', resolve_flats: bool = False) -> DataArray:
    """D8 flow direction: for every cell the ESRI code (E 1, SE 2, S 4, SW 8, W 16, NW 32, N 64, NE 128) of the neighbour with
    the steepest drop, 0 where no neighbour lies lower, NaN at NaN cells (the rule: module docstring).

    agg: 2-D DataArray of elevations (or a Dataset: every variable on its own), NumPy- or DeviceArray-backed (the result's
    backend); the cell size comes from `attrs['res']` or the coordinates, as for `slope`.  resolve_flats: give every cell of a
    level area that has a drained cell the code of the neighbour one step nearer to it (on `fill(agg)` every path then ends at
    the rim of the raster).  Returns a float32 DataArray with agg's coords, dims and attrs."""
    refuse_split_backends(agg, 'flow_direction')
    rows, cols = _check_raster(agg.data, 'flow_direction')
    cx, cy, dg = cell_distances(agg) if rows * cols else (1.0, 1.0, float(np.sqrt(2.0)))
    out = _run_direction(agg.data, cx, cy, dg, bool(resolve_flats))
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

"""proximity, allocation, direction: distance to, value of and bearing to every cell's nearest target.  Reference:
xrspatial/proximity.py.

The reference ports GDAL's four-pass line sweep: a cell inherits the nearest target of its upper, left and upper-right
neighbour.  That is serial along rows and from row to row, and a heuristic: it can miss the true nearest target.  This backend
computes the minimum itself (csrc/proximity.hip), by this rule for the cell (i, j) at (x2, y2) = (xs[j], ys[i]):

  1. a target is a cell that is non-zero and finite (`target_values` empty) or equals one of `target_values` under NumPy's `==`;
  2. its distance is the reference's `_distance(xs[c], x2, ys[r], y2, metric)`: float64 on the coordinate values, then float32;
  3. the smallest float32 distance wins; of equal ones targets in rows r <= i come first, among them the first in row-major
     order, among rows r > i the last in row-major order (the order in which the sweep meets them).  EUCLIDEAN and MANHATTAN
     follow that at every cell, also where a whole run of targets in one row shares a float32 distance (long thin cells,
     distances that underflow); GREAT_CIRCLE names the nearest target of such a run on either side of the cell, where the
     rule may name another (`proximity` is the same either way);
  4. with s = d32 * d32 in float32 the cell is kept if float64(max_distance)**2 >= s, else all three products are NaN;
  5. proximity = float32(sqrt(float64(s))), allocation = float32(raster[r, c]), direction = the reference's `_calc_direction`.

That equals the reference wherever its heuristic finds the nearest target: executed as plain Python on 60 random rasters
(31 876 cells; 6-40 cells per side, 0.4-40 % targets, all metrics, dtypes, NaN, max_distance, target_values) the rule equals
it bit for bit at all but 2 cells for each product, and at those the reference's distance is the larger one (an earlier run:
3 of 25 844 cells; worst case 1 cell in 442).  The tie order picked the reference's target in 2183 of 2186 two-way ties.

The host checks the arguments (the reference's, plus finite and strictly monotonic coordinates, which the search rests on),
uploads the coordinates as float64 -- for GREAT_CIRCLE also np.radians / np.cos of them, NumPy's values -- and launches.  The
result is float32 whatever the raster's dtype, as upstream.  Every dtype the kernels read (the ten XRS_DT_* codes) is read in
place; bool and float16 rasters are widened on the host to uint8 / float32 first, so a `DeviceArray` of those two dtypes makes
one round trip through host memory per call.  There is no CPU fallback; dask- and ShardedArray-backed rasters
raise NotImplementedError.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, resident, settle, widened, workspace
from ._xr import DataArray
from .dataset_support import supports_dataset
from .device import DTYPE_CODE, DeviceArray

EUCLIDEAN = 0
GREAT_CIRCLE = 1
MANHATTAN = 2

PROXIMITY = 0
ALLOCATION = 1
DIRECTION = 2
ALL_THREE = 3                       # `mode` of xrs_proximity: the three planes at once
SCAN_ONLY, SEARCH_ONLY = 16, 32     # XRS_PROX_SCAN_ONLY / XRS_PROX_SEARCH_ONLY: one half of the call (tools/proximity_bench.py)

DISTANCE_METRICS = {"EUCLIDEAN": EUCLIDEAN, "GREAT_CIRCLE": GREAT_CIRCLE, "MANHATTAN": MANHATTAN}
_VALUES_F64, _VALUES_I64, _VALUES_U64 = 0, 1, 2


# ------------------------------------------------------------------ the three scalar helpers
def euclidean_distance(x1: float, x2: float, y1: float, y2: float) -> float:
    """Straight-line distance between (x1, y1) and (x2, y2), as `xrspatial.euclidean_distance`."""
    x = x1 - x2
    y = y1 - y2
    return np.sqrt(x * x + y * y)


def manhattan_distance(x1: float, x2: float, y1: float, y2: float) -> float:
    """Sum of the distances along x and y between (x1, y1) and (x2, y2), as `xrspatial.manhattan_distance`."""
    x = x1 - x2
    y = y1 - y2
    return abs(x) + abs(y)


def great_circle_distance(x1: float, x2: float, y1: float, y2: float, radius: float = 6378137) -> float:
    """Haversine distance between the longitude / latitude pairs (x1, y1) and (x2, y2) on a sphere of `radius`, as
    `xrspatial.great_circle_distance`, with its range errors."""
    if x1 > 180 or x1 < -180:
        raise ValueError("Invalid x-coordinate of the first point.Must be in the range [-180, 180]")
    if x2 > 180 or x2 < -180:
        raise ValueError("Invalid x-coordinate of the second point.Must be in the range [-180, 180]")
    if y1 > 90 or y1 < -90:
        raise ValueError("Invalid y-coordinate of the first point.Must be in the range [-90, 90]")
    if y2 > 90 or y2 < -90:
        raise ValueError("Invalid y-coordinate of the second point.Must be in the range [-90, 90]")
    lat1, lon1, lat2, lon2 = np.radians(y1), np.radians(x1), np.radians(y2), np.radians(x2)
    dlon = lon2 - lon1
    dlat = lat2 - lat1
    a = np.sin(dlat / 2.0) ** 2 + np.cos(lat1) * np.cos(lat2) * np.sin(dlon / 2.0) ** 2
    return radius * 2 * np.arcsin(np.sqrt(a))


# ------------------------------------------------------------------ argument checks (before any device work)
def _host(a):
    return np.asarray(a.get() if isinstance(a, DeviceArray) else a)


def check_axis(coords, n, axis):
    """One finite coordinate per cell along `axis`, strictly rising or strictly falling; returns them as float64."""
    coords = _host(coords)
    if coords.shape != (n,):
        raise ValueError(f"proximity: one {axis} coordinate per cell is needed, got shape {coords.shape} for {n} cells")
    c = coords.astype(np.float64)
    if not np.isfinite(c).all():
        raise ValueError(f"proximity: the {axis} coordinates are not finite")
    step = np.diff(c)
    if not ((step > 0).all() or (step < 0).all()):
        raise ValueError(f"proximity: the {axis} coordinates are not strictly monotonic")
    return c


def target_array(target_values, dtype):
    """(8-byte values, kind) as the kernel compares them with a raster of `dtype`: integers with an integer raster as
    integers, everything else as float64 (NumPy's promotion of `raster == value`)."""
    tv = np.asarray(target_values)
    if tv.ndim != 1:
        tv = tv.ravel()
    if tv.size == 0:
        return np.zeros(0, np.float64), _VALUES_F64
    if tv.dtype.kind == "b":
        tv = tv.astype(np.int64)
    if tv.dtype.kind not in "iuf":
        raise TypeError(f"proximity: target_values of dtype {tv.dtype} are not supported")
    if np.dtype(dtype).kind in "iu" and tv.dtype.kind in "iu":
        if tv.dtype.kind == "u" and tv.size and int(tv.max()) > np.iinfo(np.int64).max:
            return tv.astype(np.uint64), _VALUES_U64
        return tv.astype(np.int64), _VALUES_I64
    return tv.astype(np.float64), _VALUES_F64


def _prepare(raster, x, y, target_values, max_distance, distance_metric):
    """The reference's argument handling (`_process`) and this backend's checks; what the launch needs."""
    if tuple(raster.dims) != (y, x):
        raise ValueError("raster.coords should be named as coordinates:({0}, {1})".format(y, x))
    metric = DISTANCE_METRICS.get(distance_metric, None) if isinstance(distance_metric, str) else None
    if metric is None:
        metric = EUCLIDEAN
    if max_distance is None:
        max_distance = np.inf
    max_distance = float(max_distance)
    if np.isnan(max_distance):
        raise ValueError("proximity: max_distance is NaN")
    rows, cols = (int(s) for s in raster.shape)
    xs = check_axis(raster[x].data, cols, x)
    ys = check_axis(raster[y].data, rows, y)
    if metric == GREAT_CIRCLE and rows and cols:
        great_circle_distance(xs[0], xs[-1], ys[0], ys[-1])             # the reference's range errors (`_process`)
    return metric, max_distance, xs, ys


# ------------------------------------------------------------------ the launch
def widen(what):
    """The `widen` of `_launch.widened` for the kernels that read the ten XRS_DT_* dtypes: bool and float16 widen without loss."""
    def to(dtype):
        if dtype not in (np.bool_, np.float16):
            raise TypeError(f"{what}: unsupported raster dtype {dtype}")
        return np.uint8 if dtype == np.bool_ else np.float32
    return to


def _run(data, xs, ys, target_values, max_distance, metric, mode):
    """A NumPy raster gets NumPy back, a DeviceArray a DeviceArray."""
    _lib.require_device()
    like_numpy = isinstance(data, np.ndarray)
    stream = get_stream()
    data = widened(data, stream, DTYPE_CODE, widen("proximity"))
    values, kind = target_array(target_values, data.dtype)              # (its TypeError comes before the upload)
    src, _ = resident(data, stream)
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float32)
    if rows * cols:
        parts = [xs, ys]
        if metric == GREAT_CIRCLE:
            lat = np.radians(ys)
            parts += [np.radians(xs), lat, np.cos(lat)]
        parts.append(values.view(np.float64))
        aux = DeviceArray.from_numpy(np.concatenate(parts), stream=stream)
        gc = aux.ptr + 8 * (cols + rows) if metric == GREAT_CIRCLE else None
        vals = aux.ptr + 8 * (sum(p.size for p in parts) - values.size) if values.size else None
        work = workspace("proximity", rows, cols)
        _lib.call("xrs_proximity", src.ptr, DTYPE_CODE[src.dtype], rows, cols, aux.ptr, aux.ptr + 8 * cols, gc, vals, kind,
                  int(values.size), max_distance, metric, mode, work.ptr, out.ptr, stream)
        settle(stream, like_numpy)
    return finish(out, like_numpy)


def _process(raster, x, y, target_values, max_distance, distance_metric, mode):
    refuse_split_backends(raster, ("proximity", "allocation", "direction")[mode])
    metric, max_distance, xs, ys = _prepare(raster, x, y, target_values, max_distance, distance_metric)
    out = _run(raster.data, xs, ys, target_values, max_distance, metric, mode)
    return DataArray(out, coords=raster.coords, dims=raster.dims, attrs=raster.attrs)


@supports_dataset
def proximity(raster, x: str = "x", y: str = "y", target_values: list = [], max_distance: float = np.inf,
              distance_metric: str = "EUCLIDEAN"):
    """Distance from every cell to its nearest target cell.

    raster: 2-D DataArray (or a Dataset: every variable on its own) with dims (y, x) and one finite, strictly monotonic
    coordinate per row and column; NumPy- or DeviceArray-backed (the result's backend).  target_values: the cell values that
    are targets; empty: every non-zero finite cell.  max_distance: cells whose nearest target is farther are NaN (None: no
    limit); in the metric's unit.  distance_metric: 'EUCLIDEAN', 'GREAT_CIRCLE' (coordinates are degrees of longitude and
    latitude, the distance metres on a sphere of radius 6378137) or 'MANHATTAN'; anything else means 'EUCLIDEAN'.  Returns a
    float32 DataArray with raster's coords, dims and attrs.  Same signature as `xrspatial.proximity`; the result is the exact
    minimum, which equals the reference's wherever its sweep finds the nearest target (module docstring)."""
    return _process(raster, x, y, target_values, max_distance, distance_metric, PROXIMITY)


@supports_dataset
def allocation(raster, x: str = "x", y: str = "y", target_values: list = [], max_distance: float = np.inf,
               distance_metric: str = "EUCLIDEAN"):
    """The value of every cell's nearest target cell, as float32; arguments as for `proximity`.  Same signature as
    `xrspatial.allocation`."""
    return _process(raster, x, y, target_values, max_distance, distance_metric, ALLOCATION)


@supports_dataset
def direction(raster, x: str = "x", y: str = "y", target_values: list = [], max_distance: float = np.inf,
              distance_metric: str = "EUCLIDEAN"):
    """The compass bearing in degrees from every cell to its nearest target cell (90 east, 180 south, 270 west, 360 north, 0 at
    a target itself), as float32; arguments as for `proximity`.  Same signature as `xrspatial.direction`."""
    return _process(raster, x, y, target_values, max_distance, distance_metric, DIRECTION)

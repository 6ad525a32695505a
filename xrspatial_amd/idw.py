"""idw: inverse-distance interpolation of scattered points onto a raster, the way in for point samples (rain gauges, boreholes,
soundings, LiDAR returns).  The reference has no idw; the rule is written down in DESIGN.md §6t and computed by csrc/idw.hip:
pixel (row j, column i) is the square [i, i + 1] x [j, j + 1] with its centre at (i + 0.5, j + 0.5), every cell takes its `k`
nearest points by `(d2, index)` -- a total order, `d2 = dx * dx + dy * dy` rounded step by step -- within `max_distance`, and
its value is `sum(w * v) / sum(w)` with `w = 1 / d ** power`, summed nearest first.  The result is a function of the input bit
for bit.  `k=1` is nearest-neighbour (Thiessen / Voronoi) interpolation.

`neighbors` is the search without the arithmetic: the index and squared distance of every cell's k nearest points.  `idw`
is also exported from the package, where the name then means the function; `xrspatial_amd.idw.neighbors` and
`xrspatial_amd.idw.plan_bins` work either way.

The points are sorted on the device into square bins of `bin_cells` x `bin_cells` cells (`plan_bins`); `bin_cells=` overrides
the plan.  It is a tuning and testing knob: results never depend on it.

Non-integer powers, a radius search without `k`, several value columns per call, kriging, splines, natural neighbour, kernel
density, anisotropy, barriers and geopandas inputs are not built.  NumPy- and DeviceArray-backed `like` rasters are accepted;
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import operator

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, settle, workspace
from ._xr import DataArray
from .device import DTYPE_CODE, DeviceArray
from .rasterize import check_fill, inverse_transform

MAX_CELLS = (1 << 32) - 1            # 32-bit cell indices in csrc/idw.hip
MAX_POINTS = (1 << 31) - 1           # XRS_IDW_MAX_POINTS
MAX_BINS = 1 << 26                   # XRS_IDW_MAX_BINS, the apron ring included
MAX_K = 64                           # XRS_IDW_MAX_K
NONFINITE = 1                        # XRS_IDW_NONFINITE


def n_bins(rows, cols, bin_cells):
    """Bins of `bin_cells` x `bin_cells` cells over a raster, with the apron ring around them."""
    return (-(-cols // bin_cells) + 2) * (-(-rows // bin_cells) + 2)


def whole_raster_bin(rows, cols):
    """The smallest power of two that puts the whole raster into one bin."""
    return 1 << (max(rows, cols) - 1).bit_length()


def plan_bins(n_points, rows, cols):
    """The bin size B, in cells, a power of two: the smallest with at least 1.41 points per bin on average for points spread
    over the raster (so between 1.41 and 5.66, about 2 - 4), no larger than one bin over the whole raster and no smaller than
    keeps the bin count within MAX_BINS.  Host only; never grows with n_points.  The target was set by reasoning, not tuned: the
    sweep in DESIGN.md §6t, run afterwards, finds the search flat from 0.24 to 4 points per bin and slower above."""
    cap = whole_raster_bin(rows, cols)
    b = 1
    while b < cap and 100 * n_points * b * b < 141 * rows * cols:
        b *= 2
    while n_bins(rows, cols, b) > MAX_BINS:
        b *= 2
    return b


def _check_like(like, what):
    if like.ndim != 2 or like.shape[0] < 1 or like.shape[1] < 1:
        raise ValueError(f"{what}: `like` must be 2D with a shape of at least (1, 1)")
    refuse_split_backends(like, what)
    rows, cols = (int(s) for s in like.shape)
    if rows * cols > MAX_CELLS:
        raise ValueError(f"{what}: {rows} x {cols} cells exceed the 2**32 - 1 cells this backend indexes; "
                         "split your raster into smaller chunks.")
    return rows, cols


def _check_points(points, what):
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.size == 0:
        points = points.reshape(0, 2)
    if points.ndim != 2 or points.shape[1] != 2:
        raise ValueError(f"{what}: points must have shape (n, 2), not {points.shape}")
    if len(points) > MAX_POINTS:
        raise ValueError(f"{what}: more than {MAX_POINTS} points")
    if not np.isfinite(points).all():
        raise ValueError(f"{what}: a coordinate is not finite (NaN or infinite, as given or after the transform)")
    return points


def _check_int(value, lo, hi, name, what):
    try:
        v = operator.index(value)
    except TypeError:
        if isinstance(value, (float, np.floating)) and float(value).is_integer():
            v = int(value)
        else:
            raise ValueError(f"{what}: {name} must be an integer of {lo} .. {hi}, not {value!r}")
    if not lo <= v <= hi:
        raise ValueError(f"{what}: {name} must be an integer of {lo} .. {hi}, not {value!r}")
    return v


def radius_squared(max_distance, transform):
    """`max_distance`, in cells, squared, once, in float64; -1.0 for None.  With a transform the distance is in world units and
    the transform must have square, unrotated cells: t1 = t3 = 0 and |t0| = |t4|."""
    if max_distance is None:
        return -1.0
    d = float(max_distance)
    if math.isnan(d) or d < 0:
        raise ValueError(f"idw: max_distance must be a number >= 0, not {max_distance!r}")
    if transform is not None:
        t = [float(v) for v in np.asarray(transform).reshape(-1)]
        if len(t) != 6 or t[1] != 0 or t[3] != 0 or abs(t[0]) != abs(t[4]) or t[0] == 0:
            raise ValueError("idw: max_distance in world units needs a transform with t1 = t3 = 0 and |t0| = |t4| "
                             "(square cells, no rotation)")
        d = d / abs(t[0])
    return d * d


def _check_bin_cells(bin_cells, n_points, rows, cols, what):
    if bin_cells is None:
        return plan_bins(n_points, rows, cols)
    b = _check_int(bin_cells, 1, 1 << 32, "bin_cells", what)
    if b & (b - 1):
        raise ValueError(f"{what}: bin_cells must be a power of two, not {bin_cells!r}")
    if n_bins(rows, cols, b) > MAX_BINS:
        raise ValueError(f"{what}: bin_cells={b} makes {n_bins(rows, cols, b)} bins, more than {MAX_BINS}")
    return b


def search(points, values, rows, cols, inverse, k, power, max_d2, min_points, fill, dtype, bin_cells, stream,
           want_out=True, want_planes=False):
    """(out, index, d2, keep): DeviceArrays or None.  The two calls of csrc/idw.hip."""
    _lib.require_device()
    n = len(points)
    inv = (ctypes.c_double * 6)(*inverse) if inverse is not None else None
    pts = DeviceArray.from_numpy(points, stream=stream) if n else None
    work = workspace("idw", n, rows, cols, bin_cells)
    flags = ctypes.c_int(0)
    _lib.call("xrs_idw_bin", pts.ptr if n else None, n, rows, cols, bin_cells, inv, work.ptr, ctypes.byref(flags), stream)
    if flags.value & NONFINITE:
        raise ValueError("idw: a coordinate is not finite (NaN or infinite, as given or after the transform)")
    vals = DeviceArray.from_numpy(values, stream=stream) if want_out and n else None
    out = DeviceArray((rows, cols), dtype) if want_out else None
    index = DeviceArray((k, rows, cols), np.int32) if want_planes else None
    d2 = DeviceArray((k, rows, cols), np.float64) if want_planes else None
    _lib.call("xrs_idw_search", work.ptr, vals.ptr if vals is not None else None, n, rows, cols, bin_cells, k, power, max_d2,
              min_points, float(fill), DTYPE_CODE[np.dtype(dtype)], out.ptr if want_out else None,
              index.ptr if want_planes else None, d2.ptr if want_planes else None, stream)
    return out, index, d2, [pts, work, vals]


def idw(points, values, like, *, k=12, power=2, max_distance=None, min_points=1, transform=None, fill=np.nan,
        dtype=np.float64, name="idw", bin_cells=None, stats=None):
    """
    Interpolate scattered points onto a raster shaped like `like` by inverse
    distance weighting over the `k` nearest points of every cell centre.

    Parameters
    ----------
    points: array (n, 2) of float64
        `(x, y)` in pixel space (pixel (row j, column i) is the square
        [i, i + 1] x [j, j + 1]), or in world space with `transform`.  Points
        may lie outside the raster.  A coordinate that is not finite raises
        ValueError.

    values: array (n,)
        One value per point, cast to float64.  A point whose value is NaN is
        dropped; "index" below is the position among the points kept.

    like: DataArray
        2D, NumPy- or DeviceArray-backed.  Only its shape, dims, coords and
        attrs are used; the result carries them and has its backend.

    k: int, default=12
        Neighbours per cell, 1 .. 64: the first `k` candidates by
        `(d2, index)`, `d2 = dx * dx + dy * dy` from the cell centre.  `k=1`
        is nearest-neighbour interpolation.

    power: int, default=2
        1 .. 8; the weight of a neighbour is `1 / d ** power`, computed as
        products of `d2` (times `sqrt(d2)` for an odd power).  A neighbour at
        distance 0 gives its value (the lowest index among coincident ones).

    max_distance: float, optional
        Only points with `d2 <= max_distance ** 2` are candidates.  In cells
        without a transform; in world units with one, which must then have
        square, unrotated cells (t1 = t3 = 0, |t0| = |t4|).

    min_points: int, default=1
        1 .. k; a cell with fewer candidates gets `fill`.

    transform: sequence of 6 floats, optional
        Pixel to world, as `rasterize` takes it.

    fill: scalar, default=nan
        Must be exactly representable in `dtype`.

    dtype: float64 or float32, default=float64
        The sums are float64; the result is rounded once.

    name: str, default="idw"
        Name of the result.

    bin_cells: int, optional
        Side of the search bins in cells, a power of two; default
        `plan_bins(n, rows, cols)`.  A tuning and testing knob: results never
        depend on it.

    stats: dict, optional
        Receives `bin_cells`, `bins` and `points` (the points kept).

    Returns
    -------
    DataArray with `like`'s shape, dims, coords and attrs.
    """
    rows, cols = _check_like(like, "idw")
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise TypeError(f"idw: dtype must be float64 or float32, not {dtype}")
    k = _check_int(k, 1, MAX_K, "k", "idw")
    power = _check_int(power, 1, 8, "power", "idw")
    min_points = _check_int(min_points, 1, k, "min_points", "idw")
    points = _check_points(points, "idw")
    values = np.asarray(values, dtype=np.float64)
    if values.shape != (len(points),):
        raise ValueError(f"idw: values must have shape ({len(points)},), not {values.shape}")
    keep = ~np.isnan(values)
    if not keep.all():
        points, values = np.ascontiguousarray(points[keep]), values[keep]
    values = np.ascontiguousarray(values)
    fill_item = check_fill(fill, dtype)
    max_d2 = radius_squared(max_distance, transform)
    inverse = inverse_transform(transform)
    bin_cells = _check_bin_cells(bin_cells, len(points), rows, cols, "idw")
    if stats is not None:
        stats.update(bin_cells=bin_cells, bins=n_bins(rows, cols, bin_cells), points=len(points))
    stream = get_stream()
    like_numpy = not isinstance(like.data, DeviceArray)
    out, _, _, held = search(points, values, rows, cols, inverse, k, power, max_d2, min_points, fill_item, dtype, bin_cells, stream)
    result = finish(out, like_numpy)
    settle(stream, like_numpy)                            # the workspace goes back to the pool
    del held
    return DataArray(result, name=name, coords=like.coords, dims=like.dims, attrs=like.attrs)


def neighbors(points, like, *, k, max_distance=None, transform=None, bin_cells=None, stats=None):
    """
    The search of `idw` without the arithmetic: `(index, d2)` of every cell's
    `k` nearest points, nearest first by `(d2, index)`.

    `index` is int32 `[k, H, W]`, -1 where a cell has fewer than `k`
    candidates; `d2` is float64 `[k, H, W]`, +inf there.  NumPy arrays for a
    NumPy-backed `like`, DeviceArrays for a DeviceArray-backed one.  `points`,
    `like`, `k`, `max_distance`, `transform`, `bin_cells` and `stats` are
    `idw`'s; there are no values, so no point is dropped.
    """
    rows, cols = _check_like(like, "idw.neighbors")
    k = _check_int(k, 1, MAX_K, "k", "idw.neighbors")
    points = _check_points(points, "idw.neighbors")
    max_d2 = radius_squared(max_distance, transform)
    inverse = inverse_transform(transform)
    bin_cells = _check_bin_cells(bin_cells, len(points), rows, cols, "idw.neighbors")
    if stats is not None:
        stats.update(bin_cells=bin_cells, bins=n_bins(rows, cols, bin_cells), points=len(points))
    stream = get_stream()
    like_numpy = not isinstance(like.data, DeviceArray)
    _, index, d2, held = search(points, None, rows, cols, inverse, k, 1, max_d2, 1, 0.0, np.float64, bin_cells, stream,
                                want_out=False, want_planes=True)
    index, d2 = finish(index, like_numpy), finish(d2, like_numpy)
    settle(stream, like_numpy)
    del held
    return index, d2


# `from xrspatial_amd import idw` binds the function over the module's name in the package; the module's other entry points stay
# reachable through it
idw.neighbors = neighbors
idw.plan_bins = plan_bins

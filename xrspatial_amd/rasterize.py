"""rasterize: burn polygons into a raster, the way back from `polygonize`.  The reference has no rasterize; the rule is
written down in DESIGN.md §6r and computed by csrc/rasterize.hip: pixel (row j, column i) is the square [i, i + 1] x
[j, j + 1], a cell belongs to a polygon when its centre is inside it by the even-odd rule (a centre on a left edge is inside,
on a right edge outside), and where polygons overlap `merge` says which one a cell takes.  `rasterize(polygonize(a))` gives
`a` back.

Polygons come in either of polygonize's formats with the column split off: the `return_type="numpy"` list (one list of
`(n, 2)` rings per polygon, the exterior first, then the holes) or the flat 3-tuple `(points [n, 2] float64, ring_offsets int64,
polygon_offsets int64)`.  Holes need no special handling and ring orientation does not matter.  `all_touched`, lines, points
and geopandas / shapely objects are not supported.

NumPy- and DeviceArray-backed `like` rasters are accepted; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, settle, workspace
from ._xr import DataArray
from .device import DTYPE_CODE, DeviceArray
from .experimental.polygonize import _free_bytes

MAX_CELLS = (1 << 32) - 1            # 32-bit cell indices in csrc/rasterize.hip
MAX_POLYGONS = (1 << 31) - 1         # XRS_RASTERIZE_MAX_POINTS: polygons, rings and ring points are 32-bit indices with a bit to spare
MAX_CROSSINGS = (1 << 31) - 2        # XRS_RASTERIZE_MAX_CROSSINGS
NONFINITE = 1                        # XRS_RASTERIZE_NONFINITE
MERGES = ("last", "first", "min", "max", "count")


def flatten(polygons):
    """(points, ring_offsets, polygon_offsets) of either polygon format, validated; no device needed."""
    if isinstance(polygons, tuple) and len(polygons) == 3 and not isinstance(polygons[0], (list, tuple)):
        points = np.ascontiguousarray(polygons[0], dtype=np.float64)
        ring_offsets = np.ascontiguousarray(polygons[1], dtype=np.int64).reshape(-1)
        polygon_offsets = np.ascontiguousarray(polygons[2], dtype=np.int64).reshape(-1)
        if points.ndim != 2 or points.shape[1] != 2:
            raise ValueError(f"rasterize: points must have shape (n, 2), not {points.shape}")
    else:
        rings = []
        counts = []
        for poly in polygons:
            counts.append(len(poly))
            for ring in poly:
                ring = np.asarray(ring, dtype=np.float64)
                if ring.size == 0:
                    ring = ring.reshape(0, 2)
                if ring.ndim != 2 or ring.shape[1] != 2:
                    raise ValueError(f"rasterize: every ring must have shape (n, 2), not {ring.shape}")
                rings.append(ring)
        points = np.concatenate(rings) if rings else np.empty((0, 2), np.float64)
        points = np.ascontiguousarray(points)
        ring_offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
        polygon_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    for name, off, end, of in (("ring_offsets", ring_offsets, len(points), "points"),
                               ("polygon_offsets", polygon_offsets, len(ring_offsets) - 1, "rings")):
        if len(off) < 1 or off[0] != 0:
            raise ValueError(f"rasterize: {name} must start at 0")
        if np.any(np.diff(off) < 0):
            raise ValueError(f"rasterize: {name} must be non-decreasing")
        if off[-1] != end:
            raise ValueError(f"rasterize: {name} ends at {int(off[-1])}, not at the number of {of} ({end})")
    if len(polygon_offsets) - 1 > MAX_POLYGONS:
        raise ValueError(f"rasterize: more than {MAX_POLYGONS} polygons")
    if len(points) > MAX_POLYGONS or len(ring_offsets) - 1 > MAX_POLYGONS:
        raise ValueError(f"rasterize: more than {MAX_POLYGONS} rings or ring points")
    return points, ring_offsets, polygon_offsets


def inverse_transform(transform):
    """(a0, a1, a2, a3, t2, t5) of a pixel-to-world transform, or None for None; ValueError for a singular one."""
    if transform is None:
        return None
    t = [float(v) for v in np.asarray(transform).reshape(-1)]
    if len(t) != 6:
        raise ValueError(f"Incorrect transform length of {len(t)} instead of 6")
    det = t[0] * t[4] - t[1] * t[3]
    if not all(math.isfinite(v) for v in t) or not math.isfinite(det) or det == 0:
        raise ValueError(f"rasterize: the transform {tuple(t)} is singular or not finite")
    return t[4] / det, -t[1] / det, -t[3] / det, t[0] / det, t[2], t[5]


def transform_from_coords(like):
    """The pixel-to-world transform `(dx, 0, x0 - dx / 2, 0, dy, y0 - dy / 2)` of a raster whose 1-D x and y coords hold the
    cell centres, evenly spaced; ValueError otherwise."""
    if like.ndim != 2:
        raise ValueError("transform_from_coords: `like` must be 2D")
    ydim, xdim = like.dims
    out = []
    for dim, n in ((xdim, like.shape[1]), (ydim, like.shape[0])):
        if dim not in like.coords:
            raise ValueError(f"transform_from_coords: `like` has no coords for {dim!r}")
        c = np.asarray(like.coords[dim].values if hasattr(like.coords[dim], "values") else like.coords[dim], dtype=np.float64)
        if c.ndim != 1 or len(c) != n:
            raise ValueError(f"transform_from_coords: the coords of {dim!r} are not 1-D of length {n}")
        if n == 1:
            raise ValueError(f"transform_from_coords: one coordinate along {dim!r} gives no cell size")
        step = (c[-1] - c[0]) / (n - 1)                   # utils.calc_res's cell size
        if not np.isfinite(step) or step == 0 or not np.allclose(np.diff(c), step, rtol=1e-6, atol=0.0):
            raise ValueError(f"transform_from_coords: the coords of {dim!r} are not evenly spaced")
        out.append((float(step), float(c[0])))
    (dx, x0), (dy, y0) = out
    return (dx, 0.0, x0 - dx / 2, 0.0, dy, y0 - dy / 2)


def check_fill(fill, dtype):
    """`fill` as one item of `dtype`; ValueError unless it is exactly representable (NaN is, for the float dtypes)."""
    dtype = np.dtype(dtype)
    bad = ValueError(f"rasterize: fill {fill!r} is not exactly representable in {dtype}")
    if dtype.kind == "f":
        try:
            f = float(fill)
        except (TypeError, ValueError):
            raise bad
        with np.errstate(all="ignore"):
            item = dtype.type(f)
        if math.isnan(f) or float(item) == f:
            return item
        raise bad
    if isinstance(fill, (float, np.floating)):
        if not math.isfinite(fill) or fill != int(fill):
            raise bad
    try:
        i = int(fill)
    except (TypeError, ValueError):
        raise bad
    if i != fill:
        raise bad
    info = np.iinfo(dtype)
    if not info.min <= i <= info.max:
        raise bad
    return dtype.type(i)


def plan_merge(merge, column, n_polygons, dtype):
    """(values in the output dtype or None, priority uint32 [P], order uint32 [P], output dtype): priority[p] is polygon p's rank,
    a cell takes the covering polygon with the highest; order[rank] = p."""
    if merge not in MERGES:
        raise ValueError(f"rasterize: merge must be one of {MERGES}, not {merge!r}")
    if merge == "count":
        dtype = np.dtype(np.int32 if dtype is None else dtype)
        if dtype not in DTYPE_CODE:
            raise TypeError(f"rasterize: unsupported dtype {dtype}")
        return None, None, None, dtype
    if column is None:
        values = np.arange(1, n_polygons + 1, dtype=np.int32)
    else:
        values = np.asarray(column)
        if values.ndim != 1 or len(values) != n_polygons:
            raise ValueError(f"rasterize: column holds {values.shape} values for {n_polygons} polygons")
    if values.dtype == np.bool_:
        values = values.astype(np.uint8)
    dtype = np.dtype(values.dtype if dtype is None else dtype)
    if dtype not in DTYPE_CODE:
        raise TypeError(f"rasterize: unsupported dtype {dtype}")
    values = np.ascontiguousarray(values.astype(dtype, copy=False))
    p = np.arange(n_polygons, dtype=np.int64)
    if merge == "last":
        order = p
    elif merge == "first":
        order = p[::-1]
    else:
        if values.dtype.kind == "f" and np.isnan(values).any():
            raise ValueError(f'rasterize: merge="{merge}" with a NaN in the column')
        if merge == "max":                                # rising values, equal ones by position: the later polygon ranks higher
            order = np.argsort(values, kind="stable")
        else:                                             # falling values, equal ones by position
            order = (n_polygons - 1 - np.argsort(values[::-1], kind="stable"))[::-1]
    priority = np.empty(n_polygons, np.uint32)
    priority[order] = p
    return values, priority, np.ascontiguousarray(order, dtype=np.uint32), dtype


def key_bits(rows, cols, n_polygons):
    """Bits of the (polygon, row, column) sort key.  Within MAX_CELLS and MAX_POLYGONS it never exceeds 31 + 33 = 64."""
    return max(n_polygons - 1, 0).bit_length() + (rows - 1).bit_length() + cols.bit_length()


def burn(points, ring_offsets, polygon_offsets, rows, cols, inverse, values, priority, order, dtype, fill_item, count,
         stream, stats=None):
    """The DeviceArray of the result.  The four calls of csrc/rasterize.hip."""
    n_points, n_rings, n_polygons = len(points), len(ring_offsets) - 1, len(polygon_offsets) - 1
    _lib.require_device()
    inv = (ctypes.c_double * 6)(*inverse) if inverse is not None else None
    n_crossings = n_items = n_spans = 0
    spans = None
    keep = []                                             # what the launches read, until the result is done
    if n_points and n_polygons:
        pts = DeviceArray.from_numpy(points, stream=stream)
        ro = DeviceArray.from_numpy(ring_offsets, stream=stream)
        po = DeviceArray.from_numpy(polygon_offsets, stream=stream)
        work = workspace("rasterize", n_points)
        keep += [pts, ro, po, work]
        shape_args = (pts.ptr, ro.ptr, po.ptr, n_points, n_rings, n_polygons, rows, cols, inv)
        c, flags = ctypes.c_uint64(0), ctypes.c_int(0)
        _lib.call("xrs_rasterize_census", *shape_args, work.ptr, ctypes.byref(c), ctypes.byref(flags), stream)
        if flags.value & NONFINITE:
            raise ValueError("rasterize: a vertex is not finite (NaN or infinite, as given or after the transform)")
        n_crossings = int(c.value)
        if n_crossings > MAX_CROSSINGS:
            raise ValueError(f"rasterize: {n_crossings} crossings of edges and rows exceed the {MAX_CROSSINGS} this backend sorts; "
                             "split your polygons or your raster into smaller chunks.")
        if n_crossings:
            span_bytes = _lib.workspace_bytes("rasterize_spans", n_crossings)
            need = span_bytes + rows * cols * (4 + dtype.itemsize)
            free = _free_bytes()
            if need > free:
                raise MemoryError(f"rasterize: {n_crossings} crossings need {need} bytes of device memory, {free} are free; "
                                  "split your polygons or your raster into smaller chunks.")
            spans = DeviceArray((span_bytes,), np.uint8)
            keep.append(spans)
            ns, ni = ctypes.c_uint64(0), ctypes.c_uint64(0)
            _lib.call("xrs_rasterize_spans", *shape_args, work.ptr, spans.ptr, n_crossings, ctypes.byref(ns), ctypes.byref(ni), stream)
            n_spans, n_items = int(ns.value), int(ni.value)
    if stats is not None:
        stats.update(crossings=n_crossings, spans=n_spans, items=n_items)
    plane = DeviceArray((rows, cols), np.uint32)
    prio_dev = order_dev = values_dev = None
    if not count and n_polygons:
        prio_dev = DeviceArray.from_numpy(priority, stream=stream)
        order_dev = DeviceArray.from_numpy(order, stream=stream)
        values_dev = DeviceArray.from_numpy(values, stream=stream)
        keep += [prio_dev, order_dev, values_dev]
    _lib.call("xrs_rasterize_burn", rows, cols, spans.ptr if spans is not None else None, n_crossings, n_polygons, n_items,
              prio_dev.ptr if prio_dev is not None else None, int(count), plane.ptr, stream)
    out = DeviceArray((rows, cols), dtype)
    fill_buf = np.zeros(1, dtype)
    fill_buf[0] = fill_item
    _lib.call("xrs_rasterize_gather", plane.ptr, rows, cols, values_dev.ptr if values_dev is not None else None,
              order_dev.ptr if order_dev is not None else None, DTYPE_CODE[dtype], fill_buf.ctypes.data, int(count), out.ptr, stream)
    keep.append(plane)
    return out, keep


def rasterize(polygons, like, column=None, *, transform=None, fill=0, dtype=None, merge="last", name="rasterize"):
    """
    Burn polygons into a raster shaped like `like`.  The inverse of
    `polygonize`: `rasterize(polygons, r, column)` of
    `column, polygons = polygonize(r)` gives `r` back.

    Parameters
    ----------
    polygons: list or 3-tuple
        Either a list of polygons, each a list of (n, 2) float arrays, the
        exterior first, then the holes (polygonize's "numpy" format), or
        `(points, ring_offsets, polygon_offsets)` (its "flat" format without
        the column).

    like: DataArray
        2D, NumPy- or DeviceArray-backed.  Only its shape, dims, coords and
        attrs are used; the result carries them and has its backend.

    column: array, optional
        One value per polygon.  Default: 1 .. P as int32, the polygon's
        position plus one.

    transform: sequence of 6 floats, optional
        Pixel to world, as `polygonize` takes it: x = t0 * i + t1 * j + t2,
        y = t3 * i + t4 * j + t5 with i the column and j the row.  Default:
        the points are in pixel space.  See `transform_from_coords`.

    fill: scalar, default=0
        Value of the cells that no polygon covers; must be exactly
        representable in `dtype` (NaN is, for float dtypes).

    dtype: dtype, optional
        Dtype of the result.  Default: the column's (int32 for "count").

    merge: str, default="last"
        Where polygons overlap: "last" (the polygon latest in the list),
        "first", "min", "max" (by column value, equal values going to the
        later polygon), or "count" (the number of polygons covering the
        cell; ignores `column` and `fill`).

    name: str, default="rasterize"
        Name of the result.

    Returns
    -------
    DataArray with `like`'s shape, dims, coords and attrs.
    """
    if like.ndim != 2 or like.shape[0] < 1 or like.shape[1] < 1:
        raise ValueError("rasterize: `like` must be 2D with a shape of at least (1, 1)")
    refuse_split_backends(like, "rasterize")
    rows, cols = (int(s) for s in like.shape)
    if rows * cols > MAX_CELLS:
        raise ValueError(f"rasterize: {rows} x {cols} cells exceed the 2**32 - 1 cells this backend indexes; "
                         "split your raster into smaller chunks.")
    points, ring_offsets, polygon_offsets = flatten(polygons)
    n_polygons = len(polygon_offsets) - 1
    values, priority, order, dtype = plan_merge(merge, column, n_polygons, dtype)
    fill_item = check_fill(fill, dtype)
    inverse = inverse_transform(transform)
    stream = get_stream()
    like_numpy = not isinstance(like.data, DeviceArray)
    out, keep = burn(points, ring_offsets, polygon_offsets, rows, cols, inverse, values, priority, order, dtype, fill_item,
                     merge == "count", stream)
    result = finish(out, like_numpy)
    settle(stream, like_numpy)                            # the workspaces go back to the pool
    del keep
    return DataArray(result, name=name, coords=like.coords, dims=like.dims, attrs=like.attrs)

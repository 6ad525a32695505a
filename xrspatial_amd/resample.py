"""resample: regrid a raster onto another axis-aligned grid, the way in for a raster that lies on a different grid (a 10 m land
cover against a 30 m DEM, a DEM halved before `viewshed`, a coarse rainfall grid used as `weights=`, pyramids and thumbnails).
The reference has no resample; the rule is written down in DESIGN.md §6u and computed by csrc/resample.hip: ALL GEOMETRY LIVES
IN TABLES of one entry per destination row and one per destination column, computed here in float64 NumPy (`tables`); the device
only loads, compares, multiplies, adds and divides in a fixed order.  The result is a function of the input bit for bit.

Per axis the source pixel position of destination position `p` is `s(p) = ((D0 * p + D2) - S2) / S0`, every operation rounded,
with `D` the destination's and `S` the source's `(scale, offset)`; a cell centre is `p = i + 0.5` and cell `c` covers
`[c, c + 1]`.  `nearest` takes the cell `floor(s(i + 0.5))`; `bilinear`, `cubic` (Catmull-Rom) and `lanczos` (a = 3) weigh 2, 4
and 6 taps per axis around it; `average`, `sum`, `min`, `max` and `mode` work over the source cells that the destination cell
`[s(i), s(i + 1)]` overlaps.

Reprojection between coordinate systems, rotated or sheared grids, 3-D / multiband input, support scaling of the interpolation
kernels when downsampling (use `average` there), `all_touched`-style options, and sharded or dask rasters are not built.  NumPy-
and DeviceArray-backed rasters are accepted; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, resident, settle
from ._xr import DataArray
from .device import DTYPE_CODE, DeviceArray
from .rasterize import check_fill, transform_from_coords

MAX_CELLS = (1 << 32) - 1            # 32-bit cell indices in csrc/resample.hip
MAX_AXIS = (1 << 31) - 1             # int32 tables
MAX_TAPS = 256                       # XRS_RESAMPLE_MAX_TAPS
MODE_MAX_WINDOW = 1024               # XRS_RESAMPLE_MODE_MAX_WINDOW
POINT_METHODS = ("nearest", "bilinear", "cubic", "lanczos")
AREA_METHODS = ("average", "sum", "min", "max", "mode")
METHODS = POINT_METHODS + AREA_METHODS
SELECT_OP = {"min": 0, "max": 1, "mode": 2}                       # XRS_RESAMPLE_MIN, _MAX, _MODE
_INTERP = {"bilinear": (0, 2), "cubic": (1, 4), "lanczos": (2, 6)}    # taps in front of c0, taps
IDENTITY = (1.0, 0.0)


# ------------------------------------------------------------------ the tables: all the geometry there is
def axes_of(transform):
    """((x scale, x offset), (y scale, y offset)) of a pixel-to-world transform `(t0, t1, t2, t3, t4, t5)`; the identity for
    None.  ValueError for rotation or shear (t1, t3 != 0) and for a scale that is 0 or not finite."""
    if transform is None:
        return IDENTITY, IDENTITY
    t = [float(v) for v in np.asarray(transform).reshape(-1)]
    if len(t) != 6:
        raise ValueError(f"Incorrect transform length of {len(t)} instead of 6")
    if t[1] != 0 or t[3] != 0:
        raise ValueError(f"resample: the transform {tuple(t)} has rotation or shear (t1, t3 != 0); only axis-aligned grids "
                         "are supported")
    if not all(math.isfinite(v) for v in t) or t[0] == 0 or t[4] == 0:
        raise ValueError(f"resample: the transform {tuple(t)} is singular or not finite")
    return (t[0], t[2]), (t[4], t[5])


def positions(p, D, S):
    """`s(p) = ((D0 * p + D2) - S2) / S0` of float64 positions `p`, every operation rounded."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = ((np.float64(D[0]) * p + np.float64(D[1])) - np.float64(S[1])) / np.float64(S[0])
    if not np.isfinite(s).all():
        raise ValueError("resample: a destination position is not finite in source pixels")
    return s


def _index(first, taps, n_src):
    # a window that lies wholly outside stays wholly outside, and fits int32
    return np.clip(first, -float(taps), float(n_src)).astype(np.int32)


def near_table(n_src, n_dst, D=IDENTITY, S=IDENTITY):
    """int32 [n_dst]: `floor(s(i + 0.5))`, or -1 where that lies outside `[0, n_src)`."""
    f = np.floor(positions(np.arange(n_dst, dtype=np.float64) + 0.5, D, S))
    return np.where((f >= 0) & (f < n_src), f, -1.0).astype(np.int32)


def _cubic(x):
    ax = np.abs(x)
    inner = (1.5 * ax - 2.5) * ax * ax + 1.0
    outer = ((-0.5 * ax + 2.5) * ax - 4.0) * ax + 2.0
    return np.where(ax <= 1.0, inner, np.where(ax < 2.0, outer, 0.0))


def _lanczos(x):
    px = np.pi * x
    with np.errstate(all="ignore"):
        w = 3.0 * np.sin(px) * np.sin(px / 3.0) / (px * px)
    return np.where(x == 0.0, 1.0, np.where((np.abs(x) >= 3.0) | (x == np.floor(x)), 0.0, w))


def interp_table(method, n_src, n_dst, D=IDENTITY, S=IDENTITY):
    """(first int32 [n_dst], w float64 [n_dst][taps]) of `bilinear`, `cubic` or `lanczos`: `u = s(i + 0.5) - 0.5`,
    `c0 = floor(u)`, `t = u - c0`; the taps start at `c0`, `c0 - 1`, `c0 - 2`; tap k lies `x = t - k` from the point; every row of
    weights is divided by its sum, taken left to right."""
    lead, taps = _INTERP[method]
    u = positions(np.arange(n_dst, dtype=np.float64) + 0.5, D, S) - 0.5
    c0 = np.floor(u)
    t = u - c0
    if method == "bilinear":
        w = np.stack([1.0 - t, t], axis=1)
    else:
        x = t[:, None] - (np.arange(taps, dtype=np.float64) - lead)[None, :]
        w = _cubic(x) if method == "cubic" else _lanczos(x)
    total = w[:, 0]
    for k in range(1, taps):
        total = total + w[:, k]
    return _index(c0 - lead, taps, n_src), np.ascontiguousarray(w / total[:, None])


def area_table(n_src, n_dst, D=IDENTITY, S=IDENTITY):
    """(first int32 [n_dst], w float64 [n_dst][taps]): destination cell i covers `[lo, hi]` between `s(i)` and `s(i + 1)`; its
    taps are the source cells `floor(lo) .. ceil(hi) - 1`, each weighted by its overlap `min(hi, c + 1) - max(lo, c)`; rows are
    padded with zeros to the longest.  ValueError for more than MAX_TAPS taps."""
    e = positions(np.arange(n_dst + 1, dtype=np.float64), D, S)
    lo, hi = np.minimum(e[:-1], e[1:]), np.maximum(e[:-1], e[1:])
    first = np.floor(lo)
    count = np.ceil(hi) - 1.0 - first + 1.0
    taps = max(int(count.max()), 1)
    if taps > MAX_TAPS:
        raise ValueError(f"resample: a destination cell covers {taps} source cells along an axis, more than the {MAX_TAPS} taps "
                         "of one call; resample in two steps")
    k = np.arange(taps, dtype=np.float64)[None, :]
    c = first[:, None] + k
    w = np.minimum(hi[:, None], c + 1.0) - np.maximum(lo[:, None], c)
    w = np.where(k < count[:, None], w, 0.0)
    return _index(first, taps, n_src), np.ascontiguousarray(w)


def tables(method, src_shape, dst_shape, src_transform=None, dst_transform=None):
    """The tables of one call as a dict of NumPy arrays, per axis `a` in `y`, `x`:

    `near_a` (the four point methods), `first_a` and `w_a` (all but `nearest`), and for `cubic` and `lanczos` `fb_first_a` and
    `fb_w_a`, bilinear's tables, by which a cell with an incomplete window is computed.  `None` for a transform is the identity;
    `tables(method, src_shape, dst_shape, None, shape_transform(src_shape, dst_shape))` are the tables of `shape=`."""
    if method not in METHODS:
        raise ValueError(f"resample: method must be one of {METHODS}, not {method!r}")
    (sx, sy), (dx, dy) = axes_of(src_transform), axes_of(dst_transform)
    out = {}
    for a, n_src, n_dst, D, S in (("y", src_shape[0], dst_shape[0], dy, sy), ("x", src_shape[1], dst_shape[1], dx, sx)):
        if method in POINT_METHODS:
            out[f"near_{a}"] = near_table(n_src, n_dst, D, S)
            if method != "nearest":
                out[f"first_{a}"], out[f"w_{a}"] = interp_table(method, n_src, n_dst, D, S)
            if method in ("cubic", "lanczos"):
                out[f"fb_first_{a}"], out[f"fb_w_{a}"] = interp_table("bilinear", n_src, n_dst, D, S)
        else:
            out[f"first_{a}"], out[f"w_{a}"] = area_table(n_src, n_dst, D, S)
    if method == "mode" and out["w_y"].shape[1] * out["w_x"].shape[1] > MODE_MAX_WINDOW:
        raise ValueError(f"resample: a mode window of {out['w_y'].shape[1]} x {out['w_x'].shape[1]} source cells, more than "
                         f"{MODE_MAX_WINDOW}; resample in two steps")
    return out


def shape_transform(src_shape, dst_shape):
    """The destination transform of `shape=`: the same extent, `src / dst` source cells per destination cell, no offset."""
    return (src_shape[1] / dst_shape[1], 0.0, 0.0, 0.0, src_shape[0] / dst_shape[0], 0.0)


# ------------------------------------------------------------------ the call
def _check_shape(shape, what):
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"resample: {what} must be 2D with a shape of at least (1, 1)")
    rows, cols = (int(s) for s in shape)
    if rows * cols > MAX_CELLS or max(rows, cols) > MAX_AXIS:
        raise ValueError(f"resample: {rows} x {cols} cells exceed the 2**32 - 1 cells (2**31 - 1 along an axis) this backend "
                         "indexes; split your raster into smaller chunks.")
    return rows, cols


def _nodata_item(nodata, dtype):
    """`nodata` as one item of the raster's dtype, or None where no cell can equal it."""
    if nodata is None:
        return None
    try:
        item = check_fill(nodata, dtype)
    except ValueError:
        return None
    return None if item != item else item


def _shape_coords(agg, rows, cols):
    """`agg`'s coords stretched over (rows, cols) cells of the same extent, or None where they are not evenly spaced."""
    try:
        t = transform_from_coords(agg)
    except ValueError:
        return None
    ydim, xdim = agg.dims
    dx, dy = t[0] * (agg.shape[1] / cols), t[4] * (agg.shape[0] / rows)
    return {ydim: t[5] + dy * (np.arange(rows) + 0.5), xdim: t[2] + dx * (np.arange(cols) + 0.5)}


def _ptr(array):
    return None if array is None else array.ptr


def resample(agg, like=None, *, shape=None, method="bilinear", src_transform=None, dst_transform=None, nodata=None, fill=None,
             dtype=None, name=None):
    """
    Regrid `agg` onto another axis-aligned grid.

    Parameters
    ----------
    agg: DataArray
        2D, NumPy- or DeviceArray-backed, of any of the ten numeric dtypes.
        A sharded or dask raster raises NotImplementedError.

    like: DataArray, optional
        The destination grid: its shape, dims and coords.  Exactly one of
        `like` and `shape` must be given (ValueError otherwise).

    shape: (rows, cols), optional
        A destination of the same extent as `agg` with another cell size; no
        transforms are used.  The result's coords are `agg`'s, recomputed,
        where those are evenly spaced; otherwise it has none.

    method: str, default="bilinear"
        `nearest`, `bilinear`, `cubic`, `lanczos` (values at the cell centre),
        `average`, `sum`, `min`, `max`, `mode` (over the source cells that the
        destination cell overlaps).  Anything else raises ValueError.

    src_transform, dst_transform: sequence of 6 floats, optional
        Pixel to world, as `rasterize` takes it, with `like`.  Default:
        `transform_from_coords` of `agg` and of `like`.  Rotation or shear
        (t1, t3 != 0) raises ValueError; a scale of either sign is allowed.

    nodata: scalar, optional
        A source cell equal to it is invalid, as NaN cells are.

    fill: scalar, optional
        The value of a cell without data.  Default NaN for a float result,
        0 for an integer one.  Must be exactly representable in the result's
        dtype (ValueError otherwise).

    dtype: float64 or float32, optional
        Of the result of `bilinear`, `cubic`, `lanczos`, `average` and `sum`:
        default float32 for float32 input, else float64.  The sums are float64;
        the result is rounded once.  `nearest`, `min`, `max` and `mode` return
        the input's dtype (TypeError for another).

    name: str, optional
        Name of the result; default `agg`'s.

    Returns
    -------
    DataArray on the destination grid.  More than 256 source cells per
    destination cell along an axis, or a `mode` window of more than 1024
    cells, raises ValueError: resample in two steps.
    """
    if agg.ndim != 2:
        raise ValueError("resample: `agg` must be 2D")
    refuse_split_backends(agg, "resample")
    if (like is None) == (shape is None):
        raise ValueError("resample: give exactly one of `like` and `shape`")
    if method not in METHODS:
        raise ValueError(f"resample: method must be one of {METHODS}, not {method!r}")
    src_rows, src_cols = _check_shape(agg.shape, "`agg`")
    in_dtype = np.dtype(agg.dtype)
    if in_dtype not in DTYPE_CODE:
        raise TypeError(f"resample: unsupported dtype {in_dtype}")

    weighted = method in ("bilinear", "cubic", "lanczos", "average", "sum")
    if weighted:
        out_dtype = np.dtype(dtype) if dtype is not None else np.dtype(np.float32 if in_dtype == np.float32 else np.float64)
        if out_dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError(f"resample: dtype must be float64 or float32 for method {method!r}, not {out_dtype}")
    else:
        out_dtype = in_dtype
        if dtype is not None and np.dtype(dtype) != in_dtype:
            raise TypeError(f"resample: method {method!r} returns the input's dtype {in_dtype}, not {np.dtype(dtype)}")
    if fill is None:
        fill = np.nan if out_dtype.kind == "f" else 0
    try:
        fill_item = check_fill(fill, out_dtype)
    except ValueError:
        raise ValueError(f"resample: fill {fill!r} is not exactly representable in {out_dtype}") from None
    nodata_item = _nodata_item(nodata, in_dtype)

    if like is not None:
        if like.ndim != 2:
            raise ValueError("resample: `like` must be 2D")
        refuse_split_backends(like, "resample")
        rows, cols = _check_shape(like.shape, "`like`")
        S = src_transform if src_transform is not None else transform_from_coords(agg)
        D = dst_transform if dst_transform is not None else transform_from_coords(like)
        dims, coords = like.dims, like.coords
    else:
        if src_transform is not None or dst_transform is not None:
            raise ValueError("resample: `shape=` keeps the extent of `agg` and takes no transforms")
        rows, cols = _check_shape(tuple(shape), "`shape`")
        S, D = None, shape_transform((src_rows, src_cols), (rows, cols))
        dims, coords = agg.dims, _shape_coords(agg, rows, cols)
    tab = tables(method, (src_rows, src_cols), (rows, cols), S, D)

    _lib.require_device()
    stream = get_stream()
    src, like_numpy = resident(agg.data, stream)
    dev = {key: DeviceArray.from_numpy(value, stream=stream) for key, value in tab.items()}
    out = DeviceArray((rows, cols), out_dtype)
    nodata_buf = None if nodata_item is None else np.array([nodata_item], dtype=in_dtype)
    nodata_ptr = None if nodata_buf is None else nodata_buf.ctypes.data
    fill_buf = np.array([fill_item], dtype=out_dtype)
    head = (src.ptr, DTYPE_CODE[in_dtype], src_rows, src_cols, nodata_ptr, rows, cols)
    if method == "nearest":
        _lib.call("xrs_resample_gather", *head, dev["near_y"].ptr, dev["near_x"].ptr, fill_buf.ctypes.data, out.ptr, stream)
    elif weighted:
        taps = (dev["first_y"].ptr, dev["w_y"].ptr, tab["w_y"].shape[1], dev["first_x"].ptr, dev["w_x"].ptr, tab["w_x"].shape[1])
        fb = "fb_w_y" in tab
        _lib.call("xrs_resample_weighted", *head, *taps, _ptr(dev.get("near_y")), _ptr(dev.get("near_x")),
                  _ptr(dev.get("fb_first_y")), _ptr(dev.get("fb_w_y")), 2 if fb else 0,
                  _ptr(dev.get("fb_first_x")), _ptr(dev.get("fb_w_x")), 2 if fb else 0,
                  int(method != "sum"), DTYPE_CODE[out_dtype], float(fill_item), out.ptr, stream)
    else:
        _lib.call("xrs_resample_select", *head, dev["first_y"].ptr, dev["w_y"].ptr, tab["w_y"].shape[1], dev["first_x"].ptr,
                  dev["w_x"].ptr, tab["w_x"].shape[1], SELECT_OP[method], fill_buf.ctypes.data, out.ptr, stream)
    result = finish(out, like_numpy)
    settle(stream, like_numpy)                                    # the tables go back to the pool
    del dev, src
    return DataArray(result, name=agg.name if name is None else name, coords=coords, dims=dims, attrs=agg.attrs)


# `from xrspatial_amd import resample` binds the function over the module's name in the package; the table builders stay
# reachable through it
resample.tables = tables
resample.shape_transform = shape_transform
resample.near_table = near_table
resample.interp_table = interp_table
resample.area_table = area_table
resample.METHODS = METHODS

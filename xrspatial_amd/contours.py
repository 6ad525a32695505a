"""contours: the isolines of a raster at given levels.  The reference has no contours; the rule is written down in DESIGN.md
§6s and computed by csrc/contours.hip, so that the result is a function of the input, bit for bit.

Node (r, c) is the centre of cell (r, c), at pixel position (c + 0.5, r + 0.5) (polygonize's convention: the cell is the square
[c, c + 1] x [r, r + 1]).  A node is high at a level when z > level (matplotlib's and contourpy's choice); a quad of four
neighbouring nodes with a corner that is not finite draws nothing.  With x to the right and rows increasing downward the high
nodes lie to the right of the direction of travel.  A closed line begins at its smallest edge id and repeats that point at its
end; an open line begins where it enters the raster or leaves a quad that drew nothing.  The lines of a level are ordered by
their first edge id.  Points where a node equals a level coincide and are kept.

`return_type="numpy"` gives `(levels, lines)`: the float64 levels used and, per level, a list of `(n, 2)` float64 arrays.
`return_type="flat"` gives `(levels, points, line_offsets, level_offsets, closed)`: points is float64 `[N, 2]`; line i owns
`points[line_offsets[i]:line_offsets[i + 1]]`; level k owns lines `level_offsets[k]:level_offsets[k + 1]`; `closed[i]` is 1 for a
ring.  The lists of `"numpy"` are views of that one points array.

NumPy- and DeviceArray-backed rasters of the ten XRS_DT_* dtypes are accepted; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import math
import numbers

import numpy as np

from . import _lib
from ._launch import get_stream, refuse_split_backends, resident, settle, workspace
from .device import DTYPE_CODE, DeviceArray
from .experimental.polygonize import _free_bytes

MAX_CELLS = (1 << 31) - 1            # XRS_CONTOURS_MAX_CELLS: an edge id, two per cell, is a 32-bit word
MAX_LEVELS = 1 << 22                 # XRS_CONTOURS_MAX_LEVELS
MAX_SEGMENTS = (1 << 32) - 2         # XRS_CONTOURS_MAX_SEGMENTS: 32-bit segment ids, one value kept for "none"
_RETURN_TYPES = ("numpy", "flat")


def check_levels(levels):
    """`levels` as a float64 array: finite and strictly increasing, or ValueError."""
    try:
        out = np.array(levels, dtype=np.float64).reshape(-1) if np.ndim(levels) <= 1 else None
    except (TypeError, ValueError):
        out = None
    if out is None:
        raise ValueError("contours: levels must be a sequence of numbers or an int")
    if not np.all(np.isfinite(out)):
        raise ValueError("contours: every level must be finite")
    if np.any(np.diff(out) <= 0):
        raise ValueError("contours: the levels must be strictly increasing")
    if len(out) > MAX_LEVELS:
        raise ValueError(f"contours: {len(out)} levels, at most {MAX_LEVELS}")
    return np.ascontiguousarray(out)


def interior_levels(lo, hi, n):
    """The n levels lo + (k + 1) * ((hi - lo) / (n + 1)), k = 0 .. n - 1, in float64, every operation rounded on its own."""
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(all="ignore"):
        step = (hi - lo) / np.float64(n + 1)
        return np.array([lo + np.float64(k + 1) * step for k in range(n)], np.float64)


def _finite_range(dev):
    """(count, min, max) of the finite cells of a resident raster, found on the device."""
    from .classify import _Stats
    if dev.size == 0:
        return 0, math.nan, math.nan
    count, lo, hi, _ = _Stats(dev).moments()
    return count, lo, hi


def assemble(points, line_offsets, level_offsets):
    """Per level, the list of its lines; every line is a view of `points`."""
    lo = [int(v) for v in line_offsets]
    lines = [points[lo[i]:lo[i + 1]] for i in range(len(lo) - 1)]
    ko = [int(v) for v in level_offsets]
    return [lines[ko[k]:ko[k + 1]] for k in range(len(ko) - 1)]


def _empty(n_levels):
    return (np.empty((0, 2), np.float64), np.zeros(1, np.int64), np.zeros(n_levels + 1, np.int64), np.empty(0, np.uint8))


def flat(values, levels, transform=None, stats=None):
    """(levels, points, line_offsets, level_offsets, closed) as NumPy arrays.  `values`: a NumPy array or a DeviceArray; `levels`:
    a sequence or an int.  `stats`: a dict that receives the counts and the rounds of the three calls."""
    dtype = np.dtype(values.dtype)
    if dtype == np.bool_:
        values, dtype = values.view(np.uint8) if isinstance(values, np.ndarray) else values, np.dtype(np.uint8)
    if dtype not in DTYPE_CODE:
        raise TypeError(f"contours: unsupported raster dtype {dtype}")
    rows, cols = (int(s) for s in values.shape)
    if rows * cols > MAX_CELLS:
        raise ValueError(f"contours: {rows} x {cols} cells exceed the 2**31 - 1 cells this backend indexes; "
                         "split your raster into smaller chunks.")
    by_count = isinstance(levels, numbers.Integral) and not isinstance(levels, bool)
    if by_count:
        if levels < 1:
            raise ValueError(f"contours: levels={levels}: the number of levels must be at least 1")
        if levels > MAX_LEVELS:
            raise ValueError(f"contours: {levels} levels, at most {MAX_LEVELS}")
    else:
        levels = check_levels(levels)
    _lib.require_device()
    stream = get_stream()
    dev = None
    if by_count:
        dev, _ = resident(values, stream)
        count, lo, hi = _finite_range(dev)
        if count == 0:
            raise ValueError("contours: the raster has no finite cell to take levels from")
        made = interior_levels(lo, hi, int(levels))
        if not np.all(np.isfinite(made)) or np.any(np.diff(made) <= 0) or (len(made) and not made[0] > lo):
            raise ValueError(f"contours: {int(levels)} levels between {lo} and {hi} do not come out strictly increasing")
        levels = made
    n_levels = len(levels)
    if stats is not None:
        stats.update(levels=n_levels, segments=0, lines=0, points=0, leader_rounds=0, rank_rounds=0)
    if n_levels == 0 or rows < 2 or cols < 2:
        return (levels,) + _empty(n_levels)
    if dev is None:
        dev, _ = resident(values, stream)
    code = DTYPE_CODE[dtype]
    work = workspace("contours", rows, cols, n_levels)
    n_segments = ctypes.c_uint64(0)
    _lib.call("xrs_contours_census", dev.ptr, code, rows, cols, levels.ctypes.data, n_levels, work.ptr, ctypes.byref(n_segments), stream)
    n_segments = int(n_segments.value)
    if stats is not None:
        stats.update(segments=n_segments)
    if n_segments == 0:
        return (levels,) + _empty(n_levels)
    if n_segments > MAX_SEGMENTS:
        raise ValueError(f"contours: {n_segments} segments exceed the {MAX_SEGMENTS} (2**32 - 2) this backend ranks; "
                         "use fewer levels or split your raster into smaller chunks.")
    line_bytes = _lib.workspace_bytes("contours_lines", n_segments)
    # the line workspace, then at most one line per segment: its sort records, its points and its offsets
    need = line_bytes + n_segments * (24 + 8 + 32 + 9) + (n_levels + 1) * 8
    free = _free_bytes()
    if need > free:
        raise MemoryError(f"contours: {n_segments} segments need up to {need} bytes of device memory, {free} are free; "
                          "use fewer levels or split your raster into smaller chunks.")
    lines = DeviceArray((line_bytes,), np.uint8)
    n_lines, n_points = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rounds = (ctypes.c_int * 2)()
    _lib.call("xrs_contours_lines", dev.ptr, code, rows, cols, n_levels, work.ptr, lines.ptr, n_segments, ctypes.byref(n_lines),
              ctypes.byref(n_points), rounds, stream)
    n_lines, n_points = int(n_lines.value), int(n_points.value)
    if stats is not None:
        stats.update(lines=n_lines, points=n_points, leader_rounds=int(rounds[0]), rank_rounds=int(rounds[1]))
    sort = workspace("contours_scatter", n_lines)
    points = DeviceArray((n_points, 2), np.float64)
    line_offsets = DeviceArray((n_lines + 1,), np.int64)
    level_offsets = DeviceArray((n_levels + 1,), np.int64)
    closed = DeviceArray((n_lines,), np.uint8)
    tf = None
    if transform is not None:
        tf = (ctypes.c_double * 6)(*[float(v) for v in transform])
    _lib.call("xrs_contours_scatter", dev.ptr, code, rows, cols, n_levels, work.ptr, lines.ptr, sort.ptr, n_segments, n_lines, tf,
              points.ptr, line_offsets.ptr, level_offsets.ptr, closed.ptr, stream)
    out = (levels, points.get(stream), line_offsets.get(stream), level_offsets.get(stream), closed.get(stream))
    settle(stream)                                       # the workspaces go back to the pool
    return out


def contours(agg, levels, *, transform=None, return_type="numpy"):
    """
    Contour lines (isolines) of a raster at the given levels, by marching
    squares over the cell centres.  The result is a function of the input,
    bit for bit.

    Parameters
    ----------
    agg: DataArray
        2D, NumPy- or DeviceArray-backed, of any of the ten XRS_DT_* dtypes.
        Cells that are not finite (NaN, inf) draw nothing: neither do the
        four quads around them.

    levels: sequence of floats, or int
        A sequence: K >= 0 finite values, strictly increasing.  An int
        n >= 1: the n interior levels lo + (k + 1) * ((hi - lo) / (n + 1)),
        k = 0 .. n - 1, between the minimum and maximum of the finite cells.

    transform: sequence of 6 floats, optional
        Pixel to world, as `polygonize` takes it: x' = t0 * x + t1 * y + t2,
        y' = t3 * x + t4 * y + t5 for the pixel position (x, y); the centre
        of cell (r, c) is at (c + 0.5, r + 0.5).  See
        `transform_from_coords`.

    return_type: str, default="numpy"
        "numpy": (levels, lines): the float64 levels and, per level, a list
        of (n, 2) float64 arrays.  "flat": (levels, points, line_offsets,
        level_offsets, closed) as five arrays (module docstring).

    Returns
    -------
    NumPy arrays in the format `return_type` names, whatever backs `agg`.
    """
    if agg.ndim != 2:
        raise ValueError("contours: the raster must be 2D")
    refuse_split_backends(agg, "contours")
    if transform is not None:
        transform = np.asarray(transform)
        if transform.ndim != 1 or len(transform) != 6:
            raise ValueError(f"Incorrect transform length of {transform.size} instead of 6")
    if return_type not in _RETURN_TYPES:
        raise ValueError(f"Invalid return_type '{return_type}'")
    result = flat(agg.data, levels, transform)
    if return_type == "flat":
        return result
    return result[0], assemble(*result[1:4])

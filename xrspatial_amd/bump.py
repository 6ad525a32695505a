"""bump: the reference's bump map (xrspatial/bump.py), bit for bit.

The locations are the reference's own NumPy lines -- two `np.random.choice` draws on the global state, stored as uint16 -- and
`height_func` is called on that array.  The loop over the bumps (`_finish_bump`) is serial and order dependent in the reference;
the device runs it as sorted (cell, bump) events folded in passes (csrc/bump.hip) and returns every cell's float64
sum in the reference's order.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
import operator

import numpy as np

from . import _lib
from ._launch import get_stream
from ._xr import DataArray
from .device import DeviceArray

MAX_CELLS = 1 << 31                       # xrs_bump_f64: the cell number is 31 bits of an event key
DEFAULT_MAX_EVENTS = 1 << 27              # events of one chunk: 16 bytes of sort keys and 4 of cursor each, ~2.7 GB of workspace
STATUS_WORDS = ("chunks", "events", "passes", "touched_cells", "expand_ns", "sort_ns", "fold_ns")


def _heights_f64(heights, count):
    """`heights` as the float64 the reference's `out[y, x] + z` makes of it; ValueError unless it is `count` numbers."""
    try:
        z = np.asarray(heights)
        if z.dtype.kind not in "biuf":
            raise TypeError(z.dtype)
        z = np.ascontiguousarray(z, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"bump: heights must be numbers ({e})") from None
    if z.ndim != 1 or z.shape[0] != count:
        raise ValueError(f"bump: {count} heights are needed, one per location; got shape {z.shape}")
    return z


def _locs_u16(locs):
    locs = np.asarray(locs)
    if locs.ndim != 2 or locs.shape[1] != 2 or locs.dtype.kind not in "iu":
        raise ValueError("bump: locations are a (count, 2) integer array of (x, y)")
    if locs.dtype != np.uint16:
        if locs.size and (locs.min() < 0 or locs.max() > 65535):
            raise ValueError("bump: locations are uint16 in the reference: 0 .. 65535")
        locs = locs.astype(np.uint16)
    return np.ascontiguousarray(locs)


def finish_bump(width, height, locs, heights, spread, device=False, *, max_events=None, status=None):
    """`_finish_bump` of the reference for given locations ((count, 2) of (x, y)) and heights: the (height, width) float64 plane,
    as a NumPy array or, for `device=True`, a DeviceArray.

    `max_events` caps the events of one chunk (default 2^27; bumps are processed in index-order chunks that fit), and `status`,
    a dict, receives the call's status words (STATUS_WORDS)."""
    width, height, spread = operator.index(width), operator.index(height), operator.index(spread)
    if width < 1 or height < 1:
        raise ValueError(f"bump: width and height must be at least 1 ({width} x {height})")
    if width * height > MAX_CELLS:
        raise ValueError(f"bump: at most 2^31 cells ({width} x {height})")
    locs = _locs_u16(locs)
    count = locs.shape[0]
    z = _heights_f64(heights, count)
    max_events = DEFAULT_MAX_EVENTS if max_events is None else operator.index(max_events)
    _lib.require_device()
    stream = get_stream()
    nbytes = _lib.workspace_bytes("bump", count, width, height, spread, max_events)
    out = DeviceArray((height, width), np.float64)
    # (a workspace of 0 bytes: the call refuses the arguments and says why)
    work = DeviceArray((max(nbytes, 256),), np.uint8)
    locs_d = DeviceArray.from_numpy(locs, stream=stream) if count else None
    z_d = DeviceArray.from_numpy(z, stream=stream) if count else None
    words = (ctypes.c_int64 * 8)()
    _lib.call("xrs_bump_f64", locs_d.ptr if count else None, z_d.ptr if count else None, count, width, height, spread, out.ptr,
              work.ptr, nbytes, max_events, words, stream)
    if status is not None:
        status.update(zip(STATUS_WORDS, (int(w) for w in words)))
    return out if device else out.get(stream)


def bump(width, height, count=None, height_func=None, spread=1):
    """Bump map of `count` bumps (default: width * height // 10) at random locations of a width x height raster, each of height
    `height_func(locations)[i]` (default: 1) spread over `spread` cells.  Same signature, random draws and result as
    `xrspatial.bump`: a NumPy-backed float64 DataArray with dims ['y', 'x'] and attrs {'res': 1}."""
    if count is None:
        count = width * height // 10
    if width < 1 or height < 1 or count < 0:
        raise ValueError(f"bump: width and height of at least 1 and a count of at least 0 are needed "
                         f"({width} x {height}, count {count})")
    if width * height > MAX_CELLS:
        raise ValueError(f"bump: at most 2^31 cells ({width} x {height})")
    _lib.require_device()                 # (before the draws: a call that cannot run leaves NumPy's global state alone)
    if height_func is None:
        height_func = lambda bumps: np.ones(len(bumps))  # noqa: E731
    linx = range(width)
    liny = range(height)
    # the reference's lines (bump.py:207-209): two draws on the global state, wrapped to uint16
    locs = np.empty((count, 2), dtype=np.uint16)
    locs[:, 0] = np.random.choice(linx, count)
    locs[:, 1] = np.random.choice(liny, count)
    heights = height_func(locs)
    bumps = finish_bump(width, height, locs, heights, spread)
    return DataArray(bumps, dims=['y', 'x'], attrs=dict(res=1))


# `from xrspatial_amd import bump` is this function, as in the reference, and hides the module of the same name: the
# deterministic entry stays reachable as xrspatial_amd.bump.finish_bump
bump.finish_bump = finish_bump

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
the calls run eagerly.  There is no CPU fallback.

stream_order, stream_link, watershed, flow_length (csrc/streams.hip; stated in NumPy by tests/streams_oracle.py).
`flow_dir` is a raster of codes as above and rules 1-3, 6 and 7 hold for it; all rasters of a call have one shape.

The stream graph (stream_order, stream_link):
  1. `flow_accum` is read in place when float32 or float64; any other numeric dtype is cast to float64 on the host;
  2. `threshold` is a float64; NaN raises ValueError;
  3. a stream cell is a cell with a non-NaN code and float64(flow_accum) >= threshold; a NaN accumulation is no stream cell;
  4. the stream parent of a stream cell u is its downstream cell if that is a stream cell, else u has none: with a user's
     accumulation a stream may end inside the raster and another begin below it;
  5. children(v) = the stream cells whose stream parent is v; a source has none, a junction two or more;
  6. method='shreve': the number of sources in v's upstream stream tree, v included (exact below 2^32);
  7. method='strahler': 1 at a source; elsewhere, with m the largest order among the children, m + 1 if at least two children
     have order m, else m;
  8. stream_order is float64 for both methods, NaN at every cell that is no stream cell;
  9. stream_link: head(u) = u if u has 0 or >= 2 children, else head(child);
 10. the link value at u is 1 + the number of heads whose linear index row * W + col is below head(u)'s: dense ids 1 .. L in
     row-major order of the heads; a junction cell opens the link below it;
 11. stream_link is float64, NaN off the streams.
The cycle test of rule 6 above runs on the stream cells, where the work is: a ring of stream cells raises ValueError, a ring
that lies wholly off the streams touches no result and is not looked for.

watershed:
  1. a pour point is a cell that is a target of `pour_points` by `proximity`'s rule (`target_values` empty: non-zero and finite;
     otherwise equal to one of them, compared as `proximity.target_array` says) and whose code is not NaN;
  2. for a cell u with a non-NaN code, walk u, down(u), .. to the outlet: the result is float32(pour_points[p]) of the first
     pour point p met, u itself included (the conversion `cost_allocation` makes), NaN if none is met;
  3. NaN at NaN cells; nested pour points split a basin;
  4. `pour_points`: the ten XRS_DT_* dtypes are read in place, bool and float16 widened on the host as `proximity` does.
A cycle that holds a pour point is cut there and raises nothing; any other cycle raises.

flow_length:
  1. cx, cy, dg = cell_distances(flow_dir);
  2. nx, ny, nd = the numbers of E/W, N/S and diagonal steps on the path from u to its outlet; the outlet's own code is no step;
  3. the result is fl(fl(fl(nx * cx) + fl(ny * cy)) + fl(nd * dg)) in float64, the counts converted exactly, never fused;
  4. 0.0 at outlets, NaN at NaN cells.
This is the length by step counts: the counts are integers, so the value depends on the order of nothing; it lies within a few
ulp of the sum taken step by step along the path and is not equal to it.

flow_direction(method='dinf'), flow_accumulation(method='dinf' | weights=..): Tarboton's D-infinity and the accumulation of float
shares (csrc/flow_frac.hip; stated in NumPy by tests/dinf_oracle.py).

Neighbours and the table.  The neighbours counter-clockwise from east are n = 0 .. 7: E (0, +1), NE (-1, +1), N (-1, 0),
NW (-1, -1), W (0, -1), SW (+1, -1), S (+1, 0), SE (+1, +1); their D8 codes are 1, 128, 64, 32, 16, 8, 4, 2.  With cx, cy as
above the host computes td = np.arctan2(cy, cx) and b[0 .. 8] = 0, td, pi/2, pi - td, pi, pi + td, 3 pi/2, 2 pi - td, 2 pi in
float64 and passes the table by value: b[n] is neighbour n's angle, in radians counter-clockwise from east (north is
drow = -1).  A table that does not increase strictly (extreme cell-size ratios) raises ValueError, for 'dinf' only.

The direction from elevations (float64 angles in [0, 2 pi); -1.0 at a non-NaN cell with no direction; NaN at NaN cells):
  1. D8's winner exactly as rules 1-4 of flow_direction find it: `best` (the drop) and its neighbour; with none see 4;
  2. bestq = fl(best * best), angle = b[winner];
  3. for each facet o = 0 .. 7, between the neighbours o and (o + 1) % 8: the cardinal neighbour is the even one, at d1 (cx for
     E / W, cy for N / S), d2 the other cell size; s1 = (z - z_card) / d1, s2 = (z_card - z_diag) / d2, each one IEEE
     subtraction and one division in float64; the facet has an interior candidate iff s1 > 0, s2 > 0 and
     fl(s2 * d1) < fl(s1 * d2) (all false on NaN); its weight is q = fl(fl(s1 * s1) + fl(s2 * s2)), taken iff q > bestq
     (strict: ties keep what is there), and then bestq = q, r = atan2(s2, s1) and the angle is b[o] + r for even o,
     b[o + 1] - r for odd o, clamped to [b[o], b[o + 1]]; a result of b[8] becomes 0.0.  Squares that underflow or overflow
     leave the D8 winner in place: a cell has a direction exactly where its D8 code is not 0;
  4. a cell with no D8 winner gets -1.0; with resolve_flats=True it gets b[n] of the code that flow_direction(resolve_flats=True)
     gives it (the same two kernels, unchanged), -1.0 if that code is still 0.
Which candidate wins takes exact operations only; an interior angle goes through atan2, whose last bits are the library's.
No cycle: an interior candidate has s1 > 0 and s2 > 0, so both receivers lie strictly lower; a single receiver lies strictly
lower (its drop is > 0); a flat cell's receiver has equal height and a smaller count d.  Height never rises along a path and,
among equal heights, d falls strictly.

Decoding a direction raster for the accumulation.  A D8 code has one receiver with share 1.0, and a value that is no code is
refused as above.  An angle a (float64; any other numeric dtype is cast to float64 on the host): NaN is outside the graph;
-1.0 has no receiver; any other value must lie in [0, 2 pi), else ValueError (found on the device, raised before a result is
returned).  With o such that b[o] <= a < b[o + 1], neighbour o gets share_lo = (b[o + 1] - a) / (b[o + 1] - b[o]) and neighbour
(o + 1) % 8 gets share_hi = (a - b[o]) / (b[o + 1] - b[o]), each its own subtraction and division; a share that is not > 0 is
no edge.  A receiver outside the raster or at a NaN cell loses the water.

The accumulation (float64).  acc[v] = w[v], then for the donors u of v in the order of their positions around v -- E, SE, S,
SW, W, NW, N, NE -- acc = fl(acc + fl(share(u -> v) * acc[u])).  w is 1.0, or with `weights` the cell's weight (float32 and
float64 read in place, any other numeric dtype cast to float64 on the host); NaN and inf are ordinary values.  A cell is
computed once, when all its donors are final: the result is a function of the direction raster and the weights alone,
whatever the order of the launches, and the tests compare it bit for bit.  When a round makes no cell final and non-NaN cells
are left, those cells lie on or below a cycle: ValueError with their number.  More than 2^32 - 2 cells raise ValueError.
flow_accumulation(method='d8') without weights is the count of rule 4 above, by the same code as before.

Not built: multiple flow directions (MFD), which need eight share planes; the wetness index; upstream (longest) flow length,
which is a maximum over float sums; HAND; snapping of pour points.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, resident, settle, widened, workspace
from ._xr import DataArray
from .dataset_support import supports_dataset
from .device import DTYPE_CODE, FLOAT_SUFFIX, DeviceArray, to_device_f32
from .proximity import target_array, widen
from .utils import get_dataarray_resolution

ACCUMULATION, BASINS = 1, 2             # XRS_FLOW_ACCUMULATION / XRS_FLOW_BASINS
INVALID_CODE, CYCLE = 1, 2              # XRS_FLOW_INVALID_CODE / XRS_FLOW_CYCLE (status word 1)
TIMED = 1                               # XRS_FLOW_TIMED
STATUS_WORDS = 80
MAX_CELLS = 2 ** 32 - 2
CODES = (0, 1, 2, 4, 8, 16, 32, 64, 128)
TILE = 64                               # XRS_FILL_TILE: the tile edge of the fill / flat relaxer
FILL_STATUS_WORDS, FILL_STATUS_ROUNDS = 256, 80     # XRS_FILL_STATUS_WORDS / XRS_FILL_STATUS_ROUNDS
STRAHLER, SHREVE, LINK = 1, 2, 4        # XRS_STREAM_STRAHLER / XRS_STREAM_SHREVE / XRS_STREAM_LINK
STREAM_STATUS_WORDS = 136               # XRS_STREAM_STATUS_WORDS
# xrs_stream_network's status words (beside [0] rounds and [1] the bits above)
STREAM_LEVELS, STREAM_CELLS, STREAM_SOURCES, STREAM_HEADS, STREAM_HEAD_ROUNDS = 2, 3, 4, 5, 6
STREAM_NS, STREAM_LIVE, STREAM_JOINTS, STREAM_LEVEL_ROUNDS = 8, 16, 56, 96
POUR_POINTS = 37                        # xrs_flow_watershed's status word
D8, DINF = 0, 1                         # XRS_FLOW_D8 / XRS_FLOW_DINF
METHODS = {'d8': D8, 'dinf': DINF}
FRAC_STATUS_WORDS = 256                 # XRS_FRAC_STATUS_WORDS: relax_rounds' layout and the three words below
FRAC_BITS, FRAC_LEFT, FRAC_GRAPH = 4, 5, 6
NEIGHBOUR_CODES = (1, 128, 64, 32, 16, 8, 4, 2)     # the D8 code of neighbour n = 0 .. 7, counter-clockwise from east


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
def _check_method(method, what):
    if method not in METHODS:
        raise ValueError(f"{what}: method must be 'd8' or 'dinf', got {method!r}")


def resolve_flats_plane(src: DeviceArray, codes: DeviceArray, flags: int = 0, stream=None):
    """xrs_flow_flats: the codes of xrs_flow_direction for the resident plane `src`, updated in place; the status words."""
    rows, cols = src.shape
    status = (ctypes.c_int64 * FILL_STATUS_WORDS)()
    if rows * cols:
        work = workspace("flow_flats", rows, cols)
        _lib.call("xrs_flow_flats", src.ptr, DTYPE_CODE[src.dtype], rows, cols, codes.ptr, work.ptr, status, flags, stream)
    return [int(w) for w in status]


def angle_table(cx, cy):
    """b[0 .. 8] of the D-infinity rule: the angles of the neighbours n = 0 .. 7 (E, NE, N, NW, W, SW, S, SE), counter-clockwise
    from east in radians, and 2 pi, as a float64 array.  ValueError where they do not increase strictly."""
    cx, cy = np.float64(cx), np.float64(cy)
    td, pi = np.arctan2(cy, cx), np.float64(np.pi)
    b = np.array([0.0, td, pi / 2, pi - td, pi, pi + td, 3 * pi / 2, 2 * pi - td, 2 * pi], np.float64)
    if not (np.isfinite(b).all() and (np.diff(b) > 0).all()):
        raise ValueError(f"method='dinf': the cell sizes ({cx}, {cy}) leave no room between the neighbours' angles {b.tolist()}")
    return b


def _c_table(table):
    return (ctypes.c_double * 9)(*[float(v) for v in table])


def dinf_direction_plane(src: DeviceArray, cx, cy, dg, table, codes: DeviceArray = None, stream=None):
    """xrs_flow_direction_dinf on a resident float32 / float64 plane: the float64 angles.  `codes`: the resolved D8 codes."""
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float64)
    if rows * cols:
        _lib.call("xrs_flow_direction_dinf", src.ptr, DTYPE_CODE[src.dtype], rows, cols, cx, cy, dg, _c_table(table),
                  codes.ptr if codes is not None else None, out.ptr, stream)
    return out


def _run_direction_dinf(data, cx, cy, dg, table, resolve_flats):
    _lib.require_device()
    stream = get_stream()
    src, like_numpy = resident(data, stream, FLOAT_SUFFIX, np.float64)
    rows, cols = src.shape
    codes = None
    if resolve_flats and rows * cols:                                    # the two D8 kernels, unchanged, then the angles
        codes = DeviceArray((rows, cols), np.float32)
        _lib.call("xrs_flow_direction", src.ptr, DTYPE_CODE[src.dtype], rows, cols, cx, cy, dg, codes.ptr, stream)
        resolve_flats_plane(src, codes, stream=stream)
    out = dinf_direction_plane(src, cx, cy, dg, table, codes, stream)
    if rows * cols and (src is not data or resolve_flats):
        settle(stream, like_numpy)                                       # the widened copy, the codes and the workspace go back to the pool
    return finish(out, like_numpy)


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
def flow_direction(agg: DataArray, name: str = 'flow_direction', resolve_flats: bool = False, method: str = 'd8') -> DataArray:
    """D8 flow direction: for every cell the ESRI code (E 1, SE 2, S 4, SW 8, W 16, NW 32, N 64, NE 128) of the neighbour with
    the steepest drop, 0 where no neighbour lies lower, NaN at NaN cells (the rule: module docstring).

    method='dinf': Tarboton's D-infinity instead -- the float64 angle of steepest descent over the eight triangular facets, in
    radians counter-clockwise from east (north is the row above) in [0, 2 pi), -1.0 where D8 gives 0, NaN at NaN cells; with
    resolve_flats a flat cell gets the angle of the neighbour its D8 code names.  Any other method raises ValueError.

    agg: 2-D DataArray of elevations (or a Dataset: every variable on its own), NumPy- or DeviceArray-backed (the result's
    backend); the cell size comes from `attrs['res']` or the coordinates, as for `slope`.  resolve_flats: give every cell of a
    level area that has a drained cell the code of the neighbour one step nearer to it (on `fill(agg)` every path then ends at
    the rim of the raster).  Returns a float32 DataArray (float64 for 'dinf') with agg's coords, dims and attrs."""
    _check_method(method, 'flow_direction')
    refuse_split_backends(agg, 'flow_direction')
    rows, cols = _check_raster(agg.data, 'flow_direction')
    cx, cy, dg = cell_distances(agg) if rows * cols else (1.0, 1.0, float(np.sqrt(2.0)))
    if method == 'dinf':
        out = _run_direction_dinf(agg.data, cx, cy, dg, angle_table(cx, cy), bool(resolve_flats))
    else:
        out = _run_direction(agg.data, cx, cy, dg, bool(resolve_flats))
    return DataArray(out, name=name, coords=agg.coords, dims=agg.dims, attrs=agg.attrs)


# ------------------------------------------------------------------ flow_accumulation, basins
def _raise_for(words):
    """ValueError for the status bits every graph call shares (word 1; word 0: the rounds run)."""
    if words[1] & INVALID_CODE:
        raise ValueError("flow direction raster holds a value that is not one of the D8 codes 0, 1, 2, 4, 8, 16, 32, 64, 128")
    if words[1] & CYCLE:
        raise ValueError(f"flow direction raster contains a cycle (pointers still live after {words[0]} doubling rounds)")


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
    _raise_for(words)
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


def frac_plane(src: DeviceArray, method: int, table=None, weights: DeviceArray = None, flags: int = 0, stream=None):
    """xrs_flow_accumulate_frac on a resident plane of D8 codes (float32, method D8) or of angles (float64, DINF, with `table`):
    (the float64 accumulation, status words).  `weights`: a float32 / float64 plane or None.  Raises ValueError for a value that
    is no direction and for a cycle."""
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float64)
    status = (ctypes.c_int64 * FRAC_STATUS_WORDS)()
    if rows * cols:
        work = workspace("flow_accumulate_frac", rows, cols)
        _lib.call("xrs_flow_accumulate_frac", src.ptr, method, _c_table(table) if method == DINF else None,
                  weights.ptr if weights is not None else None, DTYPE_CODE[weights.dtype] if weights is not None else 0, rows, cols,
                  work.ptr, out.ptr, status, flags, stream)                 # (waits for the stream: the status words)
    words = [int(w) for w in status]
    if words[FRAC_BITS] & INVALID_CODE:
        raise ValueError("flow direction raster holds a value that is not one of the D8 codes 0, 1, 2, 4, 8, 16, 32, 64, 128"
                         if method == D8 else "flow direction raster holds a value that is no angle in [0, 2 pi), -1.0 or NaN")
    if words[FRAC_BITS] & CYCLE:
        raise ValueError(f"flow direction raster contains a cycle: {words[FRAC_LEFT]} cells lie on or below one (no cell became "
                         f"final in round {words[0]})")
    return out, words


def _run_frac(flow_dir, weights, method):
    rows, cols = (int(n) for n in flow_dir.data.shape)
    table = None
    if method == 'dinf':
        cx, cy, _ = cell_distances(flow_dir) if rows * cols else (1.0, 1.0, 0.0)
        table = angle_table(cx, cy)
    _lib.require_device()
    stream = get_stream()
    if method == 'dinf':
        src, _ = resident(flow_dir.data, stream, {np.dtype(np.float64): "f64"}, np.float64)
    else:
        src = to_device_f32(flow_dir.data)
    wts = None
    if weights is not None:
        wts, _ = resident(weights.data, stream, FLOAT_SUFFIX, np.float64)     # staged on its own, as cost_distance's friction
    out, _ = frac_plane(src, METHODS[method], table, wts, stream=stream)
    return finish(out, not isinstance(flow_dir.data, DeviceArray))      # flow_dir's backend, whatever the weights' is


@supports_dataset
def flow_accumulation(flow_dir: DataArray, name: str = 'flow_accumulation', method: str = 'd8', weights: DataArray = None) -> DataArray:
    """For every cell the number of cells whose D8 flow path reaches it, itself included; NaN at NaN cells.

    flow_dir: 2-D DataArray of D8 codes as `flow_direction` returns them (or a Dataset: every variable on its own), NumPy- or
    DeviceArray-backed (the result's backend).  A value that is no code, or a cycle, raises ValueError.

    method='dinf': flow_dir holds the angles of `flow_direction(method='dinf')` instead (NaN: outside the graph; -1.0: no
    receiver; else in [0, 2 pi), anything else raises ValueError); a cell's water is split between the two neighbours its angle
    lies between, in proportion to the angles; the cell size comes from `attrs['res']` or the coordinates.  weights: a DataArray
    of flow_dir's shape (any numeric dtype, read as float64; staged on its own) with every cell's own contribution in place
    of 1.0, for both methods; NaN and inf are ordinary values.  With a method other than 'd8' or with weights the result is the
    gather of the module docstring, a sum of floats in a fixed order.  Returns a float64 DataArray with flow_dir's coords, dims
    and attrs."""
    _check_method(method, 'flow_accumulation')
    if method == 'd8' and weights is None:
        return _graph_product(flow_dir, name, 'flow_accumulation', ACCUMULATION)
    if weights is None:
        refuse_split_backends(flow_dir, 'flow_accumulation')
        _check_raster(flow_dir.data, 'flow_accumulation')
    else:
        _check_pair(flow_dir, weights, "weights", 'flow_accumulation')
    out = _run_frac(flow_dir, weights, method)
    return DataArray(out, name=name, coords=flow_dir.coords, dims=flow_dir.dims, attrs=flow_dir.attrs)


@supports_dataset
def basins(flow_dir: DataArray, name: str = 'basins') -> DataArray:
    """For every cell the linear index `row * W + col` of the outlet its D8 flow path ends in (an outlet: a cell with code 0,
    or whose code names a neighbour outside the raster or a NaN neighbour); NaN at NaN cells.  Arguments and errors as for
    `flow_accumulation`.  Returns a float64 DataArray."""
    return _graph_product(flow_dir, name, 'basins', BASINS)


# ------------------------------------------------------------------ stream_order, stream_link, watershed, flow_length
def stream_network(src: DeviceArray, accum: DeviceArray, threshold: float, want: int, flags: int = 0, stream=None):
    """xrs_stream_network on a resident float32 plane of codes and a float32 / float64 accumulation: (Strahler or None, Shreve or
    None, links or None, status words).  Raises ValueError for an invalid code or a ring of stream cells."""
    rows, cols = src.shape
    outs = [DeviceArray((rows, cols), np.float64) if want & bit else None for bit in (STRAHLER, SHREVE, LINK)]
    status = (ctypes.c_int64 * STREAM_STATUS_WORDS)()
    if rows * cols:
        work = workspace("stream_network", rows, cols)
        _lib.call("xrs_stream_network", src.ptr, accum.ptr, DTYPE_CODE[accum.dtype], rows, cols, float(threshold), want, work.ptr,
                  *[o.ptr if o else None for o in outs], status, flags, stream)
        settle(stream)
    words = [int(w) for w in status]
    _raise_for(words)
    return (*outs, words)


def watershed_plane(src: DeviceArray, pour: DeviceArray, values, kind, flags: int = 0, stream=None):
    """xrs_flow_watershed on resident planes: (the float32 labels, status words).  `pour`: one of the ten dtypes of DTYPE_CODE;
    `values`, `kind`: `proximity.target_array`'s."""
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float32)
    status = (ctypes.c_int64 * STATUS_WORDS)()
    if rows * cols:
        vals = DeviceArray.from_numpy(values.view(np.float64), stream=stream) if values.size else None
        work = workspace("flow_watershed", rows, cols)
        _lib.call("xrs_flow_watershed", src.ptr, pour.ptr, DTYPE_CODE[pour.dtype], vals.ptr if vals else None, kind, int(values.size),
                  rows, cols, work.ptr, out.ptr, status, flags, stream)
        settle(stream)
    words = [int(w) for w in status]
    _raise_for(words)
    return out, words


def length_plane(src: DeviceArray, cx, cy, dg, flags: int = 0, stream=None):
    """xrs_flow_length on a resident float32 plane of codes: (the float64 lengths, status words)."""
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float64)
    status = (ctypes.c_int64 * STATUS_WORDS)()
    if rows * cols:
        work = workspace("flow_length", rows, cols)
        _lib.call("xrs_flow_length", src.ptr, rows, cols, cx, cy, dg, work.ptr, out.ptr, status, flags, stream)
        settle(stream)
    words = [int(w) for w in status]
    _raise_for(words)
    return out, words


def _check_pair(flow_dir, other, label, what):
    for agg in (flow_dir, other):
        refuse_split_backends(agg, what)
    _check_raster(flow_dir.data, what)
    _check_raster(other.data, what)
    if tuple(flow_dir.data.shape) != tuple(other.data.shape):
        raise ValueError(f"{what}: flow_dir and {label} differ in shape, {tuple(flow_dir.data.shape)} and {tuple(other.data.shape)}")


def _like(flow_dir, out, name):
    # the result has flow_dir's backend, whatever the second raster's is (as cost_distance's has `raster`'s)
    return DataArray(finish(out, not isinstance(flow_dir.data, DeviceArray)), name=name, coords=flow_dir.coords, dims=flow_dir.dims,
                     attrs=flow_dir.attrs)


def _stream_product(flow_dir, flow_accum, threshold, want, name, what):
    _check_pair(flow_dir, flow_accum, "flow_accum", what)
    threshold = float(np.float64(threshold))
    if np.isnan(threshold):
        raise ValueError(f"{what}: threshold is NaN")
    _lib.require_device()
    stream = get_stream()
    src = to_device_f32(flow_dir.data)
    acc, _ = resident(flow_accum.data, stream, FLOAT_SUFFIX, np.float64)
    *outs, _ = stream_network(src, acc, threshold, want, stream=stream)
    return _like(flow_dir, next(o for o in outs if o is not None), name)


def stream_order(flow_dir: DataArray, flow_accum: DataArray, threshold: float = 100, method: str = 'strahler',
                 name: str = 'stream_order') -> DataArray:
    """The order of every stream cell, NaN off the streams: Strahler's (1 at a source, one more where two streams of the same
    order meet) or Shreve's (the number of sources upstream).  The rule: module docstring.

    flow_dir: 2-D DataArray of D8 codes as `flow_direction` returns them; flow_accum: DataArray of the same shape, as
    `flow_accumulation` returns it (any numeric raster will do); a stream cell is one with flow_accum >= threshold.  method:
    'strahler' or 'shreve'.  NumPy- or DeviceArray-backed, each input staged on its own (the result's backend is flow_dir's).
    A value that is no code, or a ring of stream cells, raises ValueError.  Returns a float64 DataArray with flow_dir's coords,
    dims and attrs."""
    if method not in ('strahler', 'shreve'):
        raise ValueError(f"stream_order: method must be 'strahler' or 'shreve', got {method!r}")
    return _stream_product(flow_dir, flow_accum, threshold, STRAHLER if method == 'strahler' else SHREVE, name, 'stream_order')


def stream_link(flow_dir: DataArray, flow_accum: DataArray, threshold: float = 100, name: str = 'stream_link') -> DataArray:
    """The streams cut into links (reaches between sources, junctions and stream ends): every stream cell gets the id of its
    link, 1 .. L in row-major order of the links' upstream ends; a junction cell opens the link below it; NaN off the streams.
    Arguments and errors as for `stream_order`.  Returns a float64 DataArray."""
    return _stream_product(flow_dir, flow_accum, threshold, LINK, name, 'stream_link')


def watershed(flow_dir: DataArray, pour_points: DataArray, target_values: list = [], name: str = 'watershed') -> DataArray:
    """What drains to each pour point: every cell gets, as float32, the value `pour_points` holds at the first pour point on its
    D8 flow path (the cell itself included); NaN where the path meets none and at NaN cells.  The rule: module docstring.

    flow_dir: 2-D DataArray of D8 codes; pour_points: DataArray of the same shape whose pour points are the cells equal to one
    of `target_values`, or with none given every non-zero finite cell.  NumPy- or DeviceArray-backed, each input staged on its
    own (the result's backend is flow_dir's).  A value that is no code, or a cycle without a pour point, raises ValueError.
    Returns a float32 DataArray with flow_dir's coords, dims and attrs."""
    _check_pair(flow_dir, pour_points, "pour_points", 'watershed')
    _lib.require_device()
    stream = get_stream()
    data = widened(pour_points.data, stream, DTYPE_CODE, widen('watershed'))
    values, kind = target_array(target_values, data.dtype)              # (its TypeError comes before the upload)
    pour, _ = resident(data, stream)
    out, _ = watershed_plane(to_device_f32(flow_dir.data), pour, values, kind, stream=stream)
    return _like(flow_dir, out, name)


@supports_dataset
def flow_length(flow_dir: DataArray, name: str = 'flow_length') -> DataArray:
    """The downstream length of every cell's D8 flow path to its outlet, in the units of the cell size: 0 at outlets, NaN at NaN
    cells.  It is the length by step counts -- (E/W steps) * cx + (N/S steps) * cy + (diagonal steps) * sqrt(cx^2 + cy^2), each
    product and sum rounded once -- within a few ulp of the sum taken step by step and not equal to it (module docstring).

    flow_dir: 2-D DataArray of D8 codes (or a Dataset: every variable on its own), NumPy- or DeviceArray-backed (the result's
    backend); the cell size comes from `attrs['res']` or the coordinates, as for `flow_direction`.  A value that is no code, or a
    cycle, raises ValueError.  Returns a float64 DataArray with flow_dir's coords, dims and attrs."""
    refuse_split_backends(flow_dir, 'flow_length')
    rows, cols = _check_raster(flow_dir.data, 'flow_length')
    cx, cy, dg = cell_distances(flow_dir) if rows * cols else (1.0, 1.0, float(np.sqrt(2.0)))
    _lib.require_device()
    out, _ = length_plane(to_device_f32(flow_dir.data), cx, cy, dg, stream=get_stream())
    return _like(flow_dir, out, name)

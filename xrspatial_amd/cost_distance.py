"""cost_distance, cost_allocation, cost_backlink: the accumulated least cost from a set of sources over a friction surface, the
source each cell is reached from, and the neighbour it is reached through.  The reference (0.5.3) has none of the three, so the
result is a written rule (csrc/cost_distance.hip; stated in NumPy by tests/cost_distance_oracle.py), and it is
exact: the tests compare bit for bit.

`raster` says where the sources are, `friction` what a cell costs to cross; both 2-D and of one shape.  (cx, cy, dg) =
`hydrology.cell_distances(raster)`: float64, dg = sqrt(cx^2 + cy^2).
  1. passable: a cell whose friction is finite and > 0.  NaN, +-inf, 0 and negative friction cannot be entered;
  2. source: a passable cell of `raster` that is a target by `proximity`'s rule 1 (`target_values` empty: non-zero and finite;
     otherwise equal to one of them under NumPy's ==, compared as `proximity.target_array` says).  A target on an impassable
     cell is no source; without a source every output is NaN;
  3. step: from u to a neighbour v, both passable, over the length L = cx (E, W), cy (N, S) or dg (the diagonals),
     w(u, v) = L * ((float64(f(u)) + float64(f(v))) * 0.5): one IEEE add, then two multiplies, in this order, never fused.
     `connectivity=4` has no diagonal steps; a diagonal step needs only its two end cells passable;
  4. distance field: D is the least plane with D(s) = 0 at sources and D(v) = min over the passable neighbours u of
     fl(D(u) + w(u, v)) elsewhere.  It is unique and does not depend on the order of the updates (fl(d + w) is monotone in d
     and >= d; §6o has the proof), so the tile relaxation on the GPU equals a heap Dijkstra bit for bit;
  5. cost_distance = D as float64; NaN where the cell is impassable, where D is +inf (unreached, or overflowed) or where
     D > float64(max_cost).  (D never falls along a path, so the kernel may drop candidates above max_cost as it goes.)
  6. cost_backlink = float32 ESRI codes as `flow_direction` writes them (E 1, SE 2, S 4, SW 8, W 16, NW 32, N 64, NE 128): at a
     reached cell c that is no source, the first neighbour n in that order with D(n) < D(c) and fl(D(n) + w(n, c)) == D(c);
     0 at sources; NaN wherever rule 5 gives NaN.  The strict < makes the graph acyclic.  A reached cell without such a
     neighbour exists only where a step was absorbed by rounding (friction spread beyond ~2^52: the row
     [1, 1e20, 1e-20, 1e-20, 1e-20] with the source in column 0 has D = [0, 5e19, 1e20, 1e20, 1e20], and columns 3 and 4 have
     none).  Such cells are counted; `cost_backlink` and `cost_allocation` then raise ValueError naming the count,
     `cost_distance` does not;
  7. cost_allocation = float32(raster[source]) of the source the cell's back-link chain ends in (float32 for every dtype, as
     `allocation`); NaN wherever rule 5 gives NaN;
  8. `raster`: the ten XRS_DT_* dtypes are read in place, bool and float16 widened on the host as `proximity` does.  `friction`:
     float32 and float64 are read in place, every other numeric dtype is cast to float64 on the host, as `fill` does.  NumPy- or
     DeviceArray-backed, each input staged on its own; the result has `raster`'s backend.  dask- and ShardedArray-backed inputs
     raise NotImplementedError.  There is no CPU fallback;
  9. more than 2^32 - 2 cells, shapes that differ, an input that is not 2-D, a connectivity other than 4 or 8 and a NaN or
     negative max_cost raise ValueError.  Empty rasters give empty results.

Least-cost paths between named points, direction-dependent friction and friction in `a_star_search` are not built.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, hydrology
from ._launch import finish, get_stream, refuse_split_backends, resident, settle, widened, workspace
from ._xr import DataArray
from .device import DTYPE_CODE, FLOAT_SUFFIX, DeviceArray
from .proximity import target_array, widen

TIMED = 1                               # XRS_COST_TIMED
STATUS_WORDS = 256                      # XRS_COST_STATUS_WORDS: laid out as xrs_fill's (hydrology.relax_rounds reads the rounds)
SOURCES, ABSORBED, REACHED = 4, 5, 6    # status words
DISTANCE, ALLOCATION, BACKLINK = 0, 1, 2
_NAMES = ("cost_distance", "cost_allocation", "cost_backlink")


def cost_planes(src: DeviceArray, friction: DeviceArray, values, kind, cx, cy, dg, max_cost=np.inf, connectivity=8, backlink=True,
                flags: int = 0, stream=None):
    """xrs_cost_distance on resident planes: (the float64 distances, the float32 back-links or None, the status words).
    `src`: one of the ten dtypes of DTYPE_CODE; `friction`: float32 or float64; `values`, `kind`: `proximity.target_array`'s."""
    rows, cols = src.shape
    dist = DeviceArray((rows, cols), np.float64)
    link = DeviceArray((rows, cols), np.float32) if backlink else None
    status = (ctypes.c_int64 * STATUS_WORDS)()
    if rows * cols:
        vals = DeviceArray.from_numpy(values.view(np.float64), stream=stream) if values.size else None
        work = workspace("cost_distance", rows, cols)
        _lib.call("xrs_cost_distance", src.ptr, DTYPE_CODE[src.dtype], vals.ptr if vals else None, kind, int(values.size), friction.ptr,
                  DTYPE_CODE[friction.dtype], rows, cols, cx, cy, dg, float(max_cost), int(connectivity), dist.ptr,
                  link.ptr if link else None, work.ptr, status, flags, stream)      # (waits for the stream: the status words)
    return dist, link, [int(w) for w in status]


def allocation_plane(src: DeviceArray, link: DeviceArray, stream=None):
    """The float32 plane of rule 7 from the back-link plane: `basins` of the links, then one gather of the sources' values."""
    rows, cols = src.shape
    out = DeviceArray((rows, cols), np.float32)
    if rows * cols:
        _, basin, _ = hydrology.flow_graph(link, hydrology.BASINS, stream=stream)
        _lib.call("xrs_cost_allocation", basin.ptr, src.ptr, DTYPE_CODE[src.dtype], rows, cols, out.ptr, stream)
        settle(stream)                                                   # `basin` goes back to the pool
    return out


def _check(raster, friction, max_cost, connectivity, what):
    for agg, label in ((raster, "raster"), (friction, "friction")):
        refuse_split_backends(agg, what)
        if len(agg.data.shape) != 2:
            raise ValueError(f"{what}: expected a 2D {label}, got shape {tuple(agg.data.shape)}")
        if np.dtype(agg.data.dtype).kind not in "iufb":
            raise TypeError(f"{what}: unsupported {label} dtype {agg.data.dtype}")
    if tuple(raster.data.shape) != tuple(friction.data.shape):
        raise ValueError(f"{what}: raster and friction differ in shape, {tuple(raster.data.shape)} and {tuple(friction.data.shape)}")
    rows, cols = (int(s) for s in raster.data.shape)
    if rows * cols > hydrology.MAX_CELLS:
        raise ValueError(f"{what}: more than 2**32 - 2 cells ({rows} x {cols})")
    if connectivity not in (4, 8):
        raise ValueError(f"{what}: connectivity must be 4 or 8, got {connectivity!r}")
    max_cost = float(np.inf if max_cost is None else max_cost)
    if np.isnan(max_cost) or max_cost < 0:
        raise ValueError(f"{what}: max_cost must be a number >= 0, got {max_cost}")
    return rows, cols, max_cost


def _process(raster, friction, x, y, target_values, max_cost, connectivity, name, product):
    what = _NAMES[product]
    rows, cols, max_cost = _check(raster, friction, max_cost, connectivity, what)
    if tuple(raster.dims) != (y, x):
        raise ValueError("raster.coords should be named as coordinates:({0}, {1})".format(y, x))
    cx, cy, dg = hydrology.cell_distances(raster) if rows * cols else (1.0, 1.0, float(np.sqrt(2.0)))
    _lib.require_device()
    stream = get_stream()
    data = widened(raster.data, stream, DTYPE_CODE, widen(what))
    values, kind = target_array(target_values, data.dtype)              # (its TypeError comes before the upload)
    src, _ = resident(data, stream)
    like_numpy = not isinstance(raster.data, DeviceArray)               # what the caller gave, whatever the widening did
    fr, _ = resident(friction.data, stream, FLOAT_SUFFIX, np.float64)
    dist, link, words = cost_planes(src, fr, values, kind, cx, cy, dg, max_cost, connectivity, backlink=product != DISTANCE, stream=stream)
    if product != DISTANCE and words[ABSORBED]:
        raise ValueError(f"{what}: {words[ABSORBED]} reached cells have no neighbour their cost comes from: a step was absorbed by "
                         "rounding (the friction values span more than float64 resolves); cost_distance still answers")
    out = dist if product == DISTANCE else (link if product == BACKLINK else allocation_plane(src, link, stream))
    return DataArray(finish(out, like_numpy), name=name, coords=raster.coords, dims=raster.dims, attrs=raster.attrs)


def cost_distance(raster: DataArray, friction: DataArray, x: str = 'x', y: str = 'y', target_values: list = [], max_cost: float = np.inf,
                  connectivity: int = 8, name: str = 'cost_distance') -> DataArray:
    """The least accumulated cost of a path from any source to every cell over a friction surface (the rule: module docstring).

    raster: 2-D DataArray with dims (y, x) that marks the sources: the cells equal to one of `target_values`, or with none given
    every non-zero finite cell.  friction: DataArray of the same shape, the cost of crossing a cell per unit of length; a cell
    whose friction is not finite and > 0 cannot be entered.  A step between neighbours costs its length (from `attrs['res']` or
    the coordinates, as for `slope`) times the mean of the two frictions.  max_cost: cells that cost more are NaN.
    connectivity: 8 (with diagonal steps) or 4.  NumPy- or DeviceArray-backed (the result's backend is raster's).  Returns a
    float64 DataArray with raster's coords, dims and attrs: 0 at sources, NaN at cells that are impassable, unreached or beyond
    max_cost."""
    return _process(raster, friction, x, y, target_values, max_cost, connectivity, name, DISTANCE)


def cost_allocation(raster: DataArray, friction: DataArray, x: str = 'x', y: str = 'y', target_values: list = [],
                    max_cost: float = np.inf, connectivity: int = 8, name: str = 'cost_allocation') -> DataArray:
    """The value of the source every cell is reached from at least cost, as float32 (of equal costs the one the back-links lead
    to); NaN where `cost_distance` is NaN.  Arguments as for `cost_distance`.  Raises ValueError where rounding absorbed a step
    (module docstring, rule 6)."""
    return _process(raster, friction, x, y, target_values, max_cost, connectivity, name, ALLOCATION)


def cost_backlink(raster: DataArray, friction: DataArray, x: str = 'x', y: str = 'y', target_values: list = [], max_cost: float = np.inf,
                  connectivity: int = 8, name: str = 'cost_backlink') -> DataArray:
    """For every cell the neighbour its least-cost path comes from, as `flow_direction`'s codes (E 1, SE 2, S 4, SW 8, W 16, NW 32,
    N 64, NE 128), float32: 0 at sources, NaN where `cost_distance` is NaN.  Following the codes leads to the cell's source, so
    `basins`, `flow_accumulation` and every other reader of a D8 raster work on it.  Arguments as for `cost_distance`.  Raises
    ValueError where rounding absorbed a step (module docstring, rule 6)."""
    return _process(raster, friction, x, y, target_values, max_cost, connectivity, name, BACKLINK)

"""polygonize: vector polygons for the connected regions of equal-valued pixels of a raster.  Reference:
xrspatial/experimental/polygonize.py.

The reference labels the regions in one serial scan and then walks every boundary serially.  Its result has a closed form
(DESIGN.md §6h), which csrc/polygonize.hip computes in parallel: regions are the connected components of a fixed set of
links, every ring is a cycle of a successor function over boundary states, and the start, the order and the vertices of
every ring follow from minima, ranks and a sort.  For `return_type="numpy"` the result is the reference's, value for value:
polygon order, ring order (exterior, then holes), start vertex, vertex sequence and closing point.

`return_type="flat"` is an addition: `(column, points, ring_offsets, polygon_offsets)` as four NumPy arrays -- points is
float64 `[total, 2]`; ring k owns `points[ring_offsets[k]:ring_offsets[k + 1]]`; polygon p owns rings
`polygon_offsets[p]:polygon_offsets[p + 1]`, the exterior first; `column[p]` is its pixel value in the raster's dtype.  The
lists of `"numpy"` are views of that one points array.

NumPy- and DeviceArray-backed rasters of the ten XRS_DT_* dtypes are accepted; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from .. import _lib
from .._launch import get_stream, resident, settle, workspace
from .._xr import DataArray
from ..device import DTYPE_CODE, DeviceArray

MAX_CELLS = (1 << 32) - 1            # 32-bit cell indices in csrc/polygonize.hip
MAX_STATES = (1 << 31) - 1           # XRS_POLYGONIZE_MAX_STATES: boundary states (cell, direction); a state id and a flag share 32 bits
MAX_REGIONS = (1 << 32) - 1          # the reference's uint32 region ids
_RETURN_TYPES = ("numpy", "flat", "awkward", "geopandas", "spatialpandas")


def assemble(column, points, ring_offsets, polygon_offsets):
    """The reference's (column, polygons) lists from the flat arrays; every ring is a view of `points`."""
    ro = [int(v) for v in ring_offsets]
    rings = [points[ro[k]:ro[k + 1]] for k in range(len(ro) - 1)]
    po = [int(v) for v in polygon_offsets]
    return list(column), [rings[po[p]:po[p + 1]] for p in range(len(po) - 1)]


def _mask_code(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.bool_:
        return DTYPE_CODE[np.dtype(np.uint8)]
    if dtype not in DTYPE_CODE:
        raise TypeError(f"polygonize: unsupported mask dtype {dtype}")
    return DTYPE_CODE[dtype]


def _free_bytes():
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.call("xrs_mem_info", ctypes.byref(free), ctypes.byref(total))
    return int(free.value)


def flat(values, mask, connectivity_8, transform, stats=None):
    """(column, points, ring_offsets, polygon_offsets) as NumPy arrays.  `values`, `mask`: NumPy arrays or DeviceArrays."""
    dtype = np.dtype(values.dtype)
    if dtype not in DTYPE_CODE:
        raise TypeError(f"polygonize: unsupported raster dtype {dtype}")
    rows, cols = (int(s) for s in values.shape)
    if rows * cols > MAX_CELLS:
        raise ValueError(f"polygonize: {rows} x {cols} cells exceed the 2**32 - 1 cells this backend indexes; "
                         "split your raster into smaller chunks.")
    mask_code = _mask_code(mask.dtype) if mask is not None else 0
    _lib.require_device()
    stream = get_stream()
    dev, _ = resident(values, stream)
    mdev = resident(mask, stream)[0] if mask is not None else None
    work = workspace("polygonize", rows, cols)
    n_regions, n_states = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.call("xrs_polygonize_census", dev.ptr, DTYPE_CODE[dtype], mdev.ptr if mdev is not None else None, mask_code, rows, cols,
              8 if connectivity_8 else 4, work.ptr, ctypes.byref(n_regions), ctypes.byref(n_states), stream)
    n_regions, n_states = int(n_regions.value), int(n_states.value)
    if stats is not None:
        stats.update(regions=n_regions, states=n_states, leader_rounds=0, rank_rounds=0, rings=0, points=0)
    if n_regions > MAX_REGIONS:
        raise RuntimeError("polygonize generates too many polygons, split your raster into smaller chunks.")
    if n_states == 0:                                    # every pixel masked out
        return (np.empty(0, dtype), np.empty((0, 2), np.float64), np.zeros(1, np.int64), np.zeros(1, np.int64))
    if n_states > MAX_STATES:
        raise ValueError(f"polygonize: {n_states} boundary states exceed the {MAX_STATES} this backend ranks; "
                         "split your raster into smaller chunks.")
    ring_bytes = _lib.workspace_bytes("polygonize_rings", n_states)
    # the ring workspace, then the points (at most one per state and one more per ring) and the offsets
    need = ring_bytes + (n_states + n_states // 4 + 1) * 16 + (n_states // 4 + 2) * 16 + n_regions * dtype.itemsize
    free = _free_bytes()
    if need > free:
        raise MemoryError(f"polygonize: {n_states} boundary states need {need} bytes of device memory, {free} are free; "
                          "split your raster into smaller chunks.")
    rings = DeviceArray((ring_bytes,), np.uint8)
    n_rings, n_points = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rounds = (ctypes.c_int * 2)()
    _lib.call("xrs_polygonize_rings", rows, cols, work.ptr, rings.ptr, n_states, n_regions, ctypes.byref(n_rings),
              ctypes.byref(n_points), rounds, stream)
    n_rings, n_points = int(n_rings.value), int(n_points.value)
    if stats is not None:
        stats.update(leader_rounds=int(rounds[0]), rank_rounds=int(rounds[1]), rings=n_rings, points=n_points)
    points = DeviceArray((n_points, 2), np.float64)
    ring_offsets = DeviceArray((n_rings + 1,), np.int64)
    polygon_offsets = DeviceArray((n_regions + 1,), np.int64)
    column = DeviceArray((n_regions,), dtype)
    tf = None
    if transform is not None:
        tf = (ctypes.c_double * 6)(*[float(v) for v in transform])
    _lib.call("xrs_polygonize_scatter", dev.ptr, DTYPE_CODE[dtype], rows, cols, work.ptr, rings.ptr, n_states, n_regions, n_rings,
              tf, points.ptr, ring_offsets.ptr, polygon_offsets.ptr, column.ptr, stream)
    out = (column.get(stream), points.get(stream), ring_offsets.get(stream), polygon_offsets.get(stream))
    settle(stream)                                       # the workspaces go back to the pool
    return out


def _to_awkward(column, polygon_points):
    import awkward as ak
    return column, ak.Array(polygon_points)


def _to_geopandas(column, polygon_points, column_name):
    import geopandas as gpd
    from shapely.geometry import Polygon
    polygons = list(map(lambda points: Polygon(points[0], points[1:]), polygon_points))
    return gpd.GeoDataFrame({column_name: column, "geometry": polygons})


def _to_spatialpandas(column, polygon_points, column_name):
    from spatialpandas import GeoDataFrame
    from spatialpandas.geometry import PolygonArray
    for i, arrays in enumerate(polygon_points):          # spatialpandas expects 1d numpy arrays
        polygon_points[i] = list(map(lambda array: np.reshape(array, -1), arrays))
    return GeoDataFrame({column_name: column, "geometry": PolygonArray(polygon_points)})


def polygonize(
    raster: DataArray,                       # shape (ny, nx) integer or float
    mask: Optional[DataArray] = None,        # shape (ny, nx) bool/integer/float
    connectivity: int = 4,                   # 4 or 8
    transform: Optional[np.ndarray] = None,  # shape (6,)
    column_name: str = "DN",
    return_type: str = "numpy",
):
    """
    Polygonize creates vector polygons for connected regions of pixels in a
    raster that share the same pixel value.  It is a raster to vector
    converter.  Same signature and, for return_type "numpy", the same result
    as `xrspatial.experimental.polygonize`.

    Parameters
    ----------
    raster: DataArray
        Input raster, NumPy- or DeviceArray-backed.

    mask: DataArray, optional
        Optional input mask.  Pixels to include should have mask values of 1
        or True, pixels to exclude should have 0 or False.  This is the
        opposite of a NumPy mask.

    connectivity: int, default=4
        Whether to use 4-connectivity (adjacent along long edge only) or
        8-connectivity (adjacent along long edge or diagonal) to determine
        which pixels are connected.

    transform: ndarray, optional
        Optional affine transform to apply to return polygon coordinates.

    column_name: str, default="DN"
        Name to use for column returned.  Only used if return_type is
        "geopandas" or "spatialpandas".

    return_type: str, default="numpy"
        Format of returned data.  Allowed values are "numpy", "flat",
        "spatialpandas", "geopandas" and "awkward".  "numpy" and "flat" are
        always available, the others require optional dependencies.

    Returns
    -------
    Polygons and their corresponding values in a format determined by
    return_type.  "numpy": (column, polygons), a list of pixel values and a
    list, one entry per polygon, of lists of (n, 2) float64 arrays, the
    exterior ring first, then the holes.  "flat": (column, points,
    ring_offsets, polygon_offsets) as four arrays (module docstring).
    """
    if raster.ndim != 2 or raster.shape[0] < 1 or raster.shape[1] < 1:
        raise ValueError(
            "Raster array must be 2D with a shape of at least (1, 1)")

    # Check mask.
    if mask is not None:
        if not (type(raster.data) is type(mask.data)):  # noqa: E721
            raise TypeError(
                "raster and mask have different underlying types: "
                f"{type(raster.data)} and {type(mask.data)}")
        if raster.shape != mask.shape:
            raise ValueError(
                f"raster and mask must have the same shape: {raster.shape} "
                f"{mask.shape}")

    mask_data = mask.data if mask is not None else None

    # Check connectivity.
    if connectivity not in (4, 8):
        raise ValueError(
            f"connectivity must be either 4 or 8, not {connectivity}")
    connectivity_8 = (connectivity == 8)

    # Check transform.
    if transform is not None:
        transform = np.asarray(transform)
        if len(transform) != 6:
            raise ValueError(
                f"Incorrect transform length of {len(transform)} instead of 6")

    if not isinstance(raster.data, (np.ndarray, DeviceArray)):
        raise TypeError(f"Unsupported array type: {type(raster.data)}")
    if return_type not in _RETURN_TYPES:
        raise ValueError(f"Invalid return_type '{return_type}'")

    result = flat(raster.data, mask_data, connectivity_8, transform)
    if return_type == "flat":
        return result
    column, polygon_points = assemble(*result)
    if return_type == "numpy":
        return column, polygon_points
    elif return_type == "awkward":
        return _to_awkward(column, polygon_points)
    elif return_type == "geopandas":
        return _to_geopandas(column, polygon_points, column_name)
    else:
        return _to_spatialpandas(column, polygon_points, column_name)

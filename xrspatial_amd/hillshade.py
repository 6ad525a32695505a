"""xrspatial.hillshade drop-in.  Reference: xrspatial/hillshade.py:103-208.

`shadows=True` is the reference's ray-traced path (gpu_rtx/hillshade.py, gpu_rtx/mesh_utils.py: OptiX on NVIDIA RT cores)
as a rule, evaluated by csrc/hillshade_shadow.hip with one ray walk per cell.  Everything is float64 unless
marked; only + - * /, sqrt and comparisons, every sum left to right:
  1 sun     (sin(az) cos(alt), -cos(az) cos(alt), sin(alt)), az / alt in radians (`_get_sun_dir`); x is the column, y the row.
            Any angle, at or below the horizon too.
  2 mesh    vertex (w, h, zv[h, w]), zv = (float32)((double)value * scale), scale = max(H, W) / max of the raster; every cell
            with h < H - 1, w < W - 1 carries T0 = [(h+1, w), (h+1, w+1), (h, w)] and T1 = [(h+1, w+1), (h, w+1), (h, w)].
  3 hit     interior cells only: x0 = (double)(float)(j + 1e-3), y0 likewise from i (the float32 camera origin), fx = x0 - j,
            fy = y0 - i; the point is in T0 when fy >= fx, else T1; with C, D = zv[i, j], zv[i, j+1] and A, B = zv[i+1, j],
            zv[i+1, j+1] the plane's gradient is (gx, gy) = (B - A, A - C) in T0, (D - C, B - D) in T1; zh = C + fx gx + fy gy;
            n = (-gx, -gy, 1) / sqrt(gx^2 + gy^2 + 1), the reference's flipped normal.  Computed, not traced.
  4 shadow  origin (x0, y0, zh) + n * 1e-3, direction sun; in shadow when any triangle of the mesh is hit with t > 1e-3, by
            Moller-Trumbore: e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1 . p, s = o - v0, u = (s . p) / det, q = s x e1,
            v = (d . q) / det, t = (e2 . q) / det; hit iff det != 0, u >= 0, v >= 0, u + v <= 1, t > 1e-3.  A face turned away
            from the sun shadows itself through its own triangle, as in the reference.
  5 shade   (sun . n + 1) / 2, halved in shadow, clamped to [0, 1], float32; NaN on rows 0, H - 1 and columns 0, W - 1.
  6 inputs  2-D, NumPy- or DeviceArray-backed (the result's backend, float32); float32 / float64 read in place, other dtypes
            through float64.  A non-finite cell or a maximum <= 0 raises ValueError (the reference's scale is NaN or negative
            there); H < 3 or W < 3 gives all NaN; dask, ShardedArray and fuse() scopes raise NotImplementedError.
Departures from the reference: the camera hit is computed (its camera at height 10000 is inside the terrain from
max(H, W) = 10000 on), non-finite rasters are refused, and the trace is float64.  There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _lib, fused
from ._launch import finish, get_stream, refuse_split_backends, resident, settle, stencil, widened, workspace
from ._xr import DataArray
from .dataset_support import supports_dataset
from .device import FLOAT_SUFFIX, DeviceArray
from .sharded import ShardedArray
from .utils import dask_overlap, is_dask

# The reference's NumPy runner returns float64 under NumPy >= 2 (its final combine is
# promoted by a np.float64 scalar) and float32 under NumPy 1.x; its CuPy
# runner returns float32.  Mirror both: numpy in -> what NumPy would give, device in -> f32.
_NUMPY_RESULT_DTYPE = np.float64 if int(np.__version__.split('.')[0]) >= 2 else np.float32


def _run_numpy(data, azimuth, angle_altitude):
    return _hill(data, _NUMPY_RESULT_DTYPE, azimuth, angle_altitude)


def _run_hip(data, azimuth, angle_altitude):
    return _hill(data, np.float32, azimuth, angle_altitude)


def _hill(data, out_dtype, azimuth, angle_altitude):
    # replaces _run_numpy (hillshade.py:20-35); the entry point has an `out_f64` flag after `out`
    return stencil("xrs_hillshade_f32", data, out_dtype, (float(azimuth), float(angle_altitude)),
                   pre=(int(np.dtype(out_dtype) == np.float64),))


# ------------------------------------------------------------------ shadows=True (module docstring)
def sun_vector(azimuth, angle_altitude):
    """rule 1: the unit vector towards the sun (gpu_rtx/hillshade.py:133-143 `_get_sun_dir`, without the rotations)"""
    az, alt = math.radians(float(azimuth)), math.radians(float(angle_altitude))
    return math.sin(az) * math.cos(alt), -math.cos(az) * math.cos(alt), math.sin(alt)


def _height_scale(count, cells, zmin, zmax, rows, cols, what="hillshade(shadows=True)"):
    """rule 6's refusals and rule 2's scale from { count, min, max } of the finite cells"""
    if int(count) != cells:
        raise ValueError(f"{what}: the raster holds {cells - int(count)} non-finite cells")
    if not zmax > 0:
        raise ValueError(f"{what}: the raster's maximum must be positive, got {zmax}")
    scale = float(max(rows, cols)) / zmax                    # mesh_utils.py:17-19
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f"{what}: the raster's maximum {zmax} gives no usable height scale")
    return scale


def mesh_source(data, stream, what="hillshade(shadows=True)"):
    """(resident float32 / float64 raster, scale, min, max) for the mesh of rule 2, with rule 6's refusals; shared with
    viewshed(method='mesh').  A host raster is checked where it lies, before any device work; a resident one by one reduction."""
    rows, cols = data.shape
    if isinstance(data, np.ndarray):
        data = widened(data, stream, FLOAT_SUFFIX, np.float64)         # integers, bool, float16: float64, as viewshed reads them
        count = int(np.isfinite(data).sum())
        zmin, zmax = (float(data.min()), float(data.max())) if count == data.size else (math.nan, math.nan)
        scale = _height_scale(count, data.size, zmin, zmax, rows, cols, what)
        _lib.require_device()
        return resident(data, stream)[0], scale, zmin, zmax
    _lib.require_device()
    src, _ = resident(data, stream, FLOAT_SUFFIX, np.float64)
    suffix = FLOAT_SUFFIX[src.dtype]
    stats = DeviceArray((4,), np.float64)                    # { count, min, max, sum } of the finite cells, one pass
    work = workspace("classify", 1, int(suffix == "f64"))
    _lib.call("xrs_classify_finite_stats_" + suffix, src.ptr, rows * cols, work.ptr, stats.ptr, stream)
    count, zmin, zmax, _ = (float(v) for v in stats.get(stream))
    return src, _height_scale(count, rows * cols, zmin, zmax, rows, cols, what), zmin, zmax


def _run_shadows(data, azimuth, angle_altitude, shadows=1):
    """A NumPy raster gets NumPy back, a DeviceArray a DeviceArray; float32 either way."""
    sun = sun_vector(azimuth, angle_altitude)
    if not all(math.isfinite(v) for v in sun):
        raise ValueError("hillshade: azimuth and angle_altitude must be finite")
    like_numpy = isinstance(data, np.ndarray)
    rows, cols = data.shape
    stream = get_stream()
    src, scale, zmin, zmax = mesh_source(data, stream)
    out = DeviceArray((rows, cols), np.float32)
    work = workspace("hillshade_shadow", rows, cols)
    _lib.call("xrs_hillshade_shadow_" + FLOAT_SUFFIX[src.dtype], src.ptr, rows, cols, scale, zmin, zmax, sun[0], sun[1], sun[2],
              int(shadows), work.ptr, out.ptr, stream)
    settle(stream, like_numpy)
    return finish(out, like_numpy)


def _hillshade_shadows(agg, azimuth, angle_altitude, name):
    if len(agg.shape) != 2:
        raise ValueError(f"hillshade(shadows=True): a 2-D raster is needed, got {len(agg.shape)} dimensions")
    if 0 in agg.shape:
        raise ValueError(f"hillshade(shadows=True): an empty raster, shape {tuple(agg.shape)}")
    if fused.current() is not None:
        raise NotImplementedError("hillshade(shadows=True) cannot join a fuse() scope: a shadow ray reads cells far from its "
                                  "own, and the fused pass hands every product one row strip at a time")
    refuse_split_backends(
        agg, None, named=agg.data,
        sharded="hillshade(shadows=True) does not support row-sharded (multi-GPU) DataArray: rays cross shards",
        dask="hillshade(shadows=True) does not support dask backed DataArray: rays cross chunks")
    out = _run_shadows(agg.data, azimuth, angle_altitude)
    return DataArray(out, name=name, coords=agg.coords, dims=agg.dims, attrs=agg.attrs)


@supports_dataset
def hillshade(agg: DataArray,
              azimuth: int = 225,
              angle_altitude: int = 25,
              name: Optional[str] = 'hillshade',
              shadows: bool = False) -> DataArray:
    """Illumination of every cell for a light at `azimuth` / `angle_altitude` (degrees), in [0, 1].

    Same signature and results as `xrspatial.hillshade`; runs on the MI355X.
    `shadows=True` shades the reference's triangle mesh instead and halves the value of every cell whose ray towards the
    sun hits the mesh (what upstream traces through OptiX; the rule is in this module's docstring): float32, NumPy- or
    DeviceArray-backed rasters without non-finite cells and with a positive maximum.
    """
    if shadows:
        return _hillshade_shadows(agg, azimuth, angle_altitude, name)
    scope = fused.current()
    if scope is not None:
        return scope.defer('hillshade', agg, name, {'light': (float(azimuth), float(angle_altitude))},
                           numpy_dtype=_NUMPY_RESULT_DTYPE)
    if isinstance(agg.data, np.ndarray):
        out = _run_numpy(agg.data, azimuth, angle_altitude)
    elif isinstance(agg.data, (DeviceArray, ShardedArray)):
        out = _run_hip(agg.data, azimuth, angle_altitude)
    elif is_dask(agg.data):                 # hillshade.py:38-46: map_overlap(depth=(1, 1), boundary=nan) around the numpy runner
        out = dask_overlap(_run_numpy, (1, 1))(agg.data, azimuth, angle_altitude)
    else:
        raise TypeError('Unsupported Array Type: {}'.format(type(agg.data)))
    return DataArray(out, name=name, coords=agg.coords, dims=agg.dims, attrs=agg.attrs)

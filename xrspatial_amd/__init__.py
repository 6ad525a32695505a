"""xrspatial_amd -- MI355X (gfx950) backend for xarray-spatial's dense 2-D raster hot path.

Drop-in for the `xrspatial.*` functions on that path (same names, signatures, DataArray
in/out): slope, aspect, hillshade, curvature, focal.mean / apply / focal_stats,
convolution.convolve_2d / convolution_2d, multispectral ndvi / evi / savi (+ nbr, nbr2, ndmi),
zonal.stats, zonal.regions, classify (binary, reclassify, equal_interval, quantile, percentiles, box_plot, std_mean,
head_tail_breaks, maximum_breaks), natural_breaks, perlin, generate_terrain, bump, viewshed (the sweep and the ray-traced mesh variant), proximity / allocation / direction, a_star_search, cost_distance / cost_allocation / cost_backlink (least accumulated cost over a friction surface), fill / flow_direction / flow_accumulation / basins (D8 hydrology with depression fill and flat resolution; method='dinf' gives Tarboton's D-infinity angles and the accumulation of their float shares, weights= a float-weighted accumulation for either method), stream_order / stream_link / watershed / flow_length (Strahler and Shreve orders, stream links, watersheds from pour points, downstream flow length), local (cell_stats, combine, the frequencies, positions, rank, popularity),
experimental.polygonize, rasterize (polygons back into a raster; no counterpart upstream), and contours (the isolines of a raster at given levels by marching squares, open and closed lines per level; no counterpart upstream), and idw (inverse-distance interpolation of scattered points from an exact k-nearest-neighbour search per cell, idw.neighbors for the search alone; no counterpart upstream), and resample (a raster onto another axis-aligned grid: nearest, bilinear, cubic, lanczos, average, sum, min, max, mode; no counterpart upstream).  Python host code calling hand-written HIP kernels through the C ABI of
libxrs_hip.so (include/xrs_hip.h); no PyTorch, CuPy, Numba or Triton involved.

    import xrspatial_amd as xrspatial        # numpy-backed DataArray in -> numpy-backed out
    from xrspatial_amd import DeviceArray    # keep rasters resident in HBM between calls
    with xrspatial.fuse(): ...               # several products of one raster from a single pass (fused.py)
    from xrspatial_amd import ShardedArray   # this rank's rows of a raster spread over several GPUs (sharded.py)
"""
from ._lib import XrsError, LIB_PATH  # noqa: F401
from ._xr import DataArray, Dataset  # noqa: F401
from .device import DeviceArray, empty_cache, synchronize  # noqa: F401
from .utils import has_hip  # noqa: F401

from .aspect import aspect  # noqa: F401
from .bump import bump  # noqa: F401
from .contours import contours  # noqa: F401
from .classify import (binary, box_plot, equal_interval, head_tail_breaks, maximum_breaks, percentiles,  # noqa: F401
                       quantile, reclassify, std_mean)
from .cost_distance import cost_allocation, cost_backlink, cost_distance  # noqa: F401
from .curvature import curvature  # noqa: F401
from .focal import mean  # noqa: F401
from .fused import fuse  # noqa: F401
from .sharded import ShardedArray  # noqa: F401
from .hillshade import hillshade  # noqa: F401
from .hydrology import basins, fill, flow_accumulation, flow_direction  # noqa: F401
from .hydrology import flow_length, stream_link, stream_order, watershed  # noqa: F401
from .idw import idw  # noqa: F401  (the function; idw.neighbors and idw.plan_bins hang on it)
from .jenks import natural_breaks  # noqa: F401
from .multispectral import arvi, evi, nbr, ndvi, savi, sipi  # noqa: F401
from .pathfinding import a_star_search  # noqa: F401
from .perlin import perlin  # noqa: F401
from .experimental.polygonize import polygonize  # noqa: F401
from .proximity import (allocation, direction, euclidean_distance, great_circle_distance, manhattan_distance,  # noqa: F401
                        proximity)
from .rasterize import rasterize, transform_from_coords  # noqa: F401
from .resample import resample  # noqa: F401  (the function; resample.tables and the table builders hang on it)
from .slope import slope  # noqa: F401
from .terrain import generate_terrain  # noqa: F401
from .viewshed import viewshed, viewshed_mesh  # noqa: F401
from .zonal import crosstab as zonal_crosstab  # noqa: F401
from .zonal import regions  # noqa: F401
from .zonal import stats as zonal_stats  # noqa: F401

from . import analytics, classify, convolution, experimental, focal, local, multispectral, pathfinding, zonal  # noqa: F401

__version__ = "0.1.0"

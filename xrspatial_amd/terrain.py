"""generate_terrain: 16 octaves of lattice noise shaped into a pseudo-random DEM.  Reference: xrspatial/terrain.py, its
NumPy path (`_gen_terrain`, `_terrain_numpy`).

All 16 octaves, the divide and the cube run in ONE launch of csrc/noise.hip that writes every cell once (the reference's
GPU path is 16 read-modify-write launches and seven more full-plane passes); the normalisation, the water line and
`* zfactor` are a second, in-place launch.  A DeviceArray-backed `agg` gets its terrain in HBM with no host-to-device copy
of the plane: the only uploads are the 16 permutation tables of seeds `seed .. seed + 15`, cached on the device (perlin.py).
"""
from __future__ import annotations

import numpy as np

from ._launch import refuse_split_backends
from ._xr import DataArray
from .perlin import MODE_TERRAIN, check_dtype, check_lattice, run
from .utils import get_dataarray_resolution

N_OCTAVES = 16
WATER_LINE = 0.3                          # `data[data < 0.3] = 0`, compared in the data's dtype


def _scale(value, old_range, new_range):
    d = (value - old_range[0]) / (old_range[1] - old_range[0])
    return d * (new_range[1] - new_range[0]) + new_range[0]


def _run_terrain(data, seed, x_range_scaled, y_range_scaled, zfactor):
    return run(data, [seed + i for i in range(N_OCTAVES)], x_range_scaled, y_range_scaled, MODE_TERRAIN, threshold=WATER_LINE,
               scale=zfactor)


def cell_centres(lo, hi, n):
    """lo + (j + 0.5) * (hi - lo) / n for j < n."""
    return lo + (np.arange(n, dtype=np.float64) + 0.5) * (hi - lo) / n


def generate_terrain(agg, x_range=(0, 500), y_range=(0, 500), seed=10, zfactor=4000, full_extent=None, name='terrain'):
    """A pseudo-random terrain over `agg`'s shape: 16 octaves of perlin noise (seeds seed .. seed + 15), cubed,
    normalised to [0, 1], cells below 0.3 set to 0 (water) and the rest multiplied by `zfactor`.

    agg: 2-D float32 / float64 DataArray; its backend (NumPy or DeviceArray) and dtype are the result's.  x_range, y_range:
    the extent of the result's coordinates.  full_extent: (xmin, ymin, xmax, ymax) of the whole terrain that x_range /
    y_range are a window of (default: the window itself).  Same signature and values as `xrspatial.generate_terrain`
    (NumPy path).

    The result has dims ('y', 'x'), cell-centre coordinates `range[0] + (j + 0.5) * (range[1] - range[0]) / n` and
    attrs {'res': (xres, yres)}.  The reference takes both from a datashader Canvas; that these coordinates equal
    datashader's has not been verified (datashader is not a dependency of this package)."""
    check_dtype(agg.data, "generate_terrain")
    height, width = agg.shape
    if height == 0 or width == 0:
        raise ValueError("generate_terrain: the raster has no cells")

    if full_extent is None:
        full_extent = (x_range[0], y_range[0], x_range[1], y_range[1])
    elif not isinstance(full_extent, (list, tuple)) or len(full_extent) != 4:
        raise TypeError('full_extent must be tuple(4)')

    full_xrange = (full_extent[0], full_extent[2])
    full_yrange = (full_extent[1], full_extent[3])
    if full_xrange[0] == full_xrange[1] or full_yrange[0] == full_yrange[1]:
        raise ValueError("generate_terrain: the full extent is empty")

    x_range_scaled = (_scale(x_range[0], full_xrange, (0.0, 1.0)), _scale(x_range[1], full_xrange, (0.0, 1.0)))
    y_range_scaled = (_scale(y_range[0], full_yrange, (0.0, 1.0)), _scale(y_range[1], full_yrange, (0.0, 1.0)))
    check_lattice("generate_terrain", x_range_scaled, y_range_scaled, agg.shape, N_OCTAVES)

    refuse_split_backends(agg, 'generate_terrain')
    out = _run_terrain(agg.data, int(seed), x_range_scaled, y_range_scaled, zfactor)

    coords = {'y': cell_centres(y_range[0], y_range[1], height), 'x': cell_centres(x_range[0], x_range[1], width)}
    result = DataArray(out, name=name, coords=coords, dims=('y', 'x'))
    if height > 1 and width > 1:
        res = get_dataarray_resolution(result)
    else:           # one cell along an axis leaves no coordinate spacing to measure: the cells' own extent
        res = ((x_range[1] - x_range[0]) / width, (y_range[1] - y_range[0]) / height)
    result.attrs = {'res': res}
    return result

"""local: statistics, frequencies, positions, rank, popularity and combine across the variables of a Dataset, cell by cell.
Reference: xrspatial/local.py.

The reference builds a Python tuple per cell with `np.nditer` and calls a NumPy function on it.  This backend computes the
same values with one thread per cell (csrc/local.hip): N planes read once, each in its own dtype, one 8-byte
plane written.  Signatures, argument errors and the return value (a bare DataArray: default dims, no coords, no attrs;
`combine` carries attrs['key']) are the reference's.  The rule:

  working type  int64 when every participating variable (`ref_var` included) is an integer and the function is max, min, sum,
                a frequency, a position, rank, popularity or combine: exact, `sum` wraps as NumPy's does.  Otherwise float64
                after exact widening; mean, median and std always.  An int64 variable next to a floating one is exact only for
                |v| <= 2^53 -- as it is for the reference's np.max / np.sum / ...; the reference's per-item comparisons in the
                frequencies, positions and rank are Python's and stay exact beyond 2^53, these are not.
  result dtype  float64 if any participating variable is floating or the function is mean, median, std, rank, popularity or
                combine (the last three can give NaN whatever the inputs), else int64.  The reference's dtype depends on the
                DATA (`np.array(out)` is int64 when no cell happened to be NaN); it is the values that are matched.
  cell_stats    any NaN among the cell's values gives NaN for all six functions.  sum is NumPy's pairwise block: n < 8 left to
                right; n >= 8 eight accumulators a[k] = v[k], a[k] += v[i + k] for every full group of eight,
                ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)), then the remainder left to right.  mean = sum / n;
                std = sqrt(pairwise((x - mean) * (x - mean)) / n); correctly rounded division and sqrt, no contraction.
                median is the middle value, or (a + b) / 2 of the two middle ones.
  frequencies   any NaN among the data variables gives NaN; else the count of items with ref > item (lesser), ref == item
                (equal), ref < item (greater); a NaN ref counts 0.  With a float32 `ref_var` every item is rounded to float32
                first (NumPy 2: a float32 scalar against a Python number compares in float32).
  positions     any NaN gives NaN; else the 1-based index of the first variable equal to the minimum / maximum (-0.0 == 0.0).
  rank          any NaN among the data variables gives NaN.  k = ref - 1 (in ref_var's dtype, wrapping), n data variables:
                k >= n NaN; 0 <= k < n the k-th smallest; -n <= k < 0 the (k + n)-th smallest (Python's wrap); k < -n NaN
                (the reference raises IndexError there).
  popularity    u = the number of distinct values of the cell.  NaN if any value is NaN or u >= n; the value if u == 1; else
                with k = ref - 1: k >= u NaN, 0 <= k < u the k-th smallest distinct value, -u <= k < 0 wraps, k < -u NaN (the
                reference raises).  That is what the reference does, not what its name says.
  combine       a cell with any NaN gives NaN; else the 1-based id of the cell's tuple, ids in order of first occurrence in
                row-major order, tuples equal under `==` (-0.0 is 0.0).  attrs['key'] = {id: tuple} holds the first-seen cell's
                values as Python ints / floats.  At most 2^31 - 1 cells.

Checks this backend adds, all raised before any device work: every selected variable is 2-D and of one shape (the reference's
`nditer` broadcasts and flattens; that is not reproduced) -- ValueError; at most XRS_LOCAL_MAX_PLANES = 64 data variables --
ValueError; dtypes are the ones the kernels read in place: bool, float16 and uint64 raise TypeError (their NumPy-2 scalar
comparison rules differ); `ref_var` of rank and popularity has an integer dtype -- TypeError (with a floating one the reference
dies in `list[float]`).  Variables may be NumPy- or DeviceArray-backed: all NumPy gives a NumPy result, any DeviceArray a
DeviceArray.  There is no CPU fallback; dask- and ShardedArray-backed variables raise NotImplementedError.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._launch import finish, get_stream, refuse_split_backends, resident, settle, workspace
from ._xr import DataArray, Dataset
from .device import DTYPE_CODE, DeviceArray

XRS_LOCAL_MAX_PLANES = 64

# XRS_LOCAL_* of include/xrs_hip.h
MAX, MIN, SUM, MEAN, STD, MEDIAN, LESSER, EQUAL, GREATER, LOWEST, HIGHEST, RANK, POPULARITY = range(13)
funcs = {'max': MAX, 'mean': MEAN, 'median': MEDIAN, 'min': MIN, 'std': STD, 'sum': SUM}      # (the reference's order)
_FLOAT_RESULT = (MEAN, STD, MEDIAN, RANK, POPULARITY)


# ------------------------------------------------------------------ argument checks: the reference's, word for word
def _check_raster(raster):
    if not isinstance(raster, Dataset):
        raise TypeError(
            "Expected raster to be a 'xarray.Dataset'. "
            f"Received '{type(raster).__name__}' instead."
        )


def _check_ref_var(raster, ref_var):
    if not isinstance(ref_var, str):
        raise TypeError(
            "Expected ref_var to be a 'str'. "
            f"Received '{type(ref_var).__name__}' instead."
        )
    if ref_var not in list(raster.data_vars):
        raise ValueError('raster must contain ref_var.')


def _check_data_vars(raster, data_vars, ref_var=None):
    if data_vars:
        if (
            not isinstance(data_vars, list) or
            not all([isinstance(var, str) for var in data_vars])
        ):
            raise TypeError('Expected data_vars to be a list of string.')
        if not set(data_vars).issubset(raster.data_vars):
            raise ValueError(
                "raster must contain all the variables of data_vars. "
                f"The variables available are '{list(raster.data_vars)}'."
            )
        if ref_var is not None and ref_var in data_vars:
            raise ValueError('ref_var must not be an element of data_vars.')
        return list(data_vars)
    data_vars = list(raster.data_vars)
    if ref_var is not None:
        data_vars.remove(ref_var)
    return data_vars


# ------------------------------------------------------------------ this backend's checks (before any device work)
def _arrays(raster, what, data_vars, ref_var=None, integer_ref=False):
    """The arrays of `data_vars` (and of `ref_var`) after the checks of the module docstring."""
    names = data_vars + ([ref_var] if ref_var is not None else [])
    for name in names:
        refuse_split_backends(raster[name], what)
    if not data_vars:
        raise ValueError(f"{what}: no data variables")
    if len(data_vars) > XRS_LOCAL_MAX_PLANES:
        raise ValueError(f"{what}: {len(data_vars)} data variables, at most {XRS_LOCAL_MAX_PLANES} are supported")
    arrays = [raster[name].data for name in names]
    shape = tuple(arrays[0].shape)
    for name, a in zip(names, arrays):
        if len(a.shape) != 2:
            raise ValueError(f"{what}: variable '{name}' is {len(a.shape)}-D, 2-D variables are needed")
        if tuple(a.shape) != shape:
            raise ValueError(f"{what}: variable '{name}' has shape {tuple(a.shape)}, '{names[0]}' has {shape}")
        dtype = np.dtype(a.dtype)
        if dtype not in DTYPE_CODE or dtype == np.uint64:
            raise TypeError(f"{what}: variable '{name}' has unsupported dtype {dtype}")
    ref = arrays.pop() if ref_var is not None else None
    if integer_ref and np.dtype(ref.dtype).kind not in "iu":
        raise TypeError(f"{what}: ref_var '{ref_var}' has dtype {ref.dtype}, an integer dtype is needed")
    return arrays, ref


# ------------------------------------------------------------------ the launches
def _on_device(arrays, stream):
    return [resident(a, stream)[0] for a in arrays]


def _plane_table(dev):
    n = len(dev)
    return (ctypes.c_void_p * n)(*[d.ptr for d in dev]), (ctypes.c_int * n)(*[DTYPE_CODE[d.dtype] for d in dev])


def result_dtype(op, dtypes):
    """float64 or int64, by the rule of the module docstring; `dtypes`: of every participating variable."""
    if op in _FLOAT_RESULT or any(np.dtype(d).kind == "f" for d in dtypes):
        return np.dtype(np.float64)
    return np.dtype(np.int64)


def _run_cells(op, arrays, ref=None):
    _lib.require_device()
    everything = arrays + ([ref] if ref is not None else [])
    like_numpy = all(isinstance(a, np.ndarray) for a in everything)
    stream = get_stream()
    dev = _on_device(everything, stream)
    ref_dev = dev.pop() if ref is not None else None
    out_dtype = result_dtype(op, [a.dtype for a in everything])
    out = DeviceArray(dev[0].shape, out_dtype)
    if out.size:
        ptrs, codes = _plane_table(dev)
        _lib.call("xrs_local_cells", op, ptrs, codes, len(dev), ref_dev.ptr if ref_dev is not None else None,
                  DTYPE_CODE[ref_dev.dtype] if ref_dev is not None else 0, out.size, out.ptr, int(out_dtype == np.int64), stream)
        if any(d is not a for d, a in zip(dev + [ref_dev], everything)):
            settle(stream)                                               # uploaded copies go back to the pool when this returns
    return finish(out, like_numpy)


def _run_combine(arrays):
    """(ids, key)"""
    _lib.require_device()
    like_numpy = all(isinstance(a, np.ndarray) for a in arrays)
    stream = get_stream()
    dev = _on_device(arrays, stream)
    out = DeviceArray(dev[0].shape, np.float64)
    n = out.size
    if n >= 2 ** 31:
        raise ValueError(f"combine: {n} cells, at most 2^31 - 1 are supported")
    key = {}
    if n:
        ptrs, codes = _plane_table(dev)
        work = workspace("local_combine", n, len(dev))
        nbytes = work.nbytes
        classes = ctypes.c_int64(0)
        _lib.call("xrs_local_combine", ptrs, codes, len(dev), n, work.ptr, nbytes, out.ptr, None, 0, ctypes.byref(classes), stream)
        count = int(classes.value)
        if count:
            first = DeviceArray((count,), np.uint32)
            _lib.call("xrs_local_combine", ptrs, codes, len(dev), n, work.ptr, nbytes, out.ptr, first.ptr, count, ctypes.byref(classes),
                      stream)
            values = DeviceArray((count, len(dev)), np.uint64)
            _lib.call("xrs_local_gather", ptrs, codes, len(dev), n, first.ptr, count, values.ptr, stream)
            table = values.get(stream)
            columns = [table[:, j].view(np.float64 if d.dtype.kind == "f" else np.int64).tolist() for j, d in enumerate(dev)]
            key = {i + 1: comb for i, comb in enumerate(zip(*columns))}
        settle(stream)
    return finish(out, like_numpy), key


def _wrap(data, attrs=None):
    return DataArray(data, attrs=attrs) if attrs else DataArray(data)


# ------------------------------------------------------------------ the nine functions
def cell_stats(raster, data_vars=None, func='sum'):
    """max, mean, median, min, std or sum (`func`) of the variables `data_vars` (default: all) of the Dataset `raster`, cell by
    cell; NaN where any of them is NaN.  Same signature as `xrspatial.local.cell_stats`; the rule is the module docstring's."""
    _check_raster(raster)
    if func not in funcs:
        raise ValueError(
            f'{func} is not supported. '
            f"The supported types are '{list(funcs.keys())}'."
        )
    data_vars = _check_data_vars(raster, data_vars)
    arrays, _ = _arrays(raster, "cell_stats", data_vars)
    return _wrap(_run_cells(funcs[func], arrays))


def combine(raster, data_vars=None):
    """A unique 1-based id for every unique combination of the variables' values, in order of first occurrence; NaN where any
    variable is NaN; attrs['key'] = {id: values}.  Same signature as `xrspatial.local.combine`."""
    _check_raster(raster)
    data_vars = _check_data_vars(raster, data_vars)
    arrays, _ = _arrays(raster, "combine", data_vars)
    ids, key = _run_combine(arrays)
    return DataArray(ids, attrs=dict(key=key))


def _with_ref(op, what, raster, ref_var, data_vars, integer_ref=False):
    _check_raster(raster)
    _check_ref_var(raster, ref_var)
    data_vars = _check_data_vars(raster, data_vars, ref_var)
    arrays, ref = _arrays(raster, what, data_vars, ref_var, integer_ref)
    return _wrap(_run_cells(op, arrays, ref))


def lesser_frequency(raster, ref_var, data_vars=None):
    """How many of `data_vars` (default: all but `ref_var`) are less than `ref_var`, cell by cell (ref > item).  Same signature
    as `xrspatial.local.lesser_frequency`."""
    return _with_ref(LESSER, "lesser_frequency", raster, ref_var, data_vars)


def equal_frequency(raster, ref_var, data_vars=None):
    """How many of `data_vars` equal `ref_var`, cell by cell.  Same signature as `xrspatial.local.equal_frequency`."""
    return _with_ref(EQUAL, "equal_frequency", raster, ref_var, data_vars)


def greater_frequency(raster, ref_var, data_vars=None):
    """How many of `data_vars` are greater than `ref_var`, cell by cell (ref < item).  Same signature as
    `xrspatial.local.greater_frequency`."""
    return _with_ref(GREATER, "greater_frequency", raster, ref_var, data_vars)


def _position(op, what, raster, data_vars):
    _check_raster(raster)
    data_vars = _check_data_vars(raster, data_vars)
    arrays, _ = _arrays(raster, what, data_vars)
    return _wrap(_run_cells(op, arrays))


def lowest_position(raster, data_vars=None):
    """The 1-based index of the first variable that holds the cell's minimum.  Same signature as
    `xrspatial.local.lowest_position`."""
    return _position(LOWEST, "lowest_position", raster, data_vars)


def highest_position(raster, data_vars=None):
    """The 1-based index of the first variable that holds the cell's maximum.  Same signature as
    `xrspatial.local.highest_position`."""
    return _position(HIGHEST, "highest_position", raster, data_vars)


def popularity(raster, ref_var, data_vars=None):
    """The `ref_var`-th smallest distinct value of the cell where values repeat (the module docstring has the exact rule, which
    is the reference's).  Same signature as `xrspatial.local.popularity`; where the reference raises IndexError (`ref_var` below
    the wrap range) the result is NaN."""
    return _with_ref(POPULARITY, "popularity", raster, ref_var, data_vars, integer_ref=True)


def rank(raster, ref_var, data_vars=None):
    """The `ref_var`-th smallest value of the cell.  Same signature as `xrspatial.local.rank`; where the reference raises
    IndexError (`ref_var` below the wrap range) the result is NaN."""
    return _with_ref(RANK, "rank", raster, ref_var, data_vars, integer_ref=True)

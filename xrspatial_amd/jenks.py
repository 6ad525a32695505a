"""natural_breaks: the reference's Jenks classification (xrspatial/classify.py:508-654, 736-835, its CPU path).

What is host work in the reference stays the reference's NumPy lines: the seeded index shuffle, the finite filter, the unique
count, the sort, the float32 cast and the backtrack over the class limits.  The device does the rest: it gathers the sample out
of the resident raster in the raster's own dtype (xrs_gather_elems), finds the finite max (classify._Stats), runs the dynamic
programme -- one launch per class column, one thread per row, the reference's arithmetic operation by operation
(csrc/jenks.hip) -- and bins every cell (classify's bin pass).

dask- and ShardedArray-backed rasters raise NotImplementedError, like the other statistic-driven classifiers.
"""
from __future__ import annotations

import warnings

import numpy as np

from . import _lib
from . import classify as _classify
from ._launch import get_stream, workspace
from ._xr import DataArray
from .dataset_support import supports_dataset
from .device import DeviceArray

_SEED = 1234567890
_MAX_SAMPLE = (1 << 24) - 1               # xrs_jenks_matrices_f32: the class limits are float32 row numbers
_MAX_CELLS = 1 << 32                      # the reference's index array is uint32
_index_cache = []                         # [((num_data, num_sample), indices)], the two most recent last


def sample_indices(num_data, num_sample):
    """The first `num_sample` entries of the reference's shuffle of 0 .. num_data-1 (classify.py:602-607).  O(num_data) on
    the host by the reference's definition; the seed is fixed, so the last two results are kept (read-only)."""
    key = (int(num_data), int(num_sample))
    for i, (k, idx) in enumerate(_index_cache):
        if k == key:
            _index_cache.append(_index_cache.pop(i))
            return idx
    generator = np.random.RandomState(_SEED)
    idx = np.linspace(0, key[0], key[0], endpoint=False, dtype=np.uint32)
    generator.shuffle(idx)
    sample_idx = idx[:key[1]].copy()
    sample_idx.setflags(write=False)
    _index_cache.append((key, sample_idx))
    del _index_cache[:-2]
    return sample_idx


def kclass_from_limits(lower_class_limits, sorted_sample, k):
    """The backtrack of _run_jenks (classify.py:574-586) over the limits table: the k + 1 class boundaries, float32."""
    data, n_classes = sorted_sample, k
    k = data.shape[0]
    kclass = np.zeros(n_classes + 1, dtype=np.float32)
    kclass[0] = data[0]
    kclass[-1] = data[-1]
    count_num = n_classes
    while count_num > 1:
        elt = int(lower_class_limits[k][count_num] - 2)
        kclass[count_num - 1] = data[elt]
        k = int(lower_class_limits[k][count_num] - 1)
        count_num -= 1
    return kclass


def jenks_matrices(sorted_sample, k):
    """(lower_class_limits, var_combinations) of _run_numpy_jenks_matrices for a sorted float32 sample, from the device."""
    data = np.ascontiguousarray(sorted_sample, dtype=np.float32)
    n = data.shape[0]
    if not 1 <= n <= _MAX_SAMPLE:
        raise _lib.XrsError(f"natural_breaks: the model is fitted on 1 .. 2^24-1 sample values ({n})")
    stream = get_stream()
    data_d = DeviceArray.from_numpy(data, stream=stream)
    limits_d = DeviceArray((n + 1, k + 1), np.float32)
    var_d = DeviceArray((n + 1, k + 1), np.float32)
    work = workspace("jenks", n, k)
    _lib.call("xrs_jenks_matrices_f32", data_d.ptr, n, k, limits_d.ptr, var_d.ptr, work.ptr, work.nbytes, stream)
    return limits_d.get(stream), var_d.get(stream)


def _sample(dev, host, num_sample):
    """The reference's `sample_data`, in the raster's dtype: the shuffled sample gathered on the device, or every cell (the
    caller's own array where the raster came from the host, one download where it is resident)."""
    num_data = dev.size
    if num_sample is not None and num_sample < num_data:
        if num_data > _MAX_CELLS:
            raise _lib.XrsError(f"natural_breaks: sampling takes at most 2^32 cells per raster ({num_data})")
        idx = sample_indices(num_data, num_sample)       # (a negative num_sample slices like the reference's idx[:num_sample])
        stream = get_stream()
        idx_d = DeviceArray.from_numpy(idx, stream=stream)
        out = DeviceArray((idx.size,), dev.dtype)
        _lib.call("xrs_gather_elems", dev.ptr, dev.dtype.itemsize, num_data, idx_d.ptr, idx.size, out.ptr, stream)
        return out.get(stream)
    return host.reshape(-1) if host is not None else dev.get(get_stream()).reshape(-1)


def natural_break_bins(sample_data, k, max_data):
    """_compute_natural_break_bins (classify.py:612-644) from the sample on: (bins, uvk)."""
    if sample_data.size >= 40000:
        with warnings.catch_warnings():
            warnings.simplefilter('default')
            warnings.warn('natural_breaks Warning: Natural break '
                          'classification (Jenks) has a complexity of O(n^2), '
                          'your classification with {} data points may take '
                          'a long time.'.format(sample_data.size),
                          Warning)
    sample_data = np.asarray(sample_data)
    sample_data = sample_data[np.isfinite(sample_data)]
    uv = np.unique(sample_data)
    uvk = len(uv)
    if uvk < k:
        with warnings.catch_warnings():
            warnings.simplefilter('default')
            warnings.warn('natural_breaks Warning: Not enough unique values '
                          'in data array for {} classes. '
                          'n_samples={} should be >= n_clusters={}. '
                          'Using k={} instead.'.format(k, uvk, k, uvk),
                          Warning)
        uv.sort()
        return uv, uvk
    sample_data.sort()
    sorted_f32 = sample_data.astype(np.float32)          # `np.float32(data[i4])` of the loop, `kclass[...] = data[elt]` after it
    limits = jenks_matrices(sorted_f32, k)[0] if k > 1 else None     # (the backtrack reads the table from 2 classes on)
    bins = np.array(kclass_from_limits(limits, sorted_f32, k)[1:])
    bins[-1] = max_data
    return bins, uvk


def _run_natural_break(data, num_sample, k):
    dev, like_numpy = _classify._resident(data)
    st = _classify._Stats(dev)
    count, _, max_data, _ = st.moments()
    if count == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    sample = _sample(dev, np.asarray(data) if like_numpy else None, num_sample)
    bins, uvk = natural_break_bins(sample, k, float(max_data))
    return _classify._classified(st, like_numpy, bins, np.arange(uvk))


@supports_dataset
def natural_breaks(agg, num_sample=20000, name='natural_breaks', k=5):
    """Natural breaks (Jenks): k classes that minimise the within-class variance, fitted on a seeded sample of `num_sample`
    cells (None: every cell).  Same signature, sample, warnings and results as `xrspatial.classify.natural_breaks`."""
    run = _classify._statistic_mapper(_run_natural_break)(agg)
    return DataArray(run(agg.data, num_sample, k), name=name, dims=agg.dims, coords=agg.coords, attrs=agg.attrs)

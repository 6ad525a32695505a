"""NumPy restatement of the classify bin pass, for the tests only (never imported by the package).

`bin_values` is _cpu_bin (xrspatial/classify.py:153-187) cell for cell: searchsorted-left for non-decreasing NaN-free
bins, the reference's bisection verbatim -- run once per distinct value -- for any other bins."""
import numpy as np


def _literal(v, bins):
    nb = len(bins)
    if not np.isfinite(v):
        return -1
    if v <= bins[0]:
        return 0
    if not v <= bins[nb - 1]:
        return -1
    start, end = 0, nb - 1
    mid = (end + start) // 2
    while start <= end:
        if bins[mid] < v:
            start = mid + 1
        elif v > bins[mid - 1]:
            break
        else:
            end = mid - 1
        mid = (end + start) // 2
    return mid


def bin_index(data, bins):
    """The bin of every cell (-1: none), comparisons in float64."""
    bins = np.asarray(bins, dtype=np.float64)
    x = np.asarray(data).astype(np.float64)
    if bins.size == 0:                  # only a raster without a finite cell gets no bins: nothing reads them
        return np.full(x.shape, -1, np.int64)
    if not np.isnan(bins).any() and np.all(bins[1:] >= bins[:-1]):
        idx = np.searchsorted(bins, x, side="left")
        return np.where(np.isfinite(x) & (x <= bins[-1]), idx, -1)
    u, inv = np.unique(x.ravel(), return_inverse=True)
    return np.array([_literal(v, bins) for v in u], dtype=np.int64)[inv.ravel()].reshape(x.shape)


def bin_values(data, bins, new_values):
    idx = bin_index(data, bins)
    nv = np.append(np.asarray(new_values).astype(np.float32), np.float32(np.nan))
    return np.where(idx > -1, nv[np.where(idx > -1, idx, len(nv) - 1)], np.float32(np.nan)).astype(np.float32)


def binary(data, values):
    data = np.asarray(data)
    x = data.astype(np.float64)
    hit = np.isin(x, np.asarray(values, dtype=np.float64))
    if data.dtype.kind != "f":
        return hit.astype(data.dtype)
    return np.where(hit, 1, np.where(np.isfinite(x), 0, np.nan)).astype(data.dtype)

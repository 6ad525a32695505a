"""Rasters of 64-bit ids shared by tests/test_zonal_ids_host.py (CPU stand-in of the C ABI) and
tests/test_gpu_zonal_ids.py (the MI355X), and the exact comparison of a zonal frame with the oracle's columns."""
import numpy as np

P53, P60, P62 = 1 << 53, 1 << 60, 1 << 62
I64 = np.iinfo(np.int64)

# int64 ids a double does not tell apart (or only just does): name -> ascending ids
INT64_ID_SETS = {
    "above_2p53": [P53 + 1, P53 + 2, P53 + 5],
    "above_2p60": [P60 + 1, P60 + 3, P60 + 4],
    "below_m2p62": [-P62 - 1, -P62 + 1],
    "extremes": [I64.min, I64.min + 1, -1, 0, I64.max - 1, I64.max],
    "straddle_2p53": [P53 - 2, P53 - 1, P53, P53 + 1, P53 + 2],
    "straddle_m2p53": [-P53 - 2, -P53 - 1, -P53, -P53 + 1, -P53 + 2],
}


def id_raster(ids, dtype=np.int64, shape=(37, 61), seed=0):
    """A raster that holds every id of `ids`: runs of 1..9 equal cells (zone rasters come in runs), the last id the most
    frequent, every id present."""
    rng = np.random.default_rng(seed)
    ids = np.array(ids, dtype=dtype)
    n = shape[0] * shape[1]
    weights = np.ones(len(ids))
    weights[-1] = 2.0
    picks = rng.choice(len(ids), size=n, p=weights / weights.sum())
    flat = np.repeat(picks, rng.integers(1, 10, n))[:n]
    flat[:len(ids)] = np.arange(len(ids))
    return ids[flat].reshape(shape)


def small_values(shape, seed=0, dtype=np.float32, nan_frac=0.02):
    """Integral values 0..49 (every statistic of them is exact in float32), a few NaN."""
    rng = np.random.default_rng(1000 + seed)
    v = rng.integers(0, 50, shape).astype(dtype)
    if np.dtype(dtype).kind == "f" and nan_frac:
        v[rng.random(shape) < nan_frac] = np.nan
    return v


def small_zones(shape, n_zones=4, seed=0, dtype=np.int32):
    rng = np.random.default_rng(2000 + seed)
    return rng.integers(0, n_zones, shape).astype(dtype)


def assert_stats_frame(got, want, stats, zone_dtype=None, label=""):
    """`got` (the package's DataFrame) equals `want` (oracle.xrs_oracle.zonal_stats columns) cell for cell."""
    zone = got["zone"].to_numpy()
    np.testing.assert_array_equal(zone, np.asarray(want["zone"]), err_msg=f"{label} zone")
    assert len(zone) == len(want["zone"]), label
    if zone_dtype is not None:
        assert zone.dtype == np.dtype(zone_dtype), (label, zone.dtype)
    assert list(got.columns) == ["zone"] + list(stats), label
    for s in stats:
        np.testing.assert_array_equal(got[s].to_numpy(), want[s], err_msg=f"{label} {s}")


def assert_crosstab_frame(got, want, agg="count", zone_dtype=None, label=""):
    """`got` (DataFrame) equals `want` (oracle.xrs_oracle.crosstab_2d): counts exactly, percentages to rtol 1e-6."""
    cats = [k for k in want if k != "zone"]
    assert list(got.columns) == ["zone"] + cats, (label, list(got.columns), cats)
    zone = got["zone"].to_numpy()
    np.testing.assert_array_equal(zone, np.asarray(want["zone"]), err_msg=f"{label} zone")
    assert len(zone) == len(want["zone"]), label
    if zone_dtype is not None:
        assert zone.dtype == np.dtype(zone_dtype), (label, zone.dtype)
    for c in cats:
        if agg == "count":
            np.testing.assert_array_equal(got[c].to_numpy(), want[c], err_msg=f"{label} category {c}")
        else:
            np.testing.assert_allclose(got[c].to_numpy(), want[c], rtol=1e-6, equal_nan=True, err_msg=f"{label} category {c}")

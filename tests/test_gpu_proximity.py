"""proximity / allocation / direction on the MI355X, through the public functions, against the rule (tests/proximity_oracle.py)
and the reference's own outputs (tests/golden/proximity_exec.npz).

EUCLIDEAN and MANHATTAN use +, -, *, |.| and a correctly rounded float64 sqrt only, so `proximity` and `allocation` equal the
rule bit for bit at every cell, and the fixture at every cell that is not one of the reference's misses (the cells at which
the rule and the executed reference differ: tests/test_proximity_host.py).  `direction` goes through the device's float64
atan2, which may differ from libm's by a few float64 ulp; that moves a float32 rounding by one step at most: within 1 float32
ulp of the rule, and exactly 0 at targets.

GREAT_CIRCLE goes through sin and asin, by the same argument `proximity` is within 1 float32 ulp.  Two targets whose float32
distances are within 2 ulp of one another may then change places, so `allocation` and `direction` are compared where the
rule's best and second-best target are more than 2 ulp apart; at most 0.5 % of a case's cells may be left out by that.

Every comparison records the number of cells that are not bit-equal (tests/parity_log.py)."""
import numpy as np
import pytest

from tests import parity_log
from tests import proximity_oracle as po
from tests.golden import make_proximity_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)
GC_GAP_ULP, GC_LEFT_OUT = 2, 0.005
SPAN = 256                                       # columns per step of the row scan and per block of the search


@pytest.fixture(scope="module")
def xa():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xa, z, xs, ys, **kw):
    return xa.DataArray(z, dims=["y", "x"], coords={"y": ys, "x": xs}, **kw)


def _products(xa, agg, tv, md, metric):
    kw = dict(target_values=tv, max_distance=md, distance_metric=metric)
    return {"proximity": xa.proximity(agg, **kw), "allocation": xa.allocation(agg, **kw), "direction": xa.direction(agg, **kw)}


def _same_nan(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:10].tolist())
    return ~np.isnan(want)


def _check(got, want, z, tv, metric, what, fixture=None):
    """the rules of the module docstring; got: the three planes from the device, want: tests/proximity_oracle.run"""
    exact = metric != "GREAT_CIRCLE"
    targets = po.targets(z, tv)
    use = np.ones(z.shape, bool)
    if not exact:
        use = ~(np.isfinite(want["second"]) & (po.ulps(want["d32"], want["second"]) <= GC_GAP_ULP))
        print(f"{what}: {int((~use).sum())} of {use.size} cells have a second target within {GC_GAP_ULP} ulp")
        assert (~use).mean() <= GC_LEFT_OUT, what
    for p in gen.PRODUCTS:
        g, w = got[p], want[p]
        num = _same_nan(g, w, f"{what} {p}")
        cells = num if (exact or p == "proximity") else num & use
        off = po.ulps(g[cells], w[cells])
        differ = int(np.count_nonzero(off))
        note = f"{differ} of {int(cells.sum())} compared cells not bit-equal, largest difference {int(off.max()) if off.size else 0} ulp"
        if not exact:
            note += f"; {int((~use).sum())} of {use.size} cells left out of allocation / direction (second target within 2 ulp)"
        print(f"{what} {p}: {note}")
        parity_log.record(what, p, g[cells], w[cells], tol=0 if exact and p != "direction" else 2.0 ** -23, note=note)
        if p == "allocation" or (exact and p == "proximity"):
            assert differ == 0, (what, p, note)
        else:
            assert (off <= 1).all(), (what, p, note)
    assert (got["direction"][targets] == 0).all() and (got["proximity"][targets] == 0).all(), what
    if fixture is not None and exact:
        miss = np.zeros(z.shape, bool)
        for p in gen.PRODUCTS:
            miss |= want[p].view(np.uint32) != fixture[p].view(np.uint32)
        for p in ("proximity", "allocation"):
            assert np.array_equal(got[p].view(np.uint32)[~miss], fixture[p].view(np.uint32)[~miss]), (what, p)


# ------------------------------------------------------------------ the fixture's cases
@pytest.mark.parametrize("case", CASES)
def test_equals_the_rule_and_the_reference(xa, case):
    z, xs, ys, tv, md, metric = gen.call_args(FIXTURE, case)
    before = z.copy()
    agg = _agg(xa, z, xs, ys, attrs={"crs": "EPSG:4326"})
    out = _products(xa, agg, tv, md, metric)
    for p, res in out.items():
        assert isinstance(res.data, np.ndarray) and tuple(res.dims) == ("y", "x") and res.attrs == {"crs": "EPSG:4326"}, p
        assert np.array_equal(np.asarray(res["x"].data), xs) and np.array_equal(np.asarray(res["y"].data), ys), p
    assert agg.data is z and np.array_equal(z, before, equal_nan=True)   # the input is left alone
    want = po.run(z, xs, ys, tv, md, metric)
    _check({p: r.data for p, r in out.items()}, want, z, tv, metric, case, {p: FIXTURE[f"{case}/{p}"] for p in gen.PRODUCTS})


# ------------------------------------------------------------------ beside the fixture, against the rule only
def _scatter_case(shape, seed, density, dtype=np.float32):
    z = gen.scatter(shape, seed, density, dtype)
    return z, 10.0 + 0.75 * np.arange(shape[1]), 400.0 - 1.25 * np.arange(shape[0])


@pytest.mark.parametrize("metric", ["EUCLIDEAN", "MANHATTAN", "GREAT_CIRCLE"])
@pytest.mark.parametrize("width", [129, SPAN + 1, 2 * SPAN + 1])
def test_widths_past_a_wave_and_past_the_scan_span(xa, width, metric):
    z, xs, ys = _scatter_case((9, width), width, 0.01)
    z[3, :] = 0                                                          # an empty row between the others
    z[4, 0], z[4, -1], z[5, min(SPAN, width - 1) - 1] = 4, 6, 8          # the ends of a row, the last column of a span
    if metric == "GREAT_CIRCLE":
        xs, ys = gen.geo(9, width, -30.0, 12.0)
    out = _products(xa, _agg(xa, z, xs, ys), [], np.inf, metric)
    _check({p: r.data for p, r in out.items()}, po.run(z, xs, ys, [], np.inf, metric), z, [], metric, f"proximity_9x{width}_{metric}")


def test_great_circle_round_the_back_of_the_sphere(xa):
    """longitudes more than 180 degrees apart: the nearest target of a row may be the one at its far end"""
    z = gen.scatter((12, 90), 31, 0.01, np.int32)
    z[2, 0], z[7, -1], z[9, 1] = 5, 6, 7
    xs, ys = gen.geo(12, 90, -178.9, 70.0)
    xs = -178.9 + (xs - xs[0]) * (357.6 / (xs[-1] - xs[0]))              # -178.9 .. 178.7 in uneven steps of about 4 degrees
    ys = 70.0 + (ys - ys[0]) * 120.0                                     # 70 down to about 58
    want = po.run(z, xs, ys, [], np.inf, "GREAT_CIRCLE")
    far = np.abs(xs[want["col"]] - xs[None, :]) > 180.0
    assert far.sum() >= 10                                               # the case does reach round the back
    out = _products(xa, _agg(xa, z, xs, ys), [], np.inf, "GREAT_CIRCLE")
    _check({p: r.data for p, r in out.items()}, want, z, [], "GREAT_CIRCLE", "proximity_great_circle_wrap")


@pytest.mark.parametrize("metric", ["EUCLIDEAN", "MANHATTAN"])
def test_one_target_in_each_corner(xa, metric):
    z = np.zeros((41, 71), np.int16)
    z[0, 0], z[0, -1], z[-1, 0], z[-1, -1] = 1, 2, 3, 4
    xs, ys = np.arange(71.0), np.arange(41.0)[::-1].copy()               # the centre row and column are equidistant: ties
    out = _products(xa, _agg(xa, z, xs, ys), [], np.inf, metric)
    _check({p: r.data for p, r in out.items()}, po.run(z, xs, ys, [], np.inf, metric), z, [], metric, f"proximity_corners_{metric}")
    assert set(np.unique(out["allocation"].data)) == {1.0, 2.0, 3.0, 4.0}


def test_max_distance_below_one_cell(xa):
    z, xs, ys = _scatter_case((33, 70), 7, 0.05, np.float64)
    out = _products(xa, _agg(xa, z, xs, ys), [], 0.5, "EUCLIDEAN")
    want = po.run(z, xs, ys, [], 0.5, "EUCLIDEAN")
    _check({p: r.data for p, r in out.items()}, want, z, [], "EUCLIDEAN", "proximity_max_below_a_cell")
    targets = po.targets(z)
    assert targets.any() and np.array_equal(~np.isnan(out["proximity"].data), targets)


def test_int64_targets_that_differ_beyond_2_to_the_53(xa):
    big = 2 ** 53
    rng = np.random.default_rng(3)
    pick = rng.random((20, 70))
    z = np.where(pick < 0.03, big + 1, np.where(pick < 0.10, big, 0)).astype(np.int64)
    xs, ys = np.arange(70.0), np.arange(20.0)
    assert np.float64(big + 1) == np.float64(big)                        # through float64 the two would be one value
    for tv in ([big + 1], [big], [big + 1, big + 3]):
        out = _products(xa, _agg(xa, z, xs, ys), tv, np.inf, "EUCLIDEAN")
        want = po.run(z, xs, ys, tv, np.inf, "EUCLIDEAN")
        assert np.array_equal(po.targets(z, tv), z == tv[0])
        _check({p: r.data for p, r in out.items()}, want, z, tv, "EUCLIDEAN", f"proximity_int64_" + "_".join(str(v - big) for v in tv))
    u = z.astype(np.uint64) + np.uint64(2 ** 63)                         # and beyond int64, where the raster is nonzero
    tv = np.array([2 ** 63 + big + 1], np.uint64)
    got = xa.proximity(_agg(xa, u, xs, ys), target_values=tv).data
    assert np.array_equal(got.view(np.uint32), po.run(z, xs, ys, [big + 1])["proximity"].view(np.uint32))


@pytest.mark.parametrize("dtype", [np.float32, np.int64, np.uint8, np.bool_])
def test_device_array_in_device_array_out(xa, dtype):
    z, xs, ys = _scatter_case((37, 53), 5, 0.03, np.float64)
    z = z.astype(dtype)
    dev_in = xa.DeviceArray.from_numpy(z)
    want = po.run(z, xs, ys)
    got = {}
    for p, fn in (("proximity", xa.proximity), ("allocation", xa.allocation), ("direction", xa.direction)):
        res = fn(_agg(xa, dev_in, xs, ys, attrs={"k": 1}))
        assert isinstance(res.data, xa.DeviceArray) and res.data.dtype == np.float32 and res.attrs == {"k": 1}, p
        got[p] = res.data.get()
    assert dev_in.dtype == np.dtype(dtype) and np.array_equal(dev_in.get(), z)          # the input is left alone
    _check(got, want, z, [], "EUCLIDEAN", f"proximity_device_{np.dtype(dtype).name}")


def test_dataset_in_dataset_out(xa):
    z, xs, ys = _scatter_case((20, 30), 8, 0.05, np.int32)
    ds = xa.Dataset({"a": _agg(xa, z, xs, ys), "b": _agg(xa, z.astype(np.float64) * 0.5, xs, ys)}, attrs={"k": 2})
    for p, fn in (("proximity", xa.proximity), ("allocation", xa.allocation), ("direction", xa.direction)):
        res = fn(ds, target_values=[1, 2, 3], distance_metric="MANHATTAN")
        assert isinstance(res, xa.Dataset) and set(res.data_vars) == {"a", "b"} and res.attrs == {"k": 2}
        for var in ("a", "b"):
            raster = np.asarray(ds[var].data)
            want = po.run(raster, xs, ys, [1, 2, 3], np.inf, "MANHATTAN")[p]
            num = _same_nan(res[var].data, want, f"{p} {var}")
            assert (po.ulps(res[var].data[num], want[num]) <= (1 if p == "direction" else 0)).all(), (p, var)


def test_sharded_raster_is_refused(xa):
    sh = xa.DataArray(xa.ShardedArray(8, 8, np.float32), dims=["y", "x"])
    for fn in (xa.proximity, xa.allocation, xa.direction):
        with pytest.raises(NotImplementedError, match="sharded"):
            fn(sh)

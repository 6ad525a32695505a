"""CPU checks of proximity / allocation / direction: the rule (tests/proximity_oracle.py) against the reference's own outputs
(tests/golden/proximity_exec.npz), the docstring examples, the argument checks and refusals, which all run before any device
work, and the three scalar helpers.

The reference's sweep is a heuristic.  A miss is a cell at which any of the three products differs between
the rule and the executed reference; there the rule's proximity must be strictly below the reference's, and every other
difference fails.  At most 0.5 % of one case's cells and 0.05 % of all cells may be misses (measured when the rule was
written: 0.23 % in the worst case, 0.006 % overall; this fixture: 1 cell of 55 597, 0.016 % of its case)."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import proximity_oracle as po
from tests.golden import make_proximity_exec as gen

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)
GC_CASES = [n for n in CASES if str(FIXTURE[f"{n}/metric"]) == "GREAT_CIRCLE"]
GC_GAP_ULP, GC_LEFT_OUT = 2, 0.005


def _agg(z, xs=None, ys=None, dims=("y", "x"), **kw):
    import xrspatial_amd as xa
    coords = None if xs is None else {dims[0]: ys, dims[1]: xs}
    return xa.DataArray(z, dims=list(dims), coords=coords, **kw)


@pytest.fixture(scope="module")
def oracle_runs():
    return {name: po.run(*gen.call_args(FIXTURE, name)) for name in CASES}


# ------------------------------------------------------------------ the rule against the executed reference
@pytest.mark.parametrize("case", CASES)
def test_rule_equals_the_reference_outside_its_misses(oracle_runs, case):
    got = oracle_runs[case]
    differ = np.zeros(got["proximity"].shape, bool)
    for p in gen.PRODUCTS:
        want = FIXTURE[f"{case}/{p}"]
        assert got[p].dtype == want.dtype == np.float32 and got[p].shape == want.shape
        differ |= got[p].view(np.uint32) != want.view(np.uint32)
    with np.errstate(invalid="ignore"):
        below = got["proximity"] < FIXTURE[f"{case}/proximity"]
    print(f"{case}: the sweep misses {int(differ.sum())} of {differ.size} cells")
    assert not (differ & ~below).any(), np.argwhere(differ & ~below)[:10].tolist()
    assert differ.mean() <= gen.CASE_CAP


def test_misses_over_the_whole_fixture():
    bad, missed, cells = gen.complaints(FIXTURE)
    print(f"the sweep misses {missed} of {cells} cells")
    assert not bad and missed <= gen.TOTAL_CAP * cells


def test_docstring_examples_as_the_reference_prints_them(oracle_runs):
    prox = [[3.1622777, 2.236068, 1.4142135, 1., 1.4142135], [3., 2., 1., 0., 1.], [3.1622777, 2.236068, 1.4142135, 1., 1.4142135],
            [3.6055512, 2.828427, 2.236068, 2., 2.236068], [4.2426405, 3.6055512, 3.1622777, 3., 3.1622777]]
    alloc = [[1., 1., 2., 2., 2.], [1., 1., 1., 2., 2.], [1., 1., 3., 2., 2.], [1., 3., 3., 3., 2.], [3., 3., 3., 3., 3.]]
    direc = [[45., 26.56505, 360., 333.43494, 315.], [63.434948, 45., 360., 315., 296.56506], [90., 90., 0., 270., 270.],
             [360., 135., 180., 225., 243.43495], [0., 270., 180., 206.56505, 225.]]
    for name, want in (("proximity", prox), ("allocation", alloc), ("direction", direc)):
        want = np.array(want, np.float32)                                # float32's repr round-trips
        assert np.array_equal(FIXTURE[f"doc_{name}/{name}"], want), name
        assert np.array_equal(oracle_runs[f"doc_{name}"][name], want), name


def test_fixture_covers_what_the_spec_lists():
    assert FIXTURE["line_1x9/z"].shape == (1, 9) and FIXTURE["line_9x1/z"].shape == (9, 1)
    for p in gen.PRODUCTS:
        assert np.isnan(FIXTURE[f"no_targets/{p}"]).all()
    assert (FIXTURE["all_targets/proximity"] == 0).all() and (FIXTURE["all_targets/direction"] == 0).all()
    assert np.array_equal(FIXTURE["all_targets/allocation"], FIXTURE["all_targets/z"].astype(np.float32))
    assert (np.diff(FIXTURE["ascending_y_20x25/ys"]) > 0).all() and (np.diff(FIXTURE["descending_x_20x25/xs"]) < 0).all()
    steps = np.diff(FIXTURE["nonuniform_20x25/xs"])
    assert steps.min() > 0 and steps.max() > 2 * steps.min()
    assert np.isinf(FIXTURE["nonuniform_20x25/max_distance"]) and FIXTURE["nonuniform_20x25_max6/max_distance"] == 6.0
    assert np.isnan(FIXTURE["nonuniform_20x25_max6/proximity"]).any()
    seen = set()
    for n in CASES:
        z = FIXTURE[f"{n}/z"]
        if z.shape in ((37, 53), (64, 96)):
            seen.add((str(FIXTURE[f"{n}/metric"]), z.dtype.name, bool(z.dtype.kind == "f" and np.isnan(z).any()),
                      FIXTURE[f"{n}/target_values"].size > 0))
    assert {m for m, _, _, _ in seen} == {"EUCLIDEAN", "GREAT_CIRCLE", "MANHATTAN"}
    assert {d for _, d, _, _ in seen} == {"int32", "int64", "float32", "float64"}
    assert {nan for _, _, nan, _ in seen} == {True, False} and {tv for _, _, _, tv in seen} == {True, False}
    comb = FIXTURE["comb_70x300/z"]
    assert comb.shape == (70, 300) and not comb[:, 1:-1].any() and comb[::7, 0].all() and comb[::7, -1].all()
    assert not np.delete(comb, np.s_[::7], axis=0).any()


@pytest.mark.parametrize("case", GC_CASES)
def test_great_circle_cases_have_few_near_ties(oracle_runs, case):
    """the GPU test compares allocation and direction under GREAT_CIRCLE only where the best and the second-best target are
    more than 2 float32 ulp apart; the cases are built so that this leaves out at most 0.5 % of the cells"""
    run = oracle_runs[case]
    close = np.isfinite(run["second"]) & (po.ulps(run["d32"], run["second"]) <= GC_GAP_ULP)
    print(f"{case}: {int(close.sum())} of {close.size} cells have a second target within {GC_GAP_ULP} ulp")
    assert close.mean() <= GC_LEFT_OUT


def test_tie_order_of_the_rule():
    """rows r <= i before rows r > i; above: the first in row-major order; below: the last"""
    z = np.zeros((5, 5), np.int32)
    z[0, 2], z[2, 0], z[2, 4], z[4, 2] = 1, 2, 3, 4                      # four targets at distance 2 of the centre
    xs, ys = np.arange(5.0), np.arange(5.0)
    assert po.run(z, xs, ys)["allocation"][2, 2] == 1
    z[0, 2] = 0
    assert po.run(z, xs, ys)["allocation"][2, 2] == 2                    # the cell's own row counts as above
    z[2, 0] = z[2, 4] = 0
    z[4, 1] = z[4, 3] = 5
    z[3, 2], z[4, 2] = 0, 0
    assert po.run(z, xs, ys)["allocation"][3, 2] == 5 and po.run(z, xs, ys)["col"][3, 2] == 3     # below: the last one


# ------------------------------------------------------------------ the host side of the public functions
def test_the_new_names_are_exported():
    import xrspatial_amd as xa
    for name in ("proximity", "allocation", "direction", "euclidean_distance", "manhattan_distance", "great_circle_distance"):
        assert callable(getattr(xa, name)), name


def test_scalar_helpers():
    import xrspatial_amd as xa
    assert xa.euclidean_distance(142.32, 312.54, 23.23, 432.01) == 442.80462599209596           # the reference's docstrings
    assert xa.manhattan_distance(142.32, 312.54, 23.23, 432.01) == pytest.approx(579.0, rel=1e-15)
    assert xa.great_circle_distance(123.2, 178.0, 82.32, 65.09) == pytest.approx(2378290.489801402, rel=1e-12)
    assert xa.great_circle_distance(0, 90, 0, 0, radius=1) == pytest.approx(np.pi / 2, rel=1e-15)
    for args, text in (((180.1, 0, 0, 0), "x-coordinate of the first"), ((0, -181, 0, 0), "x-coordinate of the second"),
                       ((0, 0, 90.5, 0), "y-coordinate of the first"), ((0, 0, 0, -91), "y-coordinate of the second")):
        with pytest.raises(ValueError, match=text):
            xa.great_circle_distance(*args)
    for c in GC_CASES[:1]:                                               # the helper is the rule's arithmetic
        xs, ys = FIXTURE[f"{c}/xs"], FIXTURE[f"{c}/ys"]
        assert np.float32(xa.great_circle_distance(xs[3], xs[40], ys[5], ys[30])) == po.distance(xs[3], xs[40], ys[5], ys[30], 1)


def _capture(monkeypatch):
    mod = importlib.import_module("xrspatial_amd.proximity")
    seen = {}

    def fake(data, xs, ys, target_values, max_distance, metric, mode):
        seen.update(xs=xs, ys=ys, target_values=target_values, max_distance=max_distance, metric=metric, mode=mode)
        return np.zeros(data.shape, np.float32)

    monkeypatch.setattr(mod, "_run", fake)
    return mod, seen


def test_argument_handling_of_the_reference(monkeypatch):
    import xrspatial_amd as xa
    mod, seen = _capture(monkeypatch)
    z = np.zeros((3, 4), np.int16)
    agg = _agg(z, [10, 20, 30, 40], [3.0, 2.0, 1.0], attrs={"crs": 4326})
    out = xa.proximity(agg, max_distance=None, distance_metric="CHEBYSHEV")
    assert (seen["metric"], seen["mode"], seen["max_distance"]) == (mod.EUCLIDEAN, mod.PROXIMITY, np.inf)
    assert seen["xs"].dtype == np.float64 and seen["xs"].tolist() == [10, 20, 30, 40] and seen["ys"].tolist() == [3, 2, 1]
    assert tuple(out.dims) == ("y", "x") and out.attrs == {"crs": 4326} and out.data.dtype == np.float32
    assert np.array_equal(np.asarray(out["x"].data), [10, 20, 30, 40]) and np.array_equal(np.asarray(out["y"].data), [3.0, 2.0, 1.0])
    xa.allocation(agg, target_values=[2, 3], max_distance=5, distance_metric="MANHATTAN")
    assert (seen["metric"], seen["mode"], seen["max_distance"], list(seen["target_values"])) == (mod.MANHATTAN, mod.ALLOCATION, 5.0, [2, 3])
    xa.direction(agg, distance_metric="GREAT_CIRCLE")
    assert (seen["metric"], seen["mode"]) == (mod.GREAT_CIRCLE, mod.DIRECTION)
    lonlat = _agg(z, [1., 2., 3., 4.], [5., 6., 7.], dims=("lat", "lon"))
    with pytest.raises(ValueError, match=r"raster.coords should be named as coordinates:\(y, x\)"):
        xa.proximity(lonlat)
    assert tuple(xa.proximity(lonlat, x="lon", y="lat").dims) == ("lat", "lon")
    with pytest.raises(ValueError, match="should be named"):
        xa.proximity(_agg(z, dims=("x", "y")))
    ds = xa.Dataset({"a": agg, "b": agg}, attrs={"k": 1})                # Dataset in, Dataset out
    res = xa.direction(ds)
    assert isinstance(res, xa.Dataset) and set(res.data_vars) == {"a", "b"} and res.attrs == {"k": 1}


def test_coordinate_checks_come_before_device_work():
    import xrspatial_amd as xa
    z = np.zeros((3, 4), np.float32)
    for fn in (xa.proximity, xa.allocation, xa.direction):
        with pytest.raises(ValueError, match="x coordinates are not strictly monotonic"):
            fn(_agg(z, [0., 1., 1., 2.], [0., 1., 2.]))
        with pytest.raises(ValueError, match="y coordinates are not strictly monotonic"):
            fn(_agg(z, [0., 1., 2., 3.], [0., 2., 1.]))
        with pytest.raises(ValueError, match="x coordinates are not finite"):
            fn(_agg(z, [0., 1., np.nan, 3.], [0., 1., 2.]))
        with pytest.raises(ValueError, match="y coordinates are not finite"):
            fn(_agg(z, [0., 1., 2., 3.], [0., np.inf, 2.]))
    with pytest.raises(ValueError, match="lat coordinates are not strictly"):
        xa.proximity(_agg(z, [0., 1., 2., 3.], [0., 0., 1.], dims=("lat", "lon")), x="lon", y="lat")
    with pytest.raises(ValueError, match="max_distance is NaN"):
        xa.proximity(_agg(z), max_distance=float("nan"))
    # GREAT_CIRCLE: the reference's range errors
    with pytest.raises(ValueError, match=r"Invalid x-coordinate of the second point.Must be in the range \[-180, 180\]"):
        xa.proximity(_agg(z, [100., 140., 179., 181.], [0., 1., 2.]), distance_metric="GREAT_CIRCLE")
    with pytest.raises(ValueError, match=r"Invalid y-coordinate of the first point.Must be in the range \[-90, 90\]"):
        xa.allocation(_agg(z, [0., 1., 2., 3.], [91., 1., 0.]), distance_metric="GREAT_CIRCLE")
    with pytest.raises(ValueError, match="Invalid x-coordinate of the first"):
        xa.direction(_agg(z, [-181., 1., 2., 3.], [9., 1., 0.]), distance_metric="GREAT_CIRCLE")


def test_target_values_reach_the_kernel_in_the_rasters_kind():
    mod = importlib.import_module("xrspatial_amd.proximity")
    big = 2 ** 53
    v, kind = mod.target_array([big + 1, 3], np.int64)
    assert kind == 1 and v.dtype == np.int64 and v.tolist() == [big + 1, 3]
    v, kind = mod.target_array(np.array([2 ** 63 + 5], np.uint64), np.uint64)
    assert kind == 2 and v.dtype == np.uint64 and int(v[0]) == 2 ** 63 + 5
    v, kind = mod.target_array([2, 3.5], np.int32)                       # floats: NumPy compares as float64
    assert kind == 0 and v.dtype == np.float64 and v.tolist() == [2.0, 3.5]
    v, kind = mod.target_array([2, 3], np.float32)
    assert kind == 0 and v.dtype == np.float64
    v, kind = mod.target_array([], np.int64)
    assert kind == 0 and v.size == 0
    with pytest.raises(TypeError):
        mod.target_array(["a"], np.int32)


def test_dask_backed_rasters_are_refused(monkeypatch):
    import xrspatial_amd as xa
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.zeros((8, 8), np.float32), (4, 4)))
    for fn in (xa.proximity, xa.allocation, xa.direction):
        with pytest.raises(NotImplementedError, match="dask"):
            fn(lazy)


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xa
    if xa.has_hip():
        pytest.skip("a GPU is present")
    for dt in (np.float32, np.int64, np.bool_):
        with pytest.raises(xa.XrsError):
            xa.proximity(_agg(np.zeros((4, 4), dt)))


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_proximity validates on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    up = lambda v: (v + 255) // 256 * 256                                # noqa: E731
    assert lib.xrs_proximity_workspace_bytes(300, 400) == 2 * up(300 * 400 * 4) + 2 * up(300 * 4) + 256
    assert lib.xrs_proximity_workspace_bytes(0, 5) == 0 and lib.xrs_proximity_workspace_bytes(5, -1) == 0

    def call(data=fake, dtype=9, rows=4, cols=5, xs=fake, ys=fake, gc=None, values=None, kind=0, n=0, md=np.inf, metric=0, mode=0,
             work=fake, out=fake):
        return lib.xrs_proximity(data, dtype, rows, cols, xs, ys, gc, values, kind, n, md, metric, mode, work, out, None)

    for kw, text in ((dict(rows=-1), "negative shape"), (dict(mode=4), "unknown mode"), (dict(mode=48), "unknown mode"),
                     (dict(metric=3), "unknown metric"), (dict(dtype=10), "dtype"), (dict(dtype=-1), "dtype"), (dict(n=-1), "negative number"),
                     (dict(kind=3), "kind"), (dict(kind=1, dtype=8), "float raster"), (dict(data=None), "null"), (dict(xs=None), "null"),
                     (dict(ys=None), "null"), (dict(work=None), "null"), (dict(out=None), "null"), (dict(n=2), "null"),
                     (dict(metric=1), "radians"), (dict(md=float("nan")), "NaN"), (dict(cols=1 << 31), "too large"),
                     (dict(rows=1 << 30, cols=1 << 12), "too large"),
                     (dict(mode=3 | 16 | 32), "unknown mode"), (dict(mode=16 | 32), "unknown mode"),      # both halves left out
                     (dict(mode=3 | 64), "unknown mode"), (dict(mode=8), "unknown mode"), (dict(mode=-1), "unknown mode"),
                     (dict(mode=1 | 256), "unknown mode"),
                     (dict(mode=32, out=None), "null"), (dict(mode=3 | 32, out=None), "null"),             # SEARCH_ONLY writes planes
                     (dict(mode=16, out=None, work=None), "null"), (dict(mode=16, out=None, cols=1 << 31), "too large")):
        assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    assert call(rows=0) == 0 and call(cols=0, data=None, work=None, out=None) == 0       # nothing to do
    # SCAN_ONLY writes no plane: a null out_dev is accepted.  Without a device that shows in the NEXT check being the one that
    # refuses (max_distance is looked at after the pointers); tests/test_gpu_proximity_abi.py runs every scan that way.
    for mode in (16, 3 | 16):
        assert call(mode=mode, out=None, md=float("nan")) != 0 and "NaN" in _lib.last_error(), mode
    assert call(mode=32, out=None, md=float("nan")) != 0 and "null" in _lib.last_error()

"""CPU checks of viewshed: the restatement (tests/viewshed_oracle.py) against the reference's own outputs
(tests/golden/viewshed_exec.npz), bit for bit; how far the reference's cells lie from the verdict's edge; the viewpoint lookup,
the argument checks and the refusals, all of which run before any device work."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import viewshed_oracle as vo
from tests.golden import make_viewshed_exec as gen

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)
RELIEF = [n for n in CASES if n.startswith("relief_")]
BAND, BAND_SHARE = 1e-10, 0.005
# cases whose cells at the verdict's edge are ties of gradients that are exactly 0 on both sides (level ground seen from
# ground level): tests/test_gpu_viewshed.py asks the device for the same verdict there, atan(0) being 0 everywhere
ZERO_TIES = ("plane_obs0", "doc")


def _agg(a, **kw):
    import xrspatial_amd as xs
    return xs.DataArray(a, dims=["y", "x"], **kw)


@pytest.fixture(scope="module")
def oracle_runs():
    return {name: vo.run(*gen.call_args(FIXTURE, name)) for name in CASES}


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference_bit_for_bit(oracle_runs, case):
    got, want = oracle_runs[case][0], FIXTURE[f"{case}/out"]
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{np.count_nonzero(got != want)} cells differ"


@pytest.mark.parametrize("case", RELIEF)
def test_relief_cells_lie_clear_of_the_verdicts_edge(oracle_runs, case):
    """no cell of the executed reference is within 1e-10 rad of changing its verdict (the band the GPU test leaves open);
    0.5 % is the bound, so that a regenerated fixture cannot drift into the band unnoticed"""
    margin = oracle_runs[case][1]
    share = float(np.mean(margin <= BAND))
    print(f"{case}: {int(np.sum(margin <= BAND))} of {margin.size} cells in band, smallest margin {margin.min():.3g}")
    assert share <= BAND_SHARE
    assert share == 0.0


@pytest.mark.parametrize("case", ZERO_TIES)
def test_zero_ties_are_level_cells(oracle_runs, case):
    out, margin = oracle_runs[case]
    tie = margin <= BAND
    assert tie.any() and (margin[tie] == 0).all() and (out[tie] == 90.0).all()        # visible, at the observer's height


def test_fixture_covers_what_the_spec_lists():
    doc = [[-1., 90., 135., 90., -1.], [-1., 161.56505118, 180., 90., 90.], [167.39561735, 144.73561032, 168.69006753, 144.73561032, -1.],
           [165.57993189, -1., -1., 166.0472636, -1.]]                                   # as the reference's docstring prints it
    np.testing.assert_allclose(FIXTURE["doc/out"], np.array(doc), rtol=0, atol=5e-9)
    for obs in (5, 2):                                                                   # the reference's test_viewshed_flat
        for tgt in (0, 1):
            z, xs, ys, x, y, _, _ = gen.call_args(FIXTURE, f"flat_obs{obs}_tgt{tgt}")
            assert z.shape == (5, 4) and (z == 1.3).all()
            xx, yy = np.meshgrid(xs, ys)
            angle = np.rad2deg(np.arctan2(np.sqrt((xx - x) ** 2 + (yy - y) ** 2), obs - tgt))
            angle[0, 0] = 180.0
            np.testing.assert_allclose(FIXTURE[f"flat_obs{obs}_tgt{tgt}/out"], angle)
    assert (np.delete(FIXTURE["plane_obs0/out"].ravel(), 4 * 13 + 7) == 90.0).all() and FIXTURE["plane_obs0/out"][4, 7] == 180.0
    assert {"ramp", "stairs", "nan_0", "nan_1"} <= set(CASES)
    assert np.isnan(FIXTURE["nan_0/z"]).any() and np.isnan(FIXTURE["nan_1/z"]).any()
    assert not any(np.isnan(FIXTURE[f"{n}/z"]).any() for n in CASES if not n.startswith("nan_"))
    for shape in ((37, 53), (64, 96)):
        for dt in ("f32", "f64"):
            z = FIXTURE[f"relief_{shape[0]}x{shape[1]}_{dt}/z"]
            assert z.shape == shape and z.dtype == np.dtype("float32" if dt == "f32" else "float64")
            assert (z != np.round(z)).all()
    views, resolutions, dtypes = set(), set(), set()
    for n in RELIEF:
        z, xs, ys, x, y, _, _ = gen.call_args(FIXTURE, n)
        r, c = vo.locate(ys, y, "y"), vo.locate(xs, x, "x")
        h, w = z.shape
        views.add(((r == 0) - (r == h - 1), (c == 0) - (c == w - 1)))
        resolutions.add((round(float(xs[1] - xs[0]), 6), round(float(ys[1] - ys[0]), 6)))
        dtypes.add(z.dtype.name)
        out = FIXTURE[f"{n}/out"]
        assert out[r, c] == 180.0 and (out == -1).any() and ((out >= 0) & (out < 180)).any()
    assert len(views) == 9                                           # four corners, four edges, inside
    assert resolutions == set(gen.RESOLUTIONS) and dtypes == {"float32", "float64"}


# ------------------------------------------------------------------ the host side of the public function
def _capture(monkeypatch):
    mod = importlib.import_module("xrspatial_amd.viewshed")
    seen = {}

    def fake(data, row, col, observer_elev, target_elev, ew_res, ns_res):
        seen.update(row=row, col=col, observer_elev=observer_elev, target_elev=target_elev, ew_res=ew_res, ns_res=ns_res,
                    dtype=data.dtype)
        return np.full(data.shape, -1.0)

    monkeypatch.setattr(mod, "_run", fake)
    return mod, seen


def test_viewpoint_lookup(monkeypatch):
    import xrspatial_amd as xs
    mod, seen = _capture(monkeypatch)
    z = np.zeros((4, 6), np.float32)
    agg = _agg(z, coords={"y": [40.0, 30.0, 20.0, 10.0], "x": [0.0, 2.5, 5.0, 7.5, 10.0, 12.5]}, attrs={"crs": 3857})
    out = xs.viewshed(agg, x=7.4, y=21, observer_elev=3, target_elev=1.5)
    assert seen == dict(row=2, col=3, observer_elev=3.0, target_elev=1.5, ew_res=2.5, ns_res=-10.0, dtype=np.float32)
    assert tuple(out.dims) == ("y", "x") and out.attrs == {"crs": 3857} and out.data.dtype == np.float64
    assert np.array_equal(np.asarray(out["y"].data), [40.0, 30.0, 20.0, 10.0]) and np.array_equal(np.asarray(out["x"].data), agg["x"].data)
    # of two equally near coordinates the larger one wins, on an ascending and on a descending axis (pandas' `nearest`)
    xs.viewshed(agg, x=3.75, y=25)
    assert (seen["row"], seen["col"]) == (1, 2)
    xs.viewshed(agg, x=12.5, y=10)                                   # the ranges are closed
    assert (seen["row"], seen["col"]) == (3, 5)
    for coords, v, want in (([10.0, 20.0, 30.0, 40.0], 15, 1), ([40.0, 30.0, 20.0, 10.0], 15, 2), ([0, 1, 2, 3], 1.5, 2),
                            ([0.0, 1.0, 1.0, 2.0], 1.2, 1), ([5.0, 5.0, 7.0], 5, 0), ([3.0, 1.0, 2.0], 1.4, 1)):
        assert mod.nearest_index(np.array(coords), v, "x") == want == vo.locate(coords, v, "x"), (coords, v)
    # no coordinates: the integer index; integer rasters are read as float64
    out = xs.viewshed(xs.DataArray(np.zeros((3, 5), np.int16), dims=["lat", "lon"]), x=3.2, y=0.5)
    assert (seen["row"], seen["col"], seen["ew_res"], seen["ns_res"]) == (1, 3, 1.0, 1.0) and tuple(out.dims) == ("lat", "lon")
    # the fixture's viewpoints, through the package's lookup and the restatement's
    for n in CASES:
        z, xc, yc, x, y, obs, tgt = gen.call_args(FIXTURE, n)
        xs.viewshed(_agg(z, coords={"y": yc, "x": xc}), x, y, obs, tgt)
        assert (seen["row"], seen["col"]) == (vo.locate(yc, y, "y"), vo.locate(xc, x, "x"))
        assert seen["ew_res"] == (xc[-1] - xc[0]) / (z.shape[1] - 1) and seen["ns_res"] == (yc[-1] - yc[0]) / (z.shape[0] - 1)


def test_argument_errors_come_before_device_work():
    import xrspatial_amd as xs
    agg = _agg(np.zeros((4, 5), np.float32), coords={"y": np.arange(4) * 2.0, "x": np.arange(5) + 10.0})
    with pytest.raises(ValueError, match="x argument outside of raster x_range"):
        xs.viewshed(agg, x=9.9, y=2)
    with pytest.raises(ValueError, match="x argument outside of raster x_range"):
        xs.viewshed(agg, x=14.01, y=2)
    with pytest.raises(ValueError, match="y argument outside of raster y_range"):
        xs.viewshed(agg, x=12, y=-0.5)
    with pytest.raises(ValueError, match="y argument outside of raster y_range"):
        xs.viewshed(agg, x=12, y=float("nan"))
    with pytest.raises(ValueError, match="2-D"):
        xs.viewshed(xs.DataArray(np.zeros(5, np.float32), dims=["x"]), x=1, y=0)
    with pytest.raises(ValueError, match="2-D"):
        xs.viewshed(xs.DataArray(np.zeros((2, 3, 4), np.float32), dims=["b", "y", "x"]), x=1, y=0)
    for shape in ((1, 5), (5, 1), (1, 1)):
        with pytest.raises(ValueError, match="two cells"):
            xs.viewshed(_agg(np.zeros(shape, np.float64)), x=0, y=0)
    for kw in (dict(observer_elev=float("inf")), dict(target_elev=float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            xs.viewshed(agg, x=12, y=2, **kw)


def test_dask_backed_raster_is_refused(monkeypatch):
    import xrspatial_amd as xs
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.zeros((8, 8), np.float32), (4, 4)))
    with pytest.raises(NotImplementedError, match="dask"):
        xs.viewshed(lazy, x=1, y=1)


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xs
    if xs.has_hip():
        pytest.skip("a GPU is present")
    for dt in (np.float32, np.float64, np.int32):
        with pytest.raises(xs.XrsError):
            xs.viewshed(_agg(np.zeros((4, 4), dt)), x=1, y=1)


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_viewshed_* validate on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    assert lib.xrs_viewshed_workspace_bytes(300, 400) == 300 * 400 * 24 and lib.xrs_viewshed_workspace_bytes(0, 5) == 0

    def call(fn=lib.xrs_viewshed_f32, data=fake, rows=4, cols=5, vr=1, vc=2, obs=0.0, tgt=0.0, ew=1.0, ns=1.0, work=fake, out=fake):
        return fn(data, rows, cols, vr, vc, obs, tgt, ew, ns, work, out, None)

    for kw, text in ((dict(rows=1), "2 x 2"), (dict(cols=1), "2 x 2"), (dict(rows=-3), "2 x 2"), (dict(vr=4), "outside"),
                     (dict(vc=-1), "outside"), (dict(data=None), "null"), (dict(work=None), "null"), (dict(out=None), "null"),
                     (dict(ew=float("nan")), "non-finite"), (dict(obs=float("inf")), "non-finite"), (dict(rows=1 << 30), "too large"),
                     (dict(fn=lib.xrs_viewshed_f64, vr=9), "outside")):
        assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())

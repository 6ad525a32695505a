"""viewshed on the MI355X, through the public function, against the reference's own outputs (tests/golden/viewshed_exec.npz)
and, at the shapes the fixture lacks, against the restatement (tests/viewshed_oracle.py).

Rule: the visible mask equals the expected one at every cell whose margin (|largest occluder gradient - the cell's own
gradient|, from the restatement) is above 1e-10 rad; a cell within that band may fall either way, and at most 0.5 % of a
case's cells may lie in it (the executed reference has none on relief: tests/test_viewshed_host.py).  Why 1e-10: the device's
atan may differ from libm's by a few ulp (4e-16 on values up to pi / 2), and the interpolation weight divides by an angular
span of at least ~2e-3 rad at these ray lengths, so a gradient is off by ~1e-12 at most; 1e-10 leaves two orders of room and
is still below every margin of these cases (the smallest of a case: 4e-9 .. 3e-5 on relief of up to 120 000 cells).  Ties of gradients that are exactly 0 on both sides (level ground
seen from ground level: the flat plane with observer 0 and one cell of the docstring example) are not in that band for
this purpose: atan(0) is 0 on any device, and the mask must equal the reference's everywhere.

Values at the cells both sides see: assert_allclose(rtol=1e-12, atol=0), four orders above a few ulp of atan; the largest
error seen is recorded (tests/parity_log.py) together with the number of cells in band."""
import numpy as np
import pytest

from tests import parity_log
from tests import viewshed_oracle as vo
from tests.golden import make_viewshed_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = [n for n in gen.names(FIXTURE) if n not in gen.EXACT]
ZERO_TIES = ("plane_obs0", "doc")
BAND, BAND_SHARE, RTOL = 1e-10, 0.005, 1e-12


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xs, z, xc=None, yc=None, **kw):
    coords = None if xc is None else {"y": yc, "x": xc}
    return xs.DataArray(z, dims=["y", "x"], coords=coords, **kw)


def _check(got, want, margin, what, exact=False):
    """the rule of the module docstring"""
    assert got.dtype == np.float64 and got.shape == want.shape, what
    band = np.zeros(want.shape, bool) if exact else margin <= BAND
    differ = (got == -1) != (want == -1)
    print(f"{what}: {int(band.sum())} of {band.size} cells in band, {int(differ.sum())} verdicts differ")
    assert band.mean() <= BAND_SHARE, (what, int(band.sum()))
    assert not (differ & ~band).any(), (what, np.argwhere(differ & ~band)[:10].tolist(), margin[differ & ~band][:10])
    both = (got != -1) & (want != -1)
    max_rel, _ = parity_log.record(what, "viewshed", got[both], want[both], tol=RTOL,
                                   note=f"{int(band.sum())} cells within {BAND} rad of the verdict's edge, {int(differ.sum())} differ")
    print(f"{what}: largest relative error of the angle {max_rel:.3g}")
    np.testing.assert_allclose(got[both], want[both], rtol=RTOL, atol=0, err_msg=what)
    assert ((got == -1) | ((got >= 0) & (got <= 180))).all(), what


# ------------------------------------------------------------------ against the executed reference
@pytest.mark.parametrize("case", CASES)
def test_viewshed_equals_the_reference(xs, case):
    z, xc, yc, x, y, obs, tgt = gen.call_args(FIXTURE, case)
    before = z.copy()
    agg = _agg(xs, z, xc, yc, attrs={"crs": "EPSG:3857"})
    out = xs.viewshed(agg, x, y, obs, tgt)
    assert isinstance(out.data, np.ndarray) and tuple(out.dims) == ("y", "x") and out.attrs == {"crs": "EPSG:3857"}
    assert np.array_equal(np.asarray(out["x"].data), xc) and np.array_equal(np.asarray(out["y"].data), yc)
    assert agg.data is z and z.dtype == before.dtype and np.array_equal(z, before, equal_nan=True)      # the input is left alone
    _, margin = vo.run(z, xc, yc, x, y, obs, tgt)
    _check(out.data, FIXTURE[f"{case}/out"], margin, case, exact=case in ZERO_TIES)
    if case == "plane_obs0":
        assert (out.data != -1).all()


# ------------------------------------------------------------------ against the restatement, shapes the fixture lacks
# 16 x 16 tiles of 8 x 8 waves divide neither shape; rays from a corner cross up to 25 tiles
BIG = {(130, 257): dict(res=(2.5, 70.0), observer_elev=150, target_elev=0), (300, 400): dict(res=(30.0, -30.0), observer_elev=100, target_elev=1.5)}
VIEWS = {"corner": lambda h, w: (h - 1, 0), "edge": lambda h, w: (0, w // 2), "centre": lambda h, w: (h // 2, w // 2)}
_expected = {}


def _big_case(shape, where):
    """raster, arguments and the restatement's (out, margin), computed once per shape and viewpoint: the relief is drawn in
    float32, so the float64 raster holds the same values and both dtypes share one reference"""
    key = (shape, where)
    if key not in _expected:
        kw = BIG[shape]
        z = gen.relief(shape, 11 + shape[0], np.float32)
        xc = 100.0 + kw["res"][0] * np.arange(shape[1])
        yc = 5000.0 + kw["res"][1] * np.arange(shape[0])
        vr, vc = VIEWS[where](*shape)
        args = (float(xc[vc]), float(yc[vr]), kw["observer_elev"], kw["target_elev"])
        _expected[key] = (z, xc, yc, args, vo.run(z, xc, yc, *args))
    return _expected[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("where", list(VIEWS))
@pytest.mark.parametrize("shape", list(BIG))
def test_viewshed_equals_the_restatement(xs, shape, where, dtype):
    z, xc, yc, args, (want, margin) = _big_case(shape, where)
    out = xs.viewshed(_agg(xs, z.astype(dtype), xc, yc), *args)
    assert 0.02 < np.mean(want != -1) < 0.98                       # hidden and seen cells, both in numbers
    _check(out.data, want, margin, f"viewshed_{shape[0]}x{shape[1]}_{where}_{np.dtype(dtype).name}")


@pytest.mark.parametrize("shape,view", [((2, 2), (0, 1)), ((2, 2), (1, 0)), ((2, 40), (1, 5)), ((2, 40), (0, 39)), ((40, 2), (17, 0)),
                                        ((40, 2), (0, 1))])
def test_thin_rasters(xs, shape, view):
    z = gen.relief(shape, 3, np.float64)
    want, margin = vo.viewshed(z, view[0], view[1], 1.0, 1.0, 2, 0)
    out = xs.viewshed(_agg(xs, z), x=view[1], y=view[0], observer_elev=2)          # no coordinates: the integer index
    _check(out.data, want, margin, f"viewshed_{shape[0]}x{shape[1]}_{view[0]}_{view[1]}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16, np.bool_])
def test_device_array_in_device_array_out(xs, dtype):
    rng = np.random.default_rng(5)
    z = (gen.relief((37, 53), 9, np.float64) if np.dtype(dtype).kind == "f" else rng.integers(0, 2 if dtype is np.bool_ else 40, (37, 53))).astype(dtype)
    xc, yc = np.arange(53) * 10.0, np.arange(37) * 10.0
    host = xs.viewshed(_agg(xs, z, xc, yc), 250, 180, 5, 1)
    dev_in = xs.DeviceArray.from_numpy(z)
    dev = xs.viewshed(_agg(xs, dev_in, xc, yc, attrs={"k": 1}), 250, 180, 5, 1)
    assert isinstance(dev.data, xs.DeviceArray) and dev.data.dtype == np.float64 and dev.attrs == {"k": 1}
    assert np.array_equal(dev.data.get(), host.data)
    assert dev_in.dtype == np.dtype(dtype) and np.array_equal(dev_in.get(), z)     # the input is left alone
    want, margin = vo.run(z, xc, yc, 250, 180, 5, 1)
    _check(host.data, want, margin, f"viewshed_37x53_{np.dtype(dtype).name}")


def test_nan_viewpoint_and_nan_cells(xs):
    """NaN cells are never visible and never hide a cell; from a NaN viewpoint nothing is visible (where the reference's
    sweep raises for some NaN layouts, the predicate is the contract)"""
    z = gen.relief((20, 30), 4, np.float64)
    z[np.random.default_rng(4).random(z.shape) < 0.06] = np.nan
    z[7, 12] = 30.0
    want, margin = vo.viewshed(z, 7, 12, 1.0, 1.0, 5, 0)
    out = xs.viewshed(_agg(xs, z), x=12, y=7, observer_elev=5)
    _check(out.data, want, margin, "viewshed_nan_cells")
    assert (out.data[np.isnan(z)] == -1).all()
    z[7, 12] = np.nan
    out = xs.viewshed(_agg(xs, z), x=12, y=7, observer_elev=5).data
    assert out[7, 12] == 180 and (np.delete(out.ravel(), 7 * 30 + 12) == -1).all()


def test_sharded_raster_is_refused(xs):
    sh = xs.ShardedArray(8, 8, np.float32)
    with pytest.raises(NotImplementedError, match="sharded"):
        xs.viewshed(xs.DataArray(sh, dims=["y", "x"]), x=1, y=1)

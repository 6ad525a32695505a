"""viewshed(method='mesh') on the MI355X, through the public function, against the brute-force evaluation of the rule
(tests/viewshed_mesh_oracle.py: every target against every triangle, NumPy float64).

Rule of the comparison: the -1 mask equals the oracle's at EVERY cell -- nothing is tolerated and no cell is left out: the
kernel runs the rule's own operations in the rule's order with contraction off, and the walk's accelerations may only skip
triangles the rule rejects -- and the visible values equal the oracle's as float32 bits.  One exception: the device's `atan`
need not equal `math.atan` to the last float64 bit, so a cell may differ by one float32 ulp where the oracle's float64 angle
lies within 1e-13 relative (500 float64 ulps, against a float32 spacing of 2^29 of them) of the midpoint of the two float32
values; the test computes that per cell and records any such cell with tests/parity_log.py.  None is expected.

Shapes: 2 x 2, 2 x 40 and 40 x 2 (every cell is a border cell), 5 x 4, 9 x 130 and 70 x 17 (long thin both ways), 33 x 47 (odd),
16 x 16 and 33 x 33, each from every viewpoint (the four corners, the centre, a mid-edge cell, (H - 2, W - 2) beside the
stepped-back origins, (H - 1, W // 2)) at every elevation pair; 64 x 64 and 65 x 49 (63 and 64 cells: one short of the walk's
32-cell blocks and exactly two of them) with one case per viewpoint and pair.  Every raster other than the level plane must
show a visible share between 0.1 and 0.9 at some viewpoint and pair wherever it has at least 9 rows and columns (asserted
per raster and shape): no case passes on an empty or a full mask alone."""
import numpy as np
import pytest

from tests import parity_log
from tests import viewshed_mesh_oracle as vo
from tests.test_gpu_hillshade_shadow import ridge, rough

pytestmark = pytest.mark.gpu

ELEVS = [(0, 0), (5, 0), (2, 1), (30, 0)]                          # (observer_elev, target_elev)
SMALL = [(2, 2), (2, 40), (40, 2), (5, 4), (9, 130), (70, 17), (33, 47), (16, 16), (33, 33)]
LARGE = [(64, 64), (65, 49)]                   # the brute force takes about a second per case here: one case per parameter
EW, NS = 0.5, 1.5                              # cell sizes: they move the angles, never the verdicts


def smooth(shape):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return (10 + 6 * np.sin(0.35 * xx) * np.cos(0.28 * yy) + 4 * np.sin(0.11 * (xx + yy))).astype(np.float32)


def plane(shape):
    return np.full(shape, 5.0, np.float32)


RASTERS = {"ridge": ridge, "smooth": smooth, "rough": rough, "plane": plane}


def viewpoints(shape):
    H, W = shape
    return list(dict.fromkeys([(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (0, W // 2), (H - 2, W - 2), (H - 1, W // 2)]))


def _coords(shape):
    return {"y": np.arange(shape[0]) * NS, "x": np.arange(shape[1]) * EW}


def _resolutions(shape):
    c = _coords(shape)
    return float(c["x"][-1] - c["x"][0]) / (shape[1] - 1), float(c["y"][-1] - c["y"][0]) / (shape[0] - 1)


_expected = {}


def expected(kind, shape, view, elev, dtype=np.float32):
    """(raster, oracle out, invisible mask, float64 angles), computed once per case and left unchanged"""
    key = (kind, shape, view, elev, np.dtype(dtype).name)
    if key not in _expected:
        z = RASTERS[kind](shape).astype(dtype)
        ew, ns = _resolutions(shape)
        out, mask, ang = vo.viewshed_mesh(z, view[0], view[1], elev[0], elev[1], ew, ns)
        for a in (z, out, mask, ang):
            a.setflags(write=False)
        _expected[key] = (z, out, mask, ang)
    return _expected[key]


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xs, z, **kw):
    return xs.DataArray(z, dims=["y", "x"], coords=_coords(z.shape), **kw)


def _check(got, want, mask, ang, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    got_mask = got == -1
    differ = got_mask != mask
    share = 1.0 - float(mask.mean())
    seen = ~mask
    off = seen & ~differ & (got.view(np.uint32) != want.view(np.uint32))
    print(f"{what}: visible share {share:.3f}, {int(differ.sum())} verdicts differ, {int(off.sum())} values differ")
    assert not differ.any(), (what, np.argwhere(differ)[:10].tolist())
    if off.any():                              # (module docstring: one ulp, and only on a float32 rounding midpoint)
        g, w, a = got[off], want[off], ang[off]
        assert (np.abs(g.view(np.int32).astype(np.int64) - w.view(np.int32)) == 1).all(), (what, np.argwhere(off)[:10].tolist())
        mid = (g.astype(np.float64) + w.astype(np.float64)) / 2
        assert (np.abs(a - mid) <= 1e-13 * np.abs(a)).all(), (what, np.argwhere(off)[:10].tolist(), g[:10], w[:10])
        parity_log.record("viewshed_mesh", what, g, w, note=f"{int(off.sum())} cells one float32 ulp off on a rounding midpoint")
    return share


def _run_case(xs, kind, shape, view, elev):
    z, want, mask, ang = expected(kind, shape, view, elev)
    before = z.copy()
    c = _coords(shape)
    out = xs.viewshed(_agg(xs, z, attrs={"crs": 3857}), x=c["x"][view[1]], y=c["y"][view[0]], observer_elev=elev[0], target_elev=elev[1],
                      method="mesh")
    assert isinstance(out.data, np.ndarray) and tuple(out.dims) == ("y", "x") and out.attrs == {"crs": 3857} and out.name == "viewshed"
    assert np.array_equal(np.asarray(out["x"].data), c["x"]) and np.array_equal(np.asarray(out["y"].data), c["y"])
    assert np.array_equal(z, before)                               # the input is left alone
    assert out.data[view] == 180 and not mask[view]
    return _check(out.data, want, mask, ang, f"viewshed_mesh_{kind}_{shape[0]}x{shape[1]}_v{view[0]}_{view[1]}_oe{elev[0]}_te{elev[1]}")


def _id(v):
    return "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v)


SMALL_CASES = [(kind, shape, view) for kind in RASTERS for shape in SMALL for view in viewpoints(shape)]
LARGE_CASES = [(kind, shape, view, elev) for kind in RASTERS for shape in LARGE for view in viewpoints(shape) for elev in ELEVS]


@pytest.mark.parametrize("kind,shape,view", SMALL_CASES, ids=lambda v: _id(v))
def test_equals_the_brute_force_at_every_elevation_pair(xs, kind, shape, view):
    shares = [_run_case(xs, kind, shape, view, elev) for elev in ELEVS]
    if kind == "plane":
        assert shares == [1.0] * len(ELEVS)                        # level with the observer too


@pytest.mark.parametrize("kind,shape,view,elev", LARGE_CASES, ids=lambda v: _id(v))
def test_equals_the_brute_force_across_blocks(xs, kind, shape, view, elev):
    share = _run_case(xs, kind, shape, view, elev)
    assert kind != "plane" or share == 1.0


@pytest.mark.parametrize("shape", [s for s in SMALL + LARGE if min(s) >= 9], ids=_id)
@pytest.mark.parametrize("kind", ["ridge", "smooth", "rough"])
def test_cases_hold_mixed_masks(kind, shape):
    """the condition on the visible shares (the oracle's results are shared with the cases above): from the centre, where
    every one of these rasters shows one; small shapes from the other viewpoints as well"""
    H, W = shape
    views = [(H // 2, W // 2)] + ([] if shape in LARGE else [v for v in viewpoints(shape) if v != (H // 2, W // 2)])
    for view in views:
        for elev in ELEVS:
            if 0.1 < 1.0 - expected(kind, shape, view, elev)[2].mean() < 0.9:
                return
    raise AssertionError((kind, shape))


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_other_dtypes(xs, dtype):
    """a float64 copy holds the same values (one reference); int16 truncates them and goes through the float64 conversion"""
    shape, view, elev = (33, 47), (16, 23), (5, 0)
    z, want, mask, ang = expected("rough", shape, view, elev, np.float32 if dtype is np.float64 else dtype)
    z = z.astype(dtype)
    before = z.copy()
    c = _coords(shape)
    out = xs.viewshed_mesh(_agg(xs, z), c["x"][view[1]], c["y"][view[0]], elev[0], elev[1])
    assert z.dtype == np.dtype(dtype) and np.array_equal(z, before)
    share = _check(out.data, want, mask, ang, f"viewshed_mesh_rough_33x47_{np.dtype(dtype).name}")
    assert 0.1 < share < 0.9


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16])
def test_device_array_in_device_array_out(xs, dtype):
    shape, view, elev = (33, 47), (16, 23), (2, 1)
    z, want, mask, ang = expected("ridge", shape, view, elev, dtype)
    c = _coords(shape)
    dev_in = xs.DeviceArray.from_numpy(np.array(z))
    dev = xs.viewshed(_agg(xs, dev_in, attrs={"k": 1}), x=c["x"][view[1]], y=c["y"][view[0]], observer_elev=elev[0], target_elev=elev[1],
                      method="mesh")
    assert isinstance(dev.data, xs.DeviceArray) and dev.data.dtype == np.float32 and dev.attrs == {"k": 1} and dev.name == "viewshed"
    assert dev_in.dtype == np.dtype(dtype) and np.array_equal(dev_in.get(), z)      # the input is left alone
    share = _check(dev.data.get(), want, mask, ang, f"viewshed_mesh_ridge_33x47_device_{np.dtype(dtype).name}")
    assert 0.1 < share < 0.9


def test_abi_probe_walks_with_every_block_size(xs):
    """the measuring entry point at 65 x 49: every block size, one result, and counts that show the walk ran"""
    from xrspatial_amd import _lib
    shape, view, elev = (65, 49), (32, 24), (5, 0)
    z, want, mask, ang = expected("ridge", shape, view, elev)
    ew, ns = _resolutions(shape)
    lib = _lib.load()
    src = xs.DeviceArray.from_numpy(np.array(z))
    work = xs.DeviceArray((int(lib.xrs_viewshed_mesh_workspace_bytes(*shape)),), np.uint8)
    args = (src.ptr, shape[0], shape[1], float(max(shape)) / float(z.max()), float(z.min()), float(z.max()), view[0], view[1],
            float(elev[0]), float(elev[1]), ew, ns)
    out = xs.DeviceArray(shape, np.float32)
    _lib.call("xrs_viewshed_mesh_f32", *args, work.ptr, out.ptr, None)
    _lib.call("xrs_device_sync")
    _check(out.get(), want, mask, ang, "viewshed_mesh_abi_65x49")
    first = out.get()
    for block in (0, 8, 16, 32):
        out = xs.DeviceArray(shape, np.float32)
        counts = xs.DeviceArray.from_numpy(np.zeros(4, np.uint64))
        _lib.call("xrs_viewshed_mesh_probe_f32", *args, block, work.ptr, out.ptr, counts.ptr, None)
        _lib.call("xrs_device_sync")
        assert np.array_equal(out.get().view(np.uint32), first.view(np.uint32)), block
        c = counts.get()
        assert c[0] > 0 and 0 < c[1] <= max(shape) * 3 and (c[2] > 0) == (block != 0) and (c[3] > 0) == (block != 0), (block, c.tolist())


def test_sweep_is_the_existing_path(xs):
    z = expected("ridge", (33, 47), (16, 23), (5, 0))[0]
    a = xs.viewshed(_agg(xs, z), x=3.0, y=6.0, observer_elev=5, method="sweep")
    b = xs.viewshed(_agg(xs, z), x=3.0, y=6.0, observer_elev=5)
    assert a.data.dtype == b.data.dtype == np.float64 and np.array_equal(a.data, b.data) and a.name is None


def test_refusals_on_the_device(xs):
    z = rough((8, 9))
    bad = z.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        xs.viewshed(_agg(xs, bad), x=1, y=1.5, method="mesh")
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        xs.viewshed(_agg(xs, xs.DeviceArray.from_numpy(bad)), x=1, y=1.5, method="mesh")
    with pytest.raises(ValueError, match="positive"):
        xs.viewshed(_agg(xs, xs.DeviceArray.from_numpy(-z)), x=1, y=1.5, method="mesh")

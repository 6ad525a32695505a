"""hillshade(shadows=True) on the MI355X, through the public function, against the brute-force evaluation of the rule
(tests/hillshade_shadow_oracle.py: every interior cell against every triangle, NumPy float64).

Rule of the comparison: the float32 result equals the oracle's exactly at every cell, the NaN border included, and the shadow
mask -- recovered from the result as `out < 0.75 * unshadowed shade`, the unshadowed shade being positive at every interior
cell of these cases (asserted), so no cell is left out -- equals the oracle's mask at every cell.  Nothing is tolerated: the
kernel runs the rule's own operations in the rule's order with contraction off, and the walk's accelerations may only skip
triangles the rule rejects.

Shapes: 3 x 3 and 3 x 40 (one interior row), 9 x 130 and 70 x 17 (long thin both ways, many 8 x 8 patches and several blocks
along one axis), 33 x 47 (odd), 64 x 64 and 65 x 49 (63 and 64 cells: one short of the walk's 32-cell blocks and exactly two
of them), 16 x 16 and 33 x 33 (no interior block boundary at 16 and at 32 cells a block; one call at the ABI walks 65 x 49
with every block size).  Suns: every quadrant, both axes exactly, the horizon, the zenith, below the horizon.  Every raster other than the
level plane must have a sun position with a shadow share between 0.1 and 0.9 (asserted per raster and shape): no test passes
on an empty or a full mask alone."""
import importlib

import numpy as np
import pytest

from tests import hillshade_shadow_oracle as ho

pytestmark = pytest.mark.gpu

SUNS = [(225, 25), (90, 5), (0, 60), (315, 85), (180, 0), (45, 90), (135, -10)]            # (azimuth, altitude)
SMALL = [(3, 3), (3, 40), (9, 130), (70, 17), (33, 47), (16, 16), (33, 33)]
LARGE = [(64, 64), (65, 49)]                   # the brute force takes a second or two per sun here: one case per sun


def rough(shape):
    return (np.random.default_rng(shape[0] * 1000 + shape[1]).random(shape) * 100 + 1).astype(np.float32)


def ridge(shape):
    """two Gaussian walls, one along each axis, over a small periodic texture"""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    z = 20 * np.exp(-((xx - w * 0.3) / 2.0) ** 2) + 30 * np.exp(-((yy - h * 0.6) / 1.5) ** 2) + 0.5 * np.sin(xx * 1.3) * np.cos(yy * 0.9) + 2
    return z.astype(np.float32)


def plane(shape):
    return np.full(shape, 5.0, np.float32)


RASTERS = {"rough": rough, "ridge": ridge, "plane": plane}
_expected = {}


def expected(kind, shape, sun):
    """(raster, oracle out, mask, unshadowed shade), computed once per case and left unchanged"""
    key = (kind, shape, sun)
    if key not in _expected:
        z = RASTERS[kind](shape)
        out, mask, plain = ho.hillshade(z, sun[0], sun[1])
        for a in (z, out, mask, plain):
            a.setflags(write=False)
        _expected[key] = (z, out, mask, plain)
    return _expected[key]


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xs, z, **kw):
    return xs.DataArray(z, dims=["y", "x"], **kw)


def _check(got, want, mask, plain, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    border = np.ones(want.shape, bool)
    border[1:-1, 1:-1] = False
    assert np.isnan(got[border]).all() and not np.isnan(got[~border]).any(), what
    assert (plain[~border] > 0).all(), what                        # so that the mask can be read off every interior cell
    got_mask = np.zeros(want.shape, bool)
    got_mask[~border] = got[~border] < 0.75 * plain[~border]
    differ = got_mask != mask
    share = float(mask[~border].mean()) if (~border).any() else 0.0
    print(f"{what}: shadow share {share:.3f}, {int(differ.sum())} verdicts differ, "
          f"{int(np.sum(got[~border] != want[~border]))} values differ")
    assert not differ.any(), (what, np.argwhere(differ)[:10].tolist())
    assert np.array_equal(got[~border].view(np.uint32), want[~border].view(np.uint32)), what
    return share


def _run_case(xs, kind, shape, sun):
    z, want, mask, plain = expected(kind, shape, sun)
    before = z.copy()
    out = xs.hillshade(_agg(xs, z, attrs={"crs": 3857}), azimuth=sun[0], angle_altitude=sun[1], shadows=True)
    assert isinstance(out.data, np.ndarray) and tuple(out.dims) == ("y", "x") and out.attrs == {"crs": 3857} and out.name == "hillshade"
    assert np.array_equal(z, before)                               # the input is left alone
    return _check(out.data, want, mask, plain, f"hillshade_shadow_{kind}_{shape[0]}x{shape[1]}_az{sun[0]}_alt{sun[1]}")


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["rough", "ridge"])
def test_equals_the_brute_force_at_every_sun(xs, kind, shape):
    shares = [_run_case(xs, kind, shape, sun) for sun in SUNS]
    if shape[0] > 3:                                               # (one interior row: a share of a handful of cells)
        assert any(0.1 < s < 0.9 for s in shares), shares


@pytest.mark.parametrize("sun", SUNS, ids=lambda s: f"az{s[0]}_alt{s[1]}")
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["rough", "ridge"])
def test_equals_the_brute_force_across_blocks(xs, kind, shape, sun):
    _run_case(xs, kind, shape, sun)


@pytest.mark.parametrize("kind", ["rough", "ridge"])
@pytest.mark.parametrize("shape", LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_cases_hold_mixed_masks(kind, shape):
    """the condition on the shares for the shapes whose suns are separate cases (the oracle's results are shared with them)"""
    assert any(0.1 < expected(kind, shape, sun)[2][1:-1, 1:-1].mean() < 0.9 for sun in SUNS[:3])


def test_level_plane(xs):
    for sun in SUNS:
        share = _run_case(xs, "plane", (33, 47), sun)
        assert share == (1.0 if sun[1] < 0 else 0.0)               # below the horizon every face shadows itself
        if sun[1] >= 0:
            z, want, _, _ = expected("plane", (33, 47), sun)
            assert np.allclose(want[1:-1, 1:-1], (np.sin(np.radians(sun[1])) + 1) / 2, rtol=1e-6)


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_other_dtypes(xs, dtype):
    """a float64 copy holds the same values (one reference); int16 truncates them and goes through the float64 conversion"""
    shape, sun = (33, 47), SUNS[0]
    z32 = expected("rough", shape, sun)[0]
    z = z32.astype(dtype)
    if dtype is np.float64:
        _, want, mask, plain = expected("rough", shape, sun)
    else:
        want, mask, plain = ho.hillshade(z, *sun)
    before = z.copy()
    out = xs.hillshade(_agg(xs, z), shadows=True)
    assert z.dtype == np.dtype(dtype) and np.array_equal(z, before)
    share = _check(out.data, want, mask, plain, f"hillshade_shadow_rough_33x47_{np.dtype(dtype).name}")
    assert 0.1 < share < 0.9


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16])
def test_device_array_in_device_array_out(xs, dtype):
    shape, sun = (33, 47), SUNS[1]
    z = expected("ridge", shape, sun)[0].astype(dtype)
    host = xs.hillshade(_agg(xs, z), azimuth=sun[0], angle_altitude=sun[1], shadows=True)
    dev_in = xs.DeviceArray.from_numpy(z)
    dev = xs.hillshade(_agg(xs, dev_in, attrs={"k": 1}), azimuth=sun[0], angle_altitude=sun[1], shadows=True)
    assert isinstance(dev.data, xs.DeviceArray) and dev.data.dtype == np.float32 and dev.attrs == {"k": 1}
    assert np.array_equal(dev.data.get().view(np.uint32), host.data.view(np.uint32))
    assert dev_in.dtype == np.dtype(dtype) and np.array_equal(dev_in.get(), z)      # the input is left alone
    if dtype is not np.int16:
        _, want, mask, plain = expected("ridge", shape, sun)
        _check(host.data, want, mask, plain, f"hillshade_shadow_ridge_33x47_device_{np.dtype(dtype).name}")


def test_abi_without_shadows_is_the_plain_ray_traced_shade(xs):
    """shadows = 0 at the ABI: Lambert's shade on the mesh's normals, and the mask read off a second call"""
    from xrspatial_amd import _lib
    shape, sun = (65, 49), SUNS[0]
    z, want, mask, plain = expected("ridge", shape, sun)
    lib = _lib.load()
    src = xs.DeviceArray.from_numpy(z)
    work = xs.DeviceArray((int(lib.xrs_hillshade_shadow_workspace_bytes(*shape)),), np.uint8)
    s = ho.sun_dir(*sun)
    outs = []
    for flag in (0, 1):
        out = xs.DeviceArray(shape, np.float32)
        _lib.call("xrs_hillshade_shadow_f32", src.ptr, shape[0], shape[1], float(max(shape)) / float(z.max()), float(z.min()),
                  float(z.max()), float(s[0]), float(s[1]), float(s[2]), flag, work.ptr, out.ptr, None)
        _lib.call("xrs_device_sync")
        outs.append(out.get())
    inner = (slice(1, -1), slice(1, -1))
    assert np.array_equal(outs[0][inner].view(np.uint32), plain[inner].astype(np.float32).view(np.uint32))
    assert np.isnan(outs[0][0]).all() and np.isnan(outs[0][:, -1]).all()
    assert np.array_equal(outs[1][inner].view(np.uint32), want[inner].view(np.uint32))
    assert np.array_equal(outs[1][inner] != outs[0][inner], mask[inner])
    for block in (0, 8, 16, 32):                                   # the measuring entry point: every block size, one verdict
        out = xs.DeviceArray(shape, np.float32)
        counts = xs.DeviceArray.from_numpy(np.zeros(4, np.uint64))
        _lib.call("xrs_hillshade_shadow_probe_f32", src.ptr, shape[0], shape[1], float(max(shape)) / float(z.max()), float(z.min()),
                  float(z.max()), float(s[0]), float(s[1]), float(s[2]), block, work.ptr, out.ptr, counts.ptr, None)
        _lib.call("xrs_device_sync")
        assert np.array_equal(out.get()[inner].view(np.uint32), want[inner].view(np.uint32)), block
        c = counts.get()
        assert c[0] > 0 and c[1] <= max(shape) * 3 and (c[2] > 0) == (block != 0), (block, c.tolist())


def test_shadows_false_is_the_existing_path(xs):
    mod = importlib.import_module("xrspatial_amd.hillshade")
    z = expected("rough", (33, 47), SUNS[0])[0]
    a = xs.hillshade(_agg(xs, z), azimuth=100, angle_altitude=40, shadows=False)
    b = xs.hillshade(_agg(xs, z), azimuth=100, angle_altitude=40)
    direct = mod._run_numpy(z, 100, 40)
    assert a.data.dtype == direct.dtype and np.array_equal(a.data, direct, equal_nan=True) and np.array_equal(b.data, direct, equal_nan=True)


def test_small_rasters_are_all_nan(xs):
    for shape in ((2, 5), (5, 2), (1, 1), (2, 2)):
        out = xs.hillshade(_agg(xs, np.full(shape, 3.0, np.float32)), shadows=True)
        assert out.data.dtype == np.float32 and out.data.shape == shape and np.isnan(out.data).all()


def test_refusals_on_the_device(xs):
    z = rough((8, 9))
    bad = z.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        xs.hillshade(_agg(xs, bad), shadows=True)
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        xs.hillshade(_agg(xs, xs.DeviceArray.from_numpy(bad)), shadows=True)
    with pytest.raises(ValueError, match="positive"):
        xs.hillshade(_agg(xs, -z), shadows=True)
    with pytest.raises(ValueError, match="positive"):
        xs.hillshade(_agg(xs, np.zeros((8, 9), np.int32)), shadows=True)

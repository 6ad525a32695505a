"""CPU checks of hillshade(shadows=True): every piece of the rule (tests/hillshade_shadow_oracle.py) that the reference computes
outside its OptiX trace, against the reference's own functions executed on the CPU (tests/golden/hillshade_shadow_exec.npz);
analytic cases for the brute force; and the argument checks and refusals, which run before any device work."""
import ctypes
import importlib

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import hillshade_shadow_oracle as ho
from tests.golden import make_hillshade_shadow_exec as gen

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)


def _agg(a, **kw):
    import xrspatial_amd as xs
    return xs.DataArray(a, dims=["y", "x"], **kw)


# ------------------------------------------------------------------ the rule against the executed reference
def test_sun_vector_equals_get_sun_dir():
    """atol 1e-15: the reference turns (0, 1, 0) by two scipy rotations, the rule writes the product out (2e-16 seen)"""
    from xrspatial_amd.hillshade import sun_vector
    assert len(FIXTURE["sun/args"]) == 5
    for (alt, az), want in zip(FIXTURE["sun/args"], FIXTURE["sun/out"]):
        got = ho.sun_dir(az, alt)
        print(f"alt {alt} az {az}: largest difference {np.abs(got - want).max():.3g}")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
        np.testing.assert_allclose(np.array(sun_vector(az, alt)), want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("case", CASES)
def test_mesh_equals_triangulate_cpu(case):
    scale, zv, verts, triangles = ho.mesh(FIXTURE[f"{case}/data"])
    assert scale == float(FIXTURE[f"{case}/scale"])
    want_v, want_t = FIXTURE[f"{case}/verts"], FIXTURE[f"{case}/triangles"]
    assert verts.dtype == want_v.dtype == np.float32 and np.array_equal(verts.view(np.uint32), want_v.view(np.uint32))
    assert triangles.dtype == want_t.dtype == np.int32 and np.array_equal(triangles, want_t)
    # the vertex triples the brute force tests are those of the index buffer, in its order
    v0, v1, v2 = ho.triangle_vertices(zv)
    H, W = zv.shape
    xyz = want_v.reshape(-1, 3).astype(np.float64)
    tri = want_t.reshape(-1, 2, 3)                                   # per cell: T0, T1
    n = (H - 1) * (W - 1)
    for k, v in enumerate((v0, v1, v2)):
        for which in (0, 1):
            got = np.stack([v[0][which * n:(which + 1) * n], v[1][which * n:(which + 1) * n], v[2][which * n:(which + 1) * n]], axis=-1)
            assert np.array_equal(got, xyz[tri[:, which, k]])


@pytest.mark.parametrize("case", CASES)
def test_ray_origins_equal_the_primary_ray_kernel(case):
    want = FIXTURE[f"{case}/primary"]
    H, W = want.shape[:2]
    got = ho.primary_origins(H, W)
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want[..., :2].view(np.uint32))
    assert (want[..., 2] == 10000).all() and (want[..., 3] == np.float32(1e-3)).all() and (want[..., 4:7] == [0, 0, -1]).all()


@pytest.mark.parametrize("case", CASES)
def test_shadow_ray_equals_the_shadow_ray_kernel(case):
    """origin, flipped normal and tmin to float32 rounding: rtol 1e-6 (2^-24 per stored float32, fewer than ten per result)"""
    rays, normals, sun = FIXTURE[f"{case}/shadow_rays"], FIXTURE[f"{case}/normals"], FIXTURE[f"{case}/sun"]
    _, zv, _, _ = ho.mesh(FIXTURE[f"{case}/data"])
    hit = ho.camera_hits(zv)
    H, W = zv.shape
    inner = (slice(1, H - 1), slice(1, W - 1))
    n = hit["n"][inner]
    assert (FIXTURE[f"{case}/hits"][inner][..., 3] < 0).all()        # the triangle's own normal points down: the kernel flips it
    np.testing.assert_allclose(normals[inner], n, rtol=1e-6, atol=0)
    assert (normals[inner][..., 2] > 0).all()
    origin = np.stack([hit["x0"][inner] + n[..., 0] * ho.EPS, hit["y0"][inner] + n[..., 1] * ho.EPS, hit["zh"][inner] + n[..., 2] * ho.EPS], axis=-1)
    np.testing.assert_allclose(rays[inner][..., :3], origin, rtol=1e-6, atol=0)
    assert (rays[inner][..., 3] == np.float32(ho.TMIN)).all() and np.isinf(rays[inner][..., 7]).all()
    assert np.array_equal(rays[inner][..., 4:7], np.broadcast_to(sun.astype(np.float32), n.shape))


@pytest.mark.parametrize("case", CASES)
def test_shade_equals_the_lambert_kernel(case):
    sun, nrm, hits = FIXTURE[f"{case}/sun"], FIXTURE[f"{case}/shade_normals"].astype(np.float64), FIXTURE[f"{case}/shade_hits"][..., 0]
    plain, cast = FIXTURE[f"{case}/shade_plain"], FIXTURE[f"{case}/shade_cast"]
    hit = hits >= 0
    assert hit.any() and not hit.all() and hit[0, 0] and hits[0, 0] == 0
    np.testing.assert_allclose(ho.shade_values(sun, nrm, False), plain, rtol=1e-6, atol=0)
    np.testing.assert_allclose(ho.shade_values(sun, nrm, hit), cast, rtol=1e-6, atol=0)
    # clamping and halving are exact
    assert plain[0, 1] == 0.0 and cast[0, 1] == 0.0 and plain[1, 1] == 1.0 and cast[1, 1] == 1.0
    assert ho.shade_values(sun, nrm, False)[0, 1] == 0.0 and ho.shade_values(sun, nrm, hit)[1, 1] == 1.0
    free = np.ones(hit.shape, bool)
    free[0, 1] = free[1, 1] = False
    assert np.array_equal(cast[hit & free], plain[hit & free] / np.float32(2)) and np.array_equal(cast[~hit], plain[~hit])
    assert ((cast >= 0) & (cast <= 1)).all()


# ------------------------------------------------------------------ analytic cases for the brute force
def test_level_plane_has_no_shadow():
    for az, alt in ((225, 25), (90, 5), (0, 60), (45, 90)):
        out, mask, plain = ho.hillshade(np.full((7, 9), 3.5), az, alt)
        assert not mask.any()
        np.testing.assert_allclose(out[1:-1, 1:-1], (np.sin(np.radians(alt)) + 1) / 2, rtol=1e-6)
        assert np.isnan(out[0]).all() and np.isnan(out[-1]).all() and np.isnan(out[:, 0]).all() and np.isnan(out[:, -1]).all()


def test_wall_across_a_plane_casts_height_over_tan_altitude():
    """a wall one vertex wide at column 25 of a 9 x 41 plane, 0.1 of the maximum above it: 4.1 mesh units after the scale
    max(H, W) / max; the sun due east (azimuth 90: the sun vector points along +x) at 45 degrees: the four cells west of the
    wall are in shadow (the nearest one through its own face, which is turned away), the fifth is lit, as is everything else"""
    z = np.full((9, 41), 9.0)
    z[:, 25] = 10.0
    out, mask, plain = ho.hillshade(z, 90, 45)
    want = np.zeros(z.shape, bool)
    want[1:-1, 21:25] = True
    assert np.array_equal(mask, want)
    flat = np.float32((np.sin(np.radians(45)) + 1) / 2)
    np.testing.assert_allclose(out[1:-1, 20], flat, rtol=1e-6)
    np.testing.assert_allclose(out[1:-1, 21:24], flat / 2, rtol=1e-6)
    # lower sun, longer shadow: 4.1 / tan(20 degrees) = 11.26 cells
    _, mask, _ = ho.hillshade(z, 90, 20)
    want[:] = False
    want[1:-1, 25 - 11:25] = True
    assert np.array_equal(mask, want)
    # the sun on the other side: the shadow falls east of the wall
    _, mask, _ = ho.hillshade(z, 270, 45)
    assert mask[1:-1, 25:29].all() and not mask[1:-1, :25].any() and not mask[1:-1, 30:].any()


def test_small_rasters_are_all_nan_in_the_oracle():
    for shape in ((2, 5), (5, 2), (1, 1)):
        out, mask, _ = ho.hillshade(np.ones(shape), 225, 25)
        assert out.dtype == np.float32 and np.isnan(out).all() and not mask.any()


# ------------------------------------------------------------------ the host side of the public function
def test_argument_errors_come_before_device_work():
    import xrspatial_amd as xs
    good = np.random.default_rng(0).random((6, 7)).astype(np.float32) + 1
    with pytest.raises(ValueError, match="2-D"):
        xs.hillshade(xs.DataArray(np.ones((2, 3, 4), np.float32), dims=["b", "y", "x"]), shadows=True)
    with pytest.raises(ValueError, match="2-D"):
        xs.hillshade(xs.DataArray(np.ones(5, np.float32), dims=["x"]), shadows=True)
    with pytest.raises(ValueError, match="empty"):
        xs.hillshade(_agg(np.ones((0, 4), np.float32)), shadows=True)
    for value in (np.nan, np.inf, -np.inf):
        bad = good.astype(np.float64)
        bad[2, 3] = value
        with pytest.raises(ValueError, match="1 non-finite"):
            xs.hillshade(_agg(bad), shadows=True)
    with pytest.raises(ValueError, match="positive"):
        xs.hillshade(_agg(-good), shadows=True)
    with pytest.raises(ValueError, match="positive"):
        xs.hillshade(_agg(np.zeros((6, 7), np.int16)), shadows=True)
    with pytest.raises(ValueError, match="finite"):
        xs.hillshade(_agg(good), azimuth=float("nan"), shadows=True)


def test_fuse_scope_refuses_shadows():
    import xrspatial_amd as xs
    agg = _agg(np.ones((6, 7), np.float32))
    with pytest.raises(NotImplementedError, match="fuse"):
        with xs.fuse():
            xs.hillshade(agg, shadows=True)


def test_dask_backed_raster_is_refused(monkeypatch):
    import xrspatial_amd as xs
    from xrspatial_amd import utils
    mod = importlib.import_module("xrspatial_amd.hillshade")
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.ones((8, 8), np.float32), (4, 4)))
    assert mod.is_dask(lazy.data)
    with pytest.raises(NotImplementedError, match="dask"):
        xs.hillshade(lazy, shadows=True)


def test_dataset_input_keeps_working(monkeypatch):
    import xrspatial_amd as xs
    mod = importlib.import_module("xrspatial_amd.hillshade")
    seen = []
    monkeypatch.setattr(mod, "_run_shadows", lambda data, az, alt: seen.append((az, alt)) or np.zeros(data.shape, np.float32))
    ds = xs.Dataset({"a": _agg(np.ones((4, 5), np.float32)), "b": _agg(np.ones((4, 5), np.float64))})
    out = xs.hillshade(ds, azimuth=90, angle_altitude=5, shadows=True)
    assert sorted(out.data_vars) == ["a", "b"] and seen == [(90, 5), (90, 5)] and out["a"].data.dtype == np.float32


def test_no_gpu_raises_xrs_error_not_the_rtxpy_error():
    """without a device the call fails like every other compute function here, no longer with the reference's
    "Can only calculate shadows if cupy and rtxpy are available" """
    entry.build()
    import xrspatial_amd as xs
    agg = _agg(np.random.default_rng(1).random((5, 6)).astype(np.float32) + 1)
    if xs.has_hip():
        assert xs.hillshade(agg, shadows=True).data.dtype == np.float32
        return
    for dt in (np.float32, np.float64, np.int32):
        with pytest.raises(xs.XrsError):
            xs.hillshade(_agg(agg.data.astype(dt)), shadows=True)


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_hillshade_shadow_* validate on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    up = lambda v: (v + 255) // 256 * 256                            # noqa: E731
    assert lib.xrs_hillshade_shadow_workspace_bytes(300, 400) == up(300 * 400 * 4) + up((38 * 50 + 1) * 4)
    assert lib.xrs_hillshade_shadow_workspace_bytes(0, 5) == 0

    def call(fn=lib.xrs_hillshade_shadow_f32, data=fake, rows=4, cols=5, scale=1.0, zmin=0.0, zmax=5.0, sun=(0.6, 0.0, 0.8), flag=1,
             work=fake, out=fake):
        return fn(data, rows, cols, scale, zmin, zmax, sun[0], sun[1], sun[2], flag, work, out, None)

    for kw, text in ((dict(rows=0), "1 x 1"), (dict(cols=-2), "1 x 1"), (dict(rows=1 << 30), "too large"), (dict(data=None), "null"),
                     (dict(work=None), "null"), (dict(out=None), "null"), (dict(scale=0.0), "scale"), (dict(scale=float("nan")), "scale"),
                     (dict(scale=-1.0), "scale"), (dict(zmin=float("nan")), "bounds"), (dict(zmin=6.0), "bounds"),
                     (dict(sun=(0.0, 0.0, 0.0)), "sun"), (dict(sun=(float("inf"), 0.0, 0.0)), "sun"),
                     (dict(fn=lib.xrs_hillshade_shadow_f64, zmax=float("inf")), "bounds")):
        assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    probe = lib.xrs_hillshade_shadow_probe_f32
    assert probe(fake, 4, 5, 1.0, 0.0, 5.0, 0.6, 0.0, 0.8, 12, fake, fake, None, None) != 0 and "block" in _lib.last_error()

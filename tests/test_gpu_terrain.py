"""perlin / generate_terrain on the MI355X against the reference's own outputs (tests/golden/terrain_exec.npz) and, at the
shapes the fixture lacks, against the restatement (tests/terrain_oracle.py).

Tolerance: the reference's own cross-backend one, assert_allclose(rtol=1e-5, atol=1e-7) (xrspatial/tests/test_terrain.py:62,
test_perlin.py:64).  The raw plane is also compared bit for bit with the restatement and the number of cells that differ
is recorded (tests/parity_log.py), not asserted: the kernel's multiply chains and NumPy's `pow` may round a few cells apart.

Water line: a terrain cell whose reference value before `data[data < 0.3] = 0` lies within 2e-5 of 0.3 (the relative
tolerance at 0.3, doubled) may land on either side of the line; it passes if it is 0 or normalised * zfactor within the
tolerance.  At most 0.5 % of a case's cells may need that; the executed reference has 0.10 - 0.11 % of its cells within the
five-times-wider band at 37x53 and 96x130 (tests/test_terrain_host.py asserts it for the fixture)."""
import importlib

import numpy as np
import pytest

from tests import parity_log
from tests import terrain_oracle as to
from tests.golden import make_terrain_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = dict(gen.cases())
PERLIN = [n for n, c in CASES.items() if c["kind"] == "perlin"]
TERRAIN = [n for n, c in CASES.items() if c["kind"] == "terrain"]
RTOL, ATOL = 1e-5, 1e-7
WATER_BAND, WATER_SHARE = 2e-5, 0.005


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


@pytest.fixture(scope="module")
def noise_mod(xs):
    return importlib.import_module("xrspatial_amd.perlin")


def _agg(xs, a, **kw):
    return xs.DataArray(a, dims=["y", "x"], **kw)


def _zeros(xs, shape, dtype):
    return _agg(xs, np.zeros(shape, dtype))


def _close(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=what)


def _close_terrain(got, want_out, want_norm, zfactor, what):
    """assert_allclose(rtol=1e-5, atol=1e-7) except for the cells at the water line (module docstring)"""
    assert got.dtype == want_out.dtype and got.shape == want_out.shape, what
    near = np.abs(want_norm.astype(np.float64) - 0.3) <= WATER_BAND
    assert near.mean() <= WATER_SHARE, (what, float(near.mean()))
    np.testing.assert_allclose(got[~near], want_out[~near], rtol=RTOL, atol=ATOL, equal_nan=True, err_msg=what)
    land = want_norm[near] * want_out.dtype.type(zfactor)
    g = got[near]
    ok = (np.abs(g) <= ATOL) | (np.abs(g - land) <= ATOL + RTOL * np.abs(land))
    assert ok.all(), (what, g[~ok], land[~ok])
    parity_log.record(what, "generate_terrain", np.where(near, want_out, got), want_out, tol=RTOL,
                      note=f"{int(near.sum())} cells within {WATER_BAND} of the water line")


def _terrain(xs, c, data=None):
    agg = _zeros(xs, c["shape"], c["dtype"]) if data is None else data
    return xs.generate_terrain(agg, x_range=c["x_range"], y_range=c["y_range"], seed=c["seed"], zfactor=c["zfactor"],
                               full_extent=c["full_extent"])


# ------------------------------------------------------------------ against the executed reference
@pytest.mark.parametrize("case", PERLIN)
def test_perlin_equals_the_reference(xs, case):
    c = CASES[case]
    out = xs.perlin(_zeros(xs, c["shape"], c["dtype"]), freq=c["freq"], seed=c["seed"])
    assert out.name == "perlin" and tuple(out.dims) == ("y", "x") and isinstance(out.data, np.ndarray)
    _close(out.data, FIXTURE[f"{case}/out"], case)
    parity_log.record(case, "perlin", out.data, FIXTURE[f"{case}/out"], tol=RTOL)


@pytest.mark.parametrize("case", TERRAIN)
def test_terrain_equals_the_reference(xs, case):
    c = CASES[case]
    out = _terrain(xs, c)
    assert out.name == "terrain" and tuple(out.dims) == ("y", "x") and isinstance(out.data, np.ndarray)
    _close_terrain(out.data, FIXTURE[f"{case}/out"], FIXTURE[f"{case}/norm"], c["zfactor"], case)
    h, w = c["shape"]
    assert np.array_equal(np.asarray(out["x"].data), to.cell_centres(c["x_range"][0], c["x_range"][1], w))
    assert np.array_equal(np.asarray(out["y"].data), to.cell_centres(c["y_range"][0], c["y_range"][1], h))


# ------------------------------------------------------------------ against the restatement, shapes the fixture lacks
DOC = dict(x_range=(-20e6, 20e6), y_range=(-20e6, 20e6), seed=2, zfactor=10)      # the generate_terrain docstring example
ORACLE_TERRAIN = [((1, 7), np.float32, {}), ((7, 1), np.float64, {}), ((130, 257), np.float32, {}), ((130, 257), np.float64, {}),
                  ((300, 400), np.float32, DOC), ((65, 300), np.float32, dict(DOC, seed=40, zfactor=2.5))]


@pytest.mark.parametrize("shape,dtype,kw", ORACLE_TERRAIN)
def test_terrain_equals_the_restatement(xs, shape, dtype, kw):
    what = f"terrain_{shape[0]}x{shape[1]}_{np.dtype(dtype).name}_seed{kw.get('seed', 10)}"
    _, norm, want = to.terrain_planes(shape, dtype, **kw)
    out = xs.generate_terrain(_zeros(xs, shape, dtype), **kw)
    _close_terrain(out.data, want, norm, kw.get("zfactor", 4000), what)
    if min(shape) > 1:
        assert out.attrs["res"] == xs.utils.get_dataarray_resolution(out)


@pytest.mark.parametrize("shape,dtype,freq,seed", [((1, 7), np.float32, (1, 1), 5), ((7, 1), np.float64, (3, 2), 5),
                                                   ((130, 257), np.float32, (8, 8), 11), ((130, 257), np.float64, (3, 7.3), 5),
                                                   ((300, 400), np.float32, (1000.5, 77), 6)])
def test_perlin_equals_the_restatement(xs, shape, dtype, freq, seed):
    want = to.perlin(shape, dtype, freq, seed)
    out = xs.perlin(_zeros(xs, shape, dtype), freq=freq, seed=seed)
    _close(out.data, want, f"perlin {shape} {freq}")
    parity_log.record(f"perlin_{shape[0]}x{shape[1]}_{np.dtype(dtype).name}", "perlin", out.data, want, tol=RTOL)


# ------------------------------------------------------------------ at the ABI: the raw plane, its min / max, banding
def _raw(xs, noise_mod, shape, dtype, seeds, xr, yr, mode, row0=0, rows=None):
    rows = shape[0] - row0 if rows is None else rows
    out = xs.DeviceArray((rows, shape[1]), dtype)
    mn, mx = noise_mod.raw_plane(out, seeds, xr, yr, mode, row0=row0, total_rows=shape[0])
    return out.get(), mn, mx


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_raw_plane_min_max_and_bit_differences(xs, noise_mod, dtype):
    shape, seed = (96, 130), 10
    seeds = [seed + i for i in range(16)]
    got, mn, mx = _raw(xs, noise_mod, shape, dtype, seeds, (0.0, 1.0), (0.0, 1.0), noise_mod.MODE_TERRAIN)
    assert got.dtype == np.dtype(dtype) and (mn, mx) == (float(got.min()), float(got.max()))
    want = to.terrain_raw(shape, dtype, seed, (0.0, 1.0), (0.0, 1.0))
    assert np.array_equal(want, FIXTURE[f"terrain_96x130_{'f32' if dtype == np.float32 else 'f64'}/raw"])
    differ = int(np.count_nonzero(got != want))
    _, worst = parity_log.record(f"terrain_raw_96x130_{np.dtype(dtype).name}", "xrs_noise_raw", got, want,
                                 note=f"{differ} of {got.size} cells not bit-equal to the restatement")
    print(f"raw plane {np.dtype(dtype).name}: {differ} of {got.size} cells differ, worst abs {worst:.3g}")
    # the raw plane spans ~0.028: 1e-5 relative on the normalised plane is 2.8e-7 absolute here; a rounding step is far below
    np.testing.assert_allclose(got, want, rtol=0, atol=np.ptp(want) * RTOL * 0.3)
    # one octave, stored without the divide and the cube
    got, mn, mx = _raw(xs, noise_mod, (37, 53), dtype, [7], (0, 3), (0, 7.3), noise_mod.MODE_PERLIN)
    want = to.perlin_raw((37, 53), dtype, (3, 7.3), 7)
    assert (mn, mx) == (float(got.min()), float(got.max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-7)
    print(f"perlin raw {np.dtype(dtype).name}: {int(np.count_nonzero(got != want))} of {got.size} cells differ")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bands_are_bit_identical_to_the_whole_plane(xs, noise_mod, dtype):
    shape = (96, 130)
    seeds = [10 + i for i in range(16)]
    args = (seeds, (0.0, 1.0), (0.0, 1.0), noise_mod.MODE_TERRAIN)
    whole, mn, mx = _raw(xs, noise_mod, shape, dtype, *args)
    top, mn0, mx0 = _raw(xs, noise_mod, shape, dtype, *args, row0=0, rows=40)
    bot, mn1, mx1 = _raw(xs, noise_mod, shape, dtype, *args, row0=40, rows=56)
    iv = np.dtype("u%d" % np.dtype(dtype).itemsize)
    assert np.array_equal(np.concatenate([top, bot]).view(iv), whole.view(iv))
    assert (min(mn0, mn1), max(mx0, mx1)) == (mn, mx)
    assert (mn1, mx1) == (float(bot.min()), float(bot.max()))
    # tiles: more than one block in both directions, and a band that starts inside a tile of the whole plane
    shape = (150, 600)
    whole, _, _ = _raw(xs, noise_mod, shape, dtype, [5], (0, 9), (0, 4), noise_mod.MODE_PERLIN)
    band, _, _ = _raw(xs, noise_mod, shape, dtype, [5], (0, 9), (0, 4), noise_mod.MODE_PERLIN, row0=70, rows=80)
    assert np.array_equal(band.view(iv), whole[70:].view(iv))
    want = to.perlin_raw(shape, dtype, (9, 4), 5)
    np.testing.assert_allclose(whole, want, rtol=0, atol=1e-7)


# ------------------------------------------------------------------ backends, cache, refusals
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_array_in_device_array_out(xs, dtype):
    shape = (37, 53)
    dev = _agg(xs, xs.DeviceArray(shape, dtype), attrs={"crs": "EPSG:3857"})
    host = _zeros(xs, shape, dtype)
    t_dev = xs.generate_terrain(dev, seed=10, name="dem")
    assert isinstance(t_dev.data, xs.DeviceArray) and t_dev.data.dtype == np.dtype(dtype) and t_dev.name == "dem"
    t_host = xs.generate_terrain(host, seed=10)
    assert np.array_equal(t_dev.data.get(), t_host.data)
    assert t_dev.attrs == t_host.attrs and set(t_dev.attrs) == {"res"}
    p_dev = xs.perlin(dev, freq=(3, 7.3), seed=7, name="n")
    assert isinstance(p_dev.data, xs.DeviceArray) and p_dev.name == "n" and p_dev.attrs == {"crs": "EPSG:3857"}
    assert np.array_equal(p_dev.data.get(), xs.perlin(host, freq=(3, 7.3), seed=7).data)


def test_tables_are_cached_per_seed(xs, noise_mod, monkeypatch):
    agg = _zeros(xs, (8, 9), np.float32)
    xs.empty_cache()
    before = noise_mod.table_cache_info()
    assert before["size"] == 0
    first = xs.generate_terrain(agg, seed=100).data
    mid = noise_mod.table_cache_info()
    assert mid["uploads"] - before["uploads"] == 16 and mid["size"] == 16
    again = xs.generate_terrain(agg, seed=100).data
    after = noise_mod.table_cache_info()
    assert after["uploads"] == mid["uploads"] and after["hits"] - mid["hits"] == 16      # no table upload
    assert np.array_equal(first, again)
    noise_one = xs.perlin(agg, seed=100).data               # octave 0 of the terrain: cached too
    assert noise_mod.table_cache_info()["uploads"] == after["uploads"]
    monkeypatch.setattr(noise_mod, "_TABLE_CACHE_MAX", 20)  # the LRU is bounded: the oldest tables go
    xs.generate_terrain(agg, seed=108)                      # octaves 0 .. 7 of seed 108 are octaves 8 .. 15 of seed 100
    info = noise_mod.table_cache_info()
    assert info["uploads"] - after["uploads"] == 8 and info["size"] == 20
    xs.generate_terrain(agg, seed=108)
    assert noise_mod.table_cache_info()["uploads"] == info["uploads"]
    xs.empty_cache()
    assert noise_mod.table_cache_info()["size"] == 0
    assert np.array_equal(xs.perlin(agg, seed=100).data, noise_one)
    assert noise_mod.table_cache_info()["uploads"] - info["uploads"] == 1


def test_global_random_state_is_left_alone(xs):
    np.random.seed(1234)
    want = np.random.random(3)
    np.random.seed(1234)
    xs.perlin(_zeros(xs, (4, 4), np.float32), seed=77)
    assert np.array_equal(np.random.random(3), want)


def test_sharded_raster_is_refused(xs):
    sh = xs.ShardedArray(8, 8, np.float32)
    for fn in (xs.perlin, xs.generate_terrain):
        with pytest.raises(NotImplementedError, match="sharded"):
            fn(xs.DataArray(sh, dims=["y", "x"]))

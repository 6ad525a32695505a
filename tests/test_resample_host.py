"""resample without a GPU: the package's table builders against the oracle's, bit for bit; argument validation; the oracle
(tests/resample_oracle.py, the rule of DESIGN.md §6u) against independent libraries, so that the rule itself is pinned; and the
properties the rule promises."""
import types

import numpy as np
import pytest

import xrspatial_amd as xs
from tests import resample_oracle as ro

R = xs.resample
METHODS = ("nearest", "bilinear", "cubic", "lanczos", "average", "sum", "min", "max", "mode")
DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64)
IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _tables_equal(method, src_shape, dst_shape, S, D):
    got, want = R.tables(method, src_shape, dst_shape, S, D), ro.tables(method, src_shape, dst_shape, S, D)
    assert got.keys() == want.keys()
    for key in got:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (method, key)
        assert np.array_equal(_bits(got[key]), _bits(want[key])), (method, key, src_shape, dst_shape, S, D)
    return got


def _raster(shape, seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.normal(100.0, 30.0, shape).astype(dtype)
    return rng.integers(0, 100, shape).astype(dtype)


# ------------------------------------------------------------------ the package's tables are the oracle's
GRIDS = {
    "up": ((17, 33), (40, 70), None, None),
    "down": ((70, 130), (17, 33), None, None),
    "identity": ((17, 33), (17, 33), None, None),
    "identity_transforms": ((17, 33), (17, 33), (30.0, 0.0, 120.0, 0.0, -30.0, 900.0), (30.0, 0.0, 120.0, 0.0, -30.0, 900.0)),
    "world": ((17, 33), (20, 30), (30.0, 0.0, 100.0, 0.0, -30.0, 900.0), (13.0, 0.0, 90.0, 0.0, -11.0, 905.0)),
    "irrational": ((17, 33), (20, 30), (0.3, 0.0, 0.1, 0.0, -0.7, 11.3), (0.11, 0.0, 0.7, 0.0, -0.13, 9.1)),
    "flipped_x": ((17, 33), (20, 30), (30.0, 0.0, 100.0, 0.0, -30.0, 900.0), (-13.0, 0.0, 800.0, 0.0, -11.0, 905.0)),
    "flipped_y": ((17, 33), (20, 30), (30.0, 0.0, 100.0, 0.0, -30.0, 900.0), (13.0, 0.0, 90.0, 0.0, 11.0, 500.0)),
    "flipped_source": ((17, 33), (20, 30), (-30.0, 0.0, 1000.0, 0.0, 30.0, 100.0), (13.0, 0.0, 90.0, 0.0, -11.0, 905.0)),
    "partly_outside": ((17, 33), (20, 30), IDENT, (0.7, 0.0, -6.3, 0.0, 0.8, 9.9)),
    "around": ((17, 33), (20, 30), IDENT, (2.1, 0.0, -8.0, 0.0, 2.3, -7.0)),
    "wholly_outside": ((17, 33), (20, 30), IDENT, (0.7, 0.0, 100.0, 0.0, 0.8, -300.0)),
    "far_outside": ((17, 33), (5, 6), IDENT, (1.0, 0.0, -1e15, 0.0, 1.0, 1e15)),
    "one_source_cell": ((1, 1), (5, 7), None, None),
    "one_destination_cell": ((17, 33), (1, 1), None, None),
    "one_cell_axes": ((1, 200), (9, 1), None, None),
}


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("method", METHODS)
def test_package_tables_are_the_oracles(method, grid):
    src_shape, dst_shape, S, D = GRIDS[grid]
    if D is None:
        D = R.shape_transform(src_shape, dst_shape)
        assert D == ro.shape_transform(src_shape, dst_shape)
    t = _tables_equal(method, src_shape, dst_shape, S, D)
    if grid in ("wholly_outside", "far_outside") and method in ("nearest", "bilinear"):
        assert (t["near_y"] == -1).all() or (t["near_x"] == -1).all()
    if grid == "identity" and method != "nearest":
        taps = t["w_x"].shape[1]
        centre = {2: 0, 4: 1, 6: 2, 1: 0}[taps]
        assert np.array_equal(t["first_x"] + centre, np.arange(33))
        assert np.array_equal(t["w_x"], np.eye(taps)[[centre] * 33])          # exactly one tap, of weight 1


def test_tap_limits_and_their_messages():
    for n_src, ok in ((256, True), (257, False)):
        args = ("average", (n_src, 3), (1, 3), None, R.shape_transform((n_src, 3), (1, 3)))
        if ok:
            assert _tables_equal(*args)["w_y"].shape == (1, 256)
        else:
            with pytest.raises(ValueError, match="257 source cells along an axis, more than the 256 taps of one call; resample in two steps"):
                R.tables(*args)
            with pytest.raises(ValueError, match="two steps"):
                ro.tables(*args)
    for src_shape, ok in (((64, 64), True), ((64, 66), False)):
        args = ("mode", src_shape, (2, 2), None, R.shape_transform(src_shape, (2, 2)))
        if ok:
            t = _tables_equal(*args)
            assert t["w_y"].shape[1] * t["w_x"].shape[1] == 1024
        else:
            with pytest.raises(ValueError, match="mode window of 32 x 33 source cells, more than 1024; resample in two steps"):
                R.tables(*args)
            with pytest.raises(ValueError, match="two steps"):
                ro.tables(*args)
            _tables_equal("max", *args[1:])                       # the same window is fine for the others


# ------------------------------------------------------------------ argument validation (all before any device call)
def _agg(shape=(8, 8), dtype=np.float32):
    return xs.DataArray(np.zeros(shape, dtype), dims=["y", "x"])


def test_like_and_shape():
    with pytest.raises(ValueError, match="exactly one of `like` and `shape`"):
        xs.resample(_agg())
    with pytest.raises(ValueError, match="exactly one of `like` and `shape`"):
        xs.resample(_agg(), _agg((4, 4)), shape=(4, 4))
    with pytest.raises(ValueError, match="takes no transforms"):
        xs.resample(_agg(), shape=(4, 4), src_transform=IDENT)
    with pytest.raises(ValueError, match="at least \\(1, 1\\)"):
        xs.resample(_agg(), shape=(0, 4))
    with pytest.raises(ValueError, match="`agg` must be 2D"):
        xs.resample(xs.DataArray(np.zeros((2, 3, 4), np.float32)), shape=(4, 4))
    with pytest.raises(ValueError, match="no coords"):
        xs.resample(_agg(), _agg((4, 4)))                         # neither transforms nor coords


def test_rotation_shear_and_singular_transforms():
    for bad in ((1.0, 0.1, 0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 0.0, -0.2, 1.0, 0.0)):
        with pytest.raises(ValueError, match="rotation or shear"):
            xs.resample(_agg(), _agg((4, 4)), src_transform=IDENT, dst_transform=bad)
        with pytest.raises(ValueError, match="rotation or shear"):
            xs.resample(_agg(), _agg((4, 4)), src_transform=bad, dst_transform=IDENT)
    with pytest.raises(ValueError, match="singular or not finite"):
        xs.resample(_agg(), _agg((4, 4)), src_transform=(0.0, 0.0, 0.0, 0.0, 1.0, 0.0), dst_transform=IDENT)
    with pytest.raises(ValueError, match="transform length"):
        xs.resample(_agg(), _agg((4, 4)), src_transform=(1.0, 0.0), dst_transform=IDENT)


def test_unknown_method_dtype_and_fill():
    with pytest.raises(ValueError, match="method must be one of .*not 'gauss'"):
        xs.resample(_agg(), shape=(4, 4), method="gauss")
    with pytest.raises(ValueError, match="method must be one of"):
        R.tables("gauss", (8, 8), (4, 4))
    with pytest.raises(ValueError, match="fill 0.5 is not exactly representable in int16"):
        xs.resample(_agg(dtype=np.int16), shape=(4, 4), method="nearest", fill=0.5)
    with pytest.raises(ValueError, match="fill 300 is not exactly representable in uint8"):
        xs.resample(_agg(dtype=np.uint8), shape=(4, 4), method="mode", fill=300)
    with pytest.raises(ValueError, match="not exactly representable in float32"):
        xs.resample(_agg(), shape=(4, 4), method="bilinear", fill=0.1)
    with pytest.raises(TypeError, match="returns the input's dtype"):
        xs.resample(_agg(), shape=(4, 4), method="max", dtype=np.float64)
    with pytest.raises(TypeError, match="float64 or float32"):
        xs.resample(_agg(), shape=(4, 4), method="average", dtype=np.int32)
    with pytest.raises(TypeError, match="unsupported dtype"):
        xs.resample(_agg(dtype=np.complex64), shape=(4, 4))


def test_sharded_and_dask_rasters_are_refused(monkeypatch):
    from xrspatial_amd import _launch
    sharded = object.__new__(xs.ShardedArray)                     # (its constructor needs a device)
    sharded.local = types.SimpleNamespace(shape=(8, 8), dtype=np.dtype(np.float32), size=64, ptr=0)
    with pytest.raises(NotImplementedError, match="resample\\(\\) does not support row-sharded"):
        xs.resample(xs.DataArray(sharded, dims=["y", "x"]), shape=(4, 4))
    with pytest.raises(NotImplementedError, match="resample\\(\\) does not support row-sharded"):
        xs.resample(_agg(), xs.DataArray(sharded, dims=["y", "x"]), src_transform=IDENT, dst_transform=IDENT)

    class Chunked:
        shape, dtype, ndim = (8, 8), np.dtype(np.float32), 2

    monkeypatch.setattr(_launch, "is_dask", lambda data: isinstance(data, Chunked))
    with pytest.raises(NotImplementedError, match="resample\\(\\) does not support dask backed DataArray"):
        xs.resample(xs.DataArray(Chunked(), dims=["y", "x"]), shape=(4, 4))


# ------------------------------------------------------------------ the oracle against independent libraries
@pytest.mark.parametrize("src_shape,dst_shape", [((40, 50), (93, 117)), ((40, 50), (17, 23)), ((13, 17), (29, 40)), ((9, 1), (4, 5))])
def test_bilinear_against_scipy_map_coordinates(src_shape, dst_shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    src = _raster(src_shape, 41, np.float64)
    T = ro.shape_transform(src_shape, dst_shape)
    uy = ro.s_of(np.arange(dst_shape[0]) + 0.5, (T[4], T[5]), (1.0, 0.0)) - 0.5
    ux = ro.s_of(np.arange(dst_shape[1]) + 0.5, (T[0], T[2]), (1.0, 0.0)) - 0.5
    yy, xx = np.meshgrid(uy, ux, indexing="ij")
    want = ndimage.map_coordinates(src, [yy, xx], order=1, mode="nearest")
    np.testing.assert_allclose(ro.resample(src, dst_shape, "bilinear", by_shape=True), want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("method,pillow", [("bilinear", "BILINEAR"), ("cubic", "BICUBIC"), ("lanczos", "LANCZOS")])
def test_interpolation_against_pillow_on_complete_windows(method, pillow):
    """40 x 50 float32 (values around 100, up to about 220) -> 93 x 117 against Pillow's `resize` in mode F, on the cells whose
    window lies inside the raster (Pillow clips the window at the rim, the rule falls back to bilinear there).  Measured with
    Pillow 12.2: the largest difference is 1.5258789e-05 for each of the three filters, one unit in the last place of a float32
    between 128 and 256, which is Pillow's output type.  Tolerance: 4 x that, 6.2e-05, for other Pillow builds."""
    Image = pytest.importorskip("PIL.Image")
    src_shape, dst_shape = (40, 50), (93, 117)
    src = _raster(src_shape, 40)
    got = ro.resample(src, dst_shape, method, by_shape=True)
    want = np.asarray(Image.fromarray(src, mode="F").resize((dst_shape[1], dst_shape[0]), getattr(Image, pillow)))
    t = ro.tables(method, src_shape, dst_shape, None, ro.shape_transform(src_shape, dst_shape))
    taps = t["w_y"].shape[1]
    complete = (((t["first_y"] >= 0) & (t["first_y"] + taps <= src_shape[0]))[:, None]
                & ((t["first_x"] >= 0) & (t["first_x"] + taps <= src_shape[1]))[None, :])
    assert complete.mean() >= 0.75
    worst = float(np.abs(got - want)[complete].max())
    print(method, "complete", complete.mean(), "largest difference", worst)
    assert worst <= 6.2e-05


@pytest.mark.parametrize("factor", [(2, 2), (3, 5), (8, 8), (9, 4), (16, 20)])
def test_area_methods_by_integer_factors(factor):
    fy, fx = factor
    h, w = 6, 7
    rng = np.random.default_rng(fy * 31 + fx)
    for dtype in (np.float32, np.float64, np.int32, np.uint8):
        a = rng.integers(0, 50, (h * fy, w * fx)).astype(dtype)
        blocks = a.reshape(h, fy, w, fx)
        wide = blocks.astype(np.float64)
        out = np.float32 if dtype == np.float32 else np.float64
        want = {"sum": wide.sum(axis=(1, 3)).astype(out), "average": (wide.sum(axis=(1, 3)) / (fy * fx)).astype(out),
                "min": blocks.min(axis=(1, 3)), "max": blocks.max(axis=(1, 3))}
        mode = np.empty((h, w), dtype)
        for r in range(h):
            for c in range(w):
                values, counts = np.unique(blocks[r, :, c, :], return_counts=True)
                mode[r, c] = values[np.argmax(counts)]            # the first maximum of sorted values: ties to the smaller
        want["mode"] = mode
        for method in ("sum", "average", "min", "max") + (("mode",) if fy * fx <= 1024 else ()):
            got = ro.resample(a, (h, w), method, by_shape=True)
            assert got.dtype == want[method].dtype and np.array_equal(got, want[method]), (method, dtype, factor)


# ------------------------------------------------------------------ properties of the rule
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_identity_returns_the_input_bit_for_bit(dtype):
    dtype = np.dtype(dtype)
    src = _raster((11, 13), 42, dtype)
    if dtype.kind == "f":
        src[3, 4], src[0, 0], src[9, 9], src[5, 5] = np.nan, -0.0, np.inf, 1e-310 if dtype == np.float64 else 1e-42
    else:
        src[0, 0], src[1, 1] = np.iinfo(dtype).max, np.iinfo(dtype).min
    for method in METHODS:
        keep = method in ("nearest", "min", "max", "mode")
        got = ro.resample(src, src.shape, method, by_shape=True, dtype=None if keep or dtype.kind != "f" else dtype)
        want = src if keep or dtype.kind == "f" else src.astype(np.float64)
        assert got.dtype == want.dtype, method
        same = (np.ascontiguousarray(got).view(np.uint8) == np.ascontiguousarray(want).view(np.uint8)).reshape(want.shape + (-1,)).all(axis=-1)
        assert (same | ((got != got) & (want != want))).all(), method


def test_a_flipped_transform_equals_flipping_the_arrays():
    src = _raster((17, 33), 43)
    src[4, 7], src[:2, :5] = np.nan, np.nan
    S = (30.0, 0.0, 120.0, 0.0, -30.0, 900.0)
    D = (13.0, 0.0, 100.0, 0.0, -11.0, 905.0)
    D_flip = (-13.0, 0.0, 100.0 + 13.0 * 30, 0.0, 11.0, 905.0 - 11.0 * 20)
    S_flip = (-30.0, 0.0, 120.0 + 30.0 * 33, 0.0, 30.0, 900.0 - 30.0 * 17)
    for method in METHODS:
        plain = ro.resample(src, (20, 30), method, S, D)
        for name, got in (("destination", ro.resample(src, (20, 30), method, S, D_flip)[::-1, ::-1]),
                          ("source", ro.resample(src[::-1, ::-1], (20, 30), method, S_flip, D))):
            if method in ("nearest", "min", "max", "mode"):
                assert np.array_equal(got, plain, equal_nan=True), (method, name)
            else:                                                 # the sums run the other way round: last bits
                np.testing.assert_allclose(got, plain, rtol=1e-5, atol=0.0, equal_nan=True, err_msg=f"{method} {name}")


@pytest.mark.parametrize("grid", ["up", "down", "world", "partly_outside", "around"])
def test_the_four_point_methods_share_their_nan_mask(grid):
    src_shape, dst_shape, S, D = GRIDS[grid]
    src = _raster(src_shape, 44)
    src[src_shape[0] // 2, src_shape[1] // 3] = np.nan
    src[1::4, ::3] = np.nan
    src[src_shape[0] // 4:src_shape[0] // 2, :src_shape[1] // 3] = np.nan
    kw = {"by_shape": True} if D is None else {"src_transform": S, "dst_transform": D}
    masks = [np.isnan(ro.resample(src, dst_shape, method, **kw)) for method in ("nearest", "bilinear", "cubic", "lanczos")]
    assert masks[0].any() and not masks[0].all()
    for m in masks[1:]:
        assert np.array_equal(m, masks[0])
    clean = _raster(src_shape, 44)                                # and without invalid cells the mask is the footprint alone
    t = ro.tables("nearest", src_shape, dst_shape, S, D if D is not None else ro.shape_transform(src_shape, dst_shape))
    outside = (t["near_y"] < 0)[:, None] | (t["near_x"] < 0)[None, :]
    for method in ("nearest", "bilinear", "cubic", "lanczos"):
        assert np.array_equal(np.isnan(ro.resample(clean, dst_shape, method, **kw)), outside)


def test_shape_coords_are_recomputed():
    y, x = 5000.0 - 12.5 - 25.0 * np.arange(70), 300.0 + 12.5 + 25.0 * np.arange(130)
    from xrspatial_amd.resample import _shape_coords
    agg = xs.DataArray(np.zeros((70, 130), np.float32), dims=["lat", "lon"], coords={"lat": y, "lon": x})
    coords = _shape_coords(agg, 35, 65)
    np.testing.assert_allclose(coords["lat"], 5000.0 - 25.0 - 50.0 * np.arange(35), rtol=1e-12)
    np.testing.assert_allclose(coords["lon"], 300.0 + 25.0 + 50.0 * np.arange(65), rtol=1e-12)
    uneven = xs.DataArray(np.zeros((3, 3), np.float32), dims=["y", "x"], coords={"y": [0.0, 1.0, 5.0], "x": [0.0, 1.0, 2.0]})
    assert _shape_coords(uneven, 2, 2) is None
    assert _shape_coords(_agg(), 2, 2) is None

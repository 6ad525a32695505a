"""resample on the MI355X, bit for bit against the written rule (tests/resample_oracle.py), tolerance 0.  The
cases are the smallest that reach each path of csrc/resample.hip: destinations cut around the 32 x 8 tile on both axes, every
method up and down by a ratio that is no integer, the tap count at which `weighted` changes from the LDS tile to one wave per
cell, windows of 256 taps and of 1024 `mode` cells, every dtype, every kind of invalid cell, destinations that leave the source
on every side, and the three entries at the C ABI with tables the Python layer never makes.  Every comparison records its cell
count (tests/parity_log.py)."""
import re

import numpy as np
import pytest

from tests import parity_log
from tests import resample_oracle as ro

pytestmark = pytest.mark.gpu

METHODS = ("nearest", "bilinear", "cubic", "lanczos", "average", "sum", "min", "max", "mode")
WEIGHTED = ("bilinear", "cubic", "lanczos", "average", "sum")
KEEP_DTYPE = ("nearest", "min", "max", "mode")
DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64)
CODE = {np.dtype(d): c for c, d in enumerate((np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64,
                                               np.float64, np.float32))}


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(config, op, got, want):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (config, op, got.dtype, want.dtype, got.shape, want.shape)
    parity_log.record(config, op, got, want, tol=0)
    ok = (_bits(got) == _bits(want)) | ((got != got) & (want != want))
    assert ok.all(), (config, op, np.argwhere(~ok)[:5].tolist(), got[~ok][:5].tolist(), want[~ok][:5].tolist())


def _raster(shape, seed=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.normal(100.0, 30.0, shape).astype(dtype)
    return rng.integers(0, 100, shape).astype(dtype)


def _by_shape(xs, config, src, dst_shape, method, **kw):
    """`resample(shape=)` against the oracle; returns the oracle's result."""
    want = ro.resample(src, dst_shape, method, by_shape=True, **kw)
    got = xs.resample(xs.DataArray(src, dims=["y", "x"]), shape=dst_shape, method=method, **kw)
    _same(config, f"resample_{method}", got.data, want)
    return want


def _by_like(xs, config, src, dst_shape, method, S, D, **kw):
    want = ro.resample(src, dst_shape, method, S, D, **kw)
    like = xs.DataArray(np.zeros(dst_shape, np.uint8), dims=["y", "x"])
    got = xs.resample(xs.DataArray(src, dims=["y", "x"]), like, method=method, src_transform=S, dst_transform=D, **kw)
    _same(config, f"resample_{method}", got.data, want)
    return want


# ------------------------------------------------------------------ tiles cut on both axes
@pytest.mark.parametrize("src_shape", [(1, 1), (1, 300), (300, 1), (17, 33)])
def test_shapes_around_the_tile(xs, src_shape):
    src = _raster(src_shape, sum(src_shape))
    for dst_shape in ((7, 31), (8, 32), (9, 33)):
        for method in METHODS:
            _by_shape(xs, f"shape_{src_shape[0]}x{src_shape[1]}_to_{dst_shape[0]}x{dst_shape[1]}", src, dst_shape, method)


# ------------------------------------------------------------------ every method, up and down
@pytest.mark.parametrize("method", METHODS)
def test_methods_up_and_down(xs, method):
    up = _by_shape(xs, "up_17x33_to_40x70", _raster((17, 33), 1), (40, 70), method)
    down = _by_shape(xs, "down_70x130_to_17x33", _raster((70, 130), 2), (17, 33), method)
    assert not np.isnan(up).any() and not np.isnan(down).any()
    ints = _raster((70, 130), 3, np.int16)
    _by_shape(xs, "down_70x130_to_17x33_int16", ints, (17, 33), method)


# ------------------------------------------------------------------ the tap count between the two weighted kernels
def test_tap_boundary_of_the_tile_kernel(xs):
    for src_shape, taps in (((64, 64), (8, 8)), ((72, 72), (9, 9)), ((64, 72), (8, 9)), ((72, 64), (9, 8)), ((54, 54), (8, 8)),
                            ((61, 63), (9, 9)), ((54, 61), (8, 9))):
        t = xs.resample.tables("average", src_shape, (8, 8), None, xs.resample.shape_transform(src_shape, (8, 8)))
        assert (t["w_y"].shape[1], t["w_x"].shape[1]) == taps
        src = _raster(src_shape, taps[0] + taps[1])
        src[5, 7] = np.nan
        for method in ("average", "sum"):
            _by_shape(xs, f"taps_{taps[0]}x{taps[1]}_{src_shape[0]}", src, (8, 8), method)


def test_256_taps_are_accepted_and_257_refused(xs):
    src = _raster((256, 300), 4)
    t = xs.resample.tables("average", src.shape, (1, 3), None, xs.resample.shape_transform(src.shape, (1, 3)))
    assert (t["w_y"].shape[1], t["w_x"].shape[1]) == (256, 100)
    for method in ("average", "sum", "min", "max"):
        _by_shape(xs, "taps_256x100", src, (1, 3), method)
    with pytest.raises(ValueError, match="more than the 256 taps.*two steps"):
        xs.resample(xs.DataArray(np.zeros((257, 3), np.float32), dims=["y", "x"]), shape=(1, 3), method="average")


# ------------------------------------------------------------------ large windows
def test_direct_walk_300_to_3(xs):
    src = _raster((300, 300), 5)
    src[::7, ::5] = np.nan
    for method in ("average", "sum", "min", "max"):
        _by_shape(xs, "direct_300_to_3", src, (3, 3), method)
    _by_shape(xs, "direct_300_to_3_f64", src.astype(np.float64), (3, 3), "average", dtype=np.float32)


@pytest.mark.parametrize("src_shape,dst_shape,window", [((6, 8), (6, 8), 1), ((4, 8), (4, 4), 2), ((16, 16), (2, 2), 64),
                                                       ((10, 26), (2, 2), 65), ((64, 64), (2, 2), 1024)])
def test_mode_windows_with_exact_ties(xs, src_shape, dst_shape, window):
    t = xs.resample.tables("mode", src_shape, dst_shape, None, xs.resample.shape_transform(src_shape, dst_shape))
    assert t["w_y"].shape[1] * t["w_x"].shape[1] == window
    rng = np.random.default_rng(window)
    few = rng.integers(3, 7, src_shape)                           # four classes: ties by the dozen
    pairs = np.arange(src_shape[0] * src_shape[1]).reshape(src_shape) // 2 % 5    # every class of a window as often
    for name, values in (("few", few), ("pairs", pairs)):
        for dtype in (np.uint8, np.int64, np.float32, np.float64):
            _by_shape(xs, f"mode_window_{window}_{name}", values.astype(dtype), dst_shape, "mode")
    zeros = np.where(rng.random(src_shape) < 0.5, -0.0, 0.0).astype(np.float32)   # one class: its first member's sign
    zeros[rng.random(src_shape) < 0.2] = 1.0
    want = _by_shape(xs, f"mode_window_{window}_signed_zero", zeros, dst_shape, "mode")
    assert window == 1 or (want == 0).any()
    holes = few.astype(np.float64)
    holes[rng.random(src_shape) < 0.3] = np.nan
    _by_shape(xs, f"mode_window_{window}_nan", holes, dst_shape, "mode")


def test_mode_window_above_1024_is_refused(xs):
    with pytest.raises(ValueError, match="mode window.*more than 1024.*two steps"):
        xs.resample(xs.DataArray(np.zeros((66, 64), np.uint8), dims=["y", "x"]), shape=(2, 2), method="mode")


# ------------------------------------------------------------------ dtypes
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_dtype(xs, dtype):
    dtype = np.dtype(dtype)
    src = _raster((17, 33), 6, dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        src[::3, ::4] = info.max
        src[1::3, 1::4] = info.min
        src[2::5, 2::3] = info.max - 1
    for method in KEEP_DTYPE:
        for dst_shape in ((40, 70), (5, 9)):
            want = _by_shape(xs, f"dtype_{dtype.name}", src, dst_shape, method)
            assert want.dtype == dtype
    for method in WEIGHTED:
        for dst_shape in ((40, 70), (5, 9)):
            want = _by_shape(xs, f"dtype_{dtype.name}", src, dst_shape, method)
            assert want.dtype == (np.float32 if dtype == np.float32 else np.float64)


def test_dtype_override(xs):
    src = _raster((17, 33), 7)
    for method in WEIGHTED:
        assert _by_shape(xs, "f32_to_f64", src, (40, 70), method, dtype=np.float64).dtype == np.float64
        assert _by_shape(xs, "f64_to_f32", src.astype(np.float64) * 1.000001, (40, 70), method, dtype=np.float32).dtype == np.float32
    with pytest.raises(TypeError, match="returns the input's dtype"):
        xs.resample(xs.DataArray(src, dims=["y", "x"]), shape=(4, 4), method="nearest", dtype=np.float64)
    with pytest.raises(TypeError, match="float64 or float32"):
        xs.resample(xs.DataArray(src, dims=["y", "x"]), shape=(4, 4), method="bilinear", dtype=np.int32)


# ------------------------------------------------------------------ invalid cells
def _holes(kind, shape, seed):
    src = _raster(shape, seed)
    if kind == "one":
        src[shape[0] // 2, shape[1] // 3] = np.nan
    elif kind == "rim":
        src[0], src[-1], src[:, 0], src[:, -1] = np.nan, np.nan, np.nan, np.nan
    elif kind == "checkerboard":
        jj, ii = np.mgrid[0:shape[0], 0:shape[1]]
        src[(jj + ii) % 2 == 0] = np.nan
    elif kind == "all":
        src[:] = np.nan
    return src


@pytest.mark.parametrize("kind", ["one", "rim", "checkerboard", "all"])
def test_nan_cells(xs, kind):
    for src_shape, dst_shape in (((17, 33), (40, 70)), ((70, 130), (17, 33))):
        src = _holes(kind, src_shape, 8)
        for method in METHODS:
            want = _by_shape(xs, f"nan_{kind}_{src_shape[0]}", src, dst_shape, method)
            if kind == "all":
                assert np.isnan(want).all()
        _by_shape(xs, f"nan_{kind}_{src_shape[0]}_fill", src, dst_shape, "bilinear", fill=-1.0)


def test_clean_path_and_bilinear_fallback_in_one_tile(xs):
    src = _holes("one", (17, 33), 9)
    for method in ("cubic", "lanczos"):
        want = _by_shape(xs, "fallback_in_tile", src, (40, 70), method)
        clean = ro.resample(_raster((17, 33), 9), (40, 70), method, by_shape=True)
        bilinear = ro.resample(src, (40, 70), "bilinear", by_shape=True)
        tile = (slice(16, 24), slice(0, 32))                      # the tile of destination rows 16 .. 23, columns 0 .. 31
        differs = want[tile] != clean[tile]
        assert differs.any() and not differs.all()                # both rules in this one tile
        assert np.array_equal(want[tile][differs & ~np.isnan(want[tile])], bilinear[tile][differs & ~np.isnan(want[tile])])


def test_nodata_on_an_integer_raster(xs):
    for src_shape, dst_shape in (((70, 130), (17, 33)), ((17, 33), (40, 70))):
        src = _raster(src_shape, 10, np.int16)
        src[src % 7 == 0] = -9999
        for method in METHODS:
            fill = -1 if method in KEEP_DTYPE else None
            kw = {} if fill is None else {"fill": fill}
            want = _by_shape(xs, f"nodata_int16_{dst_shape[0]}", src, dst_shape, method, nodata=-9999, **kw)
            assert not (want == -9999).any()
    unsigned = _raster((20, 30), 11, np.uint8)
    _by_shape(xs, "nodata_not_representable", unsigned, (7, 9), "mode", nodata=-9999)
    _by_shape(xs, "nodata_255", np.where(unsigned > 50, 255, unsigned).astype(np.uint8), (7, 9), "average", nodata=255)


# ------------------------------------------------------------------ outside the source
OUTSIDE = {
    "left": (0.7, 0.0, -6.3, 0.0, 0.8, 1.2), "right": (0.7, 0.0, 20.4, 0.0, 0.8, 1.2), "top": (0.7, 0.0, 3.1, 0.0, 0.8, -5.5),
    "bottom": (0.7, 0.0, 3.1, 0.0, 0.8, 9.9), "around": (2.1, 0.0, -8.0, 0.0, 2.3, -7.0),
    "wholly": (0.7, 0.0, 100.0, 0.0, 0.8, 1.2), "wholly_negative": (0.7, 0.0, -300.0, 0.0, 0.8, -200.0),
}


@pytest.mark.parametrize("side", list(OUTSIDE))
def test_destination_outside_the_source(xs, side):
    src = _raster((17, 33), 12)
    S, D = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), OUTSIDE[side]
    for method in METHODS:
        want = _by_like(xs, f"outside_{side}", src, (20, 30), method, S, D)
        if side.startswith("wholly"):
            assert np.isnan(want).all()
        else:
            assert np.isnan(want).any() and not np.isnan(want).all()
    ints = _raster((17, 33), 12, np.int32)
    for method in KEEP_DTYPE:
        _by_like(xs, f"outside_{side}_int32", ints, (20, 30), method, S, D, fill=-7)


# ------------------------------------------------------------------ properties on the device
def test_identity_is_bit_for_bit(xs):
    for dtype in (np.float32, np.float64, np.int64, np.uint8):
        src = _raster((17, 33), 13, dtype)
        if np.dtype(dtype).kind == "f":
            src[3, 4], src[0, 0], src[9, 9] = np.nan, -0.0, np.inf
        for method in METHODS:
            got = xs.resample(xs.DataArray(src, dims=["y", "x"]), shape=src.shape, method=method, dtype=dtype if method in WEIGHTED and np.dtype(dtype).kind == "f" else None)
            want = src if method in KEEP_DTYPE or np.dtype(dtype).kind == "f" else src.astype(np.float64)
            _same(f"identity_{np.dtype(dtype).name}", f"resample_{method}", got.data, want)


def test_flips_and_the_shared_nan_mask(xs):
    src = _holes("one", (17, 33), 14)
    src[:2, :5] = np.nan
    S = (30.0, 0.0, 120.0, 0.0, -30.0, 900.0)
    D = (13.0, 0.0, 100.0, 0.0, -11.0, 905.0)                     # 20 x 30 cells from (100, 905): partly outside
    D_flip = (-13.0, 0.0, 100.0 + 13.0 * 30, 0.0, 11.0, 905.0 - 11.0 * 20)
    masks = []
    for method in METHODS:
        plain = _by_like(xs, "flip_plain", src, (20, 30), method, S, D)
        flipped = _by_like(xs, "flip_flipped", src, (20, 30), method, S, D_flip)
        if method in ("nearest", "min", "max", "mode"):
            assert np.array_equal(flipped[::-1, ::-1], plain, equal_nan=True)
        else:
            np.testing.assert_allclose(flipped[::-1, ::-1], plain, rtol=1e-5, equal_nan=True)
        if method in ("nearest", "bilinear", "cubic", "lanczos"):
            masks.append(np.isnan(plain))
    assert masks[0].any() and not masks[0].all() and all(np.array_equal(m, masks[0]) for m in masks[1:])


# ------------------------------------------------------------------ backends, dims and coords
def test_backends_give_the_same_bits(xs):
    src = _holes("one", (70, 130), 15)
    y, x = 5000.0 - 12.5 - 25.0 * np.arange(70), 300.0 + 12.5 + 25.0 * np.arange(130)
    host = xs.DataArray(src, dims=["lat", "lon"], coords={"lat": y, "lon": x}, attrs={"res": 25}, name="dem")
    dev = xs.DataArray(xs.DeviceArray.from_numpy(src), dims=["lat", "lon"], coords={"lat": y, "lon": x}, attrs={"res": 25})
    like = xs.DataArray(np.zeros((17, 33), np.int8), dims=["y", "x"],
                        coords={"y": 5000.0 - 50.0 - 100.0 * np.arange(17), "x": 300.0 + 50.0 + 100.0 * np.arange(33)})
    S, D = xs.transform_from_coords(host), xs.transform_from_coords(like)
    for method in METHODS:
        a = xs.resample(host, like, method=method)
        b = xs.resample(dev, like, method=method, name="out")
        assert isinstance(a.data, np.ndarray) and isinstance(b.data, xs.DeviceArray)
        assert a.dims == b.dims == ("y", "x") and a.name == "dem" and b.name == "out" and a.attrs == {"res": 25}
        assert np.array_equal(a.coords["y"].values, like.coords["y"].values)
        want = ro.resample(src, (17, 33), method, S, D)
        _same("backend_host", f"resample_{method}", a.data, want)
        _same("backend_device", f"resample_{method}", b.data.get(), want)
        c = xs.resample(dev, shape=(35, 65), method=method)
        assert isinstance(c.data, xs.DeviceArray) and c.dims == ("lat", "lon")
        np.testing.assert_allclose(c.coords["lat"].values, 5000.0 - 25.0 - 50.0 * np.arange(35))
        _same("backend_device_shape", f"resample_{method}", c.data.get(), ro.resample(src, (35, 65), method, by_shape=True))
    with pytest.raises(NotImplementedError, match="resample\\(\\) does not support row-sharded"):
        xs.resample(xs.DataArray(xs.ShardedArray(8, 8, np.float32), dims=["y", "x"]), shape=(4, 4))


# ------------------------------------------------------------------ at the C ABI, with tables the Python layer never makes
def _random_taps(rng, n_dst, n_src, taps, inside):
    """Non-monotone `first`, weights of either sign with zeros in the middle of a row."""
    if inside:
        first = rng.integers(0, max(n_src - taps, 0) + 1, n_dst)
    else:
        first = rng.integers(-taps - 3, n_src + 3, n_dst)
    w = rng.normal(0.0, 1.0, (n_dst, taps))
    w[rng.random((n_dst, taps)) < 0.3] = 0.0
    return first.astype(np.int32), np.ascontiguousarray(w)


def _dev(xs, *arrays):
    return [None if a is None else xs.DeviceArray.from_numpy(a) for a in arrays]


def _ptr(a):
    return None if a is None else a.ptr


@pytest.mark.parametrize("src_shape,taps", [((40, 50), (5, 8)), ((200, 50), (8, 3)), ((40, 50), (9, 4)), ((90, 70), (3, 70)),
                                            ((300, 20), (130, 2))])
def test_abi_weighted_on_hand_built_tables(xs, src_shape, taps):
    from xrspatial_amd import _lib
    rng = np.random.default_rng(sum(src_shape) + sum(taps))
    src = _raster(src_shape, 16, np.float64)
    src[rng.random(src_shape) < 0.05] = np.nan
    rows, cols = 11, 35
    dsrc, = _dev(xs, src)
    for inside in (True, False):
        fy, wy = _random_taps(rng, rows, src_shape[0], taps[0], inside)
        fx, wx = _random_taps(rng, cols, src_shape[1], taps[1], inside)
        ny = rng.integers(-1, src_shape[0] + 2, rows).astype(np.int32)
        nx = rng.integers(-1, src_shape[1] + 2, cols).astype(np.int32)
        by, bwy = _random_taps(rng, rows, src_shape[0], 2, inside)
        bx, bwx = _random_taps(rng, cols, src_shape[1], 3, inside)
        bwy, bwx = np.abs(bwy), np.abs(bwx)
        d = _dev(xs, fy, wy, fx, wx, ny, nx, by, bwy, bx, bwx)
        for near, fb, divide, code, dtype in ((False, False, 1, 8, np.float64), (True, True, 1, 9, np.float32),
                                              (False, True, 0, 8, np.float64), (True, False, 0, 9, np.float32)):
            out = xs.DeviceArray((rows, cols), dtype)
            _lib.call("xrs_resample_weighted", dsrc.ptr, 8, src_shape[0], src_shape[1], None, rows, cols,
                      d[0].ptr, d[1].ptr, taps[0], d[2].ptr, d[3].ptr, taps[1],
                      d[4].ptr if near else None, d[5].ptr if near else None,
                      d[6].ptr if fb else None, d[7].ptr if fb else None, 2 if fb else 0,
                      d[8].ptr if fb else None, d[9].ptr if fb else None, 3 if fb else 0,
                      divide, code, -3.0, out.ptr, None)
            _lib.call("xrs_device_sync")
            want = ro.weighted(src, fy, wy, fx, wx, ny if near else None, nx if near else None,
                               (by, bwy, bx, bwx) if fb else None, bool(divide), None, -3.0, dtype)
            _same(f"abi_weighted_{taps[0]}x{taps[1]}_{src_shape[0]}_in{int(inside)}_near{int(near)}_fb{int(fb)}",
                  "resample_weighted", out.get(), want)


@pytest.mark.parametrize("dtype", [np.uint8, np.int64, np.float32])
def test_abi_gather_and_select_on_hand_built_tables(xs, dtype):
    from xrspatial_amd import _lib
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(17)
    src_shape, rows, cols = (40, 50), 19, 37
    src = rng.integers(0, 6, src_shape).astype(dtype)
    if dtype.kind == "f":
        src[rng.random(src_shape) < 0.1] = np.nan
    dsrc, = _dev(xs, src)
    nodata, fill = np.array([3], dtype), np.array([77], dtype)
    ny = rng.integers(-2, src_shape[0] + 2, rows).astype(np.int32)
    nx = rng.integers(-2, src_shape[1] + 2, cols).astype(np.int32)
    ny[0], nx[0] = 10**6, -10**6
    dny, dnx = _dev(xs, ny, nx)
    for nd in (None, nodata):
        out = xs.DeviceArray((rows, cols), dtype)
        _lib.call("xrs_resample_gather", dsrc.ptr, CODE[dtype], *src_shape, None if nd is None else nd.ctypes.data, rows, cols,
                  dny.ptr, dnx.ptr, fill.ctypes.data, out.ptr, None)
        _lib.call("xrs_device_sync")
        _same(f"abi_gather_{dtype.name}_nodata{int(nd is not None)}", "resample_gather", out.get(),
              ro.gather(src, ny, nx, None if nd is None else nd[0], fill[0]))
    for taps in ((3, 4), (8, 8), (9, 8), (32, 32)):
        for inside in (True, False):
            fy, wy = _random_taps(rng, rows, src_shape[0], taps[0], inside)
            fx, wx = _random_taps(rng, cols, src_shape[1], taps[1], inside)
            d = _dev(xs, fy, wy, fx, wx)
            for op, name in enumerate(("min", "max", "mode")):
                out = xs.DeviceArray((rows, cols), dtype)
                _lib.call("xrs_resample_select", dsrc.ptr, CODE[dtype], *src_shape, nodata.ctypes.data, rows, cols, d[0].ptr, d[1].ptr,
                          taps[0], d[2].ptr, d[3].ptr, taps[1], op, fill.ctypes.data, out.ptr, None)
                _lib.call("xrs_device_sync")
                _same(f"abi_select_{dtype.name}_{taps[0]}x{taps[1]}_in{int(inside)}", f"resample_{name}", out.get(),
                      ro.select(src, fy, wy, fx, wx, name, nodata[0], fill[0]))


def test_abi_refusals(xs):
    from xrspatial_amd import _lib
    lib = _lib.load()
    src = xs.DeviceArray.from_numpy(np.zeros((8, 8), np.float32))
    out = xs.DeviceArray((4, 4), np.float64)
    first, w = _dev(xs, np.zeros(4, np.int32), np.ones((4, 2)))
    fill = np.zeros(1, np.float32)
    head = (src.ptr, 9, 8, 8, None, 4, 4)
    taps = (first.ptr, w.ptr, 2, first.ptr, w.ptr, 2)
    none6 = (None, None, 0, None, None, 0)
    refusals = [
        (lambda: lib.xrs_resample_gather(src.ptr, 12, 8, 8, None, 4, 4, first.ptr, first.ptr, fill.ctypes.data, out.ptr, None),
         "dtype code 12"),
        (lambda: lib.xrs_resample_gather(*head, None, first.ptr, fill.ctypes.data, out.ptr, None), "null pointer"),
        (lambda: lib.xrs_resample_gather(None, 9, 8, 8, None, 4, 4, first.ptr, first.ptr, fill.ctypes.data, out.ptr, None),
         "null pointer"),
        (lambda: lib.xrs_resample_gather(src.ptr, 9, 0, 8, None, 4, 4, first.ptr, first.ptr, fill.ctypes.data, out.ptr, None),
         "at least \\(1, 1\\)"),
        (lambda: lib.xrs_resample_gather(src.ptr, 9, 2**17, 2**15, None, 4, 4, first.ptr, first.ptr, fill.ctypes.data, out.ptr, None),
         "exceed the 32-bit cell index"),
        (lambda: lib.xrs_resample_weighted(*head, first.ptr, w.ptr, 257, first.ptr, w.ptr, 2, None, None, *none6, 1, 8, 0.0, out.ptr,
                                           None), "257 taps on the y axis"),
        (lambda: lib.xrs_resample_weighted(*head, first.ptr, w.ptr, 2, first.ptr, w.ptr, 0, None, None, *none6, 1, 8, 0.0, out.ptr,
                                           None), "0 taps on the x axis"),
        (lambda: lib.xrs_resample_weighted(*head, *taps, first.ptr, None, *none6, 1, 8, 0.0, out.ptr, None), "one axis only"),
        (lambda: lib.xrs_resample_weighted(*head, *taps, None, None, first.ptr, None, 2, None, None, 0, 1, 8, 0.0, out.ptr, None),
         "fallback y"),
        (lambda: lib.xrs_resample_weighted(*head, *taps, None, None, *none6, 1, 4, 0.0, out.ptr, None), "output dtype code 4"),
        (lambda: lib.xrs_resample_weighted(*head, *taps, None, None, *none6, 1, 8, 0.0, None, None), "null pointer"),
        (lambda: lib.xrs_resample_select(*head, *taps, 3, fill.ctypes.data, out.ptr, None), "unknown op 3"),
        (lambda: lib.xrs_resample_select(*head, first.ptr, w.ptr, 33, first.ptr, w.ptr, 32, 2, fill.ctypes.data, out.ptr, None),
         "mode window of 33 x 32"),
        (lambda: lib.xrs_resample_select(*head, *taps, 0, None, out.ptr, None), "null pointer"),
    ]
    for call, text in refusals:
        assert call() != 0
        assert re.search(text, _lib.last_error()), (text, _lib.last_error())

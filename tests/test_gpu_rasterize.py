"""rasterize on the MI355X, bit for bit against the written rule (tests/rasterize_oracle.py): the round trip of
polygonize's own output, the seams of the 64-cell chunks and the 256-thread blocks of csrc/rasterize.hip, polygons outside the
raster and inputs without a crossing, holes, the five merges in the ten dtypes, partitions, transforms, and the calls at the C
ABI.  Tolerance 0 throughout; every comparison records its cell count (tests/parity_log.py)."""
import ctypes

import numpy as np
import pytest

from tests import parity_log
from tests import rasterize_oracle as ro
from tests.golden import make_polygonize_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = gen.case_names(FIXTURE)
DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float64, np.float32)   # XRS_DT_* 0 .. 9
SHEAR = gen.FMA_TRANSFORM


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _like(xs, shape):
    return xs.DataArray(np.zeros(shape, np.float32), dims=["y", "x"])


def _same(config, got, want, op="rasterize"):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (config, got.dtype, want.dtype)
    parity_log.record(config, op, got, want, tol=0)
    assert gen.same(got, want), (config, np.argwhere(~((got == want) | ((got != got) & (want != want))))[:10].tolist())


def _check(xs, config, shapes, shape, column=None, **kw):
    want = ro.rasterize(*shapes, shape, column, **kw)
    _same(config, xs.rasterize(tuple(shapes), _like(xs, shape), column, **kw).data, want)
    return want


def _square(x0, y0, x1, y1, reverse=False):
    ring = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]], np.float64)
    return ring[::-1].copy() if reverse else ring


# ------------------------------------------------------------------ the fixture, there and back
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("case", CASES)
def test_round_trip_of_polygonize(xs, case, c):
    a, mask, transform = FIXTURE[f"{case}/in"], FIXTURE.get(f"{case}/mask"), FIXTURE.get(f"{case}/transform")
    agg = xs.DataArray(a, dims=["y", "x"])
    magg = None if mask is None else xs.DataArray(mask, dims=["y", "x"])
    column, polygons = xs.polygonize(agg, mask=magg, connectivity=c, transform=transform)
    flat = xs.polygonize(agg, mask=magg, connectivity=c, transform=transform, return_type="flat")
    fill = np.nan if a.dtype.kind == "f" else 7
    col = np.array(column, dtype=a.dtype)
    if a.dtype.kind == "f":                                      # a region carries its first cell's value: NaNs, values within the tolerance
        want = ro.rasterize(*flat[1:], a.shape, col, transform=transform, fill=fill)
    else:
        want = np.where(np.ones(a.shape, bool) if mask is None else mask != 0, a, a.dtype.type(fill))
    for form, shapes in (("list", polygons), ("flat", tuple(flat[1:]))):
        got = xs.rasterize(shapes, agg, col, transform=transform, fill=fill)
        assert got.dims == agg.dims and got.name == "rasterize"
        _same(f"fixture_{case}_c{c}_{form}", got.data, want)


# ------------------------------------------------------------------ chunk and block seams
@pytest.mark.parametrize("shape", [(5, 1), (7, 63), (7, 64), (7, 65), (3, 129), (1, 1), (300, 1), (1, 300), (300, 129)])
def test_chunk_and_block_seams(xs, shape):
    H, W = shape
    polys = [[_square(-1, -1, W + 1, H + 1)],                                       # covers the whole raster
             [np.array([[0.2, -1.0], [W * 0.7, H + 1.0], [-3.0, H + 1.0]])],        # one edge through every row
             [np.array([[W * 0.3, H * 0.1], [W * 0.9, H * 0.2], [W * 0.8, H * 0.95], [W * 0.2, H * 0.7]])],   # spans start and end mid-chunk
             [_square(0, 0, W, H)],                                                 # edges on the cell borders
             [_square(0.5, 0.5, W - 0.5, H - 0.5)]]                                 # edges through the outermost centres
    shapes = ro.flatten(polys)
    for merge in ("last", "count", "first"):
        want = _check(xs, f"seams_{H}x{W}_{merge}", shapes, shape, merge=merge)
    assert want.min() >= 1
    cover = _check(xs, f"seams_{H}x{W}_cover", ro.flatten(polys[:1]), shape, np.array([9], np.uint16))
    assert np.all(cover == 9)
    for k in (1, 2):
        _check(xs, f"seams_{H}x{W}_poly{k}", ro.flatten(polys[k:k + 1]), shape, merge="count")


# ------------------------------------------------------------------ outside the raster, and nothing to burn
def test_polygons_outside_and_straddling(xs):
    shape = H, W = (9, 70)
    outside = [[_square(-9, 2, -1, 5)], [_square(W + 1, 2, W + 8, 5)], [_square(3, -7, 30, -0.6)], [_square(3, H + 0.6, 30, H + 9)]]
    for k, poly in enumerate(outside):
        want = _check(xs, f"outside_{k}", ro.flatten([poly]), shape, fill=3)
        assert np.all(want == 3)
    straddling = [[_square(-4.3, 2.2, 3.4, 6.6)], [_square(W - 2.6, 1.5, W + 5, 7.7)], [_square(10.2, -3, 20.7, 2.4)],
                  [_square(40.5, H - 2.5, 66.5, H + 4)], [np.array([[-5.0, -5.0], [W + 5.0, -2.0], [W * 0.5, H + 6.0]])]]
    for k, poly in enumerate(straddling):
        want = _check(xs, f"straddling_{k}", ro.flatten([poly]), shape, merge="count")
        assert want.any() and not want.all()
    _check(xs, "outside_and_straddling", ro.flatten(outside + straddling), shape)
    _check(xs, "outside_and_straddling_count", ro.flatten(outside + straddling), shape, merge="count")


def test_inputs_without_a_crossing(xs):
    shape = (6, 11)
    ring = np.array([[1.2, 0.7], [9.1, 1.3], [4.4, 5.2]])
    inputs = {"no_polygons": [], "polygon_without_rings": [[]], "empty_ring": [[np.empty((0, 2))]],
              "one_point": [[np.array([[3.0, 3.0]])]], "horizontal_only": [[np.array([[1.0, 2.5], [8.0, 2.5], [4.0, 2.5]])]],
              "between_the_centre_lines": [[_square(1, 1.6, 9, 2.4)]], "same_ring_twice": [[ring, ring[::-1].copy()]],
              "same_ring_twice_same_way": [[ring, ring.copy()]]}
    for name, polys in inputs.items():
        shapes = ro.flatten(polys)
        for kw in (dict(fill=-4), dict(merge="count"), dict(column=np.full(len(polys), 2.5, np.float32), fill=np.nan)):
            want = _check(xs, f"nothing_{name}", shapes, shape, **kw)
            assert np.all(want == 0) if "merge" in kw else np.all((want == -4) | np.isnan(want))
        _same(f"nothing_{name}_list", xs.rasterize(polys, _like(xs, shape), fill=-4).data, np.full(shape, -4, np.int32))
    mixed = [[np.empty((0, 2)), ring], [], [np.array([[1.0, 2.5], [8.0, 2.5]])], [ring + 1.0, np.empty((0, 2))]]
    _check(xs, "empty_rings_among_others", ro.flatten(mixed), shape)
    _same("empty_rings_among_others_list", xs.rasterize(mixed, _like(xs, shape)).data, ro.rasterize(*ro.flatten(mixed), shape))


# ------------------------------------------------------------------ holes
def test_holes_islands_and_orientation(xs):
    shape = (40, 70)
    outer = _square(2.3, 1.7, 66.6, 38.2)
    for k, (ho, isl) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        polys = [[outer, _square(10, 8, 50.5, 30.5, reverse=ho), _square(54, 5, 60, 35, reverse=not ho)],
                 [_square(20.5, 12.5, 40, 25, reverse=isl), _square(25, 15, 30, 20)]]
        want = _check(xs, f"holes_{k}", ro.flatten(polys), shape, np.array([5, 9], np.int64))
        assert want[20, 15] == 0 and want[20, 22] == 9 and want[17, 27] == 0 and want[3, 3] == 5 and want[20, 56] == 0
        _check(xs, f"holes_{k}_count", ro.flatten(polys), shape, merge="count")


# ------------------------------------------------------------------ merges and dtypes
@pytest.mark.parametrize("code", range(10))
def test_merges_in_every_dtype(xs, code):
    from xrspatial_amd.device import DTYPE_CODE
    dtype = np.dtype(DTYPES[code])
    assert DTYPE_CODE[dtype] == code
    shape = (97, 129)
    shapes = ro.random_polygons(100 + code, 40, shape)
    rng = np.random.default_rng(code)
    column = rng.integers(0, 6, 40).astype(dtype)                # equal values: min / max go to the later polygon
    if dtype.kind == "f":
        column = column + dtype.type(0.25)
    fill = np.nan if dtype.kind == "f" else 100
    for merge in (ro.MERGES[code % 5], ro.MERGES[(code + 2) % 5]):
        want = _check(xs, f"merge_{merge}_{dtype.name}", shapes, shape, column, fill=fill, dtype=dtype, merge=merge)
        assert want.dtype == dtype
    if code < 5:                                                 # the column in one dtype, the raster in another
        _check(xs, f"merge_cast_{dtype.name}", shapes, shape, column, fill=-1, dtype=np.float32, merge=ro.MERGES[code])


def test_default_column_and_backends(xs):
    shape = (33, 65)
    shapes = ro.random_polygons(7, 12, shape)
    want = ro.rasterize(*shapes, shape)
    assert want.dtype == np.int32 and want.max() <= 12
    dev_like = xs.DataArray(xs.DeviceArray.from_numpy(np.zeros(shape, np.uint8)), dims=["lat", "lon"], attrs={"res": 2})
    got = xs.rasterize(shapes, dev_like, name="zones")
    assert isinstance(got.data, xs.DeviceArray) and got.dims == ("lat", "lon") and got.attrs == {"res": 2} and got.name == "zones"
    _same("device_like", got.data.get(), want)
    host = xs.rasterize(shapes, _like(xs, shape))
    assert isinstance(host.data, np.ndarray)
    _same("host_like", host.data, want)
    _same("two_runs", xs.rasterize(shapes, _like(xs, shape)).data, host.data)
    with pytest.raises(NotImplementedError, match="rasterize\\(\\) does not support row-sharded"):
        xs.rasterize(shapes, xs.DataArray(xs.ShardedArray(8, 8, np.float32), dims=["y", "x"]))
    bad = shapes[0].copy()
    for v in (np.nan, np.inf, -np.inf):
        bad[5, 1] = v
        with pytest.raises(ValueError, match="a vertex is not finite"):
            xs.rasterize((bad,) + tuple(shapes[1:]), _like(xs, shape))


# ------------------------------------------------------------------ partitions
@pytest.mark.parametrize("snap", [False, True])
def test_partitions(xs, snap):
    shape = (13, 17)
    for seed in (0, 1):
        shapes = ro.partition(seed, snap)
        assert np.all(_check(xs, f"partition_{seed}_{int(snap)}_count", shapes, shape, merge="count") == 1)
        assert np.all(_check(xs, f"partition_{seed}_{int(snap)}_last", shapes, shape) >= 1)


# ------------------------------------------------------------------ transforms
def test_transforms(xs):
    shape = (40, 70)
    pts, ring_off, poly_off = ro.random_polygons(3, 25, shape)
    t = SHEAR
    world = np.stack([t[0] * pts[:, 0] + t[1] * pts[:, 1] + t[2], t[3] * pts[:, 0] + t[4] * pts[:, 1] + t[5]], axis=1)
    _check(xs, "transform_shear", (world, ring_off, poly_off), shape, transform=SHEAR)
    _check(xs, "transform_shear_count", (world, ring_off, poly_off), shape, transform=SHEAR, merge="count")
    from tests.golden import make_rasterize_witness as wit
    w = wit.load()                                               # an edge within a rounding error of a centre: fusing moves it
    for name in wit.TRANSFORMS:
        tw = w.get(f"{name}/transform")
        _check(xs, f"witness_{name}", (w[f"{name}/points"], np.array([0, 3]), np.array([0, 1])), tuple(int(v) for v in w["shape"]),
               transform=None if tw is None else tuple(tw))
    rng = np.random.default_rng(11)
    r = rng.integers(0, 4, (23, 31)).astype(np.int16)
    like = xs.DataArray(r, dims=["y", "x"], coords={"y": 5000.0 - 25.0 * np.arange(23), "x": 300.0 + 25.0 * np.arange(31)})
    T = xs.transform_from_coords(like)
    assert T[4] < 0
    column, polygons = xs.polygonize(like, transform=np.array(T))
    back = xs.rasterize(polygons, like, np.array(column, np.int16), transform=T)
    _same("transform_from_coords_round_trip", back.data, r)
    assert np.array_equal(back.coords["y"].values, like.coords["y"].values)


# ------------------------------------------------------------------ at the C ABI
@pytest.mark.parametrize("count", [0, 1])
def test_abi_crossings_and_plane(xs, count):
    from xrspatial_amd import _lib
    lib = _lib.load()
    shape = rows, cols = (97, 129)
    pts, ring_off, poly_off = ro.random_polygons(21, 40, shape)
    t = SHEAR
    world = np.ascontiguousarray(np.stack([t[0] * pts[:, 0] + t[1] * pts[:, 1] + t[2], t[3] * pts[:, 0] + t[4] * pts[:, 1] + t[5]], axis=1))
    n_points, n_rings, n_polys = len(world), len(ring_off) - 1, len(poly_off) - 1
    rng = np.random.default_rng(2)
    priority = rng.permutation(n_polys).astype(np.uint32)
    stats = {}
    want_count, want_winner = ro.planes(world, ring_off, poly_off, shape, priority, SHEAR, stats=stats)
    dev = [xs.DeviceArray.from_numpy(v) for v in (world, ring_off, poly_off, priority)]
    inv = (ctypes.c_double * 6)(*ro.inverse(SHEAR))
    work = xs.DeviceArray((_lib.workspace_bytes("rasterize", n_points),), np.uint8)
    args = (dev[0].ptr, dev[1].ptr, dev[2].ptr, n_points, n_rings, n_polys, rows, cols, inv)
    c, flags = ctypes.c_uint64(0), ctypes.c_int(-1)
    _lib.call("xrs_rasterize_census", *args, work.ptr, ctypes.byref(c), ctypes.byref(flags), None)
    assert c.value == stats["crossings"] and c.value % 2 == 0 and flags.value == 0
    spans = xs.DeviceArray((_lib.workspace_bytes("rasterize_spans", c.value),), np.uint8)
    ns, ni = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.call("xrs_rasterize_spans", *args, work.ptr, spans.ptr, c.value, ctypes.byref(ns), ctypes.byref(ni), None)
    assert 0 < ns.value <= c.value // 2 and ns.value <= ni.value <= ns.value * (cols // 64 + 2)
    plane = xs.DeviceArray(shape, np.uint32)
    _lib.call("xrs_rasterize_burn", rows, cols, spans.ptr, c.value, n_polys, ni.value, dev[3].ptr, count, plane.ptr, None)
    _lib.call("xrs_device_sync")
    _same(f"abi_plane_{'count' if count else 'winner'}", plane.get(), want_count if count else want_winner, op="rasterize_plane")
    # nothing to burn: the call clears the plane and reads no workspace
    _lib.call("xrs_rasterize_burn", rows, cols, None, 0, n_polys, 0, None, count, plane.ptr, None)
    _lib.call("xrs_device_sync")
    assert not plane.get().any()
    # refused before any launch
    assert lib.xrs_rasterize_spans(*args, work.ptr, spans.ptr, c.value + 1, ctypes.byref(ns), ctypes.byref(ni), None) != 0
    assert "not an even number" in _lib.last_error()
    assert lib.xrs_rasterize_census(dev[0].ptr, dev[1].ptr, dev[2].ptr, n_points, n_rings, n_polys, 2**17, 2**15, inv, work.ptr,
                                    ctypes.byref(c), ctypes.byref(flags), None) != 0
    assert "exceed the 32-bit cell index" in _lib.last_error()

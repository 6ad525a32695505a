"""polygonize on the MI355X: value for value against the reference's own outputs (tests/golden/polygonize_exec.npz, point
arrays bit for bit), against the restatement of DESIGN.md §6h (tests/polygonize_oracle.py) where the reference cannot be run
as plain Python (float32) or is slow (shapes that cross the 64 x 32 tile seams of csrc/polygonize.hip), and at the C ABI."""
import ctypes

import numpy as np
import pytest

from tests import polygonize_oracle as po
from tests.golden import make_polygonize_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = gen.case_names(FIXTURE)
KEYS = ("column", "points", "ring_offsets", "polygon_offsets")
SEAM_SHAPES = [(32, 64), (64, 32), (33, 65), (65, 33), (97, 129), (129, 97)]      # one tile exactly; just over; many tiles


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xs, a):
    return xs.DataArray(a, dims=["y", "x"])


def _flat(xs, a, mask=None, c=4, transform=None):
    return xs.polygonize(_agg(xs, a), mask=None if mask is None else _agg(xs, mask), connectivity=c, transform=transform,
                         return_type="flat")


def _same_flat(got, want):
    for k, g, w in zip(KEYS, got, want):
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert gen.same(g, w), k                                 # floats bit for bit


def _check_oracle(xs, a, mask=None, c=4, transform=None):
    _same_flat(_flat(xs, a, mask, c, transform), po.flat(a, mask, c == 8, transform))


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("case", CASES)
def test_equals_the_reference(xs, case, c):
    a, mask, transform = FIXTURE[f"{case}/in"], FIXTURE.get(f"{case}/mask"), FIXTURE.get(f"{case}/transform")
    _same_flat(_flat(xs, a, mask, c, transform), [FIXTURE[f"{case}/c{c}/{k}"] for k in KEYS])


def test_numpy_lists_are_the_flat_arrays_reassembled(xs):
    from xrspatial_amd.experimental.polygonize import assemble
    for case in ("ref_big_masked_float64", "nested_bridge", "transform_fma"):
        a, mask, transform = FIXTURE[f"{case}/in"], FIXTURE.get(f"{case}/mask"), FIXTURE.get(f"{case}/transform")
        kw = dict(mask=None if mask is None else _agg(xs, mask), connectivity=8, transform=transform)
        column, polygons = xs.polygonize(_agg(xs, a), **kw)
        flat = xs.polygonize(_agg(xs, a), return_type="flat", **kw)
        want_column, want_polygons = assemble(*flat)
        assert isinstance(column, list) and column == want_column and all(type(v) is a.dtype.type for v in column)
        assert len(polygons) == len(want_polygons)
        for p, q in zip(polygons, want_polygons):
            assert isinstance(p, list) and len(p) == len(q)
            for ring, want in zip(p, q):
                assert ring.dtype == np.float64 and ring.shape == want.shape and gen.same(ring, want)
        _same_flat(po.flatten(column, polygons, a.dtype), [FIXTURE[f"{case}/c8/{k}"] for k in KEYS])


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("shape", SEAM_SHAPES)
def test_float32_and_tile_seams_against_the_restatement(xs, shape, c):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + c)
    a = rng.integers(0, 3, shape).astype(np.float32)
    _check_oracle(xs, a, None, c)
    a[rng.random(shape) < 0.03] = np.nan
    _check_oracle(xs, a, rng.random(shape) < 0.9, c, gen.FMA_TRANSFORM)
    # large regions that cross the seams in both directions, with holes in them
    b = (rng.random(shape) < 0.85).astype(np.int16)
    _check_oracle(xs, b, None, c)
    # float32 near the tolerance: the threshold is float64 (the reference's Numba typing)
    base = np.float32(7470.702)
    t = np.float32(1e-05 * float(base) + 1e-08)
    f = (base + rng.integers(-2, 3, shape) * t * np.float32(rng.choice([0.5, 0.999, 1.0, 1.001]))).astype(np.float32)
    _check_oracle(xs, f, None, c)


@pytest.mark.parametrize("c", [4, 8])
def test_float32_follows_the_numba_typing(xs, c):
    from tests.test_regions_host import TYPING_PAIRS
    for v, w in list(TYPING_PAIRS) + [(7470.702, 7470.6274)]:
        for pair in ((v, w), (w, v)):
            _check_oracle(xs, np.array([pair], np.float32), None, c)
            a = np.full((34, 70), pair[0], np.float32)           # the pair at the seams (column 63 | 64, row 31 | 32)
            a[2, 63], a[31, 5], a[33, 64] = pair[1], pair[1], pair[1]
            _check_oracle(xs, a, None, c)


@pytest.mark.parametrize("c", [4, 8])
def test_threshold_is_multiply_then_add(xs, c):
    """pairs on which a fused multiply-add threshold would link what the reference keeps apart, or the reverse"""
    from tests import regions_oracle as ro
    for v, w in ro.fma_sensitive_pairs():
        for pair in ((v, w), (w, v)):
            _check_oracle(xs, np.array([pair]), None, c)
            _check_oracle(xs, np.array([pair]).T.copy(), None, c)


@pytest.mark.parametrize("c", [4, 8])
def test_one_ring_visits_every_tile(xs, c):
    a = gen.serpentine(129, 97).astype(np.float32)               # 5 x 2 tiles, one region through all of them
    got = _flat(xs, a, None, c)
    _same_flat(got, po.flat(a, None, c == 8))
    assert (got[0] == 1).sum() == 1
    b = gen.serpentine(131, 70).T.copy()                         # and column-wise
    _check_oracle(xs, b, None, c)
    _check_oracle(xs, gen.spiral(70, 130), None, c, gen.FMA_TRANSFORM)


def test_masks_of_every_kind(xs):
    rng = np.random.default_rng(8)
    a = rng.integers(0, 2, (40, 70)).astype(np.uint8)
    m = rng.random(a.shape) < 0.8
    want = po.flat(a, m, True)
    for dt in (np.bool_, np.int8, np.uint16, np.int64, np.float32, np.float64):
        mm = m.astype(dt)
        if np.dtype(dt).kind == "f":
            mm[m & (rng.random(a.shape) < 0.3)] = np.nan        # truth is != 0: NaN counts
            mm[m & (rng.random(a.shape) < 0.3)] = -0.5
        _same_flat(_flat(xs, a, mm, 8), want)
    empty = _flat(xs, a, np.zeros(a.shape, bool), 4)
    assert empty[0].shape == (0,) and empty[0].dtype == a.dtype and empty[1].shape == (0, 2)
    assert empty[2].tolist() == [0] and empty[3].tolist() == [0]
    assert xs.polygonize(_agg(xs, a), mask=_agg(xs, np.zeros(a.shape, bool))) == ([], [])


def test_device_arrays_in(xs):
    case = "ref_big_masked_int64"
    a, mask = FIXTURE[f"{case}/in"], FIXTURE[f"{case}/mask"]
    dev, mdev = xs.DeviceArray.from_numpy(a), xs.DeviceArray.from_numpy(mask)
    got = xs.polygonize(_agg(xs, dev), mask=_agg(xs, mdev), connectivity=8, return_type="flat")
    _same_flat(got, [FIXTURE[f"{case}/c8/{k}"] for k in KEYS])
    assert all(isinstance(g, np.ndarray) for g in got)
    with pytest.raises(TypeError, match="raster and mask have different underlying types"):
        xs.polygonize(_agg(xs, dev), mask=_agg(xs, mask))
    for dt in (np.float32, np.uint8):
        b = (a % 2).astype(dt)
        _same_flat(xs.polygonize(_agg(xs, xs.DeviceArray.from_numpy(b)), return_type="flat"), po.flat(b))


def test_two_runs_are_identical(xs):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 3, (150, 210)).astype(np.int32)
    for c in (4, 8):
        _same_flat(_flat(xs, a, None, c), _flat(xs, a, None, c))
        _check_oracle(xs, a, None, c)


def test_sharded_raster_is_refused(xs):
    sh = xs.ShardedArray(8, 8, np.float32)
    with pytest.raises(TypeError, match="Unsupported array type: .*ShardedArray"):
        xs.polygonize(xs.DataArray(sh, dims=["y", "x"]))


@pytest.mark.parametrize("c", [4, 8])
def test_abi_census_regions_and_state_count(xs, c):
    """the three calls at the C ABI: the region plane and the counts of the first, the ring table of the second"""
    from xrspatial_amd import _lib
    from xrspatial_amd.device import DTYPE_CODE
    lib = _lib.load()
    rng = np.random.default_rng(17 + c)
    a = rng.integers(0, 3, (70, 130)).astype(np.float64)
    a[rng.random(a.shape) < 0.02] = np.nan
    mask = (rng.random(a.shape) < 0.9).astype(np.float32)
    rows, cols = a.shape
    stats = {}
    want = po.flat(a, mask, c == 8, gen.FMA_TRANSFORM, stats=stats)
    want_regions, n_regions, _ = po.regions(a, mask, c == 8)
    dev, mdev = xs.DeviceArray.from_numpy(a), xs.DeviceArray.from_numpy(mask)
    work = xs.DeviceArray((lib.xrs_polygonize_workspace_bytes(rows, cols),), np.uint8)
    nr, ns = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.call("xrs_polygonize_census", dev.ptr, DTYPE_CODE[a.dtype], mdev.ptr, DTYPE_CODE[mask.dtype], rows, cols, c, work.ptr,
              ctypes.byref(nr), ctypes.byref(ns), None)
    assert nr.value == n_regions == stats["regions"] and ns.value == stats["states"]
    plane = xs.DeviceArray((rows, cols), np.uint32, _ptr=work.ptr, _base=work).get()     # the workspace's first words
    assert np.array_equal(plane, want_regions)
    rings = xs.DeviceArray((lib.xrs_polygonize_rings_workspace_bytes(ns.value),), np.uint8)
    n_rings, n_points = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rounds = (ctypes.c_int * 2)()
    _lib.call("xrs_polygonize_rings", rows, cols, work.ptr, rings.ptr, ns.value, nr.value, ctypes.byref(n_rings),
              ctypes.byref(n_points), rounds, None)
    assert n_rings.value == stats["rings"] == len(want[2]) - 1 and n_points.value == stats["points"] == len(want[1])
    assert 1 <= rounds[0] <= 32 and 1 <= rounds[1] <= 32
    points = xs.DeviceArray((n_points.value, 2), np.float64)
    ring_offsets = xs.DeviceArray((n_rings.value + 1,), np.int64)
    polygon_offsets = xs.DeviceArray((nr.value + 1,), np.int64)
    column = xs.DeviceArray((nr.value,), a.dtype)
    tf = (ctypes.c_double * 6)(*gen.FMA_TRANSFORM)
    _lib.call("xrs_polygonize_scatter", dev.ptr, DTYPE_CODE[a.dtype], rows, cols, work.ptr, rings.ptr, ns.value, nr.value,
              n_rings.value, tf, points.ptr, ring_offsets.ptr, polygon_offsets.ptr, column.ptr, None)
    _lib.call("xrs_device_sync")
    _same_flat((column.get(), points.get(), ring_offsets.get(), polygon_offsets.get()), want)

"""contours on the MI355X, bit for bit against the written rule (tests/contours_oracle.py): points, line offsets,
level offsets, closed flags and order.  Degenerate shapes, the seams of the 256-cell workgroups and 64-lane waves of
csrc/contours.hip, one long open and one long closed line (the doubling rounds), saddles, ties, nodata, the level axis, the ten
dtypes, both backends, the transform, contourpy's recorded lines, the rings burnt back by rasterize, and the calls at the C ABI.
Tolerance 0 throughout; every comparison records its count (tests/parity_log.py)."""
import ctypes

import numpy as np
import pytest

from tests import contours_oracle as co
from tests import parity_log
from tests.golden import make_contours_witness as wit
from tests.golden import make_polygonize_exec as gen

pytestmark = pytest.mark.gpu

DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float64, np.float32)   # XRS_DT_* 0 .. 9
WITNESS = wit.load()


@pytest.fixture(scope="module")
def xs():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xs, z):
    return xs.DataArray(z, dims=["y", "x"])


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_flat(config, got, want):
    """got: (levels, points, line_offsets, level_offsets, closed) of the product; want: the oracle's four arrays"""
    names = ("points", "line_offsets", "level_offsets", "closed")
    for name, g, w in zip(names, got[1:], want):
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, (config, name, g.dtype, g.shape, w.dtype, w.shape)
        parity_log.record(config, f"contours_{name}", g, w, tol=0)
        assert _bits(g) == _bits(w), (config, name, np.argwhere(np.atleast_1d(g != w))[:8].tolist())


def _check(xs, config, z, levels, transform=None, stats=None):
    from xrspatial_amd.contours import flat
    want = co.contours(z, levels, transform)
    got = flat(z, levels, transform, stats=stats)
    assert _bits(got[0]) == _bits(np.asarray(levels, np.float64))
    _same_flat(config, got, want)
    return want


def _field(seed, shape, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, shape).astype(dtype)


LEVELS3 = [-0.6, 0.05, 0.8]


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (2, 2), (2, 300)])
def test_degenerate_shapes(xs, shape):
    want = _check(xs, f"degenerate_{shape[0]}x{shape[1]}", _field(1, shape), LEVELS3)
    assert (len(want[0]) > 0) == (min(shape) >= 2)


@pytest.mark.parametrize("shape", [(3, 63), (4, 64), (5, 65), (6, 255), (7, 256), (3, 257), (300, 129)])
def test_block_and_wave_seams(xs, shape):
    z = _field(shape[0] * 1000 + shape[1], shape)
    want = _check(xs, f"seams_{shape[0]}x{shape[1]}", z, LEVELS3)
    assert len(want[3]) > 0
    z[np.random.default_rng(5).random(shape) < 0.05] = np.nan
    _check(xs, f"seams_nan_{shape[0]}x{shape[1]}", z, LEVELS3)


# ------------------------------------------------------------------ long lines
def test_one_long_open_line(xs):
    """a serpentine ridge: one open line of some thousand segments around it, so the doubling needs more than 8 rounds"""
    z = np.zeros((64, 65), np.float32)
    z[1:-1, 1:-1] = gen.serpentine(62, 63)
    z[1, 1] = np.nan                                       # the ridge's first cell: the ring around the ridge is cut open there
    stats = {}
    want = _check(xs, "serpentine_open", z, [0.5], stats=stats)
    lengths = np.diff(want[1])
    assert len(lengths) == 1 and lengths[0] > 2000 and not want[3][0]
    assert 8 < stats["leader_rounds"] <= 32 and 8 < stats["rank_rounds"] <= 32
    assert stats["segments"] == len(want[0]) - len(want[3]) and stats["lines"] == len(want[3])


def test_one_long_closed_line(xs):
    """a ring around a spiral: its smallest edge id is far from the segment the emit order begins with"""
    z = np.zeros((64, 65), np.float64)
    z[2:-2, 2:-2] = gen.spiral(60, 61)
    stats = {}
    want = _check(xs, "spiral_closed", z, [0.5], stats=stats)
    lengths = np.diff(want[1])
    assert want[3].all() and lengths.max() > 1000
    assert 8 < stats["leader_rounds"] <= 32
    # a ring whose first quad in raster order holds a later edge of it: the start is the smallest edge id, not the first segment
    ring = np.zeros((64, 65), np.float32)
    ring[10:50, 10:50] = 1.0
    ring[20:40, 20:40] = 0.0
    _check(xs, "ring_closed", ring, [0.25, 0.5], gen.FMA_TRANSFORM)


# ------------------------------------------------------------------ saddles and ties
@pytest.mark.parametrize("level", [0.25, 0.5, 0.75])
def test_checkerboard_saddles(xs, level):
    """centres at 0.5: low, exactly on the level (low) and high"""
    z = (np.indices((9, 70)).sum(axis=0) % 2).astype(np.float64)
    want = _check(xs, f"checkerboard_{level}", z, [level])
    assert len(want[3]) > 100
    both = _check(xs, "checkerboard_all", z, [0.25, 0.5, 0.75])
    assert np.diff(both[2]).min() > 0


def test_ties_are_kept(xs):
    rng = np.random.default_rng(11)
    z = rng.integers(0, 4, (40, 67)).astype(np.int16)      # nodes equal to the levels all over
    want = _check(xs, "ties_int", z, [0.0, 1.0, 2.0, 3.0])
    pts, off = want[0], want[1]
    seg = np.concatenate([np.all(pts[off[i]:off[i + 1] - 1] == pts[off[i] + 1:off[i + 1]], axis=1) for i in range(len(off) - 1)])
    assert seg.any()                                       # zero-length segments are in the result
    plateau = np.zeros((12, 70), np.float32)
    plateau[3:9, 5:60] = 1.0                               # a plateau equal to the level: low, like its surroundings below
    plateau[5:7, 20:30] = 2.0
    _check(xs, "plateau", plateau, [1.0])
    _check(xs, "plateau_under", plateau, [0.0, 1.0, 2.0])


# ------------------------------------------------------------------ nodata
def test_nodata(xs):
    z = _field(21, (50, 131), np.float64)
    holes = z.copy()
    holes[np.random.default_rng(3).random(z.shape) < 0.08] = np.nan
    want = _check(xs, "nan_holes", holes, LEVELS3)
    assert (want[3] == 0).any() and (want[3] == 1).any()
    infs = z.copy()
    infs[7, 9], infs[30, 100], infs[0, 0] = np.inf, -np.inf, np.inf
    _check(xs, "inf_corners", infs, LEVELS3)
    _check(xs, "inf_corners_f32", infs.astype(np.float32), LEVELS3)
    want = _check(xs, "all_nan", np.full((20, 70), np.nan, np.float32), LEVELS3)
    assert len(want[0]) == 0 and want[2].tolist() == [0, 0, 0, 0]
    none_whole = z.copy()
    none_whole[::2, ::2] = np.nan                          # every quad has a corner on the even grid
    want = _check(xs, "no_whole_quad", none_whole, LEVELS3)
    assert len(want[0]) == 0


# ------------------------------------------------------------------ levels
def test_level_axis(xs):
    z = _field(31, (37, 70))
    for k in (0, 1, 257):
        levels = np.linspace(-2.0, 2.0, k) if k != 1 else np.array([0.1])
        want = _check(xs, f"levels_{k}", z, levels)
        assert len(want[2]) == k + 1
    lo, hi = float(z.min()), float(z.max())
    for name, levels in (("below", [lo - 2.0, lo - 1.0]), ("above", [hi, hi + 1.0])):        # z > level: nothing at the maximum
        want = _check(xs, f"levels_{name}", z, levels)
        assert len(want[0]) == 0
    want = _check(xs, "levels_at_min", z, [lo - 1.0, lo])                                     # ... but the minimum is low, the rest high
    assert want[2].tolist()[1] == 0 and len(want[0]) > 0
    cliff = np.zeros((6, 9), np.float64)
    cliff[:, 5:] = 1000.0
    cliff[3, 5] = 500.0
    want = _check(xs, "cliff_257", cliff, np.linspace(1.0, 999.0, 257))
    assert np.diff(want[2]).min() >= 1


def test_bad_levels_raise(xs):
    agg = _agg(xs, _field(41, (8, 9)))
    for bad in ([0.5, 0.5], [1.0, 0.0], [np.nan], [0.0, np.inf], [-np.inf, 0.0]):
        with pytest.raises(ValueError):
            xs.contours(agg, bad)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int16, np.uint64])
def test_levels_by_count(xs, dtype):
    rng = np.random.default_rng(51)
    z = (rng.normal(0, 100, (33, 70))).astype(np.float64)
    if np.dtype(dtype).kind == "f":
        z[rng.random(z.shape) < 0.05] = np.nan
        z[3, 3], z[4, 4] = np.inf, -np.inf
    else:
        z = np.abs(z)
    z = z.astype(dtype)
    for n in (1, 7):
        want_levels = co.interior_levels(z, n)
        levels, points, line_offsets, level_offsets, closed = xs.contours(_agg(xs, z), n, return_type="flat")
        assert _bits(levels) == _bits(want_levels)
        _same_flat(f"by_count_{np.dtype(dtype).name}_{n}", (levels, points, line_offsets, level_offsets, closed),
                   co.contours(z, want_levels))
    with pytest.raises(ValueError):
        xs.contours(_agg(xs, np.full((5, 6), 3, dtype)), 4)               # a constant raster: the levels do not increase
    with pytest.raises(ValueError):
        xs.contours(_agg(xs, np.full((5, 6), 3, dtype)), 1)
    if np.dtype(dtype).kind == "f":
        with pytest.raises(ValueError):
            xs.contours(_agg(xs, np.full((5, 6), np.nan, dtype)), 3)      # no finite cell


# ------------------------------------------------------------------ dtypes, backends, transform
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_dtypes(xs, dtype):
    rng = np.random.default_rng(61)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        z = rng.normal(0, 40, (21, 67)).astype(dt)
    else:
        info = np.iinfo(dt)
        z = rng.integers(max(info.min, -100), min(info.max, 100) + 1, (21, 67)).astype(dt)
    _check(xs, f"dtype_{dt.name}", z, [-30.5, 0.0, 12.25, 64.0])
    if dt.itemsize == 8 and dt.kind in "iu":               # beyond 2^53 the conversion rounds, as astype(np.float64) does
        big = (np.uint64(np.iinfo(dt).max) - rng.integers(0, 1 << 12, (9, 66)).astype(np.uint64)).astype(dt)
        big[::3, ::2] = dt.type(2) ** 60
        f = big.astype(np.float64)
        levels = np.array([2.0 ** 61, float(np.nextafter(f.max(), 0.0))])
        want = _check(xs, f"dtype_{dt.name}_big", big, levels)
        assert len(want[0]) > 0


def test_device_backed_input_equals_numpy_input(xs):
    z = _field(71, (45, 130))
    z[5, 5] = np.nan
    a = xs.contours(_agg(xs, z), LEVELS3, return_type="flat")
    b = xs.contours(_agg(xs, xs.DeviceArray.from_numpy(z)), LEVELS3, return_type="flat")
    assert all(isinstance(v, np.ndarray) for v in b)
    assert [_bits(v) for v in a] == [_bits(v) for v in b]
    _same_flat("device_backed", b, co.contours(z, LEVELS3))


def test_transform_and_return_types(xs):
    z = _field(81, (40, 70), np.float64)
    z[10:12, 30] = np.nan
    want = _check(xs, "sheared", z, LEVELS3, gen.FMA_TRANSFORM)
    x, y = co.contours(z, LEVELS3)[0].T
    t = gen.FMA_TRANSFORM
    assert _bits(want[0][:, 0]) == _bits(t[0] * x + t[1] * y + t[2])        # the separately rounded products, left to right
    assert _bits(want[0][:, 1]) == _bits(t[3] * x + t[4] * y + t[5])
    levels, lines = xs.contours(_agg(xs, z), LEVELS3, transform=gen.FMA_TRANSFORM)
    flat = xs.contours(_agg(xs, z), LEVELS3, transform=np.array(gen.FMA_TRANSFORM), return_type="flat")
    assert _bits(levels) == _bits(flat[0]) and len(lines) == len(LEVELS3)
    want_lines = co.lines_of(want)
    for k in range(len(LEVELS3)):
        assert len(lines[k]) == len(want_lines[k]) > 0
        for a, b in zip(lines[k], want_lines[k]):
            assert a.shape == b.shape and _bits(a) == _bits(b)
    assert _bits(np.concatenate([ln for lv in lines for ln in lv])) == _bits(flat[1])


# ------------------------------------------------------------------ contourpy's lines, and the way back
@pytest.mark.parametrize("i", range(int(WITNESS["n_cases"])))
def test_witness_through_the_gpu(xs, i):
    z, levels = WITNESS[f"{i}/z"], WITNESS[f"{i}/levels"]
    got = xs.contours(_agg(xs, z), levels, return_type="flat")
    _same_flat(f"witness_{i}", got, co.contours(z, levels))
    ours, theirs = co.lines_of(got[1:]), wit.case_lines(WITNESS, i)
    tol = 4.0 * float(WITNESS["max_diff"])
    assert tol < 4e-12
    for k in range(len(levels)):
        assert len(ours[k]) == len(theirs[k])
        assert wit.match(theirs[k], ours[k], tol) is not None, (i, k)


@pytest.mark.parametrize("seed", range(6))
def test_burn_back_through_the_product(xs, seed):
    rng = np.random.default_rng(2000 + seed)
    H, W = (int(v) for v in rng.integers(20, 140, 2))
    z = rng.normal(0, 1, (H, W)).astype(np.float32)
    level = float(rng.uniform(-0.8, 0.8))
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = level - 1.5
    assert not np.any(z.astype(np.float64) == level)
    agg = _agg(xs, z)
    _, points, line_offsets, level_offsets, closed = xs.contours(agg, [level], return_type="flat")
    assert closed.all() and len(closed) > 0
    burnt = xs.rasterize((points, line_offsets, np.array([0, len(closed)], np.int64)), agg).data
    parity_log.record(f"burn_back_{seed}", "contours_rasterize", burnt != 0, z > level, tol=0)
    assert np.array_equal(burnt != 0, z > level)


# ------------------------------------------------------------------ the C ABI
def test_abi_refusals(xs):
    from xrspatial_amd import _lib
    lib = _lib.load()
    size = ctypes.c_uint64(0)
    n = ctypes.c_uint64(7)
    levels = (ctypes.c_double * 2)(0.25, 0.75)
    p = ctypes.c_void_p(256)                               # never dereferenced: every refusal comes before any launch

    def refused(rc, *words):
        assert rc != 0
        assert all(w in _lib.last_error() for w in words), _lib.last_error()

    refused(lib.xrs_contours_workspace_size(4, 5, 2, None), "null")
    refused(lib.xrs_contours_workspace_size(0, 5, 2, ctypes.byref(size)), "shape")
    refused(lib.xrs_contours_workspace_size(1 << 16, 1 << 15, 2, ctypes.byref(size)), "cells")
    refused(lib.xrs_contours_workspace_size(4, 5, (1 << 22) + 1, ctypes.byref(size)), "levels")
    refused(lib.xrs_contours_lines_workspace_size(0, ctypes.byref(size)), "0 segments")
    refused(lib.xrs_contours_lines_workspace_size((1 << 32) - 1, ctypes.byref(size)), "4294967295 segments")
    refused(lib.xrs_contours_lines_workspace_size(5, None), "null")
    refused(lib.xrs_contours_scatter_workspace_size(0, ctypes.byref(size)), "lines")
    assert lib.xrs_contours_lines_workspace_size((1 << 32) - 2, ctypes.byref(size)) == 0 and size.value > 40 * ((1 << 32) - 2)
    refused(lib.xrs_contours_census(None, 8, 4, 5, levels, 2, p, ctypes.byref(n), None), "null")
    refused(lib.xrs_contours_census(p, 8, 4, 5, levels, 2, None, ctypes.byref(n), None), "null")
    refused(lib.xrs_contours_census(p, 8, 4, 5, levels, 2, p, None, None), "null")
    refused(lib.xrs_contours_census(p, 8, 4, 5, None, 2, p, ctypes.byref(n), None), "null")
    refused(lib.xrs_contours_census(p, 77, 4, 5, levels, 2, p, ctypes.byref(n), None), "dtype")
    refused(lib.xrs_contours_census(p, 8, 4, 5, (ctypes.c_double * 2)(0.5, 0.5), 2, p, ctypes.byref(n), None), "strictly increasing")
    refused(lib.xrs_contours_census(p, 8, 4, 5, (ctypes.c_double * 2)(0.5, float("nan")), 2, p, ctypes.byref(n), None), "finite")
    nl, npts = ctypes.c_uint64(0), ctypes.c_uint64(0)
    refused(lib.xrs_contours_lines(p, 8, 4, 5, 2, p, p, (1 << 32) - 1, ctypes.byref(nl), ctypes.byref(npts), None, None),
            "4294967295 segments")
    refused(lib.xrs_contours_lines(p, 8, 4, 5, 2, p, p, 0, ctypes.byref(nl), ctypes.byref(npts), None, None), "0 segments")
    refused(lib.xrs_contours_lines(p, 8, 4, 5, 2, p, None, 6, ctypes.byref(nl), ctypes.byref(npts), None, None), "null")
    refused(lib.xrs_contours_lines(p, 8, 4, 5, 2, p, p, 6, None, ctypes.byref(npts), None, None), "null")
    refused(lib.xrs_contours_scatter(p, 8, 4, 5, 2, p, p, p, 6, 7, None, p, p, p, p, None), "7 lines")
    refused(lib.xrs_contours_scatter(p, 8, 4, 5, 2, p, p, p, 6, 2, None, None, p, p, p, None), "null")
    refused(lib.xrs_contours_scatter(p, 8, 4, 5, 2, p, p, None, 6, 2, None, p, p, p, p, None), "null")


def test_abi_census_without_a_crossing_and_the_three_calls(xs):
    from xrspatial_amd import _lib
    from xrspatial_amd.device import DTYPE_CODE
    z = _field(91, (23, 70), np.float64)
    z[4, 4] = np.nan
    rows, cols = z.shape
    dev = xs.DeviceArray.from_numpy(z)
    code = DTYPE_CODE[np.dtype(np.float64)]

    def census(levels):
        lv = (ctypes.c_double * len(levels))(*levels)
        work = xs.DeviceArray((_lib.workspace_bytes("contours", rows, cols, len(levels)),), np.uint8)
        n = ctypes.c_uint64(99)
        _lib.call("xrs_contours_census", dev.ptr, code, rows, cols, lv, len(levels), work.ptr, ctypes.byref(n), None)
        return work, n.value

    assert census([100.0, 200.0])[1] == 0                  # no crossing: 0, and no further call is needed
    assert census([])[1] == 0
    levels = [-0.5, 0.5]
    want = co.contours(z, levels, gen.FMA_TRANSFORM)
    work, n_segments = census(levels)
    assert n_segments == len(want[0]) - len(want[3])
    lines = xs.DeviceArray((_lib.workspace_bytes("contours_lines", n_segments + 1),), np.uint8)
    nl, npts = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rounds = (ctypes.c_int * 2)()
    # a segment count that is not the census's (one too many, in a block sized for it) is refused by the emit pass
    with pytest.raises(_lib.XrsError, match="do not match the census"):
        _lib.call("xrs_contours_lines", dev.ptr, code, rows, cols, 2, work.ptr, lines.ptr, n_segments + 1, ctypes.byref(nl),
                  ctypes.byref(npts), rounds, None)
    _lib.call("xrs_contours_lines", dev.ptr, code, rows, cols, 2, work.ptr, lines.ptr, n_segments, ctypes.byref(nl), ctypes.byref(npts),
              rounds, None)
    assert (nl.value, npts.value) == (len(want[3]), len(want[0])) and 0 < rounds[0] <= 32 and 0 < rounds[1] <= 32
    sort = xs.DeviceArray((_lib.workspace_bytes("contours_scatter", nl.value),), np.uint8)
    points = xs.DeviceArray((npts.value, 2), np.float64)
    line_offsets = xs.DeviceArray((nl.value + 1,), np.int64)
    level_offsets = xs.DeviceArray((3,), np.int64)
    closed = xs.DeviceArray((nl.value,), np.uint8)
    tf = (ctypes.c_double * 6)(*gen.FMA_TRANSFORM)
    _lib.call("xrs_contours_scatter", dev.ptr, code, rows, cols, 2, work.ptr, lines.ptr, sort.ptr, n_segments, nl.value, tf,
              points.ptr, line_offsets.ptr, level_offsets.ptr, closed.ptr, None)
    _lib.call("xrs_device_sync")
    _same_flat("abi_three_calls", (None, points.get(), line_offsets.get(), level_offsets.get(), closed.get()), want)

"""stream_order / stream_link / watershed / flow_length on the MI355X, through the public functions, against the rule in NumPy
(tests/streams_oracle.py).  Every output is a count, an id, an input value or the count rule of flow_length:
every comparison is `np.array_equal` on the values with equal NaN masks, no tolerance.  tests/test_streams_host.py pins the
oracle to hand-worked literals on the CPU.  A block of every doubling kernel takes 2048 cells (or stream cells).

Every comparison records its cell count (tests/parity_log.py)."""

import numpy as np
import pytest

from tests import hydrology_oracle as ho
from tests import parity_log
from tests import streams_oracle as so

pytestmark = pytest.mark.gpu

RAMP_LENGTHS = (1, 2, 3, 2048, 2049, 4097)
ACC_DTYPES = (np.float32, np.float64, np.int32, np.uint8, np.int64)


@pytest.fixture(scope="module")
def xa():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xa, z, res=(1.0, 1.0)):
    return xa.DataArray(z, dims=["y", "x"], attrs={"res": res})


def _equal(got, want, dtype, config, op):
    got = np.asarray(got)
    assert got.dtype == dtype and got.shape == want.shape, (config, op, got.dtype, got.shape)
    nan = np.isnan(want)
    differ = int(np.count_nonzero(got[~nan] != want[~nan])) + int(np.count_nonzero(np.isnan(got) != nan))
    note = f"{differ} of {want.size} cells not bit-equal"
    print(f"{config} {op}: {note}")
    parity_log.record(config, op, got, want, tol=0, note=note)
    assert np.array_equal(np.isnan(got), nan), (config, op, np.argwhere(np.isnan(got) != nan)[:10].tolist())
    assert np.array_equal(got[~nan], want[~nan].astype(dtype)), (config, op, note, np.argwhere((got != want) & ~nan)[:10].tolist())


def _streams(xa, d, acc, thr, config, want=None):
    """Both orders and the links of (d, acc, thr) against the oracle (or `want` = (strahler, shreve, link))."""
    want = want or (so.stream_order(d, acc, thr), so.stream_order(d, acc, thr, 'shreve'), so.stream_link(d, acc, thr))
    fd, fa = _agg(xa, d), _agg(xa, acc)
    _equal(xa.stream_order(fd, fa, thr).data, want[0], np.float64, config, "stream_order_strahler")
    _equal(xa.stream_order(fd, fa, thr, method='shreve').data, want[1], np.float64, config, "stream_order_shreve")
    _equal(xa.stream_link(fd, fa, thr).data, want[2], np.float64, config, "stream_link")


def _words(xa, d, acc, thr, want=7):
    """xrs_stream_network's status words for host rasters."""
    from xrspatial_amd import hydrology
    src = xa.DeviceArray.from_numpy(np.asarray(d, np.float32))
    return hydrology.stream_network(src, xa.DeviceArray.from_numpy(np.asarray(acc, np.float64)), thr, want)[-1]


def _length(xa, d, res, config):
    _equal(xa.flow_length(_agg(xa, d, res)).data, so.flow_length(d, *res), np.float64, config, "flow_length")


# ------------------------------------------------------------------ chains
@pytest.mark.parametrize("n", RAMP_LENGTHS)
def test_ramps_across_block_edges(xa, n):
    from xrspatial_amd import hydrology as hy
    for code in (1, 16):
        d = ho.ramp(n, code)
        one = np.ones((1, n))
        # one source, one link: the chain's upstream end is its only head
        _streams(xa, d, one, 1, f"streams_ramp_{code}_{n}", (one, one, one))
        steps = np.arange(n - 1, -1, -1, dtype=np.float64)[None, :]
        for res in ((1.0, 1.0), (2.0, 0.5)):
            want = (steps if code == 1 else steps[:, ::-1]) * res[0]
            _equal(xa.flow_length(_agg(xa, d, res)).data, want, np.float64, f"streams_ramp_{code}_{n}_res_{res[0]:g}", "flow_length")
        words = _words(xa, d, one, 1)
        rounds = (n - 1).bit_length()                                    # a path of n - 1 steps
        assert words[0] == rounds and words[hy.STREAM_HEAD_ROUNDS] == rounds and words[1] == 0
        assert (words[hy.STREAM_CELLS], words[hy.STREAM_SOURCES], words[hy.STREAM_HEADS], words[hy.STREAM_LEVELS]) == (n, 1, 1, 1)
        assert words[hy.STREAM_LIVE] == n - 1
        src = xa.DeviceArray.from_numpy(d)
        assert hy.length_plane(src, 1.0, 1.0, 2.0 ** 0.5)[1][0] == rounds
        assert hy.watershed_plane(src, xa.DeviceArray.from_numpy(np.zeros((1, n), np.uint8)), np.zeros(0), 0)[1][0] == rounds


def test_serpentine_depth_2144(xa):
    d = ho.serpentine(33, 65)
    one = np.ones(d.shape)
    _streams(xa, d, one, 1, "streams_serpentine_33x65", (one, one, one))
    _length(xa, d, (1.0, 1.0), "streams_serpentine_33x65")
    _length(xa, d, (2.0, 0.5), "streams_serpentine_33x65_res_2x0.5")
    assert np.asarray(xa.flow_length(_agg(xa, d)).data).max() == 2144
    assert _words(xa, d, one, 1)[0] == 12


# ------------------------------------------------------------------ comb, trees, junctions
def test_comb_stays_at_order_2_over_256_junctions(xa):
    from xrspatial_amd import hydrology as hy
    d = so.comb(65, 257)
    acc = so.ones_like_streams(d)
    _streams(xa, d, acc, 1, "streams_comb_65x257")
    strahler = np.asarray(xa.stream_order(_agg(xa, d), _agg(xa, acc), 1).data)
    assert (strahler[-1, 1:] == 2).all() and strahler.max() == 2
    shreve = np.asarray(xa.stream_order(_agg(xa, d), _agg(xa, acc), 1, method='shreve').data)
    assert np.array_equal(shreve[-1], np.arange(1, 258))
    words = _words(xa, d, acc, 1)
    assert (words[hy.STREAM_LEVELS], words[hy.STREAM_SOURCES], words[hy.STREAM_HEADS]) == (2, 257, 257 + 256)
    assert words[hy.STREAM_JOINTS + 1] == 256 and words[hy.STREAM_JOINTS + 2] == 0
    _length(xa, d, (3.0, 4.0), "streams_comb_65x257_res_3x4")


@pytest.mark.parametrize("order", range(1, 9))
def test_binary_trees_reach_their_order_in_as_many_levels(xa, order):
    from xrspatial_amd import hydrology as hy
    tree, outlet = so.binary_tree(order)
    d = so.padded(tree, 300)                                             # (from order 7 on the raster spans two blocks)
    acc = so.ones_like_streams(d)
    _streams(xa, d, acc, 1, f"streams_tree_{order}")
    fd, fa = _agg(xa, d), _agg(xa, acc)
    assert np.asarray(xa.stream_order(fd, fa, 1).data)[outlet] == order
    assert np.asarray(xa.stream_order(fd, fa, 1, method='shreve').data)[outlet] == 2 ** (order - 1)
    words = _words(xa, d, acc, 1)
    assert words[hy.STREAM_LEVELS] == order and words[hy.STREAM_SOURCES] == 2 ** (order - 1)
    assert [words[hy.STREAM_JOINTS + k] for k in range(1, order + 1)] == [2 ** (order - k) - 1 for k in range(1, order)] + [0]


@pytest.mark.parametrize("name", sorted(so.LITERALS))
def test_multi_child_junctions_tiled_across_a_block_boundary(xa, name):
    d, strahler, shreve, link = so.tiled(name, 400)                      # 3 .. 5 rows of 1600 .. 2400 columns: cell 2048 lies inside
    assert d.size > 2048 + d.shape[1]
    _streams(xa, d, so.ones_like_streams(d), 1, f"streams_tiled_{name}", (strahler, shreve, link))


# ------------------------------------------------------------------ dense ids, user accumulations
def test_dense_link_ids_across_blocks(xa):
    d = np.zeros((129, 257), np.float32)
    ids = np.arange(1, 129 * 257 + 1, dtype=np.float64).reshape(129, 257)
    one = np.ones(d.shape)
    _streams(xa, d, one, 1, "streams_all_zero_129x257", (one, one, ids))
    assert ids.max() == 33153
    acc = (np.random.default_rng(7).random(d.shape) >= 1 / 3).astype(np.float64)     # a random third of the cells off-stream
    _streams(xa, d, acc, 1, "streams_all_zero_129x257_two_thirds")


@pytest.mark.parametrize("dtype", ACC_DTYPES, ids=lambda d: np.dtype(d).name)
def test_user_accumulation_that_is_not_monotone(xa, dtype):
    d = ho.random_directions(129, 257, 5)
    rng = np.random.default_rng(np.dtype(dtype).itemsize + (np.dtype(dtype).kind == 'f'))
    acc = rng.integers(0, 6, d.shape).astype(dtype)
    if np.dtype(dtype).kind == 'f':
        acc[rng.random(d.shape) < 0.02] = np.nan
    for thr in (2, 3.5):
        _streams(xa, d, acc, thr, f"streams_random_{np.dtype(dtype).name}_thr_{thr}")
    _streams(xa, d, acc, np.inf, f"streams_random_{np.dtype(dtype).name}_thr_inf")      # no stream cell at all: every cell NaN


# ------------------------------------------------------------------ watershed
@pytest.fixture(scope="module")
def shed_case():
    """Random codes (cycles cut) with five pour points, two of them nested below others on the same path."""
    d = ho.random_directions(129, 257, 9)
    acc = ho.flow_accumulation(d)
    down, valid = ho.downstream(d)
    top = np.argsort(np.where(np.isnan(acc), -1, acc).ravel())[::-1]
    big = int(top[0])                                                    # the largest tree: its outlet-side cell,
    kids = np.flatnonzero(down == big)
    up1 = int(kids[np.argmax(acc.ravel()[kids])])                        # a cell right above it, and one further up: nested
    kids = np.flatnonzero(down == up1)
    up2 = int(kids[np.argmax(acc.ravel()[kids])]) if kids.size else int(top[1])
    points = [big, up1, up2]
    points += [int(t) for t in top[7:40] if int(t) not in points][:2]   # and two more large ones, wherever they lie
    assert len(set(points)) == 5
    return d, points


def test_watershed_five_pour_points_with_nested_ones(xa, shed_case):
    d, points = shed_case
    pour = np.zeros(d.shape, np.int32)
    pour.ravel()[points] = [11, 12, 13, 14, 15]
    want = so.watershed(d, pour)
    assert set(np.unique(want[~np.isnan(want)]).tolist()) == {11, 12, 13, 14, 15}
    _equal(xa.watershed(_agg(xa, d), _agg(xa, pour)).data, want, np.float32, "streams_shed_random_129x257", "watershed")
    pour.ravel()[::7] += 100                                             # other values all over: only the listed ones count
    _equal(xa.watershed(_agg(xa, d), _agg(xa, pour), target_values=[111, 112, 13, 113]).data, so.watershed(d, pour, [111, 112, 13, 113]),
           np.float32, "streams_shed_random_129x257", "watershed_target_values")


def test_watershed_labels_dtypes_and_corner_cases(xa, shed_case):
    d, points = shed_case
    big = np.zeros(d.shape, np.int64)
    big.ravel()[points] = [2 ** 24 + 1, 2 ** 24 + 3, 2 ** 40 + 1, -(2 ** 24) - 1, 5]
    want = so.watershed(d, big)
    assert np.float32(2 ** 24) in want and np.float32(2 ** 24 + 4) in want                 # float32 of the label: ties to even
    _equal(xa.watershed(_agg(xa, d), _agg(xa, big)).data, want, np.float32, "streams_shed_int64_labels", "watershed")
    for dtype in (np.bool_, np.float16, np.uint8, np.float64):
        pour = np.zeros(d.shape, dtype)
        pour.ravel()[points] = [1, 1, 1, 1, 1] if dtype == np.bool_ else [1, 2, 3, 4, 5]
        if np.dtype(dtype).kind == 'f':
            pour.ravel()[5::11] = np.nan                                 # NaN and inf are no pour points
            pour.ravel()[6::11] = np.inf
        _equal(xa.watershed(_agg(xa, d), _agg(xa, pour)).data, so.watershed(d, pour), np.float32,
               f"streams_shed_{np.dtype(dtype).name}", "watershed")
    none = np.zeros(d.shape, np.float32)
    _equal(xa.watershed(_agg(xa, d), _agg(xa, none)).data, np.full(d.shape, np.nan, np.float32), np.float32, "streams_shed_no_pour_point",
           "watershed")
    # a pour point at an outlet labels its whole basin; one on a NaN cell is none
    basin = ho.basins(d)
    outlet = int(basin[np.unravel_index(points[0], d.shape)])
    at = np.zeros(d.shape, np.float32)
    at.ravel()[outlet] = 3.5
    at[np.isnan(d)] = 8.0
    want = np.where(basin == outlet, np.float32(3.5), np.float32(np.nan)).astype(np.float32)
    _equal(xa.watershed(_agg(xa, d), _agg(xa, at)).data, want, np.float32, "streams_shed_outlet", "watershed")
    _equal(so.watershed(d, at), want, np.float32, "streams_shed_outlet", "watershed_oracle")


# ------------------------------------------------------------------ flow_length
def test_flow_length_random_directions_and_extreme_cell_sizes(xa):
    d = ho.random_directions(129, 257, 5)
    for res in ((1.0, 1.0), (2.0, 0.5), (1e-160, 1e-160), (1e150, 3e150)):
        _length(xa, d, res, f"streams_length_random_res_{res[0]:g}x{res[1]:g}")
    one = np.asarray(xa.flow_length(_agg(xa, d)).data)
    two = np.asarray(xa.flow_length(_agg(xa, d, (2.0, 0.5))).data)
    assert not np.array_equal(one, two, equal_nan=True)                  # the cell size is not ignored


# ------------------------------------------------------------------ errors and backends
def _calls(xa):
    one = lambda d: _agg(xa, np.ones(np.asarray(d.data).shape))          # noqa: E731
    return (lambda d: xa.stream_order(d, one(d), 1), lambda d: xa.stream_order(d, one(d), 1, method='shreve'),
            lambda d: xa.stream_link(d, one(d), 1), lambda d: xa.watershed(d, _agg(xa, np.zeros(np.asarray(d.data).shape))),
            xa.flow_length)


@pytest.mark.parametrize("name", ["two_cells", "four_cells", "300_cells"])
def test_cycles_raise(xa, name):
    d = {"two_cells": np.array([[0, 1, 16, 0]], np.float32), "four_cells": ho.ring(4, 5, 1, 1, 2, 2),
         "300_cells": ho.ring(80, 300, 3, 100, 70, 82)}[name]
    for fn in _calls(xa):
        with pytest.raises(ValueError, match="contains a cycle"):
            fn(_agg(xa, d))
    cut = ho.break_cycles(d)                                             # the same raster with the cycle cut is served
    _streams(xa, cut, np.ones(cut.shape), 1, f"streams_cut_cycle_{name}")
    _length(xa, cut, (1.0, 1.0), f"streams_cut_cycle_{name}")


def test_a_ring_of_stream_cells_with_tributaries_raises(xa):
    d = ho.ring(12, 40, 3, 10, 5, 6)
    d[2, 10:16] = 4.0                                                    # a source above every cell of the ring's top side
    d[8, 10:16] = 64.0                                                   # ... and below its bottom side: ring cells with two children
    acc = np.where(d != 0, 5.0, 0.0)
    for fn in (xa.stream_order, xa.stream_link):
        with pytest.raises(ValueError, match="contains a cycle"):
            fn(_agg(xa, d), _agg(xa, acc), 1)
    # a pour point on the ring cuts it; the ring off the streams touches nothing
    pour = np.zeros(d.shape, np.int16)
    pour[3, 10] = 4
    _equal(xa.watershed(_agg(xa, d), _agg(xa, pour)).data, so.watershed(d, pour), np.float32, "streams_ring_cut_by_pour_point", "watershed")
    off = np.where(d != 0, 0.0, 5.0)
    _streams(xa, d, off, 1, "streams_ring_off_the_streams", tuple(np.where(off > 0, v, np.nan) for v in (1.0, 1.0, np.cumsum(off > 0).reshape(d.shape))))


def test_invalid_codes_raise(xa):
    for bad in (3.0, -1.0, 0.5, 256.0, np.inf):
        d = np.zeros((5, 300), np.float32)
        d[3, 277] = bad
        for fn in _calls(xa):
            with pytest.raises(ValueError, match="D8 codes"):
                fn(_agg(xa, d))
    d = np.zeros((5, 300), np.float32)
    d[3, 277] = 3.0
    with pytest.raises(ValueError, match="D8 codes"):                    # ... also where the cell is no stream cell
        xa.stream_order(_agg(xa, d), _agg(xa, np.zeros(d.shape)), 1)


def test_device_arrays_mixed_backends_empty_rasters_and_dataset(xa):
    d, acc, thr = ho.random_directions(33, 70, 4), np.random.default_rng(1).integers(0, 4, (33, 70)).astype(np.float32), 2
    res = (2.0, 1.5)
    dev = lambda a: xa.DataArray(xa.DeviceArray.from_numpy(a), dims=["y", "x"], attrs={"res": res})      # noqa: E731
    host = lambda a: _agg(xa, a, res)                                    # noqa: E731
    pour = (acc == 3).astype(np.int32) * 6
    for fd, other, on_device in ((dev(d), dev(acc), True), (dev(d), host(acc), True), (host(d), dev(acc), False)):
        tag = f"streams_backend_{'dev' if on_device else 'host'}_{type(other.data).__name__}"
        got = xa.stream_order(fd, other, thr, name="so")
        assert isinstance(got.data, xa.DeviceArray) == on_device and got.name == "so" and got.attrs == {"res": res}
        assert tuple(got.dims) == ("y", "x")
        _equal(got.data.get() if on_device else got.data, so.stream_order(d, acc, thr), np.float64, tag, "stream_order_strahler")
        got = xa.stream_link(fd, other, thr)
        assert isinstance(got.data, xa.DeviceArray) == on_device
        _equal(got.data.get() if on_device else got.data, so.stream_link(d, acc, thr), np.float64, tag, "stream_link")
        shed = xa.watershed(fd, dev(pour) if isinstance(other.data, xa.DeviceArray) else host(pour))
        assert isinstance(shed.data, xa.DeviceArray) == on_device and shed.name == "watershed"
        _equal(shed.data.get() if on_device else shed.data, so.watershed(d, pour), np.float32, tag, "watershed")
    got = xa.flow_length(dev(d))
    assert isinstance(got.data, xa.DeviceArray) and got.attrs == {"res": res}
    _equal(got.data.get(), so.flow_length(d, *res), np.float64, "streams_backend_dev", "flow_length")
    d2 = ho.serpentine(5, 9)
    out = xa.flow_length(xa.Dataset({"a": host(d), "b": host(d2)}))
    _equal(out["a"].data, so.flow_length(d, *res), np.float64, "streams_dataset_a", "flow_length")
    _equal(out["b"].data, so.flow_length(d2, *res), np.float64, "streams_dataset_b", "flow_length")
    with xa.fuse():                                                      # eager inside a scope
        _equal(xa.flow_length(host(d)).data, so.flow_length(d, *res), np.float64, "streams_in_fuse_scope", "flow_length")
        _equal(xa.stream_order(host(d), host(acc), thr).data, so.stream_order(d, acc, thr), np.float64, "streams_in_fuse_scope",
               "stream_order_strahler")
    for shape in ((0, 7), (5, 0)):
        e = _agg(xa, np.zeros(shape, np.float32))
        for got, dtype in ((xa.stream_order(e, e), np.float64), (xa.stream_link(e, e), np.float64), (xa.watershed(e, e), np.float32),
                           (xa.flow_length(e), np.float64)):
            assert got.shape == shape and np.asarray(got.data).dtype == dtype


# ------------------------------------------------------------------ end to end
def test_end_to_end_on_generated_terrain(xa):
    terrain = xa.generate_terrain(xa.DataArray(np.zeros((257, 513), np.float32), dims=["y", "x"]))
    fd = xa.flow_direction(xa.fill(terrain), resolve_flats=True)
    fa = xa.flow_accumulation(fd)
    d, acc = np.asarray(fd.data), np.asarray(fa.data)
    res = terrain.attrs["res"]
    from xrspatial_amd import hydrology as hy
    for thr in (1, 50, 2000):
        _streams(xa, d, acc, thr, f"streams_terrain_257x513_thr_{thr}")
    words = _words(xa, d, acc, 50)
    strahler = so.stream_order(d, acc, 50)
    assert words[hy.STREAM_LEVELS] == np.nanmax(strahler) and words[hy.STREAM_CELLS] == np.count_nonzero(~np.isnan(strahler))
    pour = np.zeros(d.shape, np.int32)
    top = np.argsort(acc.ravel())[::-1][:5]
    pour.ravel()[top] = [1, 2, 3, 4, 5]
    _equal(xa.watershed(fd, _agg(xa, pour)).data, so.watershed(d, pour), np.float32, "streams_terrain_257x513", "watershed")
    _equal(xa.flow_length(fd).data, so.flow_length(d, *res), np.float64, "streams_terrain_257x513", "flow_length")


# ------------------------------------------------------------------ workspace
def test_workspace_sizes_restate_the_carve_layout(xa):
    from xrspatial_amd import _lib
    up = lambda v: (v + 255) // 256 * 256                                # noqa: E731
    head = up(4 * (33 * 64 * 64 + 2 * 64))                               # 33 rows of live counts, the invalid-code word, a pass's count
    for rows, cols in ((1, 1), (300, 400), (129, 257)):
        cells = rows * cols
        plane = up(4 * cells)
        assert _lib.workspace_bytes("flow_watershed", rows, cols) == head + 4 * plane          # two pointer planes, two root planes
        assert _lib.workspace_bytes("flow_length", rows, cols) == head + 8 * plane             # two pointer planes, 2 x 3 count planes
        net = _lib.workspace_bytes("stream_network", rows, cols)
        # the scanned marks and the head ids (cells + 1 words each), ten planes a stream cell, the child masks; then hipCUB's
        # block for a scan of cells + 1 words, whose size is hipCUB's to say: a multiple of 256 bytes, small against a plane
        fixed = head + 2 * up(4 * (cells + 1)) + 10 * plane + up(cells)
        assert fixed < net <= fixed + 65536 + cells // 16 and (net - fixed) % 256 == 0, (net, fixed)
    for name in ("stream_network", "flow_watershed", "flow_length"):
        for shape in ((0, 5), (5, 0), (1 << 16, 1 << 16), (1, (1 << 32) - 1)):
            assert _lib.workspace_bytes(name, *shape) == 0

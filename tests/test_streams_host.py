"""CPU checks of stream_order / stream_link / watershed / flow_length.  The reference has none of them, so there
is nothing to execute: the rule's NumPy statement (tests/streams_oracle.py) is pinned to small literals worked out by hand, the
kernels' level-set and count-doubling recurrences (as NumPy models) are held against Kahn's order and the cell-by-cell walk on
a few thousand random forests, and the argument checks and refusals run before any device work."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import hydrology_oracle as ho
from tests import streams_oracle as so

NAN = np.nan


def _agg(z, res=(1.0, 1.0), **kw):
    import xrspatial_amd as xa
    return xa.DataArray(z, dims=["y", "x"], attrs={"res": res}, **kw)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want, np.asarray(got).dtype)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), (got, want)


# ------------------------------------------------------------------ the stream graph on literals
@pytest.mark.parametrize("name", sorted(so.LITERALS))
def test_orders_and_links_of_the_hand_worked_junctions(name):
    d, strahler, shreve, link = so.literal(name)
    assert 3 <= min(d.shape) and max(d.shape) <= 5
    acc = so.ones_like_streams(d)
    got = so.stream_order(d, acc, 1, 'strahler')
    assert got.dtype == np.float64
    _same(got, strahler)
    _same(so.stream_order(d, acc, 1, 'shreve'), shreve)
    _same(so.stream_link(d, acc, 1), link)
    _same(so.levelset_model(d, acc, 1)[0], strahler)
    assert so.levelset_model(d, acc, 1)[1] == np.nanmax(strahler)


def test_the_literals_cover_the_child_orders_the_rule_names():
    found = set()
    for name in so.LITERALS:
        d, strahler, _, _ = so.literal(name)
        par, stream, nchild = so.stream_forest(d, so.ones_like_streams(d), 1)
        for v in np.flatnonzero(nchild >= 2):
            found.add(tuple(sorted((int(strahler.ravel()[u]) for u in np.flatnonzero(par == v)), reverse=True)))
    assert {(1, 1), (2, 1), (2, 2, 1), (2, 1, 1), (3, 2, 2)} <= found


def test_a_stream_that_ends_in_a_non_stream_cell_and_restarts_below_it():
    d = np.array([[1, 1, 1, 1, 0]], np.float32)
    acc = np.array([[5, 5, 1, 5, 5]], np.float64)                        # a user's accumulation need not grow downstream
    _same(so.stream_order(d, acc, 2), [[1, 1, NAN, 1, 1]])
    _same(so.stream_order(d, acc, 2, 'shreve'), [[1, 1, NAN, 1, 1]])
    _same(so.stream_link(d, acc, 2), [[1, 1, NAN, 2, 2]])


def test_threshold_edge_nan_accumulation_and_infinite_threshold():
    d = np.array([[1, 1, 1, 0]], np.float32)
    acc = np.array([[1, 2, NAN, 4]], np.float64)
    _same(so.stream_order(d, acc, 2), [[NAN, 1, NAN, 1]])                # exactly at the threshold: a stream cell
    _same(so.stream_order(d, acc, np.nextafter(2.0, 3.0)), [[NAN, NAN, NAN, 1]])
    _same(so.stream_link(d, acc, 2), [[NAN, 1, NAN, 2]])                 # the NaN accumulation cuts the stream
    for fn in (so.stream_order, so.stream_link):
        _same(fn(d, acc, np.inf), np.full((1, 4), NAN))
    _same(so.stream_order(d, np.array([[1, 2, 3, np.inf]]), np.inf), [[NAN, NAN, NAN, 1]])
    dn = np.array([[1, NAN, 0]], np.float32)
    _same(so.stream_order(dn, np.ones((1, 3)), 1), [[1, NAN, 1]])        # a NaN code is no stream cell, whatever its accumulation


def test_a_ring_of_stream_cells_raises_and_invalid_codes_raise():
    ring = ho.ring(4, 5, 1, 1, 2, 2)
    for fn in (so.stream_order, so.stream_link, lambda *a: so.levelset_model(*a)):
        with pytest.raises(ValueError, match="cycle"):
            fn(ring, np.ones(ring.shape), 1)
        with pytest.raises(ValueError, match="code"):
            fn(np.array([[1, 3, 0]], np.float32), np.ones((1, 3)), 1)
    for fn in (so.watershed, lambda d, p: so.flow_length(d), lambda d, p: so.count_doubling_model(d)):
        with pytest.raises(ValueError, match="cycle"):
            fn(ring, np.zeros(ring.shape))
        with pytest.raises(ValueError, match="code"):
            fn(np.array([[1, 3, 0]], np.float32), np.zeros((1, 3)))


# ------------------------------------------------------------------ watershed and flow_length on literals
def test_nested_pour_points_split_a_basin():
    d = np.array([[1, 1, 1, 1, 0], [64, 64, 0, 64, NAN]], np.float32)
    pour = np.array([[0, 7, 0, 0, 9], [0, 0, 3, 0, 5]], np.int32)       # 7 lies above 9 on the same path; 5 lies on a NaN cell
    got = so.watershed(d, pour)
    assert got.dtype == np.float32
    _same(got, [[7, 7, 9, 9, 9], [7, 7, 3, 9, NAN]])
    _same(so.watershed(d, pour, [9]), [[9, 9, 9, 9, 9], [9, 9, NAN, 9, NAN]])
    _same(so.watershed(d, np.zeros((2, 5))), [[NAN] * 5, [NAN] * 5])     # no pour point at all
    big = np.array([[0, 0, 0, 0, 2 ** 24 + 1], [0] * 5], np.int64)
    assert so.watershed(d, big)[0, 0] == np.float32(2 ** 24)             # float32 of the label, as cost_allocation


def test_flow_length_on_a_ramp_and_on_the_3_4_5_cell():
    _same(so.flow_length(np.array([[1, 1, 1, 1, 0]], np.float32), 2.0, 0.5), [[8, 6, 4, 2, 0]])
    _same(so.flow_length(np.array([[4], [4], [0]], np.float32), 2.0, 0.5), [[1.0], [0.5], [0]])
    _same(so.flow_length(np.array([[2, 4], [1, 0]], np.float32), 3.0, 4.0), [[5, 4], [3, 0]])
    # an outlet's own code is no step: the last cell points out of the raster, the first into NaN
    _same(so.flow_length(np.array([[16, NAN, 1, 1]], np.float32)), [[0, NAN, 1, 0]])
    # by counts: 3 diagonal steps are fl(3 * sqrt(2)), not sqrt(2) + sqrt(2) + sqrt(2)
    d = np.array([[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 2, 0], [0, 0, 0, 0]], np.float32)
    assert so.flow_length(d)[0, 0] == 3.0 * np.sqrt(2.0)


# ------------------------------------------------------------------ the kernels' recurrences against the rule
def test_level_set_model_equals_kahn_on_random_forests():
    checked = junctions = 0
    for seed in range(3000):
        d, acc, thr = so.random_forest(6, 7, seed)
        want = so.stream_order(d, acc, thr)
        got, levels = so.levelset_model(d, acc, thr)
        _same(got, want)
        assert levels == (0 if np.isnan(want).all() else np.nanmax(want))
        checked += 1
        junctions += int((so.stream_forest(d, acc, thr)[2] >= 2).sum())
    assert checked == 3000 and junctions > 3000


def test_level_set_model_on_trees_and_the_comb():
    for order in range(1, 9):
        d, outlet = so.binary_tree(order)
        assert d.shape == (order, 2 ** order - 1)
        acc = so.ones_like_streams(d)
        strahler = so.stream_order(d, acc, 1)
        assert strahler[outlet] == order and so.stream_order(d, acc, 1, 'shreve')[outlet] == 2 ** (order - 1)
        got, levels = so.levelset_model(d, acc, 1)
        _same(got, strahler)
        assert levels == order
    d = so.comb(65, 257)
    acc = so.ones_like_streams(d)
    strahler, shreve, link = so.stream_order(d, acc, 1), so.stream_order(d, acc, 1, 'shreve'), so.stream_link(d, acc, 1)
    assert (strahler[:-1] == 1).all() and strahler[-1, 0] == 1 and (strahler[-1, 1:] == 2).all()      # 2 over 256 junctions
    _same(shreve[-1], np.arange(1, 258))
    assert np.unique(link).size == 257 + 256                             # one link per tooth and per stem segment
    _same(so.levelset_model(d, acc, 1)[0], strahler)


def test_count_doubling_model_equals_the_walk():
    rasters = [so.random_forest(6, 7, seed)[0] for seed in range(300)]
    rasters += [ho.ramp(n, c) for n in (1, 2, 3, 9, 257) for c in (1, 16)] + [ho.serpentine(9, 7), ho.random_directions(40, 50, 3)]
    for d in rasters:
        counts, valid = so.step_counts(d)
        got, valid2, rounds = so.count_doubling_model(d)
        assert np.array_equal(valid, valid2) and np.array_equal(got[valid], counts[valid])
        assert rounds <= int(d.size).bit_length()
    d = ho.serpentine(33, 65)
    counts, _ = so.step_counts(d)
    assert counts.sum(axis=1).max() == 2144 and so.count_doubling_model(d)[2] == 12


def test_invariants_on_random_forests():
    for seed in range(200):
        d, acc, thr = so.random_forest(9, 11, seed)
        par, stream, nchild = so.stream_forest(d, acc, thr)
        strahler, shreve = so.stream_order(d, acc, thr).ravel(), so.stream_order(d, acc, thr, 'shreve').ravel()
        link = so.stream_link(d, acc, thr).ravel()
        heads = stream & (nchild != 1)
        assert np.unique(link[stream]).size == int(heads.sum())         # as many ids as heads, and dense:
        assert not stream.any() or (link[stream].min() == 1 and link[stream].max() == heads.sum())
        for lid in np.unique(link[stream]):
            assert np.unique(strahler[link == lid]).size == 1           # the order is constant along a link
        sources = stream & (nchild == 0)
        outlets = np.flatnonzero(stream & (par < 0))
        root = np.arange(par.size)
        for _ in range(par.size):
            root = np.where(par[root] >= 0, par[root], root)
        for o in outlets:                                                # Shreve at a stream outlet = the sources above it
            assert shreve[o] == int((sources & (root == o)).sum())


# ------------------------------------------------------------------ the package's host side
def test_the_new_names_are_exported():
    import xrspatial_amd as xa
    from xrspatial_amd import hydrology
    for name in ("stream_order", "stream_link", "watershed", "flow_length"):
        assert getattr(xa, name) is getattr(hydrology, name)
    assert (hydrology.STRAHLER, hydrology.SHREVE, hydrology.LINK) == (1, 2, 4)


def _two_raster_calls(xa):
    return ((lambda d, o: xa.stream_order(d, o, 1), "stream_order"), (lambda d, o: xa.stream_order(d, o, 1, 'shreve'), "stream_order"),
            (lambda d, o: xa.stream_link(d, o, 1), "stream_link"), (lambda d, o: xa.watershed(d, o), "watershed"))


def test_argument_checks_come_before_device_work():
    import xrspatial_amd as xa
    ok = _agg(np.zeros((3, 4), np.float32))
    cube = xa.DataArray(np.zeros((2, 3, 4), np.float32), dims=["b", "y", "x"])
    for fn, _ in _two_raster_calls(xa):
        for a, b in ((cube, ok), (ok, cube)):
            with pytest.raises(ValueError, match="2D"):
                fn(a, b)
        for a, b in ((_agg(np.zeros((3, 4), np.complex64)), ok), (ok, _agg(np.zeros((3, 4), np.complex64)))):
            with pytest.raises(TypeError, match="dtype"):
                fn(a, b)
        with pytest.raises(ValueError, match="differ in shape"):
            fn(ok, _agg(np.zeros((4, 3), np.float32)))
    with pytest.raises(ValueError, match="2D"):
        xa.flow_length(cube)
    with pytest.raises(TypeError, match="dtype"):
        xa.flow_length(_agg(np.zeros((3, 4), np.complex64)))
    with pytest.raises(ValueError, match="method"):
        xa.stream_order(ok, ok, 1, method='horton')
    for fn in (xa.stream_order, xa.stream_link):
        with pytest.raises(ValueError, match="threshold is NaN"):
            fn(ok, ok, threshold=NAN)
    for res in ((0.0, 1.0), (np.inf, 1.0), (1e-200, 1e-200)):
        with pytest.raises(ValueError, match="cell size"):
            xa.flow_length(_agg(np.zeros((3, 4), np.float32), res=res))


def test_dask_and_sharded_rasters_are_refused_before_the_other_checks(monkeypatch):
    import xrspatial_amd as xa
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.zeros((8, 8), np.float32), (4, 4)))
    shard = object.__new__(xa.ShardedArray)                              # (its constructor wants a device; the refusal does not)
    shard.local = np.zeros((8, 8), np.float32)
    other = _agg(np.zeros((3, 4), np.float32))                           # another shape: the refusal comes first
    for fn, _ in _two_raster_calls(xa):
        for a, b in ((lazy, other), (other, lazy)):
            with pytest.raises(NotImplementedError, match="dask"):
                fn(a, b)
        for a, b in ((_agg(shard), other), (other, _agg(shard))):
            with pytest.raises(NotImplementedError, match="sharded"):
                fn(a, b)
    with pytest.raises(NotImplementedError, match="dask"):
        xa.flow_length(lazy)
    with pytest.raises(NotImplementedError, match="sharded"):
        xa.flow_length(_agg(shard))


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xa
    if xa.has_hip():
        pytest.skip("a GPU is present")
    for dt in (np.float32, np.float64, np.int64, np.bool_):
        d, o = _agg(np.zeros((4, 4), np.float32)), _agg(np.zeros((4, 4), dt))
        for fn, _ in _two_raster_calls(xa):
            with pytest.raises(xa.XrsError):
                fn(d, o)
    with xa.fuse():                                                      # eager inside a scope: the same error, at the call
        with pytest.raises(xa.XrsError):
            xa.flow_length(_agg(np.zeros((4, 4), np.float32)))
    with pytest.raises(xa.XrsError):
        xa.flow_length(xa.Dataset({"a": _agg(np.zeros((4, 4), np.float32))}))


def test_abi_refuses_bad_arguments_before_device_work():
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    fake, other, third = ctypes.c_void_p(256), ctypes.c_void_p(512), ctypes.c_void_p(768)
    nan, inf = float("nan"), float("inf")
    for name in ("stream_network", "flow_watershed", "flow_length"):
        for shape in ((0, 5), (5, -1), (1 << 16, 1 << 16), (1, (1 << 32) - 1)):
            assert _lib.workspace_bytes(name, *shape) == 0, (name, shape)
        assert _lib.workspace_bytes(name, 1, (1 << 32) - 2) > 4 * ((1 << 32) - 2)

    status = (ctypes.c_int64 * 136)()

    def network(d=fake, acc=other, dtype=9, rows=4, cols=5, thr=1.0, want=7, work=third, o1=ctypes.c_void_p(1024), o2=ctypes.c_void_p(2048),
                o3=ctypes.c_void_p(4096), st=status, flags=0):
        return lib.xrs_stream_network(d, acc, dtype, rows, cols, thr, want, work, o1, o2, o3, st, flags, None)

    for kw, text in ((dict(rows=-1), "negative shape"), (dict(flags=2), "flags"), (dict(want=0), "want"), (dict(want=8), "want"),
                     (dict(dtype=4), "dtype"), (dict(dtype=10), "dtype"), (dict(thr=nan), "NaN"), (dict(st=None), "null"),
                     (dict(d=None), "null"), (dict(acc=None), "null"), (dict(work=None), "null"), (dict(o2=None), "null"),
                     (dict(o1=fake), "overwrite"), (dict(o3=other), "overwrite"), (dict(o2=ctypes.c_void_p(1024)), "share"),
                     (dict(rows=1 << 16, cols=1 << 16), "2^32 - 2")):
        assert network(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    status[0] = 7
    assert network(rows=0, d=None, work=None) == 0 and status[0] == 0   # nothing to do; the words are cleared
    assert network(want=1, o2=None, o3=None, rows=0) == 0                # a plane that `want` does not name may be null

    words = (ctypes.c_int64 * 80)()

    def shed(d=fake, pour=other, dtype=4, vals=None, kind=0, n=0, rows=4, cols=5, work=third, out=ctypes.c_void_p(1024), st=words, flags=0):
        return lib.xrs_flow_watershed(d, pour, dtype, vals, kind, n, rows, cols, work, out, st, flags, None)

    for kw, text in ((dict(cols=-1), "negative shape"), (dict(flags=2), "flags"), (dict(dtype=10), "dtype"), (dict(dtype=-1), "dtype"),
                     (dict(n=-1), "n_values"), (dict(kind=3), "values_kind"), (dict(st=None), "null"), (dict(d=None), "null"),
                     (dict(pour=None), "null"), (dict(work=None), "null"), (dict(out=None), "null"), (dict(n=2), "null"),
                     (dict(out=fake), "overwrite"), (dict(out=other), "overwrite"), (dict(rows=1, cols=(1 << 32) - 1), "2^32 - 2")):
        assert shed(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    words[0] = 7
    assert shed(rows=0) == 0 and words[0] == 0

    def length(d=fake, rows=4, cols=5, cx=1.0, cy=1.0, dg=2.0 ** 0.5, work=third, out=other, st=words, flags=0):
        return lib.xrs_flow_length(d, rows, cols, cx, cy, dg, work, out, st, flags, None)

    for kw, text in ((dict(rows=-1), "negative shape"), (dict(flags=4), "flags"), (dict(cx=0.0), "positive"), (dict(cy=-1.0), "positive"),
                     (dict(dg=nan), "positive"), (dict(cx=inf), "positive"), (dict(st=None), "null"), (dict(d=None), "null"),
                     (dict(work=None), "null"), (dict(out=None), "null"), (dict(out=fake), "overwrite"),
                     (dict(rows=1 << 16, cols=1 << 16), "2^32 - 2")):
        assert length(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    words[0] = 7
    assert length(cols=0) == 0 and words[0] == 0

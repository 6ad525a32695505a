"""CPU checks of a_star_search: the rule (tests/pathfinding_oracle.py) against the reference's own outputs
(tests/golden/astar_exec.npz), and the host side of the public function and of the C entry point, which all runs before any
device work.

What the rule owes the reference: the same answer to "is there a path", a path of exactly a + b + 1 cells (a
shortest one), the reference's image bit for bit where the shortest path is unique, and elsewhere the goal's cost within
2 (a + b) 2^-53 relative: both are sequential float64 sums of the same a ones and b sqrt(2)s, and each partial sum carries at
most one rounding."""
import ctypes
import importlib
import inspect
import json
import warnings

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import pathfinding_oracle as po
from tests.golden import make_astar_exec as gen

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)


def _agg(z, dims=("y", "x"), **kw):
    import xrspatial_amd as xa
    h, w = z.shape
    return xa.DataArray(z, dims=list(dims), coords={dims[0]: np.arange(h, dtype=np.float64), dims[1]: np.arange(w, dtype=np.float64)}, **kw)


@pytest.fixture(scope="module")
def oracle_runs():
    return {name: po.run(*gen.call_args(FIXTURE, name)) for name in CASES}


# ------------------------------------------------------------------ the rule against the executed reference
@pytest.mark.parametrize("case", CASES)
def test_rule_against_the_reference(oracle_runs, case):
    got, want = oracle_runs[case], FIXTURE[f"{case}/image"]
    img = got["image"]
    assert img.dtype == want.dtype == np.float64 and img.shape == want.shape
    assert got["found"] == (not np.isnan(want).all())                    # whether a path exists
    assert [got["warn_start"], got["warn_goal"]] == FIXTURE[f"{case}/warned"].tolist()
    if not got["found"]:
        assert np.isnan(img).all()
        return
    a, b = got["a"], got["b"]
    assert int((~np.isnan(want)).sum()) == a + b + 1 == int((~np.isnan(img)).sum())      # the reference's path is a shortest one
    goal = got["goal"]
    print(f"{case}: a = {a}, b = {b}, {got['n_paths']} shortest paths, goal {img[goal]!r} vs {want[goal]!r}")
    if got["n_paths"] == 1:
        assert np.array_equal(img.view(np.uint64), want.view(np.uint64))
    else:
        assert abs(img[goal] - want[goal]) <= 2 * (a + b) * 2.0 ** -53 * want[goal]


def test_enough_cases_have_exactly_one_shortest_path(oracle_runs):
    unique = [n for n in CASES if oracle_runs[n]["n_paths"] == 1]
    tied = [n for n in CASES if oracle_runs[n]["n_paths"] > 1]
    print(f"{len(unique)} cases with exactly one shortest path, {len(tied)} with several, {len(CASES) - len(unique) - len(tied)} without a path")
    assert len(unique) >= gen.MIN_UNIQUE and len(tied) >= 10
    assert sum(1 for n in unique if oracle_runs[n]["a"] + oracle_runs[n]["b"] >= 100) >= 5          # long ones among them


def test_fixture_covers_what_the_spec_lists(oracle_runs):
    shapes = [FIXTURE[f"{n}/z"].shape for n in CASES]
    assert max(max(s) for s in shapes) <= gen.MAX_SIDE
    want = np.array([[np.nan] * 4, [0.] + [np.nan] * 3, [np.nan, 1.4142135623730951, np.nan, np.nan],
                     [np.nan, np.nan, 2.8284271247461903, np.nan], [np.nan, 4.242640687119286, np.nan, np.nan]])
    assert np.array_equal(FIXTURE["doc_example/image"], want, equal_nan=True)            # as the reference's docstring prints it
    assert np.array_equal(FIXTURE["upstream_connectivity_4/image"][:4, 1], [1., 2., 3., 4.])         # its test module's results
    assert np.allclose(FIXTURE["upstream_connectivity_8/image"][1:4, 1], [1.41421356, 2.41421356, 3.41421356])
    for n in ("upstream_snap_none", "upstream_snap_start", "upstream_snap_goal", "snap_all_barriers", "snap_opposite_corner_start",
              "snap_opposite_corner_goal", "walled_off_goal_c4", "walled_off_goal_c8", "diagonal_wall_c4", "nan_wall_across"):
        assert np.isnan(FIXTURE[f"{n}/image"]).all(), n
    assert oracle_runs["snap_opposite_corner_start"]["start"] == (-1, -1) and not oracle_runs["snap_opposite_corner_start"]["warn_start"]
    assert oracle_runs["snap_next_to_opposite_corner"]["start"] == (5, 5) and oracle_runs["snap_next_to_opposite_corner"]["found"]
    assert oracle_runs["snap_all_barriers"]["warn_start"] and oracle_runs["snap_all_barriers"]["warn_goal"]
    assert oracle_runs["diagonal_wall_c8"]["found"]
    kinds = {FIXTURE[f"{n}/z"].dtype.name for n in CASES}
    assert {"int8", "int32", "int64", "uint8", "uint16", "uint32", "float32", "float64"} <= kinds
    assert {int(FIXTURE[f"{n}/args"][0]) for n in CASES} == {4, 8}
    z = FIXTURE["nan_inf_crossable_c8/z"]
    img = FIXTURE["nan_inf_crossable_c8/image"]
    assert np.isnan(z).any() and np.isposinf(z).any() and np.isneginf(z).any() and np.isinf(z[~np.isnan(img)]).any()   # crossed
    assert int(FIXTURE["int64_beyond_2_53_c8/barriers"][0]) == 2 ** 53 + 1 and oracle_runs["int64_beyond_2_53_c8"]["found"]
    assert oracle_runs["int64_beyond_2_53_other_value"]["a"] == 4 and oracle_runs["int64_beyond_2_53_other_value"]["b"] == 11
    assert FIXTURE["start_is_goal/image"][0, 0] == 0 and int((~np.isnan(FIXTURE["start_is_goal/image"])).sum()) == 1


def test_exact_comparison_of_distances():
    assert po.sign(0, 0) == 0 and po.sign(1, 0) == 1 and po.sign(0, -1) == -1 and po.sign(-3, 2) == -1 and po.sign(3, -2) == 1
    assert po.sign(-7, 5) == 1 and po.sign(7, -5) == -1                  # 7 < 5 sqrt(2) = 7.07...
    p, q = 1, 1
    for _ in range(35):                                                  # convergents of sqrt(2): p / q on alternating sides of it
        assert po.sign(p, -q) == (1 if p * p > 2 * q * q else -1)
        p, q = p + 2 * q, p + q
    assert p > 2 ** 40 and float(p) / float(q) == 2.0 ** 0.5             # (far beyond what float64 tells apart)


# ------------------------------------------------------------------ the host side of the public function
def test_exported_with_the_reference_signature():
    import xrspatial_amd as xa
    assert xa.a_star_search is importlib.import_module("xrspatial_amd.pathfinding").a_star_search
    params = inspect.signature(xa.a_star_search).parameters.values()
    got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else json.dumps(p.default)] for p in params]
    assert got == json.loads(str(FIXTURE["signature"]))


def test_pixel_ids():
    mod = importlib.import_module("xrspatial_amd.pathfinding")
    import xrspatial_amd as xa
    z = np.zeros((5, 4))
    agg = xa.DataArray(z, dims=["lat", "lon"], coords={"lat": np.linspace(4, 0, 5), "lon": np.linspace(0, 3, 4)})
    assert mod._get_pixel_id((3, 0), agg, "lon", "lat") == (1, 0) and mod._get_pixel_id((0, 1), agg, "lon", "lat") == (4, 1)
    assert mod._get_pixel_id((0.4, 2.9), agg) == (3, 2)                  # truncation, and the raster's own dims by default
    half = xa.DataArray(z, dims=["lat", "lon"], coords={"lat": np.linspace(2, 0, 5), "lon": np.linspace(0, 1.5, 4)}, attrs={"res": (0.5, 0.5)})
    assert mod._get_pixel_id((1.5, 1), half, "lon", "lat") == (1, 2) and mod._get_pixel_id((0, 0.5), half, "lon", "lat") == (4, 1)
    assert mod._get_pixel_id((9, 9), agg, "lon", "lat") == (5, 9)        # outside: for the caller to refuse


def test_argument_errors_of_the_reference():
    import xrspatial_amd as xa
    z = np.ones((5, 4), np.float32)
    with pytest.raises(ValueError, match="input `surface` must be 2D"):
        xa.a_star_search(xa.DataArray(np.ones((2, 3, 4)), dims=["b", "y", "x"]), (0, 0), (1, 1))
    with pytest.raises(ValueError, match=r"`surface.coords` should be named as coordinates:\(y, x\)"):
        xa.a_star_search(_agg(z, ("lat", "lon")), (0, 0), (1, 1))
    with pytest.raises(ValueError, match=r"should be named as coordinates:\(lat, lon\)"):
        xa.a_star_search(_agg(z), (0, 0), (1, 1), x="lon", y="lat")
    with pytest.raises(ValueError, match="should be named"):
        xa.a_star_search(_agg(z, ("x", "y")), (0, 0), (1, 1))
    for conn in (3, 6, 0):
        with pytest.raises(ValueError, match="Use either 4 or 8-connectivity."):
            xa.a_star_search(_agg(z), (0, 0), (1, 1), connectivity=conn)
    with pytest.raises(ValueError, match="start location outside the surface graph."):
        xa.a_star_search(_agg(z), (5, 0), (1, 1))
    with pytest.raises(ValueError, match="start location outside the surface graph."):
        xa.a_star_search(_agg(z), (0, 4), (1, 1))
    with pytest.raises(ValueError, match="goal location outside the surface graph."):
        xa.a_star_search(_agg(z), (0, 0), (1, 7))


def test_what_reaches_the_launch(monkeypatch):
    import xrspatial_amd as xa
    mod = importlib.import_module("xrspatial_amd.pathfinding")
    seen = {}

    def fake(data, start, goal, barriers, connectivity, snap_flags):
        seen.update(start=start, goal=goal, barriers=barriers, connectivity=connectivity, snap_flags=snap_flags)
        return np.full(data.shape, np.nan)

    monkeypatch.setattr(mod, "_run", fake)
    z = np.ones((5, 4), np.int16)
    agg = xa.DataArray(z, dims=["lat", "lon"], coords={"lat": np.linspace(4, 0, 5), "lon": np.linspace(0, 3, 4)}, attrs={"crs": 4326})
    out = xa.a_star_search(agg, (3, 0), (0, 1), [0, 2], "lon", "lat", 4, snap_goal=True)
    assert (seen["start"], seen["goal"], seen["connectivity"], seen["snap_flags"]) == ((1, 0), (4, 1), 4, mod.SNAP_GOAL)
    assert isinstance(seen["barriers"], np.ndarray) and seen["barriers"].tolist() == [0, 2]
    assert tuple(out.dims) == ("lat", "lon") and out.attrs == {"crs": 4326} and out.data.dtype == np.float64
    assert np.array_equal(np.asarray(out["lat"].data), np.linspace(4, 0, 5)) and np.array_equal(np.asarray(out["lon"].data), np.linspace(0, 3, 4))
    xa.a_star_search(agg, (3, 0), (0, 1), x="lon", y="lat", snap_start=True, snap_goal=True)
    assert seen["snap_flags"] == mod.SNAP_START | mod.SNAP_GOAL and seen["connectivity"] == 8 and seen["barriers"].size == 0


def test_dask_and_sharded_surfaces_are_refused(monkeypatch):
    import xrspatial_amd as xa
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = xa.DataArray(fake_dask.from_array(np.zeros((8, 8), np.float32), (4, 4)), dims=["y", "x"])
    with pytest.raises(NotImplementedError, match="dask"):
        xa.a_star_search(lazy, (0, 0), (1, 1))
    with pytest.raises(NotImplementedError, match="sharded"):
        shard = object.__new__(xa.ShardedArray)                          # (its constructor wants a device; the refusal does not)
        shard.local = np.zeros((8, 8), np.float32)                       # what its shape and dtype are read from
        xa.a_star_search(xa.DataArray(shard, dims=["y", "x"]), (0, 0), (1, 1))


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xa
    if xa.has_hip():
        pytest.skip("a GPU is present")
    for dt in (np.float32, np.int64, np.bool_):
        with pytest.raises(xa.XrsError):
            xa.a_star_search(_agg(np.ones((4, 4), dt)), (0, 0), (3, 3))


def test_abi_refuses_bad_arguments_before_device_work():
    """xrs_astar validates on the host side of the library: testable without a device"""
    entry.build()
    from xrspatial_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(256)
    status = (ctypes.c_int64 * 8)()
    up = lambda v: (v + 255) // 256 * 256                                # noqa: E731
    tiles = 10 * 7                                                       # 300 x 400 in tiles of 32 rows x 64 columns
    assert lib.xrs_astar_workspace_bytes(300, 400) == up(300 * 400 * 8) + 2 * up(tiles * 4) + 256 + 256 + 1024 * 32
    assert lib.xrs_astar_workspace_bytes(0, 5) == 0 and lib.xrs_astar_workspace_bytes(5, -1) == 0
    assert lib.xrs_astar_workspace_bytes(1 << 15, 1 << 15) > 0 and lib.xrs_astar_workspace_bytes(1 << 15, (1 << 15) + 1) == 0

    def call(data=fake, dtype=9, rows=4, cols=5, start=(0, 0), goal=(3, 4), barriers=None, kind=0, n=0, conn=8, snap=0, work=fake, out=fake,
             st=status):
        return lib.xrs_astar(data, dtype, rows, cols, start[0], start[1], goal[0], goal[1], barriers, kind, n, conn, snap, work, out, st, None)

    for kw, text in ((dict(data=None), "null"), (dict(work=None), "null"), (dict(out=None), "null"), (dict(st=None), "null"),
                     (dict(n=2), "null"), (dict(conn=3), "neither 4 nor 8"), (dict(conn=0), "neither 4 nor 8"),
                     (dict(start=(4, 0)), "start outside"), (dict(start=(0, 5)), "start outside"), (dict(start=(-1, 0)), "start outside"),
                     (dict(goal=(0, -1)), "goal outside"), (dict(goal=(4, 4)), "goal outside"), (dict(n=-1), "negative number"),
                     (dict(rows=-1), "negative shape"), (dict(dtype=10), "dtype"), (dict(kind=3), "kind"), (dict(kind=1, dtype=8), "float raster"),
                     (dict(snap=8), "snap_flags"), (dict(snap=65 << 8), "snap_flags"),
                     (dict(rows=1 << 15, cols=(1 << 15) + 1), "more than 2^30 cells"), (dict(rows=1 << 31, cols=1 << 31), "more than 2^30 cells"),
                     (dict(rows=0, cols=0), "start outside")):
        assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())


def test_warnings_follow_the_status_flags(monkeypatch):
    mod = importlib.import_module("xrspatial_amd.pathfinding")
    for flags, texts in ((3, []), (2, ["Start at a non crossable location"]), (1, ["End at a non crossable location"]),
                         (0, ["Start at a non crossable location", "End at a non crossable location"])):
        monkeypatch.setattr(mod, "search", lambda *a, flags=flags: ("image", [0, 0, 1, 1, flags, -1, -1, 1]))
        monkeypatch.setattr(mod, "finish", lambda out, like_numpy: out)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            assert mod._run(np.ones((2, 2)), (0, 0), (1, 1), np.array([]), 8, 0) == "image"
        assert [str(w.message) for w in caught] == texts

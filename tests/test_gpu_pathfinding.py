"""a_star_search on the MI355X, through the public function, against the rule (tests/pathfinding_oracle.py) and the reference's
own outputs (tests/golden/astar_exec.npz).

The device and the oracle follow the same rule with the same arithmetic -- exact integer distances and one float64 running sum
in walk order -- so the image is equal bit for bit at every cell, the warnings and the all-NaN cases included.  It follows that
the device equals the reference's image wherever the shortest path is unique (tests/test_pathfinding_host.py).

Every comparison records the number of cells that are not bit-equal (tests/parity_log.py).  Each call runs once."""
import importlib
import warnings

import numpy as np
import pytest

from tests import parity_log
from tests import pathfinding_oracle as po
from tests.golden import make_astar_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)
TILE_ROWS, TILE_COLS = 32, 64                    # one workgroup's tile (csrc/pathfinding.hip)
MESSAGES = ("Start at a non crossable location", "End at a non crossable location")


@pytest.fixture(scope="module")
def xa():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xa, z, **kw):
    h, w = z.shape
    return xa.DataArray(z, dims=["y", "x"], coords={"y": np.arange(h, dtype=np.float64), "x": np.arange(w, dtype=np.float64)},
                        attrs={"res": (1.0, 1.0), **kw})                 # (a one-row raster has no resolution of its own)


def _call(xa, agg, start, goal, barriers=(), connectivity=8, snap_start=False, snap_goal=False):
    """(result, [was the start warning issued, the goal warning])"""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = xa.a_star_search(agg, start, goal, barriers, connectivity=connectivity, snap_start=snap_start, snap_goal=snap_goal)
    texts = [str(w.message) for w in caught]
    assert set(texts) <= set(MESSAGES), texts
    return out, [m in texts for m in MESSAGES]


def _same(got, want, what):
    """bit for bit, recorded"""
    assert got.dtype == np.float64 and got.shape == want["image"].shape, what
    differ = int(np.count_nonzero(got.view(np.uint64) != want["image"].view(np.uint64)))
    note = f"{differ} of {got.size} cells not bit-equal; a = {want['a']}, b = {want['b']}, {want['n_paths']} shortest paths"
    print(f"{what}: {note}")
    parity_log.record(what, "a_star_search", got, want["image"], tol=0, note=note)
    assert differ == 0, (what, note, np.argwhere(got.view(np.uint64) != want["image"].view(np.uint64))[:10].tolist())


def _against_oracle(xa, z, start, goal, barriers=(), connectivity=8, snap_start=False, snap_goal=False, what=""):
    want = po.run(z, start, goal, barriers, connectivity, snap_start, snap_goal)
    out, warned = _call(xa, _agg(xa, z), start, goal, barriers, connectivity, snap_start, snap_goal)
    assert isinstance(out.data, np.ndarray), what
    _same(out.data, want, what)
    assert warned == [want["warn_start"], want["warn_goal"]], what
    return want


def _status(xa, z, start, goal, barriers, connectivity):
    """the status words of the same search, straight from the entry point"""
    mod = importlib.import_module("xrspatial_amd.pathfinding")
    return mod.search(z, start, goal, np.array(barriers), connectivity)[1]


def _passes(what, st):
    """the relaxation passes a call ran: recorded, and only ever held against the cap of rows * cols + 2"""
    note = f"{st[7]} passes for {st[5]} + {st[6]} steps"
    print(f"{what}: {note}")
    parity_log.record(what, "passes", [st[7]], [st[7]], note=note)


# ------------------------------------------------------------------ the fixture's cases
@pytest.mark.parametrize("case", CASES)
def test_equals_the_rule_and_the_reference(xa, case):
    z, start, goal, barriers, conn, ss, sg = gen.call_args(FIXTURE, case)
    before = z.copy()
    h, w = z.shape
    ys, xs = np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)
    agg = xa.DataArray(z, dims=["y", "x"], coords={"y": ys, "x": xs}, attrs={"crs": "EPSG:4326", "res": (1.0, 1.0)})
    out, warned = _call(xa, agg, start, goal, barriers, conn, ss, sg)
    assert isinstance(out.data, np.ndarray) and tuple(out.dims) == ("y", "x") and out.attrs == {"crs": "EPSG:4326", "res": (1.0, 1.0)}
    assert np.array_equal(np.asarray(out["x"].data), xs) and np.array_equal(np.asarray(out["y"].data), ys)
    assert agg.data is z and np.array_equal(z, before, equal_nan=z.dtype.kind == "f")    # the input is left alone
    want = po.run(z, start, goal, barriers, conn, ss, sg)
    _same(out.data, want, case)
    assert warned == [want["warn_start"], want["warn_goal"]] == FIXTURE[f"{case}/warned"].tolist()
    if want["n_paths"] <= 1:                                             # no path, or one shortest path: the reference's image
        assert np.array_equal(out.data.view(np.uint64), FIXTURE[f"{case}/image"].view(np.uint64))


# ------------------------------------------------------------------ tile geometry, against the rule
def _scatter(shape, seed, share=0.30, dtype=np.int32):
    rng = np.random.default_rng(seed)
    z = (rng.random(shape) >= share).astype(dtype)
    z[0, 0] = z[-1, -1] = z[0, -1] = z[-1, 0] = 1
    return z


# the first seed at which 30 % barriers leave all four corners 4-connected: a raster without a path compares NaN with NaN only
GEOMETRY_SEED = {(32, 64): 8, (31, 63): 4, (33, 65): 2, (65, 129): 7, (97, 193): 6}


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (2, 2), (TILE_ROWS, TILE_COLS), (TILE_ROWS - 1, TILE_COLS - 1),
                                   (TILE_ROWS + 1, TILE_COLS + 1), (2 * TILE_ROWS + 1, 2 * TILE_COLS + 1),
                                   (3 * TILE_ROWS + 1, 3 * TILE_COLS + 1)])
def test_tile_geometry(xa, shape, connectivity):
    h, w = shape
    z = _scatter(shape, GEOMETRY_SEED.get(shape, 1))
    if min(shape) == 1:
        z[:] = 1                                                         # (a line with a barrier in it has no path at all)
    what = f"astar_{h}x{w}_c{connectivity}"
    for start, goal, tag in (((0, 0), (h - 1, w - 1), ""), ((h - 1, 0), (0, w - 1), "_other_corners")):
        want = _against_oracle(xa, z, start, goal, [0], connectivity, what=what + tag)
        assert want["found"], (what, tag)


def _serpentine(h, w):
    z = np.ones((h, w), np.uint8)
    for k, r in enumerate(range(1, h, 2)):
        z[r, :] = 0
        z[r, -1 if k % 2 == 0 else 0] = 1
    return z


def _spiral(n):
    """a one-cell corridor from the corner (0, 0) inwards; walls and corridor one cell wide each"""
    z = np.zeros((n, n), np.uint8)
    r, c, dr, dc = 0, 0, 0, 1
    z[0, 0] = 1
    last = (0, 0)
    while True:
        moved = False
        while True:
            nr, nc = r + dr, c + dc
            ar, ac = nr + dr, nc + dc                                    # the cell after the next one must not be corridor already
            if not (0 <= nr < n and 0 <= nc < n) or z[nr, nc] or (0 <= ar < n and 0 <= ac < n and z[ar, ac]):
                break
            side = [(nr + dc, nc + dr), (nr - dc, nc - dr)]              # nor may the next one touch an earlier turn of the spiral
            if any(0 <= y < n and 0 <= x < n and z[y, x] and (y, x) != (r, c) for y, x in side):
                break
            r, c = nr, nc
            z[r, c] = 1
            last = (r, c)
            moved = True
        if not moved:
            return z, last
        dr, dc = dc, -dr                                                 # turn right


@pytest.mark.parametrize("connectivity", [4, 8])
def test_serpentine_needs_many_passes(xa, connectivity):
    z = _serpentine(96, 130)
    start, goal = (0, 0), (94, 0)
    want = _against_oracle(xa, z, start, goal, [0], connectivity, what=f"astar_serpentine_96x130_c{connectivity}")
    assert want["found"] and want["a"] + want["b"] > 5500 and (connectivity == 8 or want["n_paths"] == 1)
    st = _status(xa, z, start, goal, [0], connectivity)
    _passes(f"astar_serpentine_96x130_c{connectivity}", st)
    assert (st[5], st[6]) == (want["a"], want["b"]) and st[4] == 7 and st[7] < z.size + 2


@pytest.mark.parametrize("connectivity", [4, 8])
def test_spiral(xa, connectivity):
    z, centre = _spiral(70)
    assert int(z.sum()) > 1000
    want = _against_oracle(xa, z, centre, (0, 0), [0], connectivity, what=f"astar_spiral_70_c{connectivity}")
    assert want["found"] and want["a"] + want["b"] > 1000
    st = _status(xa, z, centre, (0, 0), [0], connectivity)
    _passes(f"astar_spiral_70_c{connectivity}", st)
    assert (st[5], st[6]) == (want["a"], want["b"]) and st[7] < z.size + 2


@pytest.mark.parametrize("connectivity", [4, 8])
def test_random_raster_with_nan_cells(xa, connectivity):
    rng = np.random.default_rng(5)
    z = rng.integers(0, 4, (257, 300)).astype(np.float32)                # value 0: barriers, a quarter of the cells
    z[rng.random(z.shape) < 0.08] = np.nan
    z[3, 2] = z[250, 290] = 1
    want = _against_oracle(xa, z, (3, 2), (250, 290), [0], connectivity, what=f"astar_random_257x300_c{connectivity}")
    assert want["found"] and want["n_paths"] > 1


def test_two_calls_are_bit_equal(xa):
    z = _scatter((97, 193), 23, 0.25, np.float64)
    agg = _agg(xa, z)
    first, _ = _call(xa, agg, (0, 0), (96, 192), [0])
    second, _ = _call(xa, agg, (0, 0), (96, 192), [0])
    assert not np.isnan(first.data).all()
    assert np.array_equal(first.data.view(np.uint64), second.data.view(np.uint64))


def test_walled_off_goal_returns_all_nan(xa):
    z = np.ones((65, 129), np.float32)
    z[40:50, 100] = z[40:50, 110] = z[40, 100:111] = z[49, 100:111] = 0
    for connectivity in (4, 8):
        want = _against_oracle(xa, z, (0, 0), (45, 105), [0], connectivity, what=f"astar_walled_off_65x129_c{connectivity}")
        assert not want["found"] and not want["warn_start"] and not want["warn_goal"]
        st = _status(xa, z, (0, 0), (45, 105), [0], connectivity)
        assert st[4] == 3 and (st[5], st[6]) == (-1, -1) and st[:4] == [0, 0, 45, 105] and st[7] < z.size + 2


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float64, np.float32,
                                   np.bool_, np.float16])
def test_every_dtype(xa, dtype):
    z = _scatter((33, 70), 3, 0.3).astype(dtype)
    barriers = [False] if dtype == np.bool_ else [0]
    _against_oracle(xa, z, (0, 0), (32, 69), barriers, 8, what=f"astar_dtype_{np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [np.float32, np.int64, np.bool_])
def test_device_array_in_device_array_out(xa, dtype):
    z = _scatter((37, 83), 9, 0.3).astype(dtype)
    z[20, 40] = 0
    dev_in = xa.DeviceArray.from_numpy(z)
    args = dict(barriers=[0], connectivity=8, snap_start=True, snap_goal=False)
    res, warned = _call(xa, _agg(xa, dev_in, k=1), (20, 40), (36, 82), **args)
    assert isinstance(res.data, xa.DeviceArray) and res.data.dtype == np.float64 and res.attrs == {"res": (1.0, 1.0), "k": 1}
    assert dev_in.dtype == np.dtype(dtype) and np.array_equal(dev_in.get(), z)           # the input is left alone
    host, warned_host = _call(xa, _agg(xa, z), (20, 40), (36, 82), **args)
    assert warned == warned_host == [False, False]
    assert np.array_equal(res.data.get().view(np.uint64), host.data.view(np.uint64))
    _same(res.data.get(), po.run(z, (20, 40), (36, 82), [0], 8, True, False), f"astar_device_{np.dtype(dtype).name}")


def test_snap_across_tiles(xa):
    """the nearest crossable cell lies in another tile and another block of the reduction; equidistant ones: the first wins"""
    z = np.zeros((70, 200), np.int32)
    z[20, 170] = z[40, 150] = z[40, 190] = z[60, 170] = 1                # (40, 170) is 20 cells away from all four
    z[61:66, 150] = z[65, 150:160] = 1
    want = _against_oracle(xa, z, (40, 170), (69, 140), [0], 8, True, True, what="astar_snap_across_tiles")
    assert want["start"] == (20, 170) and want["goal"] == (65, 150) and not want["found"]
    want = _against_oracle(xa, z, (67, 158), (69, 140), [0], 4, True, True, what="astar_snap_across_tiles_path")
    assert want["start"] == (65, 158) and want["goal"] == (65, 150) and want["found"] and want["a"] == 8

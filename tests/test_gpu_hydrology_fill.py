"""fill and flow_direction(resolve_flats=True) on the MI355X, through the public functions, against the rules in NumPy
(tests/hydrology_fill_oracle.py).  Every output value is an input value or an integer code: every comparison is
value-equal with equal NaN masks, tolerance 0.  The relaxer's tile edge is T = 64 (`hydrology.TILE`); the shapes are (T - 1)^2,
T^2, (T + 1)^2, (2T + 1) x (T + 2), 1 x 1, 1 x 65, 65 x 1, 2 x 2 and 3 x 3, and the featured rasters are built around the tile
borders.  tests/test_hydrology_fill_host.py shows on the CPU that the oracle's formulations agree on these rasters and that every
path of the filled and resolved rasters drains.

Every comparison records its cell count (tests/parity_log.py)."""
import numpy as np
import pytest

from tests import hydrology_fill_oracle as fo
from tests import hydrology_oracle as ho
from tests import parity_log

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
CASE_NAMES = tuple(fo.cases(np.float32))


@pytest.fixture(scope="module")
def xa():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    assert xrspatial_amd.hydrology.TILE == fo.TILE
    return xrspatial_amd


def _agg(xa, z, res=(1.0, 1.0)):
    return xa.DataArray(z, dims=["y", "x"], attrs={"res": res})


def _equal(got, want, dtype, config, op):
    got = np.asarray(got)
    assert got.dtype == dtype and got.shape == want.shape, (config, op, got.dtype, got.shape)
    nan = np.isnan(want)
    differ = int(np.count_nonzero(got[~nan] != want[~nan])) + int(np.count_nonzero(np.isnan(got) != nan))
    note = f"{differ} of {want.size} cells not value-equal"
    print(f"{config} {op}: {note}")
    parity_log.record(config, op, got, want, tol=0, note=note)
    assert np.array_equal(np.isnan(got), nan), (config, op, np.argwhere(np.isnan(got) != nan)[:10].tolist())
    assert np.array_equal(got[~nan], want[~nan].astype(dtype)), (config, op, note, np.argwhere((got != want) & ~nan)[:10].tolist())


# ------------------------------------------------------------------ every shared raster, both dtypes
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_fill_and_resolved_directions(xa, name, dtype):
    z, want_fill, want_dir, want_dir_filled = fo.expected(name, dtype)
    config = f"hydrofill_{name}_{np.dtype(dtype).name}"
    _equal(xa.fill(_agg(xa, z)).data, want_fill, np.dtype(dtype), config, "fill")
    _equal(xa.flow_direction(_agg(xa, z), resolve_flats=True).data, want_dir, np.float32, config, "flow_direction_flats")
    _equal(xa.flow_direction(_agg(xa, want_fill), resolve_flats=True).data, want_dir_filled, np.float32, config + "_filled",
           "flow_direction_flats")


def test_the_literals_of_the_featured_rasters(xa):
    w = np.asarray(xa.fill(_agg(xa, fo.lake_four_tiles(np.float32))).data)
    assert w[1:-1, 1:-1].min() == 7 == w[1:-1, 1:-1].max()                 # the whole bed stands at the far spill cell's level
    w = np.asarray(xa.fill(_agg(xa, fo.diagonal_pits(np.float32))).data)
    assert w[fo.TILE - 1, fo.TILE - 1] == 3 == w[fo.TILE, fo.TILE]         # A spills through B, across the tile corner
    z = fo.lake_with_nan_hole(np.float64)
    w = np.asarray(xa.fill(_agg(xa, z)).data)
    assert np.array_equal(w[69:74, 29:35][~np.isnan(z[69:74, 29:35])], z[69:74, 29:35][~np.isnan(z[69:74, 29:35])])   # rim of the hole
    assert w[1:-1, 1:-1][~np.isnan(w[1:-1, 1:-1])].max() <= 5             # nothing rises to the wall


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_serpentine_takes_many_rounds(xa, dtype):
    """The status words of the two entry points: the level (and then the step count) crosses tile borders one or two a round."""
    from xrspatial_amd import hydrology
    z, length = fo.serpentine_corridor(dtype)
    assert length > 2 * fo.TILE * fo.TILE and z.shape[0] >= 2 * fo.TILE and z.shape[1] >= 2 * fo.TILE
    src = xa.DeviceArray.from_numpy(z)
    out, words = hydrology.fill_plane(src)
    xa.synchronize()
    info = hydrology.relax_rounds(words)
    print("fill rounds", info["rounds"], "tiles", info["tiles_launched"], info["changed"][:10], info["tiles"][:10])
    assert info["rounds"] > 3 and all(c > 0 for c in info["changed"][:3])   # more than one round moved cells
    assert info["rounds"] > hydrology.FILL_STATUS_ROUNDS or info["changed"][-1] == 0       # the last round moved none
    assert info["tiles"][0] == 9 and min(info["tiles"][1:]) < 9           # round 0 launches every tile, later rounds only some
    want = fo.expected("serpentine_corridor", dtype)
    _equal(out.get(), want[1], np.dtype(dtype), f"hydrofill_serpentine_abi_{np.dtype(dtype).name}", "fill")
    assert int((want[1] == 0).sum()) == length                             # all of the corridor stands at the mouth's level
    filled = xa.DeviceArray.from_numpy(np.array(want[1]))
    codes = xa.flow_direction(_agg(xa, filled)).data
    words = hydrology.resolve_flats_plane(filled, codes)
    xa.synchronize()
    info = hydrology.relax_rounds(words)
    print("flats rounds", info["rounds"], "tiles", info["tiles_launched"], info["changed"][:10], info["tiles"][:10])
    assert info["rounds"] > 3 and all(c > 0 for c in info["changed"][:3])
    _equal(codes.get(), want[3], np.float32, f"hydrofill_serpentine_abi_{np.dtype(dtype).name}", "flow_direction_flats")


def test_int16_raster(xa):
    z = np.random.default_rng(3).integers(0, 4, (67, 259)).astype(np.int16)
    _equal(xa.fill(_agg(xa, z)).data, fo.fill(z), np.float64, "hydrofill_int16_67x259", "fill")
    _equal(xa.flow_direction(_agg(xa, z), resolve_flats=True).data, fo.resolve_flats(z)[0], np.float32, "hydrofill_int16_67x259",
           "flow_direction_flats")
    _equal(xa.flow_direction(_agg(xa, z, (3.0, 4.0)), resolve_flats=True).data, fo.resolve_flats(z, 3.0, 4.0)[0], np.float32,
           "hydrofill_int16_67x259_res_3x4", "flow_direction_flats")


def test_device_array_dataset_fuse_scope_and_empty_rasters(xa):
    z32, _, _, _ = fo.expected("featured_129x257", np.float32)
    z64 = ho.random_terrain(33, 70, 4, np.float64)
    res = (2.0, 1.5)
    got = xa.fill(_agg(xa, xa.DeviceArray.from_numpy(np.array(z32)), res), name="filled")
    assert isinstance(got.data, xa.DeviceArray) and got.name == "filled" and got.attrs == {"res": res} and tuple(got.dims) == ("y", "x")
    _equal(got.data.get(), fo.fill(z32), np.float32, "hydrofill_device_array", "fill")
    d = xa.flow_direction(got, resolve_flats=True)                       # stays in HBM through the next stage
    assert isinstance(d.data, xa.DeviceArray) and d.attrs == {"res": res}
    _equal(d.data.get(), fo.resolve_flats(fo.fill(z32), *res)[0], np.float32, "hydrofill_device_array", "flow_direction_flats")
    ds = xa.Dataset({"a": _agg(xa, np.array(z32), res), "b": _agg(xa, z64, res)})
    out = xa.fill(ds)
    _equal(out["a"].data, fo.fill(z32), np.float32, "hydrofill_dataset_a", "fill")
    _equal(out["b"].data, fo.fill(z64), np.float64, "hydrofill_dataset_b", "fill")
    out = xa.flow_direction(ds, resolve_flats=True)
    _equal(out["b"].data, fo.resolve_flats(z64, *res)[0], np.float32, "hydrofill_dataset_b", "flow_direction_flats")
    with xa.fuse():                                                      # eager inside a scope
        _equal(xa.fill(_agg(xa, z64, res)).data, fo.fill(z64), np.float64, "hydrofill_in_fuse_scope", "fill")
        _equal(xa.flow_direction(_agg(xa, z64, res), resolve_flats=True).data, fo.resolve_flats(z64, *res)[0], np.float32,
               "hydrofill_in_fuse_scope", "flow_direction_flats")
    for shape in ((0, 7), (5, 0), (0, 0)):
        for dt, want in ((np.float32, np.float32), (np.float64, np.float64), (np.int32, np.float64)):
            got = xa.fill(_agg(xa, np.zeros(shape, dt)))
            assert got.shape == shape and got.dtype == want
            assert xa.flow_direction(_agg(xa, np.zeros(shape, dt)), resolve_flats=True).shape == shape


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_resolve_flats_false_is_the_plain_direction(xa, dtype):
    z = fo.featured_terrain(dtype)
    plain = np.asarray(xa.flow_direction(_agg(xa, z)).data)
    _equal(xa.flow_direction(_agg(xa, z), resolve_flats=False).data, plain, np.float32, f"hydrofill_plain_{np.dtype(dtype).name}",
           "flow_direction")
    _equal(plain, ho.flow_direction(z), np.float32, f"hydrofill_plain_{np.dtype(dtype).name}", "flow_direction")
    resolved = np.asarray(xa.flow_direction(_agg(xa, z), resolve_flats=True).data)
    drained = fo.drained_mask(z, plain)
    assert np.array_equal(resolved[drained], plain[drained]) and (resolved != plain).sum() > 0     # only flat cells change


def test_end_to_end_on_generated_terrain(xa):
    terrain = xa.generate_terrain(xa.DataArray(np.zeros((257, 513), np.float32), dims=["y", "x"]))
    z = np.asarray(terrain.data)
    res = terrain.attrs["res"]
    want_fill = fo.fill(z)
    filled = xa.fill(terrain)
    _equal(filled.data, want_fill, np.float32, "hydrofill_terrain_257x513", "fill")
    want_dir = fo.resolve_flats(want_fill, *res)[0]
    got_dir = xa.flow_direction(filled, resolve_flats=True)
    _equal(got_dir.data, want_dir, np.float32, "hydrofill_terrain_257x513", "flow_direction_flats")
    want_acc, want_bas = ho.flow_accumulation(want_dir), ho.basins(want_dir)
    acc = np.asarray(xa.flow_accumulation(got_dir).data)                 # raises nothing: no cycle
    bas = np.asarray(xa.basins(got_dir).data)
    _equal(acc, want_acc, np.float64, "hydrofill_terrain_257x513", "flow_accumulation")
    _equal(bas, want_bas, np.float64, "hydrofill_terrain_257x513", "basins")
    rim = fo.rim_mask(z)
    outlets = np.unique(bas).astype(np.int64)
    assert rim.ravel()[outlets].all()                                    # every outlet is a rim cell
    assert acc.ravel()[outlets].sum() == z.size                          # every cell arrives at one
    assert (np.asarray(got_dir.data)[~rim] != 0).all()
    plain = ho.flow_accumulation(ho.flow_direction(z, *res))
    print(f"257 x 513 terrain: largest accumulation {acc.max():.0f} (unfilled: {plain.max():.0f}), {outlets.size} outlets")
    assert acc.max() > plain.max()

"""cost_distance, cost_backlink and cost_allocation on the MI355X, through the public functions, against the rule in NumPy
(tests/cost_distance_oracle.py: a heap Dijkstra).  The distance field is the unique fixed point of a written
float64 rule, the links and the allocation follow from it by comparisons: every comparison is value-equal with equal NaN masks,
tolerance 0.  The relaxer's tile edge is T = 64; the random fields have the shapes (T - 1)^2, T^2, (T + 1)^2, (2T + 1) x (T + 2),
1 x 1, 1 x 65, 65 x 1, 2 x 2 and 3 x 3, and the featured rasters are built around the tile borders.
tests/test_cost_distance_host.py shows on the CPU that the oracle's formulations agree and what the featured rasters hold.

Every comparison records its cell count (tests/parity_log.py)."""
import importlib

import numpy as np
import pytest

from tests import cost_distance_oracle as co
from tests import parity_log

pytestmark = pytest.mark.gpu

PRODUCTS = ("cost_distance", "cost_backlink", "cost_allocation")


@pytest.fixture(scope="module")
def xa():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    assert xrspatial_amd.hydrology.TILE == co.TILE
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


def _call(xa, product, case, raster=None, friction=None):
    raster = case["raster"] if raster is None else raster
    friction = case["friction"] if friction is None else friction
    return getattr(xa, product)(_agg(xa, raster, case["res"]), _agg(xa, friction, case["res"]), target_values=case["target_values"],
                                max_cost=case["max_cost"], connectivity=case["connectivity"])


def _all_three(xa, case, want, config):
    """The three public functions and basins of the links against a solved case; returns the links."""
    _equal(_call(xa, "cost_distance", case).data, want["distance"], np.float64, config, "cost_distance")
    links = _call(xa, "cost_backlink", case)
    _equal(links.data, want["backlink"], np.float32, config, "cost_backlink")
    _equal(_call(xa, "cost_allocation", case).data, want["allocation"], np.float32, config, "cost_allocation")
    _equal(xa.basins(links).data, want["index"], np.float64, config, "cost_backlink_basins")
    return links


# ------------------------------------------------------------------ every shared raster
@pytest.mark.parametrize("name", [n for n in co.CASES if n != "absorbed_row"])
def test_the_three_products(xa, name):
    links = _all_three(xa, co.CASES[name], co.expected(name), f"cost_{name}")
    assert links.name == "cost_backlink" and tuple(links.dims) == ("y", "x") and links.attrs == {"res": co.CASES[name]["res"]}


def test_the_absorbed_row_raises_from_links_and_allocation_only(xa):
    case, want = co.CASES["absorbed_row"], co.expected("absorbed_row")
    _equal(_call(xa, "cost_distance", case).data, want["distance"], np.float64, "cost_absorbed_row", "cost_distance")
    for product in ("cost_backlink", "cost_allocation"):
        with pytest.raises(ValueError, match="2 reached cells"):
            _call(xa, product, case)


def test_the_literals_of_the_featured_rasters(xa):
    case = co.CASES["diagonal_gap_c8"]
    d = np.asarray(_call(xa, "cost_distance", case).data)
    assert d[64, 64] == d[63, 63] + np.sqrt(np.float64(2.0)) and np.isfinite(d[64:, 64:]).all()        # in through the tile corner
    assert np.isnan(np.asarray(_call(xa, "cost_distance", co.CASES["diagonal_gap_c4"]).data)[64:, 64:]).all()
    case = co.CASES["two_sources_across_edge"]
    assert np.asarray(_call(xa, "cost_allocation", case).data)[2, 62:66].tolist() == [7, 7, 9, 9]       # E before W at column 64
    case = co.CASES["max_cost_cuts_a_tile"]
    d = np.asarray(_call(xa, "cost_distance", case).data)
    assert np.nanmax(d) <= case["max_cost"] and 0.2 < np.isnan(d).mean() < 0.8
    for product in PRODUCTS:
        assert np.isnan(np.asarray(_call(xa, product, co.CASES["no_source"]).data)).all()


def test_the_serpentine_takes_many_rounds(xa):
    """The status words: the cost crosses tile borders a few a round; later rounds launch only the tiles beside a change."""
    from xrspatial_amd import hydrology
    cd = importlib.import_module("xrspatial_amd.cost_distance")
    case, want = co.CASES["serpentine_impassable_walls"], co.expected("serpentine_impassable_walls")
    assert want["longest"] > 2 * co.TILE * co.TILE and case["raster"].shape == (2 * co.TILE + 3,) * 2
    src, fr = xa.DeviceArray.from_numpy(case["raster"]), xa.DeviceArray.from_numpy(case["friction"])
    dist, link, words = cd.cost_planes(src, fr, np.zeros(0), 0, 1.0, 1.0, float(np.sqrt(2.0)))
    xa.synchronize()
    info = hydrology.relax_rounds(words)
    print("rounds", info["rounds"], "tiles", info["tiles_launched"], info["changed"][:10], info["tiles"][:10], words[4:7])
    assert info["rounds"] > 3 and all(c > 0 for c in info["changed"][:3])   # more than one round moved cells
    assert info["rounds"] > hydrology.FILL_STATUS_ROUNDS or info["changed"][-1] == 0       # the last round moved none
    assert info["tiles"][0] == 9 and min(info["tiles"][1:]) < 9           # round 0 launches every tile, later rounds only some
    assert words[cd.SOURCES] == 1 and words[cd.ABSORBED] == 0 and words[cd.REACHED] == int(np.isfinite(want["distance"]).sum())
    _equal(dist.get(), want["distance"], np.float64, "cost_serpentine_abi", "cost_distance")
    _equal(link.get(), want["backlink"], np.float32, "cost_serpentine_abi", "cost_backlink")
    _equal(cd.allocation_plane(src, link).get(), want["allocation"], np.float32, "cost_serpentine_abi", "cost_allocation")
    timed = cd.cost_planes(src, fr, np.zeros(0), 0, 1.0, 1.0, float(np.sqrt(2.0)), backlink=False, flags=cd.TIMED)[2]
    assert timed[:2] == words[:2] and timed[2] > 0 and timed[3] > 0 and all(ns > 0 for ns in hydrology.relax_rounds(timed)["ns"])


def test_device_arrays_stay_resident_and_backends_mix(xa):
    name = "random_uniform_float32_65x65_c8"
    case, want = co.CASES[name], co.expected(name)
    raster, friction = xa.DeviceArray.from_numpy(case["raster"]), xa.DeviceArray.from_numpy(case["friction"])
    for product, key, dtype in zip(PRODUCTS, ("distance", "backlink", "allocation"), (np.float64, np.float32, np.float32)):
        got = _call(xa, product, case, raster, friction)
        assert isinstance(got.data, xa.DeviceArray) and got.name == product
        _equal(got.data.get(), want[key], dtype, "cost_device_array", product)
        got = _call(xa, product, case, raster, None)                     # the result has the raster's backend
        assert isinstance(got.data, xa.DeviceArray)
        _equal(got.data.get(), want[key], dtype, "cost_device_raster_host_friction", product)
        got = _call(xa, product, case, None, friction)
        assert isinstance(got.data, np.ndarray)
        _equal(got.data, want[key], dtype, "cost_host_raster_device_friction", product)
    assert _call(xa, "cost_distance", case).data.dtype == np.float64 and xa.cost_distance(
        _agg(xa, case["raster"]), _agg(xa, case["friction"]), name="minutes").name == "minutes"


def test_bool_and_float16_rasters_and_unsigned_friction(xa):
    rng = np.random.default_rng(41)
    friction = rng.integers(0, 4, (66, 67)).astype(np.uint8)              # 0: impassable
    for raster in ((rng.random((66, 67)) < 0.002), (rng.random((66, 67)) < 0.002).astype(np.float16) * 3):
        case = dict(raster=raster, friction=friction, res=(1.0, 1.0), target_values=[], max_cost=np.inf, connectivity=8)
        want = co.solve(case)
        assert want["absorbed"] == 0 and np.isfinite(want["distance"]).sum() > 1000
        _all_three(xa, case, want, f"cost_{raster.dtype.name}_raster_uint8_friction")


def test_empty_rasters(xa):
    for shape in ((0, 7), (5, 0), (0, 0)):
        for product, dtype in zip(PRODUCTS, (np.float64, np.float32, np.float32)):
            got = getattr(xa, product)(_agg(xa, np.zeros(shape, np.int32)), _agg(xa, np.zeros(shape, np.float32)))
            assert got.shape == shape and got.dtype == dtype


def test_end_to_end_on_generated_terrain(xa):
    terrain = xa.generate_terrain(xa.DataArray(np.zeros((257, 513), np.float32), dims=["y", "x"]))
    friction = (1.0 + np.asarray(xa.slope(terrain).data)).astype(np.float32)     # NaN on the raster's edge: impassable there
    rng = np.random.default_rng(43)
    raster = np.zeros(friction.shape, np.int32)
    raster[rng.integers(1, 256, 6), rng.integers(1, 512, 6)] = np.arange(1, 7)
    case = dict(raster=raster, friction=friction, res=terrain.attrs["res"], target_values=[], max_cost=np.inf, connectivity=8)
    want = co.solve(case)
    assert want["absorbed"] == 0 and np.isfinite(want["distance"][1:-1, 1:-1]).all() and np.isnan(want["distance"][0]).all()
    links = _all_three(xa, case, want, "cost_terrain_257x513")
    acc = np.asarray(xa.flow_accumulation(links).data)                   # a D8 raster like any other: every reached cell arrives at a source
    assert acc[raster != 0].sum() == np.isfinite(want["distance"]).sum()
    print(f"257 x 513 terrain: largest cost {np.nanmax(want['distance']):.1f}, longest chain {want['longest']} links, "
          f"{np.unique(want['allocation'][~np.isnan(want['allocation'])]).size} sources own cells")

"""flow_direction / flow_accumulation / basins on the MI355X, through the public functions, against the rule in NumPy
(tests/hydrology_oracle.py).  Every output is an integer code, a count or an index: every comparison is
`np.array_equal` on the values with equal NaN masks, no tolerance.  tests/test_hydrology_host.py shows on the CPU that the
direction rasters used here reach the round counts they are meant to (ramps: every count up to 11, serpentine: 12, fan: 8).

Every comparison records its cell count (tests/parity_log.py)."""
import numpy as np
import pytest

from tests import hydrology_oracle as ho
from tests import parity_log

pytestmark = pytest.mark.gpu

RAMP_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 1025)
DTYPES = (np.float32, np.float64)


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


def _direction(xa, z, res, config):
    got = xa.flow_direction(_agg(xa, z, res))
    _equal(got.data, ho.flow_direction(z, *res), np.float32, config, "flow_direction")
    return got


def _graph(xa, d, config, want=None):
    """flow_accumulation and basins of the direction raster `d` against the oracle (or `want`, computed once by the caller)."""
    want = want or (ho.flow_accumulation(d), ho.basins(d))
    agg = _agg(xa, d)
    _equal(xa.flow_accumulation(agg).data, want[0], np.float64, config, "flow_accumulation")
    _equal(xa.basins(agg).data, want[1], np.float64, config, "basins")


# ------------------------------------------------------------------ direction
def _featured_terrain(dtype):
    z = ho.random_terrain(129, 257, 1, dtype)
    z[40:47, 100:131] = np.nan                                           # a NaN block
    z[80:95, 20:60] = 512.0                                              # a plateau
    z[10, 10], z[100, 200] = np.inf, -np.inf
    return z


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_direction_random_terrain_with_nan_plateau_and_infinities(xa, dtype):
    _direction(xa, _featured_terrain(dtype), (1.0, 1.0), f"hydro_featured_129x257_{np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (65, 1), (2, 2), (63, 64), (64, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_direction_block_and_row_edges(xa, shape, dtype):
    _direction(xa, ho.random_terrain(*shape, seed=shape[0] + shape[1], dtype=dtype), (1.0, 1.0),
               f"hydro_edges_{shape[0]}x{shape[1]}_{np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_direction_anisotropic_cells(xa, dtype):
    z = ho.random_terrain(129, 257, 2, dtype)
    got = _direction(xa, z, (0.5, 3.0), f"hydro_res_0.5x3_{np.dtype(dtype).name}")
    assert not np.array_equal(np.asarray(got.data), ho.flow_direction(z, 1.0, 1.0))      # the cell size is not ignored


def test_direction_int16_raster_with_exact_ties(xa):
    z = np.random.default_rng(3).integers(0, 4, (67, 259)).astype(np.int16)
    _direction(xa, z, (1.0, 1.0), "hydro_int16_ties_67x259")
    _direction(xa, z, (3.0, 4.0), "hydro_int16_ties_67x259_res_3x4")     # diagonal exactly 5: ties across the three distances


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_direction_cone(xa, dtype):
    z = (-ho.pit_cone(65, 131)).astype(dtype)                            # a peak: every cell flows outwards
    _direction(xa, z, (1.0, 1.0), f"hydro_peak_cone_65x131_{np.dtype(dtype).name}")


def test_direction_device_array_and_dataset(xa):
    z32, z64 = _featured_terrain(np.float32), ho.random_terrain(33, 70, 4, np.float64)
    res = (2.0, 1.5)
    got = xa.flow_direction(_agg(xa, xa.DeviceArray.from_numpy(z32), res), name="fd")
    assert isinstance(got.data, xa.DeviceArray) and got.name == "fd" and got.attrs == {"res": res} and tuple(got.dims) == ("y", "x")
    _equal(got.data.get(), ho.flow_direction(z32, *res), np.float32, "hydro_device_array", "flow_direction")
    acc = xa.flow_accumulation(got)                                      # stays in HBM through the next stage
    assert isinstance(acc.data, xa.DeviceArray) and acc.attrs == {"res": res}
    _equal(acc.data.get(), ho.flow_accumulation(ho.flow_direction(z32, *res)), np.float64, "hydro_device_array", "flow_accumulation")
    ds = xa.Dataset({"a": _agg(xa, z32, res), "b": _agg(xa, z64, res)})
    out = xa.flow_direction(ds)
    _equal(out["a"].data, ho.flow_direction(z32, *res), np.float32, "hydro_dataset_a", "flow_direction")
    _equal(out["b"].data, ho.flow_direction(z64, *res), np.float32, "hydro_dataset_b", "flow_direction")
    with xa.fuse():                                                      # eager inside a scope
        inside = xa.flow_direction(_agg(xa, z64, res))
        _equal(inside.data, ho.flow_direction(z64, *res), np.float32, "hydro_in_fuse_scope", "flow_direction")
    assert xa.flow_direction(_agg(xa, np.zeros((0, 7), np.float32))).shape == (0, 7)
    assert xa.flow_accumulation(_agg(xa, np.zeros((5, 0), np.float32))).shape == (5, 0)


# ------------------------------------------------------------------ accumulation and basins on given direction rasters
@pytest.mark.parametrize("code", [1, 16], ids=["east", "west"])
@pytest.mark.parametrize("n", RAMP_LENGTHS)
def test_graph_ramps_around_every_power_of_two(xa, n, code):
    count = np.arange(1, n + 1, dtype=np.float64)
    want = (count[None, :], np.full((1, n), n - 1.0)) if code == 1 else (count[None, ::-1], np.zeros((1, n)))
    _graph(xa, ho.ramp(n, code), f"hydro_ramp_{'e' if code == 1 else 'w'}_{n}", want)


def test_graph_serpentine_depth_2144(xa):
    d = ho.serpentine(33, 65)
    _graph(xa, d, "hydro_serpentine_33x65")
    assert np.asarray(xa.flow_accumulation(_agg(xa, d)).data).max() == 2145


def test_graph_fan_contends_one_outlet(xa):
    z = ho.pit_cone(129, 257)
    d = xa.flow_direction(_agg(xa, z))
    _equal(d.data, ho.flow_direction(z), np.float32, "hydro_fan_129x257", "flow_direction")
    _graph(xa, np.asarray(d.data), "hydro_fan_129x257")
    acc = np.asarray(xa.flow_accumulation(d).data)
    assert acc.max() == 33153 == acc[64, 128]                            # no update lost: every cell arrives


def test_graph_random_directions_with_holes(xa):
    d = ho.random_directions(129, 257, 5)
    _graph(xa, d, "hydro_random_dirs_129x257")
    _graph(xa, d.astype(np.float64), "hydro_random_dirs_129x257_f64")    # any numeric raster of codes


def test_graph_all_zero_codes(xa):
    d = np.zeros((37, 300), np.int32)
    want = (np.ones((37, 300)), np.arange(37 * 300, dtype=np.float64).reshape(37, 300))
    _graph(xa, d, "hydro_all_zero_37x300", want)


@pytest.mark.parametrize("name", ["two_cells", "four_cells", "300_cells"])
def test_graph_cycles_raise(xa, name):
    d = {"two_cells": np.array([[0, 1, 16, 0]], np.float32), "four_cells": ho.ring(4, 5, 1, 1, 2, 2),
         "300_cells": ho.ring(80, 300, 3, 100, 70, 82)}[name]
    for fn in (xa.flow_accumulation, xa.basins):
        with pytest.raises(ValueError, match="contains a cycle"):
            fn(_agg(xa, d))
    _graph(xa, ho.break_cycles(d), f"hydro_cut_cycle_{name}")            # the same raster with the cycle cut is served


def test_graph_invalid_code_raises(xa):
    for bad in (3.0, -1.0, 0.5, 256.0, np.inf):
        d = np.zeros((5, 300), np.float32)
        d[3, 277] = bad
        for fn in (xa.flow_accumulation, xa.basins):
            with pytest.raises(ValueError, match="D8 codes"):
                fn(_agg(xa, d))


def test_end_to_end_on_generated_terrain(xa):
    terrain = xa.generate_terrain(xa.DataArray(np.zeros((257, 513), np.float32), dims=["y", "x"]))
    z = np.asarray(terrain.data)
    res = terrain.attrs["res"]
    want_dir = ho.flow_direction(z, *res)
    got_dir = xa.flow_direction(terrain)
    _equal(got_dir.data, want_dir, np.float32, "hydro_terrain_257x513", "flow_direction")
    want = (ho.flow_accumulation(want_dir), ho.basins(want_dir))
    _graph(xa, want_dir, "hydro_terrain_257x513_oracle_dirs", want)      # on the oracle's own direction plane
    _equal(xa.flow_accumulation(got_dir).data, want[0], np.float64, "hydro_terrain_257x513", "flow_accumulation")
    _equal(xa.basins(got_dir).data, want[1], np.float64, "hydro_terrain_257x513", "basins")
    assert want[0][~np.isnan(want[0])].min() == 1 and want[0][~np.isnan(want[0])].max() > 1


@pytest.mark.parametrize("scale", [1.0, 1e-300, 1e300, 5e-324], ids=["unit", "tiny", "huge", "subnormal"])
def test_direction_near_ties_at_every_magnitude(xa, scale):
    """Quotients a few ulp apart, across the three distances (3, 4 and exactly 5), where the kernel's estimate must leave the
    decision to the division; at magnitudes where the quotients underflow or the estimate is not used at all."""
    rng = np.random.default_rng(11)
    z = rng.integers(0, 5, (67, 259)).astype(np.float64)
    if scale != 5e-324:
        z *= 1.0 + rng.integers(-4, 5, z.shape) * 2.0 ** -52
    z = z * scale if scale != 1e300 else z * 1e150 * 1e150
    for res in ((3.0, 4.0), (1.0, 1.0), (1e-160, 1e-160), (1e150, 3e150)):
        _direction(xa, z, res, f"hydro_near_ties_{scale:g}_res_{res[0]:g}x{res[1]:g}")

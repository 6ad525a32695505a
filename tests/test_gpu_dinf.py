"""flow_direction(method='dinf') and flow_accumulation(method='dinf' | weights=..) on the MI355X, through the public functions,
against the rule in NumPy (tests/dinf_oracle.py).  tests/test_dinf_host.py pins the oracle to hand-worked
literals on the CPU.

Directions: which candidate wins takes exact operations only, so every cell whose oracle angle is a table entry, -1 or NaN
must be equal bit for bit; an interior angle goes through atan2 and is compared in ulps of the angle.  The largest difference
measured over every case of this file is MEASURED_MAX_ULP (profiles/dinf/parity_dinf.json); the bound is twice that and at
least 2 ulp.  No cell is left out.  Accumulations: tolerance 0, the bits of every cell.

Every comparison records its cell count (tests/parity_log.py)."""
import functools

import numpy as np
import pytest

from tests import dinf_oracle as do
from tests import hydrology_fill_oracle as fo
from tests import hydrology_oracle as ho
from tests import parity_log
from tests.test_dinf_host import workspace_layout

pytestmark = pytest.mark.gpu

MEASURED_MAX_ULP = 8.0
ULP_BOUND = max(2.0, 2.0 * MEASURED_MAX_ULP)
NAN, PI = np.nan, np.pi
RES = ((1.0, 1.0), (2.0, 0.5))


@pytest.fixture(scope="module")
def xa():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def _agg(xa, z, res=(1.0, 1.0)):
    return xa.DataArray(z, dims=["y", "x"], attrs={"res": res})


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _angles_equal(got, want, res, config):
    """Bit-equal where the oracle's angle is a table entry, -1 or NaN; within ULP_BOUND ulps of the angle everywhere else."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, (config, got.dtype, got.shape)
    exact = np.isnan(want) | (want == -1.0) | np.isin(want, do.table(*res))
    wrong = int(np.count_nonzero(_bits(got)[exact] != _bits(want)[exact]))
    inner = ~exact
    assert not np.isnan(got[inner]).any(), config
    err = do.ulps(got[inner], want[inner])
    worst = float(err.max()) if err.size else 0.0
    note = f"{int(inner.sum())} interior angles, max {worst:g} ulp; {wrong} of {int(exact.sum())} exact cells not bit-equal"
    print(f"{config} flow_direction_dinf: {note}")
    parity_log.record(config, "flow_direction_dinf", got, want, tol=f"{ULP_BOUND:g} ulp", note=note)
    assert wrong == 0, (config, note, np.argwhere(exact & (_bits(got) != _bits(want)))[:10].tolist())
    assert worst <= ULP_BOUND, (config, note, np.argwhere(inner & (np.abs(got - want) > ULP_BOUND * np.spacing(np.abs(want))))[:10].tolist())
    in_range = got[inner]
    assert ((in_range >= 0) & (in_range < 2 * PI)).all(), config
    return worst


def _direction(xa, z, res, config, **kw):
    got = xa.flow_direction(_agg(xa, z, res), method='dinf', **kw).data
    return _angles_equal(got, do.flow_direction(z, *res), res, config), np.asarray(got)


def _acc_equal(got, want, config, op="flow_accumulation_dinf"):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, (config, op, got.dtype, got.shape)
    nan = np.isnan(want)
    differ = int(np.count_nonzero(np.isnan(got) != nan)) + int(np.count_nonzero(_bits(got)[~nan] != _bits(want)[~nan]))
    note = f"{differ} of {want.size} cells not bit-equal"
    print(f"{config} {op}: {note}")
    parity_log.record(config, op, got, want, tol=0, note=note)
    assert differ == 0, (config, op, note, np.argwhere((_bits(got) != _bits(want)) & ~(np.isnan(got) & nan))[:10].tolist())


def _accumulate(xa, d, res, config, weights=None, method='dinf'):
    got = xa.flow_accumulation(_agg(xa, d, res), method=method, weights=None if weights is None else _agg(xa, weights)).data
    _acc_equal(got, do.flow_accumulation(d, method, *res, weights=weights), config, f"flow_accumulation_{method}")
    return np.asarray(got)


def _words(xa, d, res=(1.0, 1.0), method='dinf'):
    from xrspatial_amd import hydrology as hy
    if method == 'dinf':
        src = xa.DeviceArray.from_numpy(np.asarray(d, np.float64))
        return hy.frac_plane(src, hy.DINF, hy.angle_table(*res))[1]
    return hy.frac_plane(xa.DeviceArray.from_numpy(np.asarray(d, np.float32)), hy.D8)[1]


@functools.lru_cache(maxsize=None)
def _terrain(rows, cols):
    import xrspatial_amd as xa
    terrain = xa.generate_terrain(xa.DataArray(np.zeros((rows, cols), np.float32), dims=["y", "x"]))
    return np.asarray(terrain.data), tuple(float(v) for v in terrain.attrs["res"])


# ------------------------------------------------------------------ directions
def test_direction_literals(xa):
    for res in RES:
        b = do.table(*res)
        for z in (np.array([[5.0]]), np.array([[NAN]]), np.array([[5.0, 4.0, NAN, 1.0, 2.0]]), np.array([[5.0], [4.0], [4.0], [1.0], [2.0]])):
            _direction(xa, z, res, f"dinf_literal_{z.shape[0]}x{z.shape[1]}")
        got = np.asarray(xa.flow_direction(_agg(xa, np.array([[5.0, 4.0, NAN, 1.0, 2.0]]), res), method='dinf').data)
        assert np.array_equal(_bits(got), _bits([[b[0], -1.0, NAN, -1.0, b[4]]]))
        for ring, centre in (([8, 7, 10, 10, 10, 10, 10, 10], 10.0), ([10, 8.5, 9, 10, 10, 10, 10, 10], 10.0), ([5.0] * 8, 1.0),
                             ([NAN, 7, 8, 10, 10, 10, 10, 10], 10.0), ([0.0] * 8, np.inf), ([-np.inf, 0, 10, 10, 10, 10, 10, 10], 10.0),
                             ([8, -np.inf, 10, 10, 10, 10, 10, 10], 10.0), ([-1e-200, -1.5e-200, 0, 0, 0, 0, 0, 0], 0.0),
                             ([-1e200, -1.2e200, 0, 0, 0, 0, 0, 0], 1e200), ([8, 7.9375, 10, 10, 10, 10, 10, 10], 10.0),
                             ([8, 7.875, 10, 10, 10, 10, 10, 10], 10.0)):
            z = np.full((3, 3), centre)
            for (dr, dc), v in zip(do.OFFSETS, ring):
                z[1 + dr, 1 + dc] = v
            _direction(xa, z, res, "dinf_literal_3x3")
    got = np.asarray(xa.flow_direction(_agg(xa, np.array([[10.0, 10, 7], [10, 10, 8], [10, 10, 10]])), method='dinf').data)
    assert abs(got[1, 1] - 0.4636476090008061) <= ULP_BOUND * np.spacing(0.4636476090008061)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(8, 63), (9, 64), (17, 65), (9, 130), (17, 130), (8, 257)])
def test_direction_across_block_edges(xa, shape, dtype):
    z = ho.random_terrain(*shape, seed=shape[1], dtype=dtype)
    z[shape[0] // 2, shape[1] // 3] = NAN
    z[1, 5:9] = z[1, 5]                                                  # a flat run
    for res in RES:
        _direction(xa, z, res, f"dinf_terrain_{shape[0]}x{shape[1]}_{np.dtype(dtype).name}_res_{res[0]:g}")
    ints = ho.random_terrain(*shape, seed=1, dtype=np.float64).round(0).astype(np.int32)       # widened on the host; ties and flats
    _angles_equal(xa.flow_direction(_agg(xa, ints), method='dinf').data, do.flow_direction(ints), (1.0, 1.0), f"dinf_int32_{shape[0]}x{shape[1]}")


@pytest.mark.parametrize("res", RES)
def test_direction_of_tilted_planes_and_a_cone(xa, res):
    b = do.table(*res)
    for az in (0, 20, 45, 75, 90, 133, 180, 200, 260, 315, 350):
        for dtype in (np.float32, np.float64):
            z = do.plane(20, 70, az, dtype)
            _, got = _direction(xa, z, res, f"dinf_plane_az{az}_{np.dtype(dtype).name}_res_{res[0]:g}")
        if res == (1.0, 1.0):                                            # the float64 plane's interior cells point down the azimuth
            assert np.allclose(got[1:-1, 1:-1], np.radians(az), atol=1e-9), az
    _, got = _direction(xa, do.cone(65, 130), res, f"dinf_cone_65x130_res_{res[0]:g}")
    assert (~np.isin(got, b) & (got >= 0)).sum() > 6000                  # the cone's angles are interior ones


def test_direction_on_generated_terrain_raw_and_filled(xa):
    z, res = _terrain(129, 257)
    _direction(xa, z, res, "dinf_generate_terrain_129x257")
    filled = np.asarray(xa.fill(_agg(xa, z, res)).data)
    want_codes = fo.resolve_flats(filled, *res)[0]
    got = np.asarray(xa.flow_direction(_agg(xa, filled, res), method='dinf', resolve_flats=True).data)
    _angles_equal(got, do.flow_direction(filled, *res, codes=want_codes), res, "dinf_generate_terrain_129x257_filled_resolved")
    codes = np.asarray(xa.flow_direction(_agg(xa, filled, res), resolve_flats=True).data)
    assert np.array_equal(got == -1.0, codes == 0) and np.array_equal(np.isnan(got), np.isnan(codes))
    plain = np.asarray(xa.flow_direction(_agg(xa, filled, res), method='dinf').data)
    flat = np.asarray(xa.flow_direction(_agg(xa, filled, res)).data) == 0
    assert np.array_equal(_bits(plain[~flat]), _bits(got[~flat])) and (plain[flat] == -1.0).all() and (got[flat] != -1.0).sum() > 0


# ------------------------------------------------------------------ accumulation of a given direction raster
def test_serpentine_longer_than_cap_in_one_tile(xa):
    from xrspatial_amd import hydrology as hy
    d = do.codes_to_angles(ho.serpentine(64, 64))
    got = _accumulate(xa, d, (1.0, 1.0), "dinf_serpentine_64x64")
    assert got.max() == 4096
    words = _words(xa, d)
    assert words[0] > 2 and words[hy.FRAC_BITS] == 0 and words[hy.FRAC_LEFT] == 0 and words[hy.FRAC_GRAPH] == 4096
    rounds = hy.relax_rounds(words)
    assert sum(rounds["changed"]) == 4096 and max(rounds["changed"]) < 4096 and rounds["tiles"] == [1] * (words[0] - 1) + [0]      # CAP stops every launch but the last; the closing round has no tile


def test_serpentine_across_tiles_of_all_four_colours(xa):
    for res in RES:
        d = do.codes_to_angles(ho.serpentine(65, 130), *res)
        assert _accumulate(xa, d, res, f"dinf_serpentine_65x130_res_{res[0]:g}").max() == 65 * 130
    _accumulate(xa, ho.serpentine(65, 130), (1.0, 1.0), "dinf_serpentine_65x130", weights=np.full((65, 130), 0.1), method='d8')


def test_ramp_of_4097_cells(xa):
    for code in (1, 16):
        d = do.codes_to_angles(ho.ramp(4097, code))
        got = _accumulate(xa, d, (1.0, 1.0), f"dinf_ramp_{code}_4097")
        want = np.arange(1, 4098, dtype=np.float64)[None, :]
        assert np.array_equal(got, want if code == 1 else want[:, ::-1])
    _accumulate(xa, do.codes_to_angles(ho.ramp(4097, 1).T * 4), (1.0, 1.0), "dinf_ramp_south_4097")


def test_d8_codes_as_table_angles_equal_method_d8_bit_for_bit(xa):
    d = ho.random_directions(130, 130, 5)
    plain = np.asarray(xa.flow_accumulation(_agg(xa, d)).data)
    assert plain.dtype == np.float64
    for res in RES:
        got = np.asarray(xa.flow_accumulation(_agg(xa, do.codes_to_angles(d, *res), res), method='dinf').data)
        _acc_equal(got, plain, f"dinf_d8_identity_130x130_res_{res[0]:g}")
    _acc_equal(do.flow_accumulation(do.codes_to_angles(d)), plain, "dinf_d8_identity_130x130_oracle")
    for ones in (np.ones(d.shape, np.float64), np.ones(d.shape, np.float32), np.ones(d.shape, np.uint8), np.ones(d.shape, bool)):
        got = xa.flow_accumulation(_agg(xa, d), method='d8', weights=_agg(xa, ones)).data
        _acc_equal(got, plain, f"dinf_d8_weights_ones_{ones.dtype.name}", "flow_accumulation_d8_weights")


def test_float_negative_and_nan_weights(xa):
    rng = np.random.default_rng(3)
    d8 = ho.random_directions(70, 90, 2)
    dag = do.random_dag(70, 90, 4, (2.0, 0.5))
    for w, tag in ((rng.random((70, 90)), "float"), (rng.normal(size=(70, 90)), "negative"), (rng.random((70, 90)).astype(np.float32), "float32"),
                   (rng.integers(-3, 9, (70, 90)).astype(np.int16), "int16")):
        _accumulate(xa, d8, (1.0, 1.0), f"dinf_weights_{tag}_d8", weights=w, method='d8')
        _accumulate(xa, dag, (2.0, 0.5), f"dinf_weights_{tag}_dinf", weights=w)
    w = rng.random((70, 90))
    w[10, 10], w[40, 50], w[69, 0] = NAN, np.inf, -np.inf
    got = _accumulate(xa, dag, (2.0, 0.5), "dinf_weights_nan_inf", weights=w)
    assert np.isnan(got[10, 10])
    _accumulate(xa, d8, (1.0, 1.0), "dinf_weights_nan_inf_d8", weights=w, method='d8')


@pytest.mark.parametrize("res", RES)
def test_interior_angles_of_planes_and_terrain_feed_both_sides(xa, res):
    for az in (20, 133, 260):
        ang = np.asarray(xa.flow_direction(_agg(xa, do.plane(70, 130, az), res), method='dinf').data)
        _accumulate(xa, ang, res, f"dinf_acc_plane_az{az}_res_{res[0]:g}")
    z, tres = _terrain(129, 257)
    filled = xa.fill(_agg(xa, z, tres))
    ang = np.asarray(xa.flow_direction(filled, method='dinf', resolve_flats=True).data)
    got = _accumulate(xa, ang, tres, "dinf_acc_generate_terrain_129x257")
    assert not np.isnan(got).any() and got.min() >= 1.0
    _accumulate(xa, np.asarray(xa.flow_direction(_agg(xa, do.cone(65, 130), res), method='dinf').data), res, f"dinf_acc_cone_res_{res[0]:g}")


def test_nan_cells_all_nan_and_angles_exactly_at_the_table(xa):
    dag = do.random_dag(66, 67, 9)
    assert np.isnan(dag).sum() > 100
    _accumulate(xa, dag, (1.0, 1.0), "dinf_nan_cells_66x67")
    got = _accumulate(xa, np.full((5, 70), NAN), (1.0, 1.0), "dinf_all_nan")
    assert np.isnan(got).all()
    for res in RES:
        b = do.table(*res)
        rng = np.random.default_rng(7)
        z = rng.random((40, 70))                                         # every cell points at a lower neighbour, exactly at b[o]
        order = np.full((40, 70), -1.0)
        for i in range(40):
            for j in range(70):
                lower = [n for n, (dr, dc) in enumerate(do.OFFSETS) if 0 <= i + dr < 40 and 0 <= j + dc < 70 and z[i + dr, j + dc] < z[i, j]]
                if lower:
                    order[i, j] = b[lower[(i + j) % len(lower)]]
        got = _accumulate(xa, order, res, f"dinf_angles_at_table_res_{res[0]:g}")
        assert np.array_equal(got, np.round(got))                        # every share is 1.0: counts


def test_cycles_raise_with_the_count_of_cells_left(xa):
    from xrspatial_amd import hydrology as hy
    b = do.table()
    two = np.array([[0.0, PI, -1.0]])
    ring300 = do.codes_to_angles(ho.ring(80, 100, 5, 9, 70, 82))         # 300 cells, across tiles
    assert int((ring300 >= 0).sum()) == 300
    trib = do.codes_to_angles(ho.ring(70, 70, 20, 20, 30, 30))           # 116 cells, with tributaries and cells below it
    trib[19, 25] = b[6]                                                  # flows into the ring: becomes final
    trib[18, 25] = b[6]
    trib[20, 30] = (b[0] + b[1]) / 2                                     # a ring cell that also gives to (19, 31), outside the ring
    trib[19, 31] = b[0]                                                  # which flows on to (19, 32): both lie below the cycle
    for d, left in ((two, 2), (ring300, 300), (trib, 118)):
        with pytest.raises(ValueError, match=f"cycle: {left} cells"):
            do.flow_accumulation(d)
        with pytest.raises(ValueError, match=f"cycle: {left} cells"):
            xa.flow_accumulation(_agg(xa, d), method='dinf')
    codes = ho.ring(80, 100, 5, 9, 70, 82)
    with pytest.raises(ValueError, match="cycle: 300 cells"):
        xa.flow_accumulation(_agg(xa, codes), weights=_agg(xa, np.ones(codes.shape)))
    src = xa.DeviceArray.from_numpy(trib)
    with pytest.raises(ValueError, match="cycle"):
        hy.frac_plane(src, hy.DINF, hy.angle_table(1.0, 1.0))


def test_invalid_values_raise(xa):
    for bad in (7.0, -0.5, np.inf, -np.inf, 2 * PI, -1.0000000000000002):
        d = np.full((70, 70), -1.0)
        d[65, 66] = bad
        with pytest.raises(ValueError, match="angle"):
            xa.flow_accumulation(_agg(xa, d), method='dinf')
    d = ho.random_directions(20, 30, 1)
    d[3, 4] = 3.0
    with pytest.raises(ValueError, match="D8 codes"):
        xa.flow_accumulation(_agg(xa, d), method='d8', weights=_agg(xa, np.ones(d.shape)))
    with pytest.raises(ValueError, match="method"):
        xa.flow_accumulation(_agg(xa, d), method='mfd')
    ok = np.full((3, 3), 2 * PI)
    ok[:] = np.nextafter(2 * PI, 0.0)                                    # the largest angle below 2 pi is one
    _accumulate(xa, ok, (1.0, 1.0), "dinf_largest_angle")
    _accumulate(xa, np.full((3, 3), -0.0), (1.0, 1.0), "dinf_negative_zero")


def test_backends_dataset_input_and_empty_rasters(xa):
    z, res = _terrain(129, 257)
    host = _agg(xa, z, res)
    dev = _agg(xa, xa.DeviceArray.from_numpy(z), res)
    ang_host = xa.flow_direction(host, method='dinf')
    ang_dev = xa.flow_direction(dev, method='dinf', name='angles')
    assert isinstance(ang_host.data, np.ndarray) and isinstance(ang_dev.data, xa.DeviceArray) and ang_dev.name == 'angles'
    assert ang_dev.dtype == np.float64 and ang_dev.attrs == host.attrs and ang_dev.dims == host.dims
    assert np.array_equal(_bits(ang_dev.data.get()), _bits(ang_host.data))
    w = np.random.default_rng(0).random(z.shape).astype(np.float32)
    filled = xa.flow_direction(xa.fill(dev), method='dinf', resolve_flats=True)
    want = xa.flow_accumulation(_agg(xa, filled.data.get(), res), method='dinf', weights=_agg(xa, w))
    mixed = xa.flow_accumulation(filled, method='dinf', weights=_agg(xa, w))                     # the result's backend is flow_dir's
    both = xa.flow_accumulation(filled, method='dinf', weights=_agg(xa, xa.DeviceArray.from_numpy(w)))
    up = xa.flow_accumulation(_agg(xa, filled.data.get(), res), method='dinf', weights=_agg(xa, xa.DeviceArray.from_numpy(w)))
    assert isinstance(want.data, np.ndarray) and isinstance(up.data, np.ndarray)
    for other in (mixed, both):
        assert isinstance(other.data, xa.DeviceArray) and np.array_equal(_bits(other.data.get()), _bits(want.data))
    assert np.array_equal(_bits(up.data), _bits(want.data))
    ds = xa.Dataset({"a": host, "b": _agg(xa, z[::-1].copy(), res)}, attrs={"k": 1})
    out = xa.flow_direction(ds, method='dinf')
    assert set(out.data_vars) == {"a", "b"} and out.attrs == {"k": 1} and np.array_equal(_bits(out["a"].data), _bits(ang_host.data))
    acc = xa.flow_accumulation(out, method='dinf', weights=_agg(xa, w))
    assert acc["b"].name == "b" and acc["a"].dtype == np.float64
    with xa.fuse():                                                      # eager inside a scope
        inside = xa.flow_direction(host, method='dinf')
    assert np.array_equal(_bits(inside.data), _bits(ang_host.data))
    for shape in ((0, 5), (5, 0), (0, 0)):
        empty = _agg(xa, np.zeros(shape, np.float32))
        got = xa.flow_direction(empty, method='dinf')
        assert got.shape == shape and got.dtype == np.float64
        got = xa.flow_accumulation(_agg(xa, np.zeros(shape)), method='dinf', weights=_agg(xa, np.zeros(shape)))
        assert got.shape == shape and got.dtype == np.float64
        assert xa.flow_accumulation(_agg(xa, np.zeros(shape, np.float32)), weights=_agg(xa, np.zeros(shape))).shape == shape


def test_workspace_size_against_its_written_layout(xa):
    from xrspatial_amd import _lib
    for shape in ((1, 1), (64, 64), (65, 130), (1, 4097), (257, 513), (8192, 8192)):
        assert _lib.workspace_bytes("flow_accumulate_frac", *shape) == workspace_layout(*shape), shape
    assert _lib.workspace_bytes("flow_accumulate_frac", 0, 7) == 0


# ------------------------------------------------------------------ the chain
def test_end_to_end_chain_on_generated_terrain(xa):
    """terrain -> fill -> flow_direction(dinf, resolve_flats) -> flow_accumulation(dinf) at 257 x 513.  Every non-NaN cell is final
    (the call raises otherwise), and the water that leaves at the rim equals the cell count up to the rounding of the sums:
    the relative difference is printed and recorded, not gated."""
    z, res = _terrain(257, 513)
    terrain = _agg(xa, z, res)
    ang = xa.flow_direction(xa.fill(terrain), method='dinf', resolve_flats=True)
    acc = xa.flow_accumulation(ang, method='dinf')
    a, got = np.asarray(ang.data), np.asarray(acc.data)
    assert not np.isnan(got).any() and (a >= 0).sum() + (a == -1.0).sum() == a.size
    words = _words(xa, a, res)
    assert words[5] == 0 and words[6] == a.size and words[4] == 0
    valid, out = do.edges(a, 'dinf', *res)
    b = do.table(*res)
    leaving = 0.0
    for u in range(a.size):                                              # what a cell gives to receivers outside the raster, and all of an outlet's
        angle = a.ravel()[u]
        if angle == -1.0:
            leaving += got.ravel()[u]
            continue
        o = max(k for k in range(8) if angle >= b[k])
        width = b[o + 1] - b[o]
        kept = sum(share for _, _, share in out[u])
        leaving += got.ravel()[u] * (((b[o + 1] - angle) / width + (angle - b[o]) / width) - kept)
    rel = abs(leaving - a.size) / a.size
    print(f"dinf_chain_257x513: water leaving at the rim {leaving!r} of {a.size} cells, relative difference {rel:.3e}; "
          f"largest accumulation {got.max():.1f}; rounds {words[0]}")
    parity_log.record("dinf_chain_257x513", "rim_outflow", np.array([leaving]), np.array([float(a.size)]), note=f"relative difference {rel:.3e}")
    _acc_equal(got, do.flow_accumulation(a, 'dinf', *res), "dinf_chain_257x513")

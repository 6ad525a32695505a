"""The inputs of tests/test_gpu_zonal_partials.py, checked without a GPU: the references of tests/zonal_partial_cases.py
against plain Python loops, and -- with the CPU model of zonal_kernel's wave paths -- that every case reaches the paths it is
named for.  A GPU test that compares tables exactly proves nothing about a path no wave of its input takes."""
import math

import numpy as np
import pytest

from tests import zonal_partial_cases as pc

VTYPES = [np.float32, np.float64]
ids = lambda d: np.dtype(d).name  # noqa: E731


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("dtype", VTYPES, ids=ids)
def test_reference_vs_python_loop(dtype):
    nz, shift, nodata = 7, 3.0, 17.0
    z, _ = pc.segment_layout(45_000, nz, 2, seed=1)
    z = z[-600:].copy()
    z[::41], z[5::43] = -1, nz
    v = pc.value_plane(z, dtype, seed=2, nodata=nodata)
    v[7], v[8] = nodata, 2000.0
    want = {"count": [0] * nz, "sum": [0.0] * nz, "sumsq": [0.0] * nz, "min": [math.inf] * nz, "max": [-math.inf] * nz}
    for zi, x in zip(z.tolist(), v.tolist()):
        if not (0 <= zi < nz) or math.isnan(x) or math.isinf(x) or x == nodata:
            continue
        want["count"][zi] += 1
        want["sum"][zi] += x - shift                     # (multiples of 1/4 far below 2^53: exact)
        want["sumsq"][zi] += (x - shift) ** 2
        want["min"][zi] = min(want["min"][zi], x)
        want["max"][zi] = max(want["max"][zi], x)
    got = pc.reference(z, v, nz, shift, nodata)
    assert sum(want["count"]) < z.size - 30              # (cells were left out)
    for key in want:
        np.testing.assert_array_equal(got[key], np.array(want[key]), err_msg=key)
    assert got["count"].dtype == np.uint64 and got["min"].dtype == np.dtype(dtype)
    fs = pc.reference_fsum(z, v, nz, shift, nodata)
    np.testing.assert_array_equal(fs[0], got["sum"])
    np.testing.assert_array_equal(fs[1], got["sumsq"])
    assert (fs[2][:-1] > 0).all() and (fs[3][:-1] > 0).all() and got["count"][-1] == 0   # (the last zone is drawn nowhere)


def test_reference_of_a_zone_without_cells_and_of_nodata_that_is_no_number():
    z = np.array([0, 0, 2, 2, -1, 3], np.int32)
    v = np.array([1.0, np.nan, np.inf, -np.inf, 5.0, 6.0], np.float32)
    for nodata in (None, float("nan"), float("inf")):
        got = pc.reference(z, v, 3, 0.0, nodata)
        assert got["count"].tolist() == [1, 0, 0] and got["sum"].tolist() == [1.0, 0.0, 0.0]
        assert got["min"].tolist() == [1.0, np.inf, np.inf] and got["max"].tolist() == [1.0, -np.inf, -np.inf]


def test_fsum_bound_is_the_derived_one():
    z = np.zeros(5, np.int32)
    v = np.array([1.5, -2.25, 4.0, np.nan, 0.125])
    s, q, bs, bq = pc.reference_fsum(z, v, 1, 1.0)[:, 0]
    t = [0.5, -3.25, 3.0, -0.875]
    assert s == math.fsum(t) and q == math.fsum(x * x for x in t)
    assert bs == 4 * 2.0 ** -52 * math.fsum(abs(x) for x in t) and bq == 4 * 2.0 ** -52 * q


def test_lut_helpers():
    ids_ = np.array([-5, -2, 4])
    lut = pc.lut_table(ids_, -5, 12)
    assert lut.tolist() == [0, -1, -1, 1, -1, -1, -1, -1, -1, 2, -1, -1]
    raw = np.array([-5, -6, 4, 6, 7, pc.I32.max, pc.I32.min, -2], np.int32)
    assert pc.lut_map(raw, -5, lut).tolist() == [0, -1, 2, -1, -1, -1, -1, 1]


# -------------------------------------------------------------------------------------------------- the wave model
def test_wave_model_on_hand_made_waves():
    nz = 10
    ok = np.ones(512, bool)
    one = np.full(512, 3)
    assert pc.wave_paths(one, ok, nz, 2)["one_zone"] == 1
    assert pc.wave_paths(one, ~ok, nz, 2)["one_zone_no_valid"] == 1
    assert pc.wave_paths(np.full(512, nz), ok, nz, 2)["one_zone_skipped"] == 1
    assert pc.wave_paths(one, ok, nz, 2, aligned=False) == {**dict.fromkeys(pc.PATHS, 0), "tail_cells": 512}
    # U = 4: the same 512 cells are half a wave, padded with cells of no zone
    got = pc.wave_paths(one, ok, nz, 4)
    assert (got["one_zone"], got["partial_wave"], got["rows16"], got["lane_by_lane"]) == (0, 1, 8, 2)
    # two zones, the boundary at a row's edge: 8 rows, nothing else
    z = np.repeat([1, 2], 256)
    got = pc.wave_paths(z, ok, nz, 2)
    assert (got["rows16"], got["mixed"], got["lane_by_lane"], got["over8"], got["lane_split"]) == (8, 0, 0, 0, 0)
    # the boundary inside lane 16's cells (cell 66): row 1 of slot 0 goes lane by lane, lane 16 splits its last two cells off
    z = np.concatenate([np.full(66, 1), np.full(446, 2)])
    got = pc.wave_paths(z, ok, nz, 2)
    assert (got["rows16"], got["mixed"], got["lane_split"]) == (7, 1, 1)
    # a lane without a valid cell breaks its row
    bad = ok.copy()
    bad[8:12] = False
    got = pc.wave_paths(np.repeat([1, 2], 256), bad, nz, 2)
    assert (got["rows16"], got["mixed"]) == (7, 1)
    # a row whose FIRST lane is empty is not folded either, and an invalid cell inside a lane changes nothing
    bad = ok.copy()
    bad[0:4], bad[301] = False, False
    got = pc.wave_paths(np.repeat([1, 2], 256), bad, nz, 2)
    assert (got["rows16"], got["mixed"], got["lane_split"]) == (7, 1, 0)
    # 9 runs under a slot: no row test; 8 runs: rows where they fit
    z = np.concatenate([np.repeat(np.arange(9), 28), np.full(4, 9), np.repeat(np.arange(8), 32)])
    got = pc.wave_paths(z, ok, nz, 2)
    assert (got["over8"], got["lane_by_lane"], got["rows16"]) == (1, 1, 0)
    # tails
    got = pc.wave_paths(np.full(515, 3), ok[:1].repeat(515), nz, 2)
    assert (got["one_zone"], got["one_zone_skipped"], got["partial_wave"], got["tail_cells"]) == (1, 0, 0, 3)


def test_launches():
    assert pc.launch_window(np.float32) == 5266 and pc.launch_window(np.float64) == 4096
    assert pc.launches(2340, np.float32) == [(0, 2340, 2)] and pc.launches(2341, np.float32) == [(0, 2341, 4)]
    assert pc.launches(1820, np.float64) == [(0, 1820, 2)] and pc.launches(1821, np.float64) == [(0, 1821, 4)]
    assert pc.launches(2341, np.float32, aligned=False) == [(0, 2341, 2)]
    assert pc.launches(12_000, np.float32) == [(0, 5266, 4), (5266, 5266, 4), (10532, 1468, 2)]
    assert pc.launches(9_000, np.float64) == [(0, 4096, 4), (4096, 4096, 4), (8192, 808, 2)]


# ----------------------------------------------------------------------------------- every case reaches its paths
@pytest.mark.parametrize("dtype", VTYPES, ids=ids)
def test_every_case_reaches_the_paths_it_is_named_for(dtype):
    cases = pc.all_cases(dtype)
    assert len({c.name for c in cases}) == len(cases)
    for case in cases:
        assert case.need or case.name.startswith("n"), case.name
        got = pc.case_paths(case)
        missing = [p for p in case.need if got[p] < 1]
        assert not missing, (case.name, missing, got)
        if case.need_nonzero_base:
            got = pc.case_paths(case, base_only="nonzero")
            missing = [p for p in case.need_nonzero_base if got[p] < 1]
            assert not missing, (case.name, "zbase != 0", missing, got)
        # with a plane that is not 16-byte aligned every cell takes the scalar tail
        assert pc.case_paths(case, aligned=False)["tail_cells"] >= case.z.size
        # invalid values sit inside one-zone trips too (the cell_ok test of that fold)
        if "one_zone" in case.need and case.name != "edges":
            z, bad = case.idx, ~case.ok
            where = slice(4 * pc.RUN_LONG, 5 * pc.RUN_LONG)                  # (the fifth long run)
            assert (z[where] == z[where][0]).all() and 0 <= z[where][0] < case.n_zones and bad[where].any(), case.name
            assert not bad[where].all(), case.name


@pytest.mark.parametrize("dtype", VTYPES, ids=ids)
def test_dense_cases_cover_both_instantiations_and_leave_one_zone_empty(dtype):
    seen = set()
    for case in pc.dense_cases(dtype) + [pc.windows_case(dtype)]:
        seen |= {slots for _, _, slots in pc.launches(case.n_zones, dtype)}
        want = pc.reference(case.idx, case.v, case.n_zones, case.shift, case.nodata)
        dead = case.extra["dead"]
        assert (case.idx == dead).sum() >= pc.RUN_LONG and want["count"][dead] == 0
        assert want["min"][dead] == np.inf and want["max"][dead] == -np.inf
        assert (want["count"] > 0).sum() >= min(case.n_zones - 1, 38)
        assert case.n_zones % 256
    assert seen == {2, 4}


@pytest.mark.parametrize("dtype", VTYPES, ids=ids)
def test_window_cases_place_the_invalid_id_and_the_stray_cell(dtype):
    for case in pc.window_cases(dtype) + pc.stray_cases(dtype):
        e = case.extra
        inside = (case.idx >= 0)
        np.testing.assert_array_equal(case.z[inside].astype(np.int64) - e["base"], case.idx[inside])
        assert e["base"] >= pc.I32.min and e["base"] + e["window"] - 1 <= pc.I32.max
        dead_cells = np.flatnonzero(case.idx == e["dead"])
        assert dead_cells.size == {"long": pc.RUN_LONG, "run100": 100, "tail": 1}[e["dead_at"]] and not case.ok[dead_cells].any()
        if e["dead_at"] == "tail":
            assert dead_cells[0] >= case.z.size // 4 * 4
        if "stray" in e:
            off = int(case.z[e["stray_at"]]) - e["base"]
            assert (~inside).sum() == 1 and not (0 <= off < e["window"]) and case.ok[e["stray_at"]]
            if e["stray"] == "tail":
                assert e["stray_at"] >= case.z.size // 4 * 4
            if e["stray"] == "long":
                around = np.delete(case.idx[:pc.RUN_LONG], e["stray_at"])
                assert (around == around[0]).all()
        else:
            assert inside.all()


def test_the_earlier_small_layouts_reach_no_one_zone_trip_and_no_folded_row():
    """The layouts of the small tests that compared partials with the oracle before: whatever they assert, no sum, count,
    min or max of theirs came through wave_reduce or row16_reduce."""
    for name, (z, ok, nz) in pc.earlier_layouts().items():
        got = pc.wave_paths(z, ok, nz, 2)
        print(name, got)
        assert got["one_zone"] == got["one_zone_no_valid"] == got["rows16"] == got["mixed"] == 0, (name, got)
        assert got["lane_by_lane"] + got["over8"] == 2 * -(-(z.size // 4) // 128), (name, got)
        assert got["lane_split"] > 1000, (name, got)

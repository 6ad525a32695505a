"""The Gi* class rule on the CPU (no GPU): the oracle's `hotspot_classes` and tests/fake_hip.py's emulation of
xrs_hotspots_classify_f32 against the float64 rule restated in tests/streaming_cases.py, on every float32 in [1, 3] and around every
threshold -- the inputs tests/test_gpu_streaming_abi.py gives the kernel.

The reference's `_calc_hotspots_numpy` (xrspatial/focal.py:881-915) is a Numba loop that compares a float32 z-score with Python
literals; Numba types that comparison float64.  Comparing in float32 (the thresholds rounded first) is a different function at
exactly one magnitude: |z| == float32(1.96) = 1.9600000381469727, which lies ABOVE 1.96 and is therefore +-95, where the float32
rule says +-90.  The other four thresholds round down; there the float32 rule moves a cell between two rungs of the p-value ladder
that the confidence tests do not tell apart."""

import numpy as np
import pytest

from oracle import xrs_oracle as orc
from tests import fake_hip
from tests import streaming_cases as sc

F32 = np.float32


@pytest.fixture(scope="module")
def sweep():
    z = sc.sweep()
    z.setflags(write=False)
    want = sc.classes_f64(z)
    want.setflags(write=False)
    return z, want


def _fake_classes(m, gmean, gstd):
    m = np.ascontiguousarray(m, F32)
    out = np.full(m.size + 1, 0x5A, np.int8)
    fake_hip.call("xrs_hotspots_classify_f32", m.ctypes.data, out.ctypes.data, m.size, float(gmean), float(gstd), None)
    assert out[-1] == 0x5A
    return out[:-1]


def test_float64_rule_by_hand():
    """the restated rule on cells worked out by hand from focal.py:890-914"""
    z = np.array([0.0, 1.0, 1.65, 1.7, 1.96, 1.97, 2.0, 2.33, 2.58, 2.59, 3.0, np.nan, np.inf, -1.7, -2.0, -2.6, -np.inf], F32)
    #            float32(1.65) < 1.65: 0;  float32(1.96) > 1.96: 95;  float32(2.58) < 2.58: 95
    assert sc.classes_f64(z).tolist() == [0, 0, 0, 90, 95, 95, 95, 95, 95, 99, 99, 0, 99, -90, -95, -99, -99]


def test_the_float32_rule_differs_at_one_magnitude(sweep):
    z, want = sweep
    differs = z[sc.classes_f32(z) != want]
    assert differs.tolist() == [float(F32(1.96))] and float(F32(1.96)) == 1.9600000381469727
    at = np.array([differs[0], -differs[0]], F32)
    assert sc.classes_f32(at).tolist() == [90, -90] and sc.classes_f64(at).tolist() == [95, -95]
    near = sc.neighbourhood()
    assert set(near[sc.classes_f32(near) != sc.classes_f64(near)].tolist()) == {float(differs[0]), -float(differs[0])}


@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
def test_oracle_and_emulation_on_every_float32_between_1_and_3(sweep, sign):
    z, want = sweep
    z, want = (z, want) if sign > 0 else (-z, -want)
    assert np.array_equal(orc.hotspot_classes(z), want)
    assert np.array_equal(_fake_classes(z, 0.0, 1.0), want)


def test_oracle_and_emulation_around_the_thresholds():
    z = sc.neighbourhood()
    want = sc.classes_f64(z)
    assert want[z == F32(1.96)].tolist() == [95] and want[z == -F32(1.96)].tolist() == [-95]
    assert np.array_equal(orc.hotspot_classes(z), want)
    assert np.array_equal(_fake_classes(z, 0.0, 1.0), want)


def test_emulation_forms_z_in_float32():
    gmean, gstd = F32(50.3), F32(20.7)
    m = sc.division_cells(gmean, gstd)
    want = sc.classes_f64(sc.zscore(m, gmean, gstd))
    assert np.unique(want).tolist() == [-99, -95, -90, 0, 90, 95, 99]
    assert np.array_equal(_fake_classes(m, gmean, gstd), want)
    assert not _fake_classes(m, gmean, np.nan).any()


def test_oracle_hotspots_uses_the_rule():
    """orc.hotspots end to end: its classes are `hotspot_classes` of the z-scores it returns"""
    rng = np.random.default_rng(3)
    data = rng.normal(10.0, 3.0, (40, 50)).astype(F32)
    data[5:9, 5:9] += 12.0
    classes, z = orc.hotspots(data, np.ones((3, 3)))
    assert z.dtype == F32 and classes.dtype == np.int8
    assert np.array_equal(classes, sc.classes_f64(z)) and len(np.unique(classes)) > 2


def test_cases_are_what_the_gpu_tests_say():
    """the sizes tests/test_gpu_streaming_abi.py relies on to reach the capped grids"""
    def grid(slots):
        groups = min(max((slots + 255) // 256, 1), 2048)
        groups = (groups + 7) // 8 * 8
        per = ((slots + groups - 1) // groups + 1023) // 1024 * 1024
        return groups, per
    assert sc.sweep().size == sc.SWEEP_CELLS == 12_582_913
    # classify sweep: the launch sizes its grid from n / 4 cells-of-four, 2048 workgroups, chunks of two trips, 512 of them empty
    groups, per = grid(sc.SWEEP_CELLS // 4)
    assert (groups, per, -(-(sc.SWEEP_CELLS // 4) // per), sc.SWEEP_CELLS % 4) == (2048, 2048, 1536, 1)
    n = sc.MOMENT_SIZES[-1]
    groups, per = grid(n // 4)
    assert (n, groups, per, n // 4 - 1024 * per, n % 4) == (8_388_615, 2048, 2048, 1, 3)
    n = sc.MINMAX_BIG                           # minmax sizes its grid from n / 4 too, but its slots are cells
    groups = (min(max((n // 4 + 255) // 256, 1), 2048) + 7) // 8 * 8
    per = ((n + groups - 1) // groups + 1023) // 1024 * 1024
    assert (groups, per, n - 1024 * per) == (2048, 2048, 5)
    assert len(sc.minmax_contents(70_001)) == 13 and sc.neighbourhood().size == 2 * 5 * 17 + 9

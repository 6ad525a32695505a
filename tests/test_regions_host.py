"""CPU checks of zonal.regions: the restatement of DESIGN.md §6b against the reference's own outputs
(tests/golden/regions_exec.npz), the fast oracle against the restatement, the float32 typing the device follows, and the
argument checks that run before any device work."""
import numpy as np
import pytest

import __graft_entry__ as entry
from tests import regions_oracle as ro
from tests.golden import make_regions_exec as gen

FIXTURE = gen.load()
CASES = gen.case_names(FIXTURE)


def _agg(a, **kw):
    import xrspatial_amd as xs
    return xs.DataArray(a, dims=["y", "x"], **kw)


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference(case, n):
    a = FIXTURE[f"{case}/in"]
    labels, _ = ro.restated(a, n)
    want = FIXTURE[f"{case}/n{n}"]
    got = ro.as_output(labels, a)
    assert got.dtype == want.dtype
    assert np.array_equal(got, want, equal_nan=a.dtype.kind == "f")


def test_fixture_covers_what_the_spec_lists():
    dtypes = {FIXTURE[f"{c}/in"].dtype for c in CASES}
    assert dtypes == {np.dtype(t) for t in gen.INT_DTYPES} | {np.dtype(np.float64)}
    shapes = {FIXTURE[f"{c}/in"].shape for c in CASES}
    assert (1, 1) in shapes and any(s[0] == 1 and s[1] > 1 for s in shapes) and any(s[1] == 1 and s[0] > 1 for s in shapes)
    assert max(r * c for r, c in shapes) >= 90 * 90
    flat = np.concatenate([FIXTURE[f"{c}/in"].astype(np.float64).ravel() for c in CASES])
    assert np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any()
    # the reference's docstring example, with its gaps
    assert FIXTURE["doc_cross/n4"][:, 4].tolist() == [3, 3, 2, 6, 6]


def _random_exact(rng, dtype, shape):
    a = rng.integers(0, 3, shape)
    if np.dtype(dtype).kind == "f":
        a = a.astype(dtype)
        a[rng.random(shape) < 0.1] = np.nan
        return a
    return a.astype(dtype)


@pytest.mark.parametrize("n", [4, 8])
def test_fast_oracle_equals_the_restatement(n):
    rng = np.random.default_rng(11 + n)
    for t in range(60):
        dtype = (np.float64, np.float32, np.int32, np.uint8, np.int16)[t % 5]
        shape = tuple(int(s) for s in rng.integers(1, 24, 2))
        a = _random_exact(rng, dtype, shape)
        want, cw = ro.restated(a, n)
        got, cg = ro.fast_exact(a, n)
        assert cw == cg
        assert np.array_equal(want, got, equal_nan=True), (t, shape, dtype)


def _f64_match(v, w):
    return float(np.abs(np.float32(w - v))) <= 1e-08 + 1e-05 * float(abs(v))


def _f32_match(v, w):
    return bool(np.abs(np.float32(w - v)) <= np.float32(1e-08) + np.float32(1e-05) * np.abs(v))


def _typing_sensitive_pairs(k=2):
    """float32 (v, w) that form one region under one typing and two under the other (seeded search): whether either
    cell matches the other differs between Numba's float64 threshold and NumPy 2's float32 one."""
    rng = np.random.default_rng(2)
    found = []
    for v in rng.uniform(0.5, 5e4, 200000).astype(np.float32):
        t64 = 1e-08 + 1e-05 * float(abs(v))
        for s in (1, -1):
            w = np.float32(v + np.float32(s) * np.float32(t64))
            for ww in (w, np.nextafter(w, np.float32(np.inf)), np.nextafter(w, np.float32(-np.inf))):
                one64 = _f64_match(v, ww) or _f64_match(ww, v)
                one32 = _f32_match(v, ww) or _f32_match(ww, v)
                if one64 != one32:
                    found.append((np.float32(v), np.float32(ww)))
                    break
            if len(found) >= k:
                return found
    return found


TYPING_PAIRS = _typing_sensitive_pairs()


def test_float32_follows_numba_typing():
    assert len(TYPING_PAIRS) >= 2
    for v, w in TYPING_PAIRS:
        a = np.array([[v, w]], dtype=np.float32)
        numba, _ = ro.restated(a, 4)
        numpy2, _ = ro.restated(a, 4, typing="numpy")
        assert not np.array_equal(numba, numpy2)
        assert numba[0, 1] == (1.0 if _f64_match(v, w) or _f64_match(w, v) else 2.0)
    # a pair found by the same search: one region under Numba's typing, two under NumPy 2's
    a = np.array([[7470.702, 7470.6274]], dtype=np.float32)
    assert ro.restated(a, 4)[0].tolist() == [[1.0, 1.0]]
    assert ro.restated(a, 4, typing="numpy")[0].tolist() == [[1.0, 2.0]]


def test_argument_errors_come_before_device_work():
    import xrspatial_amd as xs
    agg = _agg(np.zeros((4, 4), np.float32))
    for n in (0, 3, 6, "4"):
        with pytest.raises(ValueError) as e:
            xs.regions(agg, neighborhood=n)
        assert str(e.value) == "`neighborhood` value must be either 4 or 8)"
    with pytest.raises(ValueError):
        xs.regions(xs.DataArray(np.zeros((2, 3, 4)), dims=["b", "y", "x"]))
    with pytest.raises(ValueError):
        xs.regions(xs.DataArray(np.zeros(5), dims=["x"]))
    for dt in (np.bool_, np.complex64, np.float16):
        with pytest.raises(TypeError):
            xs.regions(_agg(np.zeros((3, 3), dt)))
    assert xs.regions is xs.zonal.regions


def test_dask_backed_raster_is_refused(monkeypatch):
    import xrspatial_amd as xs
    from xrspatial_amd import utils
    from tests import fake_dask
    monkeypatch.setattr(utils, "da", fake_dask)
    lazy = _agg(fake_dask.from_array(np.zeros((8, 8)), (4, 4)))
    with pytest.raises(NotImplementedError, match="dask"):
        xs.regions(lazy)


def test_too_many_cells_are_refused_by_name():
    import xrspatial_amd as xs

    class Big:                                   # shape only: nothing may be allocated or read
        shape = (65536, 65536)
        ndim = 2
        dtype = np.dtype(np.uint8)

    with pytest.raises(ValueError, match="2\\*\\*32 - 1 cells"):
        xs.regions(_agg(Big()))


def test_no_gpu_raises_xrs_error():
    entry.build()
    import xrspatial_amd as xs
    if xs.has_hip():
        pytest.skip("a GPU is present")
    with pytest.raises(xs.XrsError):
        xs.regions(_agg(np.zeros((4, 4), np.uint8)))


def test_fma_sensitive_pairs_separate_the_roundings():
    pairs = ro.fma_sensitive_pairs()
    assert len(pairs) >= 4
    for v, w in pairs:
        d = abs(w - v)
        ref = d <= 1e-08 + 1e-05 * abs(v) or d <= 1e-08 + 1e-05 * abs(w)
        fused = d <= ro.fused_threshold(abs(v)) or d <= ro.fused_threshold(abs(w))
        assert ref != fused
        labels, _ = ro.restated(np.array([[v, w]]), 4)
        assert labels.tolist() == [[1.0, 1.0 if ref else 2.0]]

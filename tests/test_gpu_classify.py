"""xrspatial_amd.classify on the MI355X against the reference's own outputs (tests/golden/classify_exec.npz).

Tiers: binary, reclassify, equal_interval, quantile, percentiles, box_plot and maximum_breaks are bit-identical (output
digest = the reference's); std_mean and head_tail_breaks take their mean / std from float64 device sums, numpy from
float32 pairwise sums, so their bins agree to 1e-5 of max(|edge|, std) and a cell may differ only where it lies between
the two edges (the count is recorded in the parity log)."""
import numpy as np
import pytest

import xrspatial_amd as xs
from tests import classify_oracle as orc
from tests import parity_log
from tests.golden import make_classify_exec as cx

pytestmark = pytest.mark.gpu

EXACT = ("binary", "reclassify", "equal_interval", "quantile", "percentiles", "box_plot", "maximum_breaks")
TOLERANT = ("std_mean", "head_tail_breaks")
CASES = cx.cases()
FIX = cx.load()


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not xs.has_hip():
        pytest.fail("-m gpu needs an MI355X")


def _agg(a):
    return xs.DataArray(a, dims=["y", "x"], attrs={"res": (1.0, 1.0)}, name="r")


def _new_values(fn, kw, bins):
    return kw["new_values"] if fn == "reclassify" else np.arange(len(bins))


@pytest.mark.parametrize("fn", EXACT)
@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_exact_against_reference(case, fn):
    _, a, kws = next(c for c in CASES if c[0] == case)
    key = f"{case}/{fn}"
    call = getattr(xs.classify, fn)
    if key + "/exc" in FIX:
        with pytest.raises(Exception) as ei:
            call(_agg(a.copy()), **kws[fn])
        assert type(ei.value).__name__ == str(FIX[key + "/exc"])
        return
    before = a.copy()
    out = call(_agg(a), **kws[fn])
    np.testing.assert_array_equal(a, before)                       # the input is never modified
    got = np.asarray(out.data)
    assert got.dtype.str == str(FIX[key + "/dtype"]) and got.shape == a.shape
    if key + "/out" in FIX:
        np.testing.assert_array_equal(got, FIX[key + "/out"], err_msg=key)
    assert cx.digest(got) == str(FIX[key + "/sha"]), key
    assert out.name == fn


@pytest.mark.parametrize("fn", TOLERANT)
@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_moment_classifiers_against_reference(case, fn):
    _, a, kws = next(c for c in CASES if c[0] == case)
    key = f"{case}/{fn}"
    call = getattr(xs.classify, fn)
    if key + "/exc" in FIX:
        with pytest.raises(Exception) as ei:
            call(_agg(a.copy()))
        assert type(ei.value).__name__ == str(FIX[key + "/exc"])
        return
    ref_bins = FIX[key + "/bins"]
    got = np.asarray(call(_agg(a)).data)
    want = orc.bin_values(a, ref_bins, np.arange(len(ref_bins)))
    std = float(FIX[f"{case}/in/std"])
    # the GPU's bins: recover them from the output classes is not possible; compare the classes cell by cell instead
    diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    n_diff = int(diff.sum())
    if n_diff:
        x = a.astype(np.float64)[diff]
        cls = np.minimum(got[diff], want[diff]).astype(np.int64)        # the edge between the two classes
        edge = ref_bins[cls]
        scale = np.maximum(np.abs(edge), std if np.isfinite(std) else 0.0)
        assert np.all(np.abs(got[diff] - want[diff]) == 1), key        # neighbouring classes only
        assert np.all(np.abs(x - edge) <= 1e-5 * scale), key           # and only at an edge, within the tolerance
    parity_log.record("classify", f"{fn}:{case}", got, want, note=f"{n_diff} cells between the GPU and reference edges")


@pytest.mark.parametrize("fn", EXACT + TOLERANT)
def test_reference_test_vectors(fn):
    data = FIX["vec/input"]
    r = [FIX[k] for k in sorted(k for k in FIX if k.startswith(f"vec/{fn}/"))]
    if fn == "binary":
        out = xs.classify.binary(_agg(data), list(r[0]))
    elif fn == "reclassify":
        out = xs.classify.reclassify(_agg(data), bins=list(r[0]), new_values=list(r[1]))
    elif fn in ("quantile", "equal_interval"):
        out = getattr(xs.classify, fn)(_agg(data), k=int(r[0]))
    else:
        out = getattr(xs.classify, fn)(_agg(data))
    np.testing.assert_array_equal(np.asarray(out.data), r[-1].astype(np.asarray(out.data).dtype))


@pytest.mark.parametrize("case", [c[0] for c in CASES if f"{c[0]}/quantile/stdout" in FIX])
def test_quantile_prints_what_the_reference_prints(case, capsys):
    _, a, kws = next(c for c in CASES if c[0] == case)
    xs.classify.quantile(_agg(a), **kws["quantile"])
    assert capsys.readouterr().out == str(FIX[f"{case}/quantile/stdout"])


def test_radix_select_against_partition():
    from xrspatial_amd.classify import _Stats
    rng = np.random.default_rng(7)
    n = (1 << 24) + 7
    for dtype in (np.float32, np.float64):
        a = rng.normal(0, 1e3, n).astype(dtype)
        a[rng.random(n) < 0.3] = np.round(a[:1000])[rng.integers(0, 1000, 1)]     # heavy duplicates
        a[rng.integers(0, n, 5000)] = 0.0
        a[rng.integers(0, n, 5000)] = -0.0
        a[rng.integers(0, n, 3000)] = np.nan
        a[rng.integers(0, n, 3000)] = np.inf
        a[rng.integers(0, n, 3000)] = -np.inf
        fin = a[np.isfinite(a)]
        st = _Stats(xs.DeviceArray.from_numpy(a))
        assert st.count == fin.size
        ranks = np.unique(np.concatenate([[0, fin.size - 1, fin.size // 2], rng.integers(0, fin.size, 77)]))
        got = st.select(ranks)
        want = np.partition(fin, ranks)[ranks]
        np.testing.assert_array_equal(np.array([got[int(r)] for r in ranks], dtype=dtype), want)


def test_device_array_in_device_array_out_and_unchanged():
    rng = np.random.default_rng(3)
    a = rng.normal(0, 1, (257, 263)).astype(np.float32)
    a[5, 5] = np.nan
    dev = xs.DeviceArray.from_numpy(a)
    for fn, kw in (("quantile", {"k": 5}), ("binary", {"values": [a[1, 1]]}), ("reclassify", {"bins": [0, 1], "new_values": [1, 2]}),
                   ("equal_interval", {}), ("maximum_breaks", {}), ("std_mean", {}), ("head_tail_breaks", {}),
                   ("percentiles", {}), ("box_plot", {})):
        out = getattr(xs.classify, fn)(_agg(dev), **kw)
        assert isinstance(out.data, xs.DeviceArray), fn
        np.testing.assert_array_equal(out.data.get(), np.asarray(getattr(xs.classify, fn)(_agg(a), **kw).data))
        np.testing.assert_array_equal(dev.get(), a)


def test_dataset_in_dataset_out():
    rng = np.random.default_rng(4)
    ds = xs.Dataset({"a": _agg(rng.normal(0, 1, (40, 30)).astype(np.float32)),
                     "b": _agg(rng.normal(5, 2, (40, 30)))}, attrs={"t": 1})
    out = xs.classify.quantile(ds, k=4)
    assert isinstance(out, xs.Dataset) and list(out.data_vars) == ["a", "b"] and out.attrs == {"t": 1}
    for v in ("a", "b"):
        np.testing.assert_array_equal(np.asarray(out[v].data), np.asarray(xs.classify.quantile(ds[v], k=4).data))
        assert out[v].name == v


def test_large_percentiles_match_numpy():
    rng = np.random.default_rng(5)
    a = rng.gamma(2.0, 3.0, (8192, 8192)).astype(np.float32)
    a[::97, ::89] = np.nan
    dev = xs.DeviceArray.from_numpy(a)
    pct = [1, 10, 25, 50, 75, 90, 99]
    fin = a[np.isfinite(a)]
    want = np.percentile(fin, pct)
    from xrspatial_amd.classify import _Stats, percentile_from_order_stats
    st = _Stats(dev)
    got = percentile_from_order_stats(st.count, pct, np.float32, st.select)
    assert got.dtype == want.dtype
    np.testing.assert_array_equal(got, want)
    out = xs.classify.percentiles(_agg(dev), pct=pct).data.get()
    bins = np.sort(np.unique(np.append(np.unique(want), float(fin.max()))))
    np.testing.assert_array_equal(out, orc.bin_values(a, bins, np.arange(len(bins))))


def test_dask_backed_binary_and_reclassify_go_block_by_block(monkeypatch):
    from tests import fake_dask
    from xrspatial_amd import utils
    monkeypatch.setattr(utils, "da", fake_dask)
    rng = np.random.default_rng(6)
    a = rng.normal(10, 5, (45, 61)).astype(np.float32)
    a[3, 4], a[30, 50], a[10, 10] = np.nan, np.inf, 7.0
    lazy = _agg(fake_dask.from_array(a, (16, 20)))
    for fn, kw in (("binary", {"values": [7.0, np.inf]}), ("reclassify", {"bins": [5, 10, 15, np.inf], "new_values": [1, 2, 3, 4]})):
        out = getattr(xs.classify, fn)(lazy, **kw)
        assert isinstance(out.data, fake_dask.Array) and len(lazy.data.blocks_seen) > 1
        np.testing.assert_array_equal(out.data.compute(), np.asarray(getattr(xs.classify, fn)(_agg(a), **kw).data))
    with pytest.raises(NotImplementedError):
        xs.classify.quantile(lazy)

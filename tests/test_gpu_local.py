"""xrspatial_amd.local on the MI355X, through the public functions: every case of the executed reference
(tests/golden/local_exec.npz), NumPy- and DeviceArray-backed, and larger rasters against the rule (tests/local_oracle.py).

The kernels use +, -, *, /, sqrt (correctly rounded, no contraction) and comparisons only, in the order the rule writes down, so
every result equals the fixture and the rule exactly: NaN equals NaN, -0.0 equals 0.0, no tolerance."""
import numpy as np
import pytest

from tests import local_oracle as lo
from tests.golden import make_local_exec as gen

pytestmark = pytest.mark.gpu

FIXTURE = gen.load()
CASES = gen.names(FIXTURE)
FREQ = {"lesser_frequency": "lesser", "equal_frequency": "equal", "greater_frequency": "greater"}
POS = {"lowest_position": "lowest", "highest_position": "highest"}


@pytest.fixture(scope="module")
def xa():
    import xrspatial_amd
    from xrspatial_amd import _lib
    _lib.require_device()
    return xrspatial_amd


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got.astype(np.float64), want.astype(np.float64), equal_nan=True)


def where_not(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return (got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    return [(tuple(i), got[tuple(i)], want[tuple(i)]) for i in np.argwhere(bad)[:5].tolist()]


def dataset(xa, planes, refs, on_device):
    wrap = (lambda a: xa.DeviceArray.from_numpy(a)) if on_device else (lambda a: a.copy())
    names = [f"v{j:02d}" for j in range(len(planes))]
    variables = {name: xa.DataArray(wrap(p)) for name, p in zip(names, planes)}
    for k, r in refs.items():
        variables[k] = xa.DataArray(wrap(r))
    return xa.Dataset(variables), names


def host(res, on_device, xa):
    assert isinstance(res.data, xa.DeviceArray if on_device else np.ndarray)
    assert res.dims == ("dim_0", "dim_1") and not res.coords
    return res.data.get() if on_device else res.data


def run(xa, f, ds, names, on_device):
    loc = xa.local
    if f in lo.STATS:
        res = loc.cell_stats(ds, names, f)
    elif f in FREQ:
        res = getattr(loc, f)(ds, "ref_freq", names)
    elif f in POS:
        res = getattr(loc, f)(ds, names)
    elif f == "rank":
        res = loc.rank(ds, "ref_rank", names)
    else:
        res = loc.popularity(ds, "ref_pop", names)
    assert not res.attrs
    return host(res, on_device, xa)


def rule(f, planes, refs):
    if f in lo.STATS:
        return lo.cell_stats(planes, f)
    if f in FREQ:
        return lo.frequency(planes, refs["ref_freq"], FREQ[f])
    if f in POS:
        return lo.position(planes, POS[f])
    return lo.rank(planes, refs["ref_rank"]) if f == "rank" else lo.popularity(planes, refs["ref_pop"])


def check_key(key, want_values, planes):
    assert list(key.keys()) == list(range(1, len(want_values) + 1))
    for comb, want in zip(key.values(), want_values):
        assert len(comb) == len(planes)
        for v, w, p in zip(comb, want, planes):
            assert type(v) is (float if p.dtype.kind == "f" else int) and v == w, (comb, want)


# ------------------------------------------------------------------ the executed reference
@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("case", CASES)
def test_fixture_case(xa, case, on_device):
    st = gen.stored(FIXTURE, case)
    planes = gen.planes_of(FIXTURE, case)
    refs = {k: st[k] for k in ("ref_freq", "ref_rank", "ref_pop") if k in st}
    ds, names = dataset(xa, planes, refs, on_device)
    for row, f in enumerate(gen.functions_of(st)):
        got = run(xa, f, ds, names, on_device)
        assert got.dtype == lo.result_dtype(f.split("_")[0], [p.dtype for p in planes] + ([refs["ref_freq"].dtype] if f in FREQ else []))
        assert same(got, st["outputs"][row]), (f, where_not(got, st["outputs"][row]))
    n_vars = st["combine_key_values"].shape[1]
    res = xa.local.combine(ds, names[:n_vars])
    assert set(res.attrs) == {"key"}
    got = host(res, on_device, xa)
    assert got.dtype == np.float64 and same(got, st["combine"]), where_not(got, st["combine"])
    check_key(res.attrs["key"], st["combine_key_values"].tolist(), planes[:n_vars])


# ------------------------------------------------------------------ larger rasters against the rule
def planes_for(kind, n, shape, rng):
    """full-mantissa floats ('f32', 'f64'), values from a small set ('sets', 'i32', 'i64'), or a mix of dtypes"""
    if kind in ("f32", "f64"):
        out = [rng.normal(scale=50.0, size=shape).astype(kind.replace("f", "float")) for _ in range(n)]
    elif kind == "sets":
        out = [rng.integers(-1, 3, shape).astype(np.float32) * 0.5 for _ in range(n)]
    elif kind == "i32":
        out = [rng.integers(-2, 3, shape).astype(np.int32) for _ in range(n)]
    elif kind == "i64":
        out = [rng.integers(-2, 3, shape).astype(np.int64) * (2 ** 61) for _ in range(n)]
    else:
        dtypes = (np.float32, np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.float64)
        out = [rng.integers(0, 4, shape).astype(dtypes[j % len(dtypes)]) for j in range(n)]
    floats = [p for p in out if p.dtype.kind == "f"]
    if floats:
        for p in floats[:3]:
            p[rng.random(shape) < 0.02] = np.nan
        floats[0][rng.random(shape) < 0.05] = -0.0
    return out


BIG = [((5, 1031), 5, "f32"), ((5, 1031), 64, "f64"), ((5, 1031), 64, "sets"), ((5, 1031), 64, "i32"), ((257, 300), 3, "mixed"),
       ((257, 300), 8, "sets"), ((257, 300), 9, "f64"), ((257, 300), 16, "i64"), ((257, 300), 17, "sets"), ((5, 1031), 1, "f32"),
       ((5, 1031), 12, "mixed"), ((5, 1031), 4, "i32"), ((257, 300), 23, "f32")]


@pytest.mark.parametrize("shape, n, kind", BIG, ids=[f"{s[0]}x{s[1]}_n{n}_{k}" for s, n, k in BIG])
def test_against_the_rule(xa, shape, n, kind):
    rng = np.random.default_rng(n * 1000 + shape[0])
    planes = planes_for(kind, n, shape, rng)
    like = planes[rng.integers(0, n)]
    ref_int = np.uint8 if kind == "mixed" else np.int64 if kind == "i64" else np.int32
    refs = {"ref_freq": like.copy() if kind != "f64" else like.astype(np.float32),         # float32 ref against float64 data
            # 1 .. n, beyond n, 0 and the wrap range, and below it, where the result is NaN
            "ref_rank": rng.integers(0 if kind == "mixed" else -n - 3, n + 4, shape).astype(ref_int)}
    refs["ref_pop"] = rng.integers(0 if kind == "mixed" else -7, 8, shape).astype(ref_int)
    ds, names = dataset(xa, planes, refs, True)
    for f in gen.functions_of(refs):
        got = run(xa, f, ds, names, True)
        want = rule(f, planes, refs)
        assert got.dtype == want.dtype, f
        assert same(got, want), (f, where_not(got, want))
    if kind != "mixed":
        below = refs["ref_rank"] < 1 - n
        assert below.any() and np.isnan(run(xa, "rank", ds, names, True)[below]).all()


def check_combine(xa, planes, on_device=True):
    ds, names = dataset(xa, planes, {}, on_device)
    res = xa.local.combine(ds)
    got = host(res, on_device, xa)
    ids, key = lo.combine(planes)
    assert same(got, ids), where_not(got, ids)
    check_key(res.attrs["key"], [list(v) for v in key.values()], planes)
    return got, res.attrs["key"]


@pytest.mark.parametrize("shape, n, kind", [((5, 1031), 3, "sets"), ((257, 300), 4, "mixed"), ((257, 300), 2, "i64"),
                                             ((5, 1031), 64, "i32"), ((9, 11), 2, "f64")])
def test_combine_against_the_rule(xa, shape, n, kind):
    rng = np.random.default_rng(n + shape[1])
    planes = planes_for(kind, n, shape, rng)
    if n == 64:                                          # 64 planes, a few hundred classes: most planes repeat another
        planes = [planes[j % 3] if j % 7 else planes[j] for j in range(n)]
    check_combine(xa, planes)


def test_combine_all_nan(xa):
    got, key = check_combine(xa, [np.full((7, 9), np.nan, np.float32), np.ones((7, 9), np.int32)])
    assert np.isnan(got).all() and key == {}
    got, key = check_combine(xa, [np.full((7, 9), np.nan)], on_device=False)
    assert np.isnan(got).all() and key == {}


def test_combine_every_cell_its_own_class(xa):
    rng = np.random.default_rng(3)
    a = rng.permutation(64 * 64).reshape(64, 64)
    got, key = check_combine(xa, [(a // 64).astype(np.int16), (a % 64).astype(np.float64)])
    assert np.array_equal(got, np.arange(1, 64 * 64 + 1, dtype=np.float64).reshape(64, 64)) and len(key) == 64 * 64


def test_combine_first_class_reappears_in_the_last_cell(xa):
    a = np.arange(1, 1 + 33 * 65, dtype=np.int32).reshape(33, 65) % 50 + 1
    b = (np.arange(33 * 65).reshape(33, 65) % 3).astype(np.float32)
    a[-1, -1], b[-1, -1] = a[0, 0], -0.0                 # (b[0, 0] is 0.0: the same tuple under ==)
    got, key = check_combine(xa, [a, b])
    assert got[0, 0] == 1 and got[-1, -1] == 1 and key[1] == (int(a[0, 0]), 0.0)

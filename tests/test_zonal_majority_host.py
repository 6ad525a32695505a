"""No GPU: the cases of tests/zonal_majority_cases.py reach the paths of zonal_mode.hip / zonal_majority.hip they are named
for, by the CPU model of the plan and the hashes; their references are well defined; the adversarial generator's keys land
in the part they were made for; and zonal.zonal_majority takes the sort exactly when the double behind the zones is not 0."""
import numpy as np
import pytest

from tests import zonal_majority_cases as mc

VTYPES = [np.float32, np.float64]
vt_ids = lambda d: np.dtype(d).name  # noqa: E731


def _check(case):
    """The model of `case`, after the checks every case gets."""
    m = mc.model(case)
    want = case.want()
    ok = mc.valid_mask(case.z.ravel(), case.v.ravel(), case.nz, case.nodata)
    assert m.n_valid == int(ok.sum()) and m.n_parts == int((1 << m.B).sum()), case.name
    assert m.part_len.sum() == m.n_valid, case.name
    np.testing.assert_array_equal(np.isnan(want), m.counts == 0, err_msg=case.name)
    for zone, w in case.winners.items():
        np.testing.assert_array_equal(want[zone], w, err_msg=f"{case.name} zone {zone}")
    e = case.expect
    if "B" in e:
        assert m.B.tolist() == list(e["B"]), case.name
    if "n_chunks" in e:
        assert m.n_chunks == e["n_chunks"], case.name
    if "batches" in e:
        assert m.batches == e["batches"], case.name
    assert m.n_direct == e.get("n_direct", 0), case.name
    assert m.overflow == e.get("overflow", False), (case.name, int(m.table_keys.max()))
    return m


# ------------------------------------------------------------------------------------------- the model itself
def test_hashes_in_python_integers():
    """The NumPy hashes against the same formulas in Python's unbounded integers."""
    rng = np.random.default_rng(1)

    def mix(h):
        h ^= h >> 16
        h = h * 0x85ebca6b & 0xffffffff
        h ^= h >> 13
        h = h * 0xc2b2ae35 & 0xffffffff
        h ^= h >> 16
        return h & (mc.SLOTS - 1)

    for w, U in ((32, np.uint32), (64, np.uint64)):
        keys = rng.integers(0, (1 << w) - 1, 200, dtype=np.uint64, endpoint=True).astype(U)
        fold = (lambda k: k) if w == 32 else (lambda k: (k ^ (k >> 29) ^ (k >> 47)) & 0xffffffff)
        for B in (1, 3, 11, 12, 16):
            assert mc.part_of(keys, B).tolist() == [(int(k) * mc.MULT[w] % (1 << w)) >> (w - B) for k in keys]
        assert (mc.part_of(keys, 0) == 0).all()
        assert mc.sieve_slot(keys).tolist() == [mix(fold(int(k))) for k in keys]
        rot = [((int(k) << 15 | int(k) >> (w - 15)) & ((1 << w) - 1)) ^ mc.TABLE_XOR for k in keys]
        assert mc.table_slot(keys).tolist() == [mix(fold(r)) for r in rot]
        assert mc.MULT[w] % 2 == 1 and mc.MULT[w] * pow(mc.MULT[w], -1, 1 << w) % (1 << w) == 1


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_keys_order_as_values_and_decode_back(dtype):
    fi = np.finfo(dtype)
    v = np.array([-np.inf, -fi.max, -1.5, -fi.tiny, -fi.smallest_subnormal, -0.0, 0.0, fi.smallest_subnormal, fi.tiny, 0.25, fi.max,
                  np.inf], dtype=dtype)
    k = mc.enc(v)
    assert (np.diff(k.astype(object)) > 0).all()                    # (-0.0 below +0.0: the grouping entry point keeps both)
    np.testing.assert_array_equal(mc.dec(k, dtype), v.astype(np.float64))
    assert np.signbit(mc.dec(k, dtype)[5]) and not np.signbit(mc.dec(k, dtype)[6])
    assert mc.enc(mc.canon(v))[5] == k[6]
    assert (k != np.iinfo(k.dtype).max).all()                       # all-ones is count_kernel's EMPTY: a NaN's key only


def test_parts_log2_boundaries():
    got = {c: mc.parts_log2(c) for c in (0, 1, 1280, 1281, 2048, 2049, 4096, 4097, 262_144, 262_145, 2_097_152, 2_097_153,
                                         1 << 26, (1 << 26) + 1, 1 << 31)}
    assert got == {0: 0, 1: 0, 1280: 0, 1281: 1, 2048: 1, 2049: 2, 4096: 2, 4097: 3, 262_144: 8, 262_145: 9, 2_097_152: 11,
                   2_097_153: 12, 1 << 26: 16, (1 << 26) + 1: 16, 1 << 31: 16}
    assert mc.CHUNK == 512 * 16 and mc.TILE == 256 * 16 and mc.MAX_ZONES * 4 == 64 * 1024


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_adversarial_keys_land_in_their_part(dtype):
    rng = np.random.default_rng(2)
    tiny = np.finfo(dtype).tiny
    for B, part, m in ((0, 0, 50), (1, 1, 500), (2, 1, 3000), (3, 0, 6000), (7, 77, 1100), (12, 4095, 300), (16, 40_000, 64)):
        v = mc.keys_in_part(dtype, B, part, m, rng)
        assert v.dtype == dtype and v.size == m and np.unique(v).size == m
        assert np.isfinite(v).all() and (np.abs(v) >= tiny).all()
        assert (mc.part_of(mc.enc(mc.canon(v)), B) == part).all(), (B, part)


# --------------------------------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_small_cases_reach_their_paths(dtype):
    by_name = {}
    for case in mc.small_cases(dtype):
        assert case.v.dtype == dtype and case.z.dtype == np.int32 and case.name not in by_name
        by_name[case.name] = (case, _check(case))
    assert tuple(by_name) == mc.SMALL_NAMES
    case, m = by_name["uncut zones"]
    assert m.counts.tolist() == [1, 63, 1024, 0, 1025, 1280] and m.part_len.tolist() == m.counts.tolist()
    case, m = by_name["B boundaries"]
    assert m.counts.tolist() == [1281, 2048, 2049, 4096, 4097]
    case, m = by_name["many chunks"]
    assert m.counts[1] % mc.CHUNK == 5 and m.n_chunks % 8 != 0
    case, m = by_name["B = 9"]
    assert m.n_parts == 513 and m.counts[0] == (mc.PART_TARGET << 8) + 1
    case, m = by_name[f"nz={mc.MAX_ZONES}"]
    assert case.nz == mc.MAX_ZONES and (m.B == 0).all() and (m.counts == 0).sum() > 100 and m.counts.max() > 2
    for late in (0, 1):
        case, m = by_name["dominated part" + (", winner late" if late else "")]
        w = np.asarray(case.winners[0], dtype)
        part = int(mc.part_of(mc.enc(w[None]), 7)[0])
        assert m.part_len[part] > 60_000 and m.batches >= 59
        assert (m.table_keys <= mc.SLOTS).all()
        if late:                                                     # the zone's first 1024 cells: the winner's part, not the winner
            head = case.v[:case.expect["late"]]
            assert head.size >= mc.BATCH and (mc.part_of(mc.enc(head), 7) == part).all() and (head != w).all()
            assert (case.z[:head.size] == 0).all()
    case, m = by_name[f"sieve against table, {mc.SLOTS} keys"]
    assert m.table_keys[case.expect["part"]] == mc.SLOTS and m.table_keys.max() == mc.SLOTS and m.batches == 3
    case, m = by_name["ties"]
    assert sorted(set(m.B.tolist())) == [0, 2, 3] and m.batches == 2
    pairs = [z for z in range(case.nz) if m.counts[z] == 1024 and z > 5]
    assert len(pairs) == 8
    # every valid value of the all-tie zones occurs as often as the winner
    for zone in (5, 6, 7, 8, pairs[0], case.nz - 1):
        vals = case.v[(case.z == zone) & np.isfinite(case.v)]
        assert np.unique(np.unique(vals, return_counts=True)[1]).size == 1 and vals.min() == case.winners[zone]
    case, m = by_name["run votes"]
    ok = mc.valid_mask(case.z, case.v, case.nz)
    runs = np.unique(np.stack([case.z[ok].astype(np.float64), case.v[ok].astype(np.float64)]), axis=1).shape[1]
    first_two = np.unique(case.v[case.z == 0]).size + np.unique(case.v[case.z == 1]).size
    assert runs > mc.VOTE_BLOCK and first_two < mc.VOTE_PER          # (3 + 4 runs: thread 0 crosses two zone changes)
    for n in mc.WAVE_N:
        case, m = by_name[f"wave paths n={n}"]
        assert case.n == n
    case = by_name["wave paths n=4097"][0]
    lead = case.z.reshape(-1)[64:128]
    assert np.isnan(case.v[64]) and case.v[65] == case.nodata and lead[2] == case.nz and (lead[3:] == lead[3]).all()
    assert (case.z[:64] == case.z[0]).all() and np.unique(case.z[-64:]).size == case.nz
    for nz in mc.SORT_NZ:
        case, m = by_name[f"sort nz={nz}"]
        assert (case.z == nz).any() and (case.z == -1).any() and (m.counts > 0).all()


@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_overflow_cases_must_overflow(dtype):
    over, skewed = mc.overflow_cases(dtype)
    m = _check(over)
    assert m.table_keys[over.expect["part"]] == mc.SLOTS + 1 and np.sort(m.table_keys)[-2] < mc.SLOTS
    m = _check(skewed)
    assert m.part_len[0] == 6001 and m.table_keys[0] > 2 * mc.SLOTS and m.counts[0] < 1 << 13
    # every value of these rasters is a normal number: no flush mode changes a key
    for case in (over, skewed):
        assert (np.abs(case.v) >= np.finfo(dtype).tiny).all() and np.isfinite(case.v).all()


@pytest.mark.parametrize("nz", mc.SCAN_NZ)
def test_plan_scan_cases(nz):
    case = mc.scan_carry_case(np.float32, nz)
    m = _check(case)
    assert m.n_parts == nz + int((m.B == 1).sum()) and m.n_chunks == int((m.B == 1).sum())
    if nz > 1024:                            # a carry in every scan (cells, parts, chunks), and zones behind the trip to take it
        assert m.counts[:1024].sum() > 0 and m.B[:1024].sum() > 0 and m.counts.size > 1024


@pytest.mark.parametrize("direct", [0, 1])
def test_lds_b_against_direct(direct):
    case = mc.lds_b_case(np.float32, direct)
    m = _check(case)
    assert m.counts[1] == (mc.PART_TARGET << mc.LDS_B) + direct and case.n > mc.PART_TARGET << mc.LDS_B
    assert (m.table_keys <= mc.SLOTS).all()


def test_persistent_count_loop_case():
    case = mc.persistent_case(np.float32)
    m = _check(case)
    tiles = -(-case.n // mc.TILE)
    assert tiles == mc.COUNT_GRID + 2 and case.n % mc.TILE == 1
    assert m.table_keys.max() <= 7 and m.n_chunks == sum(-(-int(c) // mc.CHUNK) for c in m.counts)


# ------------------------------------------------------------------------------- Python's choice of the path
class _Stub:
    """_lib.call in the style of tests/fake_hip.py: memory calls go to the emulation; the two majority entry points write
    recognisable results, the hash path with `overflow` behind them."""

    def __init__(self, overflow):
        from tests import fake_hip
        self.fake, self.overflow, self.calls = fake_hip, overflow, []

    def __call__(self, name, *a):
        if name.startswith("xrs_zonal_mode_f"):
            self.calls.append(name)
            nz, out = a[3], a[9]
            self.fake._arr(out, nz + 1, np.float64)[...] = np.append(np.arange(nz) + 100.0, self.overflow)
        elif name.startswith("xrs_zonal_majority_f"):
            self.calls.append(name)
            nz, out = a[3], a[8]
            self.fake._arr(out, nz, np.float64)[...] = np.arange(nz) + 200.0
        else:
            self.fake.call(name, *a)


@pytest.mark.parametrize("overflow", [0.0, 1.0, 3.0, 256.0])
@pytest.mark.parametrize("dtype", VTYPES, ids=vt_ids)
def test_python_sorts_exactly_when_the_last_double_is_nonzero(monkeypatch, dtype, overflow):
    from tests import fake_hip
    from xrspatial_amd import _lib, zonal
    fake_hip.install(monkeypatch)
    monkeypatch.setenv("XRS_ZONAL_MAJORITY", "hash")
    stub = _Stub(overflow)
    monkeypatch.setattr(_lib, "call", stub)
    z = np.array([0, 1, 2, 1], np.int32)
    v = np.array([0.5, 1.5, 2.5, 3.5], dtype)
    sfx = "f64" if dtype == np.float64 else "f32"
    for counts in (None, np.array([1, 2, 1], np.uint64)):
        stub.calls.clear()
        got = zonal.zonal_majority(z, v, 3, counts=counts)
        if overflow:
            assert stub.calls == ["xrs_zonal_mode_" + sfx, "xrs_zonal_majority_" + sfx] and got.tolist() == [200.0, 201.0, 202.0]
        else:
            assert stub.calls == ["xrs_zonal_mode_" + sfx] and got.tolist() == [100.0, 101.0, 102.0]
    # more zones than the hash path takes, and the sort asked for: the hash path is not called at all
    stub.calls.clear()
    got = zonal.zonal_majority(z, v, mc.MAX_ZONES + 1)
    assert stub.calls == ["xrs_zonal_majority_" + sfx] and got.size == mc.MAX_ZONES + 1
    monkeypatch.setenv("XRS_ZONAL_MAJORITY", "sort")
    stub.calls.clear()
    assert zonal.zonal_majority(z, v, 3).tolist() == [200.0, 201.0, 202.0] and stub.calls == ["xrs_zonal_majority_" + sfx]

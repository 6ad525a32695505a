"""CPU proof that the cases of tests/local_cases.py are what their `reaches` tags claim, from the data and the oracle alone: the
(function, working type, holder) triples and the load paths of section A, the padding value as data in C, the dtype extremes
in D, the unsigned-zero wrap in G, the exact class counts in H, the share of cells whose expected value is a number, and the
mapping of the issue's nine gaps to named cases.  No GPU; tests/test_gpu_local_abi.py runs the same cases on the device."""
import time

import numpy as np
import pytest

from tests import local_cases as lc
from tests import local_oracle as lo

F64, I64 = np.dtype(np.float64), np.dtype(np.int64)

# the nine gaps the table was written to close, each with the cases that close it (name prefixes)
GAPS = {
    "1 as_out (double)r": ["B_big_n05_out0", "B_small_n03_out0", "B_small_n09_out0"],
    "2 padding equal to data": [f"C_{k}_n{n:02d}_{op}" for k in ("f64", "i64") for n in (3, 5, 7, 9, 15) for op in lc.VALUES_OPS],
    "3 plane-count boundaries": [f"A_{k}_n{n:02d}_" for k in ("ints", "floats") for n in (2, 6, 7, 15, 24, 63)],
    "4 dtype extremes": [f"D_{dt}_c{c}_" for dt in lc.PLANE_DTYPES for c in (7, 8)],
    "5 cell counts": [f"E_c{c:04d}_" for c in lc.CELL_COUNTS],
    "6 element-aligned pointers": [f"F_{dt}_offset1" for dt in lc.F_DTYPES],
    "7 ref_minus_one": [f"G_{dt}_n{n:02d}_{op}" for dt in ("uint16", "uint32", "int8", "int16") for n in (5, 20) for op in ("rank", "popularity")],
    "8 combine sort bit ranges": [f"H_top_{dt}_{k}" for dt in lc.PLANE_DTYPES for k in (1, 2)] + [f"H_count_{c:05d}" for c in lc.CLASS_COUNTS]
    + ["H_three_planes", "H_four_planes"],
    "9 first cells and gather": ["H_nan_cell0", "H_nan_last_plane", "H_single_cell", "H_all_equal", "H_top_int8_2", "H_top_float32_2"],
}


@pytest.fixture(scope="module")
def table():
    return lc.by_name()


def section(table, letter):
    return [c for c in table.values() if c["name"][0] == letter]


def stacked(c, op):
    """the cell values in the working type of `op`: (planes, cells)"""
    return np.stack([p.astype(lc.working(c, op)) for p in c["planes"]])


def test_every_gap_maps_to_named_cases(table):
    for gap, prefixes in GAPS.items():
        for prefix in prefixes:
            assert any(name.startswith(prefix) for name in table), (gap, prefix)
    assert all(c["reaches"] and c["name"][0] in "ABCDEFGH" for c in table.values())
    assert {c["name"][0] for c in table.values()} == set("ABCDEFGH")


def test_the_table_evaluates_in_under_a_minute(table):
    start = time.perf_counter()
    for c in table.values():
        if c["ops"] == ("combine",):
            lc.expected_combine(c)
        else:
            for op in c["ops"]:
                assert lc.expected(c, op).shape == c["planes"][0].shape
    assert time.perf_counter() - start < 60.0
    assert max(c["planes"][0].size for c in table.values()) <= 65537 + 100 and max(len(c["planes"]) for c in table.values()) == 64


# ------------------------------------------------------------------------------------------------ A
def test_a_has_every_function_working_type_and_holder(table):
    a = section(table, "A")
    assert sorted({len(c["planes"]) for c in a}) == list(lc.COUNTS)
    values = {(op, lc.working(c, op).name, lc.holder(len(c["planes"]))) for c in a for op in c["ops"] if op in lc.VALUES_OPS}
    want = {("median", "float64", h) for h in (4, 8, 16, "lds")}
    want |= {(op, w, h) for op in ("rank", "popularity") for w in ("int64", "float64") for h in (4, 8, 16, "lds")}
    assert values == want
    stream = {(op, lc.working(c, op).name, lc.pairwise_branch(len(c["planes"]))) for c in a for op in c["ops"] if op not in lc.VALUES_OPS}
    want = {(op, "float64", b) for op in lc.STREAM_NO_REF + lc.FREQ for b in ("<8", "8", "8k", "8k+r")}
    want |= {(op, "int64", b) for op in lc.INT_STREAM for b in ("<8", "8", "8k", "8k+r")}
    assert stream == want
    assert set(lc.OPS) == {op for c in a for op in c["ops"]} and len(lc.OPS) == 13
    for c in a:                                          # cell counts: one past a block of the kernel the case runs
        n, cells = len(c["planes"]), c["planes"][0].size
        assert cells == (lc.STREAM_CELLS if c["ops"][0] not in lc.VALUES_OPS else lc.REG_CELLS if n <= 16 else lc.LDS_CELLS)


def test_a_takes_every_load_path_of_ld2_in_both_states(table):
    """(plane dtype, working type, pair or single-cell tail): all nine dtypes into float64, the seven integer ones into int64;
    an odd cell count ends in the tail, two cells or more start with a pair.  The ref plane goes through ld2 too."""
    seen = set()
    for c in section(table, "A"):
        cells = c["planes"][0].size
        for op in c["ops"]:
            if op in lc.VALUES_OPS:
                continue
            through = [p.dtype for p in c["planes"]] + ([c["ref"].dtype] if op in lc.FREQ else [])
            for dt in through:
                seen |= {(dt.name, lc.working(c, op).name, two) for two in ([True] if cells >= 2 else []) + ([False] if cells % 2 else [])}
    want = {(dt.name, "float64", two) for dt in lc.PLANE_DTYPES for two in (True, False)}
    want |= {(dt.name, "int64", two) for dt in lc.INTS for two in (True, False)}
    assert seen == want
    ref_dtypes = {c["ref"].dtype.name for c in section(table, "A") if c["ops"] == lc.FREQ}
    assert ref_dtypes == {dt.name for dt in lc.PLANE_DTYPES}


def test_a_data_is_what_the_sections_ask_for(table):
    for c in section(table, "A"):
        kinds = {p.dtype.kind for p in c["planes"]}
        if "_ints_" in c["name"]:
            assert kinds <= {"i", "u"} and [p.dtype for p in c["planes"]] == [lc.INTS[j % 7] for j in range(len(c["planes"]))]
            assert all(np.abs(p.astype(np.int64)).max() <= 3 for p in c["planes"])
        else:
            assert "f" in kinds
            floats = np.stack([p.astype(np.float64) for p in c["planes"] if p.dtype.kind == "f"])
            nan_cells = int(np.isnan(floats).any(axis=0).sum())
            assert nan_cells == max(1, round(0.02 * floats.shape[1])), c["name"]         # 2 % of the cells
            assert (np.signbit(floats) & (floats == 0)).any(), c["name"]
            if c["ops"] != ("popularity",):              # full mantissas: the low bits of the float64 values are in use
                f64 = [p for p in c["planes"] if p.dtype == F64]
                assert not f64 or (np.concatenate(f64).view(np.uint64) & np.uint64(0xff)).astype(bool).mean() > 0.9


def test_rank_and_popularity_refs_span_the_range_and_beyond(table):
    for c in section(table, "A") + section(table, "C"):
        n = len(c["planes"])
        ref = c["ref"].astype(np.int64) if c["ops"][0] in ("rank", "popularity") else None
        if c["ops"] == ("rank",):
            assert ref.min() == -n - 3 and ref.max() == n + 3, c["name"]
        if c["ops"] == ("popularity",):
            u = lo.distinct(c["planes"], (c["ref"].dtype,))
            assert (ref + u).min() == -2 and (ref - u).max() == 2, c["name"]
            if n >= 3:
                assert (u < n).any() and (u > 1).any(), c["name"]


def test_enough_expected_cells_are_numbers(table):
    """An all-NaN expectation would let a kernel that sorts wrongly pass.  Popularity over one plane is NaN by the rule
    (u = n = 1, "NaN if ... u >= n"): that case keeps its place in the table and is the one exception."""
    for c in table.values():
        for op in c["ops"]:
            if op not in lc.VALUES_OPS:
                continue
            numbers = 1.0 - np.isnan(lc.expected(c, op)).mean()
            if op == "popularity" and len(c["planes"]) == 1:
                assert numbers == 0.0
                continue
            assert numbers >= (0.9 if op == "median" else 0.4), (c["name"], op, numbers)


# ------------------------------------------------------------------------------------------------ B
def test_b_conversions_round_and_the_planes_are_shared(table):
    big0, big1 = table["B_big_n05_out0"], table["B_big_n05_out1"]
    assert big0["out_is_i64"] == 0 and big1["out_is_i64"] == 1
    assert all(np.array_equal(p, q) for p, q in zip(big0["planes"], big1["planes"]))
    for op in ("max", "min", "sum"):
        exact, as_f64 = lc.expected(big1, op), lc.expected(big0, op)
        assert exact.dtype == I64 and as_f64.dtype == F64 and lc.out_i64(big1, op) == 1 and lc.out_i64(big0, op) == 0
        assert np.array_equal(as_f64, exact.astype(np.float64))
        inexact = [int(f) != i for f, i in zip(as_f64.tolist(), exact.tolist())]
        assert sum(inexact) > 50, op                                    # the conversion rounds in many cells
    wide = np.stack([p.astype(object) for p in big0["planes"]]).sum(axis=0)
    assert any(not -2 ** 63 <= int(v) < 2 ** 63 for v in wide)         # the int64 sum wraps somewhere
    small = [c for c in section(table, "B") if "small" in c["name"]]
    assert {c["ops"] for c in small} == {lc.INT_STREAM} and {(len(c["planes"]), c["out_is_i64"]) for c in small} == {(3, 0), (3, 1), (9, 0), (9, 1)}
    assert all(p.dtype.kind in "iu" for c in section(table, "B") for p in c["planes"] + [c["ref"]] if p is not None)


# ------------------------------------------------------------------------------------------------ C
def test_c_puts_the_padding_value_into_cells_with_free_slots(table):
    seen = set()
    for c in section(table, "C"):
        n, op = len(c["planes"]), c["ops"][0]
        seen.add((c["name"].split("_")[1], n, op))
        v = stacked(c, op)
        largest = np.inf if "_f64_" in c["name"] else v.dtype.type(lc.I64_MAX)      # (2^63 in the float64 median)
        times = (v == largest).sum(axis=0)
        assert {0, 1, 2, n} <= set(times.tolist()), c["name"]
        assert (v == (-np.inf if "_f64_" in c["name"] else v.dtype.type(lc.I64_MIN))).any()
        if n <= 16:
            assert n < lc.holder(n)                                     # slots n .. N - 1 are padding
        else:
            assert lc.holder(n) == "lds"
        if op != "median":
            assert v.dtype == (F64 if "_f64_" in c["name"] else I64)
            got = lc.expected(c, op)                                    # the padding value is a possible RESULT, too
            assert (got == float(largest)).any() and (~np.isnan(got) & (got != float(largest))).any(), c["name"]
    assert seen == {(k, n, op) for k in ("f64", "i64") for n in lc.C_COUNTS for op in lc.VALUES_OPS}


# ------------------------------------------------------------------------------------------------ D
def test_d_holds_every_extreme_of_every_dtype(table):
    seen = set()
    for c in section(table, "D"):
        dt = c["planes"][0].dtype
        assert len(c["planes"]) == 3 and all(p.dtype == dt for p in c["planes"])
        cells = c["planes"][0].size
        seen.add((dt.name, cells, c["ops"]))
        held = np.concatenate(c["planes"])
        e = lc.extremes(dt)
        assert all(lc._same_bits(held, x).any() for x in e), c["name"]
        info = np.finfo(dt) if dt.kind == "f" else np.iinfo(dt)
        assert e.min() == (-np.inf if dt.kind == "f" else info.min) and e.max() == (np.inf if dt.kind == "f" else info.max)
        assert info.max in e and info.min in e
        if cells % 2:                                                   # the single-cell tail reads the two ends of the dtype
            last = [p[-1] for p in c["planes"]]
            assert e.min() in last and e.max() in last
        if c["ref"] is not None and c["ops"] == ("equal",):
            assert c["ref"].dtype == dt
    ops = {("max", "min", "sum", "lowest", "highest"), ("equal",), ("median",), ("rank",)}
    assert seen == {(dt.name, cells, o) for dt in lc.PLANE_DTYPES for cells in (7, 8) for o in ops}


def test_no_int64_beyond_2_53_next_to_a_float_where_the_rule_is_inexact(table):
    for c in table.values():
        for op in set(c["ops"]) & set(lc.FREQ + ("lowest", "highest", "rank")):
            through = c["planes"] + ([c["ref"]] if op in lc.FREQ else [])
            if any(p.dtype.kind == "f" for p in through):
                assert all(np.abs(p.astype(object)).max() <= 2 ** 53 for p in through if p.dtype == I64), (c["name"], op)


# ------------------------------------------------------------------------------------------------ E, F
def test_e_and_f_shapes(table):
    e = section(table, "E")
    assert sorted({c["planes"][0].size for c in e}) == list(lc.CELL_COUNTS)
    assert {(len(c["planes"]), c["planes"][0].dtype.name, c["ops"]) for c in e} == {(3, "float32", ("sum", "median")), (20, "int32", ("rank",))}
    f = section(table, "F")
    assert {c["planes"][0].dtype for c in f} == set(lc.F_DTYPES) and all(c["offset"] == 1 and c["ref"].dtype == c["planes"][0].dtype for c in f)
    assert all(c["ops"] == ("max", "sum", "std", "greater") and c["planes"][0].size == 513 for c in f)
    assert all(c["offset"] == 0 for c in table.values() if c["name"][0] != "F")
    u32 = table["F_uint32_offset1"]["planes"]
    assert max(p.max() for p in u32) >= 2 ** 31                         # the packed u2u load, unsigned


# ------------------------------------------------------------------------------------------------ G
def test_g_refs_and_the_unsigned_zero(table):
    seen = set()
    for c in section(table, "G"):
        dt, n, op = c["ref"].dtype, len(c["planes"]), c["ops"][0]
        seen.add((dt.name, n, op))
        info = np.iinfo(dt)
        special = lc.g_specials(dt, n)
        assert c["ref"][:len(special)].tolist() == special and {0, 1, n, n + 1, info.min, info.max} <= set(special)
        assert dt.kind == "u" or {-n, -n - 1} <= set(special)
        got = lc.expected(c, op)
        assert c["ref"][0] == 0
        if dt.kind == "u":
            assert np.isnan(got[0])                                     # 0 - 1 wraps to the dtype's maximum: out of range
        else:                                                           # k = -1: Python's "last element"
            want = max(p[0] for p in c["planes"])
            assert got[0] == want
        assert got[1] == min(p[1] for p in c["planes"])                 # ref 1: the smallest
        assert (lo.distinct(c["planes"]) == 3).all()
    assert seen == {(dt.name, n, op) for dt in lc.INTS for n in (5, 20) for op in ("rank", "popularity")}


# ------------------------------------------------------------------------------------------------ H
def classes_after(c, k):
    return len(lo.combine(c["planes"][:k])[1])


def test_h_class_counts_are_exact(table):
    for count in lc.CLASS_COUNTS:
        c = table[f"H_count_{count:05d}"]
        assert classes_after(c, 1) == count and classes_after(c, 2) > count and c["planes"][0].size <= 65537 + 100
    assert [classes_after(table["H_three_planes"], k) for k in (1, 2, 3)] == [200, 60000, 65637]
    assert [classes_after(table["H_four_planes"], k) for k in (1, 2, 3, 4)] == [200, 60000, 65637, 65637]
    assert {p.dtype.name for n in ("H_count_00257", "H_count_65537") for p in table[n]["planes"]} >= {"uint16", "uint32"}


def test_h_top_byte_cases_differ_in_the_top_byte_only(table):
    for dt in lc.PLANE_DTYPES:
        for k in (1, 2):
            c = table[f"H_top_{dt}_{k}"]
            assert len(c["planes"]) == k
            for p in c["planes"]:
                assert p.dtype == dt
                bits = p.view(f"u{dt.itemsize}").astype(np.uint64)
                if dt.kind == "f":
                    assert np.isfinite(p).all() and (p == 0).any() and np.signbit(p[p == 0]).any() and not np.signbit(p[p == 0]).all()
                    bits = bits[p != 0]
                low = bits & np.uint64((1 << (8 * dt.itemsize - 8)) - 1)
                assert (low == low[0]).all() and set((bits >> np.uint64(8 * dt.itemsize - 8)).tolist()) == set(lc.TOP_BYTES)
            assert classes_after(c, 1) == len(lc.TOP_BYTES) + (dt.kind == "f")     # (+0.0 and -0.0 are one class)


def test_h_nan_and_small_cases(table):
    ids, n, first, values = lc.expected_combine(table["H_nan_cell0"])
    assert np.isnan(ids[0]) and ids[1] == 1 and first[0] == 1 and first.size == n == values.shape[0] and np.isnan(ids).sum() == 3
    c = table["H_nan_last_plane"]
    assert not any(np.isnan(p).any() for p in c["planes"][:-1] if p.dtype.kind == "f") and np.isnan(c["planes"][-1]).sum() == 2
    ids, n, first, values = lc.expected_combine(c)
    assert (values[:, 0].view(np.int64) < 0).any()                      # negative int8 in the key: sign extension
    f32 = c["planes"][1][first]
    assert np.array_equal(values[:, 1].view(np.float64), f32.astype(np.float64)) and (f32.astype(np.float64) != np.round(f32.astype(np.float64), 3)).any()
    ids, n, first, values = lc.expected_combine(table["H_single_cell"])
    assert ids.tolist() == [1.0] and n == 1 and first.tolist() == [0] and values[0, 0].view(np.int64) == -7
    assert values[0, 1] == np.array([-0.0]).view(np.uint64)[0]          # the first cell's own -0.0
    ids, n, first, values = lc.expected_combine(table["H_all_equal"])
    assert (ids == 1).all() and n == 1 and first.tolist() == [0]


def test_first_cells_against_a_plain_loop(table):
    """`local_oracle.combine_first_cells` (new with this table) against a dict over Python tuples"""
    for name in ("H_nan_cell0", "H_nan_last_plane", "H_count_00005", "H_top_float64_2", "H_top_int8_2"):
        c = table[name]
        seen, first = {}, []
        for i, t in enumerate(zip(*[p.tolist() for p in c["planes"]])):
            if any(v != v for v in t):
                continue
            if t not in seen:                                           # (-0.0 == 0.0 and they hash alike)
                seen[t] = len(seen) + 1
                first.append(i)
        ids, n, got, _ = lc.expected_combine(c)
        assert got.tolist() == first and n == len(first), name
        assert [ids[i] for i in first] == list(range(1, n + 1))


def test_where_the_class_sorts_bit_range_can_show_in_a_result(table):
    """What stays unreachable: `cbits` from plane 1 on.  The H_count cases put the class count on 2^k and 2^k + 1 as asked,
    but from the second plane on a class sort over too few bits -- or none -- gives the same ids and first cells
    (`local_cases.combine_model` has the argument), so no test at the ABI can tell a wrong `cbits` from a right one there.
    The single bit of plane 0 does show, in a case with NaN cells.  The model with the kernel's own bits equals the oracle."""
    exact = lambda j, count: max(1, int(count - 1).bit_length())                          # noqa: E731
    names = [f"H_count_{c:05d}" for c in (3, 5, 257, 65537)] + ["H_three_planes", "H_four_planes", "H_nan_cell0", "H_nan_last_plane",
                                                                "H_top_float32_2"]
    for name in names:
        c = table[name]
        want_ids, _, want_first, _ = lc.expected_combine(c)
        for bits in (None, lambda j, count: 0 if j else 1, lambda j, count: exact(j, count) - (j > 0)):
            ids, first = lc.combine_model(c["planes"], bits)
            assert np.array_equal(ids, want_ids, equal_nan=True) and np.array_equal(first, want_first), name
    c = table["H_nan_cell0"]
    ids, first = lc.combine_model(c["planes"], lambda j, count: 0)
    assert not np.array_equal(ids, lc.expected_combine(c)[0], equal_nan=True)

"""The case table of xrs_local_cells, xrs_local_combine and xrs_local_gather (xrspatial_amd/csrc/local.hip) at the C ABI, shared
by tests/test_local_cases_host.py (no GPU: every case reaches what its `reaches` tag names, from the data alone) and
tests/test_gpu_local_abi.py (the MI355X: every cell equals the rule).  NumPy only; nothing here imports the package.

Expected values come from tests/local_oracle.py only (`expected`, `expected_combine`).  The oracle gained two helpers for this
table: `distinct` (u of the popularity rule, to place the popularity refs around it) and `combine_first_cells` (the first
row-major cell of every combine class, which the second call of xrs_local_combine returns).

A case is a dict:
  name        unique; its first letter is the section A .. H below
  planes      list of 1-D arrays, each in its own dtype, one element per cell
  ref         the ref plane, or None
  ops         names of the functions to run on it (OPS); ('combine',) for section H
  out_is_i64  1: a function whose result is int64 by the rule is called with out_is_i64 = 1 (as xrspatial_amd.local does);
              0: every function writes float64 (for an int64 result: the integer converted, `as_out`'s `(double)r`)
  offset      elements by which every plane pointer, the ref pointer and (in doubles) the output pointer are moved past the
              start of their allocation: 1 makes them element-aligned and not pair-aligned
  reaches     the path of local.hip the case exists for

Sections (the paths they reach are listed in DESIGN.md §6f):
  A  op x working type x holder, plane counts on every boundary, all-integer and with-floats planes
  B  float64 result from integer planes (`as_out`, out_is_i64 = 0) next to the int64 result of the same planes
  C  the padding value of the register holders (+inf, INT64_MAX) as data, 0, 1, 2 and np times in a cell
  D  the extremes of each plane dtype through the pair load, the tail load and load_as
  E  cell counts around the three block sizes
  F  element-aligned plane, ref and output pointers
  G  ref dtypes of rank and popularity (`ref_minus_one`)
  H  combine: sort bit ranges, class counts on 2^k, first cells and gathered key values

The rule excludes int64 beyond 2^53 next to a floating plane in the frequencies, positions and rank ("the reference's per-item
comparisons ... stay exact beyond 2^53, these are not", module docstring of xrspatial_amd.local): no case mixes them there.
Popularity over ONE plane is NaN everywhere by the rule ("NaN if ... u >= n": u = n = 1), so that case alone is outside the
share-of-numbers condition of the host test.

Two limits of what these cases can see, both shown on the CPU by the host test.  combine's class sort: the H_count cases put
the class count on 2^k and 2^k + 1, yet from plane 1 on no bit range of that sort changes a result (`combine_model`); only the
single class bit of plane 0 shows, in the cases with NaN cells.  Rank over int64 planes: the float64 result cannot tell
INT64_MAX from INT64_MAX - 1 (both are 2^63), so of the C_i64 cases it is popularity's distinct count that tells the padding
value from the data."""
import functools

import numpy as np

from tests import local_oracle as lo

DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float64, np.float32)  # XRS_DT_* 0..9
DTYPE_CODE = {np.dtype(d): k for k, d in enumerate(DTYPES)}
INTS = tuple(np.dtype(d) for d in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64))
FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
PLANE_DTYPES = INTS + FLOATS                                                                # the nine a plane can have
OPS = {"max": 0, "min": 1, "sum": 2, "mean": 3, "std": 4, "median": 5, "lesser": 6, "equal": 7, "greater": 8, "lowest": 9,
       "highest": 10, "rank": 11, "popularity": 12}                                         # XRS_LOCAL_* of include/xrs_hip.h
STREAM_NO_REF = ("max", "min", "sum", "mean", "std", "lowest", "highest")
FREQ = ("lesser", "equal", "greater")
INT_STREAM = ("max", "min", "sum", "lesser", "equal", "greater", "lowest", "highest")       # those with an int64 working type
VALUES_OPS = ("median", "rank", "popularity")
NEEDS_REF = FREQ + ("rank", "popularity")
COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 24, 63, 64)
STREAM_CELLS, REG_CELLS, LDS_CELLS = 513, 257, 129          # one past the cells of a streaming / register / LDS block
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def holder(n):
    """which `Sorted` holds a cell of n planes"""
    return 4 if n <= 4 else 8 if n <= 8 else 16 if n <= 16 else "lds"


def pairwise_branch(n):
    """which boundaries of NumPy's pairwise sum n planes take"""
    return "<8" if n < 8 else "8" if n == 8 else "8k" if n % 8 == 0 else "8k+r"


def working(case, op):
    dtypes = [p.dtype for p in case["planes"]] + ([case["ref"].dtype] if op in NEEDS_REF else [])
    return lo.working_dtype(op, dtypes)


def case(name, planes, ops, reaches, ref=None, out_is_i64=1, offset=0):
    planes = [np.ascontiguousarray(p) for p in planes]
    assert all(p.ndim == 1 and p.size == planes[0].size and p.dtype in PLANE_DTYPES for p in planes), name
    assert ref is None or (ref.shape == planes[0].shape and ref.dtype in PLANE_DTYPES), name
    assert all(op in OPS or op == "combine" for op in ops) and (ref is not None or not set(ops) & set(NEEDS_REF)), name
    return {"name": name, "planes": planes, "ref": ref, "ops": tuple(ops), "out_is_i64": out_is_i64, "offset": offset,
            "reaches": reaches}


# ------------------------------------------------------------------------------------------------ expected values
def out_i64(c, op):
    """the out_is_i64 argument of the call"""
    dtypes = [p.dtype for p in c["planes"]] + ([c["ref"].dtype] if op in NEEDS_REF else [])
    return int(bool(c["out_is_i64"]) and lo.result_dtype(op, dtypes) == np.int64)


def rule(c, op):
    """the oracle's result in the rule's result dtype"""
    planes, ref = c["planes"], c["ref"]
    if op in lo.STATS:
        return lo.cell_stats(planes, op)
    if op in FREQ:
        return lo.frequency(planes, ref, op)
    if op in ("lowest", "highest"):
        return lo.position(planes, op)
    return lo.rank(planes, ref) if op == "rank" else lo.popularity(planes, ref)


def expected(c, op):
    """what the 8-byte output plane holds: int64 where the call passes out_is_i64 = 1, else float64"""
    r = rule(c, op)
    return r if out_i64(c, op) else r.astype(np.float64)


def expected_combine(c):
    """ids (float64, NaN for a NaN cell), n_classes, first cells (uint32) and the gathered key table as uint64 bit patterns
    (n_classes, planes): int64 for an integer plane, float64 for a floating one"""
    planes = c["planes"]
    ids, key = lo.combine(planes)
    first = lo.combine_first_cells(planes)
    table = np.zeros((len(key), len(planes)), np.uint64)
    for j, p in enumerate(planes):
        col = np.array([key[i + 1][j] for i in range(len(key))], np.float64 if p.dtype.kind == "f" else np.int64)
        table[:, j] = col.view(np.uint64)
    return ids, len(key), first, table


# ------------------------------------------------------------------------------------------------ building blocks
def _pool_size(n):
    return 2 if n <= 3 else 3 if n == 4 else 4


def int_planes(rng, n, cells):
    """dtypes cycling through the seven integer codes, values from a set of a few: ties, repeats and u < n"""
    m = _pool_size(n)
    out = []
    for j in range(n):
        dt = INTS[j % 7]
        low = -1 if dt.kind == "i" and m >= 3 else 0
        out.append(rng.integers(low, low + m, cells).astype(dt))
    return out


FLOAT_MIX = tuple(np.dtype(d) for d in (np.float32, np.int16, np.float64, np.uint8, np.float64, np.int32, np.float32, np.uint32,
                                        np.int8, np.float64, np.uint16, np.int64))
POP_MIX = tuple(np.dtype(d) for d in (np.float32, np.float64, np.int16, np.float64, np.uint8, np.float32, np.int32, np.uint32,
                                      np.int8, np.float64, np.uint16, np.int64))


def _spoil(rng, planes, cells):
    """NaN in 2 % of the cells (one floating plane each) and -0.0 in 5 % of the first floating plane"""
    floats = [p for p in planes if p.dtype.kind == "f"]
    zero = rng.random(cells) < 0.05
    floats[0][zero] = -0.0
    for i in rng.choice(cells, max(1, round(0.02 * cells)), replace=False):
        floats[rng.integers(0, len(floats))][i] = np.nan
    return planes


def float_planes(rng, n, cells):
    """float32 and float64 mixed with integers; full-mantissa values"""
    out = []
    for j in range(n):
        dt = FLOAT_MIX[j % len(FLOAT_MIX)]
        if dt.kind == "f":
            out.append(rng.normal(scale=50.0, size=cells).astype(dt))
        else:
            out.append(rng.integers(-100 if dt.kind == "i" else 0, 101, cells).astype(dt))
    return _spoil(rng, out, cells)


def float_pool_planes(rng, n, cells):
    """the same mix for popularity, which needs repeats: the floating planes draw from a few float32-exact values (two of them
    full-mantissa, so a float32 and a float64 plane tie exactly), the integer planes from 0 .. m - 1"""
    m = _pool_size(n)
    pool = np.array([np.float32(rng.normal(scale=50.0)), 0.0, np.float32(rng.normal(scale=50.0)), 1.0], np.float64)[:m]
    out = []
    for j in range(n):
        dt = POP_MIX[j % len(POP_MIX)]
        out.append((pool[rng.integers(0, m, cells)] if dt.kind == "f" else rng.integers(0, m, cells)).astype(dt))
    return _spoil(rng, out, cells)


def pick_ref(rng, planes, dtype, cells):
    """a frequency ref: in every cell the value of one of the planes, in `dtype` (so ==, < and > all occur)"""
    dtype = np.dtype(dtype)
    which = rng.integers(0, len(planes), cells)
    v = np.stack([p.astype(np.float64) for p in planes])[which, np.arange(cells)]
    if dtype.kind == "u":
        v = np.abs(v)
    if dtype.kind != "f":
        v = np.where(np.isnan(v), 0, v)
    with np.errstate(all="ignore"):
        return v.astype(dtype)


def spread_ref(rng, lo_valid, hi_valid, margin, dtype):
    """Refs for rank (per cell n) or popularity (per cell u): arrays lo_valid .. hi_valid bound the refs whose k = ref - 1 lies
    in the rule's range -n .. n - 1.  Half of the cells draw from that range, half from the whole span, `margin` + 1 below it to
    `margin` above it (symmetric about 0), whose two ends are placed in cells 0 and 1."""
    cells = lo_valid.size
    inside = rng.integers(lo_valid, hi_valid + 1)
    anywhere = rng.integers(lo_valid - margin - 1, hi_valid + margin + 1)
    ref = np.where(rng.random(cells) < 0.5, inside, anywhere)
    if cells > 1:
        ref[0], ref[1] = lo_valid[0] - margin - 1, hi_valid[1] + margin
    return ref.astype(dtype)


def rank_ref(rng, n, cells, dtype):
    """-n - 3 .. n + 3; valid are 1 - n .. n"""
    return spread_ref(rng, np.full(cells, 1 - n), np.full(cells, n), 3, dtype)


def pop_ref(rng, planes, dtype):
    """-u - 2 .. u + 2 with u from the oracle; valid are 1 - u .. u"""
    u = lo.distinct(planes, (dtype,))
    return spread_ref(rng, 1 - u, u, 2, dtype)


SIGNED_REF = (np.int8, np.int16, np.int32, np.int64)


# ------------------------------------------------------------------------------------------------ A
def section_a():
    out = []
    for n in COUNTS:
        vc = REG_CELLS if n <= 16 else LDS_CELLS
        for kind in ("ints", "floats"):
            rng = np.random.default_rng(1000 * n + (kind == "floats"))
            make = int_planes if kind == "ints" else float_planes
            w = "i64" if kind == "ints" else "f64"
            tag = f"{pairwise_branch(n)} planes summed, ld2 pair and tail of {'the integer' if kind == 'ints' else 'all nine'} dtypes, W = {w}"
            planes = make(rng, n, STREAM_CELLS)
            out.append(case(f"A_{kind}_n{n:02d}_stream", planes, STREAM_NO_REF, "streaming, no ref: " + tag))
            ref_dt = INTS[n % 7] if kind == "ints" else FLOATS[n % 2]
            ref = pick_ref(rng, planes, ref_dt, STREAM_CELLS)
            if kind == "floats":
                ref[::50] = np.nan                                                   # "a NaN ref counts 0"
            out.append(case(f"A_{kind}_n{n:02d}_freq", planes, FREQ, f"frequencies, {ref_dt} ref: " + tag, ref=ref))
            where = f"holder {holder(n)}, W = "
            planes = make(rng, n, vc)
            out.append(case(f"A_{kind}_n{n:02d}_median", planes, ("median",), where + "f64, median " + ("odd" if n % 2 else "even")))
            out.append(case(f"A_{kind}_n{n:02d}_rank", planes, ("rank",), where + w + ", rank",
                            ref=rank_ref(rng, n, vc, SIGNED_REF[n % 4])))
            planes = planes if kind == "ints" else float_pool_planes(rng, n, vc)
            out.append(case(f"A_{kind}_n{n:02d}_popularity", planes, ("popularity",), where + w + ", popularity",
                            ref=pop_ref(rng, planes, SIGNED_REF[(n + 1) % 4])))
    return out


# ------------------------------------------------------------------------------------------------ B
def section_b():
    """The eight streaming functions with an int64 working type, out_is_i64 = 0 and 1 on the same planes.  `big`: values
    beyond 2^53 whose conversion to float64 rounds (max, min, sum; the int64 sum also wraps); `small`: all eight."""
    out = []
    rng = np.random.default_rng(20)
    cells = STREAM_CELLS
    odd = np.array([2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 62 + 1, -(2 ** 62) - 3, 2 ** 60 + 5, 2 ** 53 + 3, I64_MAX, I64_MIN, 7, -7], np.int64)
    big = [odd[rng.integers(0, odd.size, cells)] for _ in range(3)] + [rng.integers(-100, 100, cells).astype(np.int32),
                                                                        rng.integers(0, 2 ** 32, cells).astype(np.uint32)]
    small9 = int_planes(rng, 9, cells)
    small3 = int_planes(rng, 3, cells)
    for o in (0, 1):
        how = "as_out (double)r" if o == 0 else "as_out bit pattern"
        out.append(case(f"B_big_n05_out{o}", big, ("max", "min", "sum"), how + ", |v| > 2^53: the conversion rounds", out_is_i64=o))
        for planes in (small3, small9):
            ref = pick_ref(np.random.default_rng(21), planes, np.int16, cells)
            out.append(case(f"B_small_n{len(planes):02d}_out{o}", planes, INT_STREAM, how + ", the eight int64 streaming functions",
                            ref=ref, out_is_i64=o))
    return out


# ------------------------------------------------------------------------------------------------ C
C_COUNTS = (3, 5, 7, 9, 15, 17, 33)
C_CELLS = 160


def section_c():
    """Cell c holds `largest` (+inf, or INT64_MAX) [0, 1, 2, np][c % 4] times; the other values are the smallest value of the
    type and a few finite ones, shuffled over the planes.  17 and 33 planes (LDS, no padding) hold the same value sets."""
    out = []
    for n in C_COUNTS:
        for kind in ("f64", "i64"):
            rng = np.random.default_rng(300 + n + (kind == "i64"))
            top, bottom = (np.inf, -np.inf) if kind == "f64" else (I64_MAX, I64_MIN)
            others = np.array([bottom, -1.5, 0.0, 2.25] if kind == "f64" else [bottom, -1, 0, 2], np.float64 if kind == "f64" else np.int64)
            m = others.size if n > 3 else 2
            v = others[rng.integers(0, m, (n, C_CELLS))]
            times = np.array([0, 1, 2, n])[np.arange(C_CELLS) % 4]
            for c in range(C_CELLS):
                v[rng.permutation(n)[:times[c]], c] = top
            if kind == "f64":                                                        # float32 planes hold +-inf exactly too
                planes = [v[j].astype(np.float32 if j % 3 == 1 else np.float64) for j in range(n)]
            else:
                planes = [v[j] for j in range(n)]
            pad = f"{holder(n)} slots, {n} filled" if n <= 16 else "LDS, no padding"
            name = f"C_{kind}_n{n:02d}"
            what = "largest<f64> as data" if kind == "f64" else "INT64_MAX is 2^63 in float64, next to the +inf padding"
            out.append(case(name + "_median", planes, ("median",), f"{what}, median's middle index, {pad}"))
            out.append(case(name + "_rank", planes, ("rank",), f"largest<{kind}> as data, rank's k < np, {pad}",
                            ref=rank_ref(rng, n, C_CELLS, np.int32)))
            out.append(case(name + "_popularity", planes, ("popularity",), f"largest<{kind}> as data, distinct count and pick loop, {pad}",
                            ref=pop_ref(rng, planes, np.int64)))
    return out


# ------------------------------------------------------------------------------------------------ D
def extremes(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        f = np.finfo(dtype)
        return np.array([-np.inf, -f.max, -f.tiny, -0.0, 0.0, f.tiny, f.max, np.inf], dtype)
    i = np.iinfo(dtype)
    return np.array(sorted({i.min, i.min + 1, -1 if i.min < 0 else 0, 0, 1, i.max - 1, i.max}), dtype=object).astype(dtype)


def section_d():
    """Three planes of one dtype, each a rotation of the dtype's extremes; 7 cells (the last is the single-cell tail and holds
    min, max and -1 / 1) and 8 cells (pairs only).  The values kernel reads the same planes through load_as."""
    out = []
    for dt in PLANE_DTYPES:
        e = extremes(dt)
        for cells in (7, 8):
            # the last cell holds min, max and -1 (unsigned: max - 1; floating: -tiny)
            planes = [e[(at - (cells - 1) + np.arange(cells)) % e.size] for at in (0, e.size - 1, 2)]
            tag = f"{dt} extremes: ld2 {'pair and tail' if cells % 2 else 'pair'}, load_as; "
            name = f"D_{dt}_c{cells}"
            out.append(case(name + "_stream", planes, ("max", "min", "sum", "lowest", "highest"), tag + "streaming"))
            out.append(case(name + "_equal", planes, ("equal",), tag + "ref of the same dtype", ref=np.roll(planes[0], 2)))
            out.append(case(name + "_median", planes, ("median",), tag + "median"))
            out.append(case(name + "_rank", planes, ("rank",), tag + "rank", ref=(np.arange(cells) % 6 - 2).astype(np.int32)))  # inside the range
    return out


def _same_bits(a, value):
    """where `a` holds exactly `value` (-0.0 is not 0.0)"""
    a = np.ascontiguousarray(a)
    one = np.array([value], a.dtype)
    return a.view(f"u{a.dtype.itemsize}") == one.view(f"u{a.dtype.itemsize}")[0]


# ------------------------------------------------------------------------------------------------ E
CELL_COUNTS = (1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)


def section_e():
    out = []
    for cells in CELL_COUNTS:
        rng = np.random.default_rng(500 + cells)
        planes = [rng.normal(scale=50.0, size=cells).astype(np.float32) for _ in range(3)]
        out.append(case(f"E_c{cells:04d}_f32", planes, ("sum", "median"),
                        f"{cells} cells: grid and tail of the streaming (512) and register-values (256) blocks"))
        planes = [rng.integers(-50, 50, cells).astype(np.int32) for _ in range(20)]
        out.append(case(f"E_c{cells:04d}_i32", planes, ("rank",), f"{cells} cells: grid and tail of the LDS-values (128) block",
                        ref=rng.integers(-19, 21, cells).astype(np.int32)))          # every ref inside the rule's range
    return out


# ------------------------------------------------------------------------------------------------ F
F_DTYPES = tuple(np.dtype(d) for d in (np.float32, np.int32, np.uint32, np.float64, np.int64))


def section_f():
    out = []
    for dt in F_DTYPES:
        rng = np.random.default_rng(600 + DTYPE_CODE[dt])
        if dt.kind == "f":
            planes = [rng.normal(scale=50.0, size=STREAM_CELLS).astype(dt) for _ in range(3)]
        else:
            i = np.iinfo(dt)
            planes = [rng.integers(max(i.min, -2 ** 40), min(i.max, 2 ** 40), STREAM_CELLS, dtype=np.int64).astype(dt) for _ in range(3)]
        ref = pick_ref(rng, planes, dt, STREAM_CELLS) if dt.kind == "f" else planes[1][::-1].copy()
        out.append(case(f"F_{dt}_offset1", planes, ("max", "sum", "std", "greater"),
                        f"{dt} planes at ptr + {dt.itemsize}, out at ptr + 8: pair loads and store_d2u at element alignment",
                        ref=ref, offset=1))
    return out


# ------------------------------------------------------------------------------------------------ G
G_CELLS = 96


def g_specials(dt, n):
    i = np.iinfo(dt)
    s = [0, 1, n, n + 1, i.min, i.max] + ([-n, -n - 1] if i.min < 0 else [])
    return [v for v in s if i.min <= v <= i.max]


def section_g():
    """Cells 0 .. 7 hold the special refs (cell 0: ref 0); the others refs inside the rule's range.  Every cell holds the three
    values 0, 1, 2 (u = 3 < n), rotated, so popularity is a number wherever k is in range."""
    out = []
    for dt in INTS:
        for n in (5, 20):
            rng = np.random.default_rng(700 + n + DTYPE_CODE[dt])
            planes = [((j + np.arange(G_CELLS)) % 3 if j < 3 else rng.integers(0, 3, G_CELLS)).astype(np.int32) for j in range(n)]
            special = g_specials(dt, n)
            for op, hi in (("rank", n), ("popularity", 3)):
                low = 1 - hi if dt.kind == "i" else 1
                ref = rng.integers(low, hi + 1, G_CELLS)
                ref[:len(special)] = special
                out.append(case(f"G_{dt}_n{n:02d}_{op}", planes, (op,), f"ref_minus_one in {dt}: 0, 1, n, n + 1, min, max"
                                + (", -n, -n - 1" if dt.kind == "i" else "; 0 wraps to the maximum"), ref=ref.astype(dt)))
    return out


# ------------------------------------------------------------------------------------------------ H
TOP_BYTES = (0x00, 0x01, 0x40, 0x7f, 0x80, 0xc0, 0xff)
CLASS_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 65536, 65537)


def top_byte_values(dt):
    """values of `dt` that differ in nothing but their top byte (no NaN, no inf among the floating ones), and for a floating
    dtype +0.0 and -0.0, which are one value"""
    dt = np.dtype(dt)
    bits = 8 * dt.itemsize
    low = 0x0003456789abcdef & ((1 << (bits - 8)) - 1) if bits > 8 else 0           # (the exponent's lower bits are not all ones)
    if dt == np.float32:
        low &= ~(1 << 23)
    pats = np.array([(t << (bits - 8)) | low for t in TOP_BYTES], dtype=f"u{dt.itemsize}")
    v = pats.view(dt)
    if dt.kind == "f":
        assert np.isfinite(v).all()
        v = np.concatenate([v, np.array([0.0, -0.0], dt)])
    return v


def section_h():
    out = []
    ops = ("combine",)
    for dt in PLANE_DTYPES:
        rng = np.random.default_rng(800 + DTYPE_CODE[dt])
        v = top_byte_values(dt)
        a = v[rng.integers(0, v.size, 61)]
        a[:v.size] = v
        b = v[rng.integers(0, v.size, 61)]
        out.append(case(f"H_top_{dt}_1", [a], ops, f"value sort to end_bit {8 * dt.itemsize}: {dt} values that differ in the top byte only"))
        out.append(case(f"H_top_{dt}_2", [a, b], ops, f"two {dt} planes that differ in the top byte only, canon, gather's widening"))
    for c in CLASS_COUNTS:
        cells = c + 100
        i = np.arange(cells)
        dt = np.uint8 if c <= 256 else np.uint16 if c <= 65536 else np.uint32
        splits = np.where((i >= c) & (i % 3 == 0), -3, 0).astype(np.int16)
        out.append(case(f"H_count_{c:05d}", [(i % c).astype(dt), splits], ops,
                        f"cbits: exactly {c} classes after plane 0, plane 1 splits some"))
    i = np.arange(65637)
    three = [(i % 200).astype(np.uint8), (i // 200 % 300).astype(np.uint16), ((i // 60000).astype(np.uint32) << 31).astype(np.uint32)]
    out.append(case("H_three_planes", three, ops, "cbits: 200 classes, then 60000, then 65637"))
    out.append(case("H_four_planes", three + [np.full(i.size, -128, np.int8)], ops,
                    "cbits: 200 classes, then 60000, then 65637 before a further plane is sorted"))
    rng = np.random.default_rng(850)
    f = rng.integers(0, 3, 300).astype(np.float32) * np.float32(0.1)
    g = rng.integers(-2, 2, 300).astype(np.int8)
    nan0 = f.copy()
    nan0[[0, 17, 299]] = np.nan
    out.append(case("H_nan_cell0", [nan0, g], ops, "NaN in cell 0: the NaN class's 0xffffffff first cell stays out of the list"))
    last = rng.integers(0, 2, 300).astype(np.float64) - 0.5
    last[[3, 150]] = np.nan
    out.append(case("H_nan_last_plane", [g, f, last], ops, "NaN only in the last plane; float32 widened exactly, int8 sign-extended"))
    out.append(case("H_single_cell", [np.array([-7], np.int16), np.array([-0.0], np.float32)], ops, "a single cell"))
    out.append(case("H_all_equal", [np.full(300, 2 ** 31, np.uint32), np.full(300, I64_MIN, np.int64)], ops, "all cells equal: one class"))
    return out


def combine_model(planes, class_bits=None):
    """xrs_local_combine's loop re-derived from its source in NumPy, with the number of class bits of the second sort open:
    `class_bits(plane index, count)`, default the kernel's (the fewest bits that hold count - 1, at least 1).  Returns (ids,
    first cells).  Never an expected value: tests/test_local_cases_host.py uses it to show where the second sort's bit range
    can be seen in a result and where not.  At plane 0 the valid cells (class 0) and the NaN cells (class 1, value 0) lie
    mixed in index order, and the one class bit is what parts them.  After a plane the cells are ordered by (class so far,
    value) and every new class is one run of that order; the next stable value sort keeps each run together inside its
    value, so the runs of (class, value) are contiguous before the class sort, and after it whatever bits it looks at.  From
    plane 1 on the bit range only changes how the classes are numbered between planes, and the ids are numbered afresh by
    first cell."""
    n = planes[0].size
    bad = np.zeros(n, bool)
    for p in planes:
        if p.dtype.kind == "f":
            bad |= np.isnan(p)
    idx, cls, count = np.arange(n), bad.astype(np.int64), 2
    for j, p in enumerate(planes):
        canon = np.where(bad | (p == 0), 0, np.ascontiguousarray(p).view(f"u{p.dtype.itemsize}")).astype(np.uint64)
        idx = idx[np.argsort(canon[idx], kind="stable")]
        bits = class_bits(j, count) if class_bits else max(1, int(count - 1).bit_length())
        idx = idx[np.argsort(cls[idx] & ((1 << bits) - 1), kind="stable")]
        v, c = canon[idx], cls[idx]
        scan = np.cumsum(np.concatenate([[True], (c[1:] != c[:-1]) | (v[1:] != v[:-1])]))
        cls = np.empty(n, np.int64)
        cls[idx] = scan - 1
        count = int(scan[-1])
    starts = np.flatnonzero(np.concatenate([[True], scan[1:] != scan[:-1]]))
    first = np.where(bad[idx[starts]], 0xffffffff, idx[starts])                          # of classes 0 .. count - 1
    order = np.argsort(first, kind="stable")
    rank = np.empty(count, np.int64)
    rank[order] = np.arange(count)
    ids = np.where(bad, np.nan, rank[cls] + 1.0)
    listed = first[order]
    return ids, listed[listed != 0xffffffff].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _all():
    cases = section_a() + section_b() + section_c() + section_d() + section_e() + section_f() + section_g() + section_h()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def cases(section=None):
    return [c for c in _all() if section is None or c["name"][0] in section]


def by_name():
    return {c["name"]: c for c in _all()}

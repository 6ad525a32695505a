"""Cases, plain references and a CPU model of the search walk for xrs_proximity (xrspatial_amd/csrc/proximity.hip), shared by
tests/test_proximity_cases_host.py (no GPU: every case reaches what it is named for) and tests/test_gpu_proximity_abi.py (the
MI355X: the planes equal the references).  NumPy only; nothing here imports the package.

Expected values of the search always come from tests/proximity_oracle.run, the brute force over all targets.  `walk` below
re-derives the kernel's candidate set and prunings from its source; it is used to PROVE what a case reaches (rows visited, how a
side closed, whether a tie run was extended) and never as an expected value.

Geometry re-derived from the source: the row scan takes SPAN = 256 columns per step, left to right from column 0 and right to
left from the last column (so the two passes cut a row at different columns unless cols % 256 == 0), four wave totals through a
two-slot LDS buffer and a carry from step to step; the row list is compacted in steps of 256 rows the same way; the search puts
a block on 256 adjacent columns of one row.  Workspace (documented ABI, include/xrs_hip.h): `layout`."""
from dataclasses import dataclass, field

import numpy as np

from tests import proximity_oracle as po
from tests.golden import make_proximity_exec as gen

SPAN = 256
DTYPES = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64, np.float64, np.float32)  # XRS_DT_* 0..9
DTYPE_CODE = {np.dtype(d): k for k, d in enumerate(DTYPES)}
VALUES_KIND = {np.dtype(np.float64): 0, np.dtype(np.int64): 1, np.dtype(np.uint64): 2}                             # XRS_PROX_VALUES_*
SCAN_ONLY, SEARCH_ONLY = 16, 32
METRIC_NAMES = ("EUCLIDEAN", "GREAT_CIRCLE", "MANHATTAN")                                                           # codes 0, 1, 2


@dataclass
class Case:
    name: str
    z: np.ndarray
    xs: np.ndarray
    ys: np.ndarray
    why: str
    tv: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float64))
    md: float = np.inf
    metrics: tuple = ("EUCLIDEAN", "MANHATTAN")

    @property
    def kind(self):
        return VALUES_KIND[self.tv.dtype]


def unit_coords(rows, cols):
    return np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64)[::-1].copy()


# ------------------------------------------------------------------------------------------------ the workspace
def up256(v):
    return (v + 255) // 256 * 256


def layout(rows, cols):
    """Byte offsets of the five parts of the workspace and its size: left and right int32[rows * cols], flag and list
    int32[rows], count int32[1], each part rounded up to 256 bytes (the last takes 256)."""
    out = {"left": 0}
    out["right"] = up256(rows * cols * 4)
    out["flag"] = out["right"] + up256(rows * cols * 4)
    out["list"] = out["flag"] + up256(rows * 4)
    out["count"] = out["list"] + up256(rows * 4)
    out["total"] = out["count"] + 256
    return out


# ------------------------------------------------------------------------------------------------ the scan
def scan_reference(targets):
    """left[i][j]: the largest target column <= j; right[i][j]: the smallest > j; -1 for none.  flag[i]: the row holds a
    target; list[:count]: those rows, ascending."""
    t = np.asarray(targets, bool)
    rows, cols = t.shape
    idx = np.arange(cols, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(t, idx, -1), axis=1)
    at_or_right = np.minimum.accumulate(np.where(t, idx, cols)[:, ::-1], axis=1)[:, ::-1]
    right = np.concatenate([at_or_right[:, 1:], np.full((rows, 1), cols)], axis=1)
    right[right == cols] = -1
    flag = t.any(axis=1)
    lst = np.flatnonzero(flag)
    return {"left": left.astype(np.int32), "right": right.astype(np.int32), "flag": flag.astype(np.int32),
            "list": lst.astype(np.int32), "count": int(lst.size)}


def exact_targets(z, tv):
    """`z == one of tv` in Python's exact arithmetic (integers as integers of any size, floats as float64): the check on
    proximity_oracle.targets for the dtype pairs that NumPy has to promote."""
    want = [v.item() for v in np.asarray(tv).ravel()]
    flat = [v.item() for v in np.asarray(z).ravel()]
    return np.array([any(a == b for b in want) for a in flat], bool).reshape(np.shape(z))


def width_raster(cols, seed=0):
    """Eight rows, one of each kind the scan can get wrong (the issue's list; it has eight kinds, so the raster has eight
    rows): empty | a target in column 0 only | in the last column only | in columns 255 and 256 where they exist (else the
    middle column) | all targets | one target in the first span only (the carry crosses every later span rightwards) | one in
    the last span only (the same leftwards) | random at 10 %."""
    z = np.zeros((8, cols), np.int32)
    z[1, 0] = 3
    z[2, cols - 1] = 4
    seam = [c for c in (SPAN - 1, SPAN) if c < cols]
    z[3, seam if seam else [cols // 2]] = 5
    z[4, :] = 6
    z[5, min(3, cols - 1)] = 7
    z[6, max(cols - 4, 0)] = 8
    z[7, :] = gen.scatter((cols,), 100 + cols + seed, 0.10, np.int32)
    return z


WIDTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769)
HEIGHTS = (1, 255, 256, 257, 513, 700)
FLAG_PATTERNS = ("none", "all", "row0", "last", "seams", "random30", "all_but_one", "random86")


def flag_rows(rows, pattern):
    """Which rows hold a target: none | all | only row 0 | only the last | exactly rows 255, 256, 511, 512 (those that exist) |
    random at 30 % | all but one (513 rows: a list of 512) | random at 86 % (700 rows: about 600)."""
    f = np.zeros(rows, bool)
    if pattern == "all":
        f[:] = True
    elif pattern == "row0":
        f[0] = True
    elif pattern == "last":
        f[-1] = True
    elif pattern == "seams":
        f[[r for r in (255, 256, 511, 512) if r < rows]] = True
    elif pattern == "random30":
        f = np.random.default_rng(rows).random(rows) < 0.30
    elif pattern == "all_but_one":
        f[:] = True
        f[rows // 3] = False
    elif pattern == "random86":
        f = np.random.default_rng(rows + 1).random(rows) < 0.86
    elif pattern != "none":
        raise ValueError(pattern)
    return f


def flag_raster(rows, cols, pattern, dtype=np.int32):
    """A raster whose rows `flag_rows` hold random targets (at least one each, 30 % of their cells) and whose other rows are
    zero -- NaN for a float dtype, which is no target either."""
    rng = np.random.default_rng(7 * rows + cols)
    f = flag_rows(rows, pattern)
    z = np.where(rng.random((rows, cols)) < 0.30, rng.integers(1, 10, (rows, cols)), 0)
    z[np.arange(rows), rng.integers(0, cols, rows)] = 9
    z = (z * f[:, None]).astype(dtype)
    if np.dtype(dtype).kind == "f":
        z[~f] = np.nan
    return z


def dtype_raster(dtype, rows=5, cols=300):
    """Every dtype of the ABI at 5 x 300 for `n_values == 0`: zeros, small values and the ends of the format; float rasters
    hold NaN, +inf, -inf and -0.0, none of which is a target."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(31 + DTYPE_CODE[dt])
    pick = rng.random((rows, cols))
    if dt.kind == "f":
        z = np.where(pick < 0.2, rng.integers(-5, 6, (rows, cols)) * 0.5, 0.0).astype(dt)
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, np.finfo(dt).tiny, -np.finfo(dt).max)):
            z[(pick > 0.97 - 0.03 * k) & (pick <= 1.0 - 0.03 * k)] = v
        z[1, :] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], dt)[np.arange(cols) % 5]      # a row without a target
    else:
        info = np.iinfo(dt)
        z = np.where(pick < 0.2, rng.integers(1, 100, (rows, cols)), 0).astype(dt)
        z[pick > 0.97] = info.max
        z[(pick > 0.94) & (pick <= 0.97)] = info.min                      # 0 for the unsigned ones: no target
        z[1, :] = 0
    z[-1, cols - 1] = 1
    return z


def value_cases():
    """[(name, raster, target values in the dtype the ABI reads them in)]: every branch of value_match.h.  The expected mask
    is proximity_oracle.targets (NumPy's ==); the host test holds it against `exact_targets`."""
    out = []
    rows, cols = 5, 300
    rng = np.random.default_rng(77)
    pick = rng.random((rows, cols))
    for dt in (np.float32, np.float64):
        z = np.where(pick < 0.1, 2.0, 0.0).astype(dt)
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.1)):
            z[(pick > 0.5 + 0.1 * k) & (pick <= 0.6 + 0.1 * k)] = dt(v)
        name = np.dtype(dt).name
        for label, tv in (("inf", [np.inf]), ("nan", [np.nan]), ("zero", [0.0]), ("tenth", [0.1]), ("neg_inf_and_2", [-np.inf, 2.0])):
            out.append((f"{name}_{label}", z, np.array(tv, np.float64)))
    big = 2 ** 53
    z = np.where(pick < 0.1, big + 1, np.where(pick < 0.3, big, np.where(pick < 0.4, -big - 1, 0))).astype(np.int64)
    out.append(("int64_beyond_2_53", z, np.array([big + 1], np.int64)))
    out.append(("int64_negative_beyond_2_53", z, np.array([-big - 1, 5], np.int64)))
    for dt in (np.uint8, np.uint16, np.uint32, np.uint64):                # -1 has the bits of the largest value: no match
        z = np.where(pick < 0.2, np.iinfo(dt).max, np.where(pick < 0.3, 7, 0)).astype(dt)
        out.append((f"{np.dtype(dt).name}_negative_i64", z, np.array([-1], np.int64)))
        out.append((f"{np.dtype(dt).name}_negative_i64_and_7", z, np.array([-1, 7, -(2 ** 63)], np.int64)))
    top = 2 ** 63
    for dt in (np.int8, np.int16, np.int32, np.int64):                    # 2^64 - 1 has the bits of -1, 2^63 those of int64's min
        z = np.where(pick < 0.2, -1, np.where(pick < 0.3, 7, np.where(pick < 0.4, np.iinfo(dt).min, 0))).astype(dt)
        out.append((f"{np.dtype(dt).name}_u64_above_2_63", z, np.array([2 ** 64 - 1, top, top + 5], np.uint64)))
        out.append((f"{np.dtype(dt).name}_u64_above_2_63_and_7", z, np.array([2 ** 64 - 1, 7, top], np.uint64)))
    z = np.where(pick < 0.1, top + 5, np.where(pick < 0.3, top + 6, np.where(pick < 0.4, 5, 0))).astype(np.uint64)
    out.append(("uint64_u64_above_2_63", z, np.array([top + 5], np.uint64)))
    out.append(("uint64_u64_top", z.copy() | np.where(pick > 0.9, np.uint64(2 ** 64 - 1), np.uint64(0)), np.array([2 ** 64 - 1], np.uint64)))
    z = np.where(pick < 0.2, 2, np.where(pick < 0.4, 3, 0)).astype(np.int32)
    out.append(("int32_f64_two", z, np.array([2.0], np.float64)))
    out.append(("int32_f64_two_and_a_half", z, np.array([2.5], np.float64)))
    return out


# ------------------------------------------------------------------------------------------------ the search's cases
RING = [(-5, 0), (5, 0), (0, -5), (0, 5)] + [(a * s, b * t) for a, b in ((3, 4), (4, 3)) for s in (-1, 1) for t in (-1, 1)]
RING_CENTRES = ((8, 10), (8, 40), (22, 25))
LONE = (2, 70)                                                            # a target with nothing else within 10 cells


def ring_raster():
    """30 x 80, integer coordinates: the 12 lattice points at distance 5 round three centres (a 12-way tie at each), a
    same-row pair and a same-column pair four cells apart (2-way ties between them), a plus of four targets at distance 2
    (a 4-way tie) and one lone target: the cell 5 rows below it has it as its only target within 5, straight above."""
    z = np.zeros((30, 80), np.int32)
    v = 1
    for r0, c0 in RING_CENTRES:
        for dr, dc in RING:
            z[r0 + dr, c0 + dc] = v
            v += 1
    z[15, 52], z[15, 56] = 40, 41                                        # the same row
    z[20, 62], z[24, 62] = 42, 43                                        # the same column
    for dr, dc in ((-2, 0), (2, 0), (0, -2), (0, 2)):
        z[24 + dr, 48 + dc] = 44 + abs(dr) + 2 * (dc > 0) + (dr > 0)
    z[LONE] = 50
    return z


def far_raster():
    """40 x 300, unit cells.  Rows 6 .. 39 hold one target each near column 299; row 5 holds four near column 0.  For the
    cells of the last rows near column 0 the near rows hold only far-away targets and the nearest target lies 30 rows and more
    off: the walk has to pass 30 rows whose candidates lose."""
    z = np.zeros((40, 300), np.int32)
    for r in range(6, 40):
        z[r, 299 - r % 3] = 1 + r % 7
    z[5, [0, 7, 14, 21]] = 9
    return z


def mixed_raster():
    """40 x 256, unit cells: one search block per row.  Every row holds a target in column 255, row 0 one in column 0.  In the
    last row lane j has its best 255 - j from its own row and closes `up` once the bound k passes it: lane 250 after 6 rows,
    lane 230 after 26, lane 200 never (the rows run out)."""
    z = np.zeros((40, 256), np.int32)
    z[:, 255] = np.arange(1, 41)
    z[0, 0] = 77
    return z


def tie_run_raster():
    """8 x 40 int32, default_rng(1), 20 % targets of distinct values, every other row emptied."""
    rng = np.random.default_rng(1)
    t = rng.random((8, 40)) < 0.20
    t[1::2] = False
    z = np.zeros((8, 40), np.int32)
    z[t] = 1 + np.arange(int(t.sum()))
    return z


def tie_run_coords(sx, sy):
    return sx * np.arange(40), sy * np.arange(8)[::-1]


TIE_RUN_SPACINGS = {"thin_0.01x100": (0.01, 100.0), "thin_0.001x1000": (0.001, 1000.0), "all_zero_1e-46": (1e-46, 1e-46),
                    "thin_1e-6x1000": (1e-6, 1000.0), "inf_1e30x1e39": (1e30, 1e39), "all_inf_1e39": (1e39, 1e39)}
BOTH_METRICS_TIE = ("all_zero_1e-46", "thin_1e-6x1000", "inf_1e30x1e39", "all_inf_1e39")


def tie_run_cases():
    """Long thin cells: the targets of one side of a row above or below share one float32 distance, and rule 3 names the far
    end of the run.  EUCLIDEAN ties at every spacing; MANHATTAN, |dx| + |dy|, only where 40 sx is below a float32 ulp of sy
    (1e-6 x 1000), everything underflows (1e-46) or every other row is beyond float32 (1e30 x 1e39: d32 = inf; 1e39 x 1e39: every other cell, at any ratio of the float64 distances).  `metrics`: where the unextended candidate set must differ from the
    oracle at 10 cells and more; the GPU runs both metrics at every spacing."""
    z = tie_run_raster()
    out = []
    for name, (sx, sy) in TIE_RUN_SPACINGS.items():
        xs, ys = tie_run_coords(sx, sy)
        metrics = ("EUCLIDEAN", "MANHATTAN") if name in BOTH_METRICS_TIE else ("EUCLIDEAN",)
        out.append(Case(f"tie_run_{name}", z, xs, ys, "runs of float32-equidistant targets on one side of a row", metrics=metrics))
    return out


def margin_cases():
    """Two targets whose float32 distance to the cell at x = 0 is the same, as far apart as that allows: both round to
    m = 1 + 2^-23, from 0.99 of half an ulp below and above it (the ratio of the float64 distances is 1 + 0.99 * 2^-23, of
    their squares 1 + 2.36e-7: just inside what the kernel's `may_tie` filter must let through).  Rows 1e-20 apart, which
    vanishes against 1 in float64.  `above`: the targets in the row above the cell's, left of it -- the rule names the farther
    one; `below`: in the row below, right of it."""
    m, d = 1.0 + 2.0 ** -23, 0.99 * 2.0 ** -24
    xs = np.array([-(m + d), -(m - d), 0.0, m - d, m + d])
    ys = np.array([1e-20, 0.0])
    above, below = np.zeros((2, 5), np.int32), np.zeros((2, 5), np.int32)
    above[0, :2] = 1, 2
    below[1, 3:] = 3, 4
    why = "a two-target run at the widest ratio that still ties"
    return [Case("margin_above", above, xs, -ys, why), Case("margin_below", below, xs, ys, why)]


def great_circle_tie_case():
    """The limit that is left: GREAT_CIRCLE does not extend tie runs.  Longitudes 1e-9 degrees apart, latitudes 0.5."""
    xs, ys = tie_run_coords(1e-9, 0.5)
    return Case("gc_tie_run", tie_run_raster(), 10.0 + xs, 40.0 + ys, "GREAT_CIRCLE names the nearest of a tied run", metrics=("GREAT_CIRCLE",))


def uneven_coords(rows, cols, seed=5):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.uniform(0.5, 2.5, cols)), 100.0 - np.cumsum(rng.uniform(0.5, 2.5, rows))


def search_cases():
    """The EUCLIDEAN / MANHATTAN cases against the oracle (the issue's list)."""
    out = []
    for rows, cols in ((700, 5), (513, 9)):
        xs, ys = unit_coords(rows, cols)
        for pattern in FLAG_PATTERNS:
            dtype = np.float32 if pattern == "none" else np.int32          # `none`: all NaN, a list of 0 rows
            out.append(Case(f"rows_{rows}x{cols}_{pattern}", flag_raster(rows, cols, pattern, dtype), xs, ys,
                            f"row list: {pattern}; cells above every non-empty row and below every one"))
    out.append(Case("far_40x300", far_raster(), *unit_coords(40, 300), "the walk passes 30 rows of far-away targets"))
    out.append(Case("mixed_40x256", mixed_raster(), *unit_coords(40, 256), "lanes of one block close `up` many rows apart"))
    z = gen.scatter((20, 70), 11, 0.04, np.int32)
    for yname, ys in (("y_falling", np.arange(20.0)[::-1].copy()), ("y_rising", np.arange(20.0))):
        for xname, xs in (("x_rising", np.arange(70.0)), ("x_falling", np.arange(70.0)[::-1].copy())):
            out.append(Case(f"order_{yname}_{xname}", z, xs, ys, "the tie order lives in index space"))
    ring = ring_raster()
    xs, ys = unit_coords(*ring.shape)
    out.append(Case("ring", ring, xs, ys, "2-, 4- and 12-way ties"))
    out.append(Case("ring_max5", ring, xs, ys, "s == max2 is kept; a row with bound^2 == max2 is not pruned", md=5.0))
    out.append(Case("ring_max0", ring, xs, ys, "max_distance 0: the targets themselves only", md=0.0))
    z = gen.scatter((23, 90), 13, 0.03, np.int32)
    out.append(Case("uneven_23x90", z, *uneven_coords(23, 90), "uneven coordinate steps"))
    out.append(Case("uneven_23x90_max6", z, *uneven_coords(23, 90), "uneven steps and a cut", md=6.0))
    for cols in (257, 513):
        z = gen.scatter((9, cols), cols, 0.01, np.int32)
        z[4, 0], z[4, -1], z[3, :] = 4, 6, 0
        out.append(Case(f"width_{cols}", z, 10.0 + 0.75 * np.arange(cols), 400.0 - 1.25 * np.arange(9), "the last block has one valid lane"))
    for dt in (np.int8, np.uint16, np.uint32):
        info = np.iinfo(dt)
        z = gen.scatter((12, 70), 17, 0.05, np.int64)
        z = np.where(z == 9, info.max, np.where(z == 8, info.min, np.where(z == 7, info.max - 1, z))).astype(dt)
        out.append(Case(f"alloc_{np.dtype(dt).name}", z, *unit_coords(12, 70), "allocation reads the raster in its own dtype"))
    return out


def roundtrip_case():
    """20 x 300 with degrees that every metric accepts: for the half calls and the three-plane mode."""
    z = gen.scatter((20, 300), 23, 0.01, np.float32)
    z[7, :] = 0
    xs, ys = gen.geo(20, 300, -30.0, 12.0)
    return Case("roundtrip_20x300", z, xs, ys, "half calls and mode 3", metrics=METRIC_NAMES)


def great_circle_cases():
    """300 x 40 on uneven degrees, and the round-the-back construction of test_gpu_proximity.py at 300 rows (longitudes
    -178.9 .. 178.7; the latitudes' scale is the one that keeps 300 rows between 70 and 56 degrees)."""
    z = gen.scatter((300, 40), 41, 0.01, np.int32)
    xs, ys = gen.geo(300, 40, -30.0, 12.0)
    out = [Case("gc_300x40", z, xs, ys, "a long row list under haversine", metrics=("GREAT_CIRCLE",))]
    z = gen.scatter((300, 90), 31, 0.01, np.int32)
    z[2, 0], z[7, -1], z[9, 1] = 5, 6, 7
    xs, ys = gen.geo(300, 90, -178.9, 70.0)
    xs = -178.9 + (xs - xs[0]) * (357.6 / (xs[-1] - xs[0]))
    ys = 70.0 + (ys - ys[0]) * 4.8
    out.append(Case("gc_wrap_300x90", z, xs, ys, "the row's far end is the near one round the back", metrics=("GREAT_CIRCLE",)))
    return out


def tie_counts(case, metric):
    """how many targets share the winner's d32, per cell (brute force)"""
    z, xs, ys = case.z, np.asarray(case.xs, np.float64), np.asarray(case.ys, np.float64)
    tr, tc = np.nonzero(po.targets(z, case.tv))
    out = np.zeros(z.shape, np.int64)
    for i in range(z.shape[0]):
        d = po.distance(xs[tc][None, :], xs[:, None], ys[tr][None, :], ys[i], po.METRICS[metric])
        out[i] = (d == d.min(axis=1)[:, None]).sum(axis=1)
    return out


# ------------------------------------------------------------------------------------------------ the model of the walk
CLOSED_BY = ("rows", "bound", "max_distance")                             # how a side ended: out of rows | bound > best | bound^2 > max2


def walk(case, metric, extend=True):
    """proximity_search_kernel, lane by lane in NumPy: from the cell's place in the row list outwards, above and below in
    turn; per row the nearest-left and nearest-right candidate (and the row's first and last target where longitudes span
    more than 180 degrees); a side closes on float32(bound) > best or bound^2 > max2; with `extend`, EUCLIDEAN and MANHATTAN
    move the winner to the far end of its run of equal d32 in its row, found by bisection (`tied_end` of the kernel; the
    kernel's `may_tie` is a filter in front of it that changes no result, and is left out here).

    Returns per cell: row, col (the winner, -1 for none), up / dn (rows visited on each side, pruned ones not counted),
    up_closed / dn_closed (index into CLOSED_BY), extended (a tie run moved the winner), at_cut (visited rows whose
    bound^2 equals max2 exactly)."""
    m = po.METRICS[metric]
    z = case.z
    xs, ys = np.asarray(case.xs, np.float64), np.asarray(case.ys, np.float64)
    rows, cols = z.shape
    sc = scan_reference(po.targets(z, case.tv))
    left, right, lst, n = sc["left"], sc["right"], sc["list"], sc["count"]
    max2 = np.inf if np.isinf(case.md) else np.float64(case.md) ** 2
    lat = np.radians(ys)
    wraps = m == 1 and abs(np.radians(xs[-1]) - np.radians(xs[0])) > np.pi
    cells = rows * cols
    res = {k: np.full((rows, cols), -1, np.int64) for k in ("row", "col")}
    res.update({k: np.zeros((rows, cols), np.int64) for k in ("up", "dn", "up_closed", "dn_closed", "at_cut")})
    res["extended"] = np.zeros((rows, cols), bool)
    lanes = np.arange(cols)

    def d32_of(i, r, c, j):
        return po.distance(xs[c], xs[j], ys[r], ys[i], m)

    def tied_end(i, r, c, j, d32, above):
        if above:
            if c > j or c == 0:
                return c
            nb = left[r, c - 1]
            if nb < 0 or d32_of(i, r, nb, j) != d32:
                return c
            lo, hi = 0, int(nb)
            while lo < hi:
                mid = (lo + hi) >> 1
                if d32_of(i, r, mid, j) == d32:
                    hi = mid
                else:
                    lo = mid + 1
            return lo if left[r, lo] == lo else int(right[r, lo])
        if c <= j:
            return c
        nb = right[r, c]
        if nb < 0 or d32_of(i, r, nb, j) != d32:
            return c
        lo, hi = int(nb), cols - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if d32_of(i, r, mid, j) == d32:
                lo = mid
            else:
                hi = mid - 1
        return int(left[r, lo])

    for i in range(rows):
        lo = int(np.searchsorted(lst, i, side="right")) - 1
        best = np.full(cols, np.inf, np.float32)
        best_key = np.full(cols, np.iinfo(np.int64).max, np.int64)
        best_r, best_c = np.full(cols, -1, np.int64), np.full(cols, -1, np.int64)
        is_open = {True: np.ones(cols, bool), False: np.ones(cols, bool)}
        for step in range(max(lo + 1, n - lo - 1)):
            for above, k in ((True, lo - step), (False, lo + 1 + step)):
                if not 0 <= k < n or not is_open[above].any():
                    continue
                r = int(lst[k])
                side = "up" if above else "dn"
                if m == 1:
                    bound = np.float32(6378137.0 * abs(lat[i] - lat[r]) * (1.0 - 1e-12))
                else:
                    bound = np.float32(abs(ys[r] - ys[i]))
                over = np.float64(bound * bound) > max2
                shut = is_open[above] & ((bound > best) | over)
                res[side + "_closed"][i][shut] = np.where(bound > best[shut], 1, 2)
                is_open[above] &= ~shut
                go = is_open[above]
                res[side][i] += go
                if np.float64(bound * bound) == max2:
                    res["at_cut"][i] += go
                cands = [left[r], right[r]]
                if wraps:
                    cands += [np.full(cols, 0 if left[r, 0] == 0 else right[r, 0]), np.full(cols, left[r, cols - 1])]
                for c in cands:
                    c = c.astype(np.int64)
                    ok = go & (c >= 0)
                    d32 = d32_of(i, r, np.where(ok, c, 0), lanes)
                    key = r * cols + c if above else 2 * cells - (r * cols + c)
                    better = ok & ((d32 < best) | ((d32 == best) & (key < best_key)))
                    best = np.where(better, d32, best)
                    best_key = np.where(better, key, best_key)
                    best_r, best_c = np.where(better, r, best_r), np.where(better, c, best_c)
        if extend and m != 1:                                             # once per cell, after the walk
            for j in np.flatnonzero(best_r >= 0):
                e = tied_end(i, int(best_r[j]), int(best_c[j]), int(j), best[j], best_r[j] <= i)
                res["extended"][i, j] = e != best_c[j]
                best_c[j] = e
        kept = (best_r >= 0) & (max2 >= (best * best).astype(np.float64))
        res["row"][i], res["col"][i] = np.where(kept, best_r, -1), np.where(kept, best_c, -1)
    return res

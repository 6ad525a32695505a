"""Inputs, a CPU model of the wave paths and exact references for the zonal reduction kernels (xrspatial_amd/csrc/zonal.hip),
shared by tests/test_zonal_partials_host.py (no GPU: the inputs reach the paths they are named for) and
tests/test_gpu_zonal_partials.py (the MI355X: the tables equal the references).  NumPy only; nothing here imports the package.

Geometry of zonal_kernel, re-derived from the source: a workgroup of 1024 threads takes trips of 1024 x U 16-byte slots
(U = 2, or 4 when the LDS table is larger than 64 KiB and both planes are 16-byte aligned); chunks are whole trips, so wave w
of the raster always covers the 64 U slots from w * 64 U on (256 U cells), slot u of it the 256 cells from (w U + u) * 256 on,
a lane 4 consecutive cells and a row of 16 lanes 64 cells.  The n % 4 last cells -- every cell when a plane is not 16-byte
aligned -- go through the scalar tail."""
import math
from dataclasses import dataclass, field

import numpy as np

I32 = np.iinfo(np.int32)
RUN_LONG = 2048                                   # cells: 4 waves of U = 2, 2 waves of U = 4
LDS_CAP, LDS_TWO_PER_CU = 144 * 1024, 64 * 1024   # zonal_partials<VT>(): lds_cap, the `big` threshold
PATHS = ("one_zone", "one_zone_skipped", "one_zone_no_valid", "rows16", "mixed", "lane_by_lane", "over8", "lane_split",
         "partial_wave", "tail_cells")


def per_zone(dtype):
    return 16 + 2 * np.dtype(dtype).itemsize + 4  # sum f64, sumsq f64, min, max, count u32


def launch_window(dtype):
    """Zones of one launch: 5266 for float32 values, 4096 for float64."""
    return LDS_CAP // per_zone(dtype)


def launches(n_zones, dtype, aligned=True):
    """[(zbase, zones of the launch, U)] as zonal_partials<VT>() splits `n_zones`."""
    w = launch_window(dtype)
    out = []
    for base in range(0, n_zones, w):
        nzw = min(w, n_zones - base)
        out.append((base, nzw, 4 if aligned and nzw * per_zone(dtype) > LDS_TWO_PER_CU else 2))
    return out


# ------------------------------------------------------------------------------------------------------ layouts
def runs(length, run, ids):
    """`length` cells: the ids of `ids` in turn (again from the first when they run out), `run` cells each."""
    k = -(-length // run)
    return np.repeat(np.resize(np.asarray(ids, dtype=np.int32), k), run)[:length]


def segment_layout(n, n_zones, slots, seed, outside=True, dead_at="long", long_ids=None):
    """A dense index plane of `n` cells laid out as segments, one kind of run each:

        runs of RUN_LONG cells      -> whole waves in one zone, in a zone outside the table, in a zone without a valid value
        runs of 128, one trip       -> rows of 16 lanes in one zone
        runs of 100, one trip       -> waves that mix such rows with rows that straddle two zones
        uniformly random, one trip  -> more than 8 runs under a slot
        runs of 37 to the end       -> lane by lane, zone boundaries inside a lane's 4 cells; the last wave is partial

    `outside`: zones outside the table (-1 and n_zones) in the long runs and strewn over the random trip.  Zone n_zones - 1
    (returned) is drawn nowhere: it is for the caller to make invalid, and is placed by `dead_at`: 'long' a RUN_LONG run,
    'run100' one run of 100, 'tail' the last cell (n % 4 must not be 0), None nowhere."""
    rng = np.random.default_rng(seed)
    trip = 4096 * slots
    dead = n_zones - 1
    pool = np.arange(n_zones - 1)
    if long_ids is None:
        lo, hi = (-1, n_zones) if outside else (pool[2 % pool.size], pool[3 % pool.size])
        long_ids = [pool[1 % pool.size], lo, dead if dead_at == "long" else pool[4 % pool.size], hi, pool[-1]]
    parts = [runs(len(long_ids) * RUN_LONG, RUN_LONG, long_ids)]
    parts.append(runs(trip, 128, rng.choice(pool, trip // 128)))
    ids100 = rng.choice(pool, trip // 100 + 1)
    if dead_at == "run100":
        ids100[5] = dead
    parts.append(runs(trip, 100, ids100))
    scattered = rng.choice(pool, trip).astype(np.int32)
    if outside:
        u = rng.random(trip)
        scattered[u < 0.01] = -1
        scattered[u > 0.99] = n_zones
    parts.append(scattered)
    head = sum(p.size for p in parts)
    assert n > head, (n, head)
    parts.append(runs(n - head, 37, rng.choice(pool, (n - head) // 37 + 1)))
    z = np.concatenate(parts).astype(np.int32)
    if dead_at == "tail":
        assert n % 4
        z[-1] = dead
    return z, dead


def layout_length(slots, tail):
    """40 000 + tail cells for U = 2, 80 000 + tail for U = 4: the last trip is partial, and so is its last wave."""
    return 20_000 * slots + tail


# ------------------------------------------------------------------------------------------------------- values
def value_plane(z, dtype, seed, nodata=None, dead=None, specials=True):
    """Integer-valued float32 in [-2000, 2000] / float64 multiples of 0.25 in the same range; 1 % NaN, 0.5 % +inf, 0.5 % -inf
    and 2 % `nodata` (when it is a finite number) strewn over every segment; the cells of zone `dead` hold invalid values
    only."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        v = rng.integers(-2000, 2001, z.size).astype(np.float32)
    else:
        v = rng.integers(-8000, 8001, z.size) * 0.25
    finite_nodata = nodata is not None and math.isfinite(nodata)
    if specials:
        u = rng.random(z.size)
        v[u < 0.01] = np.nan
        v[(u >= 0.01) & (u < 0.015)] = np.inf
        v[(u >= 0.015) & (u < 0.02)] = -np.inf
        if finite_nodata:
            v[(u >= 0.02) & (u < 0.04)] = nodata
    if dead is not None:
        where = np.flatnonzero(z == dead)
        v[where] = np.resize(np.array([np.nan, np.inf, nodata if finite_nodata else np.nan, -np.inf], dtype=dtype), where.size)
    return v


def valid(v, nodata=None):
    """zonal.py: isfinite(values) & (values != nodata)."""
    ok = np.isfinite(v)
    if nodata is not None:
        ok &= v != nodata
    return ok


# ------------------------------------------------------------------------------------------------ the wave model
def wave_paths(z, ok, n_zones, slots, aligned=True):
    """What zonal_kernel does with index plane `z` (as the launch sees it: after the table and minus zbase) and value
    validity `ok`: the number of wave-slots (waves for the one-zone paths, lanes for lane_split, cells for tail_cells) on each path.

        one_zone            the wave's trip in one zone of the table, at least one valid cell
        one_zone_skipped    ... in one index outside [0, n_zones) (also a wave past the end of the data)
        one_zone_no_valid   ... in one zone of the table, no valid cell
        rows16              rows of 16 lanes folded by row16_reduce
        mixed               slots in which some rows are folded and other lanes add their own partial
        lane_by_lane        slots of at most 8 runs without a folded row
        over8               slots of more than 8 runs (no row test)
        lane_split          lanes that add cells one by one because a zone boundary cuts through their 4 cells
        partial_wave        waves that the end of the 16-byte body cuts through
        tail_cells          cells of the scalar tail"""
    z = np.asarray(z).astype(np.int64).ravel()
    ok = np.asarray(ok, dtype=bool).ravel()
    out = dict.fromkeys(PATHS, 0)
    n4 = z.size // 4 if aligned else 0
    out["tail_cells"] = int(z.size - 4 * n4)
    if n4 == 0:
        return out
    per_wave = 64 * slots
    waves = -(-n4 // per_wave)
    shape = (waves, slots, 64, 4)
    Z = np.full(waves * per_wave * 4, -1, np.int64)
    Z[:4 * n4] = z[:4 * n4]
    OK = np.zeros(Z.size, bool)
    OK[:4 * n4] = ok[:4 * n4]
    Z, OK = Z.reshape(shape), OK.reshape(shape)
    OK &= (Z >= 0) & (Z < n_zones)                                    # cell_ok
    out["partial_wave"] = int(n4 % per_wave != 0)
    z0 = Z[:, 0, 0, 0]
    same = (Z == z0[:, None, None, None]).all(axis=(1, 2, 3))
    in_table = same & (z0 >= 0) & (z0 < n_zones)
    any_ok = OK.any(axis=(1, 2, 3))
    out["one_zone"] = int((in_table & any_ok).sum())
    out["one_zone_no_valid"] = int((in_table & ~any_ok).sum())
    out["one_zone_skipped"] = int((same & ~in_table).sum())
    Z, OK = Z[~same], OK[~same]
    if Z.shape[0] == 0:
        return out
    first = OK.argmax(axis=-1)
    pz = np.where(OK.any(axis=-1), np.take_along_axis(Z, first[..., None], axis=-1)[..., 0], -1)   # the lane's partial
    out["lane_split"] = int((OK & (Z != pz[..., None])).any(axis=-1).sum())
    starts = np.ones(pz.shape, bool)
    starts[..., 1:] = pz[..., 1:] != pz[..., :-1]
    over = starts.sum(axis=-1) > 8
    rows = pz.shape[:-1] + (4, 16)
    row_one = ~starts.reshape(rows)[..., 1:].any(axis=-1) & (pz.reshape(rows)[..., 0] >= 0) & ~over[..., None]
    own = ((pz.reshape(rows) >= 0) & ~row_one[..., None]).any(axis=(-1, -2))
    has_row = row_one.any(axis=-1)
    out["rows16"] = int(row_one.sum())
    out["mixed"] = int((has_row & own).sum())
    out["lane_by_lane"] = int((~over & ~has_row).sum())
    out["over8"] = int(over.sum())
    return out


def paths_of_call(z, ok, n_zones, dtype, aligned=True, base_only=None):
    """wave_paths summed over the launches of one call on `n_zones` zones; base_only: only the launches with that
    property ('nonzero': zbase != 0)."""
    total = dict.fromkeys(PATHS, 0)
    for base, nzw, slots in launches(n_zones, dtype, aligned):
        if base_only == "nonzero" and base == 0:
            continue
        got = wave_paths(np.asarray(z, np.int64) - base, ok, nzw, slots, aligned)
        for k in PATHS:
            total[k] += got[k]
    return total


# --------------------------------------------------------------------------------------------------- references
def reference(z, v, n_zones, shift=0.0, nodata=None):
    """count (np.bincount), min / max (np.minimum.at / np.maximum.at), and the sums of (x - shift) and (x - shift)^2 in exact
    integer arithmetic: the values are multiples of 1/4, so 4 (x - shift) is an integer, the sums are taken in int64 and
    divided by 4 and 16 -- exact, like every partial sum in any order, as long as the sum of the squares stays below 2^53
    (asserted)."""
    z, v = np.asarray(z).ravel(), np.asarray(v).ravel()
    ok = valid(v, nodata) & (z >= 0) & (z < n_zones)
    zi, x = z[ok].astype(np.int64), v[ok]
    t = (x.astype(np.float64) - shift) * 4.0
    t4 = t.astype(np.int64)
    assert (t4 == t).all()
    assert int((t4 * t4).sum()) < 2 ** 53
    s, q = np.zeros(n_zones, np.int64), np.zeros(n_zones, np.int64)
    np.add.at(s, zi, t4)
    np.add.at(q, zi, t4 * t4)
    mn, mx = np.full(n_zones, np.inf, v.dtype), np.full(n_zones, -np.inf, v.dtype)
    np.minimum.at(mn, zi, x)
    np.maximum.at(mx, zi, x)
    return {"count": np.bincount(zi, minlength=n_zones).astype(np.uint64), "sum": s / 4.0, "sumsq": q / 16.0, "min": mn, "max": mx}


def reference_fsum(z, v, n_zones, shift, nodata=None):
    """For values that are no multiples of 1/4: per zone math.fsum of the float64 terms x - shift and (x - shift)^2, and
    the bound m * 2^-52 * sum |t| on a float64 sum of the m terms taken in any order (twice the textbook (m - 1) * 2^-53 *
    sum |t|: the factor covers the rounding of each term and a fused multiply-add).  Returns (sum, sumsq, bound of sum,
    bound of sumsq)."""
    z, v = np.asarray(z).ravel(), np.asarray(v).ravel()
    ok = valid(v, nodata) & (z >= 0) & (z < n_zones)
    zi, t = z[ok], v[ok].astype(np.float64) - shift
    order = np.argsort(zi, kind="stable")
    zi, t = zi[order], t[order]
    cuts = np.searchsorted(zi, np.arange(n_zones + 1))
    out = np.zeros((4, n_zones))
    for k in range(n_zones):
        tk = t[cuts[k]:cuts[k + 1]]
        m = tk.size
        out[0, k], out[1, k] = math.fsum(tk), math.fsum(tk * tk)
        out[2, k], out[3, k] = m * 2.0 ** -52 * math.fsum(np.abs(tk)), m * 2.0 ** -52 * math.fsum(tk * tk)
    return out


# -------------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    """One call: `z` is the plane the ABI gets (dense indices; raw ids for the LUT and window variants), `idx` what the
    launch makes of it (dense indices, -1 / n_zones: no zone)."""
    name: str
    dtype: type
    z: np.ndarray
    v: np.ndarray
    n_zones: int
    nodata: object = None          # None: has_nodata = 0
    shift: float = 0.0
    need: tuple = ()               # the paths the case is named for
    need_nonzero_base: tuple = ()  # ... in the launches with zbase != 0
    idx: np.ndarray = None
    extra: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.idx is None:
            self.idx = self.z

    @property
    def ok(self):
        return valid(self.v, self.nodata)


ALL_PATHS = PATHS
DENSE_ZONES = {2: {np.float32: 40, np.float64: 40}, 4: {np.float32: 3000, np.float64: 2000}}
NODATA = {"none": None, "17": 17.0, "nan": float("nan"), "inf": float("inf")}
SHIFTS = {np.float32: 3.0, np.float64: -12.0}
VTYPES = (np.float32, np.float64)


def dense_cases(dtype):
    """The segment layout for U = 2 and U = 4 under each nodata setting."""
    out = []
    for slots in (2, 4):
        nz = DENSE_ZONES[slots][dtype]
        assert launches(nz, dtype) == [(0, nz, slots)]
        for tag, nodata in NODATA.items():
            z, dead = segment_layout(layout_length(slots, 3), nz, slots, seed=slots)
            v = value_plane(z, dtype, seed=10 + slots, nodata=nodata, dead=dead)
            out.append(Case(f"U{slots}-nodata_{tag}", dtype, z, v, nz, nodata, SHIFTS[dtype], need=ALL_PATHS, extra={"dead": dead}))
    return out


TAILS = (1, 2, 3, 4, 5, 1023, 4097, 40_000, 40_001, 40_002, 40_003)
ALIGN = ((0, 0), (0, 1), (1, 0))                 # (zone plane shift, value plane shift) in elements


def tail_cases(dtype):
    """Lengths around the 16-byte slots, the wave and the trip: the U = 2 layout, of which the short lengths take the end (runs
    of 37)."""
    nz = 40
    full, _ = segment_layout(40_003, nz, 2, seed=21, dead_at=None)
    out = []
    for n in TAILS:
        z = full[:n] if n >= 40_000 else full[-n:]
        v = value_plane(z, dtype, seed=n, nodata=17.0)
        need = ("tail_cells",) if n % 4 else ()
        if n >= 40_000:
            need += ("one_zone", "rows16", "mixed", "over8", "lane_split", "partial_wave")
        out.append(Case(f"n{n}", dtype, z, v, nz, 17.0, SHIFTS[dtype], need=need))
    return out


WINDOW_ZONES = {np.float32: 12_000, np.float64: 9_000}


def windows_case(dtype):
    """More zones than one launch holds: RUN_LONG runs of the indices on both sides of every window boundary and of the last
    zone but one (the last is the zone without a valid cell), then the segments over all zones."""
    nz, w = WINDOW_ZONES[dtype], launch_window(dtype)
    assert [b for b, _, _ in launches(nz, dtype)] == [0, w, 2 * w]
    long_ids = [w - 1, w, 2 * w - 1, 2 * w, nz - 2, 0, -1, nz, nz - 1, w + 7]
    z, dead = segment_layout(120_003, nz, 4, seed=31, long_ids=long_ids)
    v = value_plane(z, dtype, seed=32, nodata=17.0, dead=dead)
    need = ("one_zone", "one_zone_no_valid", "rows16", "mixed", "lane_split")
    return Case("windows", dtype, z, v, nz, 17.0, SHIFTS[dtype], need=ALL_PATHS, need_nonzero_base=need, extra={"dead": dead})


def edge_cases(dtype):
    """min / max at the ends of the format: a zone of +-0.0 only, subnormals, the largest finite values; each zone once in a
    RUN_LONG run (one-zone path), in runs of 128 (rows), and scattered (lane by lane)."""
    fi = np.finfo(dtype)
    big = fi.max if dtype == np.float32 else fi.max / 2
    pools = [np.array([0.0, -0.0]), np.array([fi.smallest_subnormal, -fi.smallest_subnormal, 3 * fi.smallest_subnormal]),
             np.array([fi.smallest_subnormal, fi.tiny, 1.0]), np.array([-fi.tiny, -fi.smallest_subnormal, -1.0]),
             np.array([big, -big, 1.0]), np.array([big, 2.0]), np.array([-big, -2.0])]
    nz = len(pools)
    rng = np.random.default_rng(41)
    z = np.concatenate([runs(nz * RUN_LONG, RUN_LONG, np.arange(nz)), runs(8192, 128, rng.permutation(np.arange(64) % nz)),
                        rng.integers(0, nz, 8192 + 3).astype(np.int32)])
    v = np.zeros(z.size, dtype)
    for k, pool in enumerate(pools):
        where = np.flatnonzero(z == k)
        v[where] = pool.astype(dtype)[rng.integers(0, pool.size, where.size)]
    return Case("edges", dtype, z, v, nz, None, 0.0, need=("one_zone", "rows16", "over8", "tail_cells"))


def conditioning_case(dtype):
    """Non-integral values far from 0 with a small spread, the shift near their mean."""
    base, spread = (3.0e5, 0.05) if dtype == np.float32 else (1.0e7, 1e-3)
    z, _ = segment_layout(40_003, 40, 2, seed=51, dead_at=None)
    rng = np.random.default_rng(52)
    v = (base + rng.uniform(-spread, spread, z.size)).astype(dtype)
    v[rng.random(z.size) < 0.01] = np.nan
    return Case("conditioning", dtype, z, v, 40, None, base, need=("one_zone", "rows16", "mixed", "over8", "lane_split"))


# ---- the LUT variant: raw ids through a table over [zone_min, zone_min + zone_range)
def lut_table(ids, zone_min, zone_range):
    """int32 table: dense index of every id of `ids` (ascending), -1 elsewhere."""
    lut = np.full(zone_range, -1, np.int32)
    lut[np.asarray(ids, np.int64) - zone_min] = np.arange(len(ids), dtype=np.int32)
    return lut


def lut_map(raw, zone_min, lut):
    """The dense index plane the kernel must see, in Python-int arithmetic via int64."""
    off = raw.astype(np.int64) - zone_min
    inside = (off >= 0) & (off < lut.size)
    idx = np.full(raw.shape, -1, np.int32)
    idx[inside] = lut[off[inside]]
    return idx


LUT_SETS = {                      # name -> (n ids, zone_min, step between ids, slots of the layout)
    "gaps": (40, 100, 3, 2),
    "negative_min": (40, -500, 7, 2),
    "int32_min": (40, I32.min, 5, 2),
    "two_launches": (6000, -9000, 2, 4),
}


def lut_cases(dtype):
    """Raw ids zone_min + step * k (gaps: table entries of -1 between them); the table's window ends a little above the last
    id.  The cells the layout gives no zone hold, in turn: an id below zone_min (where there is one), ids above the window --
    INT32_MAX among them --, and an id inside the window whose table entry is -1."""
    out = []
    for name, (k, zone_min, step, slots) in LUT_SETS.items():
        ids = zone_min + step * np.arange(k, dtype=np.int64)
        zone_range = int(ids[-1] - zone_min) + 4
        lut = lut_table(ids, zone_min, zone_range)
        idx, dead = segment_layout(layout_length(slots, 3), k, slots, seed=61 + k + step)
        strangers = [I32.max, zone_min + zone_range, zone_min + 1, zone_min + zone_range + 12345, I32.max - 1]
        if zone_min > I32.min:
            strangers += [zone_min - 1, I32.min]
        raw = np.empty(idx.size, np.int64)
        none = (idx < 0) | (idx >= k)
        raw[~none] = ids[idx[~none]]
        raw[none] = np.resize(np.array(strangers, np.int64), int(none.sum()))
        assert none[RUN_LONG:2 * RUN_LONG].all() and none[3 * RUN_LONG:4 * RUN_LONG].all()
        raw[RUN_LONG:2 * RUN_LONG] = I32.max                           # (the long runs without a zone: runs of ONE raw id)
        raw[3 * RUN_LONG:4 * RUN_LONG] = strangers[-2]
        raw = raw.astype(np.int32)
        mapped = lut_map(raw, zone_min, lut)
        assert ((mapped < 0) == none).all() and (mapped[~none] == idx[~none]).all()
        v = value_plane(raw, dtype, seed=62 + k, nodata=17.0)
        v[idx == dead] = np.nan
        out.append(Case(f"lut-{name}", dtype, raw, v, k, 17.0, SHIFTS[dtype], need=ALL_PATHS, idx=mapped,
                        need_nonzero_base=("rows16",) if len(launches(k, dtype)) > 1 else (),
                        extra={"zone_min": zone_min, "zone_range": zone_range, "lut": lut, "dead": dead}))
    return out


# ---- the window variant: raw ids, tables indexed by id - base
WINDOW_BASES = {"zero": lambda w: 0, "far": lambda w: 1_000_000, "negative": lambda w: -5000 - w // 2,
                "int32_min": lambda w: I32.min, "int32_top": lambda w: I32.max + 1 - w}
WINDOW_SIZES = (256, 4096)
DEAD_AT = ("long", "run100", "tail")
STRAYS = ("long", "scattered", "tail")


def window_slots(window, dtype):
    return launches(window, dtype)[0][2]


def window_case(dtype, base_name, window, dead_at="long", stray=None):
    """All ids inside [base, base + window), one id with invalid values only (placed by `dead_at`); `stray`: ONE cell holds an
    id outside the window -- in a RUN_LONG run, in the random trip, or as the last cell (scalar tail); for the two bases at the
    ends of int32 it is the id at the other end."""
    base = WINDOW_BASES[base_name](window)
    slots = window_slots(window, dtype)
    idx, dead = segment_layout(layout_length(slots, 3), window, slots, seed=71 + window, outside=False, dead_at=dead_at)
    raw = (idx.astype(np.int64) + base)
    need = ("one_zone", "rows16", "mixed", "over8", "lane_split", "partial_wave", "tail_cells")
    need += {"long": ("one_zone_no_valid",), "run100": (), "tail": ()}[dead_at]
    extra = {"base": base, "window": window, "dead": dead, "dead_at": dead_at}
    if stray is not None:
        trip = 4096 * slots
        where = {"long": RUN_LONG // 2 + 5, "scattered": 5 * RUN_LONG + 2 * trip + 777, "tail": raw.size - 1}[stray]
        assert stray != "tail" or dead_at != "tail"
        outside_id = {"int32_min": I32.max, "int32_top": I32.min}.get(base_name, base + window if stray != "scattered" else base - 1)
        raw[where] = outside_id
        idx = idx.copy()
        idx[where] = -1
        extra.update(stray=stray, stray_at=where)
    raw = raw.astype(np.int32)
    assert stray is not None or ((raw.astype(np.int64) - base == idx).all() and idx.min() >= 0 and idx.max() < window)
    v = value_plane(raw, dtype, seed=72 + window, nodata=17.0)
    v[idx == dead] = np.resize(np.array([np.nan, 17.0, np.inf, -np.inf], dtype=dtype), int((idx == dead).sum()))
    if stray is not None:
        v[extra["stray_at"]] = 5.0                        # (a valid value: counted anywhere, it would show)
    return Case(f"window-{base_name}-{window}-dead_{dead_at}-stray_{stray}", dtype, raw, v, window, 17.0, SHIFTS[dtype],
                need=need, idx=idx, extra=extra)


def window_cases(dtype):
    out = []
    for window in WINDOW_SIZES:
        for base_name in WINDOW_BASES:
            out.append(window_case(dtype, base_name, window))
        for dead_at in DEAD_AT[1:]:
            out.append(window_case(dtype, "far", window, dead_at=dead_at))
    return out


def stray_cases(dtype):
    out = []
    for window in WINDOW_SIZES:
        for stray in STRAYS:
            out.append(window_case(dtype, "far", window, stray=stray))
        for base_name in ("int32_min", "int32_top"):
            out.append(window_case(dtype, base_name, window, stray="long"))
    return out


def all_cases(dtype):
    return (dense_cases(dtype) + tail_cases(dtype) + [windows_case(dtype), edge_cases(dtype), conditioning_case(dtype)]
            + lut_cases(dtype) + window_cases(dtype) + stray_cases(dtype))


def case_paths(case, aligned=True, base_only=None):
    return paths_of_call(case.idx, case.ok, case.n_zones, case.dtype, aligned, base_only)


# ---- the three layouts of tests/test_gpu_parity.py that compared partials with the oracle before this module existed
def earlier_layouts():
    """name -> (dense index plane, validity, zones): test_zonal_vs_oracle (blocky), test_zonal_large_offset_small_spread,
    test_zonal_one_pass_discovery (block ids)."""
    from tests import synth
    out = {}
    rng = np.random.default_rng(5)
    zones = synth.block_zones(300, 517, n_zones=40, block=37)
    ok = ~(rng.random((300, 517)) < 0.01)
    out["test_zonal_vs_oracle"] = (zones.ravel(), ok.ravel(), 40)
    rng = np.random.default_rng(8)
    zones = synth.block_zones(300, 400, n_zones=12, block=23)
    rng.normal(0, 0.05, zones.shape)
    ok = ~(rng.random(zones.shape) < 0.01)
    out["test_zonal_large_offset_small_spread"] = (zones.ravel(), ok.ravel(), 12)
    rng = np.random.default_rng(11)
    ok = ~(rng.random((700, 900)) < 0.01)
    blocks = ((np.arange(700)[:, None] // 37) * 31 + np.arange(900)[None, :] // 53) % 400
    ok &= (blocks != blocks[300, 450]) & (blocks != blocks[10, 10])          # (the test's two zones without a valid cell)
    out["test_zonal_one_pass_discovery"] = (blocks.ravel().astype(np.int32), ok.ravel(), 400)
    return out

"""Inputs, a CPU model of the plan and the hashes, and the exact reference for zonal `majority` on continuous data
(xrspatial_amd/csrc/zonal_mode.hip: cells routed by zone, then by a hash of the value, counted in LDS hash tables;
xrspatial_amd/csrc/zonal_majority.hip: two radix sorts and run voting), shared by tests/test_zonal_majority_host.py (no GPU:
every case reaches the path it is named for) and tests/test_gpu_zonal_majority.py (the MI355X: both device paths equal the
reference, and the header words of the workspace equal the model's).  NumPy only; nothing here imports the package.

The model is integer arithmetic on the keys: zone sizes -> parts_log2 -> the header (n_valid, n_parts, n_chunks, n_direct);
keys -> part_of -> the cells of every part; keys -> sieve_slot -> the keys of a part that reach the compare-and-swap table.
count_kernel sends a cell to the table when the cells of its sieve slot are not all its own (`f_cnt[slot] != add`); without a
wave whose 64 keys are one value, add is 1 and that is: the slot holds more than ONE cell -- a key that occurs twice goes to
the table even when no other key shares its slot.  A part overflows exactly when more than SLOTS distinct keys reach the
table (linear probing visits every slot in SLOTS rounds and occupied slots stay occupied, so a key is turned away only by a
full table of other keys).  With wave-uniform groups (add = 64) the model's table_keys is an upper bound."""
from dataclasses import dataclass, field

import numpy as np

TILE = 4096                    # zonal_mode.hip:38  TILE = TILE_THREADS (256) * PER_THREAD (16)
CHUNK = 8192                   # zonal_mode.hip:49  CHUNK = XRS_MODE_CHUNK_THREADS (512, :40) * PER_THREAD (16, :37)
PART_TARGET = 1024             # zonal_mode.hip:46  XRS_MODE_PART_TARGET
MAX_B = 16                     # zonal_mode.hip:51
LDS_B = 11                     # zonal_mode.hip:52
SLOTS = 2048                   # zonal_mode.hip:43  XRS_MODE_SLOTS
MAX_ZONES = 16384              # zonal_mode.hip:57
BATCH = 1024                   # zonal_mode.hip:407 CNT_BATCH (4) keys of each of count_kernel's 256 threads
COUNT_GRID = 4096              # zonal_mode.hip:695 g1: workgroups of zone_count_kernel, each a TILE per trip
VOTE_PER = 8                   # zonal_majority.hip:75
VOTE_BLOCK = 256 * VOTE_PER    # zonal_majority.hip:236 runs of one workgroup of vote_kernel
MULT = {32: 0x9E3779B1, 64: 0x9E3779B97F4A7C15}        # zonal_mode.hip:85, :87  part_of
TABLE_XOR = 0x68E31DA4         # zonal_mode.hip:488


# ------------------------------------------------------------------------------------------- keys and hashes
def width(dtype):
    return 8 * np.dtype(dtype).itemsize


def _uint(w):
    return np.uint32 if w == 32 else np.uint64


def canon(v):
    """-0.0 -> +0.0 (scatter_zone_kernel :232, make_keys_kernel :58): np.unique counts them as one value."""
    v = np.asarray(v)
    return np.where(v == 0, v.dtype.type(0), v)


def enc(v):
    """Key<VT>::enc (zonal_mode.hip:62-65, :73-76): an unsigned integer that orders as the value does."""
    v = np.ascontiguousarray(v)
    w = width(v.dtype)
    U = _uint(w)
    b = v.view(U)
    top = U(1) << U(w - 1)
    return np.where(b & top, ~b, b | top).astype(U)


def dec(k, dtype):
    """Key<VT>::dec (:66-69, :77-80), as float64."""
    k = np.ascontiguousarray(k)
    w = width(dtype)
    U = _uint(w)
    top = U(1) << U(w - 1)
    b = np.where(k & top, k & ~top, ~k).astype(U)
    with np.errstate(invalid="ignore"):                            # (a signalling NaN's key)
        return b.view(np.dtype(dtype)).astype(np.float64)


def part_of(k, B):
    """part_of<K> (:85-88): the top B bits of key * MULT modulo 2^w; B may be an array.  (B = 0: the zone is its own part.)"""
    k = np.asarray(k)
    w = 8 * k.dtype.itemsize
    U = _uint(w)
    B = np.asarray(B)
    with np.errstate(over="ignore"):
        h = k * U(MULT[w])
    shift = np.where(B > 0, w - B, 0).astype(U)
    return np.where(B > 0, h >> shift, U(0)).astype(np.int64)


def _mix32(h):
    """slot_of(unsigned) (:90-93): the murmur3 finaliser, masked to the table."""
    h = np.asarray(h).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = h ^ (h >> np.uint32(16))
        h = h * np.uint32(0x85ebca6b)
        h = h ^ (h >> np.uint32(13))
        h = h * np.uint32(0xc2b2ae35)
        h = h ^ (h >> np.uint32(16))
    return (h & np.uint32(SLOTS - 1)).astype(np.int64)


def sieve_slot(k):
    """slot_of(key) as the sieve uses it (:471, :484); 64-bit keys are folded first (:94)."""
    k = np.asarray(k)
    if k.dtype.itemsize == 8:
        k = (k ^ (k >> np.uint64(29)) ^ (k >> np.uint64(47))) & np.uint64(0xffffffff)
    return _mix32(k)


def table_slot(k):
    """First slot of a key in the compare-and-swap table (:488): slot_of(rotl(key, 15) ^ 0x68E31DA4)."""
    k = np.asarray(k)
    w = 8 * k.dtype.itemsize
    U = _uint(w)
    r = ((k << U(15)) | (k >> U(w - 15))) ^ U(TABLE_XOR)
    return sieve_slot(r.astype(U))


def parts_log2(count):
    """parts_log2 (:143-148)."""
    count = int(count)
    if count <= PART_TARGET + PART_TARGET // 4:
        return 0
    B = 1
    while B < MAX_B and (PART_TARGET << B) < count:
        B += 1
    return B


def keys_in_part(dtype, B, part, how_many, rng):
    """`how_many` distinct finite values of `dtype`, none zero or subnormal, whose key part_of() sends to `part` of 2^B:
    hash values with `part` in their top B bits, multiplied by the inverse of the (odd) multiplier modulo 2^w."""
    dtype = np.dtype(dtype)
    w = width(dtype)
    U = _uint(w)
    assert 0 <= part < (1 << B)
    inv = pow(MULT[w], -1, 1 << w)
    tiny = np.finfo(dtype).tiny
    out = np.empty(0, dtype)
    seen = np.empty(0, U)
    while out.size < how_many:
        low = rng.integers(0, (1 << (w - B)) - 1, 2 * how_many + 64, dtype=np.uint64, endpoint=True)
        h = ((np.uint64(part) << np.uint64(w - B)) if B else np.uint64(0)) | low
        with np.errstate(over="ignore"):
            k = (h.astype(U) * U(inv)).astype(U)
        _, first = np.unique(k, return_index=True)
        k = k[np.sort(first)]
        k = k[~np.isin(k, seen)]
        v = dec(k, dtype).astype(dtype)
        keep = np.isfinite(v) & (np.abs(v) >= tiny)
        out, seen = np.concatenate([out, v[keep]]), np.concatenate([seen, k[keep]])
    return out[:how_many]


# ------------------------------------------------------------------------------------------------- reference
def valid_mask(z, v, nz, nodata=None):
    ok = (z >= 0) & (z < nz) & np.isfinite(v)
    if nodata is not None:
        ok &= v != np.asarray(nodata, v.dtype)
    return ok


def reference(z, v, nz, nodata=None):
    """np.unique(valid values of the zone, return_counts=True) + the first argmax; NaN for a zone without a valid cell."""
    ok = valid_mask(z, v, nz, nodata)
    zz, vv = z[ok], v[ok]
    order = np.argsort(zz, kind="stable")
    vv = vv[order]
    ends = np.cumsum(np.bincount(zz, minlength=nz))
    out = np.full(nz, np.nan)
    lo = 0
    for zone, hi in enumerate(ends):
        if hi > lo:
            u, c = np.unique(vv[lo:hi], return_counts=True)
            out[zone] = u[np.argmax(c)]
        lo = hi
    return out


def reference_levels(z, v, nz, levels):
    """The same for a raster whose every cell is valid and holds one of the few sorted `levels`: np.bincount."""
    li = np.searchsorted(levels, v)
    assert (levels[li] == v).all() and z.min() >= 0 and z.max() < nz
    table = np.bincount(z.astype(np.int64) * levels.size + li, minlength=nz * levels.size).reshape(nz, levels.size)
    out = np.full(nz, np.nan)
    has = table.sum(axis=1) > 0
    out[has] = levels[table.argmax(axis=1)][has].astype(np.float64)
    return out


# ----------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    z: np.ndarray                   # int32 dense zone indices, any shape
    v: np.ndarray                   # float32 / float64 values
    nz: int
    nodata: float = None
    winners: dict = field(default_factory=dict)       # zone -> the value that must win (NaN: no valid cell)
    levels: np.ndarray = None       # every cell valid and one of these sorted values: the reference is a bincount
    expect: dict = field(default_factory=dict)        # what the model must say: B per zone, n_chunks, overflow, ...

    @property
    def n(self):
        return int(self.z.size)

    def want(self):
        if self.levels is not None:
            return reference_levels(self.z.ravel(), self.v.ravel(), self.nz, self.levels)
        return reference(self.z.ravel(), self.v.ravel(), self.nz, self.nodata)


@dataclass
class Model:
    counts: np.ndarray              # valid cells per zone
    B: np.ndarray                   # log2 of the parts of every zone
    n_valid: int
    n_parts: int
    n_chunks: int
    n_direct: int
    part_len: np.ndarray            # cells of every part, in the order of part_base
    table_keys: np.ndarray          # distinct keys of every part that reach the compare-and-swap table
    overflow: bool

    @property
    def header(self):
        """(n_valid, n_parts, n_chunks, n_direct): Hdr words 0, 1, 2 and 4; word 3 is the overflow count."""
        return self.n_valid, self.n_parts, self.n_chunks, self.n_direct

    @property
    def batches(self):
        return -(-int(self.part_len.max(initial=0)) // BATCH)


def _distinct_per_zone(case):
    """(zone, key, cells) of every distinct (zone, key) pair of the valid cells."""
    z, v = case.z.ravel(), case.v.ravel()
    if case.levels is not None:
        li = np.searchsorted(case.levels, v)
        table = np.bincount(z.astype(np.int64) * case.levels.size + li, minlength=case.nz * case.levels.size)
        at = np.flatnonzero(table)
        return at // case.levels.size, enc(canon(case.levels))[at % case.levels.size], table[at]
    ok = valid_mask(z, v, case.nz, case.nodata)
    zz, kk = z[ok].astype(np.int64), enc(canon(v[ok]))
    order = np.lexsort((kk, zz))
    zz, kk = zz[order], kk[order]
    head = np.ones(zz.size, bool)
    head[1:] = (zz[1:] != zz[:-1]) | (kk[1:] != kk[:-1])
    at = np.flatnonzero(head)
    return zz[at], kk[at], np.diff(np.append(at, zz.size))


def model(case):
    zd, kd, cd = _distinct_per_zone(case)
    counts = np.bincount(zd, weights=cd, minlength=case.nz).astype(np.int64)
    B = np.array([parts_log2(c) for c in counts], dtype=np.int64)
    n_parts_zone = 1 << B
    part_base = np.concatenate([[0], np.cumsum(n_parts_zone)])
    n_parts = int(part_base[-1])
    n_chunks = int(sum(-(-int(c) // CHUNK) for c, b in zip(counts, B) if b))
    gp = part_base[zd] + part_of(kd, B[zd])
    part_len = np.bincount(gp, weights=cd, minlength=n_parts).astype(np.int64)
    _, inv = np.unique(gp * SLOTS + sieve_slot(kd), return_inverse=True)
    cells_in_slot = np.bincount(inv, weights=cd)
    to_table = cells_in_slot[inv] != 1
    table_keys = np.bincount(gp[to_table], minlength=n_parts).astype(np.int64)
    return Model(counts, B, int(counts.sum()), n_parts, n_chunks, int((B > LDS_B).sum()), part_len, table_keys,
                 bool((table_keys > SLOTS).any()))


def _dt(dtype):
    return np.dtype(dtype)


def quarters(m, dtype, rng, lo=None):
    """`m` distinct multiples of 1/4 in random order, exact in float32 (|x| < 2^21)."""
    assert m < (1 << 23)
    lo = -(m // 2) if lo is None else lo
    return ((rng.permutation(m) + lo) * 0.25).astype(dtype)


def sized_zones(sizes, dtype, rng, name, shuffle=True, **expect):
    """Zone i of sizes[i] valid cells, every value of the raster distinct except that a zone of 3 cells or more holds one of
    its values three times: the winner.  Zones of 1 or 2 cells: the smallest value wins.  The cells are strewn over the
    raster (`shuffle`), with 2 % invalid cells (NaN, +-inf, zone -1, zone nz) among them."""
    sizes = np.asarray(sizes, dtype=np.int64)
    nz, n = sizes.size, int(sizes.sum())
    z = np.repeat(np.arange(nz, dtype=np.int32), sizes)
    v = quarters(n, dtype, rng)
    start = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    big = sizes >= 3
    v[start[big] + 1] = v[start[big]]
    v[start[big] + 2] = v[start[big]]
    winners = {}
    for zone in range(nz):
        s = int(sizes[zone])
        winners[zone] = np.nan if s == 0 else float(v[start[zone]] if s >= 3 else v[start[zone]:start[zone] + s].min())
    extra = max(4, n // 50)
    ze = np.concatenate([z, rng.integers(0, nz, extra).astype(np.int32)])
    ve = np.concatenate([v, np.resize(np.array([np.nan, np.inf, -np.inf, 1.0, 2.0], dtype=dtype), extra)])
    j = np.arange(extra)
    ze[n + j[j % 5 == 3]] = -1
    ze[n + j[j % 5 == 4]] = nz
    if shuffle:
        p = rng.permutation(ze.size)
        ze, ve = ze[p], ve[p]
    return Case(name, ze, ve, nz, winners=winners, expect=expect)


def uncut_case(dtype):
    """Zones of 1, 63, 1024 (one batch), 1025 and 1280 cells (two batches), and an empty one: six parts, no chunk."""
    return sized_zones([1, 63, 1024, 0, 1025, 1280], dtype, np.random.default_rng(11), "uncut zones",
                       B=[0] * 6, n_chunks=0, batches=2)


def boundary_case(dtype):
    return sized_zones([1281, 2048, 2049, 4096, 4097], dtype, np.random.default_rng(12), "B boundaries",
                       B=[1, 1, 2, 2, 3], n_chunks=5)


def chunks_case(dtype):
    """3 * 8192 + 5 cells: four chunks, the last of 5 keys; 8193 cells: two; uncut zones around them own none: six chunks
    in all, no multiple of the eight bands of xcd_tile."""
    return sized_zones([100, 3 * CHUNK + 5, 700, CHUNK + 1, 0, 3], dtype, np.random.default_rng(13), "many chunks",
                       B=[0, 5, 0, 4, 0, 0], n_chunks=6)


def b9_case(dtype):
    """262 145 cells: 512 parts (part_offsets_kernel's second trip of 256, reduce_kernel over eight parts per lane)."""
    return sized_zones([262_145, 5], dtype, np.random.default_rng(14), "B = 9", B=[9, 0], n_chunks=33)


def lds_b_case(dtype, direct):
    """2 097 152 valid cells: 2^11 parts, the last zone of the LDS-histogram kernels; one more: 2^12 parts, the DIRECT
    kernels.  Both rasters are larger than 2 097 152 cells, so both launch the DIRECT kernels."""
    big = (PART_TARGET << LDS_B) + int(direct)
    return sized_zones([7, big, 1300], dtype, np.random.default_rng(15 + direct), "DIRECT" if direct else "LDS_B",
                       B=[0, 12 if direct else 11, 1], n_direct=int(direct), n_chunks=258 if direct else 257)


def scan_carry_case(dtype, nz):
    """Sizes 1281 / 0 / 1 in turn: the scans of the counts, the parts and the chunks all carry into the second and third
    trip of plan_kernel's 1024 threads."""
    sizes = np.resize(np.array([1281, 0, 1]), nz)
    return sized_zones(sizes, dtype, np.random.default_rng(20 + nz % 7), f"plan scan nz={nz}",
                       B=np.resize(np.array([1, 0, 0]), nz).tolist(), n_chunks=int((sizes > 1280).sum()))


def lds_limit_case(dtype, nz=MAX_ZONES):
    """nz zones (MAX_ZONES: a 64 KiB histogram), two cells each on average, every 97th empty; few values: ties."""
    rng = np.random.default_rng(31)
    z = rng.integers(0, nz, 2 * nz).astype(np.int32)
    z[z % 97 == 0] += 1
    z[z >= nz] = -1
    v = (rng.integers(-6, 7, z.size) * 0.25).astype(dtype)
    v[rng.random(z.size) < 0.01] = np.nan
    return Case(f"nz={nz}", z, v, nz, winners={0: np.nan, 97: np.nan}, expect=dict(n_chunks=0))


def persistent_case(dtype):
    """4096 * 4096 + 4097 cells: zone_count_kernel's 4096 workgroups take a second tile, the first of them a third, partial
    one.  Three zones, seven values."""
    rng = np.random.default_rng(32)
    n = COUNT_GRID * TILE + TILE + 1
    levels = (np.array([-3, -1, 0, 2, 5, 9, 14]) * 0.25).astype(dtype)
    z = rng.integers(0, 3, n, dtype=np.int32)
    v = levels[rng.integers(0, 7, n, dtype=np.int8)]
    return Case("persistent count loop", z, v, 3, levels=levels, expect=dict(B=[13] * 3, n_direct=3))


def wave_case(dtype, n):
    """The three wave paths of zone_count_kernel / scatter_zone_kernel: 64-cell runs of one zone (one LDS add per wave); runs
    whose first three lanes are invalid (NaN, the nodata value, a zone outside the table: the leader is lane 3); zones
    interleaved cell by cell (an add per lane)."""
    nz = 5
    i = np.arange(n)
    z = np.where(i < n // 2 + 1, (i // 64) % nz, i % nz).astype(np.int32)
    rng = np.random.default_rng(40 + n % 11)
    v = (rng.integers(-8, 9, n) * 0.25).astype(dtype)
    odd = (i // 64) % 3 == 1
    v[odd & (i % 64 == 0)] = np.nan
    v[odd & (i % 64 == 1)] = 17.0
    z[odd & (i % 64 == 2)] = nz
    z[((i // 64) % 3 == 2) & (i % 64 == 5)] = -1
    return Case(f"wave paths n={n}", z, v, nz, nodata=17.0)


def dominated_case(dtype, late):
    """A zone of 100 000 cells (128 parts), 60 % of them one value: its part holds 60 000 equal keys (59 batches, most
    waves uniform: add = 64) among ~300 distinct ones.  `late`: the zone's first 1100 cells are distinct values of the
    dominant value's part, so the first batch of that part need not hold the winner."""
    rng = np.random.default_rng(50 + late)
    m, dom = 100_000, 60_000
    B = parts_log2(m)
    winner = np.dtype(dtype).type(1234.25)
    rest = quarters(m - dom + 1, dtype, rng, lo=8)                   # (0.25 * [8, 40 009): 1234.25 = 0.25 * 4937 is among them)
    rest = rest[rest != winner]
    head = np.empty(0, dtype)
    if late:
        part = int(part_of(enc(np.array([winner])), B)[0])
        head = keys_in_part(dtype, B, part, 1100, rng)
        head = head[(head != winner) & ~np.isin(head, rest)]
    body = np.concatenate([rest[:m - dom - head.size], np.full(dom, winner, dtype)])
    body = body[rng.permutation(body.size)]
    v = np.concatenate([head, body, quarters(700, dtype, rng, lo=-5000)])
    z = np.concatenate([np.zeros(head.size + body.size, np.int32), np.ones(700, np.int32)])
    return Case("dominated part" + (", winner late" if late else ""), z, v, 2, winners={0: float(winner)},
                expect=dict(B=[7, 0], late=int(head.size)))


def sieve_case(dtype, table_keys, B=2, part=1):
    """One part with exactly `table_keys` distinct keys that share their sieve slot with another key, one of them twice (the
    winner, not the smallest value); the other parts of the zone hold 200 keys each.  table_keys = SLOTS fills the table
    to the last slot; SLOTS + 1 must overflow."""
    rng = np.random.default_rng(60 + table_keys % 5 + width(dtype))
    pool = keys_in_part(dtype, B, part, 6000, rng)
    slot = sieve_slot(enc(pool))
    order = np.argsort(slot, kind="stable")
    pool, slot = pool[order], slot[order]
    uniq, first, cnt = np.unique(slot, return_index=True, return_counts=True)
    picked = []
    left = table_keys
    for f, c in zip(first, cnt):                                    # two keys of a slot at a time; three once when odd
        take = 3 if left % 2 and c >= 3 else 2
        if c >= take and left >= take:
            picked.extend(range(f, f + take))
            left -= take
    assert left == 0
    keys = pool[picked]
    winner = np.sort(keys)[keys.size // 2]
    others = np.concatenate([keys_in_part(dtype, B, q, 200, rng) for q in range(1 << B) if q != part])
    v = np.concatenate([keys, [winner], others])
    v = v[rng.permutation(v.size)]
    z = np.zeros(v.size, np.int32)
    return Case(f"sieve against table, {table_keys} keys", z, v, 1, winners={0: float(winner)},
                expect=dict(B=[B], table_keys=table_keys, overflow=table_keys > SLOTS, part=part))


def skewed_case(dtype):
    """6000 distinct values that all hash to part 0 of the 8 parts of their zone: far more than SLOTS of them share a sieve
    slot, so the part overflows and the sort must answer."""
    rng = np.random.default_rng(70)
    v = keys_in_part(dtype, 3, 0, 6000, rng)
    v = np.concatenate([v, v[:1], quarters(50, dtype, rng, lo=1)])
    z = np.concatenate([np.zeros(6001, np.int32), np.ones(50, np.int32)])
    return Case("6000 values in one part", z, v, 2, winners={0: float(v[0])}, expect=dict(B=[3, 0], overflow=True))


def ties_case(dtype):
    """Equal counts at every level: inside one thread's four keys, across waves, across batches, across the parts of a cut
    zone -- the smallest value wins; -0.0 and +0.0 are one value (and the answer is +0.0); +-inf and NaN are skipped; the
    nodata value does not win."""
    rng = np.random.default_rng(80)
    zones = [
        ([5.5, 2.5, 2.5, 5.5, 9.0], 2.5),
        ([3.0, -3.0, 3.0, -3.0], -3.0),
        ([-0.0, 1.0, 0.0, 1.0, -0.0, 7.0], 0.0),
        ([np.inf] * 5 + [-np.inf] * 5 + [np.nan] * 5 + [7.25], 7.25),
        ([4321.0] * 10 + [4.0, 5.0, 4.0], 4.0),
        (quarters(1024, dtype, rng), None),                          # one batch: every compare of the part is a tie
        (quarters(1280, dtype, rng), None),                          # two batches
        (quarters(5000, dtype, rng), None),                          # eight parts
        (quarters(3000, dtype, rng, lo=-100), None),                 # four parts, the smallest value negative
        ([-0.0] * 3, 0.0),
        ([np.nan, np.inf, 4321.0], np.nan),
    ]
    for _ in range(8):                                               # every value twice: every key goes to the table
        zones.append((np.repeat(quarters(512, dtype, rng), 2), None))
    for _ in range(4):                                               # the same in a cut zone
        zones.append((np.repeat(quarters(1500, dtype, rng), 2), None))
    z = np.concatenate([np.full(len(vals), i, np.int32) for i, (vals, _) in enumerate(zones)])
    v = np.concatenate([np.asarray(vals, dtype=dtype) for vals, _ in zones])
    winners = {i: (float(np.min(vals)) if w is None else w) for i, (vals, w) in enumerate(zones)}
    p = rng.permutation(z.size)
    return Case("ties", z[p], v[p], len(zones), nodata=4321.0, winners=winners)


def sort_case(dtype, nz):
    """The zone bits of the second sort at nz = 2^k - 1, 2^k, 2^k + 1 with the bucket of the invalid cells (key nz) in use."""
    rng = np.random.default_rng(90 + nz)
    n = 5003
    z = rng.integers(-1, nz + 1, n).astype(np.int32)
    z[:3] = [nz - 1, nz, -1]
    v = (rng.integers(-10, 11, n) * 0.25).astype(dtype)
    v[rng.random(n) < 0.05] = np.nan
    return Case(f"sort nz={nz}", z, v, nz)


def runs_case(dtype):
    """Runs of (zone, value): zones of 3 and 4 runs (the first thread's eight runs cross zone changes), a zone whose winner
    is its last run, a zone of 3000 runs (more than the 2048 of a workgroup), a zone whose last two runs tie."""
    rng = np.random.default_rng(99)
    zones = [
        ([1.0, 2.0, 2.0, 3.0], 2.0),
        ([1.0, 2.0, 3.0, 4.0, 4.0], 4.0),
        ([1.0, 1.0, 5.0, 9.0, 9.0, 9.0], 9.0),
        (np.concatenate([quarters(3000, dtype, rng), [700.0, 700.0]]), 700.0),
        ([6.0, 8.0, 8.0, 9.0, 9.0], 8.0),
    ]
    z = np.concatenate([np.full(len(vals), i, np.int32) for i, (vals, _) in enumerate(zones)])
    v = np.concatenate([np.asarray(vals, dtype=dtype) for vals, _ in zones])
    p = rng.permutation(z.size)
    return Case("run votes", z[p], v[p], len(zones), winners={i: w for i, (_, w) in enumerate(zones)})


WAVE_N = (1, 63, 65, 4095, 4097)
SCAN_NZ = (1, 1024, 1025, 2049)
SORT_NZ = (1, 3, 4, 5, 255, 256, 257)


SMALL_NAMES = ("uncut zones", "B boundaries", "many chunks", "B = 9", f"nz={MAX_ZONES}", "dominated part",
               "dominated part, winner late", f"sieve against table, {SLOTS} keys", "ties", "run votes") \
    + tuple(f"wave paths n={n}" for n in WAVE_N) + tuple(f"sort nz={nz}" for nz in SORT_NZ)


def small_cases(dtype):
    """Every case of at most a few hundred thousand cells, in the order of SMALL_NAMES."""
    out = [uncut_case(dtype), boundary_case(dtype), chunks_case(dtype), b9_case(dtype), lds_limit_case(dtype),
           dominated_case(dtype, 0), dominated_case(dtype, 1), sieve_case(dtype, SLOTS), ties_case(dtype), runs_case(dtype)]
    out += [wave_case(dtype, n) for n in WAVE_N]
    out += [sort_case(dtype, nz) for nz in SORT_NZ]
    return out


def overflow_cases(dtype):
    return [sieve_case(dtype, SLOTS + 1), skewed_case(dtype)]

"""Case table of the fused raster pass census (tests/test_raster_pass_host.py without a GPU, tests/test_gpu_raster_pass_census.py
on one): the rasters, the plan that places every nodata cell on them, a mirror of the strip geometry, the product-set dispatch
in the words of xrs_debug_pass_route, and models of the results that share nothing with the kernels.

The geometry mirror (`strip_classes`) and the dispatch (`expected_ops`) are csrc/strip.h's `strip_is_interior`, `load_strip` and
`strip_probe_rows` and csrc/pass.hip's `launch_pass_ops` TRANSCRIBED, not derived from anything: when those change, this table
has to be changed by hand, and the census says so by failing.

A wave strip is 256 columns x 4 rows (a workgroup: 4 strips = 16 rows), a lane owns 4 adjacent columns, and the strip loads
(4 + K - 1) x (256 + K - 1) cells.  The kernels take different paths through a strip depending on where it lies (interior: no
predicates; edge: cell-by-cell tests) and on which of its loaded rows hold a NaN or an inf (none: the clean copies; some: the
repair; and an output row none of whose K rows was hit skips the count inside a dirty strip), so every nodata cell of the census
rasters is placed by `PLAN`, none is scattered, and `strip_classes` says which strips the plan made of which class."""
import collections
import itertools

import numpy as np

from tests import synth

F32 = np.float32
RB = 4                      # rows of a wave strip (XRS_PASS_RB)
STRIP_COLS = 256
TILE_ROWS = 4 * RB          # rows of a workgroup

PRODUCTS = ('slope', 'aspect', 'curvature', 'hillshade')
LETTERS = dict(zip(PRODUCTS, 'SACH'))
SUBSETS = [tuple(p for p, take in zip(PRODUCTS, bits) if take) for bits in itertools.product((0, 1), repeat=4)]
RES = (30.0, 20.0)          # cell size (x, y) of every census call
LIGHT = (225.0, 25.0)       # azimuth, altitude


# ---------------------------------------------------------------------------------------------------------------- masks
def masks():
    """name -> (mask, compile-time?): both window sizes in the compile-time and the run-time form."""
    circle5 = np.array([[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]], float)
    cross3 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], float)
    ragged5 = np.array([[1, 0, 0, 1, 1], [0, 1, 0, 0, 0], [1, 1, 1, 0, 1], [0, 0, 0, 1, 0], [1, 0, 1, 1, 0]], float)
    return {'circle5': (circle5, True), 'box3': (np.ones((3, 3)), True), 'box5': (np.ones((5, 5)), False),
            'cross3': (cross3, False), 'ragged5': (ragged5, False)}


# ------------------------------------------------------------------------------------------------------------- dispatch
def ops_text(products):
    return ''.join(LETTERS[p] for p in PRODUCTS if p in products) or '-'


def expected_ops(products):
    """launch_pass_ops: the instantiation a requested product set runs in."""
    req = ops_text(products)
    if req in ('A', 'AH', '-', 'H', 'C', 'SH', 'CH', 'SC', 'SCH'):
        return req
    if req == 'S':
        return 'SH'            # (the hillshade skipped by a wave-uniform test)
    assert 'A' in req, req
    return 'SACH'


INSTANTIATIONS = ('A', 'AH', '-', 'H', 'SH', 'C', 'CH', 'SC', 'SCH', 'SACH')     # 11 cases of the switch, slope alone shares SH


def reachable_combinations():
    """(OPS, K, nt, cmask) the dispatch can produce: all but the focal mean alone under a run-time mask (a fall-back)."""
    return {(ops, K, nt, cm) for ops in INSTANTIATIONS for K in (3, 5) for nt in (0, 1) for cm in (0, 1)
            if not (ops == '-' and cm == 0)}


def expected_route(products, K, compile_time, nt, rows, cols, seg=(0, 0)):
    """The witness's text for a call the fused kernel takes whole (every census call but the focal mean alone under a run-time
    mask)."""
    tiles_y = (rows + TILE_ROWS - 1) // TILE_ROWS - seg[1]
    return (f"pass(ops={expected_ops(products)},K={K},nt={int(nt)},cmask={int(compile_time)},"
            f"tiles={(cols + STRIP_COLS - 1) // STRIP_COLS}x{tiles_y},seg={seg[0]}+{seg[1]})")


# -------------------------------------------------------------------------------------------------------------- rasters
# (row, column, value) of every cell of rasters A and B that is not plain terrain, and the class [a .. j] it is there for
NAN, INF = float('nan'), float('inf')
PLAN = (
    # tile column 256
    (11, 300, NAN),       # strip (12, 256): only its top halo row(s) hit [b]; strip (8, 256): a dirty strip whose row 0 is clean
    (24, 300, NAN),       # strip (20, 256): only its bottom halo row(s) hit [c]
    # (rows 34..40 x columns 380..386: the 7x7 hole, below) [i]
    # tile column 512
    *((y, 600, NAN) for y in range(10, 18)),          # strip (12, 512): every loaded row hit [f]
    (29, 620, INF), (30, 700, -INF),                  # strip (28, 512): +-inf and no NaN [g]
    (41, 650, 1e20),      # strip (40, 512): a finite cell whose gradient's square overflows; the row vote does not see it [h]
    (5, 768, NAN),        # strip (4, 512): hit only through lane 63's right halo columns [e]
    # tile column 768
    (21, 767, NAN),       # strip (20, 768): hit only through lane 0's left halo columns [d]
    (41, 900, 1e36),      # strip (40, 768): a finite cell the row vote reports (1e36 * 2000 overflows): nothing to repair [h]
    # edge strips [j]: top-left corner, top side, bottom side, bottom-right corner, left side, right side, the last lane
    (1, 100, NAN), (1, 600, NAN), (45, 400, NAN), (46, 1030, NAN), (22, 3, NAN), (26, 1035, NAN), (30, 1037, NAN),
)
HOLE = (slice(34, 41), slice(380, 387))


def _planned(shape, seed):
    z = synth.smooth_dem(shape, seed=seed)
    for y, x, v in PLAN:
        if y < shape[0] and x < shape[1]:
            z[y, x] = v
    z[HOLE] = np.nan
    z.setflags(write=False)
    return z


_cache = {}


def census_raster(name):
    """'A' 48 x 1040: three interior tile columns between an edge tile column on each side, interior and edge strip rows;
    'B' 48 x 1038: the last lane ragged with 2 cells of its own, rows that are not 16-byte multiples;
    '516' 24 x 516 / '515' its first 515 columns: the column boundary of strip_is_interior; '21': the first 21 rows of '516', the
    row boundary for K = 5;  'edges' 64 x 1040, clean;  'overflow', 'ulp': see overflow_raster, ulp_raster."""
    if name not in _cache:
        if name == 'A':
            z = _planned((48, 1040), 11)
        elif name == 'B':
            z = _planned((48, 1038), 12)
        elif name in ('516', '515', '21'):
            z = synth.smooth_dem((24, 516), seed=13)
            z[9, 300] = np.nan
            z = {'516': z, '515': z[:, :515], '21': z[:21]}[name].copy()
        elif name == 'edges':
            z = synth.smooth_dem((64, 1040), seed=14)
        elif name == 'overflow':
            z = overflow_raster()
        elif name == 'ulp':
            z = ulp_raster()
        else:
            raise KeyError(name)
        z.setflags(write=False)
        _cache[name] = z
    return _cache[name]


ULP_CELL = (10, 400)
ULP_TAPS = {(10, 398): 3000.00048828125, (10, 402): -9.1552734375e-05, (12, 400): -1.8189894035458565e-12}
ULP_SUM = float.fromhex('0x1.964000cffffffp+13')


def ulp_raster():
    """24 x 516, 1000.0 everywhere, a NaN at (9, 300) that makes strip (8, 256) a dirty one, and around ULP_CELL a window of the
    circular 5x5 mask whose 13 taps sum to ULP_SUM exactly (every tap a multiple of 2^-39, every partial sum below 2^14: exact in
    any order).  ULP_SUM * (1 / 13) lies one float64 ulp below the midpoint of two float32 values: with 1 / 13 one ulp larger the
    mean rounds the other way.  That window loses no tap and its rows are all reported, so its 1 / count comes from lane 0 of the
    wave's table, which must be the clean path's 1 / ntaps to the last bit -- a float32 result shows a float64 ulp nowhere else."""
    z = np.full((24, 516), 1000.0, F32)
    z[9, 300] = np.nan
    for cell, v in ULP_TAPS.items():
        z[cell] = v
        assert float(z[cell]) == v
    return z


OVERFLOW_CELLS = ((10, 300), (14, 401))       # the cells whose gradient is infinite: between the two cells of a pair


def overflow_raster():
    """24 x 520, 0.25 everywhere but two pairs of +-3e38, two rows apart in column 300 and two columns apart in row 14: every
    cell is finite, the row vote passes (the products of the chain stay below 7.5e37), and s - n / e - w overflow."""
    z = np.full((24, 520), 0.25, F32)
    z[9, 300], z[11, 300] = 3e38, -3e38
    z[14, 400], z[14, 402] = 3e38, -3e38
    return z


# ------------------------------------------------------------------------------------------------------ geometry mirror
Strip = collections.namedtuple('Strip', 'y0 x_tile interior hit probe nan inf big block')
Strip.__doc__ = """One wave strip as the kernel sees it.  hit: loaded rows (0 .. 4 + K - 2) holding a NaN or inf cell, the cells
load_strip fills with NaN outside the raster / the shard's halo rows included;  probe: the rows strip_probe_rows reports (its
float32 fma chain, lane by lane: `hit` plus the rows of finite cells whose products overflow);  nan / inf / big: (row, column)
inside `block` of the raster's own NaN, inf and |v| >= 1e19 cells;  block: the loaded cells, float32."""


def _fma32(a, b, c):
    with np.errstate(all='ignore'):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _probe_rows(block, K):
    """strip_probe_rows on the lanes of a loaded block (columns x_tile - RX ..): lane l holds block[:, 4 l : 4 l + NV]."""
    RX, NV = K // 2, 4 + 2 * (K // 2)
    lanes = (block.shape[1] - 2 * RX) // 4
    v = np.stack([block[:, i:i + 4 * lanes:4] for i in range(NV)])            # [i][row][lane]
    with np.errstate(all='ignore'):
        p = _fma32(v[0], v[1], v[2])
        i = 3
        while i + 2 < NV:
            p = (_fma32(v[i], v[i + 1], p) + v[i + 2]).astype(F32)
            i += 3
        if NV % 3 == 2:
            p = _fma32(v[NV - 2], v[NV - 1], p)
        if NV % 3 == 1:
            p = (p + v[NV - 1]).astype(F32)
    return frozenset(int(r) for r in np.nonzero(~np.isfinite(p).all(axis=1))[0])


def strip_classes(z, K, rows, cols, halo_top=0, halo_bot=0):
    """Every wave strip of a call on `rows` x `cols` cells; z holds them and the halo rows: z[halo_top + y] is row y."""
    z = np.asarray(z, F32)
    assert z.shape == (halo_top + rows + halo_bot, cols), (z.shape, rows, cols, halo_top, halo_bot)
    RX = RY = K // 2
    y_lo, y_hi = -halo_top, rows + halo_bot
    out = []
    for y0 in range(0, rows, RB):
        for x_tile in range(0, cols, STRIP_COLS):
            # strip_is_interior
            interior = (x_tile >= 4 and x_tile + STRIP_COLS + 4 <= cols and y0 - RY >= y_lo and y0 + RB + RY <= y_hi
                        and y0 + RB <= rows)
            # load_strip: the lanes whose first column is inside the raster, each NV cells wide; NaN outside the raster / halo
            lanes = min(64, (cols - x_tile + 3) // 4)
            ys = np.arange(y0 - RY, y0 + RB + RY)
            xs = np.arange(x_tile - RX, x_tile + 4 * lanes + RX)
            block = np.full((ys.size, xs.size), np.nan, F32)
            oky, okx = (ys >= y_lo) & (ys < y_hi), (xs >= 0) & (xs < cols)
            block[np.ix_(oky, okx)] = z[np.ix_(ys[oky] + halo_top, xs[okx])]
            own = np.full(block.shape, False)
            own[np.ix_(oky, okx)] = True
            cells = lambda m: tuple((int(r), int(c)) for r, c in zip(*np.nonzero(m & own)))      # noqa: E731
            with np.errstate(all='ignore'):
                big = np.isfinite(block) & (np.abs(block) >= 1e19)
            out.append(Strip(y0, x_tile, bool(interior), frozenset(int(r) for r in np.nonzero((~np.isfinite(block)).any(axis=1))[0]),
                             _probe_rows(block, K), cells(np.isnan(block)), cells(np.isinf(block)), cells(big), block))
    return out


def class_of(s, K):
    """The census classes (a .. i) an INTERIOR strip belongs to; j, the edge strips, are sorted by edge_sides."""
    assert s.interior
    RY = RX = K // 2
    NR, width = RB + K - 1, STRIP_COLS + 2 * RX
    got = set()
    bad = s.nan + s.inf
    if not bad and not s.big:
        got.add('a')
    if bad and not s.inf and not s.big:
        if all(r < RY for r, _ in bad):
            got.add('b')
        if all(r >= RB + RY for r, _ in bad):
            got.add('c')
        if all(c < RX for _, c in bad):
            got.add('d')
        if all(c >= width - RX for _, c in bad):
            got.add('e')
    if len(s.hit) == NR:
        got.add('f')
    if s.inf and not s.nan:
        got.add('g')
    if s.big and not bad:
        got.add('h')
    nanb = np.isnan(s.block)
    if any(nanb[r:r + min(7, NR), c:c + 7].all() for r in range(NR - min(7, NR) + 1) for c in range(width - 6)):
        got.add('i')                    # (as much of the 7x7 hole as a strip of this height can hold, across all 7 columns)
    return got


def has_clean_row_in_dirty_strip(s, K):
    """An output row none of whose K loaded rows is reported, in a strip that reports some: the `hit == 0u` shortcut."""
    return bool(s.probe) and any(not (s.probe & set(range(r, r + K))) for r in range(RB))


def edge_sides(s, K, rows, cols, halo_top=0, halo_bot=0):
    """Which of strip_is_interior's conditions an edge strip fails: the sides of the raster it touches."""
    assert not s.interior
    RY = K // 2
    sides = set()
    if s.y0 - RY < -halo_top:
        sides.add('top')
    if s.y0 + RB + RY > rows + halo_bot or s.y0 + RB > rows:
        sides.add('bottom')
    if s.x_tile < 4:
        sides.add('left')
    if s.x_tile + STRIP_COLS + 4 > cols:
        sides.add('right')
    return sides


# --------------------------------------------------------------------------------------------------------------- models
Mean = collections.namedtuple('Mean', 'sum count ntaps maxabs sumabs')


def mean_model(z, mask):
    """The window sums of the focal mean, exactly: per cell the float64 sum of the window's non-NaN taps (cells outside the
    raster are NaN) -- exact for terrain-sized float32 values, whatever the order -- their count, the largest finite |tap| and the
    sum of the finite |taps|."""
    z = np.asarray(z, F32)
    mask = np.asarray(mask)
    ry, rx = mask.shape[0] // 2, mask.shape[1] // 2
    pad = np.full((z.shape[0] + 2 * ry, z.shape[1] + 2 * rx), np.nan, np.float64)
    pad[ry:ry + z.shape[0], rx:rx + z.shape[1]] = z
    total = np.zeros(z.shape, np.float64)
    count = np.zeros(z.shape, np.int64)
    maxabs = np.zeros(z.shape, np.float64)
    sumabs = np.zeros(z.shape, np.float64)
    with np.errstate(all='ignore'):
        for ky, kx in zip(*np.nonzero(mask == 1)):
            tap = pad[ky:ky + z.shape[0], kx:kx + z.shape[1]]
            ok = ~np.isnan(tap)
            total += np.where(ok, tap, 0.0)
            count += ok
            mag = np.where(np.isfinite(tap), np.abs(tap), 0.0)
            maxabs = np.maximum(maxabs, mag)
            sumabs += mag
    return Mean(total, count, int(np.count_nonzero(mask == 1)), maxabs, sumabs)


EXACT_BELOW = 4096.0          # |taps| below this (and 25 of them): the float64 sum has bits to spare, any order gives the same


def check_mean(got, m, what, rows=slice(None), exact_huge=False):
    """strip.h's promises for the focal mean, against mean_model:
    - a window that lost no tap is float32(sum * (1 / ntaps)) bit for bit, whatever else its strip holds (the sum is exact, the
      multiplication and the rounding are IEEE);
    - a window that lost taps is within 1 float32 ulp of float32(sum / count) (rcp_count: v_rcp_f64 and a Newton step, 1e-16);
    - NaN exactly where no tap is left; inf / NaN as the sum itself where the window holds +-inf;
    - windows holding a finite cell of 4096 and beyond (the census has 1e20, 1e36, 3e38): the float64 sum depends on the order,
      by at most n 2^-53 sum|v|.  Where that is nothing next to the sum they are held to the project's 1e-6 -- or, exact_huge (a
      background so small that every order gives the same float64), bit for bit as above; where the window's cells cancel
      (+3e38 and -3e38), to twice that bound, the model's own error and the kernel's.
    Returns the number of windows of each kind."""
    got = np.asarray(got)
    total, count, maxabs, sumabs = m.sum[rows], m.count[rows], m.maxabs[rows], m.sumabs[rows]
    assert got.shape == total.shape and got.dtype == F32, what
    with np.errstate(all='ignore'):
        full = (total * (1.0 / m.ntaps)).astype(F32)                      # the clean path's own two roundings
        part = (total / np.maximum(count, 1)).astype(F32)
        bound = m.ntaps * 2.0 ** -53 * sumabs / np.maximum(count, 1)
    empty = count == 0
    assert np.isnan(got[empty]).all(), f"{what}: windows without a tap are NaN"
    special = ~np.isfinite(total) & ~empty                                # windows holding +-inf: inf, or NaN for inf - inf
    np.testing.assert_array_equal(got[special], total[special].astype(F32), err_msg=f"{what}: windows holding inf")
    huge = ~empty & ~special & (maxabs >= EXACT_BELOW)
    cancel = huge & (bound >= 1e-6 * np.abs(part.astype(np.float64)))
    exact = ~empty & ~special & (~huge | (exact_huge & ~cancel))
    whole = exact & (count == m.ntaps)
    np.testing.assert_array_equal(got[whole], full[whole], err_msg=f"{what}: windows that lost no tap are float32(sum * (1 / ntaps))")
    lost = exact & (count < m.ntaps)
    ulp = np.spacing(np.abs(part[lost]))
    off = np.abs(got[lost].astype(np.float64) - part[lost].astype(np.float64))
    assert np.isfinite(got[lost]).all() and (off <= ulp).all(), \
        f"{what}: windows that lost taps: {float((off / ulp).max()) if off.size else 0} ulp from float32(sum / count)"
    loose = huge & ~cancel & ~exact
    np.testing.assert_allclose(got[loose], part[loose], rtol=1e-6, atol=0, err_msg=f"{what}: windows holding a huge finite cell")
    off = np.abs(got[cancel].astype(np.float64) - total[cancel] / count[cancel])
    assert np.isfinite(got[cancel]).all() and (off <= 2 * bound[cancel] + np.spacing(np.abs(part[cancel]))).all(), \
        f"{what}: windows whose huge cells cancel"
    return {'whole': int(whole.sum()), 'lost': int(lost.sum()), 'empty': int(empty.sum()), 'inf': int(special.sum()),
            'huge': int(loose.sum()), 'cancel': int(cancel.sum())}

"""The census of the focal / convolve_2d window kernels: one case per mask, as plain data plus small helpers -- TEST
INFRASTRUCTURE shared by tests/test_gpu_window_census.py (runs every case on the GPU) and tests/test_window_census_host.py
(checks, without a GPU, that the table covers every walker unit and every dispatch branch).

A case is a mask and the calls made with it; a call is a statistic set (or the uniform-weight convolution), the accuracy
flags, the workspace mode, and THE ROUTE THE DISPATCH TABLE PROMISES for it (csrc/kxk.hip, the comment above
xrs_focal_stats_f32_ex) in the words of xrs_debug_window_route: `expected_route` is that table transcribed, not derived from
the library, so a call that quietly lands on another kernel fails its census test even when its numbers are right."""
import re
from collections import namedtuple

import numpy as np

from tests import synth
from xrspatial_amd.convolution import annulus_kernel, circle_kernel

STATS = ('mean', 'max', 'min', 'range', 'std', 'var', 'sum')            # XRS_STAT_* order
EXACT, SEQ = 1, 2                                                      # XRS_FOCAL_EXACT_MOMENTS, XRS_FOCAL_SEQUENTIAL_SUM
FLAG_SETS = (0, EXACT, SEQ, EXACT | SEQ)
# the compile-time plane sets: moments ALL / MVS / run-time, extrema 3 / fewer, wide MEAN / SUM
STAT_SETS = (STATS, ('mean',), ('sum',), ('mean', 'var', 'std'), ('max', 'min', 'range'), ('min',))
FLAGGED_ANNULI = ((4, 1), (9, 4), (12, 11))
ANNULI = tuple((R, RI) for R in range(4, 13) for RI in range(1, R))

Call = namedtuple('Call', 'what stats flags workspace route')          # what: 'focal' | 'conv'; workspace: 'api' | 'none'
Case = namedtuple('Case', 'id kind R RI shape calls')


# ---------------------------------------------------------------- masks
def circle_hw(R, dy):
    """CircleShape::hw (csrc/window_call.h): the largest dx with dx^2 + dy^2 <= R^2."""
    h = 0
    while (h + 1) * (h + 1) + dy * dy <= R * R:
        h += 1
    return h


def annulus_hole_hw(RI, dy):
    """annulus_hole_hw (csrc/window_call.h): half-width of the hole in the row at offset dy; -1 = no hole in this row."""
    return circle_hw(RI, dy) if dy <= RI else -1


def shape_mask(kind, R, RI=-1):
    """The mask of a shape from the walkers' row formulas: a row at offset dy is the centred run of half-width hw without the
    centred run of half-width hwi."""
    K = 2 * R + 1
    m = np.zeros((K, K))
    for ky in range(K):
        dy = abs(ky - R)
        hw = R if kind == 'box' else circle_hw(R, dy)
        hwi = annulus_hole_hw(RI, dy) if kind == 'annulus' else -1
        for kx in range(K):
            dx = abs(kx - R)
            m[ky, kx] = 1.0 if hwi < dx <= hw else 0.0
    return m


def ragged_mask(R):
    """'other': a fixed ragged 0/1 mask -- no circle, box or annulus, and too many short runs for the prefix-sum run kernels."""
    K = 2 * R + 1
    m = (np.add.outer(np.arange(K) * 3, np.arange(K) * 5) % 7 < 3).astype(float)
    m[R, R] = 1.0
    m[0, 0] = 0.0
    return m


def build_mask(case):
    if case.kind == 'circle':
        return circle_kernel(1, 1, case.R)
    if case.kind == 'box':
        return np.ones((2 * case.R + 1, 2 * case.R + 1))
    if case.kind == 'annulus':
        return annulus_kernel(1, 1, case.R, case.RI)
    return ragged_mask(case.R)


def suits_run_kernels(mask):
    """parse_runs (csrc/kxk_runs.hip): the prefix-sum run kernels take a mask of at most 61 x 61 whose rows are at most 128 runs
    of ones in all, six cells and more to a run on average; any other passes on to the tap walk."""
    runs = sum(int(np.count_nonzero(np.diff(np.concatenate(([0.0], row == 1.0, [0.0])).astype(int)) == 1)) for row in mask)
    return max(mask.shape) <= 61 and 0 < runs <= 128 and runs * 6 <= int(np.count_nonzero(mask == 1.0))


# ---------------------------------------------------------------- the dispatch table, transcribed
def _name(family, kind, R, RI):
    if kind == 'annulus':
        unit = {'wide': f'wide_annulus{R}', 'mom': f'focal_mom_annulus{R}',
                'ext': 'focal_ext_annulus_' + ('a' if R <= 9 else 'b' if R <= 11 else 'c')}[family]
        return f'{unit}({R},{RI})'
    unit = {'wide': f'focal_wide_{kind}', 'conv': f'conv_wide_{kind}', 'mom': f'focal_mom_{kind}', 'ext': f'focal_ext_{kind}',
            'f32': f'focal_{kind}_f32', 'f64': f'focal_{kind}_f64', 'sw': f'focal_sw_{kind}'}[family]
    return f'{unit}({R})'


def expected_route(kind, R, RI, stats, flags=0, workspace='api'):
    """The launch groups of xrs_focal_stats_f32_ex for this call, in order, without their tiling."""
    S = set(stats)
    exact, seq = bool(flags & EXACT), bool(flags & SEQ)
    K = 2 * R + 1
    moments, extrema, has_sum = S & {'mean', 'var', 'std'}, S & {'max', 'min', 'range'}, 'sum' in S
    shaped = kind in ('circle', 'box', 'annulus')
    runs = suits_run_kernels(shape_mask(kind, R, RI) if shaped else ragged_mask(R))
    if K > 63:
        return [f'big({R})']
    if not exact and S <= {'mean', 'sum'} and not (has_sum and seq):
        if kind in ('circle', 'box') and 3 <= R <= 12:
            return [_name('wide', kind, R, RI)]
        if kind == 'annulus' and 4 <= R <= 12:
            return [_name('wide' if S == {'mean'} else 'mom', kind, R, RI)]
    if not exact and S - {'mean', 'sum'} and shaped and 4 <= R <= 12:
        route = [_name('ext', kind, R, RI)] if extrema else []
        if moments or (has_sum and not seq):
            if kind == 'box' and workspace == 'api' and S & {'var', 'std'}:
                route.append(f'boxsep({R})')
            route.append(_name('mom', kind, R, RI))
        if has_sum and seq:
            route.append(f'tap3({R})' if kind == 'annulus' else _name('f32', kind, R, RI))
        return route
    if S == {'mean'} and K * K >= 49 and kind in ('circle', 'box') and R <= 12:
        return [_name('f64', kind, R, RI)]
    if S == {'mean'} and K * K > 49 and runs:
        return [f'focal_mean_runs({R})']
    column_walkers = kind in ('circle', 'box') and R <= 12
    if S != {'mean'} and K * K > 49 and (not moments or column_walkers or runs):
        route = []
        if moments:
            route.append(_name('f64', kind, R, RI) if column_walkers else f'focal_meanvar_runs({R})')
        if S - moments:
            if kind in ('circle', 'box') and R <= 12:
                route.append(_name('f32', kind, R, RI))
            else:
                route.append(f'tap3({R})' if not extrema else f'tap4({R})' if not has_sum else f'tap2({R})')
        return route
    if S == {'mean'}:
        if (kind, R) in (('circle', 2), ('box', 1)):
            return [f'pass({R})']
        return [f'strips3({R})' if K == 3 else f'strips5({R})' if K == 5 else f'lds_mean7({R})' if K == 7 else f'tap0({R})']
    if kind in ('circle', 'box') and R in (2, 3):
        if not exact and not (seq and has_sum) and moments:
            return [_name('sw', kind, R, RI)]
        return [_name('f32' if S - moments else 'f64', kind, R, RI)]
    return [f'strips3({R})' if K == 3 else f'strips5({R})' if K == 5 else f'tap1({R})']


def expected_conv_route(kind, R, RI):
    """xrs_convolve2d_f32 with the mask normalised to one weight."""
    if (kind in ('circle', 'box') and 3 <= R <= 12) or (kind == 'annulus' and 4 <= R <= 12):
        return [_name('wide' if kind == 'annulus' else 'conv', kind, R, RI)]
    K = 2 * R + 1
    return [f'big({R})' if K > 63 else f'conv_strips3({R})' if K == 3 else f'conv_strips5({R})' if K == 5 else f'conv_tap({R})']


# ---------------------------------------------------------------- the table
def _calls(kind, R, RI, flag_sets, conv):
    calls = []
    for flags in flag_sets:
        for stats in STAT_SETS:
            calls.append(Call('focal', stats, flags, 'api', expected_route(kind, R, RI, stats, flags, 'api')))
    # no workspace, through the raw ABI on a row shard with halo rows: slow tiles walked in place, no boxsep
    for stats in (STATS, ('mean',)):
        calls.append(Call('focal', stats, 0, 'none', expected_route(kind, R, RI, stats, 0, 'none')))
    if conv:
        calls.append(Call('conv', (), 0, 'api', expected_conv_route(kind, R, RI)))
    return tuple(calls)


def _shape(kind, R):
    # 420 x 1108: three tile rows of 128 .. 137 rows and three workgroups of 512 columns, the last of each partial; 1108 is no
    # multiple of any wave tile's width either (64, 128, boxsep's 128 - 2R).  The strip walker of radius 2 has workgroups of 1024
    # columns, so its masks get a wider raster.
    return (420, 2200) if R <= 2 and kind in ('circle', 'box') else (420, 1108)


# the row shard of the calls without a workspace: rows [13, 402) of the raster -- a prime number of rows, so the last tile row
# is partial whatever the tile height -- with a halo of the window's radius (<= 12) above and below
SHARD_FIRST, SHARD_ROWS = 13, 389


def _build():
    cases = []
    for R, RI in ANNULI:
        flag_sets = FLAG_SETS if (R, RI) in FLAGGED_ANNULI else (0,)
        cases.append(Case(f'annulus-{R}-{RI}', 'annulus', R, RI, _shape('annulus', R), _calls('annulus', R, RI, flag_sets, True)))
    for kind in ('circle', 'box'):
        for R in range(2, 13):
            cases.append(Case(f'{kind}-{R}', kind, R, -1, _shape(kind, R), _calls(kind, R, -1, FLAG_SETS, R >= 3)))
    # the dispatch branches no circle, box or annulus of radius 2..12 reaches: 3x3, ragged masks, a window beyond 63x63
    cases.append(Case('box-1', 'box', 1, -1, (420, 1108), _calls('box', 1, -1, (0,), True)))
    for R in (2, 3, 4):
        cases.append(Case(f'other-{R}', 'other', R, -1, (420, 1108), _calls('other', R, -1, (0,), True)))
    cases.append(Case('box-32', 'box', 32, -1, (90, 300), (                   # (a small raster: 4 225 taps per cell in the oracle)
        Call('focal', STATS, 0, 'api', expected_route('box', 32, -1, STATS)),
        Call('conv', (), 0, 'api', expected_conv_route('box', 32, -1)))))
    return tuple(cases)


CASES = _build()


def all_route_names():
    """Every unit / branch name some case expects, without radii."""
    return {item.split('(')[0] for case in CASES for call in case.calls for item in call.route}


# ---------------------------------------------------------------- the raster and its decorations
LAKE_VALUE = np.float32(1234.5)
# (name, first row, rows, first column, columns); rows 137 .. 256 lie in the second tile row of every walker (tiles of 128 ..
# 137 rows), columns 128 .. 1024 in interior wave tiles
DECORATIONS = (
    ('nan_block', 112, 41, 495, 36),        # larger than a 25 x 25 window, across the tile corner near (128 .. 137, 512)
    ('nan_cell', 200, 1, 350, 1),           # deep inside an interior tile
    ('nan_in_holes', 215, 1, 180, 1),       # an isolated cell: the windows centred around it see it only through their hole
    ('pos_inf', 190, 1, 700, 1),
    ('neg_inf', 225, 1, 960, 1),
    ('lake', 340, 64, 600, 64),             # flat, larger than the window
)


def census_raster(shape):
    z = synth.asv_dem(*shape).copy()
    for name, y, h, x, w in DECORATIONS:
        z[y:y + h, x:x + w] = {'pos_inf': np.inf, 'neg_inf': -np.inf, 'lake': LAKE_VALUE}.get(name, np.nan)
    return z


def lake_interior(R):
    _, y, h, x, w = DECORATIONS[-1]
    return slice(y + R + 1, y + h - R - 1), slice(x + R + 1, x + w - R - 1)


# ---------------------------------------------------------------- the witnessed geometry
_ITEM = re.compile(r'^(\w+)(?:\((\d+)(?:,(\d+))?\))?(?:\[wave=(\d+),wg=(\d+),rows=(\d+),grid=(\d+)x(\d+)\])?$')
Item = namedtuple('Item', 'name R RI wave wg tile_rows wgs_x wgs_y')


def parse_route(text):
    items = []
    for part in filter(None, text.split(';')):
        m = _ITEM.match(part)
        assert m, f"unreadable route item {part!r} in {text!r}"
        g = m.groups()
        items.append(Item(g[0], *(int(v) if v is not None else None for v in g[1:])))
    return items


def route_names(text):
    """The route without the tiling: what `expected_route` gives."""
    return [re.sub(r'\[.*?\]', '', part) for part in filter(None, text.split(';'))]


def clean_interior_wave_tiles(item, rows, cols, R, first_row=0, halo_top=0, halo_bot=0):
    """Wave tiles of this launch whose every window lies inside the raster (rows: inside the shard and its halo rows), that are
    whole, and that no window of theirs sees a decoration.  `first_row`: the raster row of the shard's row 0."""
    found = []
    n_ty = -(-rows // item.tile_rows)
    for ty in range(n_ty):
        y0, y1 = ty * item.tile_rows, (ty + 1) * item.tile_rows
        if y0 - R < -halo_top or y1 + R > rows + halo_bot or y1 > rows:
            continue
        for tx in range(-(-cols // item.wave)):
            x0, x1 = tx * item.wave, (tx + 1) * item.wave
            if x0 - R < 0 or x1 + R > cols:
                continue
            hit = False
            for _, dy, dh, dx, dw in DECORATIONS:
                dy -= first_row
                hit |= dy < y1 + R and dy + dh > y0 - R and dx < x1 + R and dx + dw > x0 - R
            if not hit:
                found.append((ty, tx))
    return found


def geometry_faults(item, rows, cols, R, **shard):
    """What the raster lacks for this launch: [] when it has three workgroups across, three tile rows down (so the RimFirst
    interior band is walked), a partial last tile both ways and a clean, whole, interior wave tile."""
    faults = []
    if item.wgs_x < 3:
        faults.append(f"{item.wgs_x} workgroups across (< 3)")
    if item.wgs_y < 3:
        faults.append(f"{item.wgs_y} tile rows (< 3)")
    if item.wgs_x != -(-cols // item.wg) or item.wgs_y != -(-rows // item.tile_rows):
        faults.append(f"grid {item.wgs_x}x{item.wgs_y} does not tile {rows}x{cols} by {item.tile_rows}x{item.wg}")
    if rows % item.tile_rows == 0:
        faults.append("no partial last tile row")
    if cols % item.wave == 0:
        faults.append("no partial last wave tile")
    if not clean_interior_wave_tiles(item, rows, cols, R, **shard):
        faults.append("no interior wave tile free of decorations")
    return faults

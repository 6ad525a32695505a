"""The D-infinity rule of xrspatial_amd/hydrology.py in NumPy and plain Python floats.  There is no reference to
execute: the rule is written, and tests/test_dinf_host.py pins this statement of it to literals worked out by hand.

  table              b[0 .. 8]: the neighbours' angles and 2 pi
  flow_direction     cell by cell: D8's winner, then the eight facets
  edges              a direction raster (codes or angles) -> every cell's receivers and shares
  flow_accumulation  Kahn's order, every cell gathered once in the fixed order of positions
  tile_model         the relaxer's schedule (tiles, colours, rounds, CAP, the column sweeps) on the same gather, for any tile
                     order: what it must equal bit for bit
"""
import math

import numpy as np

from tests import hydrology_oracle as ho

OFFSETS = ((0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))      # neighbour n = 0 .. 7: E, NE, N, NW, W, SW, S, SE
CODES = (1, 128, 64, 32, 16, 8, 4, 2)                                                  # its D8 code
D8_ORDER = (0, 7, 6, 5, 4, 3, 2, 1)                                                    # D8's order E, SE, S, .. as n
GATHER = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))        # where the donors of a cell sit, in the order they are added


def table(cx=1.0, cy=1.0):
    cx, cy = np.abs(np.float64(cx)), np.abs(np.float64(cy))
    td, pi = np.arctan2(cy, cx), np.float64(np.pi)
    b = np.array([0.0, td, pi / 2, pi - td, pi, pi + td, 3 * pi / 2, 2 * pi - td, 2 * pi], np.float64)
    if not (np.isfinite(b).all() and (np.diff(b) > 0).all()):
        raise ValueError("the table of angles is not strictly increasing")
    return b


def codes_to_angles(codes, cx=1.0, cy=1.0):
    """A raster of D8 codes as table angles: code 0 -> -1.0, NaN -> NaN."""
    b = table(cx, cy)
    d = np.asarray(codes, np.float64)
    out = np.where(np.isnan(d), np.nan, -1.0)
    for n, c in enumerate(CODES):
        out[d == c] = b[n]
    return out


def flow_direction(data, cx=1.0, cy=1.0, codes=None):
    """The angles of `data`; `codes`: the resolved D8 codes (flow_direction(resolve_flats=True)) for the cells without a winner."""
    z = np.asarray(data).astype(np.float64)
    cx, cy, dg = (float(v) for v in ho.cell_distances(cx, cy))
    b = [float(v) for v in table(cx, cy)]
    rows, cols = z.shape
    pad = np.full((rows + 2, cols + 2), np.nan)
    pad[1:-1, 1:-1] = z
    P = pad.tolist()
    out = np.full(z.shape, np.nan, np.float64)
    for i in range(rows):
        for j in range(cols):
            zc = P[i + 1][j + 1]
            if zc != zc:
                continue
            zn = [P[i + 1 + dr][j + 1 + dc] for dr, dc in OFFSETS]
            best, win = 0.0, -1
            for n in D8_ORDER:
                drop = (zc - zn[n]) / (dg if n & 1 else (cy if n & 2 else cx))
                if drop > best:
                    best, win = drop, n
            if win < 0:
                angle = -1.0
                if codes is not None and codes[i, j] in CODES:
                    angle = b[CODES.index(int(codes[i, j]))]
            else:
                bestq, angle = best * best, b[win]
                for o in range(8):
                    card, diag = ((o + 1) & 7, o) if o & 1 else (o, o + 1)
                    d1, d2 = (cy, cx) if card & 2 else (cx, cy)
                    s1, s2 = (zc - zn[card]) / d1, (zn[card] - zn[diag]) / d2
                    if s1 > 0 and s2 > 0 and s2 * d1 < s1 * d2:
                        q = s1 * s1 + s2 * s2
                        if q > bestq:
                            bestq = q
                            r = math.atan2(s2, s1)
                            angle = b[o + 1] - r if o & 1 else b[o] + r
                            angle = min(max(angle, b[o]), b[o + 1])
                            if angle == b[8]:
                                angle = 0.0
            out[i, j] = angle
    return out


def edges(flow_dir, method='dinf', cx=1.0, cy=1.0):
    """(valid, out): valid the non-NaN mask (flat); out[u] = [(n, v, share)] for the receivers of u that lie in the raster at a
    non-NaN cell.  ValueError for a value that is no direction."""
    d = np.asarray(flow_dir)
    d = d.astype(np.float32) if method == 'd8' else d.astype(np.float64)
    rows, cols = d.shape
    valid = ~np.isnan(d)
    b = [float(v) for v in table(cx, cy)] if method == 'dinf' else None
    out = [[] for _ in range(rows * cols)]
    for i in range(rows):
        for j in range(cols):
            if not valid[i, j]:
                continue
            a = float(d[i, j])
            if method == 'd8':
                if a not in (0,) + CODES:
                    raise ValueError("flow direction raster holds a value that is not a D8 code")
                parts = [(CODES.index(int(a)), 1.0)] if a else []
            elif a == -1.0:
                parts = []
            elif not (0.0 <= a < b[8]):
                raise ValueError("flow direction raster holds a value that is no angle")
            else:
                o = max(k for k in range(8) if a >= b[k])
                width = b[o + 1] - b[o]
                parts = [(o, (b[o + 1] - a) / width), ((o + 1) & 7, (a - b[o]) / width)]
            for n, share in parts:
                r, q = i + OFFSETS[n][0], j + OFFSETS[n][1]
                if share > 0 and 0 <= r < rows and 0 <= q < cols and valid[r, q]:
                    out[i * cols + j].append((n, r * cols + q, share))
    return valid.ravel(), out


def _donors(shape, out):
    """donors[v] = [(u, share)] in the gather order."""
    rows, cols = shape
    into = [dict() for _ in range(rows * cols)]
    for u, parts in enumerate(out):
        for n, v, share in parts:
            into[v][(-OFFSETS[n][0], -OFFSETS[n][1])] = (u, share)      # where u sits, seen from v
    return [[at[pos] for pos in GATHER if pos in at] for at in into]


def _own(shape, valid, weights):
    w = np.ones(shape, np.float64) if weights is None else np.asarray(weights).astype(np.float64)
    return [float(v) for v in w.ravel()]


def _gather(v, w, acc, donors):
    total = w[v]
    for u, share in donors[v]:
        total = total + share * acc[u]
    return total


def flow_accumulation(flow_dir, method='dinf', cx=1.0, cy=1.0, weights=None):
    shape = np.asarray(flow_dir).shape
    valid, out = edges(flow_dir, method, cx, cy)
    donors = _donors(shape, out)
    w = _own(shape, valid, weights)
    acc = [math.nan] * valid.size
    waiting = [len(d) for d in donors]
    ready = [int(v) for v in np.flatnonzero(valid) if waiting[v] == 0]
    seen = 0
    while ready:                                                         # Kahn: a cell is computed once all its donors are
        v = ready.pop()
        acc[v] = _gather(v, w, acc, donors)
        seen += 1
        for _, r, _ in out[v]:
            waiting[r] -= 1
            if waiting[r] == 0:
                ready.append(r)
    left = int(valid.sum()) - seen
    if left:
        raise ValueError(f"flow direction raster contains a cycle: {left} cells lie on or below one")
    return np.array(acc, np.float64).reshape(shape)


def tile_model(flow_dir, method='dinf', cx=1.0, cy=1.0, weights=None, tile=4, cap=3, rng=None):
    """The relaxer's schedule: (accumulation, rounds, reached_cap).  Tiles of `tile` cells square in 2 x 2 colours; a round runs
    the listed tiles colour by colour, the tiles of a colour in `rng`'s order; a tile iterates at most `cap` times, every column
    swept down and up against the state its iteration began with (its own column excepted); a tile in which a cell became final
    lists its eight neighbours, and itself when it stopped at `cap`.  ValueError when a round makes nothing final and cells are left."""
    rng = rng or np.random.default_rng(0)
    rows, cols = shape = np.asarray(flow_dir).shape
    valid, out = edges(flow_dir, method, cx, cy)
    donors = _donors(shape, out)
    w = _own(shape, valid, weights)
    acc = [math.nan] * valid.size
    final = [False] * valid.size
    ty, tx = -(-rows // tile), -(-cols // tile)
    listed = set(range(ty * tx))
    rounds, capped = 0, False
    while True:
        flagged, made = set(), 0
        for colour in range(4):
            mine = [t for t in sorted(listed) if ((t // tx) & 1) * 2 + ((t % tx) & 1) == colour]
            for t in rng.permutation(len(mine)):
                ti, tj = divmod(mine[t], tx)
                fell = it = 0
                pending = False
                while True:
                    before = list(final)
                    now = 0
                    for j in range(tj * tile, min(cols, (tj + 1) * tile)):
                        column = list(range(ti * tile, min(rows, (ti + 1) * tile)))
                        for i in column + column[-2::-1]:
                            v = i * cols + j
                            if not valid[v] or final[v]:
                                continue
                            if all((final if u % cols == j else before)[u] for u, _ in donors[v]):
                                acc[v] = _gather(v, w, acc, donors)
                                final[v] = True
                                now += 1
                    fell += now
                    if not now:
                        break
                    it += 1
                    if it == cap:
                        pending = capped = True
                        break
                made += fell
                if fell:
                    for di in (-1, 0, 1):
                        for dj in (-1, 0, 1):
                            if (di or dj or pending) and 0 <= ti + di < ty and 0 <= tj + dj < tx:
                                flagged.add((ti + di) * tx + tj + dj)
        rounds += 1
        if not made:
            break
        listed = flagged
    left = sum(1 for v in range(valid.size) if valid[v] and not final[v])
    if left:
        raise ValueError(f"flow direction raster contains a cycle: {left} cells lie on or below one")
    return np.array(acc, np.float64).reshape(shape), rounds, capped


# ------------------------------------------------------------------ rasters the tests share
def plane(rows, cols, azimuth_deg, dtype=np.float64):
    """A tilted plane whose downhill direction is `azimuth_deg` counter-clockwise from east."""
    i, j = np.mgrid[0:rows, 0:cols]
    t = math.radians(azimuth_deg)
    return (1000.0 - (j * math.cos(t) - i * math.sin(t)) * 3.0).astype(dtype)


def cone(rows, cols, dtype=np.float64):
    i, j = np.mgrid[0:rows, 0:cols]
    return (500.0 - np.sqrt((i - rows / 2.3) ** 2.0 + (j - cols / 1.7) ** 2.0)).astype(dtype)


def random_dag(rows, cols, seed, res=(1.0, 1.0)):
    """Angles of a random surface with NaN cells and exact ties: every kind of cell, and no cycle."""
    rng = np.random.default_rng(seed)
    z = rng.integers(0, 12, (rows, cols)).astype(np.float64) + rng.random((rows, cols)) * (seed % 3)
    z[rng.random((rows, cols)) < 0.06] = np.nan
    return flow_direction(z, *res)


def ulps(got, want):
    """|got - want| in units of the spacing of `want`."""
    return np.abs(got - want) / np.spacing(np.abs(want))

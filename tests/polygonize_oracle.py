"""Host restatement of polygonize (xrspatial/experimental/polygonize.py), for the tests only: the closed form of DESIGN.md
§6h in vectorised NumPy.  Cells are ij = i + j * nx; directions E, N, W, S = 0 .. 3.

  links    of an unmasked cell c: W if i > 0, S if j > 0, each where the neighbour d is unmasked and close(c, d); for
           connectivity 8 and j > 0, SW only where the W link is absent, SE only where the S link is absent;
  close    integers: d == c.  Floats: abs_T(d - c) <= 1e-08 + 1e-05 * abs_T(c), difference and abs in T, the threshold a
           float64 multiply then add, the comparison in float64 (the reference's Numba typing; `typing="numpy"` keeps a
           float32 threshold in float32 as plain NumPy 2 does, for the tests that tell the two apart);
  region   0 where masked, else 1 + the number of component roots (smallest cell of a component) before the cell's root;
  state    (cell of region r > 0, direction) with the right-hand cell (S of E, E of N, N of W, W of S) outside the domain
           or not in r; ids compact in (cell, direction) order;
  next     right turn if the forward-right cell is in r, else straight if the forward cell is in r, else left turn;
  start    the (root, E) state of a cycle that has one (the exterior), else the smallest W-facing state (a hole);
  vertex   the tail point ((i, j) for E, (i+1, j) N, (i+1, j+1) W, (i, j+1) S) of the start and of every state whose
           direction differs from its predecessor's, in cycle order; the first point once more at the end;
  order    polygon r - 1 = the exterior of region r, then its holes by start cell; column[r - 1] = values[root].

`mutate` names one deliberate error (the mutation list of DESIGN.md §6h), so that the host tests can show that the fixture
tells each of them apart: "fma", "hole_max", "drop_collinear_start", "sw_always", "tol_neighbour"."""
import numpy as np

E, N, W, S = 0, 1, 2, 3
FX = np.array([1, 0, -1, 0])
FY = np.array([0, 1, 0, -1])
TAILX = np.array([0, 1, 1, 0])
TAILY = np.array([0, 0, 1, 1])


def close(c, d, typing="numba", mutate=None):
    """close(c, d) elementwise: c the later cell (the reference), d its neighbour"""
    if c.dtype.kind in "iub":
        return d == c
    if mutate == "tol_neighbour":
        c, d = d, c
    with np.errstate(all="ignore"):
        diff = np.abs(d - c)
        if typing == "numpy" and c.dtype == np.float32:
            return diff <= np.float32(1e-08) + np.float32(1e-05) * np.abs(c)
        return diff.astype(np.float64) <= 1e-08 + 1e-05 * np.abs(c).astype(np.float64)


def _fma(a, b, c):
    """a * b + c rounded once, elementwise (exact rational arithmetic, then one rounding)"""
    from fractions import Fraction
    return np.array([float(Fraction(a) * Fraction(float(y)) + Fraction(float(z))) for y, z in zip(b, c)])


def links(values, mask, connectivity_8, typing="numba", mutate=None):
    """bool planes (w, s, sw, se): which links each cell has"""
    ny, nx = values.shape
    ok = np.ones((ny, nx), bool) if mask is None else (np.asarray(mask) != 0)

    def link(dy, dx):
        out = np.zeros((ny, nx), bool)
        ys = slice(max(0, -dy), ny - max(0, dy))           # cells whose neighbour (y + dy, x + dx) is inside
        xs = slice(max(0, -dx), nx - max(0, dx))
        yn = slice(max(0, -dy) + dy, ny - max(0, dy) + dy)
        xn = slice(max(0, -dx) + dx, nx - max(0, dx) + dx)
        out[ys, xs] = ok[ys, xs] & ok[yn, xn] & close(values[ys, xs], values[yn, xn], typing, mutate)
        return out

    w, s = link(0, -1), link(-1, 0)
    sw = np.zeros((ny, nx), bool)
    se = np.zeros((ny, nx), bool)
    if connectivity_8:
        sw = link(-1, -1) if mutate == "sw_always" else link(-1, -1) & ~w
        se = link(-1, 1) & ~s
    return ok, w, s, sw, se


def _components(n, a, b):
    """smallest index of each cell's component under the edges a[k] -- b[k]"""
    p = np.arange(n, dtype=np.int64)
    while True:
        pa, pb = p[a], p[b]
        lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
        ch = lo != hi
        if not ch.any():
            return p
        np.minimum.at(p, hi[ch], lo[ch])
        while True:
            q = p[p]
            if np.array_equal(q, p):
                break
            p = q


def regions(values, mask, connectivity_8, typing="numba", mutate=None):
    """(uint32 region plane, number of regions, root cell of each region)"""
    ny, nx = values.shape
    ok, w, s, sw, se = links(values, mask, connectivity_8, typing, mutate)
    idx = np.arange(ny * nx).reshape(ny, nx)
    a = np.concatenate([idx[w], idx[s], idx[sw], idx[se]])
    b = np.concatenate([idx[w] - 1, idx[s] - nx, idx[sw] - nx - 1, idx[se] - nx + 1])
    root = _components(ny * nx, a, b)
    okf = ok.reshape(-1)
    is_root = okf & (root == np.arange(ny * nx))
    before = np.cumsum(is_root) - is_root                  # roots before each cell
    reg = np.where(okf, 1 + before[root], 0).astype(np.uint32)
    return reg.reshape(ny, nx), int(is_root.sum()), np.flatnonzero(is_root)


def flat(values, mask=None, connectivity_8=False, transform=None, typing="numba", mutate=None, stats=None):
    """(column, points [total, 2] float64, ring_offsets int64, polygon_offsets int64)"""
    values = np.asarray(values)
    ny, nx = values.shape
    reg, n_regions, roots = regions(values, mask, connectivity_8, typing, mutate)
    pad = np.zeros((ny + 2, nx + 2), np.int64)             # the domain edge acts as "not in r": region 0 all round
    pad[1:-1, 1:-1] = reg

    def at(dx, dy):                                        # region of the cell at (i + dx, j + dy), flat
        return pad[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx].reshape(-1)

    r = reg.reshape(-1).astype(np.int64)
    n = ny * nx
    exists = np.zeros((n, 4), bool)
    for d in range(4):
        rd = (d + 3) & 3                                   # the right-hand side of d
        exists[:, d] = (r > 0) & (at(FX[rd], FY[rd]) != r)
    ids = (np.cumsum(exists.reshape(-1)) - 1).reshape(n, 4)
    n_states = int(exists.sum())
    if stats is not None:
        stats.update(regions=n_regions, states=n_states)
    column = values.reshape(-1)[roots]
    if n_states == 0:
        return column, np.empty((0, 2)), np.zeros(1, np.int64), np.zeros(1, np.int64)

    cell = np.repeat(np.arange(n), 4).reshape(n, 4)[exists]             # of every state, in id order
    dirn = np.tile(np.arange(4), n).reshape(n, 4)[exists]
    i, j = cell % nx, cell // nx
    rs = r[cell]
    rd = (dirn + 3) & 3
    ax, ay = i + FX[dirn], j + FY[dirn]                                  # forward
    bx, by = ax + FX[rd], ay + FY[rd]                                    # forward-right
    right = pad[by + 1, bx + 1] == rs
    straight = ~right & (pad[ay + 1, ax + 1] == rs)
    ni = np.where(right, bx, np.where(straight, ax, i))
    nj = np.where(right, by, np.where(straight, ay, j))
    nd = np.where(right, rd, np.where(straight, dirn, (dirn + 1) & 3))
    nxt0 = ids[nj * nx + ni, nd]
    assert exists[nj * nx + ni, nd].all()
    assert np.array_equal(np.sort(nxt0), np.arange(n_states))            # a bijection
    emit = np.zeros(n_states, bool)
    emit[nxt0] = nd != dirn

    # ring leader: minimum over each cycle of key, by pointer doubling
    e = np.arange(n_states, dtype=np.int64)
    is_root_e = (dirn == E) & np.isin(cell, roots)
    big = np.int64(1) << 40
    if mutate == "hole_max":
        key = np.where(is_root_e, e, np.where(dirn == W, (np.int64(1) << 32) - e, big))
    else:
        key = np.where(is_root_e, e, np.where(dirn == W, (np.int64(1) << 31) | e, big))
    nxt = nxt0.copy()
    rounds = 0
    while True:
        k2 = np.minimum(key, key[nxt])
        rounds += 1
        if np.array_equal(k2, key):
            break
        key, nxt = k2, nxt[nxt]
    if mutate == "hole_max":
        lead = np.where(key < (np.int64(1) << 31), key, (np.int64(1) << 32) - key)
    else:
        lead = key & ((np.int64(1) << 31) - 1)
    start = lead == e
    if stats is not None:
        stats.update(leader_rounds=rounds)

    # rank: suffix sums of the emit weights along each cycle cut in front of its start
    force = mutate != "drop_collinear_start"                             # the start emits its point even where it is collinear
    val = np.where(start & force, 1, emit).astype(np.int64)
    val = np.append(val, 0)
    nx_ = np.append(np.where(start[nxt0], n_states, nxt0), n_states)
    while (nx_ != n_states).any():
        val = val + val[nx_]
        nx_ = nx_[nx_]
    suffix = val[:n_states]
    count = suffix[lead]
    rank = count - suffix

    # ring table
    starts = np.flatnonzero(start)
    order = np.lexsort((starts, rs[starts]))
    starts = starts[order]
    ring_of = np.zeros(n_states, np.int64)
    ring_of[starts] = np.arange(len(starts))
    ring_offsets = np.concatenate([[0], np.cumsum(suffix[starts] + 1)]).astype(np.int64)
    ring_region = rs[starts]
    first = np.flatnonzero(np.concatenate([[True], ring_region[1:] != ring_region[:-1]]))
    assert len(first) == n_regions
    polygon_offsets = np.append(first, len(starts)).astype(np.int64)

    # points
    px = (i + TAILX[dirn]).astype(np.float64)
    py = (j + TAILY[dirn]).astype(np.float64)
    if transform is not None:
        t = [float(v) for v in transform]
        if mutate == "fma":                                              # t0 * i + fma(t1, j, .) rounds once
            px, py = _fma(t[1], py, t[0] * px) + t[2], _fma(t[4], py, t[3] * px) + t[5]
        else:
            px, py = t[0] * px + t[1] * py + t[2], t[3] * px + t[4] * py + t[5]
    does = emit | (start & force)
    points = np.empty((int(ring_offsets[-1]), 2))
    pos = ring_offsets[ring_of[lead]] + rank
    points[pos[does], 0] = px[does]
    points[pos[does], 1] = py[does]
    ends = ring_offsets[1:] - 1
    points[ends] = points[ring_offsets[:-1]]
    if stats is not None:
        stats.update(rings=len(starts), points=int(ring_offsets[-1]))
    return column, points, ring_offsets, polygon_offsets


def assemble(column, points, ring_offsets, polygon_offsets):
    """the reference's (column, polygons) lists from the flat arrays"""
    rings = [points[ring_offsets[k]:ring_offsets[k + 1]] for k in range(len(ring_offsets) - 1)]
    return list(column), [rings[polygon_offsets[p]:polygon_offsets[p + 1]] for p in range(len(polygon_offsets) - 1)]


def flatten(column, polygons, dtype):
    """flat arrays from the reference's lists"""
    rings = [ring for poly in polygons for ring in poly]
    points = np.concatenate(rings).astype(np.float64) if rings else np.empty((0, 2))
    ring_offsets = np.concatenate([[0], np.cumsum([len(ring) for ring in rings])]).astype(np.int64)
    polygon_offsets = np.concatenate([[0], np.cumsum([len(poly) for poly in polygons])]).astype(np.int64)
    return np.array(column, dtype=dtype).reshape(-1), points.reshape(-1, 2), ring_offsets, polygon_offsets

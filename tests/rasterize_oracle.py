"""Host statement of rasterize, for the tests only: the written rule in NumPy, vectorised per edge.  The
reference has no rasterize; the rule's anchor is that it inverts polygonize (tests/test_rasterize_host.py).

  pixel space  a0 = t4 / det, a1 = -t1 / det, a2 = -t3 / det, a3 = t0 / det with det = t0 * t4 - t1 * t3; every vertex goes to
               u = a0 * dx + a1 * dy, v = a2 * dx + a3 * dy with dx = x - t2, dy = y - t5, each operation float64 and rounded on
               its own.  Cell (row j, column i) has its centre at (i + 0.5, j + 0.5).
  edges        every ring point to the ring's next point, the last to the first; v0 == v1 gives nothing; every other edge is
               put in canonical order, the end with the smaller v first.
  crossings    edge (u0, v0)-(u1, v1), v0 < v1, crosses row j iff v0 <= j + 0.5 < v1 and 0 <= j < H, at
               ux = u0 + ((vc - v0) * (u1 - u0)) / (v1 - v0), vc = j + 0.5; its column is the first i with i + 0.5 >= ux,
               clamped to [0, W].
  inside       cell (j, i) is inside polygon p iff p's crossings in row j with column <= i are odd in number.
  merge        a cell takes the value of the covering polygon that `merge` ranks highest, `fill` where none covers it.

`mutate` names one deliberate error (the mutation list of DESIGN.md §6r): "no_canonical" (edges evaluated as walked),
"closed_rows" (v0 <= vc <= v1), "col_gt" (the first i with i + 0.5 > ux), "fma" (a0 * dx + a1 * dy and a2 * dx + a3 * dy with the
first product fused into the sum; ux itself holds no product that feeds a sum, so it has nothing to fuse), "winding" (non-zero
winding instead of even-odd), "last_as_first"."""
import numpy as np

from tests.polygonize_oracle import _fma

MERGES = ("last", "first", "min", "max", "count")
MUTATIONS = ("no_canonical", "closed_rows", "col_gt", "fma", "winding", "last_as_first")
CHUNK_CELLS = 4_000_000                                       # (polygons x rows x columns) worked on at a time


def flatten(polygons):
    """(points [n, 2] float64, ring_offsets, polygon_offsets) from a list of polygons, each a list of (n, 2) rings"""
    rings = [np.asarray(ring, np.float64).reshape(-1, 2) for poly in polygons for ring in poly]
    points = np.concatenate(rings) if rings else np.empty((0, 2))
    ring_offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    polygon_offsets = np.concatenate([[0], np.cumsum([len(poly) for poly in polygons])]).astype(np.int64)
    return points.reshape(-1, 2), ring_offsets, polygon_offsets


def inverse(transform):
    """(a0, a1, a2, a3, t2, t5) of a pixel-to-world transform"""
    t = [float(v) for v in transform]
    det = t[0] * t[4] - t[1] * t[3]
    return t[4] / det, -t[1] / det, -t[3] / det, t[0] / det, t[2], t[5]


def pixel_space(points, transform=None, mutate=None):
    x, y = points[:, 0].astype(np.float64), points[:, 1].astype(np.float64)
    if transform is None:
        return x, y
    a0, a1, a2, a3, t2, t5 = inverse(transform)
    dx, dy = x - t2, y - t5
    if mutate == "fma":
        return _fma(a0, dx, a1 * dy), _fma(a2, dx, a3 * dy)
    return a0 * dx + a1 * dy, a2 * dx + a3 * dy


def crossings(points, ring_offsets, polygon_offsets, shape, transform=None, mutate=None):
    """(polygon, row, column, sign) of every crossing; sign is +1 where the edge as walked goes up in v, else -1"""
    H, W = shape
    points = np.asarray(points, np.float64).reshape(-1, 2)
    ro, po = np.asarray(ring_offsets, np.int64), np.asarray(polygon_offsets, np.int64)
    n = len(points)
    empty = tuple(np.zeros(0, np.int64) for _ in range(4))
    if n == 0:
        return empty
    u, v = pixel_space(points, transform, mutate)
    ring = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    poly = np.repeat(np.arange(len(po) - 1), np.diff(po))[ring]
    nxt = np.arange(n) + 1
    ends = ro[1:][np.diff(ro) > 0] - 1                        # the last point of every ring that has points
    nxt[ends] = ro[:-1][np.diff(ro) > 0]
    ua, va, ub, vb = u, v, u[nxt], v[nxt]
    up = vb > va
    keep = va != vb
    swap = vb < va
    lo_v, hi_v = np.where(swap, vb, va), np.where(swap, va, vb)
    if mutate == "no_canonical":
        u0, v0, u1, v1 = ua, va, ub, vb
    else:
        u0, v0, u1, v1 = np.where(swap, ub, ua), lo_v, np.where(swap, ua, ub), hi_v
    vc = np.arange(H) + 0.5
    jlo = np.searchsorted(vc, lo_v, "left")                   # the first row with vc >= v0
    jhi = np.searchsorted(vc, hi_v, "right" if mutate == "closed_rows" else "left")   # the first row with vc >= v1 (> v1)
    cnt = np.where(keep, np.maximum(jhi - jlo, 0), 0)
    total = int(cnt.sum())
    if total == 0:
        return empty
    e = np.repeat(np.arange(n), cnt)
    j = jlo[e] + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    vcj = j + 0.5
    with np.errstate(all="ignore"):
        ux = u0[e] + ((vcj - v0[e]) * (u1[e] - u0[e])) / (v1[e] - v0[e])
    col = np.searchsorted(np.arange(W) + 0.5, ux, "right" if mutate == "col_gt" else "left")   # first i with i + 0.5 >= ux
    return poly[e].astype(np.int64), j.astype(np.int64), col.astype(np.int64), np.where(up[e], 1, -1).astype(np.int64)


def priorities(merge, values, n, mutate=None):
    """priority of every polygon, 0 .. n - 1 all different: a cell takes the covering polygon with the highest"""
    if mutate == "last_as_first" and merge == "last":
        merge = "first"
    p = np.arange(n, dtype=np.int64)
    if merge == "last":
        return p
    if merge == "first":
        return n - 1 - p
    if merge in ("min", "max"):
        _, level = np.unique(np.asarray(values), return_inverse=True)    # equal values share a level
        level = level.astype(np.int64).reshape(-1)
        if merge == "min":
            level = level.max(initial=0) - level
        score = level * n + p                                  # ties go to the later polygon
        prio = np.empty(n, np.int64)
        prio[np.argsort(score)] = p
        return prio
    raise ValueError(merge)


def planes(points, ring_offsets, polygon_offsets, shape, priority=None, transform=None, mutate=None, stats=None):
    """(count plane, winner plane) as uint32: the number of polygons covering each cell, and 1 + the highest priority among
    them (0 where no polygon covers the cell)"""
    H, W = shape
    n_polys = len(polygon_offsets) - 1
    p, j, col, sign = crossings(points, ring_offsets, polygon_offsets, shape, transform, mutate)
    if stats is not None:
        stats.update(crossings=len(p))
    count = np.zeros((H, W), np.int64)
    winner = np.zeros((H, W), np.int64)
    prio1 = (np.arange(n_polys, dtype=np.int64) if priority is None else np.asarray(priority, np.int64)) + 1
    per = max(1, CHUNK_CELLS // (H * (W + 1)))
    order = np.argsort(p, kind="stable")
    p, j, col, sign = p[order], j[order], col[order], sign[order]
    for pa in range(int(p.min()) if len(p) else 0, (int(p.max()) + 1) if len(p) else 0, per):
        pb = min(pa + per, n_polys)
        a, b = np.searchsorted(p, pa, "left"), np.searchsorted(p, pb, "left")
        if a == b:
            continue
        flat = ((p[a:b] - pa) * H + j[a:b]) * (W + 1) + col[a:b]
        size = (pb - pa) * H * (W + 1)
        if mutate == "winding":
            delta = np.rint(np.bincount(flat, weights=sign[a:b], minlength=size)).astype(np.int64)
            inside = np.cumsum(delta.reshape(pb - pa, H, W + 1), axis=2)[:, :, :W] != 0
        else:
            delta = np.bincount(flat, minlength=size)
            inside = (np.cumsum(delta.reshape(pb - pa, H, W + 1), axis=2)[:, :, :W] & 1) == 1
        count += inside.sum(axis=0)
        winner = np.maximum(winner, np.where(inside, prio1[pa:pb, None, None], 0).max(axis=0))
    return count.astype(np.uint32), winner.astype(np.uint32)


def rasterize(points, ring_offsets, polygon_offsets, shape, column=None, transform=None, fill=0, dtype=None, merge="last",
              mutate=None, stats=None):
    """the raster, a NumPy array of `dtype` (default: the column's; int32 for column=None and for merge="count")"""
    n_polys = len(polygon_offsets) - 1
    if merge == "count":
        dtype = np.dtype(np.int32 if dtype is None else dtype)
        count, _ = planes(points, ring_offsets, polygon_offsets, shape, None, transform, mutate, stats)
        return count.astype(dtype)
    values = np.arange(1, n_polys + 1, dtype=np.int32) if column is None else np.asarray(column)
    dtype = np.dtype(values.dtype if dtype is None else dtype)
    values = values.astype(dtype)
    prio = priorities(merge, values, n_polys, mutate)
    _, winner = planes(points, ring_offsets, polygon_offsets, shape, prio, transform, mutate, stats)
    by_prio = np.empty(n_polys, np.int64)
    by_prio[prio] = np.arange(n_polys)
    out = np.full(shape, fill, dtype)
    covered = winner > 0
    out[covered] = values[by_prio[winner[covered].astype(np.int64) - 1]]
    return out


# ------------------------------------------------------------------ shared test inputs
def partition(seed, snap, shape=(13, 17), cells=(5, 6)):
    """A jittered vertex lattice cut into triangles with random orientation and random diagonals, its hull outside the
    raster: (points, ring_offsets, polygon_offsets).  `snap` rounds every vertex to a multiple of 0.5, which puts many cell
    centres exactly on edges and vertices."""
    rng = np.random.default_rng(seed)
    H, W = shape
    ny, nx = cells
    gy = np.linspace(-2.0, H + 2.0, ny + 1)
    gx = np.linspace(-2.0, W + 2.0, nx + 1)
    X, Y = np.meshgrid(gx, gy)
    jit = 0.3 * min((H + 4.0) / ny, (W + 4.0) / nx)
    inner = np.zeros_like(X, bool)
    inner[1:-1, 1:-1] = True
    X = X + np.where(inner, rng.uniform(-jit, jit, X.shape), 0.0)
    Y = Y + np.where(inner, rng.uniform(-jit, jit, Y.shape), 0.0)
    if snap:
        X, Y = np.round(X * 2) / 2, np.round(Y * 2) / 2
    tris = []
    for a in range(ny):
        for b in range(nx):
            q = [(a, b), (a, b + 1), (a + 1, b + 1), (a + 1, b)]
            pairs = ([q[0], q[1], q[2]], [q[0], q[2], q[3]]) if rng.random() < 0.5 else ([q[0], q[1], q[3]], [q[1], q[2], q[3]])
            for tri in pairs:
                pts = np.array([[X[i], Y[i]] for i in tri])
                area = (pts[1, 0] - pts[0, 0]) * (pts[2, 1] - pts[0, 1]) - (pts[2, 0] - pts[0, 0]) * (pts[1, 1] - pts[0, 1])
                if area == 0:                                  # (a snapped sliver: covers nothing, belongs to nobody)
                    continue
                if rng.random() < 0.5:
                    pts = pts[::-1]
                if rng.random() < 0.5:                         # closed, as polygonize gives them, or open
                    pts = np.concatenate([pts, pts[:1]])
                tris.append([pts])
    return flatten(tris)


def random_polygons(seed, n, shape, spread=0.6):
    """n overlapping triangles and quadrilaterals around the raster, some reaching outside it"""
    rng = np.random.default_rng(seed)
    H, W = shape
    polys = []
    for _ in range(n):
        c = rng.uniform([-0.1 * W, -0.1 * H], [1.1 * W, 1.1 * H])
        k = int(rng.integers(3, 5))
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        rad = rng.uniform(0.1, spread) * min(H, W) * rng.uniform(0.5, 1.0, k)
        polys.append([np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], axis=1)])
    return flatten(polys)

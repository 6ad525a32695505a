"""The rule of xrspatial_amd/pathfinding.py on the CPU: a heap Dijkstra from the goal over the exact distances
(a, b) = a + b sqrt(2) with the integer comparison, the walk from the start, the snap of `_find_nearest_pixel` on integer squares,
and a counter of shortest paths.  No floats except the output's running sum.  Test infrastructure only."""
import functools
import heapq
import warnings

import numpy as np

NB8 = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))        # (dy, dx), `_neighborhood_structure`
NB4 = ((0, -1), (-1, 0), (1, 0), (0, 1))
SQRT2 = 1.4142135623730951


def sign(da, db):
    """the sign of da + db sqrt(2), in integers"""
    if da >= 0 and db >= 0:
        return 1 if (da or db) else 0
    if da <= 0 and db <= 0:
        return -1
    p, q = da * da, 2 * db * db
    return (1 if p > q else -1) if da > 0 else (1 if q > p else -1)


@functools.total_ordering
class Dist:
    __slots__ = ("a", "b")

    def __init__(self, a, b):
        self.a, self.b = a, b

    def __eq__(self, o):
        return self.a == o.a and self.b == o.b

    def __lt__(self, o):
        return sign(self.a - o.a, self.b - o.b) < 0


def crossable(data, barriers):
    """rule 1, with NumPy's own `==` (an integer raster and integer barriers compare as integers)"""
    data = np.asarray(data)
    ok = np.ones(data.shape, bool)
    if data.dtype.kind == "f":
        ok &= ~np.isnan(data)
    bar = np.asarray(barriers)
    for v in bar.ravel():
        if data.dtype.kind in "iub" and bar.dtype.kind in "iub":
            ok &= ~(data.astype(object) == int(v)).astype(bool)          # Python integers: exact beyond 2^53 and 2^63
        else:
            with np.errstate(invalid="ignore"):
                ok &= ~(data.astype(np.float64) == np.float64(v))
    return ok


def field(ok, goal, connectivity):
    """{(r, c): (a, b)} of every cell reachable from the goal"""
    nbs = NB8 if connectivity == 8 else NB4
    h, w = ok.shape
    done = {}
    heap = [(Dist(0, 0), goal)]
    while heap:
        d, (r, c) = heapq.heappop(heap)
        if (r, c) in done:
            continue
        done[(r, c)] = (d.a, d.b)
        for dy, dx in nbs:
            nr, nc = r + dy, c + dx
            if 0 <= nr < h and 0 <= nc < w and ok[nr, nc] and (nr, nc) not in done:
                heapq.heappush(heap, (Dist(d.a + (not (dy and dx)), d.b + bool(dy and dx)), (nr, nc)))
    return done


def snap(ok, py, px):
    """rule 5; (-1, -1) when no cell qualifies"""
    if ok[py, px]:
        return py, px
    h, w = ok.shape
    best, at = (h - 1) ** 2 + (w - 1) ** 2, (-1, -1)
    for r, c in np.argwhere(ok):                                         # row-major
        d2 = (int(r) - py) ** 2 + (int(c) - px) ** 2
        if d2 < best:
            best, at = d2, (int(r), int(c))
    return at


def count_paths(dist, start, connectivity, cap=1 << 62):
    """the number of shortest paths start -> goal: a DP over the field in the order of the distances"""
    nbs = NB8 if connectivity == 8 else NB4
    ways = {}
    for cell in sorted(dist, key=lambda k: Dist(*dist[k])):
        a, b = dist[cell]
        if (a, b) == (0, 0):
            ways[cell] = 1
            continue
        n = 0
        for dy, dx in nbs:
            nb = (cell[0] + dy, cell[1] + dx)
            if nb in dist and dist[nb] == (a - (not (dy and dx)), b - bool(dy and dx)):
                n += ways[nb]
        ways[cell] = min(n, cap)
    return ways[start]


def run(data, start, goal, barriers=(), connectivity=8, snap_start=False, snap_goal=False):
    """dict(image float64, start, goal after snapping, warn_start, warn_goal, found, a, b, n_paths)"""
    data = np.asarray(data)
    ok = crossable(data, barriers)
    h, w = data.shape
    sy, sx = snap(ok, *start) if snap_start else start
    gy, gx = snap(ok, *goal) if snap_goal else goal
    res = dict(image=np.full((h, w), np.nan), start=(sy, sx), goal=(gy, gx), warn_start=not ok[sy, sx], warn_goal=not ok[gy, gx],
               found=False, a=-1, b=-1, n_paths=0)                      # ([-1, -1] is the last cell, as for the reference)
    if sy < 0 or gy < 0 or not ok[sy, sx] or not ok[gy, gx]:
        return res
    dist = field(ok, (gy, gx), connectivity)
    if (sy, sx) not in dist:
        return res
    a, b = dist[(sy, sx)]
    res.update(found=True, a=a, b=b, n_paths=count_paths(dist, (sy, sx), connectivity))
    nbs = NB8 if connectivity == 8 else NB4
    cur, g = (sy, sx), 0.0
    res["image"][cur] = 0.0
    for _ in range(a + b):
        ca, cb = dist[cur]
        for dy, dx in nbs:
            nb = (cur[0] + dy, cur[1] + dx)
            if nb in dist and dist[nb] == (ca - (not (dy and dx)), cb - bool(dy and dx)):
                cur = nb
                g = g + (SQRT2 if dy and dx else 1.0)
                res["image"][cur] = g
                break
        else:
            raise AssertionError("the walk found no step")
    assert cur == (gy, gx)
    return res


def run_warned(*args, **kw):
    """`run`, issuing the two warnings the way the public function does"""
    res = run(*args, **kw)
    if res["warn_start"]:
        warnings.warn("Start at a non crossable location", Warning)
    if res["warn_goal"]:
        warnings.warn("End at a non crossable location", Warning)
    return res

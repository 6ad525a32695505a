"""The rule of proximity / allocation / direction in NumPy, brute force over all targets.  Test infrastructure
only.

For the cell (i, j) at (x2, y2) = (xs[j], ys[i]):
  1. targets: non-zero finite cells, or cells equal to one of `target_values` under NumPy's `==`;
  2. d32 = float32(_distance(xs[c], x2, ys[r], y2, metric)), float64 arithmetic on the coordinates in the reference's order;
  3. the smallest d32 wins; ties: rows r <= i before rows r > i, among the former the first in row-major order, among the
     latter the last;
  4. s = d32 * d32 in float32; kept if float64(max_distance)**2 >= s (or max_distance infinite), else NaN;
  5. proximity = float32(sqrt(float64(s))), allocation = float32(raster[r, c]), direction = `_calc_direction`.
"""
import numpy as np

METRICS = {"EUCLIDEAN": 0, "GREAT_CIRCLE": 1, "MANHATTAN": 2}
RADIUS2 = 6378137 * 2


def targets(z, target_values=()):
    tv = np.asarray(target_values).ravel()
    if tv.size == 0:
        with np.errstate(invalid="ignore"):
            return (z != 0) & np.isfinite(z)
    mask = np.zeros(z.shape, bool)
    for k in range(tv.size):
        mask |= z == tv[k:k + 1]                                         # array against array: NumPy's promotion
    return mask


def distance(xt, x2, yt, y2, metric):
    """`_distance(x1 = target x, x2 = cell x, y1 = target y, y2 = cell y)` on broadcast float64 arrays"""
    if metric == 0:
        x, y = xt - x2, yt - y2
        d = np.sqrt(x * x + y * y)
    elif metric == 2:
        d = np.abs(xt - x2) + np.abs(yt - y2)
    else:
        lat1, lon1, lat2, lon2 = np.radians(yt), np.radians(xt), np.radians(y2), np.radians(x2)
        dlon, dlat = lon2 - lon1, lat2 - lat1
        s1, s2 = np.sin(dlat / 2.0), np.sin(dlon / 2.0)
        a = s1 * s1 + np.cos(lat1) * np.cos(lat2) * (s2 * s2)
        d = RADIUS2 * np.arcsin(np.sqrt(a))
    return d.astype(np.float32)


def compass(x1, x2, y1, y2):
    """`_calc_direction` from (x1, y1) to (x2, y2), where they differ"""
    d = np.arctan2(-(y2 - y1), x2 - x1) * 57.29578
    d = np.where(d < 0, 90.0 - d, np.where(d > 90.0, 360.0 - d + 90.0, 90.0 - d))
    return d.astype(np.float32)


def run(z, xs, ys, target_values=(), max_distance=np.inf, metric="EUCLIDEAN"):
    """dict(proximity, allocation, direction: float32 planes; row, col: the winner's indices, -1 for none; second: the
    smallest d32 of any OTHER target, inf for none; d32: the winner's)"""
    z = np.asarray(z)
    metric = METRICS.get(metric, 0) if isinstance(metric, str) else int(metric)
    max_distance = np.inf if max_distance is None else max_distance
    rows, cols = z.shape
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    tr, tc = np.nonzero(targets(z, target_values))                       # row-major order
    n = rows * cols
    flat = tr.astype(np.int64) * cols + tc
    out = {k: np.full((rows, cols), np.nan, np.float32) for k in ("proximity", "allocation", "direction")}
    out["row"], out["col"] = np.full((rows, cols), -1, np.int64), np.full((rows, cols), -1, np.int64)
    out["second"], out["d32"] = np.full((rows, cols), np.inf, np.float32), np.full((rows, cols), np.inf, np.float32)
    if not tr.size:
        return out
    md2 = np.float64(max_distance) ** 2
    for i in range(rows):
        d = distance(xs[tc][None, :], xs[:, None], ys[tr][None, :], ys[i], metric)          # cols x targets
        key = np.where(tr <= i, flat, 2 * n - flat)[None, :]
        dmin = d.min(axis=1)
        pick = np.where(d == dmin[:, None], key, np.iinfo(np.int64).max).argmin(axis=1)
        r, c = tr[pick], tc[pick]
        if tr.size > 1:
            rest = d.copy()
            rest[np.arange(cols), pick] = np.inf
            out["second"][i] = rest.min(axis=1)
        s = dmin * dmin                                                   # float32
        kept = (md2 >= s.astype(np.float64)) | np.isinf(np.float64(max_distance))
        out["d32"][i] = dmin
        out["row"][i], out["col"][i] = np.where(kept, r, -1), np.where(kept, c, -1)
        prox = np.sqrt(s.astype(np.float64)).astype(np.float32)
        alloc = z[r, c].astype(np.float32)
        own = (r == i) & (c == np.arange(cols))
        with np.errstate(invalid="ignore"):
            direc = np.where(own, np.float32(0), compass(xs, xs[c], ys[i], ys[r]))
        for k, v in (("proximity", prox), ("allocation", alloc), ("direction", direc)):
            out[k][i] = np.where(kept, v, np.float32(np.nan))
    return out


def ulps(a, b):
    """distance of two non-negative float32 arrays in units in the last place (inf: a large number)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))

"""The rule of idw as brute-force NumPy: the full cells x points matrix of d2, a stable argsort per cell for the
(d2, index) order, and the rank loop for the sums with separate products and sums.  NumPy's float64 `*`, `+`, `/` and `sqrt` are
correctly rounded and never fused, which is all the rule asks for.  Small inputs only: the matrix is dense."""
import numpy as np


def inverse(transform):
    """(a0, a1, a2, a3, t2, t5) of a pixel-to-world transform: rasterize's, in the same order of operations."""
    t = [float(v) for v in transform]
    det = t[0] * t[4] - t[1] * t[3]
    return t[4] / det, -t[1] / det, -t[3] / det, t[0] / det, t[2], t[5]


def to_pixel(points, transform=None):
    points = np.asarray(points, np.float64).reshape(-1, 2)
    if transform is None:
        return points[:, 0].copy(), points[:, 1].copy()
    a0, a1, a2, a3, t2, t5 = inverse(transform)
    with np.errstate(all="ignore"):
        dx, dy = points[:, 0] - t2, points[:, 1] - t5
        return a0 * dx + a1 * dy, a2 * dx + a3 * dy


def radius_squared(max_distance, transform=None):
    if max_distance is None:
        return None
    d = float(max_distance)
    if transform is not None:
        d = d / abs(float(transform[0]))
    return d * d


def d2_matrix(px, py, shape):
    """[cells, points]: dx = p.x - c.x, dy = p.y - c.y, d2 = dx * dx + dy * dy."""
    rows, cols = shape
    cy, cx = np.mgrid[0:rows, 0:cols]
    cx, cy = cx.reshape(-1, 1) + 0.5, cy.reshape(-1, 1) + 0.5
    with np.errstate(all="ignore"):
        dx, dy = px[None, :] - cx, py[None, :] - cy
        return dx * dx + dy * dy


def neighbors(points, shape, k, max_distance=None, transform=None):
    """(index int32 [k, H, W], d2 float64 [k, H, W]): -1 and +inf where a cell has fewer than k candidates."""
    rows, cols = shape
    px, py = to_pixel(points, transform)
    n = len(px)
    index = np.full((k, rows * cols), -1, np.int32)
    d2 = np.full((k, rows * cols), np.inf)
    if n:
        m = d2_matrix(px, py, shape)
        order = np.argsort(m, axis=1, kind="stable")              # equal d2: by index
        ranked = np.take_along_axis(m, order, axis=1)
        md2 = radius_squared(max_distance, transform)
        cand = np.ones_like(ranked, bool) if md2 is None else ranked <= md2     # candidates are a prefix of the ranking
        kk = min(k, n)
        index[:kk] = np.where(cand[:, :kk], order[:, :kk], -1).T
        d2[:kk] = np.where(cand[:, :kk], ranked[:, :kk], np.inf).T
    return index.reshape(k, rows, cols), d2.reshape(k, rows, cols)


def weight(d2, power):
    with np.errstate(all="ignore"):
        half = power // 2
        if half:
            m = d2.copy()
            for _ in range(half - 1):
                m = m * d2
        else:
            m = np.ones_like(d2)
        if power % 2:
            m = m * np.sqrt(d2)
        return 1.0 / m


def idw(points, values, shape, k=12, power=2, max_distance=None, min_points=1, transform=None, fill=np.nan, dtype=np.float64):
    rows, cols = shape
    points = np.asarray(points, np.float64).reshape(-1, 2)
    values = np.asarray(values, np.float64)
    keep = ~np.isnan(values)
    points, values = points[keep], values[keep]
    index, d2 = neighbors(points, shape, k, max_distance, transform)
    index, d2 = index.reshape(k, -1), d2.reshape(k, -1)
    num, den = np.zeros(rows * cols), np.zeros(rows * cols)
    with np.errstate(all="ignore"):
        for r in range(k):                                        # rank order, nearest first
            real = index[r] >= 0
            v = np.where(real, values[np.maximum(index[r], 0)] if len(values) else 0.0, 0.0)
            w = weight(np.where(real, d2[r], 1.0), power)
            wv = w * v
            num = np.where(real, num + wv, num)
            den = np.where(real, den + w, den)
        res = num / den
    found = (index >= 0).sum(axis=0)
    if len(values):
        res = np.where((index[0] >= 0) & (d2[0] == 0), values[np.maximum(index[0], 0)], res)
    res = np.where(found < min_points, fill, res)
    with np.errstate(all="ignore"):
        return res.reshape(rows, cols).astype(dtype)

"""Host restatements of zonal.regions (xrspatial/zonal.py:1406-1549, `_area_connectivity`), for the tests only.

`restated` is the closed form of DESIGN.md §6b, line for line, with the reference's Numba typing:
  W(c)     the clamped window, in the reference's order (self and duplicates included);
  match    abs_T(w - v) <= 1e-08 + 1e-05 * abs_T(v): difference and abs in the raster's dtype (integers wrap), the
           threshold a float64 multiply then add, the comparison in float64;
  new(c)   no matching entry of W(c) has a smaller linear index;
  links    the matching entries with one another, and c with them when c is not new;
  label    the number of new cells with linear index <= the smallest index of c's component.
NumPy 2 computes the same for float64 and the integer dtypes.  For float32 it keeps the threshold in float32 where Numba
promotes it to float64; `typing="numpy"` gives that variant, for the tests that tell the two apart.

`fast_exact` is for rasters on which the tolerance reduces to exact equality (integers whose differences cannot wrap and
|v| < 1e5, integer-valued floats of that size, NaN): then the partition is plain 4- / 8-connected labelling by value,
computed here by scipy.ndimage.label per value where scipy imports, else by hooking and pointer jumping."""
import numpy as np

N4 = ((0, -1), (-1, 0), (1, 0), (0, 1))
N8 = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def _window_index(rows, cols, n):
    """[(flat index of window entry k of every cell)] in the reference's order, clamped."""
    y, x = np.mgrid[0:rows, 0:cols]
    out = []
    for dy, dx in (N8 if n == 8 else N4):
        wy, wx = np.clip(y + dy, 0, rows - 1), np.clip(x + dx, 0, cols - 1)
        out.append((wy * cols + wx).reshape(-1))
    return out


def _is_nan(a):
    return np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)


def matches(data, n, typing="numba"):
    """(window index list, match list): match[k][i] says whether window entry k of cell i matches cell i."""
    a = np.ascontiguousarray(data).reshape(-1)
    rows, cols = data.shape
    idx = _window_index(rows, cols, n)
    with np.errstate(all="ignore"):
        if typing == "numpy" and a.dtype == np.float32:
            thr = np.float32(1e-08) + np.float32(1e-05) * np.abs(a)
        else:
            thr = 1e-08 + 1e-05 * np.abs(a).astype(np.float64)
        m = []
        for k in idx:
            d = np.abs(a[k] - a)                             # in the raster's dtype: integers wrap
            m.append((d <= thr) if (typing == "numpy" and a.dtype == np.float32) else (d.astype(np.float64) <= thr))
    return idx, m


class _UF:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, a):
        p = self.p
        while p[a] != a:
            p[a] = p[p[a]]
            a = p[a]
        return a

    def union(self, a, b):
        ra, rb = self.find(a), self.find(b)
        if ra != rb:
            if ra < rb:
                self.p[rb] = ra
            else:
                self.p[ra] = rb


def restated(data, n=4, typing="numba"):
    """The reference's labels (float64 array, NaN where the input is NaN), and the number of new cells."""
    data = np.asarray(data)
    rows, cols = data.shape
    N = rows * cols
    out = np.full(N, np.nan)
    if N == 0:
        return out.reshape(rows, cols), 0
    idx, m = matches(data, n, typing)
    nan = _is_nan(data).reshape(-1)
    uf = _UF(N)
    new = np.zeros(N, np.int64)
    for i in range(N):
        if nan[i]:
            continue
        M = [int(idx[k][i]) for k in range(len(idx)) if m[k][i]]
        before = any(e < i for e in M)
        new[i] = not before
        S = M + ([i] if before else [])
        for e in S[1:]:
            uf.union(S[0], e)
    cum = np.cumsum(new)
    for i in range(N):
        if not nan[i]:
            out[i] = cum[uf.find(i)]
    return out.reshape(rows, cols), int(new.sum())


def fast_exact(data, n=4):
    """`restated` for rasters on which a match is exact equality (see the module docstring); vectorised."""
    data = np.asarray(data)
    rows, cols = data.shape
    N = rows * cols
    a = data.reshape(-1)
    valid = ~_is_nan(data).reshape(-1)
    cells = np.arange(N)
    idx = _window_index(rows, cols, n)
    eq = [valid & valid[k] & (a[k] == a) for k in idx]
    new = valid & ~np.any([e & (k < cells) for e, k in zip(eq, idx)], axis=0)
    lab = _components_scipy(data, n, valid)
    if lab is None:
        lab = _components_hook(cells, eq, idx)
    out = np.cumsum(new)[lab].astype(np.float64)
    out[~valid] = np.nan
    return out.reshape(rows, cols), int(new.sum())


def _components_scipy(data, n, valid, max_values=64):
    """smallest cell index of every cell's component (plain 4- / 8-connectivity by value), or None without scipy or
    with too many distinct values."""
    try:
        from scipy import ndimage
    except ImportError:                     # pragma: no cover (scipy is present where the suite runs)
        return None
    values = np.unique(data[~np.isnan(data)] if data.dtype.kind == "f" else data)
    if values.size > max_values:
        return None
    rows, cols = data.shape
    structure = ndimage.generate_binary_structure(2, 2 if n == 8 else 1)
    lab = np.arange(rows * cols)
    for v in values:
        comp, k = ndimage.label(data == v, structure=structure)
        comp = comp.reshape(-1)
        cells = np.flatnonzero(comp)
        first = np.full(k + 1, rows * cols, np.int64)
        np.minimum.at(first, comp[cells], cells)
        lab[cells] = first[comp[cells]]
    return lab


def _components_hook(cells, eq, idx):
    """the same by hooking roots onto smaller roots and pointer jumping, NumPy only"""
    pairs = [(cells[e], k[e]) for e, k in zip(eq, idx)]
    lab = cells.copy()
    while True:
        prev = lab.copy()
        for s, t in pairs:
            ls, lt = lab[s], lab[t]
            lo = np.minimum(ls, lt)
            np.minimum.at(lab, ls, lo)
            np.minimum.at(lab, lt, lo)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, prev):
            return lab


def as_output(labels, data):
    """Labels (float64, NaN kept) in the raster's dtype, NaN cells carrying their input value -- the device's output."""
    data = np.asarray(data)
    if data.dtype.kind == "f":
        out = labels.astype(data.dtype)
        nan = np.isnan(data)
        out[nan] = data[nan]
        return out
    return labels.astype(np.int64).astype(data.dtype)


def fused_threshold(abs_v):
    """1e-08 + 1e-05 * abs_v rounded ONCE (what a fused multiply-add gives), exactly, for the tests that separate it from
    the reference's multiply-then-add."""
    from fractions import Fraction
    return float(Fraction(1e-08) + Fraction(1e-05) * Fraction(float(abs_v)))


def fma_sensitive_pairs(v0=(123456.789, 7470.702, 3.25), per_start=2):
    """float64 (v, w) that form one region with the reference's threshold (multiply, then add) and two with a fused one,
    or the reverse.  d = |w - v| lives on the grid of ulp(v), the two thresholds one ulp(threshold) apart, about 1e-5 of
    that grid: so the search scans consecutive doubles v from each start for a threshold that sits next to a grid point,
    and keeps the pairs on which the two roundings disagree, in either direction of the match."""
    found = []
    for start in v0:
        u = np.spacing(start)
        v = start + np.arange(2_000_000) * u
        unf = 1e-08 + 1e-05 * v
        g = np.round(unf / u) * u
        kept = 0
        for vi, gi in zip(v[np.abs(g - unf) <= 2 * np.spacing(unf)], g[np.abs(g - unf) <= 2 * np.spacing(unf)]):
            vi, gi = float(vi), float(gi)
            if fused_threshold(vi) == 1e-08 + 1e-05 * vi:
                continue
            for w in (vi + gi, vi - gi):
                d = abs(w - vi)
                ref = d <= 1e-08 + 1e-05 * vi or d <= 1e-08 + 1e-05 * abs(w)
                fused = d <= fused_threshold(vi) or d <= fused_threshold(abs(w))
                if ref != fused:
                    found.append((vi, w))
                    kept += 1
                    break
            if kept >= per_start:
                break
    return found

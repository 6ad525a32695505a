"""The written rule of resample as plain NumPy and a double loop per cell: the yardstick of the resample tests.
Nothing here is imported from the package; the tables are built again from the rule's text.

Per axis, the source pixel position of destination position p is s(p) = ((D0 * p + D2) - S2) / S0, every operation rounded;
(D0, D2) and (S0, S2) are the scale and offset of the destination and source transforms along that axis, (1, 0) where there is
none.  A tap participates when its weight is not 0; a source cell is valid when it is inside the raster, not NaN and not equal to
nodata.  The sums use Python floats: IEEE double, one rounding per operation, no fused multiply-add.
"""
import math

import numpy as np

MAX_TAPS = 256
MODE_MAX_WINDOW = 1024
POINT = ("nearest", "bilinear", "cubic", "lanczos")
TAPS = {"bilinear": (0, 2), "cubic": (1, 4), "lanczos": (2, 6)}


# ------------------------------------------------------------------ tables
def axis_pair(transform, axis):
    if transform is None:
        return 1.0, 0.0
    t = [float(v) for v in transform]
    if t[1] != 0 or t[3] != 0:
        raise ValueError("rotation or shear")
    return (t[0], t[2]) if axis == "x" else (t[4], t[5])


def s_of(p, D, S):
    return ((np.float64(D[0]) * np.asarray(p, np.float64) + np.float64(D[1])) - np.float64(S[1])) / np.float64(S[0])


def clip_first(first, taps, n_src):
    return np.array([int(min(max(f, -taps), n_src)) for f in first], dtype=np.int32)


def near(n_src, n_dst, D, S):
    out = np.empty(n_dst, np.int32)
    for i in range(n_dst):
        f = math.floor(float(s_of(i + 0.5, D, S)))
        out[i] = f if 0 <= f < n_src else -1
    return out


def cubic_weight(x):
    a = abs(x)
    if a <= 1.0:
        return (1.5 * a - 2.5) * a * a + 1.0
    if a < 2.0:
        return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
    return 0.0


def interp(method, n_src, n_dst, D, S):
    lead, taps = TAPS[method]
    first = np.empty(n_dst)
    w = np.zeros((n_dst, taps))
    x = np.zeros((n_dst, taps))
    for i in range(n_dst):
        u = float(s_of(i + 0.5, D, S)) - 0.5
        c0 = math.floor(u)
        t = u - c0
        first[i] = c0 - lead
        for k in range(taps):
            x[i, k] = t - float(k - lead)
        if method == "bilinear":
            w[i] = 1.0 - t, t
        elif method == "cubic":
            w[i] = [cubic_weight(v) for v in x[i]]
    if method == "lanczos":
        px = np.pi * x
        with np.errstate(all="ignore"):
            w = 3.0 * np.sin(px) * np.sin(px / 3.0) / (px * px)
        w[(np.abs(x) >= 3.0) | (x == np.floor(x))] = 0.0           # exactly 0 at every integer but 0 and beyond the support
        w[x == 0.0] = 1.0
    for i in range(n_dst):
        total = 0.0
        for k in range(taps):
            total = total + float(w[i, k])
        w[i] = w[i] / total
    return clip_first(first, taps, n_src), w


def area(n_src, n_dst, D, S):
    rows = []
    for i in range(n_dst):
        a, b = float(s_of(float(i), D, S)), float(s_of(float(i + 1), D, S))
        lo, hi = min(a, b), max(a, b)
        c_first, c_last = math.floor(lo), math.ceil(hi) - 1
        rows.append((c_first, [min(hi, c + 1.0) - max(lo, float(c)) for c in range(c_first, c_last + 1)]))
    taps = max(max(len(r[1]) for r in rows), 1)
    if taps > MAX_TAPS:
        raise ValueError(f"{taps} taps, more than {MAX_TAPS}; resample in two steps")
    w = np.zeros((n_dst, taps))
    for i, (_, weights) in enumerate(rows):
        w[i, :len(weights)] = weights
    return clip_first([r[0] for r in rows], taps, n_src), w


def tables(method, src_shape, dst_shape, src_transform=None, dst_transform=None):
    out = {}
    for a, k in (("y", 0), ("x", 1)):
        D, S = axis_pair(dst_transform, a), axis_pair(src_transform, a)
        n_src, n_dst = src_shape[k], dst_shape[k]
        if method in POINT:
            out[f"near_{a}"] = near(n_src, n_dst, D, S)
            if method != "nearest":
                out[f"first_{a}"], out[f"w_{a}"] = interp(method, n_src, n_dst, D, S)
            if method in ("cubic", "lanczos"):
                out[f"fb_first_{a}"], out[f"fb_w_{a}"] = interp("bilinear", n_src, n_dst, D, S)
        else:
            out[f"first_{a}"], out[f"w_{a}"] = area(n_src, n_dst, D, S)
    if method == "mode" and out["w_y"].shape[1] * out["w_x"].shape[1] > MODE_MAX_WINDOW:
        raise ValueError(f"a mode window of more than {MODE_MAX_WINDOW} cells; resample in two steps")
    return out


def shape_transform(src_shape, dst_shape):
    return (src_shape[1] / dst_shape[1], 0.0, 0.0, 0.0, src_shape[0] / dst_shape[0], 0.0)


# ------------------------------------------------------------------ the three evaluations, on any tables
class Source:
    """The raster as nested lists of Python numbers, with the rule's validity test."""

    def __init__(self, src, nodata=None):
        self.a = np.asarray(src)
        self.rows, self.cols = self.a.shape
        self.v = self.a.tolist()
        self.nodata = None
        if nodata is not None and nodata == nodata:
            try:
                item = np.array([nodata]).astype(self.a.dtype)[0] if np.dtype(self.a.dtype).kind == "f" else self.a.dtype.type(int(nodata))
            except (OverflowError, ValueError):
                item = None                                       # no cell of this dtype can equal it
            if item is not None and item == nodata:
                self.nodata = item.item()

    def take(self, y, x):
        """(valid, value)"""
        if not (0 <= y < self.rows and 0 <= x < self.cols):
            return False, None
        v = self.v[y][x]
        if v != v or (self.nodata is not None and v == self.nodata):
            return False, None
        return True, v


def gather(src, near_y, near_x, nodata=None, fill=0):
    s = Source(src, nodata)
    out = np.empty((len(near_y), len(near_x)), s.a.dtype)
    for r, y in enumerate(near_y.tolist()):
        for c, x in enumerate(near_x.tolist()):
            ok, _ = s.take(y, x)
            out[r, c] = s.a[y, x] if ok else fill
    return out


def cell_sums(s, first_y, w_y, first_x, w_x, r, c):
    """(num, den, valid taps, invalid taps) of cell (r, c): rows ascending, taps ascending.  A sum begins with its first term
    and is +0.0 without one."""
    num = den = None
    good = bad = 0
    for j, wj in enumerate(w_y[r]):
        if wj == 0.0:
            continue
        rj = nj = None
        for i, wi in enumerate(w_x[c]):
            if wi == 0.0:
                continue
            ok, v = s.take(first_y[r] + j, first_x[c] + i)
            if ok:
                rj = wi * float(v) if rj is None else rj + wi * float(v)
                nj = wi if nj is None else nj + wi
                good += 1
            else:
                bad += 1
        rj, nj = (0.0, 0.0) if rj is None else (rj, nj)
        num = wj * rj if num is None else num + wj * rj
        den = wj * nj if den is None else den + wj * nj
    return (0.0, 0.0, good, bad) if num is None else (num, den, good, bad)


def weighted(src, first_y, w_y, first_x, w_x, near_y=None, near_x=None, fb=None, divide=True, nodata=None, fill=np.nan,
             dtype=np.float64):
    """`fb`: (first_y, w_y, first_x, w_x) of the fallback tables, or None."""
    s = Source(src, nodata)
    lists = [t.tolist() for t in (first_y, w_y, first_x, w_x)]
    fb_lists = None if fb is None else [t.tolist() for t in fb]
    out = np.empty((len(first_y), len(first_x)), np.float64)
    for r in range(out.shape[0]):
        for c in range(out.shape[1]):
            num, den, good, bad = cell_sums(s, *lists, r, c)
            if near_y is not None:
                is_fill = not s.take(int(near_y[r]), int(near_x[c]))[0]
            else:
                is_fill = good == 0
            if not is_fill and fb_lists is not None and bad:
                num, den, good, bad = cell_sums(s, *fb_lists, r, c)
                if near_y is None:
                    is_fill = good == 0
            if is_fill:
                out[r, c] = fill
            elif divide:
                with np.errstate(all="ignore"):
                    out[r, c] = np.float64(num) / np.float64(den)
            else:
                out[r, c] = num
    with np.errstate(all="ignore"):
        return out.astype(dtype)


def select(src, first_y, w_y, first_x, w_x, op, nodata=None, fill=0):
    s = Source(src, nodata)
    fy, wy, fx, wx = (t.tolist() for t in (first_y, w_y, first_x, w_x))
    out = np.empty((len(fy), len(fx)), s.a.dtype)
    for r in range(out.shape[0]):
        for c in range(out.shape[1]):
            window = []                                           # (y, x) of the valid participating cells, row-major
            for j, wj in enumerate(wy[r]):
                for i, wi in enumerate(wx[c]):
                    if wj != 0.0 and wi != 0.0 and s.take(fy[r] + j, fx[c] + i)[0]:
                        window.append((fy[r] + j, fx[c] + i))
            if not window:
                out[r, c] = fill
                continue
            values = [s.v[y][x] for y, x in window]
            if op == "mode":
                heads = []                                        # [first position, value, members] of every class, by ==
                for k, v in enumerate(values):
                    for h in heads:
                        if h[1] == v:
                            h[2] += 1
                            break
                    else:
                        heads.append([k, v, 1])
                pick = heads[0]
                for h in heads[1:]:
                    if h[2] > pick[2] or (h[2] == pick[2] and h[1] < pick[1]):
                        pick = h
                k = pick[0]
            else:
                k = 0
                for m, v in enumerate(values):
                    if (v < values[k]) if op == "min" else (v > values[k]):
                        k = m
            out[r, c] = s.a[window[k]]
    return out


# ------------------------------------------------------------------ the function
def resample(src, dst_shape, method, src_transform=None, dst_transform=None, nodata=None, fill=None, dtype=None, by_shape=False):
    """`by_shape`: the tables of `shape=` (the same extent, no transforms)."""
    src = np.asarray(src)
    if by_shape:
        src_transform, dst_transform = None, shape_transform(src.shape, dst_shape)
    t = tables(method, src.shape, dst_shape, src_transform, dst_transform)
    if method in ("nearest", "min", "max", "mode"):
        out_dtype = src.dtype
    else:
        out_dtype = np.dtype(dtype) if dtype is not None else np.dtype(np.float32 if src.dtype == np.float32 else np.float64)
    if fill is None:
        fill = np.nan if np.dtype(out_dtype).kind == "f" else 0
    if method == "nearest":
        return gather(src, t["near_y"], t["near_x"], nodata, fill)
    taps = (t["first_y"], t["w_y"], t["first_x"], t["w_x"])
    if method in ("min", "max", "mode"):
        return select(src, *taps, method, nodata, fill)
    fb = (t["fb_first_y"], t["fb_w_y"], t["fb_first_x"], t["fb_w_x"]) if "fb_w_y" in t else None
    return weighted(src, *taps, t.get("near_y"), t.get("near_x"), fb, method != "sum", nodata, fill, out_dtype)

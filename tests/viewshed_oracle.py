"""NumPy restatement of the reference's viewshed (xrspatial/viewshed.py, the CPU sweep) as a per-cell predicate: DESIGN.md §6d.

Test infrastructure only.  The sweep's status tree answers one question per cell q: which cells closer to the viewpoint than
q does the ray to q cross, and how steep is each of them at q's direction.  That is restated here without the sweep:

  tables()   per cell, from the cell alone: the three event angles A0 / A1 / A2 (`_calc_event_pos`, `_calculate_angle`), the
             three event gradients G0 / G1 / G2 (`_calc_event_elev`, `_calc_event_grad`), the key (`_calc_dist_n_grad`), the
             target gradient g and the vertical angle (`_get_vertical_ang`);
  viewshed() per target, a walk along the major axis of its ray: at step k the three cells around round(minor position) are
             tested with exact integer cross products (direction strictly inside the cell's angular span) and `key < d`, and
             the occluder's gradient is interpolated as `_find_max_value_within_key` does.  Vectorised over the targets
             (`_walk`).

Every `atan` goes through `math.atan` (what the reference calls, undecorated or under Numba); +, -, *, / and sqrt are IEEE
in NumPy.  So on the NumPy that executed the reference for tests/golden/viewshed_exec.npz the result is bit-equal to it
(tests/test_viewshed_host.py).  Returns (out, margin): margin = |max occluder gradient - g|, inf where no occluder raised
the maximum."""
import math

import numpy as np

PI = math.pi
INVISIBLE = -1.0

# ENTER (0) and EXIT (2) corner of a cell, in half cells (row, col), by 3 * (sign(drow) + 1) + sign(dcol) + 1
#            NW        N         NE        W         vp      E          SW        S         SE
OY0 = np.array([-1, +1, +1, -1, 0, +1, -1, -1, +1], np.int8)
OX0 = np.array([+1, +1, +1, +1, 0, -1, -1, -1, -1], np.int8)
OY2 = np.array([+1, +1, -1, +1, 0, -1, +1, -1, -1], np.int8)
OX2 = np.array([-1, -1, -1, +1, 0, -1, +1, +1, +1], np.int8)


def _atan(a):
    a = np.asarray(a, np.float64)
    return np.array([math.atan(v) for v in a.ravel().tolist()], np.float64).reshape(a.shape)


def _angle(dy, dx):
    """`_calculate_angle` of a point at (dy, dx) index offsets from the viewpoint (rows grow downwards)"""
    with np.errstate(all="ignore"):
        ang = _atan(np.abs(dy) / np.abs(dx))
    out = np.zeros(ang.shape)
    out = np.where((dx > 0) & (dy < 0), ang, out)
    out = np.where((dx < 0) & (dy < 0), PI - ang, out)
    out = np.where((dx < 0) & (dy > 0), PI + ang, out)
    out = np.where((dx > 0) & (dy > 0), PI * 2.0 - ang, out)
    out = np.where((dx < 0) & (dy == 0), PI, out)
    out = np.where((dx == 0) & (dy < 0), PI / 2, out)
    out = np.where((dx == 0) & (dy > 0), PI * 3.0 / 2.0, out)
    return out


def _gradient(elev, dy, dx, vpe, ew_res, ns_res):
    """`_calc_event_grad` at (dy, dx) index offsets"""
    x = dx * ew_res
    y = dy * ns_res
    d2 = (x * x) + (y * y)
    with np.errstate(all="ignore"):
        return _atan((elev - vpe) / np.sqrt(d2)), d2


def _corner_elev(z, oy, ox):
    """`_calc_event_elev`: mean of the 2 x 2 block behind the corner (oy, ox in {-1, +1} per cell), or the cell itself"""
    h, w = z.shape
    rr, cc = np.mgrid[0:h, 0:w]
    r1, c1 = rr + oy, cc + ox
    inside = (r1 >= 0) & (r1 < h) & (c1 >= 0) & (c1 < w)
    r1c, c1c = np.clip(r1, 0, h - 1), np.clip(c1, 0, w - 1)
    e1, e2, e3, e4 = z[r1c, c1c], z[r1c, cc], z[rr, c1c], z
    nan = np.isnan(e1) | np.isnan(e2) | np.isnan(e3) | np.isnan(e4)
    with np.errstate(all="ignore"):
        mean = (e1 + e2 + e3 + e4) / 4.0
    return np.where(inside & ~nan, mean, z)


def tables(z, vr, vc, ew_res, ns_res, observer_elev=0, target_elev=0):
    z = np.asarray(z).astype(np.float64)
    h, w = z.shape
    vpe = z[vr, vc] + observer_elev
    rr, cc = np.mgrid[0:h, 0:w]
    dr, dc = rr - vr, cc - vc
    case = 3 * (np.sign(dr) + 1) + np.sign(dc) + 1
    t = {"vpe": vpe, "case": case, "dr": dr, "dc": dc}
    for k, oy, ox in ((0, OY0[case], OX0[case]), (2, OY2[case], OX2[case])):
        dy, dx = dr + 0.5 * oy, dc + 0.5 * ox
        t[f"A{k}"] = _angle(dy, dx)
        t[f"G{k}"], _ = _gradient(_corner_elev(z, oy, ox), dy, dx, vpe, ew_res, ns_res)
    t["A1"] = _angle(dr, dc)
    t["G1"], t["key"] = _gradient(z, dr, dc, vpe, ew_res, ns_res)
    zt = z + target_elev
    t["g"], _ = _gradient(zt, dr, dc, vpe, ew_res, ns_res)
    diff = vpe - zt                                       # `_get_vertical_ang`
    with np.errstate(all="ignore"):
        root = np.sqrt(t["key"])
        above = _atan(root / diff) * 180 / PI
        below = _atan(np.abs(diff) / root) * 180 / PI + 90
    t["vert"] = np.where(diff == 0.0, 90.0, np.where(diff > 0, above, below))
    return t


CLEAR = 1e-12


def _walk(flat, shape, view, by_row, q, qr, qc, a, d, best):
    """The walk of the targets whose major axis is the row axis (`by_row`) or the column axis, sorted by descending ray
    length; raises `best` (per target) to the largest occluder gradient.  The integer tests run on every candidate (inside
    the raster, not the target, the two cross products), the survivors are compressed and tested for the key and -- before
    the interpolation -- for whether the occluder can raise the maximum at all: its gradient at any direction is a convex
    combination of two of G0 / G1 / G2, computed to a few ulp, so a cell whose largest one is CLEAR below the maximum is
    skipped without changing a bit of the result."""
    (h, w), (vr, vc) = shape, view
    qa, qb = (qr, qc) if by_row else (qc, qr)                 # offsets along the major and the minor axis
    big, small, step, lean = np.abs(qa), np.abs(qb), np.sign(qa), np.sign(qb)
    lo, hi = (-vc, w - vc) if by_row else (-vr, h - vr)       # the minor offsets inside the raster
    base = 3 * (step + 1) + 1 if by_row else step + 4         # the corner tables' index, but for the minor offset's sign
    key, top = flat["key"], flat["top"]
    for k in range(1, int(big[0]) + 1 if q.size else 1):
        n = int(np.searchsorted(-big, -k, side="right"))       # the targets whose ray is at least k steps long
        qan, qbn = qa[:n], qb[:n]
        rnd = (2 * k * small[:n] + big[:n]) // (2 * big[:n]) * lean[:n]
        ca = k * step[:n]
        last = big[:n] == k                                    # at its last step a ray meets the target itself
        for j in (-1, 0, 1):
            cb = rnd + j
            case = base[:n] + np.sign(cb) * (1 if by_row else 3)
            cr2, cc2, tr, tc = (2 * ca, 2 * cb, qan, qbn) if by_row else (2 * cb, 2 * ca, qbn, qan)
            keep = (cb >= lo) & (cb < hi) & ~(last & (cb == qbn))
            # u x v = u_r * v_c - u_c * v_r > 0: v lies counter-clockwise of u (rows grow downwards)
            keep &= (cr2 + OY0[case]) * tc - (cc2 + OX0[case]) * tr > 0              # ENTER corner x target
            keep &= tr * (cc2 + OX2[case]) - tc * (cr2 + OY2[case]) > 0              # target x EXIT corner
            i = np.flatnonzero(keep)
            cr, cc = (ca[i], cb[i]) if by_row else (cb[i], ca[i])
            c = (cr + vr) * w + (cc + vc)
            keep = (key[c] < d[i]) & (top[c] > best[i] - CLEAR)
            i, c, cr, cc = i[keep], c[keep], cr[keep], cc[keep]
            if not i.size:
                continue
            tr, tc = (qa[i], qb[i]) if by_row else (qb[i], qa[i])
            side = tr * cc - tc * cr                           # > 0: the target's direction comes before the centre's
            east = (cr == 0) & (cc > 0)
            a0, a1, a2, g0, g1, g2 = (flat[name][c] for name in ("A0", "A1", "A2", "G0", "G1", "G2"))
            ai = a[i]
            with np.errstate(all="ignore"):
                before = g1 + (g0 - g1) * (a1 - ai) / (a1 - a0)
                after = g1 + (g2 - g1) * (ai - a1) / (a2 - a1)
                east_after = g1 + (g2 - g1) * ai / a2
                east_before = g1 + (g0 - g1) * (2 * PI - ai) / (2 * PI - a0)
            cur = np.where(side > 0, before, np.where(side < 0, after, g1))
            cur = np.where(east, np.where(side > 0, east_before, east_after), cur)
            cur = np.where((ai == 0) & east, g1, cur)
            raise_it = cur > best[i]                           # a NaN gradient never raises the maximum
            best[i[raise_it]] = cur[raise_it]


def viewshed(z, vr, vc, ew_res, ns_res, observer_elev=0, target_elev=0):
    """(out, margin) of the raster `z` seen from cell (vr, vc)"""
    t = tables(z, vr, vc, ew_res, ns_res, observer_elev, target_elev)
    h, w = t["key"].shape
    flat = {k: t[k].ravel() for k in ("A0", "A1", "A2", "G0", "G1", "G2", "key")}
    with np.errstate(all="ignore"):
        top = np.maximum(np.maximum(flat["G0"], flat["G1"]), flat["G2"])
    flat["top"] = np.where(np.isnan(top), np.inf, top)         # (a cell with a NaN gradient is never skipped)
    dr, dc = t["dr"].ravel(), t["dc"].ravel()
    g = t["g"].ravel()
    best_all = np.full(h * w, -np.inf)
    ints = np.int32 if max(h, w) < (1 << 14) else np.int64      # the cross products stay below 2^31 on small rasters
    for by_row in (True, False):
        mine = (np.abs(dr) >= np.abs(dc)) == by_row
        q = np.flatnonzero(mine & ((dr != 0) | (dc != 0)))
        if not q.size:
            continue
        q = q[np.argsort(-np.maximum(np.abs(dr[q]), np.abs(dc[q])), kind="stable")]
        best = np.full(q.size, -np.inf)
        _walk(flat, (h, w), (vr, vc), by_row, q, dr[q].astype(ints), dc[q].astype(ints), flat["A1"][q], flat["key"][q], best)
        best_all[q] = best
    visible = best_all <= g                                    # a NaN g is never visible
    visible[vr * w + vc] = False
    out = np.where(visible, t["vert"].ravel(), INVISIBLE)
    out[vr * w + vc] = 180.0
    with np.errstate(all="ignore"):
        margin = np.where(np.isinf(best_all), np.inf, np.abs(best_all - g))
    return out.reshape(h, w), margin.reshape(h, w)


# ------------------------------------------------------------------ the host side: coordinates -> viewpoint, resolution
def locate(coords, v, what):
    """Index of the coordinate nearest to v as the reference finds it: outside [min, max] raises, of two coordinates equally
    near the larger one wins (pandas' `nearest`, on ascending and descending indexes alike), then the first index holding
    that value."""
    coords = np.asarray(coords)
    if not (coords.min() <= v <= coords.max()):
        raise ValueError(f"{what} argument outside of raster {what}_range")
    dist = np.abs(coords.astype(np.float64) - v)
    nearest = coords[dist == dist.min()].max()
    return int(np.where(coords == nearest)[0][0])


def run(z, xs, ys, x, y, observer_elev=0, target_elev=0):
    """(out, margin) through the coordinates, as the public function is called"""
    z = np.asarray(z)
    h, w = z.shape
    xs, ys = np.asarray(xs), np.asarray(ys)
    vc, vr = locate(xs, x, "x"), locate(ys, y, "y")
    ew_res = (xs[-1] - xs[0]) / (w - 1)
    ns_res = (ys[-1] - ys[0]) / (h - 1)
    return viewshed(z, vr, vc, ew_res, ns_res, observer_elev, target_elev)

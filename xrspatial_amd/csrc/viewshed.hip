// viewshed: the result of the reference's radial sweep as one ray walk per cell.
//
// Reference: xrspatial/viewshed.py, the CPU path (a port of GRASS r.viewshed): 3 (N - 1) events sorted by angle, a red-black
// tree of the cells the sweep line crosses, and per cell q one query, "the steepest of the cells nearer than q at q's
// direction" (`_find_max_value_within_key`).  The query's answer depends on q and the raster only, so it is computed here per
// cell without the sweep; all of it in float64, in the reference's order of operations:
//   events   per cell c: the three event gradients G0 (ENTER corner), G1 (centre), G2 (EXIT corner) = atan((elev - vpe) / dist),
//            corner elevations being the mean of the 2 x 2 block behind the corner (`_calc_event_elev`, `_calc_event_grad`).
//            One thread per cell, 24 bytes written.
//   walk     per target q: the cells that can hold q's direction strictly inside their angular span are crossed by the ray to
//            q, so step k = 1 .. max(|drow|, |dcol|) along the major axis and test the three cells around the rounded minor
//            position: inside the raster, not q, not the viewpoint, key < key(q) (the reference's float64 keys, uncontracted),
//            and two integer cross products against the cell's ENTER and EXIT corners (exact where the reference compares
//            atan values).  An occluder's gradient at q's direction is interpolated between G1 and G0 or G2 over the event
//            angles (recomputed here: two atan instead of 48 more gathered bytes).  Only the verdict leaves, so the walk stops
//            at the first occluder above g, and an occluder whose three gradients all lie clear of g is settled without its
//            angles.  One thread per target, a wave on an 8 x 8 patch so that neighbouring rays gather neighbouring cells.
// Contraction is off for the whole file: keys tie exactly in the reference (`key(c) < d`), and an fma would break the ties.
#include "xrs_common.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr double PI = 3.14159265358979323846;
constexpr int TILE = 16;                       // a block is 16 x 16 targets: four waves of 8 x 8
// ENTER / EXIT corner of a cell in half cells, by 3 * (sign(drow) + 1) + sign(dcol) + 1 (`_calc_event_pos`): bit set = +1
constexpr unsigned OY0 = 294u, OX0 = 15u, OY2 = 75u, OX2 = 456u;
// an occluder whose three gradients are all this far from g is decided without interpolating: the interpolated value is a
// convex combination of two of them, computed to a few ulp of pi / 2 (4e-16)
constexpr double CLEAR = 1e-12;

__device__ __forceinline__ int sign_of(int v) { return (v > 0) - (v < 0); }
__device__ __forceinline__ int corner(unsigned mask, int which) { return (int)((mask >> which) & 1u) * 2 - 1; }
__device__ __forceinline__ int case_of(int dr, int dc) { return 3 * (sign_of(dr) + 1) + sign_of(dc) + 1; }

// `_calculate_angle` of the point at (dy2 / 2, dx2 / 2) index offsets from the viewpoint (rows grow downwards)
__device__ __forceinline__ double event_angle(int dy2, int dx2) {
    if (dx2 == 0) return dy2 < 0 ? PI / 2 : (dy2 > 0 ? PI * 3.0 / 2.0 : 0.0);
    if (dy2 == 0) return dx2 > 0 ? 0.0 : PI;
    const double ang = atan(fabs((double)dy2) / fabs((double)dx2));
    if (dy2 < 0) return dx2 > 0 ? ang : PI - ang;
    return dx2 < 0 ? PI + ang : PI * 2.0 - ang;
}

// squared distance of the point at (dy, dx) index offsets (`_calc_dist_n_grad`)
__device__ __forceinline__ double key_of(double dy, double dx, double ew_res, double ns_res) {
    const double x = dx * ew_res, y = dy * ns_res;
    return (x * x) + (y * y);
}

template <typename T>
__device__ __forceinline__ double corner_elev(const T *__restrict__ z, long rows, long cols, long r, long c, int oy, int ox, double own) {
    const long r1 = r + oy, c1 = c + ox;
    if (r1 < 0 || r1 >= rows || c1 < 0 || c1 >= cols) return own;
    const double e1 = (double)z[r1 * cols + c1], e2 = (double)z[r1 * cols + c], e3 = (double)z[r * cols + c1];
    if (e1 != e1 || e2 != e2 || e3 != e3 || own != own) return own;
    return (e1 + e2 + e3 + own) / 4.0;
}

template <typename T>
__global__ void __launch_bounds__(256) viewshed_events_kernel(const T *__restrict__ z, long rows, long cols, int vr, int vc,
                                                              double observer_elev, double ew_res, double ns_res,
                                                              double *__restrict__ grads) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    const long r = i / cols, c = i - r * cols;
    const int dr = (int)(r - vr), dc = (int)(c - vc);
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (dr != 0 || dc != 0) {
        const double vpe = (double)z[(long)vr * cols + vc] + observer_elev;
        const double own = (double)z[i];
        const int k = case_of(dr, dc);
        const int oy0 = corner(OY0, k), ox0 = corner(OX0, k), oy2 = corner(OY2, k), ox2 = corner(OX2, k);
        const double e0 = corner_elev(z, rows, cols, r, c, oy0, ox0, own), e2 = corner_elev(z, rows, cols, r, c, oy2, ox2, own);
        g0 = atan((e0 - vpe) / sqrt(key_of(dr + 0.5 * oy0, dc + 0.5 * ox0, ew_res, ns_res)));
        g1 = atan((own - vpe) / sqrt(key_of(dr, dc, ew_res, ns_res)));
        g2 = atan((e2 - vpe) / sqrt(key_of(dr + 0.5 * oy2, dc + 0.5 * ox2, ew_res, ns_res)));
    }
    grads[3 * i] = g0;
    grads[3 * i + 1] = g1;
    grads[3 * i + 2] = g2;
}

// the gradient of occluder (cr, cc) -- offsets from the viewpoint -- at the direction `a` of target (qr, qc)
__device__ __forceinline__ double occluder_gradient(int cr, int cc, int qr, int qc, double a, double g0, double g1, double g2) {
    const long side = (long)qr * cc - (long)qc * cr;            // > 0: the target's direction comes before the centre's
    const int k = case_of(cr, cc);
    if (cr == 0 && cc > 0) {                                    // east of the viewpoint on its row: the span wraps through 0
        if (side > 0) {
            const double a0 = event_angle(2 * cr + corner(OY0, k), 2 * cc + corner(OX0, k));
            return g1 + (g0 - g1) * (2 * PI - a) / (2 * PI - a0);
        }
        const double a2 = event_angle(2 * cr + corner(OY2, k), 2 * cc + corner(OX2, k));
        return g1 + (g2 - g1) * a / a2;
    }
    if (side == 0) return g1;
    const double a1 = event_angle(2 * cr, 2 * cc);
    if (side > 0) {
        const double a0 = event_angle(2 * cr + corner(OY0, k), 2 * cc + corner(OX0, k));
        return g1 + (g0 - g1) * (a1 - a) / (a1 - a0);
    }
    const double a2 = event_angle(2 * cr + corner(OY2, k), 2 * cc + corner(OX2, k));
    return g1 + (g2 - g1) * (a - a1) / (a2 - a1);
}

template <typename T>
__global__ void __launch_bounds__(TILE * TILE) viewshed_walk_kernel(const T *__restrict__ z, long rows, long cols, long tiles_x, int vr,
                                                                    int vc, double observer_elev, double target_elev, double ew_res,
                                                                    double ns_res, const double *__restrict__ grads,
                                                                    double *__restrict__ out) {
    const long tile_y = (long)blockIdx.x / tiles_x, tile_x = (long)blockIdx.x - tile_y * tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long r = tile_y * TILE + (wave >> 1) * 8 + (lane >> 3), c = tile_x * TILE + (wave & 1) * 8 + (lane & 7);
    if (r >= rows || c >= cols) return;
    const int qr = (int)(r - vr), qc = (int)(c - vc);
    if (qr == 0 && qc == 0) {
        out[r * cols + c] = 180.0;
        return;
    }
    const double vpe = (double)z[(long)vr * cols + vc] + observer_elev;
    const double zq = (double)z[r * cols + c] + target_elev;
    const double d = key_of(qr, qc, ew_res, ns_res), root = sqrt(d);
    const double g = atan((zq - vpe) / root);
    const double a = event_angle(2 * qr, 2 * qc);
    bool visible = g == g;                                       // a NaN gradient is never visible

    // the walk: `big` steps along the major axis, the minor position rounded half up (any rounding within half a cell does)
    const bool by_row = abs(qr) >= abs(qc);
    const int big = by_row ? abs(qr) : abs(qc), small = by_row ? abs(qc) : abs(qr);
    const int step = by_row ? sign_of(qr) : sign_of(qc), lean = by_row ? sign_of(qc) : sign_of(qr);
    int rnd = 0, acc = big;                                      // floor((2 k small + big) / (2 big)) and its remainder
    for (int k = 1; k <= big && visible; ++k) {
        acc += 2 * small;
        if (acc >= 2 * big) { acc -= 2 * big; ++rnd; }
        for (int j = -1; j <= 1; ++j) {
            const int minor = rnd * lean + j;
            const int cr = by_row ? k * step : minor, cc = by_row ? minor : k * step;
            const long rr = (long)vr + cr, col = (long)vc + cc;
            if (rr < 0 || rr >= rows || col < 0 || col >= cols) continue;
            if ((cr == qr && cc == qc) || (cr == 0 && cc == 0)) continue;
            if (!(key_of(cr, cc, ew_res, ns_res) < d)) continue;
            const int kc = case_of(cr, cc);
            const long r0 = 2L * cr + corner(OY0, kc), c0 = 2L * cc + corner(OX0, kc);
            const long r2 = 2L * cr + corner(OY2, kc), c2 = 2L * cc + corner(OX2, kc);
            // u x v = u_r v_c - u_c v_r > 0: v lies counter-clockwise of u
            if (!(r0 * qc - c0 * qr > 0 && qr * c2 - qc * r2 > 0)) continue;
            const double *__restrict__ gp = grads + 3 * (rr * cols + col);
            const double g0 = gp[0], g1 = gp[1], g2 = gp[2];
            const double hi = fmax(g0, fmax(g1, g2)), lo = fmin(g0, fmin(g1, g2));
            const bool numbers = g0 == g0 && g1 == g1 && g2 == g2;
            if (numbers && hi <= g - CLEAR) continue;
            if (numbers && lo > g + CLEAR) { visible = false; break; }
            if (occluder_gradient(cr, cc, qr, qc, a, g0, g1, g2) > g) { visible = false; break; }
        }
    }

    double res = -1.0;
    if (visible) {                                               // `_get_vertical_ang`
        const double diff = vpe - zq;
        if (diff == 0.0) res = 90.0;
        else if (diff > 0) res = atan(root / diff) * 180 / PI;
        else res = atan(fabs(diff) / root) * 180 / PI + 90;
    }
    out[r * cols + c] = res;
}

template <typename T>
int viewshed_impl(const T *z, long rows, long cols, long vr, long vc, double observer_elev, double target_elev, double ew_res,
                  double ns_res, double *work, double *out, hipStream_t s) {
    if (rows < 2 || cols < 2) return fail("xrs_viewshed: a raster of at least 2 x 2 cells is needed, got %ld x %ld", rows, cols);
    if (rows >= (1L << 30) || cols >= (1L << 30)) return fail("xrs_viewshed: raster too large (%ld x %ld)", rows, cols);
    if (vr < 0 || vr >= rows || vc < 0 || vc >= cols) return fail("xrs_viewshed: viewpoint (%ld, %ld) outside the raster", vr, vc);
    if (!z || !work || !out) return fail("xrs_viewshed: null pointer");
    if (!(std::isfinite(ew_res) && std::isfinite(ns_res) && std::isfinite(observer_elev) && std::isfinite(target_elev)))
        return fail("xrs_viewshed: non-finite resolution or elevation offset");
    const long cells = rows * cols, tiles_x = (cols + TILE - 1) / TILE, tiles_y = (rows + TILE - 1) / TILE;
    if ((cells + 255) / 256 >= (1L << 31) || tiles_x * tiles_y >= (1L << 31))
        return fail("xrs_viewshed: raster too large for one call (%ld x %ld)", rows, cols);
    hipLaunchKernelGGL((viewshed_events_kernel<T>), dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, z, rows, cols, (int)vr,
                       (int)vc, observer_elev, ew_res, ns_res, work);
    XRS_LAUNCH_CHECK();
    hipLaunchKernelGGL((viewshed_walk_kernel<T>), dim3((unsigned)(tiles_x * tiles_y)), dim3(TILE * TILE), 0, s, z, rows, cols, tiles_x,
                       (int)vr, (int)vc, observer_elev, target_elev, ew_res, ns_res, work, out);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t xrs_viewshed_workspace_bytes(int64_t rows, int64_t cols) {
    return rows > 0 && cols > 0 ? (size_t)rows * (size_t)cols * 3 * sizeof(double) : 0;
}

#define XRS_VIEWSHED(SUF, T)                                                                                                       \
    int xrs_viewshed_##SUF(const T *data_dev, int64_t rows, int64_t cols, int64_t view_row, int64_t view_col, double observer_elev, \
                           double target_elev, double ew_res, double ns_res, void *work_dev, double *out_dev, void *stream) {      \
        return viewshed_impl<T>(data_dev, rows, cols, view_row, view_col, observer_elev, target_elev, ew_res, ns_res,             \
                                static_cast<double *>(work_dev), out_dev, as_stream(stream));                                      \
    }
XRS_VIEWSHED(f32, float)
XRS_VIEWSHED(f64, double)

}  // extern "C"

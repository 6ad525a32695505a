// proximity / allocation / direction: the exact nearest target of every cell.
//
// Reference: xrspatial/proximity.py, a port of GDAL's four-pass line sweep in which a cell inherits the nearest target of three
// neighbours -- serial along rows and from row to row, and a heuristic.  What is computed here is the minimum itself, with the
// reference's arithmetic per candidate and the sweep's order among equidistant targets:
//   distance   d32 = float32(_distance(xs[c], x2, ys[r], y2, metric)) in float64 on the coordinate values, uncontracted;
//   winner     the smallest d32; among equal ones targets in rows r <= i come first, there the first in row-major order, among
//              rows r > i the last in row-major order (one int64 key per candidate, smaller wins);
//   kept       where float64(max_distance)^2 >= d32 * d32 (float32), else NaN.
// One fact carries the search: along a fixed target row and strictly monotonic xs every metric is non-decreasing in |c - j|
// (haversine while |dlon| <= 180 degrees), so a row's nearest target is its nearest one at or left of j, or its nearest one
// right of j.  Longitudes in [-180, 180] may lie up to 360 degrees apart; beyond 180 degrees haversine falls again, so on a
// raster that spans more than 180 degrees the row's first and last target are two more candidates.
//   scan     one block per row: left[i][j] = largest c <= j holding a target, right[i][j] = smallest c > j, -1 for none.  A
//            max-scan over (c + 1) left to right and one over (cols - c) right to left, each a wave scan (wave_reduce.h), the
//            four wave totals through LDS and a carry from span to span of SPAN columns.  The row's flag says whether it holds
//            a target at all; a one-block pass compacts the flags into the ascending list of non-empty rows.
//   search   one thread per cell, a block on SPAN adjacent columns of one row, so the walk over rows is uniform: from the
//            cell's place in the list outwards, above and below in turn, two candidates per row.  A side is finished for a
//            lane once the row's lower bound (|dy|; R |dlat| (1 - 1e-12) for haversine) as float32 is strictly above the best
//            d32 (rounding is monotonic, so no target of that row can tie) or its square is beyond max_distance^2.
//            Several targets of one row on one side of j can share a d32: with square cells only beyond ~2^11.5 cells, with
//            long thin cells (or coordinates so small that d32 underflows) whole runs of them.  Rule 3 then names the far end
//            of the run, not the nearest: EUCLIDEAN and MANHATTAN move the winner there after the walk (tied_end).
// Known limit: GREAT_CIRCLE does not extend (the device's sin / asin are not the reference's to the last bit, so a float32 tie
// there is not the rule's tie anyway): proximity is unaffected, allocation / direction name the nearest of the float32-
// equidistant targets of a row side where the rule may name another.
// Workspace (ABI, include/xrs_hip.h): left | right | flag | list | count, each part rounded up to 256 bytes (carve()).
// Contraction is off for the whole file: dx * dx + dy * dy must round as the reference's.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "value_match.h"
#include "wave_reduce.h"
#include "workspace.h"

#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr int SPAN = 256;                      // columns per scan step and per search block: four waves
constexpr int EUCLIDEAN = 0, GREAT_CIRCLE = 1, MANHATTAN = 2;
constexpr int MODE_PROXIMITY = 0, MODE_ALLOCATION = 1, MODE_DIRECTION = 2, MODE_ALL = 3;

struct Work {
    int *left, *right, *flag, *list, *count;
    size_t total;
};
Work carve(void *base, size_t rows, size_t cols) {
    Carver c(base);
    Work w = {};
    w.left = c.take<int>(rows * cols);
    w.right = c.take<int>(rows * cols);
    w.flag = c.take<int>(rows);
    w.list = c.take<int>(rows);
    w.count = c.take_bytes<int>(256);
    w.total = c.at();
    return w;
}

// rule 1: non-zero and finite, or equal to one of `values` under NumPy's == (64-bit integers as integers)
template <typename T>
__device__ __forceinline__ bool is_target(T v, const void *__restrict__ values, int kind, int n) {
    if (n == 0) {
        if constexpr (std::is_floating_point<T>::value) return v != (T)0 && isfinite(v);
        else return v != (T)0;
    }
    return matches_any<T>(v, values, kind, n);
}

// the four wave totals of step `it` (inclusive scans' last lanes): what lies before this wave, and everything
__device__ __forceinline__ void fold_totals(const int (&tot)[2][4], int it, int wave, int carry, int &before, int &all) {
    before = all = carry;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int t = tot[it & 1][w];
        all = max(all, t);
        if (w < wave) before = max(before, t);
    }
}

template <typename T>
__global__ void __launch_bounds__(SPAN) proximity_scan_kernel(const T *__restrict__ data, long cols, const void *__restrict__ values,
                                                              int kind, int n_values, int *__restrict__ left, int *__restrict__ right,
                                                              int *__restrict__ flag) {
    __shared__ int tot[2][4];                   // two steps' totals: one barrier per step
    const long row = blockIdx.x;
    const T *__restrict__ in = data + row * cols;
    int *L = left + row * cols, *R = right + row * cols;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int it = 0, carry = 0, before, all;
    for (long base = 0; base < cols; base += SPAN, ++it) {              // left to right: the largest c + 1 so far
        const long j = base + threadIdx.x;
        const int v = (j < cols && is_target<T>(in[j], values, kind, n_values)) ? (int)j + 1 : 0;
        const int inc = wave_scan_max_i32(v);
        if (lane == 63) tot[it & 1][wave] = inc;
        __syncthreads();
        fold_totals(tot, it, wave, carry, before, all);
        if (j < cols) L[j] = max(inc, before) - 1;
        carry = all;
    }
    if (threadIdx.x == 0) flag[row] = carry > 0;
    __syncthreads();                                                     // L is read back below by other lanes
    carry = 0;
    for (long hi = cols; hi > 0; hi -= SPAN, ++it) {                     // right to left: the largest cols - c so far
        const long j = hi - 1 - threadIdx.x;
        const int v = (j >= 0 && L[j] == (int)j) ? (int)(cols - j) : 0;
        const int inc = wave_scan_max_i32(v);
        if (lane == 63) tot[it & 1][wave] = inc;
        __syncthreads();
        fold_totals(tot, it, wave, carry, before, all);
        int prev = __shfl_up(inc, 1);                                    // exclusive: c > j
        if (lane == 0) prev = 0;
        const int e = max(prev, before);
        if (j >= 0) R[j] = e > 0 ? (int)(cols - e) : -1;
        carry = all;
    }
}

// the ascending list of rows whose flag is set, and its length
__global__ void __launch_bounds__(SPAN) proximity_rows_kernel(const int *__restrict__ flag, long rows, int *__restrict__ list,
                                                              int *__restrict__ count) {
    __shared__ int tot[2][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int it = 0, carry = 0;
    for (long base = 0; base < rows; base += SPAN, ++it) {
        const long r = base + threadIdx.x;
        const int f = r < rows ? flag[r] : 0;
        const int inc = wave_scan_i32(f);
        if (lane == 63) tot[it & 1][wave] = inc;
        __syncthreads();
        int before = carry, all = carry;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int t = tot[it & 1][w];
            all += t;
            if (w < wave) before += t;
        }
        if (f) list[before + inc - 1] = (int)r;
        carry = all;
    }
    if (threadIdx.x == 0) *count = carry;
}

struct Search {
    const void *data;
    int dtype;
    long rows, cols;
    const double *xs, *ys, *lon, *lat, *coslat;  // lon / lat / coslat: np.radians(xs), np.radians(ys), np.cos(np.radians(ys))
    const int *left, *right, *list, *count;
    double max2;                                 // float64(max_distance)^2, +inf for an infinite one
    int mode;
    float *out;                                  // MODE_ALL: three planes
};

// `_calc_direction(x2, xs[c], y2, ys[r])` of a target that is not the cell itself
__device__ __forceinline__ float compass(double x, double y) {
    double d = atan2(-y, x) * 57.29578;
    if (d < 0) d = 90.0 - d;
    else if (d > 90.0) d = 360.0 - d + 90.0;
    else d = 90.0 - d;
    return (float)d;
}

template <int METRIC>
__global__ void __launch_bounds__(SPAN) proximity_search_kernel(const Search p) {
    const long spans = (p.cols + SPAN - 1) / SPAN;
    const long i = (long)blockIdx.x / spans;
    const long j0 = ((long)blockIdx.x - i * spans) * SPAN + threadIdx.x;
    const bool valid = j0 < p.cols;
    const long j = valid ? j0 : p.cols - 1;                              // surplus lanes walk along and write nothing
    const double x2 = p.xs[j], y2 = p.ys[i];
    double lon2 = 0.0, lat2 = 0.0, cos2 = 0.0;
    if (METRIC == GREAT_CIRCLE) { lon2 = p.lon[j]; lat2 = p.lat[i]; cos2 = p.coslat[i]; }
    const long cells = p.rows * p.cols;
    // longitudes more than 180 degrees apart: along a row haversine falls again beyond 180 degrees, so the row's first and
    // last target are candidates too (the far end of the row may be the near one round the back of the sphere)
    const bool wraps = METRIC == GREAT_CIRCLE && fabs(p.lon[p.cols - 1] - p.lon[0]) > 3.14159265358979323846;

    // the last non-empty row at or above i
    const int n = *p.count;
    int lo = -1, hi = n;                                                 // list[lo] <= i < list[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.list[mid] <= i) lo = mid; else hi = mid;
    }
    int up = lo, dn = hi;

    float best = INFINITY;
    long best_key = 0x7fffffffffffffffL;
    int best_r = -1, best_c = -1;
    bool open_up = valid, open_dn = valid;

    auto d32_of = [&](int r, int c) -> float {
        double d;
        if (METRIC == EUCLIDEAN) {
            const double dx = p.xs[c] - x2, dy = p.ys[r] - y2;
            d = sqrt(dx * dx + dy * dy);
        } else if (METRIC == MANHATTAN) {
            const double dx = p.xs[c] - x2, dy = p.ys[r] - y2;
            d = fabs(dx) + fabs(dy);
        } else {
            const double dlon = lon2 - p.lon[c], dlat = lat2 - p.lat[r];
            const double sa = sin(dlat / 2.0), so = sin(dlon / 2.0);
            const double a = sa * sa + p.coslat[r] * cos2 * (so * so);
            d = 12756274.0 * asin(sqrt(a));
        }
        return (float)d;
    };

    // rule 3 inside the winner's row (EUCLIDEAN / MANHATTAN), once per cell after the walk.  The keys of two rows are ordered by
    // the rows alone, so which row wins does not depend on which of its equidistant targets stands for it; the walk keeps the
    // nearest.  The columns of row r that share its d32 form one run, as d32 is monotonic in |c - j| in the very arithmetic
    // above.  Above (r <= i) the rule names the run's leftmost target: beyond the nearest-left candidate (a winner right of j
    // means that nothing at or left of j ties).  Below it names the rightmost, beyond the nearest-right one.  Whether there is
    // a run at all is decided in steps of rising cost: may_tie on the next column, the next target's d32, and only then the
    // run's far end by bisection over the column index and one step back to the first target inside it through left / right:
    // log2(cols) distances, never the chain of targets link by link.
    //
    // may_tie: can column `next` (one further from j than c) round to c's d32?  Necessary, not sufficient, and without a
    // sqrt.  Equal float32 values in the normal range lie within one ulp, at most 2^-23 relative, so the float64 distances b >= a
    // have b / a < 1 + 2^-23 < 1 + 1.2e-7 (their squares: < 1 + 2^-22 + 2^-46 < 1 + 2.4e-7; the float64 roundings of a and b, 1e-16,
    // vanish in the margin).  Outside the normal range -- below 2^-126 the spacing is absolute, above 2^127 everything is inf
    // -- the exact comparison decides.
    auto may_tie = [&](int r, int c, int next) -> bool {
        const double dy = p.ys[r] - y2, dx = p.xs[c] - x2, dn = p.xs[next] - x2;
        if (METRIC == EUCLIDEAN) {
            const double a = dx * dx + dy * dy, b = dn * dn + dy * dy;
            return b - a <= a * 2.4e-7 || b < 0x1p-250 || !(b < 0x1p254);
        }
        const double a = fabs(dx) + fabs(dy), b = fabs(dn) + fabs(dy);
        return b - a <= a * 1.2e-7 || b < 0x1p-125 || !(b < 0x1p127);
    };
    auto tied_end = [&](int r, long at, int c, float d32, bool above) -> int {
        if (above) {
            if (c > j || c == 0 || !may_tie(r, c, c - 1)) return c;
            const int nb = p.left[at + c - 1];
            if (nb < 0 || d32_of(r, nb) != d32) return c;
            int lo = 0, hi = nb;                                         // d32_of(hi) == d32: the smallest such column
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (d32_of(r, mid) == d32) hi = mid; else lo = mid + 1;
            }
            const int e = p.left[at + lo] == lo ? lo : p.right[at + lo];
            return e >= 0 && e < nb ? e : nb;                            // (inside [lo, nb] whatever the planes hold)
        }
        if (c <= j || c == (int)p.cols - 1 || !may_tie(r, c, c + 1)) return c;
        const int nb = p.right[at + c];
        if (nb < 0 || d32_of(r, nb) != d32) return c;
        int lo = nb, hi = (int)p.cols - 1;                               // d32_of(lo) == d32: the largest such column
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (d32_of(r, mid) == d32) lo = mid; else hi = mid - 1;
        }
        const int e = p.left[at + lo];
        return e > nb ? e : nb;                                          // (inside [nb, lo])
    };

    auto visit = [&](int r, bool &open, bool above) {
        float bound;
        if (METRIC == GREAT_CIRCLE) bound = (float)(6378137.0 * fabs(lat2 - p.lat[r]) * (1.0 - 1e-12));
        else bound = (float)fabs(p.ys[r] - y2);
        if (bound > best || (double)(bound * bound) > p.max2) { open = false; return; }
        const long at = (long)r * p.cols;
        int cand[4] = {p.left[at + j], p.right[at + j], -1, -1};
        if (METRIC == GREAT_CIRCLE && wraps) {                           // the row's first and last target
            cand[2] = p.left[at] == 0 ? 0 : p.right[at];
            cand[3] = p.left[at + p.cols - 1];
        }
#pragma unroll
        for (int k = 0; k < (METRIC == GREAT_CIRCLE ? 4 : 2); ++k) {
            const int c = cand[k];
            if (c < 0) continue;
            const float d32 = d32_of(r, c);
            const long key = above ? at + c : 2 * cells - (at + c);
            if (d32 < best || (d32 == best && key < best_key)) { best = d32; best_key = key; best_r = r; best_c = c; }
        }
    };

    while (true) {
        const bool go_up = up >= 0 && __ballot(open_up) != 0, go_dn = dn < n && __ballot(open_dn) != 0;
        if (!go_up && !go_dn) break;
        if (go_up) {
            if (open_up) visit(p.list[up], open_up, true);
            --up;
        }
        if (go_dn) {
            if (open_dn) visit(p.list[dn], open_dn, false);
            ++dn;
        }
    }
    if (!valid) return;
    if (METRIC != GREAT_CIRCLE && p.mode != MODE_PROXIMITY && best_r >= 0)   // (the distance is the same wherever in the run)
        best_c = tied_end(best_r, (long)best_r * p.cols, best_c, best, best_r <= i);

    const float s = best * best;
    const bool kept = best_r >= 0 && (p.max2 >= (double)s);
    float prox = nan_f32(), alloc = nan_f32(), dir = nan_f32();
    if (kept) {
        prox = (float)sqrt((double)s);
        if (p.mode == MODE_ALLOCATION || p.mode == MODE_ALL) alloc = load_as<float>(p.data, p.dtype, (long)best_r * p.cols + best_c);
        if (p.mode == MODE_DIRECTION || p.mode == MODE_ALL)
            dir = (best_r == i && best_c == j) ? 0.0f : compass(p.xs[best_c] - x2, p.ys[best_r] - y2);
    }
    const long at = i * p.cols + j;
    if (p.mode == MODE_ALL) {
        p.out[at] = prox;
        p.out[cells + at] = alloc;
        p.out[2 * cells + at] = dir;
    } else {
        p.out[at] = p.mode == MODE_PROXIMITY ? prox : (p.mode == MODE_ALLOCATION ? alloc : dir);
    }
}

template <typename T>
void launch_scan(const void *data, long rows, long cols, const void *values, int kind, int n_values, int *left, int *right,
                 int *flag, hipStream_t s) {
    hipLaunchKernelGGL((proximity_scan_kernel<T>), dim3((unsigned)rows), dim3(SPAN), 0, s, static_cast<const T *>(data), cols, values,
                       kind, n_values, left, right, flag);
}

}  // namespace

extern "C" {

size_t xrs_proximity_workspace_bytes(int64_t rows, int64_t cols) {
    return rows > 0 && cols > 0 ? carve(nullptr, (size_t)rows, (size_t)cols).total : 0;
}

int xrs_proximity(const void *data_dev, int dtype, int64_t rows, int64_t cols, const double *xs_dev, const double *ys_dev,
                  const double *gc_dev, const void *values_dev, int values_kind, int n_values, double max_distance, int metric,
                  int mode, void *work_dev, float *out_dev, void *stream) {
    const int product = mode & 3;
    const bool do_scan = !(mode & XRS_PROX_SEARCH_ONLY), do_search = !(mode & XRS_PROX_SCAN_ONLY);
    if (rows < 0 || cols < 0) return fail("xrs_proximity: negative shape");
    if (mode & ~(3 | XRS_PROX_SCAN_ONLY | XRS_PROX_SEARCH_ONLY) || !(do_scan || do_search))
        return fail("xrs_proximity: unknown mode %d", mode);
    if (metric != EUCLIDEAN && metric != GREAT_CIRCLE && metric != MANHATTAN) return fail("xrs_proximity: unknown metric %d", metric);
    if (!dtype_bytes(dtype)) return fail("xrs_proximity: unsupported dtype code %d", dtype);
    if (n_values < 0) return fail("xrs_proximity: negative number of target values");
    if (values_kind != XRS_PROX_VALUES_F64 && values_kind != XRS_PROX_VALUES_I64 && values_kind != XRS_PROX_VALUES_U64)
        return fail("xrs_proximity: unknown kind of target values %d", values_kind);
    if (values_kind != XRS_PROX_VALUES_F64 && (dtype == XRS_DT_F32 || dtype == XRS_DT_F64))
        return fail("xrs_proximity: a float raster is compared with float64 target values");
    if (rows == 0 || cols == 0) return 0;
    if (rows >= (1L << 31) - SPAN || cols >= (1L << 31) - SPAN) return fail("xrs_proximity: raster too large (%lld x %lld)", (long long)rows, (long long)cols);
    const long spans = (cols + SPAN - 1) / SPAN;
    if (rows * spans >= (1L << 31)) return fail("xrs_proximity: raster too large for one call (%lld x %lld)", (long long)rows, (long long)cols);
    if (!data_dev || !xs_dev || !ys_dev || !work_dev || (do_search && !out_dev) || (n_values > 0 && !values_dev))
        return fail("xrs_proximity: null pointer");
    if (metric == GREAT_CIRCLE && do_search && !gc_dev) return fail("xrs_proximity: GREAT_CIRCLE needs the coordinates in radians");
    if (max_distance != max_distance) return fail("xrs_proximity: max_distance is NaN");

    hipStream_t s = as_stream(stream);
    const Work w = carve(work_dev, (size_t)rows, (size_t)cols);
    if (do_scan) {
        with_dtype_f32_last(dtype, [&](auto t) {   // (the code was checked above)
            launch_scan<dtype_of<decltype(t)>>(data_dev, rows, cols, values_dev, values_kind, n_values, w.left, w.right, w.flag, s);
        });
        XRS_LAUNCH_CHECK();
        hipLaunchKernelGGL(proximity_rows_kernel, dim3(1), dim3(SPAN), 0, s, w.flag, (long)rows, w.list, w.count);
        XRS_LAUNCH_CHECK();
    }
    if (do_search) {
        Search p;
        p.data = data_dev; p.dtype = dtype; p.rows = rows; p.cols = cols;
        p.xs = xs_dev; p.ys = ys_dev;
        p.lon = gc_dev; p.lat = gc_dev ? gc_dev + cols : nullptr; p.coslat = gc_dev ? gc_dev + cols + rows : nullptr;
        p.left = w.left; p.right = w.right; p.list = w.list; p.count = w.count;
        p.max2 = std::isinf(max_distance) ? INFINITY : max_distance * max_distance;
        p.mode = product; p.out = out_dev;
        const dim3 grid((unsigned)(rows * spans));
        if (metric == EUCLIDEAN) hipLaunchKernelGGL((proximity_search_kernel<EUCLIDEAN>), grid, dim3(SPAN), 0, s, p);
        else if (metric == MANHATTAN) hipLaunchKernelGGL((proximity_search_kernel<MANHATTAN>), grid, dim3(SPAN), 0, s, p);
        else hipLaunchKernelGGL((proximity_search_kernel<GREAT_CIRCLE>), grid, dim3(SPAN), 0, s, p);
        XRS_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"

// idw: inverse-distance interpolation of scattered points onto a raster, with an exact k-nearest-neighbour search per cell.
// The reference tree has no idw; the rule is written down in DESIGN.md §6t and restated in tests/idw_oracle.py.  Pixel (row j,
// column i) is the square [i, i + 1] x [j, j + 1] and its centre is c = (i + 0.5, j + 0.5), as for rasterize (§6r).
//
//   pixel space  rasterize's: u = a0 * dx + a1 * dy, v = a2 * dx + a3 * dy with dx = x - t2, dy = y - t5, every product and
//                sum rounded on its own;
//   distance     dx = p.x - c.x, dy = p.y - c.y, d2 = dx * dx + dy * dy: two products and one sum, no fused multiply-add;
//   selection    the candidates are the points with d2 <= max_d2 (all of them without a radius); the neighbours are the first
//                min(k, candidates) of them by (d2, index): a total order, so the result does not depend on where a point sits
//                in its bin;
//   weight       m = d2 * d2 * .. (power / 2 factors, left to right; 1.0 for power 1), times sqrt(d2) for an odd power;
//                w = 1.0 / m; a first neighbour with d2 == 0 gives its value as the result;
//   value        num = sum w * v and den = sum w in rank order, nearest first, each step one rounded product and one rounded
//                sum; the result is num / den, rounded to the output's dtype.  Fewer than min_points candidates: fill.
//
// Two calls on one stream:
//   xrs_idw_bin     hist_kernel (one thread per point: pixel space, the non-finite flag, its bin; a histogram with integer
//                   atomics) + ExclusiveSum + scatter_kernel (x, y and index of every point, bin by bin).  The bins are squares
//                   of B x B cells, B a power of two, over the raster, with one apron ring around them that takes every point
//                   outside by its clamped bin coordinate.  The ORDER OF THE POINTS INSIDE A BIN is whatever the atomics give;
//                   the (d2, index) rule makes the result independent of it.
//   xrs_idw_search  search_kernel<K, LDS, THREADS>: one workgroup per tile of 16 x 16 cells (16 x 8 for K = 64), a wave on a block
//                   of 8 x 8.  It walks the bins in growing rectangles around the tile's own bins; the bins a ring adds are runs
//                   of consecutive sorted points (a whole bin row at the top and bottom, the left and right ends of the rows
//                   between), which the workgroup lists (one run per thread, a block-wide exclusive sum of their lengths) and
//                   then stages through LDS in chunks of THREADS points, one coalesced load of x, y and index per thread and
//                   chunk.  Every thread tests every staged point against its own k-best list, sorted by (d2, index).  A tile
//                   with no point in its own bins first finds the largest empty rectangle around it (the points of a rectangle
//                   are one difference of bin starts per bin row; doubling, then bisection) and starts behind it.
//
// When a thread may stop.  `bound` is the least distance from its cell centre to a side of the rectangle searched so far that
// has not reached the grid's edge (a side at the edge, apron included, has nothing beyond it: +inf).  A side lies at an integer
// multiple of B and a centre at a half-integer, so `bound` is exact in float64; b2 = bound * bound is rounded like any product.
// A point outside the rectangle lies beyond one side: |p.x - c.x| >= bound (or the same in y) as real numbers, rounding is
// monotone, so the computed |dx| >= bound, the computed dx * dx >= b2, and the computed d2 >= dx * dx >= b2.  So a thread
//   * whose list is full and whose k-th d2 is STRICTLY below b2 can ignore everything outside (a point with an equal d2 and a
//     lower index would otherwise displace the k-th), and
//   * a thread with max_d2 < b2 can too: nothing outside is a candidate.
// Such a thread is done; what it is shown afterwards cannot enter its list, so done threads need no masking (they skip the
// test to save the time, no more).  The workgroup stops when all its threads are done or the rectangle is the grid.
//
// The k-best list.  Capacities 1, 4, 8 and 16 are register arrays behind fully unrolled loops with constant indices (a
// dynamically indexed private array would go to scratch); k < K uses the upper k slots, the lower ones hold a key below every
// real one, so slot K - 1 is always the k-th best.  Capacities 32 and 64 live in LDS, [slot][thread], with the k-th kept in
// registers.  Every loop is bounded, no workgroup waits for another, and every store is an ordinary vector store.
#include "xrs_common.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

#include <type_traits>

// no fused multiply-add anywhere below: the rule's products and sums are rounded one by one
#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr int BIN_THREADS = 256;
constexpr int TILE_W = 16;                                        // cells across a tile; a wave takes 8 x 8 of them
constexpr int NONE = 0x7fffffff;                                  // index of an empty slot: above every real index (n <= 2^31 - 1)

struct Inverse {
    double a0, a1, a2, a3, t2, t5;
    int on;
};

struct Grid {                                                     // the bins: gx x gy of them, the apron ring included
    uint32_t rows, cols;
    int shift;                                                    // B = 1 << shift cells
    uint32_t nbx, nby, gx, gy;
    uint64_t n_bins;
};

// ------------------------------------------------------------------ the rule's arithmetic
__device__ __forceinline__ void to_pixel(const Inverse &m, double x, double y, double &u, double &v) {
    if (!m.on) {
        u = x, v = y;
        return;
    }
    const double dx = x - m.t2, dy = y - m.t5;
    const double ax = m.a0 * dx, by = m.a1 * dy;
    const double cx = m.a2 * dx, ey = m.a3 * dy;
    u = ax + by;
    v = cx + ey;
}

// bin coordinate of a pixel-space coordinate along an axis of `nb` bins: 0 and nb + 1 are the apron.  Comparisons and one
// exact conversion, no division: a coordinate in [0, nb * B) is below 2^33 and truncates to its cell.  NaN goes to 0.
__device__ __forceinline__ uint32_t bin_along(double u, uint32_t nb, int shift) {
    if (!(u >= 0.0)) return 0;
    if (u >= (double)((uint64_t)nb << shift)) return nb + 1;
    return (uint32_t)((uint64_t)u >> shift) + 1;
}

__device__ __forceinline__ size_t bin_of(const Grid &g, double u, double v) {
    return (size_t)bin_along(v, g.nby, g.shift) * g.gx + bin_along(u, g.nbx, g.shift);
}

__device__ __forceinline__ double weight_of(double d2, int power) {
    double m = 1.0;
    const int half = power >> 1;
    if (half) {
        m = d2;
        for (int t = 1; t < half; ++t) m = m * d2;
    }
    if (power & 1) m = m * sqrt(d2);
    return 1.0 / m;
}

__device__ __forceinline__ bool before(double d, int i, double ed, int ei) { return d < ed || (d == ed && i < ei); }

// ------------------------------------------------------------------ bins: histogram, scan, scatter
__global__ void __launch_bounds__(BIN_THREADS) hist_kernel(const double *__restrict__ pts, uint32_t n, Inverse m, Grid g,
                                                           uint32_t *__restrict__ count, uint32_t *__restrict__ flags) {
    const uint64_t t = (uint64_t)blockIdx.x * BIN_THREADS + threadIdx.x;
    bool bad = false;
    if (t < n) {
        const double x = pts[2 * t], y = pts[2 * t + 1];
        double u, v;
        to_pixel(m, x, y, u, v);
        bad = !isfinite(x) || !isfinite(y) || !isfinite(u) || !isfinite(v);
        atomicAdd(count + bin_of(g, u, v), 1u);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, (uint32_t)XRS_IDW_NONFINITE);
}

// a point takes the slot the atomic hands it: the order inside a bin differs from run to run, the result does not (see above)
__global__ void __launch_bounds__(BIN_THREADS) scatter_kernel(const double *__restrict__ pts, uint32_t n, Inverse m, Grid g,
                                                              const uint32_t *__restrict__ start, uint32_t *__restrict__ count,
                                                              double *__restrict__ sx, double *__restrict__ sy,
                                                              int32_t *__restrict__ sidx) {
    const uint64_t t = (uint64_t)blockIdx.x * BIN_THREADS + threadIdx.x;
    if (t >= n) return;
    double u, v;
    to_pixel(m, pts[2 * t], pts[2 * t + 1], u, v);
    const size_t b = bin_of(g, u, v);
    const uint32_t left = atomicSub(count + b, 1u);               // counts down from the histogram to 0
    const uint64_t pos = (uint64_t)start[b] + left - 1;
    if (left == 0 || pos >= n) return;                            // (a histogram of other points: stay inside the arrays)
    sx[pos] = u, sy[pos] = v, sidx[pos] = (int32_t)t;
}

// ------------------------------------------------------------------ the k-best lists
template <int K>
struct RegList {                                                  // slots K - k .. K - 1 are the list, nearest first
    double d[K];
    int i[K];
    __device__ __forceinline__ void init(int k) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const bool used = j >= K - k;
            d[j] = used ? INFINITY : -1.0;                        // -1.0: before every real key, never moved
            i[j] = used ? NONE : 0;
        }
    }
    __device__ __forceinline__ double kth_d() const { return d[K - 1]; }
    __device__ __forceinline__ int kth_i() const { return i[K - 1]; }
    // (cd, ci) is before the k-th: every slot takes its lower neighbour, the candidate or stays
    __device__ __forceinline__ void insert(double cd, int ci) {
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            const bool low = before(cd, ci, d[j - 1], i[j - 1]);
            const bool here = before(cd, ci, d[j], i[j]);
            d[j] = low ? d[j - 1] : (here ? cd : d[j]);
            i[j] = low ? i[j - 1] : (here ? ci : i[j]);
        }
        if (before(cd, ci, d[0], i[0])) d[0] = cd, i[0] = ci;
    }
    template <typename F>
    __device__ __forceinline__ void each(int k, F f) const {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j >= K - k) f(j - (K - k), d[j], i[j]);
    }
};

template <int K, int THREADS>
struct LdsList {                                                  // slots 0 .. k - 1, [slot][thread]
    double *d;
    int *i;
    double wd;                                                    // the k-th, kept in registers for the test
    int wi, k;
    __device__ __forceinline__ void init(int k_) {
        k = k_;
        for (int j = 0; j < k; ++j) d[j * THREADS] = INFINITY, i[j * THREADS] = NONE;
        wd = INFINITY, wi = NONE;
    }
    __device__ __forceinline__ double kth_d() const { return wd; }
    __device__ __forceinline__ int kth_i() const { return wi; }
    __device__ __forceinline__ void insert(double cd, int ci) {
        int j = k - 1;
        for (; j > 0 && before(cd, ci, d[(j - 1) * THREADS], i[(j - 1) * THREADS]); --j)
            d[j * THREADS] = d[(j - 1) * THREADS], i[j * THREADS] = i[(j - 1) * THREADS];
        d[j * THREADS] = cd, i[j * THREADS] = ci;
        wd = d[(k - 1) * THREADS], wi = i[(k - 1) * THREADS];
    }
    template <typename F>
    __device__ __forceinline__ void each(int k_, F f) const {
        for (int j = 0; j < k_; ++j) f(j, d[j * THREADS], i[j * THREADS]);
    }
};

// ------------------------------------------------------------------ search
struct Search {
    const double *sx, *sy;                                        // the points bin by bin, in pixel space
    const int32_t *sidx;
    const uint32_t *start;                                        // [n_bins + 1]
    const double *values;                                         // [n_points], by index; null without `out`
    uint32_t n_points;
    Grid g;
    uint32_t tiles_x;
    int k, power, min_points, f32;
    double max_d2;                                                // +inf without a radius
    double fill;
    void *out;                                                    // float64 or float32 [rows][cols], or null
    int32_t *nidx;                                                // [k][rows][cols] or null
    double *nd2;
};

template <int K, bool LDS, int THREADS>
__global__ void __launch_bounds__(THREADS) search_kernel(const Search a) {
    constexpr int TILE_H = THREADS / TILE_W, RUN_ROWS = THREADS / 2;
    typedef hipcub::BlockScan<uint32_t, THREADS> Scan;
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ uint32_t run_first[THREADS], run_off[THREADS + 1];
    __shared__ double st_x[THREADS], st_y[THREADS];
    __shared__ int st_i[THREADS];
    __shared__ double list_d[LDS ? K : 1][THREADS];
    __shared__ int list_i[LDS ? K : 1][THREADS];

    const Grid &g = a.g;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const uint32_t tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const uint64_t x0 = (uint64_t)tx * TILE_W, y0 = (uint64_t)ty * TILE_H;
    const uint64_t ix = x0 + (wave & 1) * 8 + (lane & 7), iy = y0 + (wave >> 1) * 8 + (lane >> 3);
    const bool cell = ix < g.cols && iy < g.rows;
    const double cx = (double)ix + 0.5, cy = (double)iy + 0.5;
    const double B = (double)(1ull << g.shift);

    typename std::conditional<LDS, LdsList<K, THREADS>, RegList<K>>::type L;
    if constexpr (LDS) L.d = &list_d[0][t], L.i = &list_i[0][t];
    L.init(a.k);

    // the tile's own bins, in grid coordinates (the apron is column 0 and gx - 1, row 0 and gy - 1)
    const uint64_t x1 = x0 + TILE_W < g.cols ? x0 + TILE_W : g.cols, y1 = y0 + TILE_H < g.rows ? y0 + TILE_H : g.rows;
    const int64_t own_xl = (int64_t)(x0 >> g.shift) + 1, own_xh = (int64_t)((x1 - 1) >> g.shift) + 1;
    const int64_t own_yl = (int64_t)(y0 >> g.shift) + 1, own_yh = (int64_t)((y1 - 1) >> g.shift) + 1;
    const int64_t gx = g.gx, gy = g.gy;

    // Rings without a point are skipped in one step.  The points of rectangle r: per bin row one difference of bin starts, the
    // rows dealt to the threads, summed over the workgroup (the same value in every thread).
    auto reach = [&](int64_t r, int64_t &xl, int64_t &xh, int64_t &yl, int64_t &yh) {
        xl = own_xl - r > 0 ? own_xl - r : 0, xh = own_xh + r < gx - 1 ? own_xh + r : gx - 1;
        yl = own_yl - r > 0 ? own_yl - r : 0, yh = own_yh + r < gy - 1 ? own_yh + r : gy - 1;
        return xl == 0 && xh == gx - 1 && yl == 0 && yh == gy - 1;
    };
    auto points_within = [&](int64_t r) {
        int64_t xl, xh, yl, yh;
        reach(r, xl, xh, yl, yh);
        uint32_t mine = 0;
        for (int64_t by = yl + t; by <= yh; by += THREADS) {
            const size_t base = (size_t)by * (size_t)gx;
            const uint32_t s = a.start[base + xl], e = a.start[base + xh + 1];
            mine += e > s ? e - s : 0;
        }
        uint32_t off, total;
        Scan(scan_tmp).ExclusiveSum(mine, off, total);
        __syncthreads();
        return total;
    };
    // the largest rectangle known to be empty is r_first - 1: doubling, then bisection; an empty ring stages nothing and ends no
    // thread that a later ring would not end with the same list, so starting behind them changes no result
    int64_t r_first = 0;
    if (points_within(0) == 0) {
        int64_t lo = 0, hi = 1, xl, xh, yl, yh;
        while (!reach(hi, xl, xh, yl, yh) && points_within(hi) == 0) lo = hi, hi *= 2;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (points_within(mid) == 0) lo = mid;
            else hi = mid;
        }
        r_first = hi;
    }

    bool done = !cell;
    int64_t pxl = 1, pxh = 0, pyl = 1, pyh = 0;                   // the rectangle before this ring: none yet
    if (r_first > 0) reach(r_first - 1, pxl, pxh, pyl, pyh);
    for (int64_t r = r_first;; ++r) {
        const int64_t xl = own_xl - r > 0 ? own_xl - r : 0, xh = own_xh + r < gx - 1 ? own_xh + r : gx - 1;
        const int64_t yl = own_yl - r > 0 ? own_yl - r : 0, yh = own_yh + r < gy - 1 ? own_yh + r : gy - 1;
        const int64_t n_rows = yh - yl + 1;
        for (int64_t row0 = 0; row0 < n_rows; row0 += RUN_ROWS) {
            // thread t lists run t of this batch: side t & 1 of bin row row0 + t / 2
            const int64_t by = yl + row0 + (t >> 1);
            uint32_t first = 0, len = 0;
            if (by <= yh) {
                int64_t ba, bb;                                   // bins ba .. bb of the row are new in this ring
                if (by < pyl || by > pyh) {
                    ba = xl, bb = (t & 1) ? xl - 1 : xh;
                } else if (t & 1) {
                    ba = pxh + 1, bb = xh;
                } else {
                    ba = xl, bb = pxl - 1;
                }
                if (ba <= bb) {
                    const size_t base = (size_t)by * (size_t)gx;
                    uint32_t s = a.start[base + ba], e = a.start[base + bb + 1];
                    if (e > a.n_points) e = a.n_points;           // (a workspace of other points: stay inside the arrays)
                    if (s > e) s = e;
                    first = s, len = e - s;
                }
            }
            uint32_t off, total;
            Scan(scan_tmp).ExclusiveSum(len, off, total);
            run_first[t] = first, run_off[t] = off;
            if (t == 0) run_off[THREADS] = total;
            __syncthreads();
            for (uint32_t c = 0; c < total; c += THREADS) {
                const uint32_t item = c + t;
                if (item < total) {
                    int lo = 0, hi = THREADS;                     // the last run with run_off <= item: 8 or 7 steps
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (run_off[mid] <= item) lo = mid;
                        else hi = mid;
                    }
                    const uint32_t p = run_first[lo] + (item - run_off[lo]);
                    st_x[t] = a.sx[p], st_y[t] = a.sy[p], st_i[t] = a.sidx[p];
                }
                __syncthreads();
                if (!done) {
                    const int cnt = total - c < (uint32_t)THREADS ? (int)(total - c) : THREADS;
                    for (int j = 0; j < cnt; ++j) {
                        const double dx = st_x[j] - cx, dy = st_y[j] - cy;
                        const double xx = dx * dx, yy = dy * dy;
                        const double d2 = xx + yy;
                        const int pi = st_i[j];
                        if (before(d2, pi, L.kth_d(), L.kth_i()) && d2 <= a.max_d2) L.insert(d2, pi);
                    }
                }
                __syncthreads();
            }
            __syncthreads();                                      // the run list is free for the next batch
        }
        const bool whole = xl == 0 && xh == gx - 1 && yl == 0 && yh == gy - 1;
        if (!done) {
            double bound = INFINITY;
            if (xl > 0) bound = fmin(bound, cx - (double)(xl - 1) * B);
            if (xh < gx - 1) bound = fmin(bound, (double)xh * B - cx);
            if (yl > 0) bound = fmin(bound, cy - (double)(yl - 1) * B);
            if (yh < gy - 1) bound = fmin(bound, (double)yh * B - cy);
            const double b2 = bound * bound;
            done = (L.kth_i() != NONE && L.kth_d() < b2) || a.max_d2 < b2;
        }
        if (__syncthreads_and(done) || whole) break;
        pxl = xl, pxh = xh, pyl = yl, pyh = yh;
    }
    if (!cell) return;

    // weights and sums in rank order, and the neighbour planes
    const size_t plane = (size_t)g.rows * g.cols, at = (size_t)iy * g.cols + ix;
    double num = 0.0, den = 0.0, first_d2 = INFINITY, first_v = 0.0;
    int found = 0;
    L.each(a.k, [&](int rank, double d2, int pi) {
        const bool real = pi != NONE;
        if (a.nidx) a.nidx[(size_t)rank * plane + at] = real ? pi : -1;
        if (a.nd2) a.nd2[(size_t)rank * plane + at] = real ? d2 : INFINITY;
        if (real && a.out) {
            const double v = (uint32_t)pi < a.n_points ? a.values[pi] : 0.0;
            const double w = weight_of(d2, a.power);
            const double wv = w * v;
            num = num + wv;
            den = den + w;
            if (rank == 0) first_d2 = d2, first_v = v;
        }
        found += real;
    });
    if (!a.out) return;
    double res;
    if (found < a.min_points) res = a.fill;
    else if (first_d2 == 0.0) res = first_v;
    else res = num / den;
    if (a.f32) ((float *)a.out)[at] = (float)res;
    else ((double *)a.out)[at] = res;
}

// ------------------------------------------------------------------ workspace
struct Work {
    double *sx, *sy;                                              // [n_points]
    int32_t *sidx;
    uint32_t *start, *count;                                      // [n_bins + 1]
    uint32_t *flags;
    void *cub;
    size_t cub_bytes, total;
};

Work carve(void *base, uint64_t n_points, uint64_t n_bins) {
    Carver c(base);
    Work p{};
    p.sx = c.take<double>(n_points);
    p.sy = c.take<double>(n_points);
    p.sidx = c.take<int32_t>(n_points);
    p.start = c.take<uint32_t>(n_bins + 1);
    p.count = c.take<uint32_t>(n_bins + 1);
    p.flags = c.take<uint32_t>(64);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, p.cub_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)(n_bins + 1));
    p.cub = c.take<char>(p.cub_bytes > 0 ? p.cub_bytes : 1);
    p.total = c.at();
    return p;
}

int grid_of(const char *fn, uint64_t n_points, int64_t rows, int64_t cols, int64_t bin_cells, Grid &g) {
    if (rows < 1 || cols < 1) return fail("%s: the raster must have a shape of at least (1, 1)", fn);
    if ((uint64_t)rows > 0xFFFFFFFFull / (uint64_t)cols)
        return fail("%s: %lld x %lld cells exceed the 32-bit cell index (at most 2^32 - 1 cells)", fn, (long long)rows,
                    (long long)cols);
    if (n_points > XRS_IDW_MAX_POINTS)
        return fail("%s: %llu points, more than %llu", fn, (unsigned long long)n_points, (unsigned long long)XRS_IDW_MAX_POINTS);
    if (bin_cells < 1 || bin_cells > (1ll << 32) || (bin_cells & (bin_cells - 1)))
        return fail("%s: bin_cells %lld is not a power of two of 1 .. 2^32", fn, (long long)bin_cells);
    g.rows = (uint32_t)rows, g.cols = (uint32_t)cols;
    g.shift = 0;
    while ((1ll << g.shift) < bin_cells) ++g.shift;
    g.nbx = (uint32_t)(((uint64_t)cols - 1) >> g.shift) + 1, g.nby = (uint32_t)(((uint64_t)rows - 1) >> g.shift) + 1;
    g.gx = g.nbx + 2, g.gy = g.nby + 2;
    g.n_bins = (uint64_t)g.gx * g.gy;
    if (g.n_bins > XRS_IDW_MAX_BINS)
        return fail("%s: bins of %lld cells make %llu bins, more than %llu; use larger bins", fn, (long long)bin_cells,
                    (unsigned long long)g.n_bins, (unsigned long long)XRS_IDW_MAX_BINS);
    return 0;
}

template <int K, bool LDS, int THREADS>
void launch_search(const Search &a, hipStream_t s) {
    Search b = a;
    constexpr int TILE_H = THREADS / TILE_W;
    b.tiles_x = (a.g.cols + TILE_W - 1) / TILE_W;
    const uint64_t tiles = (uint64_t)b.tiles_x * ((a.g.rows + TILE_H - 1) / TILE_H);   // at most 2^32 / 128 + 2^29
    hipLaunchKernelGGL((search_kernel<K, LDS, THREADS>), dim3((unsigned)tiles), dim3(THREADS), 0, s, b);
}

}  // namespace

extern "C" {

int xrs_idw_workspace_size(uint64_t n_points, int64_t rows, int64_t cols, int64_t bin_cells, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_idw_workspace_size: null pointer");
    *bytes_out = 0;
    Grid g{};
    if (int rc = grid_of("xrs_idw_workspace_size", n_points, rows, cols, bin_cells, g)) return rc;
    *bytes_out = carve(nullptr, n_points, g.n_bins).total;
    return 0;
}

int xrs_idw_bin(const double *points_dev, uint64_t n_points, int64_t rows, int64_t cols, int64_t bin_cells,
                const double *inverse_host, void *work_dev, int *flags, void *stream) {
    Grid g{};
    if (int rc = grid_of("xrs_idw_bin", n_points, rows, cols, bin_cells, g)) return rc;
    if ((n_points && !points_dev) || !work_dev || !flags) return fail("xrs_idw_bin: null pointer");
    *flags = 0;
    hipStream_t s = as_stream(stream);
    const Work p = carve(work_dev, n_points, g.n_bins);
    Inverse m{};
    if (inverse_host) {
        m.a0 = inverse_host[0], m.a1 = inverse_host[1], m.a2 = inverse_host[2], m.a3 = inverse_host[3];
        m.t2 = inverse_host[4], m.t5 = inverse_host[5];
        m.on = 1;
    }
    XRS_HIP(hipMemsetAsync(p.count, 0, (size_t)(g.n_bins + 1) * 4, s));
    XRS_HIP(hipMemsetAsync(p.flags, 0, 256, s));
    const unsigned blocks = (unsigned)((n_points + BIN_THREADS - 1) / BIN_THREADS);
    if (n_points) {
        hipLaunchKernelGGL(hist_kernel, dim3(blocks), dim3(BIN_THREADS), 0, s, points_dev, (uint32_t)n_points, m, g, p.count, p.flags);
        XRS_LAUNCH_CHECK();
    }
    size_t cub_bytes = p.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(p.cub, cub_bytes, p.count, p.start, (size_t)(g.n_bins + 1), s));
    if (n_points) {
        hipLaunchKernelGGL(scatter_kernel, dim3(blocks), dim3(BIN_THREADS), 0, s, points_dev, (uint32_t)n_points, m, g,
                           (const uint32_t *)p.start, p.count, p.sx, p.sy, p.sidx);
        XRS_LAUNCH_CHECK();
    }
    uint32_t flag_word = 0;
    XRS_HIP(hipMemcpyAsync(&flag_word, p.flags, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    *flags = (int)flag_word;
    return 0;
}

int xrs_idw_search(const void *work_dev, const double *values_dev, uint64_t n_points, int64_t rows, int64_t cols,
                   int64_t bin_cells, int k, int power, double max_d2, int min_points, double fill, int dtype, void *out_dev,
                   int32_t *index_dev, double *d2_dev, void *stream) {
    Grid g{};
    if (int rc = grid_of("xrs_idw_search", n_points, rows, cols, bin_cells, g)) return rc;
    if (k < 1 || k > XRS_IDW_MAX_K) return fail("xrs_idw_search: k %d outside 1 .. %d", k, XRS_IDW_MAX_K);
    if (power < 1 || power > 8) return fail("xrs_idw_search: power %d outside 1 .. 8", power);
    if (min_points < 1 || min_points > k) return fail("xrs_idw_search: min_points %d outside 1 .. k = %d", min_points, k);
    if (max_d2 != max_d2) return fail("xrs_idw_search: max_d2 is NaN (pass a negative number for no radius)");
    if (out_dev && dtype != XRS_DT_F64 && dtype != XRS_DT_F32)
        return fail("xrs_idw_search: dtype code %d is neither XRS_DT_F64 nor XRS_DT_F32", dtype);
    if (!work_dev || (!out_dev && !index_dev && !d2_dev) || (out_dev && n_points && !values_dev))
        return fail("xrs_idw_search: null pointer");
    const Work p = carve((void *)work_dev, n_points, g.n_bins);
    Search a{};
    a.sx = p.sx, a.sy = p.sy, a.sidx = p.sidx, a.start = p.start, a.values = values_dev;
    a.n_points = (uint32_t)n_points, a.g = g;
    a.k = k, a.power = power, a.min_points = min_points, a.f32 = dtype == XRS_DT_F32;
    a.max_d2 = max_d2 < 0.0 ? INFINITY : max_d2, a.fill = fill;
    a.out = out_dev, a.nidx = index_dev, a.nd2 = d2_dev;
    hipStream_t s = as_stream(stream);
    if (k <= 1) launch_search<1, false, 256>(a, s);
    else if (k <= 4) launch_search<4, false, 256>(a, s);
    else if (k <= 8) launch_search<8, false, 256>(a, s);
    else if (k <= 16) launch_search<16, false, 256>(a, s);
    else if (k <= 32) launch_search<32, true, 256>(a, s);
    else launch_search<64, true, 128>(a, s);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

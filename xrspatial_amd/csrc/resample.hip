// resample: regrid a raster onto another axis-aligned grid.  The reference tree has no resample; the rule is written down in
// DESIGN.md §6u and restated in tests/resample_oracle.py.  ALL GEOMETRY IS IN TABLES the host computes in float64, one entry per
// destination row and one per destination column; the kernels below only load, compare, multiply, add and divide in a fixed
// order, so a NumPy statement of the rule equals them bit for bit.
//
//   near      int32 [n_dst]: the source row (column) a destination row (column) falls into, -1 for none;
//   first, w  int32 [n_dst], float64 [n_dst][taps]: tap k of destination row i is source row first[i] + k with weight w[i][k].
//             A tap PARTICIPATES when its weight is not 0.  A tap that does not participate, or whose index lies outside the
//             raster, is never read (tile_kernel, which walks its taps without a branch, loads cell 0 of the row in its place
//             and drops the value): that is the rim rule, and it is also what keeps every load inside the source plane
//             whatever the tables hold.
//   valid     a source cell inside the raster that is not NaN and not equal to `nodata`.
//
//   gather    out = src[near_y][near_x], or fill where either index is -1 (or outside) or that cell is invalid.
//   weighted  per tap row j with wy[j] != 0, ascending:  r_j = sum wx[i] * v and n_j = sum wx[i] over the row's participating
//             valid taps, ascending, each product and each sum rounded on its own; a sum begins with its first term (so a
//             single -0.0 stays -0.0) and is +0.0 without one;  num = sum wy[j] * r_j and den = sum wy[j] * n_j the same way,
//             over every row with wy[j] != 0, a row without a valid tap included.  The cell is num / den (or num).  With
//             `near` tables the cell is fill exactly where gather's would be, without them where no valid tap participates.
//             With fallback tables, a cell whose window holds a participating invalid tap is computed from those instead.
//   select    min, max or mode over the participating valid cells of the window, row-major; fill where there are none.  min and
//             max keep the first of equals; mode is the class (by ==) with the most members, the smaller value on a tie,
//             reported as its first member.
//
// weighted has two kernels.  Up to TILE_TAPS taps on both axes, tile_kernel: one workgroup per tile of 32 x 8 destination
// cells reduces every source row the tile's tap rows span horizontally into LDS, once per (source row, destination column),
// as r, n and the counts of valid and invalid participating taps, then every thread combines its cell's tap rows from LDS:
// taps_x + taps_y multiplies per cell, in exactly the written order.  A tile whose tap rows span more source rows than its
// LDS holds (64, or 32 for the interpolation methods and short windows: twice the workgroups per CU) -- a steep scale, tables
// that are not monotone -- walks its cells directly instead, with the same operations in the same order.  Above TILE_TAPS,
// wave_kernel: one wave per destination cell, a lane per tap row, the row terms summed in ascending order by lane 0.
// Cells that need the fallback tables are recomputed directly by their own thread.
//
// Every loop is bounded, no workgroup waits for another, and every store is an ordinary vector store.
#include "dtype_dispatch.h"

#include <type_traits>

// no fused multiply-add anywhere below: the rule's products and sums are rounded one by one
#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = 32, TILE_H = 8;                            // destination cells of a tile: one per thread
constexpr int TILE_TAPS = 8;                                      // tile_kernel: at most this many taps per axis
constexpr int TILE_ROWS = 64, TILE_ROWS_SMALL = 32;               // source rows a tile can hold in LDS, two sizes
constexpr int MODE_SMALL = 64;                                    // mode: windows up to this many cells take 16 lanes per cell

struct Source {
    const void *p;
    int64_t rows, cols;
    uint64_t nodata_bits;                                         // one item of the raster's dtype
    int has_nodata;
};

struct Axis {                                                     // one axis of a tap table
    const int32_t *first;
    const double *w;
    int taps;
};

struct Weighted {
    Source src;
    uint32_t rows, cols, tiles_x;
    Axis y, x, fy, fx;                                            // fy / fx: the fallback tables, first == null for none
    const int32_t *near_y, *near_x;                               // null for none
    int divide, f32;
    double fill;
    void *out;
};

struct Gather {
    Source src;
    uint32_t rows, cols;
    const int32_t *near_y, *near_x;
    uint64_t fill_bits;
    void *out;
};

struct Select {
    Source src;
    uint32_t rows, cols;
    Axis y, x;
    int op;
    uint64_t fill_bits;
    void *out;
};

template <typename T>
__device__ __forceinline__ T item_of(uint64_t bits) {
    T v;
    __builtin_memcpy(&v, &bits, sizeof(T));
    return v;
}

// is the cell (sy, sx) inside the raster and valid?  Reads it only when it is inside.
template <typename T>
__device__ __forceinline__ bool take(const Source &s, int64_t sy, int64_t sx, T &v) {
    if (sy < 0 || sy >= s.rows || sx < 0 || sx >= s.cols) return false;
    v = static_cast<const T *>(s.p)[sy * s.cols + sx];
    if constexpr (std::is_floating_point<T>::value) {
        if (v != v) return false;
    }
    return !(s.has_nodata && v == item_of<T>(s.nodata_bits));
}

// ------------------------------------------------------------------ weighted: one cell, walked directly
// num, den and the counts of valid (good) and invalid (bad) participating taps of cell (row, col) from the tables (ay, ax)
template <typename T>
__device__ __forceinline__ void walk_cell(const Source &s, const Axis &ay, const Axis &ax, uint32_t row, uint32_t col,
                                          double &num, double &den, uint32_t &good, uint32_t &bad) {
    const int64_t y0 = ay.first[row], x0 = ax.first[col];
    const double *wy = ay.w + (size_t)row * ay.taps, *wx = ax.w + (size_t)col * ax.taps;
    num = 0.0, den = 0.0, good = 0, bad = 0;
    bool any = false;
    for (int j = 0; j < ay.taps; ++j) {
        const double wj = wy[j];
        if (wj == 0.0) continue;
        double r = 0.0, n = 0.0;
        bool some = false;
        for (int i = 0; i < ax.taps; ++i) {
            const double wi = wx[i];
            if (wi == 0.0) continue;
            T v;
            const bool ok = take<T>(s, y0 + j, x0 + i, v);
            good += ok, bad += !ok;
            if (ok) {
                const double p = wi * (double)v;
                r = some ? r + p : p;
                n = some ? n + wi : wi;
                some = true;
            }
        }
        const double pr = wj * r, pn = wj * n;
        num = any ? num + pr : pr;
        den = any ? den + pn : pn;
        any = true;
    }
}

// what the sums of a cell become: fill, the fallback rule, or num / den; one rounding to the output's dtype
// is this value valid (its cell is known to be inside the raster)?
template <typename T>
__device__ __forceinline__ bool valid_value(const Source &s, T v) {
    bool ok = true;
    if constexpr (std::is_floating_point<T>::value) ok = v == v;
    return ok && !(s.has_nodata && v == item_of<T>(s.nodata_bits));
}

// what the sums of a cell become: fill, the fallback rule, or num / den; one rounding to the output's dtype.  `near_fill`:
// what the near tables say, where there are any.
template <typename T>
__device__ __forceinline__ void finish_cell(const Weighted &a, uint32_t row, uint32_t col, double num, double den, uint32_t good,
                                            uint32_t bad, bool near_fill) {
    bool fill = a.near_y ? near_fill : good == 0;
    if (!fill && a.fy.first && bad) {
        walk_cell<T>(a.src, a.fy, a.fx, row, col, num, den, good, bad);
        if (!a.near_y) fill = good == 0;
    }
    const double res = fill ? a.fill : (a.divide ? num / den : num);
    const size_t at = (size_t)row * a.cols + col;
    if (a.f32) ((float *)a.out)[at] = (float)res;
    else ((double *)a.out)[at] = res;
}

template <typename T>
__device__ __forceinline__ void settle_cell(const Weighted &a, uint32_t row, uint32_t col, double num, double den, uint32_t good,
                                            uint32_t bad) {
    bool near_fill = false;
    if (a.near_y) {
        T v;
        near_fill = !take<T>(a.src, a.near_y[row], a.near_x[col], v);
    }
    finish_cell<T>(a, row, col, num, den, good, bad, near_fill);
}

// ROWS: the source rows a tile can hold in LDS.  Everything a thread needs from the tables is fetched before the source is,
// and the taps are walked without a branch (a tap that is not read is a load of cell 0 of its row, or of the raster, whose value
// is dropped): two round trips to memory in front of the barrier, none behind it.
template <typename T, int ROWS>
__global__ void __launch_bounds__(THREADS) tile_kernel(const Weighted a) {
    __shared__ double s_r[ROWS][TILE_W], s_n[ROWS][TILE_W];
    __shared__ uint8_t s_c[ROWS][TILE_W];                         // good | bad << 4: at most 8 taps in a row

    const int t = threadIdx.x, lx = t & (TILE_W - 1), ly = t / TILE_W;
    const uint32_t tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const uint32_t col = tx * TILE_W + lx, row = ty * TILE_H + ly;
    const bool cell = col < a.cols && row < a.rows;
    const uint32_t colc = col < a.cols ? col : a.cols - 1, rowc = row < a.rows ? row : a.rows - 1;
    const T *src = static_cast<const T *>(a.src.p);

    // the source rows the tile's tap rows span (the same in every thread)
    int64_t lo = INT64_MAX, hi = INT64_MIN;
#pragma unroll
    for (int r = 0; r < TILE_H; ++r) {
        const uint32_t rr = ty * TILE_H + r;
        const int64_t f = a.y.first[rr < a.rows ? rr : a.rows - 1];
        lo = f < lo ? f : lo;
        hi = f + a.y.taps > hi ? f + a.y.taps : hi;
    }
    if (hi - lo > ROWS) {                                         // (tables that are not monotone, a steep scale) cell by cell
        if (cell) {
            double num, den;
            uint32_t good, bad;
            walk_cell<T>(a.src, a.y, a.x, row, col, num, den, good, bad);
            settle_cell<T>(a, row, col, num, den, good, bad);
        }
        return;
    }

    // the tables of this thread's column (horizontal) and of its cell (vertical, near)
    double wx[TILE_TAPS], wy[TILE_TAPS];
    const int64_t x0 = a.x.first[colc], y0 = a.y.first[rowc];
#pragma unroll
    for (int i = 0; i < TILE_TAPS; ++i) {
        wx[i] = i < a.x.taps ? a.x.w[(size_t)colc * a.x.taps + i] : 0.0;
        wy[i] = i < a.y.taps ? a.y.w[(size_t)rowc * a.y.taps + i] : 0.0;
    }
    bool near_fill = false;
    if (a.near_y) {
        const int64_t ny = a.near_y[rowc], nx = a.near_x[colc];
        const bool in = ny >= 0 && ny < a.src.rows && nx >= 0 && nx < a.src.cols;
        const T v = src[in ? ny * a.src.cols + nx : 0];
        near_fill = !(in && valid_value<T>(a.src, v));
    }

    // horizontal: thread t takes column lx of source rows ly, ly + 8, ...
    const int n_rows = (int)(hi - lo);
    for (int r = ly; r < n_rows; r += TILE_H) {
        const int64_t sy = lo + r;
        const bool row_in = sy >= 0 && sy < a.src.rows;
        const T *line = src + (row_in ? sy : 0) * a.src.cols;
        T v[TILE_TAPS];
        bool in[TILE_TAPS];
#pragma unroll
        for (int i = 0; i < TILE_TAPS; ++i) {
            const int64_t sx = x0 + i;
            in[i] = i < a.x.taps && row_in && sx >= 0 && sx < a.src.cols;
            v[i] = i < a.x.taps ? line[in[i] ? sx : 0] : T(0);
        }
        double acc = 0.0, n = 0.0;
        uint32_t good = 0, bad = 0;
#pragma unroll
        for (int i = 0; i < TILE_TAPS; ++i) {
            if (i < a.x.taps) {                                   // (the same in every thread: no work behind the last tap)
                const bool part = wx[i] != 0.0;
                const bool ok = part && in[i] && valid_value<T>(a.src, v[i]);
                const double p = wx[i] * (double)v[i];
                const double acc1 = good ? acc + p : p, n1 = good ? n + wx[i] : wx[i];
                acc = ok ? acc1 : acc;
                n = ok ? n1 : n;
                good += ok, bad += part && !ok;
            }
        }
        s_r[r][lx] = acc, s_n[r][lx] = n, s_c[r][lx] = (uint8_t)(good | (bad << 4));
    }
    __syncthreads();
    if (!cell) return;

    // vertical: the cell's tap rows, ascending
    double num = 0.0, den = 0.0;
    uint32_t good = 0, bad = 0;
    bool any = false;
#pragma unroll
    for (int j = 0; j < TILE_TAPS; ++j) {
        if (j < a.y.taps) {                                       // (the same in every thread)
            const bool part = wy[j] != 0.0;
            const int slot = part ? (int)(y0 + j - lo) : 0;       // 0 .. n_rows - 1: lo and hi are over this row too
            const double pr = wy[j] * s_r[slot][lx], pn = wy[j] * s_n[slot][lx];
            const double num1 = any ? num + pr : pr, den1 = any ? den + pn : pn;
            num = part ? num1 : num;
            den = part ? den1 : den;
            const uint32_t c = part ? s_c[slot][lx] : 0;
            good += c & 15u, bad += c >> 4;
            any = any || part;
        }
    }
    finish_cell<T>(a, row, col, num, den, good, bad, near_fill);
}

// one wave per destination cell, lane l on tap rows l, l + 64, ...; at most XRS_RESAMPLE_MAX_TAPS of them
template <typename T>
__global__ void __launch_bounds__(THREADS) wave_kernel(const Weighted a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ double s_num[WAVES][XRS_RESAMPLE_MAX_TAPS], s_den[WAVES][XRS_RESAMPLE_MAX_TAPS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t id = (uint64_t)blockIdx.x * WAVES + wave;
    const bool cell = id < (uint64_t)a.rows * a.cols;             // wave-uniform
    const uint32_t row = cell ? (uint32_t)id / a.cols : 0, col = cell ? (uint32_t)id % a.cols : 0;
    uint32_t good = 0, bad = 0;
    if (cell) {
        const int64_t y0 = a.y.first[row], x0 = a.x.first[col];
        const double *wy = a.y.w + (size_t)row * a.y.taps, *wx = a.x.w + (size_t)col * a.x.taps;
        for (int j = lane; j < a.y.taps; j += 64) {
            const double wj = wy[j];
            double r = 0.0, n = 0.0;
            bool some = false;
            if (wj != 0.0) {
                for (int i = 0; i < a.x.taps; ++i) {
                    const double wi = wx[i];
                    if (wi == 0.0) continue;
                    T v;
                    const bool ok = take<T>(a.src, y0 + j, x0 + i, v);
                    good += ok, bad += !ok;
                    if (ok) {
                        const double p = wi * (double)v;
                        r = some ? r + p : p;
                        n = some ? n + wi : wi;
                        some = true;
                    }
                }
            }
            s_num[wave][j] = wj * r;                              // (not read for a row that does not participate)
            s_den[wave][j] = wj * n;
        }
    }
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) good += __shfl_xor(good, off), bad += __shfl_xor(bad, off);
    if (!cell || lane != 0) return;
    const double *wy = a.y.w + (size_t)row * a.y.taps;
    double num = 0.0, den = 0.0;
    bool any = false;
    for (int j = 0; j < a.y.taps; ++j) {
        if (wy[j] == 0.0) continue;
        num = any ? num + s_num[wave][j] : s_num[wave][j];
        den = any ? den + s_den[wave][j] : s_den[wave][j];
        any = true;
    }
    settle_cell<T>(a, row, col, num, den, good, bad);
}

// ------------------------------------------------------------------ gather
// a thread takes 16 bytes of one destination row: one division per thread, and one store where the row allows it
template <typename T>
__global__ void __launch_bounds__(THREADS) gather_kernel(const Gather a, uint32_t chunks_x) {
    constexpr int K = 16 / (int)sizeof(T);
    struct alignas(16) Pack { T v[K]; };
    const uint64_t id = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (id >= (uint64_t)chunks_x * a.rows) return;
    const uint32_t row = (uint32_t)(id / chunks_x), col0 = (uint32_t)(id % chunks_x) * K;
    const int64_t ny = a.near_y[row];
    const bool row_in = ny >= 0 && ny < a.src.rows;
    const T *line = static_cast<const T *>(a.src.p) + (row_in ? ny : 0) * a.src.cols;
    const T fill = item_of<T>(a.fill_bits);
    const uint32_t n = a.cols - col0 < (uint32_t)K ? a.cols - col0 : (uint32_t)K;
    Pack out;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t nx = a.near_x[col0 + ((uint32_t)k < n ? k : 0)];
        const bool in = row_in && nx >= 0 && nx < a.src.cols;
        const T v = line[in ? nx : 0];
        out.v[k] = in && valid_value<T>(a.src, v) ? v : fill;
    }
    T *dst = static_cast<T *>(a.out) + (size_t)row * a.cols + col0;
    if (n == (uint32_t)K && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        *reinterpret_cast<Pack *>(dst) = out;
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((uint32_t)k < n) dst[k] = out.v[k];
    }
}

// ------------------------------------------------------------------ select: min and max, one thread per cell
template <typename T>
__global__ void __launch_bounds__(THREADS) minmax_kernel(const Select a) {
    const uint64_t id = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (id >= (uint64_t)a.rows * a.cols) return;
    const uint32_t row = (uint32_t)id / a.cols, col = (uint32_t)id % a.cols;
    const int64_t y0 = a.y.first[row], x0 = a.x.first[col];
    const double *wy = a.y.w + (size_t)row * a.y.taps, *wx = a.x.w + (size_t)col * a.x.taps;
    T best = item_of<T>(a.fill_bits);
    bool any = false;
    for (int j = 0; j < a.y.taps; ++j) {
        if (wy[j] == 0.0) continue;
        for (int i = 0; i < a.x.taps; ++i) {
            if (wx[i] == 0.0) continue;
            T v;
            if (!take<T>(a.src, y0 + j, x0 + i, v)) continue;
            if (!any || (a.op == XRS_RESAMPLE_MIN ? v < best : v > best)) best = v;
            any = true;
        }
    }
    static_cast<T *>(a.out)[id] = best;
}

// ------------------------------------------------------------------ select: mode, G lanes per cell
// The window goes to LDS in row-major order, lane l of the group loading cells l, l + G, .., with a flag for the valid
// participating ones; then lane l counts, for elements l, l + G, .., the members of their class and finds its first member; the
// best (count, smaller value) of the group wins.
template <typename T, int G, int CAP>
__global__ void __launch_bounds__(THREADS) mode_kernel(const Select a) {
    constexpr int GROUPS = THREADS / G;
    __shared__ T s_v[GROUPS][CAP];
    __shared__ uint8_t s_ok[GROUPS][CAP];
    const int g = threadIdx.x / G, lane = threadIdx.x % G;
    const uint64_t id = (uint64_t)blockIdx.x * GROUPS + g;
    const bool cell = id < (uint64_t)a.rows * a.cols;
    const uint32_t row = cell ? (uint32_t)id / a.cols : 0, col = cell ? (uint32_t)id % a.cols : 0;
    const uint32_t window = (uint32_t)(a.y.taps * a.x.taps);     // at most CAP: the host chose the kernel by it
    const int64_t y0 = a.y.first[row], x0 = a.x.first[col];
    const double *wy = a.y.w + (size_t)row * a.y.taps, *wx = a.x.w + (size_t)col * a.x.taps;
    for (uint32_t e = lane; e < window; e += G) {
        const uint32_t j = e / (uint32_t)a.x.taps, i = e % (uint32_t)a.x.taps;
        T v = T(0);
        const bool ok = cell && wy[j] != 0.0 && wx[i] != 0.0 && take<T>(a.src, y0 + j, x0 + i, v);
        s_v[g][e] = v, s_ok[g][e] = ok;
    }
    __syncthreads();
    uint32_t best_count = 0;
    T best = item_of<T>(a.fill_bits);
    for (uint32_t e = lane; e < window; e += G) {
        if (!s_ok[g][e]) continue;
        const T v = s_v[g][e];
        uint32_t count = 0, head = e;
        for (uint32_t k = 0; k < window; ++k) {
            const bool same = s_ok[g][k] && s_v[g][k] == v;
            count += same;
            if (same && k < head) head = k;
        }
        const T rep = s_v[g][head];
        if (count > best_count || (count == best_count && rep < best)) best_count = count, best = rep;
    }
    for (int off = G / 2; off > 0; off >>= 1) {
        const uint32_t oc = __shfl_xor(best_count, off);
        uint64_t bits = 0;
        __builtin_memcpy(&bits, &best, sizeof(T));
        const uint32_t hi = __shfl_xor((uint32_t)(bits >> 32), off), lo = __shfl_xor((uint32_t)bits, off);
        const T ov = item_of<T>(((uint64_t)hi << 32) | lo);
        if (oc > best_count || (oc == best_count && oc > 0 && ov < best)) best_count = oc, best = ov;
    }
    if (cell && lane == 0) static_cast<T *>(a.out)[id] = best;
}

// ------------------------------------------------------------------ argument checks
int check_source(const char *fn, const void *src, int dtype, int64_t src_rows, int64_t src_cols, const void *nodata_host,
                 int64_t rows, int64_t cols, const void *out, Source &s) {
    if (!dtype_bytes(dtype)) return fail("%s: dtype code %d is not an XRS_DT_* code", fn, dtype);
    if (src_rows < 1 || src_cols < 1 || rows < 1 || cols < 1) return fail("%s: both rasters must have a shape of at least (1, 1)", fn);
    if ((uint64_t)src_rows > 0xFFFFFFFFull / (uint64_t)src_cols || (uint64_t)rows > 0xFFFFFFFFull / (uint64_t)cols)
        return fail("%s: %lld x %lld or %lld x %lld cells exceed the 32-bit cell index (at most 2^32 - 1 cells)", fn,
                    (long long)src_rows, (long long)src_cols, (long long)rows, (long long)cols);
    if (src_rows > INT32_MAX || src_cols > INT32_MAX)
        return fail("%s: a source axis of more than 2^31 - 1 cells does not fit the int32 tables", fn);
    if (!src || !out) return fail("%s: null pointer", fn);
    s.p = src, s.rows = src_rows, s.cols = src_cols, s.nodata_bits = 0, s.has_nodata = nodata_host != nullptr;
    if (nodata_host) memcpy(&s.nodata_bits, nodata_host, (size_t)dtype_bytes(dtype));
    return 0;
}

int check_axis(const char *fn, const char *name, const int32_t *first, const double *w, int taps, Axis &ax) {
    if (!first || !w) return fail("%s: null pointer (%s tables)", fn, name);
    if (taps < 1 || taps > XRS_RESAMPLE_MAX_TAPS)
        return fail("%s: %d taps on the %s axis, outside 1 .. %d", fn, taps, name, XRS_RESAMPLE_MAX_TAPS);
    ax.first = first, ax.w = w, ax.taps = taps;
    return 0;
}

}  // namespace

extern "C" {

int xrs_resample_gather(const void *src_dev, int dtype, int64_t src_rows, int64_t src_cols, const void *nodata_host, int64_t rows,
                        int64_t cols, const int32_t *near_y_dev, const int32_t *near_x_dev, const void *fill_host, void *out_dev,
                        void *stream) {
    Gather a{};
    if (int rc = check_source("xrs_resample_gather", src_dev, dtype, src_rows, src_cols, nodata_host, rows, cols, out_dev, a.src))
        return rc;
    if (!near_y_dev || !near_x_dev || !fill_host) return fail("xrs_resample_gather: null pointer");
    a.rows = (uint32_t)rows, a.cols = (uint32_t)cols, a.near_y = near_y_dev, a.near_x = near_x_dev, a.out = out_dev;
    memcpy(&a.fill_bits, fill_host, (size_t)dtype_bytes(dtype));
    with_dtype(dtype, [&](auto t) {
        using T = dtype_of<decltype(t)>;
        constexpr uint32_t K = 16 / sizeof(T);
        const uint32_t chunks_x = (a.cols + K - 1) / K;
        const unsigned blocks = (unsigned)(((uint64_t)chunks_x * a.rows + THREADS - 1) / THREADS);
        hipLaunchKernelGGL(gather_kernel<T>, dim3(blocks), dim3(THREADS), 0, as_stream(stream), a, chunks_x);
    });
    XRS_LAUNCH_CHECK();
    return 0;
}

int xrs_resample_weighted(const void *src_dev, int dtype, int64_t src_rows, int64_t src_cols, const void *nodata_host, int64_t rows,
                          int64_t cols, const int32_t *first_y_dev, const double *wy_dev, int taps_y, const int32_t *first_x_dev,
                          const double *wx_dev, int taps_x, const int32_t *near_y_dev, const int32_t *near_x_dev,
                          const int32_t *fb_first_y_dev, const double *fb_wy_dev, int fb_taps_y, const int32_t *fb_first_x_dev,
                          const double *fb_wx_dev, int fb_taps_x, int divide, int out_dtype, double fill, void *out_dev,
                          void *stream) {
    const char *fn = "xrs_resample_weighted";
    Weighted a{};
    if (int rc = check_source(fn, src_dev, dtype, src_rows, src_cols, nodata_host, rows, cols, out_dev, a.src)) return rc;
    if (out_dtype != XRS_DT_F64 && out_dtype != XRS_DT_F32)
        return fail("%s: output dtype code %d is neither XRS_DT_F64 nor XRS_DT_F32", fn, out_dtype);
    if (int rc = check_axis(fn, "y", first_y_dev, wy_dev, taps_y, a.y)) return rc;
    if (int rc = check_axis(fn, "x", first_x_dev, wx_dev, taps_x, a.x)) return rc;
    if ((near_y_dev == nullptr) != (near_x_dev == nullptr)) return fail("%s: near tables for one axis only", fn);
    if (fb_first_y_dev || fb_wy_dev || fb_first_x_dev || fb_wx_dev) {
        if (int rc = check_axis(fn, "fallback y", fb_first_y_dev, fb_wy_dev, fb_taps_y, a.fy)) return rc;
        if (int rc = check_axis(fn, "fallback x", fb_first_x_dev, fb_wx_dev, fb_taps_x, a.fx)) return rc;
    }
    a.rows = (uint32_t)rows, a.cols = (uint32_t)cols;
    a.near_y = near_y_dev, a.near_x = near_x_dev;
    a.divide = divide != 0, a.f32 = out_dtype == XRS_DT_F32, a.fill = fill, a.out = out_dev;
    hipStream_t s = as_stream(stream);
    if (taps_y <= TILE_TAPS && taps_x <= TILE_TAPS) {
        a.tiles_x = (a.cols + TILE_W - 1) / TILE_W;
        const uint64_t tiles = (uint64_t)a.tiles_x * ((a.rows + TILE_H - 1) / TILE_H);        // below 2^32 / 8 + 2^29
        // the interpolation methods (near tables) and short windows span few source rows per tile: half the LDS, twice the
        // workgroups per CU; a tile that spans more walks its cells directly, at most 8 x 8 taps each
        const bool few_rows = near_y_dev != nullptr || taps_y <= TILE_ROWS_SMALL / TILE_H;
        with_dtype(dtype, [&](auto t) {
            using T = dtype_of<decltype(t)>;
            if (few_rows) hipLaunchKernelGGL((tile_kernel<T, TILE_ROWS_SMALL>), dim3((unsigned)tiles), dim3(THREADS), 0, s, a);
            else hipLaunchKernelGGL((tile_kernel<T, TILE_ROWS>), dim3((unsigned)tiles), dim3(THREADS), 0, s, a);
        });
    } else {
        const uint64_t blocks = ((uint64_t)rows * cols + THREADS / 64 - 1) / (THREADS / 64);  // at most 2^30
        with_dtype(dtype, [&](auto t) {
            using T = dtype_of<decltype(t)>;
            hipLaunchKernelGGL(wave_kernel<T>, dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
        });
    }
    XRS_LAUNCH_CHECK();
    return 0;
}

int xrs_resample_select(const void *src_dev, int dtype, int64_t src_rows, int64_t src_cols, const void *nodata_host, int64_t rows,
                        int64_t cols, const int32_t *first_y_dev, const double *wy_dev, int taps_y, const int32_t *first_x_dev,
                        const double *wx_dev, int taps_x, int op, const void *fill_host, void *out_dev, void *stream) {
    const char *fn = "xrs_resample_select";
    Select a{};
    if (int rc = check_source(fn, src_dev, dtype, src_rows, src_cols, nodata_host, rows, cols, out_dev, a.src)) return rc;
    if (op != XRS_RESAMPLE_MIN && op != XRS_RESAMPLE_MAX && op != XRS_RESAMPLE_MODE) return fail("%s: unknown op %d", fn, op);
    if (int rc = check_axis(fn, "y", first_y_dev, wy_dev, taps_y, a.y)) return rc;
    if (int rc = check_axis(fn, "x", first_x_dev, wx_dev, taps_x, a.x)) return rc;
    if (!fill_host) return fail("%s: null pointer", fn);
    const int window = taps_y * taps_x;
    if (op == XRS_RESAMPLE_MODE && window > XRS_RESAMPLE_MODE_MAX_WINDOW)
        return fail("%s: a mode window of %d x %d cells, more than %d", fn, taps_y, taps_x, XRS_RESAMPLE_MODE_MAX_WINDOW);
    a.rows = (uint32_t)rows, a.cols = (uint32_t)cols, a.op = op, a.out = out_dev;
    memcpy(&a.fill_bits, fill_host, (size_t)dtype_bytes(dtype));
    hipStream_t s = as_stream(stream);
    const uint64_t cells = (uint64_t)rows * cols;
    with_dtype(dtype, [&](auto t) {
        using T = dtype_of<decltype(t)>;
        if (op != XRS_RESAMPLE_MODE) {
            hipLaunchKernelGGL(minmax_kernel<T>, dim3((unsigned)((cells + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a);
        } else if (window <= MODE_SMALL) {
            constexpr int GROUPS = THREADS / 16;
            hipLaunchKernelGGL((mode_kernel<T, 16, MODE_SMALL>), dim3((unsigned)((cells + GROUPS - 1) / GROUPS)), dim3(THREADS), 0, s, a);
        } else {
            constexpr int GROUPS = THREADS / 64;
            hipLaunchKernelGGL((mode_kernel<T, 64, XRS_RESAMPLE_MODE_MAX_WINDOW>), dim3((unsigned)((cells + GROUPS - 1) / GROUPS)),
                               dim3(THREADS), 0, s, a);
        }
    });
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

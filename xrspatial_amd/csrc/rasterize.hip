// rasterize: burn polygons into a raster.  The reference tree has no rasterize; the rule is written down in DESIGN.md §6r
// and restated in tests/rasterize_oracle.py.  It is the inverse of polygonize (§6h): pixel (row j, column i) is the square
// [i, i + 1] x [j, j + 1] and its centre is (i + 0.5, j + 0.5).
//
//   pixel space  u = a0 * dx + a1 * dy, v = a2 * dx + a3 * dy with dx = x - t2, dy = y - t5 and the inverse coefficients the
//                host worked out; every product and sum rounded on its own (no fused multiply-add);
//   edges        ring point k to the ring's next point, the last point to the first; an edge with v0 == v1 gives nothing;
//                every other edge is put in canonical order, the end with the smaller v first;
//   crossings    edge (u0, v0)-(u1, v1), v0 < v1, crosses row j iff v0 <= j + 0.5 < v1, 0 <= j < rows, at
//                ux = u0 + ((vc - v0) * (u1 - u0)) / (v1 - v0), vc = j + 0.5; its column is the first i with i + 0.5 >= ux,
//                clamped to [0, cols];
//   inside       cell (j, i) is inside polygon p iff the crossings of p in row j with column <= i are odd in number;
//   merge        a cell takes the covering polygon of the highest priority (the host turns `merge` into priorities).
//
// Four calls on one stream; the first two end in one small device-to-host read that sizes what the next one needs:
//   xrs_rasterize_census  census_kernel (one thread per ring point: its ring and polygon by binary search in the offsets, its
//                         edge, the rows the edge crosses) + ExclusiveSum (the crossing count C);
//   xrs_rasterize_spans   emit_kernel (one thread per crossing, its edge by binary search in the scanned counts), radix sort
//                         of (polygon, row, column) keys over the bits in use, pair_kernel (crossings 2k and 2k + 1 are the
//                         span [c0, c1); its 64-cell chunks) + ExclusiveSum (the work-item count);
//   xrs_rasterize_burn    burn_kernel (one wave per (span, chunk), one lane per cell: atomicMax of priority + 1, or
//                         atomicAdd of 1, on a uint32 plane where 0 is "uncovered");
//   xrs_rasterize_gather  gather_kernel (plane -> values[order[w - 1]] or fill, in the output's dtype).
// Every ring is closed, so every (polygon, row) holds an even number of crossings and a group starts at an even position of
// the sorted keys: the pairs are the global pairs (2k, 2k + 1), which pair_kernel checks.  Every loop is bounded (a binary
// search takes at most 32 steps), no workgroup waits for another, no thread's work grows with an edge's height or a span's
// width, and every store is an ordinary vector store or a vector atomic.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

using namespace xrs;

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr uint64_t BATCH = 1ull << 30;                            // threads of one launch
constexpr int CHUNK_SHIFT = 6;                                    // a work item covers 64 cells: one wave, 256 bytes
enum { FLAG_NONFINITE = XRS_RASTERIZE_NONFINITE, FLAG_UNPAIRED = 2 };

typedef unsigned long long u64;

struct Inverse {
    double a0, a1, a2, a3, t2, t5;
    int on;
};

struct Shapes {                                                   // the polygons as the caller gave them
    const double *pts;
    const int64_t *ring_off, *poly_off;
    uint32_t n_points, n_rings, n_polys;
};

// key = polygon | row | column, the column in the low bits; only the bits in use are sorted
struct KeyBits {
    int col, row, poly;
    __host__ __device__ int total() const { return col + row + poly; }
};

inline int bit_width(uint64_t v) {
    int b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

inline KeyBits key_bits(uint64_t rows, uint64_t cols, uint64_t n_polys) {
    return KeyBits{bit_width(cols), bit_width(rows - 1), bit_width(n_polys ? n_polys - 1 : 0)};   // columns run 0 .. cols
}

// ------------------------------------------------------------------ the rule's arithmetic
// a * x + b * y as two separately rounded products and one sum: hipcc at -O3 would contract them into v_fma_f64
__device__ __forceinline__ double two_products(double a, double x, double b, double y) {
#pragma clang fp contract(off)
    const double ax = a * x;
    const double by = b * y;
    return ax + by;
}

__device__ __forceinline__ void to_pixel(const Inverse &m, double x, double y, double &u, double &v) {
    if (!m.on) {
        u = x, v = y;
        return;
    }
    const double dx = x - m.t2, dy = y - m.t5;
    u = two_products(m.a0, dx, m.a1, dy);
    v = two_products(m.a2, dx, m.a3, dy);
}

// where the canonical edge (u0, v0)-(u1, v1) meets the line v = vc: every operation rounded on its own, a real division
__device__ __forceinline__ double cross_u(double u0, double v0, double u1, double v1, double vc) {
#pragma clang fp contract(off)
    const double num = (vc - v0) * (u1 - u0);
    const double q = num / (v1 - v0);
    return u0 + q;
}

__device__ __forceinline__ bool crosses(double v0, double v1, long j) {
    const double vc = (double)j + 0.5;
    return v0 <= vc && vc < v1;
}

// rows [jlo, jhi) of 0 .. rows that the edge v0 < v1 crosses: the range comes from the ends, and each end is then moved by at
// most one row until `crosses` itself agrees (the rows that cross are contiguous)
__device__ __forceinline__ void row_range(double v0, double v1, long rows, long &jlo, long &jhi) {
    const double lo = ceil(v0 - 0.5), hi = ceil(v1 - 0.5);
    jlo = lo >= (double)rows ? rows : (lo > 0.0 ? (long)lo : 0);
    jhi = hi >= (double)rows ? rows : (hi > 0.0 ? (long)hi : 0);
    if (jlo > 0 && crosses(v0, v1, jlo - 1)) --jlo;
    else if (jlo < jhi && !crosses(v0, v1, jlo)) ++jlo;
    if (jhi < rows && jhi >= jlo && crosses(v0, v1, jhi)) ++jhi;
    else if (jhi > jlo && !crosses(v0, v1, jhi - 1)) --jhi;
    if (jhi < jlo) jhi = jlo;
}

// the first column i with i + 0.5 >= ux, clamped to [0, cols]
__device__ __forceinline__ long column_of(double ux, long cols) {
    const double c = ceil(ux - 0.5);
    long i = c >= (double)cols ? cols : (c > 0.0 ? (long)c : 0);
    if (i > 0 && (double)(i - 1) + 0.5 >= ux) --i;
    else if (i < cols && !((double)i + 0.5 >= ux)) ++i;
    return i;
}

// the last k of 0 .. n - 1 with a[k] <= x, for a non-decreasing a with a[0] <= x; at most 32 steps (n <= 2^31)
template <typename T> __device__ __forceinline__ uint32_t last_at_most(const T *__restrict__ a, uint32_t n, T x) {
    uint32_t lo = 0, hi = n;
    for (int step = 0; step < 32 && hi - lo > 1; ++step) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct Edge {                                                     // canonical: v0 < v1 wherever rows > 0
    double u0, v0, u1, v1;
    long jlo, rows;                                               // the rows it crosses: jlo .. jlo + rows - 1
    bool finite;
};

__device__ __forceinline__ Edge edge_between(const Shapes &g, const Inverse &m, uint32_t k, uint32_t nxt, long raster_rows) {
    double ua, va, ub, vb;
    to_pixel(m, g.pts[2 * (size_t)k], g.pts[2 * (size_t)k + 1], ua, va);
    to_pixel(m, g.pts[2 * (size_t)nxt], g.pts[2 * (size_t)nxt + 1], ub, vb);
    Edge e;
    const bool swap = vb < va;
    e.u0 = swap ? ub : ua, e.v0 = swap ? vb : va;
    e.u1 = swap ? ua : ub, e.v1 = swap ? va : vb;
    e.finite = isfinite(ua) && isfinite(va) && isfinite(ub) && isfinite(vb);
    e.jlo = 0, e.rows = 0;
    if (e.finite && e.v0 < e.v1) {
        long jhi;
        row_range(e.v0, e.v1, raster_rows, e.jlo, jhi);
        e.rows = jhi - e.jlo;
    }
    return e;
}

// ------------------------------------------------------------------ census: one thread per ring point
__global__ void __launch_bounds__(THREADS) census_kernel(Shapes g, Inverse m, uint32_t raster_rows, u64 *__restrict__ cnt,
                                                         uint32_t *__restrict__ poly, uint32_t *__restrict__ next,
                                                         uint32_t *__restrict__ flags) {
    const uint64_t t = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    bool bad = false;
    if (t < g.n_points) {
        const uint32_t k = (uint32_t)t;
        const uint32_t r = last_at_most(g.ring_off, g.n_rings + 1, (int64_t)k);
        const uint32_t p = last_at_most(g.poly_off, g.n_polys + 1, (int64_t)r);
        const int64_t first = g.ring_off[r], end = r < g.n_rings ? g.ring_off[r + 1] : (int64_t)g.n_points;
        int64_t nx = (int64_t)k + 1 == end ? first : (int64_t)k + 1;
        if (nx < 0 || nx >= (int64_t)g.n_points) nx = k;           // (offsets the caller did not check: stay inside the array)
        const Edge e = edge_between(g, m, k, (uint32_t)nx, (long)raster_rows);
        bad = !isfinite(g.pts[2 * (size_t)k]) || !isfinite(g.pts[2 * (size_t)k + 1]) || !e.finite;
        cnt[k] = (u64)e.rows;
        poly[k] = p < g.n_polys ? p : g.n_polys - 1;
        next[k] = (uint32_t)nx;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, (uint32_t)FLAG_NONFINITE);
}

// ------------------------------------------------------------------ emit: one thread per crossing
__global__ void __launch_bounds__(THREADS) emit_kernel(Shapes g, Inverse m, uint32_t raster_rows, uint32_t raster_cols,
                                                       KeyBits kb, const u64 *__restrict__ scan, const uint32_t *__restrict__ poly,
                                                       const uint32_t *__restrict__ next, uint64_t first, uint64_t n_crossings,
                                                       u64 *__restrict__ keys) {
    const uint64_t t = first + (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= n_crossings) return;
    const uint32_t k = last_at_most(scan, g.n_points + 1, (u64)t);
    const Edge e = edge_between(g, m, k, next[k], (long)raster_rows);
    const long j = e.jlo + (long)(t - scan[k]);
    const double ux = cross_u(e.u0, e.v0, e.u1, e.v1, (double)j + 0.5);
    const long col = column_of(ux, (long)raster_cols);
    keys[t] = ((u64)poly[k] << (kb.row + kb.col)) | ((u64)j << kb.col) | (u64)col;
}

// ------------------------------------------------------------------ pair: crossings 2s and 2s + 1 are the span [c0, c1)
__global__ void __launch_bounds__(THREADS) pair_kernel(const u64 *__restrict__ keys, uint64_t n_pairs, KeyBits kb,
                                                       u64 *__restrict__ chunks, uint32_t *__restrict__ words) {
    const uint64_t s = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    bool span = false, unpaired = false;
    if (s < n_pairs) {
        const u64 a = keys[2 * s], b = keys[2 * s + 1];
        const u64 mask = (1ull << kb.col) - 1;
        const u64 c0 = a & mask, c1 = b & mask;
        unpaired = (a >> kb.col) != (b >> kb.col);
        span = !unpaired && c1 > c0;
        chunks[s] = span ? ((c1 - 1) >> CHUNK_SHIFT) - (c0 >> CHUNK_SHIFT) + 1 : 0;
    }
    const u64 spans = __ballot(span);
    if ((threadIdx.x & 63) == 0) {
        if (spans) atomicAdd(words, (uint32_t)__popcll(spans));
    }
    if (__ballot(unpaired) && (threadIdx.x & 63) == 0) atomicOr(words + 1, (uint32_t)FLAG_UNPAIRED);
}

// ------------------------------------------------------------------ burn: one wave per (span, chunk), one lane per cell
template <bool COUNT>
__global__ void __launch_bounds__(THREADS) burn_kernel(const u64 *__restrict__ keys, const u64 *__restrict__ scan,
                                                       uint32_t n_pairs, KeyBits kb, uint32_t raster_cols,
                                                       const uint32_t *__restrict__ priority, uint64_t first, uint64_t n_items,
                                                       uint32_t *plane) {
    // the item is the same for a wave's 64 lanes: made uniform, so that the search runs on scalar loads
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t item = first + (uint64_t)blockIdx.x * WAVES + wave;
    if (item >= n_items) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t s = last_at_most(scan, n_pairs + 1, (u64)item);
    const u64 a = keys[2 * (size_t)s], b = keys[2 * (size_t)s + 1];
    const u64 mask = (1ull << kb.col) - 1;
    const u64 c0 = a & mask, c1 = b & mask;
    const u64 row = (a >> kb.col) & ((1ull << kb.row) - 1);
    const u64 col = (((c0 >> CHUNK_SHIFT) + (item - scan[s])) << CHUNK_SHIFT) + lane;
    if (col < c0 || col >= c1 || col >= raster_cols) return;
    uint32_t *cell = plane + row * raster_cols + col;
    if (COUNT) {
        atomicAdd(cell, 1u);
    } else {
        atomicMax(cell, priority[a >> (kb.row + kb.col)] + 1u);
    }
}

// ------------------------------------------------------------------ gather: the plane in the output's dtype
template <typename T>
__global__ void __launch_bounds__(THREADS) gather_kernel(const uint32_t *__restrict__ plane, uint64_t n,
                                                         const T *__restrict__ values, const uint32_t *__restrict__ order,
                                                         T fill, int count, T *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = plane[i];
    out[i] = count ? (T)w : (w ? values[order[w - 1]] : fill);
}

// ------------------------------------------------------------------ workspaces
struct Work {                                                     // of xrs_rasterize_census
    u64 *cnt;                                                     // [n_points + 1]: rows per edge, then their exclusive sums
    uint32_t *poly, *next, *flags;
    void *cub;
    size_t cub_bytes, total;
};

Work carve(void *base, uint64_t n_points) {
    Carver c(base);
    Work p{};
    p.cnt = c.take<u64>(n_points + 1);
    p.poly = c.take<uint32_t>(n_points);
    p.next = c.take<uint32_t>(n_points);
    p.flags = c.take<uint32_t>(64);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, p.cub_bytes, (u64 *)nullptr, (u64 *)nullptr, (size_t)(n_points + 1));
    p.cub = c.take<char>(p.cub_bytes > 0 ? p.cub_bytes : 1);
    p.total = c.at();
    return p;
}

struct SpanWork {                                                 // of xrs_rasterize_spans
    u64 *keys[2], *chunks;                                        // chunks[n_crossings / 2 + 1], then their exclusive sums
    uint32_t *words;                                              // [0] spans that are not empty, [1] FLAG_UNPAIRED
    void *cub;
    size_t cub_bytes, total;
};

SpanWork carve_spans(void *base, uint64_t n_crossings) {
    Carver c(base);
    SpanWork p{};
    for (int k = 0; k < 2; ++k) p.keys[k] = c.take<u64>(n_crossings);
    p.chunks = c.take<u64>(n_crossings / 2 + 1);
    p.words = c.take<uint32_t>(64);
    size_t a = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, (u64 *)nullptr, (u64 *)nullptr, (size_t)n_crossings, 0, 64);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (u64 *)nullptr, (u64 *)nullptr, (size_t)(n_crossings / 2 + 1));
    p.cub_bytes = a > b ? a : b;
    p.cub = c.take<char>(p.cub_bytes > 0 ? p.cub_bytes : 1);
    p.total = c.at();
    return p;
}

int check_raster(const char *fn, int64_t rows, int64_t cols) {
    if (rows < 1 || cols < 1) return fail("%s: the raster must have a shape of at least (1, 1)", fn);
    if ((uint64_t)rows > 0xFFFFFFFFull / (uint64_t)cols)
        return fail("%s: %lld x %lld cells exceed the 32-bit cell index (at most 2^32 - 1 cells)", fn, (long long)rows,
                    (long long)cols);
    return 0;
}

int check_shapes(const char *fn, uint64_t n_points, uint64_t n_rings, uint64_t n_polygons, int64_t rows, int64_t cols) {
    if (n_points == 0 || n_points > XRS_RASTERIZE_MAX_POINTS)
        return fail("%s: %llu ring points, outside 1 .. %llu", fn, (unsigned long long)n_points,
                    (unsigned long long)XRS_RASTERIZE_MAX_POINTS);
    if (n_rings == 0 || n_rings > XRS_RASTERIZE_MAX_POINTS || n_polygons == 0 || n_polygons > XRS_RASTERIZE_MAX_POINTS)
        return fail("%s: %llu polygons and %llu rings, each outside 1 .. %llu", fn, (unsigned long long)n_polygons,
                    (unsigned long long)n_rings, (unsigned long long)XRS_RASTERIZE_MAX_POINTS);
    const KeyBits kb = key_bits((uint64_t)rows, (uint64_t)cols, n_polygons);
    if (kb.total() > 64)
        return fail("%s: (polygon, row, column) needs %d + %d + %d key bits, more than 64", fn, kb.poly, kb.row, kb.col);
    return 0;
}

Inverse inverse_of(const double *inverse_host) {
    Inverse m{};
    if (inverse_host) {
        m.a0 = inverse_host[0], m.a1 = inverse_host[1], m.a2 = inverse_host[2], m.a3 = inverse_host[3];
        m.t2 = inverse_host[4], m.t5 = inverse_host[5];
        m.on = 1;
    }
    return m;
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace

extern "C" {

int xrs_rasterize_workspace_size(uint64_t n_points, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_rasterize_workspace_size: null pointer");
    *bytes_out = 0;
    if (n_points == 0 || n_points > XRS_RASTERIZE_MAX_POINTS) return 0;
    *bytes_out = carve(nullptr, n_points).total;
    return 0;
}

int xrs_rasterize_spans_workspace_size(uint64_t n_crossings, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_rasterize_spans_workspace_size: null pointer");
    *bytes_out = 0;
    if (n_crossings == 0 || n_crossings > XRS_RASTERIZE_MAX_CROSSINGS) return 0;
    *bytes_out = carve_spans(nullptr, n_crossings).total;
    return 0;
}

int xrs_rasterize_census(const double *points_dev, const int64_t *ring_offsets_dev, const int64_t *polygon_offsets_dev,
                         uint64_t n_points, uint64_t n_rings, uint64_t n_polygons, int64_t rows, int64_t cols,
                         const double *inverse_host, void *work_dev, uint64_t *n_crossings, int *flags, void *stream) {
    if (int rc = check_raster("xrs_rasterize_census", rows, cols)) return rc;
    if (int rc = check_shapes("xrs_rasterize_census", n_points, n_rings, n_polygons, rows, cols)) return rc;
    if (!points_dev || !ring_offsets_dev || !polygon_offsets_dev || !work_dev || !n_crossings || !flags)
        return fail("xrs_rasterize_census: null pointer");
    *n_crossings = 0, *flags = 0;
    hipStream_t s = as_stream(stream);
    const Work p = carve(work_dev, n_points);
    const Shapes g{points_dev, ring_offsets_dev, polygon_offsets_dev, (uint32_t)n_points, (uint32_t)n_rings, (uint32_t)n_polygons};
    XRS_HIP(hipMemsetAsync(p.cnt + n_points, 0, 8, s));
    XRS_HIP(hipMemsetAsync(p.flags, 0, 256, s));
    hipLaunchKernelGGL(census_kernel, dim3(blocks_for(n_points)), dim3(THREADS), 0, s, g, inverse_of(inverse_host), (uint32_t)rows,
                       p.cnt, p.poly, p.next, p.flags);
    XRS_LAUNCH_CHECK();
    size_t cub_bytes = p.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(p.cub, cub_bytes, p.cnt, p.cnt, (size_t)(n_points + 1), s));
    u64 total = 0;
    uint32_t flag_word = 0;
    XRS_HIP(hipMemcpyAsync(&total, p.cnt + n_points, 8, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipMemcpyAsync(&flag_word, p.flags, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    *n_crossings = total;
    *flags = (int)flag_word;
    return 0;
}

int xrs_rasterize_spans(const double *points_dev, const int64_t *ring_offsets_dev, const int64_t *polygon_offsets_dev,
                        uint64_t n_points, uint64_t n_rings, uint64_t n_polygons, int64_t rows, int64_t cols,
                        const double *inverse_host, const void *work_dev, void *spans_dev, uint64_t n_crossings,
                        uint64_t *n_spans, uint64_t *n_items, void *stream) {
    if (int rc = check_raster("xrs_rasterize_spans", rows, cols)) return rc;
    if (int rc = check_shapes("xrs_rasterize_spans", n_points, n_rings, n_polygons, rows, cols)) return rc;
    if (n_crossings == 0 || n_crossings > XRS_RASTERIZE_MAX_CROSSINGS || (n_crossings & 1))
        return fail("xrs_rasterize_spans: %llu crossings: not an even number of 2 .. %llu (closed rings cross a row an even "
                    "number of times)", (unsigned long long)n_crossings, (unsigned long long)XRS_RASTERIZE_MAX_CROSSINGS);
    if (!points_dev || !ring_offsets_dev || !polygon_offsets_dev || !work_dev || !spans_dev || !n_spans || !n_items)
        return fail("xrs_rasterize_spans: null pointer");
    *n_spans = *n_items = 0;
    hipStream_t s = as_stream(stream);
    const Work p = carve((void *)work_dev, n_points);
    const SpanWork q = carve_spans(spans_dev, n_crossings);
    const Shapes g{points_dev, ring_offsets_dev, polygon_offsets_dev, (uint32_t)n_points, (uint32_t)n_rings, (uint32_t)n_polygons};
    const KeyBits kb = key_bits((uint64_t)rows, (uint64_t)cols, n_polygons);
    const Inverse m = inverse_of(inverse_host);
    const uint64_t n_pairs = n_crossings / 2;

    XRS_HIP(hipMemsetAsync(q.words, 0, 256, s));
    XRS_HIP(hipMemsetAsync(q.chunks + n_pairs, 0, 8, s));
    for (uint64_t first = 0; first < n_crossings; first += BATCH) {
        const uint64_t part = n_crossings - first < BATCH ? n_crossings - first : BATCH;
        hipLaunchKernelGGL(emit_kernel, dim3(blocks_for(part)), dim3(THREADS), 0, s, g, m, (uint32_t)rows, (uint32_t)cols, kb,
                           (const u64 *)p.cnt, (const uint32_t *)p.poly, (const uint32_t *)p.next, first, n_crossings, q.keys[0]);
        XRS_LAUNCH_CHECK();
    }
    size_t cub_bytes = q.cub_bytes;
    XRS_HIP(hipcub::DeviceRadixSort::SortKeys(q.cub, cub_bytes, (const u64 *)q.keys[0], q.keys[1], (size_t)n_crossings, 0,
                                              kb.total(), s));
    hipLaunchKernelGGL(pair_kernel, dim3(blocks_for(n_pairs)), dim3(THREADS), 0, s, (const u64 *)q.keys[1], n_pairs, kb, q.chunks,
                       q.words);
    XRS_LAUNCH_CHECK();
    cub_bytes = q.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(q.cub, cub_bytes, q.chunks, q.chunks, (size_t)(n_pairs + 1), s));
    u64 items = 0;
    uint32_t words[2] = {0, 0};
    XRS_HIP(hipMemcpyAsync(&items, q.chunks + n_pairs, 8, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipMemcpyAsync(words, q.words, 8, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    if (words[1] & FLAG_UNPAIRED)
        return fail("xrs_rasterize_spans: a (polygon, row) holds an odd number of crossings (a ring with a non-finite vertex?)");
    *n_spans = words[0];
    *n_items = items;
    return 0;
}

int xrs_rasterize_burn(int64_t rows, int64_t cols, const void *spans_dev, uint64_t n_crossings, uint64_t n_polygons,
                       uint64_t n_items, const uint32_t *priority_dev, int count, uint32_t *plane_dev, void *stream) {
    if (int rc = check_raster("xrs_rasterize_burn", rows, cols)) return rc;
    if (!plane_dev) return fail("xrs_rasterize_burn: null pointer");
    hipStream_t s = as_stream(stream);
    XRS_HIP(hipMemsetAsync(plane_dev, 0, (size_t)rows * (size_t)cols * 4, s));
    if (n_items == 0) return 0;                                   // nothing covered: the plane of zeros is the result
    if (n_crossings < 2 || n_crossings > XRS_RASTERIZE_MAX_CROSSINGS || (n_crossings & 1))
        return fail("xrs_rasterize_burn: bad crossing count");
    if (n_polygons == 0 || n_polygons > XRS_RASTERIZE_MAX_POINTS) return fail("xrs_rasterize_burn: bad polygon count");
    const KeyBits kb = key_bits((uint64_t)rows, (uint64_t)cols, n_polygons);
    if (kb.total() > 64) return fail("xrs_rasterize_burn: the key does not fit 64 bits");
    if (!spans_dev || (!count && !priority_dev)) return fail("xrs_rasterize_burn: null pointer");
    const SpanWork q = carve_spans((void *)spans_dev, n_crossings);
    const uint32_t n_pairs = (uint32_t)(n_crossings / 2);
    const uint64_t per_launch = BATCH / 64;                       // items: one wave each
    for (uint64_t first = 0; first < n_items; first += per_launch) {
        const uint64_t part = n_items - first < per_launch ? n_items - first : per_launch;
        const dim3 grid((unsigned)((part + WAVES - 1) / WAVES));
        if (count)
            hipLaunchKernelGGL(burn_kernel<true>, grid, dim3(THREADS), 0, s, (const u64 *)q.keys[1], (const u64 *)q.chunks, n_pairs,
                               kb, (uint32_t)cols, priority_dev, first, n_items, plane_dev);
        else
            hipLaunchKernelGGL(burn_kernel<false>, grid, dim3(THREADS), 0, s, (const u64 *)q.keys[1], (const u64 *)q.chunks, n_pairs,
                               kb, (uint32_t)cols, priority_dev, first, n_items, plane_dev);
        XRS_LAUNCH_CHECK();
    }
    return 0;
}

int xrs_rasterize_gather(const uint32_t *plane_dev, int64_t rows, int64_t cols, const void *values_dev, const uint32_t *order_dev,
                         int dtype, const void *fill_host, int count, void *out_dev, void *stream) {
    if (int rc = check_raster("xrs_rasterize_gather", rows, cols)) return rc;
    if (!dtype_bytes(dtype)) return fail("xrs_rasterize_gather: unsupported dtype code %d", dtype);
    if (!plane_dev || !out_dev || !fill_host) return fail("xrs_rasterize_gather: null pointer");
    hipStream_t s = as_stream(stream);
    const uint64_t n = (uint64_t)rows * (uint64_t)cols;
    int rc = 0;
    with_dtype(dtype, [&](auto t) {
        using T = dtype_of<decltype(t)>;
        T fill;
        memcpy(&fill, fill_host, sizeof(T));
        hipLaunchKernelGGL(gather_kernel<T>, dim3(blocks_for(n)), dim3(THREADS), 0, s, plane_dev, n, (const T *)values_dev,
                           order_dev, fill, count, (T *)out_dev);
        if (hipGetLastError() != hipSuccess) rc = fail("xrs_rasterize_gather: kernel launch failed");
    });
    return rc;
}

}  // extern "C"

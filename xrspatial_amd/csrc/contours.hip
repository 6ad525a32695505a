// contours: the isolines of a raster at K levels, by marching squares.  No counterpart in the reference; the rule is DESIGN.md §6s.
//
// Node (r, c) is the centre of cell (r, c); quad q = r * cols + c (r < rows - 1, c < cols - 1) has the corners TL = (r, c), TR =
// (r, c + 1), BR = (r + 1, c + 1), BL = (r + 1, c), and the walk TL -> TR -> BR -> BL -> TL has the sides 0 top, 1 right, 2 bottom,
// 3 left.  A quad with a corner that is not finite is not whole and produces nothing.  A node is high at a level when z > level.
//   segments  of a whole quad at level k: one from the side the walk crosses high -> low (its start) to the side it crosses
//             low -> high (its end); with two diagonal high corners two, told apart by the centre ((zTL + zTR) + (zBR + zBL)) * 0.25;
//   census    with lo / hi the least / greatest corner, the levels lo <= level < hi are the sorted levels [kl, kh), found by binary
//             search, and the saddle levels v1 <= level < v2 (v2 the lesser of the diagonal pair that is wholly above the other
//             pair, v1 the greater of that other pair) are [sl, sh) inside them: (kh - kl) + (sh - sl) segments, and
//             (min(kh, k) - min(kl, k)) + (min(sh, k) - min(sl, k)) of them below level k;
//   ids       a quad's segments are numbered by level, at a saddle level by start side, after those of every quad before it: the
//             id of the segment that starts on a given side of a given quad at a given level is closed-form from that quad's four
//             corners, so a segment finds its successor, in the quad across its end side, without a sort or a hash;
//   lines     a segment with no whole quad across its start side is the head of an open line; a ring begins at the segment whose
//             start edge id is its smallest.  Both come from one pointer doubling over the predecessors with the key (edge id + 1,
//             0 for a head): a segment that ends up with its own key starts a line.  A second doubling (Wyllie's list ranking
//             over the lists cut in front of their starts) gives every segment its position in its line and its line's start.
//
// Three calls, each ending in a small device-to-host read that sizes what the next one needs:
//   xrs_contours_census   census_kernel (one thread per cell, 256-cell workgroups: the count, its prefix in the workgroup, the
//                         workgroup's total) + ExclusiveSum over the workgroup totals;
//   xrs_contours_lines    emit_kernel (one thread per segment: its quad by binary search in the prefixes, its level and sides, its
//                         successor), leader_round x <= 32, start_kernel, rank_init + rank_round x <= 32;
//   xrs_contours_scatter  collect_kernel ((level, key) and first segment of every line; the segment count of every line), radix
//                         sort, table_kernel + ExclusiveSum (line offsets), level_kernel (level offsets), point_kernel.
// Every loop is bounded (the binary searches by 32 steps, the doublings by 32 rounds), no workgroup waits for another, and every
// store is an ordinary vector store or an atomicAdd.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

#include <cmath>

using namespace xrs;

namespace {

constexpr int THREADS = 256;
constexpr uint32_t NIL = 0xFFFFFFFFu;
constexpr int MAX_ROUNDS = 32, ROUND_GROUP = 4;
constexpr int WORD_LINES = 0, WORD_BAD = 1, WORD_SLOTS = 2, WORD_CHANGED = 8, N_WORDS = 8 + 2 * MAX_ROUNDS + 8;

typedef unsigned long long u64;

struct Grid {
    uint32_t rows, cols, n_levels;
};

// the number of levels below x: the levels are strictly increasing
__device__ __forceinline__ uint32_t count_below(const double *__restrict__ lv, uint32_t from, uint32_t to, double x) {
    uint32_t lo = from, n = to - from;
    while (n > 0) {
        const uint32_t half = n >> 1;
        if (lv[lo + half] < x) lo += half + 1, n -= half + 1;
        else n = half;
    }
    return lo;
}

struct Span {
    uint32_t kl, kh, sl, sh;                                      // levels [kl, kh) cross the quad, [sl, sh) of them at a saddle
    __device__ uint32_t count() const { return (kh - kl) + (sh - sl); }
    __device__ uint32_t before(uint32_t k) const { return (min(kh, k) - min(kl, k)) + (min(sh, k) - min(sl, k)); }
};

__device__ __forceinline__ bool all_finite(const double z[4]) {
    return __builtin_isfinite(z[0]) && __builtin_isfinite(z[1]) && __builtin_isfinite(z[2]) && __builtin_isfinite(z[3]);
}

// of a whole quad
__device__ __forceinline__ Span span_of(const double z[4], const double *__restrict__ lv, uint32_t K) {
    const double a_lo = fmin(z[0], z[2]), a_hi = fmax(z[0], z[2]), b_lo = fmin(z[1], z[3]), b_hi = fmax(z[1], z[3]);
    const double lo = fmin(a_lo, b_lo), hi = fmax(a_hi, b_hi);
    Span s;
    s.kl = count_below(lv, 0, K, lo);
    s.kh = s.kl;
    if (s.kl < K && lv[s.kl] < hi) s.kh = count_below(lv, s.kl + 1, K, hi);   // most quads of a terrain cross no level
    s.sl = s.sh = s.kl;
    if (s.kh > s.kl) {
        if (a_lo > b_hi) s.sl = count_below(lv, s.kl, s.kh, b_hi), s.sh = count_below(lv, s.sl, s.kh, a_lo);
        else if (b_lo > a_hi) s.sl = count_below(lv, s.kl, s.kh, a_hi), s.sh = count_below(lv, s.sl, s.kh, b_lo);
    }
    return s;
}

// the corners of quad (r, c) in walk order, as float64
template <typename T> __device__ __forceinline__ void corners_of(const T *__restrict__ in, Grid g, uint32_t r, uint32_t c, double z[4]) {
    const size_t i = (size_t)r * g.cols + c;
    z[0] = (double)in[i], z[1] = (double)in[i + 1], z[2] = (double)in[i + g.cols + 1], z[3] = (double)in[i + g.cols];
}
__device__ __forceinline__ void corners_of(const void *in, int dt, Grid g, uint32_t r, uint32_t c, double z[4]) {
    const long i = (long)r * g.cols + c;
    z[0] = load_as<double>(in, dt, i), z[1] = load_as<double>(in, dt, i + 1);
    z[2] = load_as<double>(in, dt, i + g.cols + 1), z[3] = load_as<double>(in, dt, i + g.cols);
}

// The segments of a whole quad at one level, as (start side, end side) pairs in start-side order; returns their number.
__device__ __forceinline__ int segments_at(const double z[4], double level, int start[2], int end[2]) {
    const bool h[4] = {z[0] > level, z[1] > level, z[2] > level, z[3] > level};
    int n = 0, e = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const bool a = h[s], b = h[(s + 1) & 3];
        if (a && !b && n < 2) start[n++] = s;
        if (!a && b) e = s;
    }
    if (n == 1) {
        end[0] = e;
    } else if (n == 2) {
#pragma clang fp contract(off)
        const double m = ((z[0] + z[1]) + (z[2] + z[3])) * 0.25;
        const int turn = m > level ? 1 : 3;                       // cut off the low corners, or the high ones
        end[0] = (start[0] + turn) & 3, end[1] = (start[1] + turn) & 3;
    }
    return n;
}

// ------------------------------------------------------------------ census: segments per quad, over all levels
template <typename T>
__global__ void __launch_bounds__(THREADS) census_kernel(const T *__restrict__ in, Grid g, uint64_t n, const double *__restrict__ lv,
                                                         uint32_t *__restrict__ pre, u64 *__restrict__ btot) {
    typedef hipcub::BlockScan<uint32_t, THREADS> Scan;
    __shared__ typename Scan::TempStorage tmp;
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    uint32_t count = 0;
    if (i < n) {
        const uint32_t r = (uint32_t)(i / g.cols), c = (uint32_t)(i - (uint64_t)r * g.cols);
        if (r + 1 < g.rows && c + 1 < g.cols) {
            double z[4];
            corners_of(in, g, r, c, z);
            if (all_finite(z)) count = span_of(z, lv, g.n_levels).count();
        }
    }
    uint32_t before, total;
    Scan(tmp).ExclusiveSum(count, before, total);
    if (i < n) pre[i] = before;
    if (threadIdx.x == 0) btot[blockIdx.x] = total;
}

__device__ __forceinline__ u64 offset_of(const u64 *__restrict__ boff, const uint32_t *__restrict__ pre, uint32_t q) {
    return boff[q / THREADS] + pre[q];
}

// edge id of a side of quad (r, c): horizontal edge (r, c)-(r, c + 1) is 2 * (r * cols + c), vertical edge (r, c)-(r + 1, c) one more
__device__ __forceinline__ uint32_t edge_of(Grid g, uint32_t q, int side) {
    const uint32_t node = q + (side == 1 ? 1u : 0u) + (side == 2 ? g.cols : 0u);
    return 2u * node + (uint32_t)(side & 1);
}

// ------------------------------------------------------------------ emit: every segment's quad, level, sides and successor
// code = level << 4 | start side << 2 | end side
__global__ void __launch_bounds__(THREADS) emit_kernel(const void *__restrict__ in, int dt, Grid g, uint32_t n_cells,
                                                       const double *__restrict__ lv, const uint32_t *__restrict__ pre,
                                                       const u64 *__restrict__ boff, uint32_t n_blocks, uint32_t S,
                                                       uint32_t *__restrict__ quad, uint32_t *__restrict__ code,
                                                       uint32_t *__restrict__ next, uint32_t *pred, uint32_t *__restrict__ key,
                                                       uint32_t *__restrict__ words) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    // the workgroup of the census whose segments hold s: the last one that begins at or before it
    uint32_t b = 0, nb = n_blocks;
    while (nb > 1) {
        const uint32_t half = nb >> 1;
        if (boff[b + half] <= (u64)s) b += half, nb -= half;
        else nb = half;
    }
    const uint32_t local = s - (uint32_t)boff[b];
    const uint32_t first = b * THREADS;
    uint32_t t = 0, nt = min((uint32_t)THREADS, n_cells - first);
    while (nt > 1) {
        const uint32_t half = nt >> 1;
        if (pre[first + t + half] <= local) t += half, nt -= half;
        else nt = half;
    }
    const uint32_t q = first + t, j = local - pre[q];
    const uint32_t r = q / g.cols, c = q - r * g.cols;
    bool bad = !(r + 1 < g.rows && c + 1 < g.cols);
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    Span sp{0, 0, 0, 0};
    if (!bad) {
        corners_of(in, dt, g, r, c, z);
        bad = !all_finite(z);
        if (!bad) sp = span_of(z, lv, g.n_levels);
    }
    bad = bad || j >= sp.count();
    uint32_t k = 0, sub = 0;
    if (!bad) {                                                   // the j-th segment of the quad: by level, two at a saddle level
        const uint32_t plain = sp.sl - sp.kl, saddle = 2 * (sp.sh - sp.sl);
        if (j < plain) k = sp.kl + j;
        else if (j < plain + saddle) k = sp.sl + ((j - plain) >> 1), sub = (j - plain) & 1;
        else k = sp.sh + (j - plain - saddle);
    }
    int start[2] = {0, 0}, end[2] = {0, 0};
    if (!bad) bad = segments_at(z, lv[k], start, end) != (k >= sp.sl && k < sp.sh ? 2 : 1);
    if (bad) {                                                    // the census and this kernel disagree: nothing of s is valid
        atomicAdd(words + WORD_BAD, 1u);
        quad[s] = 0, code[s] = 0, next[s] = NIL, key[s] = 0;
        return;
    }
    const int a = start[sub], e = end[sub];
    quad[s] = q;
    code[s] = k << 4 | (uint32_t)a << 2 | (uint32_t)e;
    const double level = lv[k];
    const int dr[4] = {-1, 0, 1, 0}, dc[4] = {0, 1, 0, -1};       // the quad across a side
    // the successor starts on this segment's end edge, which is side e ^ 2 of the quad across it
    uint32_t nx = NIL;
    {
        const long r2 = (long)r + dr[e], c2 = (long)c + dc[e];
        if (r2 >= 0 && c2 >= 0 && r2 + 1 < (long)g.rows && c2 + 1 < (long)g.cols) {
            double w[4];
            corners_of(in, dt, g, (uint32_t)r2, (uint32_t)c2, w);
            if (all_finite(w)) {
                const uint32_t q2 = (uint32_t)r2 * g.cols + (uint32_t)c2;
                const Span sp2 = span_of(w, lv, g.n_levels);
                int st2[2] = {0, 0}, en2[2] = {0, 0};
                const int n2 = segments_at(w, level, st2, en2);
                const uint32_t sub2 = (n2 == 2 && st2[1] == (e ^ 2)) ? 1u : 0u;
                const u64 id = offset_of(boff, pre, q2) + sp2.before(k) + sub2;
                if (n2 >= 1 && st2[sub2] == (e ^ 2) && id < (u64)S) nx = (uint32_t)id;
                else atomicAdd(words + WORD_BAD, 1u);
            }
        }
    }
    next[s] = nx;
    if (nx != NIL) pred[nx] = s;
    // a head: no whole quad across the start side, so no segment ends on the start edge
    bool head = true;
    {
        const long r2 = (long)r + dr[a], c2 = (long)c + dc[a];
        if (r2 >= 0 && c2 >= 0 && r2 + 1 < (long)g.rows && c2 + 1 < (long)g.cols) {
            double w[4];
            corners_of(in, dt, g, (uint32_t)r2, (uint32_t)c2, w);
            head = !all_finite(w);
        }
    }
    key[s] = head ? 0u : edge_of(g, q, a) + 1u;
}

// the key emit_kernel gave segment s
__device__ __forceinline__ uint32_t key_of(Grid g, const uint32_t *__restrict__ quad, const uint32_t *__restrict__ code,
                                           const uint32_t *__restrict__ pred, uint32_t s) {
    return pred[s] == NIL ? 0u : edge_of(g, quad[s], (int)(code[s] >> 2 & 3)) + 1u;
}

// ------------------------------------------------------------------ leader: min of key over the predecessors (a ring: over the ring)
__global__ void __launch_bounds__(THREADS) leader_round(const uint32_t *__restrict__ pin, const uint32_t *__restrict__ kin,
                                                        uint32_t *__restrict__ pout, uint32_t *__restrict__ kout, uint32_t S,
                                                        uint32_t *__restrict__ changed) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    bool ch = false;
    if (s < S) {
        uint32_t p = pin[s], k = kin[s];
        if (p != NIL) {
            const uint32_t k2 = kin[p];
            ch = k2 < k;
            k = ch ? k2 : k;
            p = pin[p];
        }
        kout[s] = k;
        pout[s] = p;
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) *changed = 1;
}

// a segment whose least key is its own starts a line: a head (0) or the least edge of a ring
__global__ void __launch_bounds__(THREADS) start_kernel(Grid g, const uint32_t *__restrict__ quad, const uint32_t *__restrict__ code,
                                                        const uint32_t *__restrict__ pred, const uint32_t *__restrict__ least,
                                                        uint8_t *__restrict__ start, uint32_t S, uint32_t *__restrict__ n_lines) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    bool is = false;
    if (s < S) {
        is = least[s] == key_of(g, quad, code, pred, s);
        start[s] = is;
    }
    const u64 b = __ballot(is);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(n_lines, (uint32_t)__popcll(b));
}

// ------------------------------------------------------------------ rank: lists cut in front of their starts
__global__ void __launch_bounds__(THREADS) rank_init(const uint32_t *__restrict__ pred, const uint8_t *__restrict__ start,
                                                     uint32_t *__restrict__ ptr, uint32_t *__restrict__ val, uint32_t *__restrict__ first,
                                                     uint32_t S) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    const bool is = start[s] != 0;
    ptr[s] = is ? NIL : pred[s];
    val[s] = is ? 0u : 1u;
    first[s] = s;
}

__global__ void __launch_bounds__(THREADS) rank_round(const uint32_t *__restrict__ pin, const uint32_t *__restrict__ vin,
                                                      const uint32_t *__restrict__ fin, uint32_t *__restrict__ pout,
                                                      uint32_t *__restrict__ vout, uint32_t *__restrict__ fout, uint32_t S,
                                                      uint32_t *__restrict__ changed) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    bool ch = false;
    if (s < S) {
        uint32_t p = pin[s], v = vin[s], f = fin[s];
        ch = p != NIL;
        if (ch) v += vin[p], f = fin[p], p = pin[p];
        pout[s] = p, vout[s] = v, fout[s] = f;
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) *changed = 1;
}

// ------------------------------------------------------------------ line table
// every start: its (level, edge) key and its segment, in any order; every last segment: its line's segment count
__global__ void __launch_bounds__(THREADS) collect_kernel(Grid g, const uint32_t *__restrict__ quad, const uint32_t *__restrict__ code,
                                                          const uint32_t *__restrict__ next, const uint8_t *__restrict__ start,
                                                          const uint32_t *__restrict__ pos, const uint32_t *__restrict__ first,
                                                          uint32_t S, u64 *__restrict__ keys, uint32_t *__restrict__ vals,
                                                          uint32_t *__restrict__ n_seg, uint32_t *__restrict__ slots, uint32_t max_lines) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    if (start[s]) {
        const uint32_t slot = atomicAdd(slots, 1u);
        if (slot < max_lines) {
            keys[slot] = (u64)(code[s] >> 4) << 32 | edge_of(g, quad[s], (int)(code[s] >> 2 & 3));
            vals[slot] = s;
        }
    }
    const uint32_t nx = next[s];
    if (nx == NIL || start[nx]) n_seg[first[s]] = pos[s] + 1u;
}

// sorted line i: its index for its first segment, its point count (one more than its segments), whether it is closed
__global__ void __launch_bounds__(THREADS) table_kernel(const uint32_t *__restrict__ vals, uint32_t L, const uint32_t *__restrict__ n_seg,
                                                        const uint32_t *__restrict__ pred, uint32_t *__restrict__ line_of,
                                                        int64_t *__restrict__ count1, uint8_t *__restrict__ closed) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i > L) return;
    if (i == L) {
        count1[i] = 0;
        return;
    }
    const uint32_t s = vals[i];
    line_of[s] = i;
    count1[i] = (int64_t)n_seg[s] + 1;
    closed[i] = pred[s] != NIL;
}

// level_off[k] = lines of the levels before k
__global__ void __launch_bounds__(THREADS) level_kernel(const u64 *__restrict__ keys, uint32_t L, uint32_t K, int64_t *__restrict__ level_off) {
    const uint32_t k = blockIdx.x * THREADS + threadIdx.x;
    if (k > K) return;
    const u64 x = (u64)k << 32;
    uint32_t lo = 0, n = L;
    while (n > 0) {
        const uint32_t half = n >> 1;
        if (keys[lo + half] < x) lo += half + 1, n -= half + 1;
        else n = half;
    }
    level_off[k] = lo;
}

// ------------------------------------------------------------------ points
struct Affine {
    double t[6];
    int on;
};

// a * i + b * j + c as two separately rounded products and two sums, left to right (hipcc at -O3 would contract them)
__device__ __forceinline__ double affine(double a, double i, double b, double j, double c) {
#pragma clang fp contract(off)
    const double ai = a * i;
    const double bj = b * j;
    const double sum = ai + bj;
    return sum + c;
}

// the crossing of a side of quad q: t = (level - z0) / (z1 - z0) along the edge from its first node
__device__ __forceinline__ void point_of(const void *in, int dt, Grid g, uint32_t q, int side, double level, const Affine &tf,
                                         double *px, double *py) {
#pragma clang fp contract(off)
    const uint32_t node = q + (side == 1 ? 1u : 0u) + (side == 2 ? g.cols : 0u);
    const bool vertical = side & 1;
    const uint32_t r = node / g.cols, c = node - r * g.cols;
    const double z0 = load_as<double>(in, dt, (long)node);
    const double z1 = load_as<double>(in, dt, (long)node + (vertical ? (long)g.cols : 1L));
    const double num = level - z0;
    const double den = z1 - z0;
    const double t = num / den;
    double x = (double)c + 0.5, y = (double)r + 0.5;
    if (vertical) y = y + t;
    else x = x + t;
    if (tf.on) {
        const double qx = affine(tf.t[0], x, tf.t[1], y, tf.t[2]), qy = affine(tf.t[3], x, tf.t[4], y, tf.t[5]);
        x = qx, y = qy;
    }
    *px = x, *py = y;
}

__global__ void __launch_bounds__(THREADS) point_kernel(const void *__restrict__ in, int dt, Grid g, const double *__restrict__ lv,
                                                        const uint32_t *__restrict__ quad, const uint32_t *__restrict__ code,
                                                        const uint32_t *__restrict__ next, const uint8_t *__restrict__ start,
                                                        const uint32_t *__restrict__ pos, const uint32_t *__restrict__ first,
                                                        const uint32_t *__restrict__ line_of, const int64_t *__restrict__ line_off,
                                                        uint32_t S, uint32_t L, Affine tf, double *__restrict__ points) {
    const uint32_t s = blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    const uint32_t cd = code[s], q = quad[s], line = line_of[first[s]];
    if (line >= L) return;                                        // (cannot be: every list ends at a start, and starts have a line)
    const u64 n_points = (u64)S + L;
    const double level = lv[cd >> 4];
    const u64 at = (u64)line_off[line] + pos[s];
    double x, y;
    point_of(in, dt, g, q, (int)(cd >> 2 & 3), level, tf, &x, &y);
    if (at < n_points) points[2 * at] = x, points[2 * at + 1] = y;
    const uint32_t nx = next[s];
    if (nx == NIL || start[nx]) {                                 // the last segment: its end point, in a ring the first point again
        point_of(in, dt, g, q, (int)(cd & 3), level, tf, &x, &y);
        if (at + 1 < n_points) points[2 * (at + 1)] = x, points[2 * (at + 1) + 1] = y;
    }
}

// ------------------------------------------------------------------ workspaces
inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }

struct Work {                                                     // of xrs_contours_census
    size_t n, blocks;
    double *levels;
    uint32_t *pre;
    u64 *boff;                                                    // [blocks + 1]: the workgroups' totals, then their prefix
    void *cub;
    size_t cub_bytes, total;
};

Work carve(void *base, uint64_t rows, uint64_t cols, uint64_t n_levels) {
    Carver c(base);
    Work p{};
    p.n = rows * cols;
    p.blocks = (p.n + THREADS - 1) / THREADS;
    p.levels = c.take<double>(n_levels);
    p.pre = c.take<uint32_t>(p.n);
    p.boff = c.take<u64>(p.blocks + 1);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, p.cub_bytes, (u64 *)nullptr, (u64 *)nullptr, (size_t)(p.blocks + 1));
    p.cub = c.take<char>(p.cub_bytes > 0 ? p.cub_bytes : 1);
    p.total = c.at();
    return p;
}

struct LineWork {                                                 // of xrs_contours_lines
    uint32_t *quad, *code, *next, *pred, *buf[6], *words;
    uint8_t *start;
    size_t total;
};

LineWork carve_lines(void *base, uint64_t n_segments) {
    Carver c(base);
    LineWork p{};
    p.quad = c.take<uint32_t>(n_segments);
    p.code = c.take<uint32_t>(n_segments);
    p.next = c.take<uint32_t>(n_segments);
    p.pred = c.take<uint32_t>(n_segments);
    for (int k = 0; k < 6; ++k) p.buf[k] = c.take<uint32_t>(n_segments);
    p.start = c.take<uint8_t>(n_segments);
    p.words = c.take<uint32_t>(N_WORDS);
    p.total = c.at();
    return p;
}

struct SortWork {                                                 // of xrs_contours_scatter
    u64 *keys[2];
    uint32_t *vals[2];
    int64_t *count1;
    void *cub;
    size_t cub_bytes, total;
};

SortWork carve_sort(void *base, uint64_t n_lines) {
    Carver c(base);
    SortWork p{};
    for (int k = 0; k < 2; ++k) p.keys[k] = c.take<u64>(n_lines);
    for (int k = 0; k < 2; ++k) p.vals[k] = c.take<uint32_t>(n_lines);
    p.count1 = c.take<int64_t>(n_lines + 1);
    size_t a = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (u64 *)nullptr, (u64 *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                             (size_t)n_lines, 0, 64);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int64_t *)nullptr, (int64_t *)nullptr, (size_t)(n_lines + 1));
    p.cub_bytes = a > b ? a : b;
    p.cub = c.take<char>(p.cub_bytes > 0 ? p.cub_bytes : 1);
    p.total = c.at();
    return p;
}

int check_shape(const char *fn, int64_t rows, int64_t cols, uint64_t n_levels) {
    if (rows < 1 || cols < 1) return fail("%s: the raster must have a shape of at least (1, 1)", fn);
    if ((uint64_t)rows > XRS_CONTOURS_MAX_CELLS / (uint64_t)cols)
        return fail("%s: %lld x %lld cells exceed the 32-bit edge id (at most 2^31 - 1 cells)", fn, (long long)rows, (long long)cols);
    if (n_levels > XRS_CONTOURS_MAX_LEVELS)
        return fail("%s: %llu levels, at most %llu", fn, (unsigned long long)n_levels, (unsigned long long)XRS_CONTOURS_MAX_LEVELS);
    return 0;
}

int check_segments(const char *fn, uint64_t n_segments) {
    if (n_segments == 0 || n_segments > XRS_CONTOURS_MAX_SEGMENTS)
        return fail("%s: %llu segments, outside 1 .. %llu (2^32 - 2)", fn, (unsigned long long)n_segments,
                    (unsigned long long)XRS_CONTOURS_MAX_SEGMENTS);
    return 0;
}

template <typename T>
int census_impl(const T *in, Grid g, const Work &p, hipStream_t s) {
    hipLaunchKernelGGL(census_kernel<T>, dim3((unsigned)p.blocks), dim3(THREADS), 0, s, in, g, (uint64_t)p.n, (const double *)p.levels, p.pre,
                       p.boff);
    XRS_LAUNCH_CHECK();
    return 0;
}

// the doubling rounds of one phase, in groups of ROUND_GROUP with one read of the flags per group; `launch(round)` enqueues one
template <typename F> int run_rounds(const char *what, uint32_t *words_dev, int word0, hipStream_t s, int *rounds_out, F &&launch) {
    uint32_t host_words[N_WORDS];
    int done = 0;
    bool settled = false;
    while (!settled && done < MAX_ROUNDS) {
        const int first = done;
        for (int k = 0; k < ROUND_GROUP && done < MAX_ROUNDS; ++k, ++done)
            if (int rc = launch(done)) return rc;
        XRS_HIP(hipMemcpyAsync(host_words, words_dev, N_WORDS * 4, hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        for (int k = first; k < done; ++k) settled |= host_words[word0 + k] == 0;      // a still round: nothing is left to do
    }
    if (!settled) return fail("xrs_contours_lines: %s did not settle in %d rounds", what, MAX_ROUNDS);
    *rounds_out = done;
    return 0;
}

}  // namespace

extern "C" {

int xrs_contours_workspace_size(int64_t rows, int64_t cols, uint64_t n_levels, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_contours_workspace_size: null pointer");
    *bytes_out = 0;
    if (int rc = check_shape("xrs_contours_workspace_size", rows, cols, n_levels)) return rc;
    *bytes_out = carve(nullptr, (uint64_t)rows, (uint64_t)cols, n_levels).total;
    return 0;
}

int xrs_contours_lines_workspace_size(uint64_t n_segments, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_contours_lines_workspace_size: null pointer");
    *bytes_out = 0;
    if (int rc = check_segments("xrs_contours_lines_workspace_size", n_segments)) return rc;
    *bytes_out = carve_lines(nullptr, n_segments).total;
    return 0;
}

int xrs_contours_scatter_workspace_size(uint64_t n_lines, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_contours_scatter_workspace_size: null pointer");
    *bytes_out = 0;
    if (n_lines == 0 || n_lines > XRS_CONTOURS_MAX_SEGMENTS)
        return fail("xrs_contours_scatter_workspace_size: %llu lines, outside 1 .. 2^32 - 2", (unsigned long long)n_lines);
    *bytes_out = carve_sort(nullptr, n_lines).total;
    return 0;
}

int xrs_contours_census(const void *data_dev, int dtype, int64_t rows, int64_t cols, const double *levels_host, uint64_t n_levels,
                        void *work_dev, uint64_t *n_segments, void *stream) {
    if (int rc = check_shape("xrs_contours_census", rows, cols, n_levels)) return rc;
    if (!dtype_bytes(dtype)) return fail("xrs_contours_census: unsupported dtype code %d", dtype);
    if (!data_dev || !work_dev || !n_segments || (n_levels && !levels_host)) return fail("xrs_contours_census: null pointer");
    *n_segments = 0;
    for (uint64_t k = 0; k < n_levels; ++k) {
        if (!std::isfinite(levels_host[k])) return fail("xrs_contours_census: level %llu is not finite", (unsigned long long)k);
        if (k && !(levels_host[k] > levels_host[k - 1]))
            return fail("xrs_contours_census: the levels must be strictly increasing (level %llu is not above the one before)",
                        (unsigned long long)k);
    }
    if (rows < 2 || cols < 2 || n_levels == 0) return 0;          // no quad, or no level: nothing to draw
    hipStream_t s = as_stream(stream);
    const Work p = carve(work_dev, rows, cols, n_levels);
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)n_levels};
    XRS_HIP(hipMemcpyAsync(p.levels, levels_host, n_levels * 8, hipMemcpyHostToDevice, s));
    XRS_HIP(hipMemsetAsync(p.boff + p.blocks, 0, 8, s));
    int rc = 0;
    with_dtype(dtype, [&](auto t) { rc = census_impl((const dtype_of<decltype(t)> *)data_dev, g, p, s); });
    if (rc) return rc;
    size_t cub_bytes = p.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(p.cub, cub_bytes, p.boff, p.boff, (size_t)(p.blocks + 1), s));
    u64 total = 0;
    XRS_HIP(hipMemcpyAsync(&total, p.boff + p.blocks, 8, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));                             // (the levels are up as well: the caller's array is free)
    *n_segments = total;
    return 0;
}

int xrs_contours_lines(const void *data_dev, int dtype, int64_t rows, int64_t cols, uint64_t n_levels, const void *work_dev,
                       void *lines_dev, uint64_t n_segments, uint64_t *n_lines, uint64_t *n_points, int *rounds, void *stream) {
    if (int rc = check_shape("xrs_contours_lines", rows, cols, n_levels)) return rc;
    if (int rc = check_segments("xrs_contours_lines", n_segments)) return rc;
    if (!dtype_bytes(dtype)) return fail("xrs_contours_lines: unsupported dtype code %d", dtype);
    if (!data_dev || !work_dev || !lines_dev || !n_lines || !n_points) return fail("xrs_contours_lines: null pointer");
    if (rows < 2 || cols < 2 || n_levels == 0) return fail("xrs_contours_lines: no quad or no level, so no segment");
    *n_lines = *n_points = 0;
    hipStream_t s = as_stream(stream);
    const Work p = carve((void *)work_dev, rows, cols, n_levels);
    const LineWork q = carve_lines(lines_dev, n_segments);
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)n_levels};
    const uint32_t S = (uint32_t)n_segments;
    const unsigned seg_blocks = blocks_for(n_segments);
    uint32_t host_words[N_WORDS];

    XRS_HIP(hipMemsetAsync(q.words, 0, N_WORDS * 4, s));
    XRS_HIP(hipMemsetAsync(q.pred, 0xFF, n_segments * 4, s));     // NIL: a segment nobody precedes
    // key -> buf[2]
    hipLaunchKernelGGL(emit_kernel, dim3(seg_blocks), dim3(THREADS), 0, s, data_dev, dtype, g, (uint32_t)p.n, (const double *)p.levels,
                       (const uint32_t *)p.pre, (const u64 *)p.boff, (uint32_t)p.blocks, S, q.quad, q.code, q.next, q.pred, q.buf[2], q.words);
    XRS_LAUNCH_CHECK();
    XRS_HIP(hipMemcpyAsync(host_words, q.words, N_WORDS * 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    if (host_words[WORD_BAD])
        return fail("xrs_contours_lines: %u of %llu segments do not match the census (another raster, other levels, or a wrong count?)",
                    host_words[WORD_BAD], (unsigned long long)n_segments);

    // leader: (pointer, key) double-buffered in (buf[0] | buf[1], buf[2] | buf[3]); round 0 reads `pred` itself
    const uint32_t *pin = q.pred, *kin = q.buf[2];
    int lead_rounds = 0, rank_rounds = 0;
    if (int rc = run_rounds("line leaders", q.words, WORD_CHANGED, s, &lead_rounds, [&](int round) {
            uint32_t *pout = q.buf[round & 1], *kout = q.buf[2 + ((round + 1) & 1)];
            hipLaunchKernelGGL(leader_round, dim3(seg_blocks), dim3(THREADS), 0, s, pin, kin, pout, kout, S, q.words + WORD_CHANGED + round);
            XRS_LAUNCH_CHECK();
            pin = pout, kin = kout;
            return 0;
        }))
        return rc;
    hipLaunchKernelGGL(start_kernel, dim3(seg_blocks), dim3(THREADS), 0, s, g, (const uint32_t *)q.quad, (const uint32_t *)q.code,
                       (const uint32_t *)q.pred, kin, q.start, S, q.words + WORD_LINES);
    XRS_LAUNCH_CHECK();

    // rank: (pointer, position, first segment) double-buffered in (buf[0] | buf[1], buf[2] | buf[3], buf[4] | buf[5])
    hipLaunchKernelGGL(rank_init, dim3(seg_blocks), dim3(THREADS), 0, s, (const uint32_t *)q.pred, (const uint8_t *)q.start, q.buf[0], q.buf[2],
                       q.buf[4], S);
    XRS_LAUNCH_CHECK();
    int at = 0;
    if (int rc = run_rounds("line ranks", q.words, WORD_CHANGED + MAX_ROUNDS, s, &rank_rounds, [&](int round) {
            hipLaunchKernelGGL(rank_round, dim3(seg_blocks), dim3(THREADS), 0, s, (const uint32_t *)q.buf[at], (const uint32_t *)q.buf[2 + at],
                               (const uint32_t *)q.buf[4 + at], q.buf[at ^ 1], q.buf[2 + (at ^ 1)], q.buf[4 + (at ^ 1)], S,
                               q.words + WORD_CHANGED + MAX_ROUNDS + round);
            XRS_LAUNCH_CHECK();
            at ^= 1;
            return 0;
        }))
        return rc;
    // rounds run in groups of ROUND_GROUP, an even number, and a round after the last change copies its input: the positions
    // are in buf[2] and the first segments in buf[4], where xrs_contours_scatter looks; buf[1] and buf[3] are free for it
    static_assert(ROUND_GROUP % 2 == 0 && MAX_ROUNDS % ROUND_GROUP == 0, "the rank buffers' parity");
    if (at != 0) return fail("xrs_contours_lines: odd number of rank rounds");
    XRS_HIP(hipMemcpyAsync(host_words, q.words, N_WORDS * 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    const uint32_t L = host_words[WORD_LINES];
    if (L == 0 || L > S) return fail("xrs_contours_lines: %u lines for %llu segments", L, (unsigned long long)n_segments);
    if (rounds) rounds[0] = lead_rounds, rounds[1] = rank_rounds;
    *n_lines = L;
    *n_points = (uint64_t)S + L;                                  // a line of n segments has n + 1 points
    return 0;
}

int xrs_contours_scatter(const void *data_dev, int dtype, int64_t rows, int64_t cols, uint64_t n_levels, const void *work_dev,
                         void *lines_dev, void *sort_dev, uint64_t n_segments, uint64_t n_lines, const double *transform_host,
                         void *points_dev, void *line_offsets_dev, void *level_offsets_dev, void *closed_dev, void *stream) {
    if (int rc = check_shape("xrs_contours_scatter", rows, cols, n_levels)) return rc;
    if (int rc = check_segments("xrs_contours_scatter", n_segments)) return rc;
    if (!dtype_bytes(dtype)) return fail("xrs_contours_scatter: unsupported dtype code %d", dtype);
    if (n_lines == 0 || n_lines > n_segments)
        return fail("xrs_contours_scatter: %llu lines for %llu segments", (unsigned long long)n_lines, (unsigned long long)n_segments);
    if (rows < 2 || cols < 2 || n_levels == 0) return fail("xrs_contours_scatter: no quad or no level, so no segment");
    if (!data_dev || !work_dev || !lines_dev || !sort_dev || !points_dev || !line_offsets_dev || !level_offsets_dev || !closed_dev)
        return fail("xrs_contours_scatter: null pointer");
    hipStream_t s = as_stream(stream);
    const Work p = carve((void *)work_dev, rows, cols, n_levels);
    const LineWork q = carve_lines(lines_dev, n_segments);
    const SortWork w = carve_sort(sort_dev, n_lines);
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)n_levels};
    const uint32_t S = (uint32_t)n_segments, L = (uint32_t)n_lines, K = (uint32_t)n_levels;
    const unsigned seg_blocks = blocks_for(n_segments);
    const uint32_t *pos = q.buf[2], *first = q.buf[4];
    uint32_t *line_of = q.buf[1], *n_seg = q.buf[3];
    int64_t *line_off = (int64_t *)line_offsets_dev;
    Affine tf{};
    if (transform_host) {
        for (int k = 0; k < 6; ++k) tf.t[k] = transform_host[k];
        tf.on = 1;
    }
    XRS_HIP(hipMemsetAsync(q.words + WORD_SLOTS, 0, 4, s));
    hipLaunchKernelGGL(collect_kernel, dim3(seg_blocks), dim3(THREADS), 0, s, g, (const uint32_t *)q.quad, (const uint32_t *)q.code,
                       (const uint32_t *)q.next, (const uint8_t *)q.start, pos, first, S, w.keys[0], w.vals[0], n_seg,
                       q.words + WORD_SLOTS, L);
    XRS_LAUNCH_CHECK();
    uint32_t slots = 0;
    XRS_HIP(hipMemcpyAsync(&slots, q.words + WORD_SLOTS, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    if (slots != L) return fail("xrs_contours_scatter: %u lines found, %llu expected", slots, (unsigned long long)n_lines);
    int level_bits = 1;
    while (level_bits < 32 && (1ull << level_bits) < n_levels) ++level_bits;
    size_t cub_bytes = w.cub_bytes;
    XRS_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cub_bytes, (const u64 *)w.keys[0], w.keys[1], (const uint32_t *)w.vals[0], w.vals[1],
                                               (size_t)L, 0, 32 + level_bits, s));
    hipLaunchKernelGGL(table_kernel, dim3(blocks_for((uint64_t)L + 1)), dim3(THREADS), 0, s, (const uint32_t *)w.vals[1], L,
                       (const uint32_t *)n_seg, (const uint32_t *)q.pred, line_of, w.count1, (uint8_t *)closed_dev);
    XRS_LAUNCH_CHECK();
    cub_bytes = w.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(w.cub, cub_bytes, w.count1, line_off, (size_t)L + 1, s));
    hipLaunchKernelGGL(level_kernel, dim3(blocks_for((uint64_t)K + 1)), dim3(THREADS), 0, s, (const u64 *)w.keys[1], L, K,
                       (int64_t *)level_offsets_dev);
    XRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(point_kernel, dim3(seg_blocks), dim3(THREADS), 0, s, data_dev, dtype, g, (const double *)p.levels,
                       (const uint32_t *)q.quad, (const uint32_t *)q.code, (const uint32_t *)q.next, (const uint8_t *)q.start, pos, first,
                       (const uint32_t *)line_of, (const int64_t *)line_off, S, L, tf, (double *)points_dev);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

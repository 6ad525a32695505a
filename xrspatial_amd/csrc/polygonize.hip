// polygonize: raster regions to polygon rings.  Reference: xrspatial/experimental/polygonize.py (`_calculate_regions`,
// `_follow`, `_scan`).
//
// The reference's serial scan and its one serial walk per ring have a closed form that this file computes
// in parallel.  Cells are c = x + y * cols, row y increasing "north"; directions are E, N, W, S = 0 .. 3.
//   links    of an unmasked cell c to W and S (and, 8-connected, to SW only without a W link, to SE only without an S
//            link), each where the neighbour is unmasked and close to c: == for integers, else
//            abs_T(d - c) <= 1e-08 + 1e-05 * abs_T(c) (difference and abs in T, threshold and comparison in float64);
//   region   1 + (number of component roots before c's root), root = smallest cell of a linked component; 0 if masked;
//   state    (cell of a region r > 0, direction) whose right-hand cell is outside the domain or not in r; state ids are
//            compact in (cell, direction) order;
//   next     right turn if the forward-right cell is in r, else straight if the forward cell is in r, else left turn;
//            a bijection on states whose cycles are the rings;
//   start    of a ring: its (root cell, E) state if it has one (the exterior), else its smallest W-facing state (a hole);
//   vertex   the tail point of the start state and of every state whose direction differs from its predecessor's, in
//            cycle order from the start, and the start's point once more.
//
// Three calls, each ending in one small device-to-host read that sizes what the next one needs:
//   xrs_polygonize_census  mask plane, link_kernel (64 x 32 tiles, union-find in LDS, union_find.h), merge_kernel (links
//                          that leave a tile, device-scope CAS), roots_kernel + ExclusiveSum (region count),
//                          region_kernel, census_kernel (4 ballots per 64 cells) + ExclusiveSum (state count E);
//   xrs_polygonize_rings   succ_kernel (next, key, emit), leader_round x <= 32 (min of key over each cycle by pointer
//                          doubling), rank_init + rank_round x <= 32 (Wyllie list ranking of the cycles cut in front of
//                          their starts, weight = emits a vertex), collect_kernel (start states -> (region, start) keys),
//                          radix sort, ring_table_kernel + ExclusiveSum (ring and polygon offsets, point count);
//   xrs_polygonize_scatter scatter_kernel (every emitting state writes its point), column_kernel, the offset copies.
// Every loop is bounded, no workgroup waits for another (the only cross-workgroup traffic is the lock-free union of
// merge_kernel and one atomicAdd per ring), and every store is an ordinary vector store.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "union_find.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

#include <type_traits>

using namespace xrs;

namespace {

constexpr int TW = 64, TH = 32, THREADS = 256, WAVES = THREADS / 64;
constexpr int HW = TW + 2, HH = TH + 1;                       // the tile, one halo column each side, one halo row below
constexpr uint32_t NIL = 0xFFFFFFFFu, HOLE_BIT = 0x80000000u;
constexpr int MAX_ROUNDS = 32, ROUND_GROUP = 4;               // a cycle has fewer than 2^31 states
enum { DIR_E = 0, DIR_N = 1, DIR_W = 2, DIR_S = 3 };
enum { LINK_W = 1, LINK_S = 2, LINK_SW = 4, LINK_SE = 8 };

typedef unsigned long long u64;

struct Grid {
    uint32_t rows, cols, tiles_x;
};

// `_is_close(reference = c, value = d)`
template <typename T> __device__ __forceinline__ bool close_to(T c, T d) {
    if constexpr (std::is_integral<T>::value) {
        return d == c;
    } else {
        return (double)__builtin_fabs(d - c) <= threshold((double)__builtin_fabs(c));
    }
}

// ------------------------------------------------------------------ mask: truth is != 0 (NaN is true)
template <typename T> __global__ void __launch_bounds__(THREADS) mask_kernel(const T *__restrict__ m, uint64_t n,
                                                                            uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) out[i] = m[i] != (T)0;
}

// ------------------------------------------------------------------ link: the links of every cell, in-tile unions
template <typename T, bool N8>
__global__ void __launch_bounds__(THREADS) link_kernel(const T *__restrict__ in, const uint8_t *__restrict__ mask, Grid g,
                                                       uint32_t *__restrict__ parent, uint8_t *__restrict__ links) {
    __shared__ T val[HH * HW];
    __shared__ uint8_t ok[HH * HW];
    __shared__ uint32_t par[TH * TW];
    const uint32_t tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
    const uint32_t x0 = tx * TW, y0 = ty * TH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int k = tid; k < HH * HW; k += THREADS) {
        const int hy = k / HW, hx = k - hy * HW;
        const long gy = (long)y0 + hy - 1, gx = (long)x0 + hx - 1;
        bool inside = gy >= 0 && gy < g.rows && gx >= 0 && gx < g.cols;
        if (inside) {
            const size_t c = (size_t)gy * g.cols + gx;
            val[k] = in[c];
            inside = mask ? mask[c] != 0 : true;
        }
        ok[k] = inside;
    }
    for (int k = tid; k < TH * TW; k += THREADS) par[k] = k;
    __syncthreads();

    for (int ly = wave; ly < TH; ly += WAVES) {
        const uint32_t y = y0 + ly, x = x0 + lane;
        if (y >= g.rows || x >= g.cols) continue;
        const int h = (ly + 1) * HW + lane + 1;               // this cell in the halo arrays
        uint32_t bits = 0;
        if (ok[h]) {
            const T v = val[h];
            const bool w = ok[h - 1] && close_to(v, val[h - 1]);              // (a halo cell outside the domain is not ok)
            const bool s = ok[h - HW] && close_to(v, val[h - HW]);
            bool sw = false, se = false;
            if (N8) {
                sw = !w && ok[h - HW - 1] && close_to(v, val[h - HW - 1]);
                se = !s && ok[h - HW + 1] && close_to(v, val[h - HW + 1]);
            }
            bits = (w ? LINK_W : 0) | (s ? LINK_S : 0) | (sw ? LINK_SW : 0) | (se ? LINK_SE : 0);
            const uint32_t self = ly * TW + lane;
            if (w && lane > 0) lds_union(par, self, self - 1);
            if (s && ly > 0) lds_union(par, self, self - TW);
            if (sw && lane > 0 && ly > 0) lds_union(par, self, self - TW - 1);
            if (se && lane < TW - 1 && ly > 0) lds_union(par, self, self - TW + 1);
        }
        links[(size_t)y * g.cols + x] = (uint8_t)bits;
    }
    __syncthreads();

    for (int ly = wave; ly < TH; ly += WAVES) {
        const uint32_t y = y0 + ly, x = x0 + lane;
        if (y < g.rows && x < g.cols) {
            const uint32_t r = lds_find(par, ly * TW + lane);
            const uint32_t ry = r / TW, rx = r - ry * TW;
            parent[y * g.cols + x] = (y0 + ry) * g.cols + x0 + rx;
        }
    }
}

// ------------------------------------------------------------------ merge: the links that leave a tile
// A lane per cell of the tile's bottom row (wave 0) and of its left and right columns (wave 1): the only cells with a link
// that leaves the tile.  A link (c, d) is made as union(parent[c], parent[d]): both tile roots are in the sets of c and d, and
// sets never split, so any value of parent[] read here, stale or not, names the same sets.  A lane skips a root
// pair that the lane before it covers for the same link: along a seam crossed by one region the links of a side collapse to one.
__global__ void __launch_bounds__(128) merge_kernel(const uint8_t *__restrict__ links, Grid g, uint32_t *parent) {
    const uint32_t tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
    const uint32_t x0 = tx * TW, y0 = ty * TH;
    const uint32_t th = min((uint32_t)TH, g.rows - y0), tw = min((uint32_t)TW, g.cols - x0);
    const uint32_t t = threadIdx.x, lane = t & 63;
    uint32_t lx, ly;
    bool on;
    if (t < 64) {
        lx = t, ly = 0, on = lx < tw;
    } else if (t < 96) {
        lx = 0, ly = t - 64, on = ly > 0 && ly < th;
    } else {
        lx = TW - 1, ly = t - 96, on = tw == TW && ly > 0 && ly < th;
    }
    const uint32_t c = on ? (y0 + ly) * g.cols + x0 + lx : 0u;
    const uint32_t bits = on ? links[c] : 0u;
    const uint32_t pc = bits ? parent[c] : NIL;
    const bool leaves[4] = {lx == 0, ly == 0, lx == 0 || ly == 0, lx == TW - 1 || ly == 0};   // W, S, SW, SE
    const uint32_t back[4] = {1u, g.cols, g.cols + 1u, g.cols - 1u};                           // c - d
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool need = (bits >> k & 1) && leaves[k];
        const uint32_t pd = need ? parent[c - back[k]] : NIL;
        const uint32_t prev_pc = __shfl_up(pc, 1), prev_pd = __shfl_up(pd, 1);
        const bool prev_need = __shfl_up((int)need, 1) != 0;
        if (!need || pd == pc) continue;
        if (lane > 0 && prev_need && prev_pc == pc && prev_pd == pd) continue;                 // the lane before covers this pair
        g_union(parent, pc, pd);
    }
}

// ------------------------------------------------------------------ roots: one ballot per 64 cells
__global__ void __launch_bounds__(THREADS) roots_kernel(const uint32_t *__restrict__ parent, const uint8_t *__restrict__ mask,
                                                        uint64_t n, u64 *__restrict__ rootbits, uint32_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool root = i < n && (mask ? mask[i] != 0 : true) && parent[i] == (uint32_t)i;
    const u64 b = __ballot(root);
    if ((threadIdx.x & 63) == 0 && i < n) {
        rootbits[i >> 6] = b;
        cnt[i >> 6] = (uint32_t)__popcll(b);
    }
}

// ------------------------------------------------------------------ region: 1 + roots before the cell's root
__global__ void __launch_bounds__(THREADS) region_kernel(uint32_t *parent, const uint8_t *__restrict__ mask, uint64_t n,
                                                         const u64 *__restrict__ rootbits, const uint32_t *__restrict__ pre,
                                                         uint32_t *__restrict__ region) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    if (mask && !mask[i]) {
        region[i] = 0;
        return;
    }
    // find with halving by plain stores: no union runs in this launch, so every value stored is an ancestor of x
    uint32_t x = (uint32_t)i, p = parent[x];
    while (p != x) {
        const uint32_t gp = parent[p];
        if (gp != p) parent[x] = gp;
        x = gp;
        p = parent[x];
    }
    region[i] = 1u + pre[x >> 6] + (uint32_t)__popcll(rootbits[x >> 6] & ((1ull << (x & 63)) - 1));
}

// ------------------------------------------------------------------ census: which states exist
__device__ __forceinline__ bool in_region(const uint32_t *__restrict__ region, Grid g, long x, long y, uint32_t r) {
    return x >= 0 && y >= 0 && x < (long)g.cols && y < (long)g.rows && region[(size_t)y * g.cols + (size_t)x] == r;
}

__global__ void __launch_bounds__(THREADS) census_kernel(const uint32_t *__restrict__ region, Grid g, uint64_t n,
                                                         u64 *__restrict__ sbits, u64 *__restrict__ scnt) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    bool e = false, nn = false, w = false, s = false;
    if (i < n) {
        const uint32_t r = region[i];
        if (r) {
            const long y = (long)(i / g.cols), x = (long)(i - (uint64_t)y * g.cols);
            e = !in_region(region, g, x, y - 1, r);               // the right-hand cell of each direction
            nn = !in_region(region, g, x + 1, y, r);
            w = !in_region(region, g, x, y + 1, r);
            s = !in_region(region, g, x - 1, y, r);
        }
    }
    const u64 be = __ballot(e), bn = __ballot(nn), bw = __ballot(w), bs = __ballot(s);
    if ((threadIdx.x & 63) == 0 && i < n) {
        const uint64_t word = i >> 6;
        sbits[4 * word + DIR_E] = be;
        sbits[4 * word + DIR_N] = bn;
        sbits[4 * word + DIR_W] = bw;
        sbits[4 * word + DIR_S] = bs;
        scnt[word] = (u64)(__popcll(be) + __popcll(bn) + __popcll(bw) + __popcll(bs));
    }
}

// the 4-bit state mask of cell c and the id of its first state; ids are compact in (cell, direction) order
__device__ __forceinline__ uint32_t state_base(const u64 *__restrict__ sbits, const u64 *__restrict__ spre, uint32_t c,
                                               uint32_t *mask4) {
    const size_t word = c >> 6;
    const int lane = c & 63;
    const u64 below = (1ull << lane) - 1;
    uint32_t id = (uint32_t)spre[word], m = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const u64 b = sbits[4 * word + d];
        id += (uint32_t)__popcll(b & below);
        m |= (uint32_t)((b >> lane) & 1) << d;
    }
    *mask4 = m;
    return id;
}
__device__ __forceinline__ uint32_t state_id(const u64 *__restrict__ sbits, const u64 *__restrict__ spre, uint32_t c, int d) {
    uint32_t m;
    const uint32_t base = state_base(sbits, spre, c, &m);
    return base + (uint32_t)__popc(m & ((1u << d) - 1));
}

// ------------------------------------------------------------------ successor, key, emit
__global__ void __launch_bounds__(THREADS) succ_kernel(const uint32_t *__restrict__ region, Grid g, uint64_t n,
                                                       const u64 *__restrict__ sbits, const u64 *__restrict__ spre,
                                                       const u64 *__restrict__ rootbits, uint32_t *__restrict__ next,
                                                       uint32_t *__restrict__ key, uint8_t *__restrict__ emit) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = (uint32_t)i;
    uint32_t m;
    uint32_t e = state_base(sbits, spre, c, &m);
    if (!m) return;
    const uint32_t r = region[c];
    const long y = (long)(c / g.cols), x = (long)(c - (uint32_t)y * g.cols);
    const bool root = (rootbits[c >> 6] >> (c & 63)) & 1;
    const int fx[4] = {1, 0, -1, 0}, fy[4] = {0, 1, 0, -1};       // forward; the right-hand side of d is forward of d + 3
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (!(m >> d & 1)) continue;
        const int rd = (d + 3) & 3;
        const long ax = x + fx[d], ay = y + fy[d];                // forward
        const long bx = ax + fx[rd], by = ay + fy[rd];            // forward-right
        long nx = x, ny = y;
        int nd = (d + 1) & 3;                                     // left turn
        if (in_region(region, g, bx, by, r)) nx = bx, ny = by, nd = rd;
        else if (in_region(region, g, ax, ay, r)) nx = ax, ny = ay, nd = d;
        const uint32_t e2 = state_id(sbits, spre, (uint32_t)((size_t)ny * g.cols + (size_t)nx), nd);
        next[e] = e2;
        emit[e2] = nd != d;
        key[e] = (d == DIR_E && root) ? e : d == DIR_W ? (HOLE_BIT | e) : NIL;
        ++e;
    }
}

// ------------------------------------------------------------------ ring leader: min of key over each cycle
__global__ void __launch_bounds__(THREADS) leader_round(const uint32_t *__restrict__ nin, const uint32_t *__restrict__ kin,
                                                        uint32_t *__restrict__ nout, uint32_t *__restrict__ kout, uint32_t n_states,
                                                        uint32_t *__restrict__ changed) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    bool ch = false;
    if (e < n_states) {
        const uint32_t nx = nin[e], k = kin[e], k2 = kin[nx];
        ch = k2 < k;
        kout[e] = ch ? k2 : k;
        nout[e] = nin[nx];
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) *changed = 1;
}

__global__ void __launch_bounds__(THREADS) lead_kernel(const uint32_t *__restrict__ key, uint32_t *__restrict__ lead,
                                                       uint32_t n_states) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e < n_states) lead[e] = key[e] & ~HOLE_BIT;
}

// ------------------------------------------------------------------ rank: cycles cut in front of their starts
__global__ void __launch_bounds__(THREADS) rank_init(const uint32_t *__restrict__ next, const uint32_t *__restrict__ lead,
                                                     const uint8_t *__restrict__ emit, uint32_t *__restrict__ nxt,
                                                     uint32_t *__restrict__ val, uint32_t n_states) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= n_states) return;
    const uint32_t nx = next[e];
    nxt[e] = lead[nx] == nx ? NIL : nx;
    val[e] = lead[e] == e ? 1u : (uint32_t)emit[e];               // the start always emits its point
}

__global__ void __launch_bounds__(THREADS) rank_round(const uint32_t *__restrict__ nin, const uint32_t *__restrict__ vin,
                                                      uint32_t *__restrict__ nout, uint32_t *__restrict__ vout, uint32_t n_states,
                                                      uint32_t *__restrict__ changed) {
    const uint32_t e = blockIdx.x * THREADS + threadIdx.x;
    bool ch = false;
    if (e < n_states) {
        const uint32_t nx = nin[e];
        uint32_t v = vin[e];
        ch = nx != NIL;
        if (ch) v += vin[nx];
        vout[e] = v;
        nout[e] = ch ? nin[nx] : NIL;
    }
    if (__ballot(ch) && (threadIdx.x & 63) == 0) *changed = 1;
}

// ------------------------------------------------------------------ ring table
// key of a ring = region << 32 | start state: sorted, a region's exterior ((root, E), the region's smallest state id
// among starts) comes first, then its holes by start cell
__global__ void __launch_bounds__(THREADS) collect_kernel(const uint32_t *__restrict__ region, uint64_t n,
                                                          const u64 *__restrict__ sbits, const u64 *__restrict__ spre,
                                                          const uint32_t *__restrict__ lead, u64 *__restrict__ keys,
                                                          uint32_t *__restrict__ n_rings, uint32_t max_rings) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t m;
    const uint32_t base = state_base(sbits, spre, (uint32_t)i, &m);
    if (!(m & ((1u << DIR_E) | (1u << DIR_W)))) return;           // starts face E or W
    const uint32_t r = region[i];
#pragma unroll
    for (int d = 0; d < 4; d += 2) {
        if (!(m >> d & 1)) continue;
        const uint32_t e = base + (uint32_t)__popc(m & ((1u << d) - 1));
        if (lead[e] != e) continue;
        const uint32_t slot = atomicAdd(n_rings, 1u);
        if (slot < max_rings) keys[slot] = ((u64)r << 32) | e;
    }
}

// sorted ring i: its index for its start state, its point count + 1 (the closing point), and where a polygon begins
__global__ void __launch_bounds__(THREADS) ring_table_kernel(const u64 *__restrict__ keys, uint32_t n_rings,
                                                             const uint32_t *__restrict__ suffix, uint32_t *__restrict__ ring_of,
                                                             u64 *__restrict__ count1, int64_t *__restrict__ poly_off,
                                                             uint32_t n_regions) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i > n_rings) return;
    if (i == n_rings) {
        count1[i] = 0;
        poly_off[n_regions] = n_rings;
        return;
    }
    const u64 k = keys[i];
    const uint32_t e = (uint32_t)k, r = (uint32_t)(k >> 32);
    ring_of[e] = i;
    count1[i] = (u64)suffix[e] + 1;
    if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != r) poly_off[r - 1] = i;
}

// ------------------------------------------------------------------ scatter
struct Affine {
    double t[6];
    int on;
};

// a * i + b * j + c as two separately rounded products and two sums, left to right: hipcc at -O3 would contract them into
// v_fma_f64, which rounds once (__dmul_rn / __dadd_rn are plain * and + in HIP and contract all the same)
__device__ __forceinline__ double affine(double a, double i, double b, double j, double c) {
#pragma clang fp contract(off)
    const double ai = a * i;
    const double bj = b * j;
    const double sum = ai + bj;
    return sum + c;
}

__global__ void __launch_bounds__(THREADS) scatter_kernel(Grid g, uint64_t n, const u64 *__restrict__ sbits,
                                                          const u64 *__restrict__ spre, const uint32_t *__restrict__ lead,
                                                          const uint8_t *__restrict__ emit, const uint32_t *__restrict__ suffix,
                                                          const uint32_t *__restrict__ ring_of, const u64 *__restrict__ ring_off,
                                                          Affine tf, double *__restrict__ points) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = (uint32_t)i;
    uint32_t m;
    uint32_t e = state_base(sbits, spre, c, &m);
    if (!m) return;
    const uint32_t y = c / g.cols, x = c - y * g.cols;
    const int tx[4] = {0, 1, 1, 0}, ty[4] = {0, 0, 1, 1};         // the tail point of a state
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (!(m >> d & 1)) continue;
        const uint32_t s = lead[e];
        const bool start = s == e;
        if (start || emit[e]) {
            double px = (double)(x + tx[d]), py = (double)(y + ty[d]);
            if (tf.on) {
                const double qx = affine(tf.t[0], px, tf.t[1], py, tf.t[2]), qy = affine(tf.t[3], px, tf.t[4], py, tf.t[5]);
                px = qx, py = qy;
            }
            const uint32_t count = suffix[s];
            const u64 off = ring_off[ring_of[s]];
            const u64 at = off + (count - suffix[e]);
            points[2 * at] = px;
            points[2 * at + 1] = py;
            if (start) {                                          // the closing point
                points[2 * (off + count)] = px;
                points[2 * (off + count) + 1] = py;
            }
        }
        ++e;
    }
}

template <typename U>
__global__ void __launch_bounds__(THREADS) column_kernel(const U *__restrict__ in, const uint32_t *__restrict__ region,
                                                         const u64 *__restrict__ rootbits, uint64_t n, U *__restrict__ column) {
    const uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < n && ((rootbits[i >> 6] >> (i & 63)) & 1)) column[region[i] - 1] = in[i];
}

// ------------------------------------------------------------------ workspaces
struct Work {                                                     // of xrs_polygonize_census; the region plane comes first
    size_t n, words;
    uint32_t *region, *parent, *cnt;                              // cnt[words], scnt[words]: the totals
    uint8_t *mask, *links;
    u64 *rootbits, *sbits, *scnt;
    void *cub;
    size_t cub_bytes, total;
};

Work carve(void *base, uint64_t rows, uint64_t cols) {
    Carver c(base);
    Work p{};
    p.n = rows * cols;
    p.words = (p.n + 63) / 64;
    p.region = c.take<uint32_t>(p.n);
    p.parent = c.take<uint32_t>(p.n);
    p.mask = c.take<uint8_t>(p.n);
    p.links = c.take<uint8_t>(p.n);
    p.rootbits = c.take<u64>(p.words);
    p.cnt = c.take<uint32_t>(p.words + 1);
    p.sbits = c.take<u64>(p.words * 4);
    p.scnt = c.take<u64>(p.words + 1);
    size_t a = 0, b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)(p.words + 1));
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (u64 *)nullptr, (u64 *)nullptr, (size_t)(p.words + 1));
    p.cub_bytes = a > b ? a : b;
    p.cub = c.take<char>(p.cub_bytes > 0 ? p.cub_bytes : 1);
    p.total = c.at();
    return p;
}

struct RingWork {                                                 // of xrs_polygonize_rings
    size_t n_states, max_rings;
    uint32_t *next, *buf[4], *lead, *words;
    uint8_t *emit;
    u64 *keys[2], *count1, *ring_off;
    int64_t *poly_off;
    void *cub;
    size_t cub_bytes, total;
};
constexpr int WORD_RINGS = 0, WORD_CHANGED = 8, N_WORDS = 8 + 2 * MAX_ROUNDS + 8;

RingWork carve_rings(void *base, uint64_t n_states) {
    Carver c(base);
    RingWork p{};
    p.n_states = n_states;
    p.max_rings = n_states / 4 + 1;                               // a ring has at least 4 states
    p.next = c.take<uint32_t>(n_states);
    for (int k = 0; k < 4; ++k) p.buf[k] = c.take<uint32_t>(n_states);
    p.lead = c.take<uint32_t>(n_states);
    p.emit = c.take<uint8_t>(n_states);
    for (int k = 0; k < 2; ++k) p.keys[k] = c.take<u64>(p.max_rings);
    p.count1 = c.take<u64>(p.max_rings + 1);
    p.ring_off = c.take<u64>(p.max_rings + 1);
    p.poly_off = c.take<int64_t>(p.max_rings + 1);
    p.words = c.take<uint32_t>(N_WORDS);
    size_t a = 0, b = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, (u64 *)nullptr, (u64 *)nullptr, (size_t)p.max_rings, 0, 64);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (u64 *)nullptr, (u64 *)nullptr, (size_t)(p.max_rings + 1));
    p.cub_bytes = a > b ? a : b;
    p.cub = c.take<char>(p.cub_bytes > 0 ? p.cub_bytes : 1);
    p.total = c.at();
    return p;
}

int check_shape(const char *fn, int64_t rows, int64_t cols) {
    if (rows < 1 || cols < 1) return fail("%s: the raster must have a shape of at least (1, 1)", fn);
    if ((uint64_t)rows > 0xFFFFFFFFull / (uint64_t)cols)
        return fail("%s: %lld x %lld cells exceed the 32-bit cell index (at most 2^32 - 1 cells)", fn, (long long)rows,
                    (long long)cols);
    return 0;
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }

template <typename T>
int census_impl(const T *in, const uint8_t *mask, int64_t rows, int64_t cols, int n8, void *work, uint64_t *n_regions,
                uint64_t *n_states, hipStream_t s) {
    const Work p = carve(work, rows, cols);
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)((cols + TW - 1) / TW)};
    const size_t tiles = (size_t)g.tiles_x * ((rows + TH - 1) / TH);
    const unsigned cell_blocks = blocks_for(p.n);
    XRS_HIP(hipMemsetAsync(p.cnt + p.words, 0, 4, s));
    XRS_HIP(hipMemsetAsync(p.scnt + p.words, 0, 8, s));
    if (n8)
        hipLaunchKernelGGL((link_kernel<T, true>), dim3((unsigned)tiles), dim3(THREADS), 0, s, in, mask, g, p.parent, p.links);
    else
        hipLaunchKernelGGL((link_kernel<T, false>), dim3((unsigned)tiles), dim3(THREADS), 0, s, in, mask, g, p.parent, p.links);
    XRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)tiles), dim3(128), 0, s, p.links, g, p.parent);
    XRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(roots_kernel, dim3(cell_blocks), dim3(THREADS), 0, s, p.parent, mask, (uint64_t)p.n, p.rootbits, p.cnt);
    XRS_LAUNCH_CHECK();
    size_t cub_bytes = p.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(p.cub, cub_bytes, p.cnt, p.cnt, (size_t)(p.words + 1), s));
    hipLaunchKernelGGL(region_kernel, dim3(cell_blocks), dim3(THREADS), 0, s, p.parent, mask, (uint64_t)p.n, p.rootbits, p.cnt, p.region);
    XRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(census_kernel, dim3(cell_blocks), dim3(THREADS), 0, s, p.region, g, (uint64_t)p.n, p.sbits, p.scnt);
    XRS_LAUNCH_CHECK();
    cub_bytes = p.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(p.cub, cub_bytes, p.scnt, p.scnt, (size_t)(p.words + 1), s));
    uint32_t regions_total = 0;
    u64 states_total = 0;
    XRS_HIP(hipMemcpyAsync(&regions_total, p.cnt + p.words, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipMemcpyAsync(&states_total, p.scnt + p.words, 8, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    *n_regions = regions_total;
    *n_states = states_total;
    return 0;
}

template <typename T> int mask_impl(const T *m, uint64_t n, uint8_t *out, hipStream_t s) {
    hipLaunchKernelGGL(mask_kernel<T>, dim3(blocks_for(n)), dim3(THREADS), 0, s, m, n, out);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t xrs_polygonize_workspace_bytes(int64_t rows, int64_t cols) {
    if (rows < 1 || cols < 1 || (uint64_t)rows > 0xFFFFFFFFull / (uint64_t)cols) return 0;
    return carve(nullptr, (uint64_t)rows, (uint64_t)cols).total;
}

size_t xrs_polygonize_rings_workspace_bytes(uint64_t n_states) {
    if (n_states == 0 || n_states > XRS_POLYGONIZE_MAX_STATES) return 0;
    return carve_rings(nullptr, n_states).total;
}

int xrs_polygonize_census(const void *data_dev, int dtype, const void *mask_dev, int mask_dtype, int64_t rows, int64_t cols,
                          int connectivity, void *work_dev, uint64_t *n_regions, uint64_t *n_states, void *stream) {
    if (int rc = check_shape("xrs_polygonize_census", rows, cols)) return rc;
    if (connectivity != 4 && connectivity != 8)
        return fail("xrs_polygonize_census: connectivity must be either 4 or 8, not %d", connectivity);
    if (!dtype_bytes(dtype)) return fail("xrs_polygonize_census: unsupported dtype code %d", dtype);
    if (mask_dev && !dtype_bytes(mask_dtype)) return fail("xrs_polygonize_census: unsupported mask dtype code %d", mask_dtype);
    if (!data_dev || !work_dev || !n_regions || !n_states) return fail("xrs_polygonize_census: null pointer");
    *n_regions = *n_states = 0;
    hipStream_t s = as_stream(stream);
    const Work p = carve(work_dev, rows, cols);
    uint8_t *mask = nullptr;
    int rc = 0;                                                   // (both codes were checked above)
    if (mask_dev) {
        mask = p.mask;
        with_dtype(mask_dtype, [&](auto t) { rc = mask_impl((const dtype_of<decltype(t)> *)mask_dev, p.n, mask, s); });
        if (rc) return rc;
    }
    const int n8 = connectivity == 8;
    with_dtype(dtype, [&](auto t) {
        rc = census_impl((const dtype_of<decltype(t)> *)data_dev, mask, rows, cols, n8, work_dev, n_regions, n_states, s);
    });
    return rc;
}

int xrs_polygonize_rings(int64_t rows, int64_t cols, const void *work_dev, void *rings_dev, uint64_t n_states,
                         uint64_t n_regions, uint64_t *n_rings, uint64_t *n_points, int *rounds, void *stream) {
    if (int rc = check_shape("xrs_polygonize_rings", rows, cols)) return rc;
    if (n_states == 0 || n_states > XRS_POLYGONIZE_MAX_STATES)
        return fail("xrs_polygonize_rings: %llu boundary states, outside 1 .. %llu", (unsigned long long)n_states,
                    (unsigned long long)XRS_POLYGONIZE_MAX_STATES);
    if (!work_dev || !rings_dev || !n_rings || !n_points) return fail("xrs_polygonize_rings: null pointer");
    *n_rings = *n_points = 0;
    hipStream_t s = as_stream(stream);
    const Work p = carve((void *)work_dev, rows, cols);
    const RingWork q = carve_rings(rings_dev, n_states);
    if (n_regions == 0 || n_regions > q.max_rings) return fail("xrs_polygonize_rings: %llu regions do not fit %llu states",
                                                               (unsigned long long)n_regions, (unsigned long long)n_states);
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)((cols + TW - 1) / TW)};
    const unsigned cell_blocks = blocks_for(p.n), state_blocks = blocks_for(n_states);
    const uint32_t E = (uint32_t)n_states;
    uint32_t host_words[N_WORDS];

    XRS_HIP(hipMemsetAsync(q.words, 0, N_WORDS * 4, s));
    // next -> `next`, key -> buf[2]
    hipLaunchKernelGGL(succ_kernel, dim3(cell_blocks), dim3(THREADS), 0, s, p.region, g, (uint64_t)p.n, p.sbits, p.scnt, p.rootbits, q.next,
                       q.buf[2], q.emit);
    XRS_LAUNCH_CHECK();

    // leader: (next, key) double-buffered in (buf[0] | buf[1], buf[2] | buf[3]); round 0 reads `next` itself
    const uint32_t *nin = q.next, *kin = q.buf[2];
    int done_rounds = 0, key_at = 2;
    bool settled = false;
    while (!settled && done_rounds < MAX_ROUNDS) {
        const int first = done_rounds;
        for (int k = 0; k < ROUND_GROUP && done_rounds < MAX_ROUNDS; ++k, ++done_rounds) {
            uint32_t *nout = q.buf[done_rounds & 1], *kout = q.buf[2 + ((done_rounds + 1) & 1)];
            hipLaunchKernelGGL(leader_round, dim3(state_blocks), dim3(THREADS), 0, s, nin, kin, nout, kout, E,
                               q.words + WORD_CHANGED + done_rounds);
            XRS_LAUNCH_CHECK();
            nin = nout, kin = kout, key_at = 2 + ((done_rounds + 1) & 1);
        }
        XRS_HIP(hipMemcpyAsync(host_words, q.words, N_WORDS * 4, hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        for (int k = first; k < done_rounds; ++k) settled |= host_words[WORD_CHANGED + k] == 0;   // a still round: minima final
    }
    if (!settled) return fail("xrs_polygonize_rings: ring leaders did not settle in %d rounds", MAX_ROUNDS);
    if (rounds) rounds[0] = done_rounds;
    hipLaunchKernelGGL(lead_kernel, dim3(state_blocks), dim3(THREADS), 0, s, (const uint32_t *)q.buf[key_at], q.lead, E);
    XRS_LAUNCH_CHECK();

    // rank: (nxt, val) double-buffered in (buf[0] | buf[1], buf[2] | buf[3])
    hipLaunchKernelGGL(rank_init, dim3(state_blocks), dim3(THREADS), 0, s, (const uint32_t *)q.next, (const uint32_t *)q.lead,
                       (const uint8_t *)q.emit, q.buf[0], q.buf[2], E);
    XRS_LAUNCH_CHECK();
    int rank_rounds = 0, at = 0;
    settled = false;
    while (!settled && rank_rounds < MAX_ROUNDS) {
        const int first = rank_rounds;
        for (int k = 0; k < ROUND_GROUP && rank_rounds < MAX_ROUNDS; ++k, ++rank_rounds) {
            hipLaunchKernelGGL(rank_round, dim3(state_blocks), dim3(THREADS), 0, s, (const uint32_t *)q.buf[at],
                               (const uint32_t *)q.buf[2 + at], q.buf[at ^ 1], q.buf[2 + (at ^ 1)], E,
                               q.words + WORD_CHANGED + MAX_ROUNDS + rank_rounds);
            XRS_LAUNCH_CHECK();
            at ^= 1;
        }
        XRS_HIP(hipMemcpyAsync(host_words, q.words, N_WORDS * 4, hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        for (int k = first; k < rank_rounds; ++k) settled |= host_words[WORD_CHANGED + MAX_ROUNDS + k] == 0;
    }
    if (!settled) return fail("xrs_polygonize_rings: ring ranks did not settle in %d rounds", MAX_ROUNDS);
    if (rounds) rounds[1] = rank_rounds;
    // rounds run in groups of ROUND_GROUP, an even number, and a round after the last change copies its input: the ranks
    // are in buf[2], and buf[0] (list pointers, spent) is free for the ring index -- where xrs_polygonize_scatter looks
    static_assert(ROUND_GROUP % 2 == 0 && MAX_ROUNDS % ROUND_GROUP == 0, "the rank buffers' parity");
    if (at != 0) return fail("xrs_polygonize_rings: odd number of rank rounds");
    const uint32_t *suffix = q.buf[2];                            // emitting states from each state to its ring's end
    uint32_t *ring_of = q.buf[0];

    hipLaunchKernelGGL(collect_kernel, dim3(cell_blocks), dim3(THREADS), 0, s, p.region, (uint64_t)p.n, p.sbits, p.scnt,
                       (const uint32_t *)q.lead, q.keys[0], q.words + WORD_RINGS, (uint32_t)q.max_rings);
    XRS_LAUNCH_CHECK();
    XRS_HIP(hipMemcpyAsync(host_words, q.words, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    const uint32_t R = host_words[WORD_RINGS];
    if (R == 0 || R > q.max_rings || R < n_regions)
        return fail("xrs_polygonize_rings: %u rings for %llu states and %llu regions", R, (unsigned long long)n_states,
                    (unsigned long long)n_regions);
    size_t cub_bytes = q.cub_bytes;
    XRS_HIP(hipcub::DeviceRadixSort::SortKeys(q.cub, cub_bytes, (const u64 *)q.keys[0], q.keys[1], (size_t)R, 0, 64, s));
    hipLaunchKernelGGL(ring_table_kernel, dim3(blocks_for((uint64_t)R + 1)), dim3(THREADS), 0, s, (const u64 *)q.keys[1], R, suffix,
                       ring_of, q.count1, q.poly_off, (uint32_t)n_regions);
    XRS_LAUNCH_CHECK();
    cub_bytes = q.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(q.cub, cub_bytes, q.count1, q.ring_off, (size_t)R + 1, s));
    u64 total = 0;
    XRS_HIP(hipMemcpyAsync(&total, q.ring_off + R, 8, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    *n_rings = R;
    *n_points = total;
    return 0;
}

int xrs_polygonize_scatter(const void *data_dev, int dtype, int64_t rows, int64_t cols, const void *work_dev,
                           const void *rings_dev, uint64_t n_states, uint64_t n_regions, uint64_t n_rings,
                           const double *transform_host, void *points_dev, void *ring_offsets_dev, void *polygon_offsets_dev,
                           void *column_dev, void *stream) {
    if (int rc = check_shape("xrs_polygonize_scatter", rows, cols)) return rc;
    const int item = dtype_bytes(dtype);
    if (!item) return fail("xrs_polygonize_scatter: unsupported dtype code %d", dtype);
    if (n_states == 0 || n_states > XRS_POLYGONIZE_MAX_STATES) return fail("xrs_polygonize_scatter: bad state count");
    const RingWork q = carve_rings((void *)rings_dev, n_states);
    if (n_rings == 0 || n_rings > q.max_rings || n_regions == 0 || n_regions > n_rings)
        return fail("xrs_polygonize_scatter: bad ring or region count");
    if (!data_dev || !work_dev || !rings_dev || !points_dev || !ring_offsets_dev || !polygon_offsets_dev || !column_dev)
        return fail("xrs_polygonize_scatter: null pointer");
    hipStream_t s = as_stream(stream);
    const Work p = carve((void *)work_dev, rows, cols);
    const uint32_t *suffix = q.buf[2], *ring_of = q.buf[0];
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)((cols + TW - 1) / TW)};
    Affine tf{};
    if (transform_host) {
        for (int k = 0; k < 6; ++k) tf.t[k] = transform_host[k];
        tf.on = 1;
    }
    const unsigned cell_blocks = blocks_for(p.n);
    hipLaunchKernelGGL(scatter_kernel, dim3(cell_blocks), dim3(THREADS), 0, s, g, (uint64_t)p.n, p.sbits, p.scnt, q.lead, q.emit, suffix,
                       ring_of, q.ring_off, tf, (double *)points_dev);
    XRS_LAUNCH_CHECK();
#define XRS_POLY_COLUMN(U)                                                                                                   \
    hipLaunchKernelGGL(column_kernel<U>, dim3(cell_blocks), dim3(THREADS), 0, s, (const U *)data_dev, p.region, p.rootbits,  \
                       (uint64_t)p.n, (U *)column_dev)
    if (item == 1) XRS_POLY_COLUMN(uint8_t);
    else if (item == 2) XRS_POLY_COLUMN(uint16_t);
    else if (item == 4) XRS_POLY_COLUMN(uint32_t);
    else XRS_POLY_COLUMN(u64);
#undef XRS_POLY_COLUMN
    XRS_LAUNCH_CHECK();
    XRS_HIP(hipMemcpyAsync(ring_offsets_dev, q.ring_off, (n_rings + 1) * 8, hipMemcpyDeviceToDevice, s));
    XRS_HIP(hipMemcpyAsync(polygon_offsets_dev, q.poly_off, (n_regions + 1) * 8, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // extern "C"

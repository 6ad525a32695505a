// stream_order / stream_link / watershed / flow_length: what follows flow_accumulation in a D8 toolbox.
//
// The reference has none of them; the result is a written rule (xrspatial_amd/hydrology.py, tests/streams_oracle.py).  All of it
// is §6m's machinery -- uint32 pointers, NIL, pointer doubling in at most bit_length rounds, live pointers counted by every
// round and read by the host every two rounds, no loop on the device that depends on the data -- with forest arithmetic on top.
//
//   stream network  mark     a cell is a stream cell when its code is not NaN and float64(accumulation) >= threshold; every
//                            non-NaN code is checked as flow_decode_kernel checks it.
//                   scan     hipCUB's exclusive sum of the marks, in place, over cells + 1 words: slot[u] = stream cells in front
//                            of u in row-major order, slot[cells] = n, and u is a stream cell iff slot[u + 1] != slot[u].
//                   compact  one pass over the raster.  A stream cell writes, at its slot: its cell index, its stream parent's
//                            SLOT (the downstream cell if that is a stream cell, else NIL), the mask of its eight neighbours
//                            that are stream cells pointing at it (its children; no atomics) and `up`, the slot of the single
//                            child.  Everything after this runs on the n slots, not on the raster.
//                   weights  §6m's round with S started at a weight: uint32 adds, exact and order-free.  Shreve: the weight is
//                            1 at a cell without children.  This run also finds every ring of stream cells (a parent pointer
//                            still live after bit_length(n) rounds) and counts the sources.
//                   Strahler by level sets.  A_k = cells of order >= k, A_1 = all.  J_k = cells with two or more children in A_k;
//                            A_{k+1} = cells whose accumulated weight 1[J_k] is > 0 (order >= k + 1 iff two children have order
//                            >= k or one child has order >= k + 1).  A level: one pass that counts children (only a junction
//                            looks), one accumulation, one pass that raises the order plane.  The host reads |J_k| once a level
//                            and stops at 0; order k needs 2^(k - 1) sources, so there are at most bit_length(sources) <= 32.
//                   heads    up-pointer jumping, §6m's `root` recurrence on `up`: at most bit_length(n) rounds.  Slots are in
//                            row-major order of their cells, so an exclusive sum of the head flags over the slots numbers the
//                            heads as rule 10 asks.
//                   finish   one streaming pass per raster: float64, NaN off the streams.
//   watershed       §6m's root doubling on the whole raster with the pointer of every pour point cut at decode, then one gather:
//                   float32(pour_points[root]) where the root is a pour point.
//   flow_length     doubling that carries three uint32 step counts (E/W, N/S, diagonal) beside the pointer:
//                   cnt_{k+1}[u] = cnt_k[u] + cnt_k[anc_k[u]].  The counts of another cell are read, so they ping-pong.  The
//                   finish pass evaluates fl(fl(fl(nx cx) + fl(ny cy)) + fl(nd dg)); contraction is off for the whole file.
//
// A block takes SPAN * ITEMS = 2048 cells (or slots) in every kernel here, as in hydrology.hip.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "value_match.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr int SPAN = 256;                       // threads per block: four waves
constexpr unsigned NIL = 0xffffffffu;
constexpr int MAX_ROUNDS = XRS_FLOW_MAX_ROUNDS;
constexpr int ITEMS = 8;                        // cells per thread, SPAN apart
constexpr int GROUP = 2;                        // rounds between two looks at the live counts
constexpr int SLOTS = 64, SLOT_STRIDE = 64;     // a round's live count, spread as in hydrology.hip
constexpr int ROW_WORDS = SLOTS * SLOT_STRIDE;
constexpr int BAD_WORD = (MAX_ROUNDS + 1) * ROW_WORDS;                   // the invalid-code word,
constexpr int SUM_WORD = BAD_WORD + 64;                                  // a pass's own count (weights, pour points),
constexpr int HEAD_WORDS = SUM_WORD + 64;
constexpr int MAX_LEVELS = 32;
static_assert(136 <= XRS_STREAM_STATUS_WORDS && 40 + MAX_ROUNDS <= XRS_FLOW_STATUS_WORDS, "status layout");

__device__ __forceinline__ double nan_f64() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ unsigned wave_count(bool live) { return (unsigned)__popcll(__ballot(live)); }
__device__ __forceinline__ void add_count(unsigned n, unsigned *__restrict__ slots) {
    if (n != 0 && (threadIdx.x & 63) == 0) atomicAdd(slots + ((blockIdx.x * (SPAN / 64) + (threadIdx.x >> 6)) & (SLOTS - 1)) * SLOT_STRIDE, n);
}
__device__ __forceinline__ void add_word(unsigned n, unsigned *__restrict__ word) {
    if (n != 0 && (threadIdx.x & 63) == 0) atomicAdd(word, n);
}

// neighbour k in the rule's order E, SE, S, SW, W, NW, N, NE (code 1 << k); the neighbour at k points back with code 1 << (k ^ 4)
__device__ __forceinline__ int drow(int k) { return (k >= 1 && k <= 3) - (k >= 5 && k <= 7); }
__device__ __forceinline__ int dcol(int k) { return (k == 0 || k == 1 || k == 7) - (k >= 3 && k <= 5); }

// the step a code names: 0 .. 7, -1 for 0 and NaN; any other value sets `bad` (flow_decode_kernel's test)
__device__ __forceinline__ int step_of(float code, bool &bad) {
    if (code == 1.0f) return 0;
    if (code == 2.0f) return 1;
    if (code == 4.0f) return 2;
    if (code == 8.0f) return 3;
    if (code == 16.0f) return 4;
    if (code == 32.0f) return 5;
    if (code == 64.0f) return 6;
    if (code == 128.0f) return 7;
    bad |= code == code && code != 0.0f;
    return -1;
}
// the cell that step k leads to from u, or -1 beyond the raster (cells and cols fit 32 bits: no 64-bit division)
__device__ __forceinline__ long neighbour(long u, int k, long rows, long cols) {
    const unsigned ui = (unsigned)u / (unsigned)cols;
    const long i = ui, j = u - (long)ui * cols;
    const long r = i + drow(k), q = j + dcol(k);
    return (r >= 0 && r < rows && q >= 0 && q < cols) ? r * cols + q : -1;
}

// proximity's rule 1: non-zero and finite, or equal to one of `values` under NumPy's == (value_match.h)
template <typename T>
__device__ __forceinline__ bool target_value(T v, const void *__restrict__ values, int kind, int n) {
    if (n == 0) {
        if constexpr (std::is_floating_point<T>::value) return v != (T)0 && isfinite(v);
        else return v != (T)0;
    }
    return matches_any<T>(v, values, kind, n);
}

// ------------------------------------------------------------------ the doubling round, on cells or on slots
// flow_round_kernel's recurrence (hydrology.hip): ACC folds the increments of the round before into S and adds S to the
// ancestor's next increment; ROOT carries root_{k+1}[u] = root_k[root_k[u]].
template <bool ACC, bool ROOT>
__global__ void __launch_bounds__(SPAN) jump_round_kernel(long count, const unsigned *__restrict__ anc, unsigned *__restrict__ anc_next,
                                                          unsigned *__restrict__ S, unsigned *__restrict__ D_prev, unsigned *__restrict__ D_cur,
                                                          const unsigned *__restrict__ root, unsigned *__restrict__ root_next,
                                                          unsigned *__restrict__ live_next) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    unsigned a[ITEMS], s[ITEMS], add[ITEMS], r[ITEMS], next[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        a[it] = NIL; s[it] = add[it] = r[it] = 0u;
        if (u < count) {
            a[it] = anc[u];
            if (ACC) { add[it] = D_prev[u]; s[it] = S[u]; }
            if (ROOT) r[it] = root[u];
        }
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        next[it] = a[it] != NIL ? anc[a[it]] : NIL;
        if (ROOT && a[it] != NIL) r[it] = root[r[it]];
    }
    unsigned live = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (u < count) {
            if (ACC) {
                if (add[it]) { s[it] += add[it]; S[u] = s[it]; D_prev[u] = 0u; }
                if (a[it] != NIL) atomicAdd(D_cur + a[it], s[it]);
            }
            anc_next[u] = next[it];
            if (ROOT) root_next[u] = r[it];
        }
        live += wave_count(next[it] != NIL);
    }
    add_count(live, live_next);
}

// ------------------------------------------------------------------ stream network: mark, compact
template <typename TA>
__global__ void __launch_bounds__(SPAN) stream_mark_kernel(const float *__restrict__ dir, const TA *__restrict__ accum, long cells, double threshold,
                                                           unsigned *__restrict__ slot, unsigned *__restrict__ head) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    float c[ITEMS];
    TA a[ITEMS];
    bool bad = false;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        c[it] = u < cells ? dir[u] : nan_f32();
        a[it] = u < cells ? accum[u] : (TA)0;
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        (void)step_of(c[it], bad);
        if (u < cells) slot[u] = (c[it] == c[it] && (double)a[it] >= threshold) ? 1u : 0u;     // (false on a NaN accumulation)
    }
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(head + BAD_WORD, 1u);
}

// slot: the scanned marks, cells + 1 words
__global__ void __launch_bounds__(SPAN) stream_compact_kernel(const float *__restrict__ dir, long rows, long cols, const unsigned *__restrict__ slot,
                                                              unsigned *__restrict__ cell, unsigned *__restrict__ par, unsigned *__restrict__ up,
                                                              unsigned char *__restrict__ cmask) {
    const long cells = rows * cols;
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    unsigned s0[ITEMS], s1[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        s0[it] = s1[it] = 0u;
        if (u < cells) { s0[it] = slot[u]; s1[it] = slot[u + 1]; }
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (s0[it] == s1[it]) continue;                                  // no stream cell (or beyond the raster)
        bool bad = false;
        const int k = step_of(dir[u], bad);
        unsigned parent = NIL;
        if (k >= 0) {
            const long v = neighbour(u, k, rows, cols);
            if (v >= 0) {
                const unsigned v0 = slot[v], v1 = slot[v + 1];
                if (v0 != v1) parent = v0;                               // (a NaN neighbour is no stream cell)
            }
        }
        unsigned mask = 0u, child = NIL;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const long v = neighbour(u, n, rows, cols);
            if (v < 0) continue;
            const unsigned v0 = slot[v], v1 = slot[v + 1];
            if (v0 != v1 && dir[v] == (float)(1 << (n ^ 4))) { mask |= 1u << n; child = v0; }
        }
        const unsigned s = s0[it];
        cell[s] = (unsigned)u;
        par[s] = parent;
        up[s] = __popc(mask) == 1 ? child : NIL;
        cmask[s] = (unsigned char)mask;
    }
}

// ------------------------------------------------------------------ stream network: on the slots
// Starts an accumulation: anc_0 = the stream parent, S = the weight, both increment planes 0.  LEVEL == 0: the weight is 1 at a
// source (Shreve).  LEVEL == k > 0: 1 at the cells of J_k, those with at least two children of order >= k.
__global__ void __launch_bounds__(SPAN) forest_init_kernel(long n, unsigned level, long cols, const unsigned *__restrict__ slot,
                                                           const unsigned *__restrict__ cell, const unsigned *__restrict__ par,
                                                           const unsigned char *__restrict__ cmask, const unsigned *__restrict__ order,
                                                           unsigned *__restrict__ anc, unsigned *__restrict__ S, unsigned *__restrict__ D0,
                                                           unsigned *__restrict__ D1, unsigned *__restrict__ head) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    unsigned live = 0, total = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long s = first + it * SPAN;
        unsigned p = NIL, w = 0u;
        if (s < n) {
            p = par[s];
            const unsigned mask = cmask[s];
            if (level == 0) w = mask == 0u;
            else if (__popc(mask) >= 2) {
                const long u = cell[s];
                int above = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (mask >> k & 1u) above += order[slot[u + drow(k) * cols + dcol(k)]] >= level;
                w = above >= 2;
            }
            anc[s] = p; S[s] = w; D0[s] = 0u; D1[s] = 0u;
        }
        live += wave_count(p != NIL);
        total += wave_count(w != 0u);
    }
    add_count(live, head);
    add_word(total, head + SUM_WORD);
}

// what an accumulation leaves: LEVEL == 0 keeps the sums (Shreve) and starts the order plane at 1; LEVEL == k raises the order
// to k + 1 where the sum is > 0
__global__ void __launch_bounds__(SPAN) forest_keep_kernel(long n, unsigned level, const unsigned *__restrict__ S, const unsigned *__restrict__ D,
                                                           unsigned *__restrict__ shreve, unsigned *__restrict__ order) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long s = first + it * SPAN;
        if (s >= n) break;
        const unsigned sum = S[s] + D[s];
        if (level == 0) { shreve[s] = sum; order[s] = 1u; }
        else if (sum != 0u) order[s] = level + 1u;
    }
}

// heads: anc_0 = up, root_0 = up or the slot itself; flag[s] = 1 at a head (0 or >= 2 children), for the scan of the ids
__global__ void __launch_bounds__(SPAN) head_init_kernel(long n, const unsigned *__restrict__ up, const unsigned char *__restrict__ cmask,
                                                         unsigned *__restrict__ anc, unsigned *__restrict__ root, unsigned *__restrict__ flag,
                                                         unsigned *__restrict__ head) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    unsigned live = 0, total = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long s = first + it * SPAN;
        unsigned p = NIL;
        bool is_head = false;
        if (s < n) {
            p = up[s];
            is_head = __popc((unsigned)cmask[s]) != 1;
            anc[s] = p; root[s] = p != NIL ? p : (unsigned)s; flag[s] = is_head;
        }
        live += wave_count(p != NIL);
        total += wave_count(is_head);
    }
    add_count(live, head);
    add_word(total, head + SUM_WORD);
}

// (a null plane is not asked for)
__global__ void __launch_bounds__(SPAN) stream_finish_kernel(long cells, const unsigned *__restrict__ slot, const unsigned *__restrict__ order,
                                                             const unsigned *__restrict__ shreve, const unsigned *__restrict__ root,
                                                             const unsigned *__restrict__ ids, double *__restrict__ strahler_out,
                                                             double *__restrict__ shreve_out, double *__restrict__ link_out) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    unsigned s0[ITEMS], s1[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        s0[it] = s1[it] = 0u;
        if (u < cells) { s0[it] = slot[u]; s1[it] = slot[u + 1]; }
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (u >= cells) break;
        const bool on = s0[it] != s1[it];
        const unsigned s = s0[it];
        if (strahler_out) st_stream(strahler_out + u, on ? (double)order[s] : nan_f64());
        if (shreve_out) st_stream(shreve_out + u, on ? (double)shreve[s] : nan_f64());
        if (link_out) st_stream(link_out + u, on ? (double)ids[root[s]] + 1.0 : nan_f64());
    }
}

// ------------------------------------------------------------------ watershed
template <typename T>
__global__ void __launch_bounds__(SPAN) shed_decode_kernel(const float *__restrict__ dir, const T *__restrict__ pour, const void *__restrict__ values,
                                                           int kind, int n_values, long rows, long cols, unsigned *__restrict__ head,
                                                           unsigned *__restrict__ anc, unsigned *__restrict__ root) {
    const long cells = rows * cols;
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    float c[ITEMS], cv[ITEMS];
    T p[ITEMS];
    long v[ITEMS];
    bool bad = false;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        c[it] = u < cells ? dir[u] : nan_f32();
        p[it] = u < cells ? pour[u] : (T)0;
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const int k = step_of(c[it], bad);
        v[it] = k >= 0 ? neighbour(first + it * SPAN, k, rows, cols) : -1;
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) cv[it] = v[it] >= 0 ? dir[v[it]] : nan_f32();
    unsigned live = 0, pours = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        const bool is_pour = c[it] == c[it] && target_value<T>(p[it], values, kind, n_values);
        const unsigned down = (cv[it] == cv[it] && !is_pour) ? (unsigned)v[it] : NIL;      // a pour point's pointer is cut
        if (u < cells) {
            anc[u] = down;
            root[u] = down != NIL ? down : (unsigned)u;
        }
        live += wave_count(down != NIL);
        pours += wave_count(is_pour);
    }
    add_count(live, head);
    add_word(pours, head + SUM_WORD);
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(head + BAD_WORD, 1u);
}

template <typename T>
__global__ void __launch_bounds__(SPAN) shed_gather_kernel(const float *__restrict__ dir, const T *__restrict__ pour, const void *__restrict__ values,
                                                           int kind, int n_values, long cells, const unsigned *__restrict__ root,
                                                           float *__restrict__ out) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    float c[ITEMS];
    unsigned r[ITEMS];
    T p[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        c[it] = nan_f32(); r[it] = 0u;
        if (u < cells) { c[it] = dir[u]; r[it] = root[u]; }
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) p[it] = pour[r[it]];              // (root[u] is a cell of the graph: its code is not NaN)
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (u >= cells) break;
        const bool hit = c[it] == c[it] && target_value<T>(p[it], values, kind, n_values);
        st_stream(out + u, hit ? (float)p[it] : nan_f32());
    }
}

// ------------------------------------------------------------------ flow_length
constexpr int LEN_ITEMS = 4;                    // three counts a cell: fewer cells a thread keep the registers down
struct Counts { unsigned *x, *y, *d; };

__global__ void __launch_bounds__(SPAN) length_decode_kernel(const float *__restrict__ dir, long rows, long cols, unsigned *__restrict__ head,
                                                             unsigned *__restrict__ anc, Counts cnt) {
    const long cells = rows * cols;
    const long first = (long)blockIdx.x * (SPAN * LEN_ITEMS) + threadIdx.x;
    float c[LEN_ITEMS], cv[LEN_ITEMS];
    long v[LEN_ITEMS];
    int k[LEN_ITEMS];
    bool bad = false;
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) {
        const long u = first + it * SPAN;
        c[it] = u < cells ? dir[u] : nan_f32();
    }
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) {
        k[it] = step_of(c[it], bad);
        v[it] = k[it] >= 0 ? neighbour(first + it * SPAN, k[it], rows, cols) : -1;
    }
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) cv[it] = v[it] >= 0 ? dir[v[it]] : nan_f32();
    unsigned live = 0;
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) {
        const long u = first + it * SPAN;
        const bool steps = cv[it] == cv[it];                             // the outlet's own code is not a step
        if (u < cells) {
            anc[u] = steps ? (unsigned)v[it] : NIL;
            const bool diagonal = k[it] & 1, along_x = (k[it] & 3) == 0;
            cnt.x[u] = steps && !diagonal && along_x;
            cnt.y[u] = steps && !diagonal && !along_x;
            cnt.d[u] = steps && diagonal;
        }
        live += wave_count(steps);
    }
    add_count(live, head);
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(head + BAD_WORD, 1u);
}

__global__ void __launch_bounds__(SPAN) length_round_kernel(long cells, const unsigned *__restrict__ anc, unsigned *__restrict__ anc_next, Counts cnt,
                                                            Counts cnt_next, unsigned *__restrict__ live_next) {
    const long first = (long)blockIdx.x * (SPAN * LEN_ITEMS) + threadIdx.x;
    unsigned a[LEN_ITEMS], x[LEN_ITEMS], y[LEN_ITEMS], d[LEN_ITEMS], next[LEN_ITEMS];
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) {
        const long u = first + it * SPAN;
        a[it] = NIL; x[it] = y[it] = d[it] = 0u;
        if (u < cells) { a[it] = anc[u]; x[it] = cnt.x[u]; y[it] = cnt.y[u]; d[it] = cnt.d[u]; }
    }
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) {
        next[it] = NIL;
        if (a[it] != NIL) { next[it] = anc[a[it]]; x[it] += cnt.x[a[it]]; y[it] += cnt.y[a[it]]; d[it] += cnt.d[a[it]]; }
    }
    unsigned live = 0;
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (u < cells) { anc_next[u] = next[it]; cnt_next.x[u] = x[it]; cnt_next.y[u] = y[it]; cnt_next.d[u] = d[it]; }
        live += wave_count(next[it] != NIL);
    }
    add_count(live, live_next);
}

__global__ void __launch_bounds__(SPAN) length_finish_kernel(const float *__restrict__ dir, long cells, Counts cnt, double cx, double cy, double dg,
                                                             double *__restrict__ out) {
    const long first = (long)blockIdx.x * (SPAN * LEN_ITEMS) + threadIdx.x;
#pragma unroll
    for (int it = 0; it < LEN_ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (u >= cells) break;
        const float c = dir[u];
        const double lx = (double)cnt.x[u] * cx, ly = (double)cnt.y[u] * cy, ld = (double)cnt.d[u] * dg;     // (uint32 -> float64: exact)
        const double sum = (lx + ly) + ld;
        st_stream(out + u, c == c ? sum : nan_f64());
    }
}

// ------------------------------------------------------------------ host side
inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
int bit_length(uint64_t v) {
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}
inline unsigned blocks(long count, int items = ITEMS) { return (unsigned)((count + SPAN * items - 1) / (SPAN * items)); }

// The host's side of a doubling: row 0 of `head` holds the live pointers of the start planes (written by the pass before);
// launch(k) runs round k, which reads the planes k & 1, writes the planes (k + 1) & 1 and counts into row k + 1.  Rounds are
// launched GROUP at a time until a count is 0 or `bound` rounds ran: at most `bound` launches, whatever the data.
struct Rounds {
    int rounds = 0, launched = 0;               // rounds that had live pointers; launches made (the planes in use: launched & 1)
    bool cycle = false;                         // a pointer was still live after `bound` rounds
    uint64_t live[MAX_ROUNDS + 1] = {};
};
template <typename L>
int run_rounds(unsigned *head, int bound, hipStream_t s, int64_t *ns, Rounds &r, L launch) {
    std::vector<unsigned> slots((size_t)(GROUP + 1) * ROW_WORDS);
    int launched = 0, checked = 0, rounds = -1;
    while (true) {
        const int n = launched - checked + 1;
        XRS_HIP(hipMemcpyAsync(slots.data(), head + (size_t)checked * ROW_WORDS, (size_t)n * ROW_WORDS * 4, hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        for (int k = checked; k <= launched; ++k) {
            r.live[k] = 0;
            for (int slot = 0; slot < SLOTS; ++slot) r.live[k] += slots[(size_t)(k - checked) * ROW_WORDS + slot * SLOT_STRIDE];
        }
        for (int k = checked; k <= launched && rounds < 0; ++k)
            if (r.live[k] == 0) rounds = k;
        checked = launched + 1;
        if (rounds >= 0 || launched >= bound) break;
        const int upto = launched + GROUP < bound ? launched + GROUP : bound;
        for (; launched < upto; ++launched) {
            const int64_t t0 = ns ? now_ns() : 0;
            if (int rc = launch(launched)) return rc;
            if (ns) { XRS_HIP(hipStreamSynchronize(s)); ns[launched] = now_ns() - t0; }
        }
    }
    r.cycle = rounds < 0;
    r.rounds = rounds < 0 ? launched : rounds;
    r.launched = launched;
    return 0;
}
int read_word(const unsigned *dev, unsigned &value, hipStream_t s) {
    XRS_HIP(hipMemcpyAsync(&value, dev, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    return 0;
}
bool too_many_cells(int64_t rows, int64_t cols) { return (uint64_t)rows > XRS_FLOW_MAX_CELLS / (uint64_t)cols; }

// ---- stream network
struct Net {
    unsigned *head, *slot;                      // slot: cells + 1 words
    unsigned *cell, *par, *up, *anc[2], *S, *D[2], *order, *shreve, *ids;       // per stream cell; sized for every cell
    unsigned char *cmask;
    char *cub;
    size_t cub_bytes, total;
};
Net carve_net(void *base, size_t cells) {
    Carver c(base);
    Net b = {};
    b.head = c.take<unsigned>(HEAD_WORDS);
    b.slot = c.take<unsigned>(cells + 1);
    b.cell = c.take<unsigned>(cells);
    b.par = c.take<unsigned>(cells);
    b.up = c.take<unsigned>(cells);
    for (int i = 0; i < 2; ++i) b.anc[i] = c.take<unsigned>(cells);
    b.S = c.take<unsigned>(cells);
    for (int i = 0; i < 2; ++i) b.D[i] = c.take<unsigned>(cells);       // the increments; the heads' root planes afterwards
    b.order = c.take<unsigned>(cells);
    b.shreve = c.take<unsigned>(cells);
    b.ids = c.take<unsigned>(cells + 1);
    b.cmask = c.take<unsigned char>(cells);
    size_t t = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (unsigned *)nullptr, (unsigned *)nullptr, (size_t)(cells + 1));
    b.cub_bytes = t > 0 ? t : 1;
    b.cub = c.take<char>(b.cub_bytes);
    b.total = c.at();
    return b;
}

// one weighted accumulation over the forest (level 0: Shreve's weight; k: 1[J_k]); `weight` = the cells that carry one.  With
// no weight anywhere (a level's end) no round runs.
int forest_accumulate(const Net &b, long n, unsigned level, long cols, hipStream_t s, Rounds &r, unsigned &weight) {
    const unsigned grid = blocks(n);
    XRS_HIP(hipMemsetAsync(b.head, 0, (size_t)HEAD_WORDS * 4, s));
    hipLaunchKernelGGL(forest_init_kernel, dim3(grid), dim3(SPAN), 0, s, n, level, cols, b.slot, b.cell, b.par, b.cmask, b.order, b.anc[0], b.S,
                       b.D[0], b.D[1], b.head);
    XRS_LAUNCH_CHECK();
    if (int rc = read_word(b.head + SUM_WORD, weight, s)) return rc;
    r = Rounds();
    if (level != 0 && weight == 0) return 0;
    if (int rc = run_rounds(b.head, bit_length((uint64_t)n), s, nullptr, r, [&](int k) {
            const int cur = k & 1, nxt = cur ^ 1;
            hipLaunchKernelGGL((jump_round_kernel<true, false>), dim3(grid), dim3(SPAN), 0, s, n, b.anc[cur], b.anc[nxt], b.S, b.D[nxt], b.D[cur],
                               (const unsigned *)nullptr, (unsigned *)nullptr, b.head + (k + 1) * ROW_WORDS);
            XRS_LAUNCH_CHECK();
            return 0;
        }))
        return rc;
    if (r.cycle) return 0;
    // the last additions lie in D[(launched - 1) & 1]; both planes are 0 when no round ran
    hipLaunchKernelGGL(forest_keep_kernel, dim3(grid), dim3(SPAN), 0, s, n, level, b.S, b.D[(r.launched + 1) & 1], b.shreve, b.order);
    XRS_LAUNCH_CHECK();
    return 0;
}

// ---- watershed, flow_length
struct Shed {
    unsigned *head, *anc[2], *root[2];
    size_t total;
};
Shed carve_shed(void *base, size_t cells) {
    Carver c(base);
    Shed b = {};
    b.head = c.take<unsigned>(HEAD_WORDS);
    for (int i = 0; i < 2; ++i) b.anc[i] = c.take<unsigned>(cells);
    for (int i = 0; i < 2; ++i) b.root[i] = c.take<unsigned>(cells);
    b.total = c.at();
    return b;
}
struct Length {
    unsigned *head, *anc[2];
    Counts cnt[2];
    size_t total;
};
Length carve_length(void *base, size_t cells) {
    Carver c(base);
    Length b = {};
    b.head = c.take<unsigned>(HEAD_WORDS);
    for (int i = 0; i < 2; ++i) b.anc[i] = c.take<unsigned>(cells);
    for (int i = 0; i < 2; ++i) {
        b.cnt[i].x = c.take<unsigned>(cells);
        b.cnt[i].y = c.take<unsigned>(cells);
        b.cnt[i].d = c.take<unsigned>(cells);
    }
    b.total = c.at();
    return b;
}

// the status words that xrs_flow_watershed and xrs_flow_length share with xrs_flow_accumulate
int graph_status(const unsigned *head, const Rounds &r, int64_t *status_host, hipStream_t s) {
    unsigned bad = 0;
    if (int rc = read_word(head + BAD_WORD, bad, s)) return rc;
    status_host[0] = r.rounds;
    status_host[1] = (bad ? XRS_FLOW_INVALID_CODE : 0) | (r.cycle ? XRS_FLOW_CYCLE : 0);
    for (int k = 0; k <= r.launched; ++k) status_host[4 + k] = (int64_t)r.live[k];
    return 0;
}

template <typename T>
int watershed_typed(const float *dir, const T *pour, const void *values, int kind, int n_values, long rows, long cols, const Shed &b, float *out,
                    int64_t *status_host, bool timed, hipStream_t s) {
    const long cells = rows * cols;
    const unsigned grid = blocks(cells);
    int64_t t0 = 0;
    XRS_HIP(hipMemsetAsync(b.head, 0, (size_t)HEAD_WORDS * 4, s));
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); t0 = now_ns(); }
    hipLaunchKernelGGL((shed_decode_kernel<T>), dim3(grid), dim3(SPAN), 0, s, dir, pour, values, kind, n_values, rows, cols, b.head, b.anc[0],
                       b.root[0]);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status_host[2] = now_ns() - t0; }
    Rounds r;
    if (int rc = run_rounds(b.head, bit_length((uint64_t)cells), s, timed ? status_host + 40 : nullptr, r, [&](int k) {
            const int cur = k & 1, nxt = cur ^ 1;
            hipLaunchKernelGGL((jump_round_kernel<false, true>), dim3(grid), dim3(SPAN), 0, s, cells, b.anc[cur], b.anc[nxt], (unsigned *)nullptr,
                               (unsigned *)nullptr, (unsigned *)nullptr, b.root[cur], b.root[nxt], b.head + (k + 1) * ROW_WORDS);
            XRS_LAUNCH_CHECK();
            return 0;
        }))
        return rc;
    if (int rc = graph_status(b.head, r, status_host, s)) return rc;
    unsigned pours = 0;
    if (int rc = read_word(b.head + SUM_WORD, pours, s)) return rc;
    status_host[37] = pours;
    if (status_host[1]) return 0;                                        // the caller raises; no product is written
    if (timed) t0 = now_ns();
    hipLaunchKernelGGL((shed_gather_kernel<T>), dim3(grid), dim3(SPAN), 0, s, dir, pour, values, kind, n_values, cells, b.root[r.launched & 1], out);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status_host[3] = now_ns() - t0; }
    return 0;
}

}  // namespace

extern "C" {

int xrs_stream_network_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_stream_network_workspace_size: null pointer");
    *bytes_out = 0;
    if (rows <= 0 || cols <= 0 || too_many_cells(rows, cols)) return 0;
    *bytes_out = carve_net(nullptr, (size_t)rows * (size_t)cols).total;
    return 0;
}

int xrs_stream_network(const float *dir_dev, const void *accum_dev, int accum_dtype, int64_t rows, int64_t cols, double threshold, int want,
                       void *work_dev, double *strahler_out_dev, double *shreve_out_dev, double *link_out_dev, int64_t *status_host, int flags,
                       void *stream) {
    const char *what = "xrs_stream_network";
    const int all = XRS_STREAM_STRAHLER | XRS_STREAM_SHREVE | XRS_STREAM_LINK;
    if (rows < 0 || cols < 0) return fail("%s: negative shape", what);
    if (flags & ~XRS_STREAM_TIMED) return fail("%s: unknown flags %d", what, flags);
    if ((want & ~all) || !(want & all)) return fail("%s: `want` must name at least one of Strahler, Shreve and link, got %d", what, want);
    if (!dtype_in(DT_FLOATS, accum_dtype)) return fail("%s: unsupported accumulation dtype code %d (float32 or float64)", what, accum_dtype);
    if (threshold != threshold) return fail("%s: the threshold is NaN", what);
    if (!status_host) return fail("%s: null status pointer", what);
    for (int w = 0; w < XRS_STREAM_STATUS_WORDS; ++w) status_host[w] = 0;
    if (rows == 0 || cols == 0) return 0;
    if (too_many_cells(rows, cols)) return fail("%s: more than 2^32 - 2 cells (%lld x %lld)", what, (long long)rows, (long long)cols);
    double *outs[3] = {want & XRS_STREAM_STRAHLER ? strahler_out_dev : nullptr, want & XRS_STREAM_SHREVE ? shreve_out_dev : nullptr,
                       want & XRS_STREAM_LINK ? link_out_dev : nullptr};
    if (!dir_dev || !accum_dev || !work_dev) return fail("%s: null pointer", what);
    for (int i = 0; i < 3; ++i) {
        if ((want >> i & 1) && !outs[i]) return fail("%s: null pointer for a result that `want` names", what);
        if (!outs[i]) continue;
        if ((const void *)outs[i] == (const void *)dir_dev || (const void *)outs[i] == accum_dev)
            return fail("%s: a result plane cannot overwrite an input", what);
        for (int j = 0; j < i; ++j)
            if (outs[i] == outs[j]) return fail("%s: two results cannot share a plane", what);
    }

    hipStream_t s = as_stream(stream);
    const bool timed = flags & XRS_STREAM_TIMED;
    const long cells = (long)rows * (long)cols;
    const Net b = carve_net(work_dev, (size_t)cells);
    const unsigned grid = blocks(cells);
    int64_t t0 = 0;
    auto lap = [&](int word) -> int {                                    // with TIMED: the nanoseconds since the lap before
        if (!timed) return 0;
        XRS_HIP(hipStreamSynchronize(s));
        const int64_t t = now_ns();
        if (word >= 0) status_host[word] = t - t0;
        t0 = t;
        return 0;
    };

    XRS_HIP(hipMemsetAsync(b.head, 0, (size_t)HEAD_WORDS * 4, s));
    XRS_HIP(hipMemsetAsync(b.slot + cells, 0, 4, s));
    if (int rc = lap(-1)) return rc;
    with_dtype<DT_FLOATS>(accum_dtype, [&](auto t) {
        using TA = dtype_of<decltype(t)>;
        hipLaunchKernelGGL((stream_mark_kernel<TA>), dim3(grid), dim3(SPAN), 0, s, dir_dev, static_cast<const TA *>(accum_dev), cells, threshold,
                           b.slot, b.head);
    });
    XRS_LAUNCH_CHECK();
    size_t cub_bytes = b.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(b.cub, cub_bytes, b.slot, b.slot, (size_t)(cells + 1), s));
    unsigned bad = 0, n_streams = 0;
    if (int rc = read_word(b.head + BAD_WORD, bad, s)) return rc;
    if (int rc = read_word(b.slot + cells, n_streams, s)) return rc;
    status_host[3] = n_streams;
    if (bad) { status_host[1] = XRS_FLOW_INVALID_CODE; return 0; }     // the caller raises; no product is written
    const long n = n_streams;

    Rounds r;
    const unsigned *roots = nullptr;
    if (n > 0) {
        hipLaunchKernelGGL(stream_compact_kernel, dim3(grid), dim3(SPAN), 0, s, dir_dev, (long)rows, (long)cols, b.slot, b.cell, b.par, b.up,
                           b.cmask);
        XRS_LAUNCH_CHECK();
        if (int rc = lap(8)) return rc;

        // Shreve's sums, always: this run finds the rings of stream cells and counts the sources
        unsigned sources = 0;
        if (int rc = forest_accumulate(b, n, 0u, (long)cols, s, r, sources)) return rc;
        status_host[0] = r.rounds;
        status_host[4] = sources;
        for (int k = 0; k <= r.launched; ++k) status_host[16 + k] = (int64_t)r.live[k];
        if (r.cycle) { status_host[1] = XRS_FLOW_CYCLE; return 0; }
        if (int rc = lap(9)) return rc;

        if (want & XRS_STREAM_STRAHLER) {
            // level k = 1, 2, ..: at most bit_length(sources) of them have a J_k that is not empty; one more look sees the 0
            const int bound = bit_length((uint64_t)sources) < MAX_LEVELS ? bit_length((uint64_t)sources) : MAX_LEVELS;
            int levels = 1;
            for (int k = 1; k <= bound; ++k) {
                unsigned joints = 0;
                Rounds lr;
                if (int rc = forest_accumulate(b, n, (unsigned)k, (long)cols, s, lr, joints)) return rc;
                status_host[56 + k] = joints;
                status_host[96 + k] = lr.rounds;
                if (joints == 0) break;
                levels = k + 1;
            }
            status_host[2] = levels;
            if (int rc = lap(10)) return rc;
        }

        if (want & XRS_STREAM_LINK) {
            const unsigned sgrid = blocks(n);
            XRS_HIP(hipMemsetAsync(b.head, 0, (size_t)HEAD_WORDS * 4, s));
            XRS_HIP(hipMemsetAsync(b.ids + n, 0, 4, s));
            hipLaunchKernelGGL(head_init_kernel, dim3(sgrid), dim3(SPAN), 0, s, n, b.up, b.cmask, b.anc[0], b.D[0], b.ids, b.head);
            XRS_LAUNCH_CHECK();
            cub_bytes = b.cub_bytes;
            XRS_HIP(hipcub::DeviceScan::ExclusiveSum(b.cub, cub_bytes, b.ids, b.ids, (size_t)(n + 1), s));
            Rounds hr;
            if (int rc = run_rounds(b.head, bit_length((uint64_t)n), s, nullptr, hr, [&](int k) {
                    const int cur = k & 1, nxt = cur ^ 1;
                    hipLaunchKernelGGL((jump_round_kernel<false, true>), dim3(sgrid), dim3(SPAN), 0, s, n, b.anc[cur], b.anc[nxt], (unsigned *)nullptr,
                                       (unsigned *)nullptr, (unsigned *)nullptr, b.D[cur], b.D[nxt], b.head + (k + 1) * ROW_WORDS);
                    XRS_LAUNCH_CHECK();
                    return 0;
                }))
                return rc;
            unsigned heads = 0;
            if (int rc = read_word(b.head + SUM_WORD, heads, s)) return rc;
            status_host[5] = heads;
            status_host[6] = hr.rounds;
            if (hr.cycle) { status_host[1] = XRS_FLOW_CYCLE; return 0; }
            roots = b.D[hr.launched & 1];
            if (int rc = lap(11)) return rc;
        }
    }
    // (without a stream cell no slot is read: every cell gets NaN)
    hipLaunchKernelGGL(stream_finish_kernel, dim3(grid), dim3(SPAN), 0, s, cells, b.slot, b.order, b.shreve, roots, b.ids, outs[0], outs[1], outs[2]);
    XRS_LAUNCH_CHECK();
    return lap(12);
}

int xrs_flow_watershed_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_flow_watershed_workspace_size: null pointer");
    *bytes_out = 0;
    if (rows <= 0 || cols <= 0 || too_many_cells(rows, cols)) return 0;
    *bytes_out = carve_shed(nullptr, (size_t)rows * (size_t)cols).total;
    return 0;
}

int xrs_flow_watershed(const float *dir_dev, const void *pour_dev, int dtype, const void *values_dev, int values_kind, int n_values,
                       int64_t rows, int64_t cols, void *work_dev, float *out_dev, int64_t *status_host, int flags, void *stream) {
    const char *what = "xrs_flow_watershed";
    if (rows < 0 || cols < 0) return fail("%s: negative shape", what);
    if (flags & ~XRS_FLOW_TIMED) return fail("%s: unknown flags %d", what, flags);
    if (!dtype_bytes(dtype)) return fail("%s: unsupported dtype code %d", what, dtype);
    if (n_values < 0) return fail("%s: negative n_values %d", what, n_values);
    if (values_kind != XRS_PROX_VALUES_F64 && values_kind != XRS_PROX_VALUES_I64 && values_kind != XRS_PROX_VALUES_U64)
        return fail("%s: unknown values_kind %d", what, values_kind);
    if (!status_host) return fail("%s: null status pointer", what);
    for (int w = 0; w < XRS_FLOW_STATUS_WORDS; ++w) status_host[w] = 0;
    if (rows == 0 || cols == 0) return 0;
    if (too_many_cells(rows, cols)) return fail("%s: more than 2^32 - 2 cells (%lld x %lld)", what, (long long)rows, (long long)cols);
    if (!dir_dev || !pour_dev || !work_dev || !out_dev || (n_values > 0 && !values_dev)) return fail("%s: null pointer", what);
    if ((const void *)out_dev == (const void *)dir_dev || (const void *)out_dev == pour_dev)
        return fail("%s: the result plane cannot overwrite an input", what);
    const Shed b = carve_shed(work_dev, (size_t)rows * (size_t)cols);
    int rc = 0;
    with_dtype(dtype, [&](auto t) {                                      // (every other code was refused above)
        using T = dtype_of<decltype(t)>;
        rc = watershed_typed(dir_dev, static_cast<const T *>(pour_dev), values_dev, values_kind, n_values, (long)rows, (long)cols, b, out_dev,
                             status_host, (flags & XRS_FLOW_TIMED) != 0, as_stream(stream));
    });
    return rc;
}

int xrs_flow_length_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out) {
    if (!bytes_out) return fail("xrs_flow_length_workspace_size: null pointer");
    *bytes_out = 0;
    if (rows <= 0 || cols <= 0 || too_many_cells(rows, cols)) return 0;
    *bytes_out = carve_length(nullptr, (size_t)rows * (size_t)cols).total;
    return 0;
}

int xrs_flow_length(const float *dir_dev, int64_t rows, int64_t cols, double cellsize_x, double cellsize_y, double diag, void *work_dev,
                    double *out_dev, int64_t *status_host, int flags, void *stream) {
    const char *what = "xrs_flow_length";
    if (rows < 0 || cols < 0) return fail("%s: negative shape", what);
    if (flags & ~XRS_FLOW_TIMED) return fail("%s: unknown flags %d", what, flags);
    if (!(cellsize_x > 0.0) || !(cellsize_y > 0.0) || !(diag > 0.0) || std::isinf(cellsize_x) || std::isinf(cellsize_y) || std::isinf(diag))
        return fail("%s: cell sizes must be positive and finite (%g, %g, diagonal %g)", what, cellsize_x, cellsize_y, diag);
    if (!status_host) return fail("%s: null status pointer", what);
    for (int w = 0; w < XRS_FLOW_STATUS_WORDS; ++w) status_host[w] = 0;
    if (rows == 0 || cols == 0) return 0;
    if (too_many_cells(rows, cols)) return fail("%s: more than 2^32 - 2 cells (%lld x %lld)", what, (long long)rows, (long long)cols);
    if (!dir_dev || !work_dev || !out_dev) return fail("%s: null pointer", what);
    if ((const void *)out_dev == (const void *)dir_dev) return fail("%s: the result plane cannot overwrite the input", what);

    hipStream_t s = as_stream(stream);
    const bool timed = flags & XRS_FLOW_TIMED;
    const long cells = (long)rows * (long)cols;
    const Length b = carve_length(work_dev, (size_t)cells);
    const unsigned grid = blocks(cells, LEN_ITEMS);
    int64_t t0 = 0;
    XRS_HIP(hipMemsetAsync(b.head, 0, (size_t)HEAD_WORDS * 4, s));
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); t0 = now_ns(); }
    hipLaunchKernelGGL(length_decode_kernel, dim3(grid), dim3(SPAN), 0, s, dir_dev, (long)rows, (long)cols, b.head, b.anc[0], b.cnt[0]);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status_host[2] = now_ns() - t0; }
    Rounds r;
    if (int rc = run_rounds(b.head, bit_length((uint64_t)cells), s, timed ? status_host + 40 : nullptr, r, [&](int k) {
            const int cur = k & 1, nxt = cur ^ 1;
            hipLaunchKernelGGL(length_round_kernel, dim3(grid), dim3(SPAN), 0, s, cells, b.anc[cur], b.anc[nxt], b.cnt[cur], b.cnt[nxt],
                               b.head + (k + 1) * ROW_WORDS);
            XRS_LAUNCH_CHECK();
            return 0;
        }))
        return rc;
    if (int rc = graph_status(b.head, r, status_host, s)) return rc;
    if (status_host[1]) return 0;                                        // the caller raises; no product is written
    if (timed) t0 = now_ns();
    hipLaunchKernelGGL(length_finish_kernel, dim3(grid), dim3(SPAN), 0, s, dir_dev, cells, b.cnt[r.launched & 1], cellsize_x, cellsize_y, diag,
                       out_dev);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status_host[3] = now_ns() - t0; }
    return 0;
}

}  // extern "C"

// flow_direction / flow_accumulation / basins: D8 hydrology.
//
// The reference has no hydrology code; the result is a written rule (xrspatial_amd/hydrology.py, tests/hydrology_oracle.py).
//   direction   a block on SPAN adjacent columns of BAND rows, a thread on one column of them.  The block stages its BAND + 2
//               rows (SPAN + 2 columns, NaN beyond the raster) in LDS, then every thread walks each cell's neighbours in the
//               fixed order E, SE, S, SW, W, NW, N, NE: drop = (z - zk) / dist, one IEEE subtraction and one IEEE division
//               in float64, taken only if drop > best (strict, false on NaN).  Contraction is off for the whole file.
//   decode      float32 code -> uint32 downstream index or NIL (code 0, a neighbour outside the raster or a NaN neighbour);
//               a non-NaN value that is no code sets the status word.
//   rounds      pointer doubling.  anc_k[u] = u's 2^k-th ancestor or NIL; S_k[v] = cells of v's upstream tree nearer than 2^k
//               (v included).  Round k: every cell with a live anc_k[u] adds S_k[u] to its ancestor's next count, then
//               anc_{k+1}[u] = anc_k[anc_k[u]] and root_{k+1}[u] = root_k[root_k[u]].  anc and root ping-pong between two
//               planes.  S does not need to: only thread u reads S[u], so S stays in place and the additions land in a plane
//               of increments D that its owner folds into S (and clears) in the next round; D ping-pongs.  uint32 integer
//               adds: the result does not depend on arrival order.  A round counts the live pointers it writes, one add per
//               wave of the ballot counts of its cells; the host reads the counts every two rounds and stops at the first 0,
//               or after (rows * cols).bit_length() rounds, when a pointer that is still live lies on or above a cycle.  No
//               loop depends on the data.
//   finish      uint32 -> float64, NaN at NaN cells.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "workspace.h"

#include <chrono>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr int SPAN = 256;                       // columns per direction block, cells per block elsewhere: four waves
constexpr unsigned NIL = 0xffffffffu;           // no downstream cell / no 2^k-th ancestor
constexpr int MAX_ROUNDS = XRS_FLOW_MAX_ROUNDS; // (2^32 - 2).bit_length()
constexpr int ITEMS = 8;                        // cells per thread of decode, round and finish, SPAN apart
constexpr int GROUP = 2;                        // rounds between two looks at the live counts
// One word for a round's count serialises its adds: with one add per wave of 64 cells a round of 8192^2 cells took 6.7 ms,
// atomics or not, and 1.0 ms with 32 adjacent words and 256 cells a wave (profiles/hydrology/README.md).  So a wave counts
// ITEMS * 64 cells before it adds, and the waves spread their adds over SLOTS words a round that lie 256 bytes apart; the host
// sums them.
constexpr int SLOTS = 64, SLOT_STRIDE = 64;
constexpr int ROW_WORDS = SLOTS * SLOT_STRIDE;                           // live[k]: one row of slots, k = 0 .. MAX_ROUNDS
constexpr int BAD_WORD = (MAX_ROUNDS + 1) * ROW_WORDS;                   // then the invalid-code word
constexpr int HEAD_WORDS = BAD_WORD + 64;
static_assert(HEAD_WORDS % 64 == 0 && 40 + MAX_ROUNDS <= XRS_FLOW_STATUS_WORDS, "head / status layout");

// ------------------------------------------------------------------ direction
// One cell, one load and one store per thread left the kernel waiting on its own loads (0.43 ms for 8192^2 float32 cells
// against 0.09 ms of the copy yardstick; dividing less did not change that): a block takes BAND rows, so a thread has
// BAND + 2 independent loads in flight before it waits.
constexpr int BAND = 8;

template <typename T>
__global__ void __launch_bounds__(SPAN) flow_direction_kernel(const T *__restrict__ data, long rows, long cols, unsigned spans, double cx,
                                                              double cy, double dg, float *__restrict__ out) {
    __shared__ T tile[BAND + 2][SPAN + 2];      // tile[r][1 + t]: row i0 - 1 + r, column j0 + t; NaN beyond the raster
    const unsigned band = blockIdx.x / spans;   // (the grid has fewer than 2^31 blocks: 32-bit division)
    const long i0 = (long)band * BAND;
    const long j0 = (long)(blockIdx.x - band * spans) * SPAN;
    const int t = threadIdx.x;
    const T nan = (T)__int_as_float(0x7fc00000);
    const long j = j0 + t;
    const long jh = t == 0 ? j0 - 1 : j0 + SPAN;                         // threads 0 and 1 also load the two halo columns
    const bool col_ok = j < cols, halo_ok = t < 2 && jh >= 0 && jh < cols;
    T mine[BAND + 2], halo[BAND + 2];
#pragma unroll
    for (int r = 0; r < BAND + 2; ++r) {
        const long row = i0 - 1 + r;
        const bool row_ok = row >= 0 && row < rows;
        const T *__restrict__ in = data + (row_ok ? row : i0) * cols;
        mine[r] = (row_ok && col_ok) ? in[j] : nan;
        halo[r] = (row_ok && halo_ok) ? in[jh] : nan;
    }
#pragma unroll
    for (int r = 0; r < BAND + 2; ++r) {
        tile[r][1 + t] = mine[r];
        if (t < 2) tile[r][t == 0 ? 0 : SPAN + 1] = halo[r];
    }
    __syncthreads();
    if (!col_ok) return;
#pragma unroll
    for (int r = 1; r <= BAND; ++r) {
        const long i = i0 - 1 + r;
        if (i >= rows) break;
        const double z = (double)tile[r][1 + t];
        float code = nan_f32();
        if (z == z) {
            double best = 0.0;
            int c = 0;
            // a difference that is not positive (NaN included) gives a drop that is not above `best`: the division is skipped
            auto take = [&](T zk, double dist, int k) {
                const double diff = z - (double)zk;
                if (diff > 0.0) {
                    const double drop = diff / dist;
                    if (drop > best) { best = drop; c = k; }
                }
            };
            take(tile[r][2 + t], cx, 1);            // E
            take(tile[r + 1][2 + t], dg, 2);        // SE
            take(tile[r + 1][1 + t], cy, 4);        // S
            take(tile[r + 1][0 + t], dg, 8);        // SW
            take(tile[r][0 + t], cx, 16);           // W
            take(tile[r - 1][0 + t], dg, 32);       // NW
            take(tile[r - 1][1 + t], cy, 64);       // N
            take(tile[r - 1][2 + t], dg, 128);      // NE
            code = (float)c;
        }
        st_stream(out + i * cols + j, code);
    }
}

// ------------------------------------------------------------------ decode
// a wave's count of live pointers: summed over its ITEMS steps, added once, to the wave's slot
__device__ __forceinline__ unsigned wave_count(bool live) { return (unsigned)__popcll(__ballot(live)); }
__device__ __forceinline__ void add_count(unsigned n, unsigned *__restrict__ slots) {
    if (n != 0 && (threadIdx.x & 63) == 0) atomicAdd(slots + ((blockIdx.x * (SPAN / 64) + (threadIdx.x >> 6)) & (SLOTS - 1)) * SLOT_STRIDE, n);
}

// (decode and round: a thread's ITEMS cells go through each step together -- own loads, dependent loads, stores -- so that
//  ITEMS loads are in flight at a time; cell by cell the stores and atomics between them kept the loads apart)
template <bool ACC, bool BASIN>
__global__ void __launch_bounds__(SPAN) flow_decode_kernel(const float *__restrict__ dir, long rows, long cols, unsigned *__restrict__ head,
                                                           unsigned *__restrict__ anc, unsigned *__restrict__ S, unsigned *__restrict__ D0,
                                                           unsigned *__restrict__ D1, unsigned *__restrict__ root) {
    const long cells = rows * cols;
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    float c[ITEMS], cv[ITEMS];
    long v[ITEMS];
    bool bad = false;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        c[it] = u < cells ? dir[u] : nan_f32();
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {                                 // the cell the code names, or -1
        const long u = first + it * SPAN;
        const float code = c[it];
        int dr = 0, dc = 0;
        if (code == 1.0f) { dc = 1; }
        else if (code == 2.0f) { dr = 1; dc = 1; }
        else if (code == 4.0f) { dr = 1; }
        else if (code == 8.0f) { dr = 1; dc = -1; }
        else if (code == 16.0f) { dc = -1; }
        else if (code == 32.0f) { dr = -1; dc = -1; }
        else if (code == 64.0f) { dr = -1; }
        else if (code == 128.0f) { dr = -1; dc = 1; }
        else bad |= code == code && code != 0.0f;
        v[it] = -1;
        if (dr | dc) {
            const unsigned ui = (unsigned)u / (unsigned)cols;            // (cells and cols fit 32 bits: no 64-bit division)
            const long i = ui, j = u - (long)ui * cols;
            const long r = i + dr, q = j + dc;
            if (r >= 0 && r < rows && q >= 0 && q < cols) v[it] = r * cols + q;
        }
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) cv[it] = v[it] >= 0 ? dir[v[it]] : nan_f32();
    unsigned live = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        const unsigned down = cv[it] == cv[it] ? (unsigned)v[it] : NIL;  // a NaN neighbour is no downstream cell
        if (u < cells) {
            anc[u] = down;
            if (ACC) { S[u] = c[it] == c[it] ? 1u : 0u; D0[u] = 0u; D1[u] = 0u; }
            if (BASIN) root[u] = down != NIL ? down : (unsigned)u;
        }
        live += wave_count(down != NIL);
    }
    add_count(live, head);
    if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(head + BAD_WORD, 1u);
}

// ------------------------------------------------------------------ one doubling round
template <bool ACC, bool BASIN>
__global__ void __launch_bounds__(SPAN) flow_round_kernel(long cells, const unsigned *__restrict__ anc, unsigned *__restrict__ anc_next,
                                                          unsigned *__restrict__ S, unsigned *__restrict__ D_prev, unsigned *__restrict__ D_cur,
                                                          const unsigned *__restrict__ root, unsigned *__restrict__ root_next,
                                                          unsigned *__restrict__ live_next) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    unsigned a[ITEMS], s[ITEMS], add[ITEMS], r[ITEMS], next[ITEMS];
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        a[it] = NIL; s[it] = add[it] = r[it] = 0u;
        if (u < cells) {
            a[it] = anc[u];
            if (ACC) { add[it] = D_prev[u]; s[it] = S[u]; }              // what round k - 1 brought: S_k = S_{k-1} + D_{k-1}
            if (BASIN) r[it] = root[u];
        }
    }
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        next[it] = a[it] != NIL ? anc[a[it]] : NIL;
        if (BASIN && a[it] != NIL) r[it] = root[r[it]];                  // (a dead pointer: root[u] is the outlet already)
    }
    unsigned live = 0;
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (u < cells) {
            if (ACC) {
                if (add[it]) { s[it] += add[it]; S[u] = s[it]; D_prev[u] = 0u; }   // cleared by its owner: the plane is round k + 1's D_cur
                if (a[it] != NIL) atomicAdd(D_cur + a[it], s[it]);
            }
            anc_next[u] = next[it];
            if (BASIN) root_next[u] = r[it];
        }
        live += wave_count(next[it] != NIL);
    }
    add_count(live, live_next);
}

template <bool ACC, bool BASIN>
__global__ void __launch_bounds__(SPAN) flow_finish_kernel(const float *__restrict__ dir, long cells, const unsigned *__restrict__ S,
                                                           const unsigned *__restrict__ D, const unsigned *__restrict__ root,
                                                           double *__restrict__ acc_out, double *__restrict__ basin_out) {
    const long first = (long)blockIdx.x * (SPAN * ITEMS) + threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int it = 0; it < ITEMS; ++it) {
        const long u = first + it * SPAN;
        if (u >= cells) break;
        const float c = dir[u];
        const bool valid = c == c;
        if (ACC) st_stream(acc_out + u, valid ? (double)(S[u] + D[u]) : nan);
        if (BASIN) st_stream(basin_out + u, valid ? (double)root[u] : nan);
    }
}

struct Buffers {
    unsigned *head, *anc[2], *S, *D[2], *root[2];
    size_t total;
};
Buffers carve(void *base, size_t cells, int want) {
    Carver c(base);
    Buffers b = {};
    b.head = c.take<unsigned>(HEAD_WORDS);
    for (int i = 0; i < 2; ++i) b.anc[i] = c.take<unsigned>(cells);
    if (want & XRS_FLOW_ACCUMULATION) {
        b.S = c.take<unsigned>(cells);
        for (int i = 0; i < 2; ++i) b.D[i] = c.take<unsigned>(cells);
    }
    if (want & XRS_FLOW_BASINS)
        for (int i = 0; i < 2; ++i) b.root[i] = c.take<unsigned>(cells);
    b.total = c.at();
    return b;
}

template <bool ACC, bool BASIN>
void launch_decode(const float *dir, long rows, long cols, const Buffers &b, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL((flow_decode_kernel<ACC, BASIN>), dim3(grid), dim3(SPAN), 0, s, dir, rows, cols, b.head, b.anc[0], b.S, b.D[0],
                       b.D[1], b.root[0]);
}
template <bool ACC, bool BASIN>
void launch_round(long cells, int k, const Buffers &b, unsigned grid, hipStream_t s) {
    const int cur = k & 1, nxt = cur ^ 1;
    // round k folds D[nxt] (round k - 1's additions) into S and adds into D[cur]
    hipLaunchKernelGGL((flow_round_kernel<ACC, BASIN>), dim3(grid), dim3(SPAN), 0, s, cells, b.anc[cur], b.anc[nxt], b.S, b.D[nxt],
                       b.D[cur], b.root[cur], b.root[nxt], b.head + (k + 1) * ROW_WORDS);
}
template <bool ACC, bool BASIN>
void launch_finish(const float *dir, long cells, int rounds, const Buffers &b, double *acc, double *basin, unsigned grid, hipStream_t s) {
    // after `rounds` launches the last additions lie in D[(rounds - 1) & 1] (both planes are 0 when none ran) and the
    // pointers in plane rounds & 1
    hipLaunchKernelGGL((flow_finish_kernel<ACC, BASIN>), dim3(grid), dim3(SPAN), 0, s, dir, cells, b.S, b.D[(rounds + 1) & 1],
                       b.root[rounds & 1], acc, basin);
}

#define XRS_FLOW_DISPATCH(fn, ...)                                        \
    do {                                                                  \
        if (acc && basin) fn<true, true>(__VA_ARGS__);                    \
        else if (acc) fn<true, false>(__VA_ARGS__);                       \
        else fn<false, true>(__VA_ARGS__);                                \
    } while (0)

inline int64_t now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int bit_length(uint64_t v) {
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

}  // namespace

extern "C" {

int xrs_flow_direction(const void *data_dev, int dtype, int64_t rows, int64_t cols, double cellsize_x, double cellsize_y, double diag,
                       float *out_dev, void *stream) {
    if (rows < 0 || cols < 0) return fail("xrs_flow_direction: negative shape");
    if (!dtype_in(DT_FLOATS, dtype)) return fail("xrs_flow_direction: unsupported dtype code %d (float32 or float64)", dtype);
    if (!(cellsize_x > 0.0) || !(cellsize_y > 0.0) || !(diag > 0.0) || std::isinf(cellsize_x) || std::isinf(cellsize_y) || std::isinf(diag))
        return fail("xrs_flow_direction: cell sizes must be positive and finite (%g, %g, diagonal %g)", cellsize_x, cellsize_y, diag);
    if (rows == 0 || cols == 0) return 0;
    const long spans = (cols + SPAN - 1) / SPAN, bands = (rows + BAND - 1) / BAND;
    if (cols >= (1L << 31) - SPAN || rows >= (1L << 31) || bands * spans >= (1L << 31))
        return fail("xrs_flow_direction: raster too large for one call (%lld x %lld)", (long long)rows, (long long)cols);
    if (!data_dev || !out_dev) return fail("xrs_flow_direction: null pointer");
    hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)(bands * spans));
    with_dtype<DT_FLOATS>(dtype, [&](auto t) {                    // (the code was checked above)
        using T = dtype_of<decltype(t)>;
        hipLaunchKernelGGL((flow_direction_kernel<T>), grid, dim3(SPAN), 0, s, static_cast<const T *>(data_dev), (long)rows,
                           (long)cols, (unsigned)spans, cellsize_x, cellsize_y, diag, out_dev);
    });
    XRS_LAUNCH_CHECK();
    return 0;
}

size_t xrs_flow_workspace_bytes(int64_t rows, int64_t cols, int want) {
    if (rows <= 0 || cols <= 0 || !(want & (XRS_FLOW_ACCUMULATION | XRS_FLOW_BASINS))) return 0;
    if ((uint64_t)rows > XRS_FLOW_MAX_CELLS / (uint64_t)cols) return 0;
    return carve(nullptr, (size_t)rows * (size_t)cols, want).total;
}

int xrs_flow_accumulate(const float *dir_dev, int64_t rows, int64_t cols, void *work_dev, double *acc_out_dev, double *basin_out_dev,
                        int64_t *status_host, int flags, void *stream) {
    if (rows < 0 || cols < 0) return fail("xrs_flow_accumulate: negative shape");
    if (flags & ~XRS_FLOW_TIMED) return fail("xrs_flow_accumulate: unknown flags %d", flags);
    if (!status_host) return fail("xrs_flow_accumulate: null status pointer");
    for (int w = 0; w < XRS_FLOW_STATUS_WORDS; ++w) status_host[w] = 0;
    if (rows == 0 || cols == 0) return 0;
    if ((uint64_t)rows > XRS_FLOW_MAX_CELLS / (uint64_t)cols)
        return fail("xrs_flow_accumulate: more than 2^32 - 2 cells (%lld x %lld)", (long long)rows, (long long)cols);
    if (!acc_out_dev && !basin_out_dev) return fail("xrs_flow_accumulate: no product asked for");
    if (!dir_dev || !work_dev) return fail("xrs_flow_accumulate: null pointer");

    hipStream_t s = as_stream(stream);
    const bool acc = acc_out_dev != nullptr, basin = basin_out_dev != nullptr, timed = flags & XRS_FLOW_TIMED;
    const long cells = (long)rows * (long)cols;
    const Buffers b = carve(work_dev, (size_t)cells, (acc ? XRS_FLOW_ACCUMULATION : 0) | (basin ? XRS_FLOW_BASINS : 0));
    const unsigned grid = (unsigned)((cells + SPAN * ITEMS - 1) / (SPAN * ITEMS));      // < 2^21 blocks
    const int bound = bit_length((uint64_t)cells);                       // a path has at most cells - 1 < 2^bound steps
    std::vector<unsigned> slots((size_t)(GROUP + 1) * ROW_WORDS);
    uint64_t live[MAX_ROUNDS + 1];

    int64_t t0 = 0;
    XRS_HIP(hipMemsetAsync(b.head, 0, (size_t)HEAD_WORDS * 4, s));
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); t0 = now_ns(); }
    XRS_FLOW_DISPATCH(launch_decode, dir_dev, (long)rows, (long)cols, b, grid, s);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status_host[2] = now_ns() - t0; }

    // rounds 0 .. bound - 1 at the most; live[k] = pointers anc_k that are not NIL (live[0] from decode, live[k + 1] from round k)
    int launched = 0, checked = 0, rounds = -1;
    while (true) {
        const int n = launched - checked + 1;                            // the rows not looked at yet: 1, then GROUP
        XRS_HIP(hipMemcpyAsync(slots.data(), b.head + (size_t)checked * ROW_WORDS, (size_t)n * ROW_WORDS * 4, hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        for (int k = checked; k <= launched; ++k) {
            live[k] = 0;
            for (int slot = 0; slot < SLOTS; ++slot) live[k] += slots[(size_t)(k - checked) * ROW_WORDS + slot * SLOT_STRIDE];
        }
        for (int k = checked; k <= launched && rounds < 0; ++k)
            if (live[k] == 0) rounds = k;
        checked = launched + 1;
        if (rounds >= 0 || launched >= bound) break;
        const int upto = launched + GROUP < bound ? launched + GROUP : bound;
        for (; launched < upto; ++launched) {
            if (timed) t0 = now_ns();
            XRS_FLOW_DISPATCH(launch_round, cells, launched, b, grid, s);
            XRS_LAUNCH_CHECK();
            if (timed) { XRS_HIP(hipStreamSynchronize(s)); status_host[40 + launched] = now_ns() - t0; }
        }
    }
    unsigned bad = 0;
    XRS_HIP(hipMemcpyAsync(&bad, b.head + BAD_WORD, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    int status = bad ? XRS_FLOW_INVALID_CODE : 0;
    if (rounds < 0) { status |= XRS_FLOW_CYCLE; rounds = launched; }   // anc_bound still live somewhere
    status_host[0] = rounds;
    status_host[1] = status;
    for (int k = 0; k <= launched; ++k) status_host[4 + k] = (int64_t)live[k];
    if (status) return 0;                                                // the caller raises; no product is written

    if (timed) t0 = now_ns();
    XRS_FLOW_DISPATCH(launch_finish, dir_dev, cells, launched, b, acc_out_dev, basin_out_dev, grid, s);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status_host[3] = now_ns() - t0; }
    return 0;
}

}  // extern "C"

// fill / flow_direction(resolve_flats=True): depression fill and flat resolution in front of D8.
//
// Both are a monotone relaxation of one plane to its greatest fixed point below a start value:
//   fill    W = +inf off the rim; W(c) <- min(W(c), max(z(c), min_n W(n)))          (values: the raster's dtype)
//   flats   d = all-ones at flat cells; d(c) <- min(d(c), 1 + min d(n) over z(n) == z(c))   (values: uint32 step counts)
// A plane only ever falls and never below the fixed point, whatever the order of the updates, so the result does not depend
// on the schedule below; the schedule is still free of races, so that a run is also repeatable round by round.
//
//   tile     a block of four waves owns TILE x TILE cells and stages them with a one-cell halo in LDS.  Wave s owns rows
//            16 s .. 16 s + 15 of the tile, lane l column l: a thread keeps its 16 cells (and their elevations) in registers.
//   iterate  read phase: every thread reads its two side columns (18 cells each) and the cells above and below its strip from
//            LDS, then sweeps its strip down and up in registers, so a value crosses the strip in one iteration (and one
//            column per iteration sideways).  __syncthreads_or of "a cell of mine fell" ends the read phase: nobody writes
//            LDS before everybody has read.  Write phase: the threads store their strips; a barrier ends it.  No LDS word is
//            read in a phase in which another thread may write it.  At most CAP iterations: a tile that still moves then
//            marks itself for the next round.
//   colours  tiles are coloured 2 x 2 and every colour is a launch of its own on the stream.  A block writes its own tile
//            and reads that plus a halo whose cells all belong to tiles of other colours, which no block of the launch
//            writes: no launch reads a global word that another block of it may write.  The plane is updated in place.
//   rounds   round 0 launches every tile.  A tile in which a cell fell marks its eight neighbours (itself too when it hit CAP)
//            in a plane of flags; one launch at the end of the round turns the flags into the four tile lists of the next
//            round, clears them and sums the round's count of fallen cells (ballot counts, one add per wave, SLOTS words 256
//            bytes apart).  The host reads five words a round, launches each colour with as many blocks as its list holds
//            and stops at the first round in which nothing fell; after rows * cols + 1 rounds it returns an error.
//            No loop depends on the data without a bound, nothing waits on another block.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "tile_rounds.h"
#include "workspace.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr unsigned INF = 0xffffffffu;           // "no drained cell of this elevation reached"

template <typename T>
__device__ __forceinline__ T nan_of() { return (T)nan_f32(); }
template <typename T>
__device__ __forceinline__ T inf_of() { return (T)__int_as_float(0x7f800000); }

// ------------------------------------------------------------------ the two operators
template <typename T>
struct FillOp {
    using Z = T;
    using V = T;
    static constexpr bool Z_IN_LDS = false;     // neighbours' elevations are not looked at
    __device__ static V outside() { return nan_of<T>(); }
    __device__ static V none() { return inf_of<T>(); }
    // (a NaN neighbour is skipped; only a rim cell has one, and a rim cell never falls)
    __device__ static V join(V acc, Z, Z, V vn) { return vn < acc ? vn : acc; }
    __device__ static bool relax(V &w, Z z, V cand) {
        const V t = cand > z ? cand : z;        // a NaN cell: t = NaN, nothing is below it
        if (t < w) { w = t; return true; }
        return false;
    }
};

template <typename T>
struct FlatOp {
    using Z = T;
    using V = unsigned;
    static constexpr bool Z_IN_LDS = true;
    __device__ static V outside() { return INF; }
    __device__ static V none() { return INF; }
    __device__ static V join(V acc, Z zc, Z zn, V vn) { return (zn == zc && vn < acc) ? vn : acc; }
    __device__ static bool relax(V &w, Z, V cand) {
        const V t = cand == INF ? INF : cand + 1u;
        if (t < w) { w = t; return true; }
        return false;
    }
};

// ------------------------------------------------------------------ the tile relaxer
template <typename Op>
__global__ void __launch_bounds__(THREADS) relax_kernel(const typename Op::Z *__restrict__ z, typename Op::V *plane, long rows, long cols,
                                                        unsigned tiles_y, unsigned tiles_x, int colour, unsigned across,
                                                        const unsigned *__restrict__ list, unsigned *__restrict__ flags,
                                                        unsigned *__restrict__ head) {
    using Z = typename Op::Z;
    using V = typename Op::V;
    __shared__ V vt[LD][LD];                    // vt[r][c]: raster cell (i0 - 1 + r, j0 - 1 + c)
    __shared__ Z zt[Op::Z_IN_LDS ? LD : 1][Op::Z_IN_LDS ? LD : 1];

    unsigned tile;
    if (list) {
        tile = list[blockIdx.x];
    } else {                                    // round 0: every tile of the colour
        const unsigned a = blockIdx.x / across, b = blockIdx.x - a * across;
        tile = (2u * a + (unsigned)(colour >> 1)) * tiles_x + 2u * b + (unsigned)(colour & 1);
    }
    const unsigned ti = tile / tiles_x, tj = tile - ti * tiles_x;
    if (ti >= tiles_y) return;                  // (cannot happen: the lists hold tile numbers only)
    const long i0 = (long)ti * TILE, j0 = (long)tj * TILE;
    const int t = threadIdx.x, lane = t & 63, r0 = (t >> 6) * STRIP;
    const long j = j0 + lane;
    const bool col_ok = j < cols;

    Z zc[STRIP];
    V w[STRIP];
#pragma unroll
    for (int k = 0; k < STRIP; ++k) {
        const long i = i0 + r0 + k;
        const bool ok = col_ok && i < rows;
        zc[k] = ok ? z[i * cols + j] : nan_of<Z>();
        w[k] = ok ? plane[i * cols + j] : Op::outside();
    }
#pragma unroll
    for (int k = 0; k < STRIP; ++k) {
        vt[1 + r0 + k][1 + lane] = w[k];
        if (Op::Z_IN_LDS) zt[1 + r0 + k][1 + lane] = zc[k];
    }
    for (int h = t; h < HALO; h += THREADS) {   // the ring: top row, bottom row, left column, right column
        int r, c;
        if (h < LD) { r = 0; c = h; }
        else if (h < 2 * LD) { r = LD - 1; c = h - LD; }
        else if (h < 2 * LD + TILE) { r = 1 + h - 2 * LD; c = 0; }
        else { r = 1 + h - 2 * LD - TILE; c = LD - 1; }
        const long i = i0 - 1 + r, q = j0 - 1 + c;
        const bool ok = i >= 0 && i < rows && q >= 0 && q < cols;
        vt[r][c] = ok ? plane[i * cols + q] : Op::outside();
        if (Op::Z_IN_LDS) zt[r][c] = ok ? z[i * cols + q] : nan_of<Z>();
    }
    __syncthreads();

    unsigned fell = 0;                          // bit k: cell k of the strip fell in this launch
    bool ever = false, pending = false;         // (block-uniform)
    for (int it = 0;;) {
        // ---- read phase
        V side[STRIP + 2], m[STRIP];
        Z zs[STRIP + 2];
#pragma unroll
        for (int q = 0; q < STRIP + 2; ++q) {
            side[q] = vt[r0 + q][lane];
            zs[q] = Op::Z_IN_LDS ? zt[r0 + q][lane] : Z(0);
        }
#pragma unroll
        for (int k = 0; k < STRIP; ++k)         // NW, W, SW
            m[k] = Op::join(Op::join(Op::join(Op::none(), zc[k], zs[k], side[k]), zc[k], zs[k + 1], side[k + 1]), zc[k], zs[k + 2], side[k + 2]);
#pragma unroll
        for (int q = 0; q < STRIP + 2; ++q) {
            side[q] = vt[r0 + q][lane + 2];
            zs[q] = Op::Z_IN_LDS ? zt[r0 + q][lane + 2] : Z(0);
        }
#pragma unroll
        for (int k = 0; k < STRIP; ++k)         // NE, E, SE
            m[k] = Op::join(Op::join(Op::join(m[k], zc[k], zs[k], side[k]), zc[k], zs[k + 1], side[k + 1]), zc[k], zs[k + 2], side[k + 2]);
        const V top = vt[r0][1 + lane], bot = vt[r0 + STRIP + 1][1 + lane];
        const Z ztop = Op::Z_IN_LDS ? zt[r0][1 + lane] : Z(0), zbot = Op::Z_IN_LDS ? zt[r0 + STRIP + 1][1 + lane] : Z(0);
        unsigned now = 0;
#pragma unroll
        for (int k = 0; k < STRIP; ++k) {       // down: the cell above has its new value
            const V up = k ? w[k - 1] : top, dn = k < STRIP - 1 ? w[k + 1] : bot;
            const Z zu = k ? zc[k - 1] : ztop, zd = k < STRIP - 1 ? zc[k + 1] : zbot;
            const V cand = Op::join(Op::join(m[k], zc[k], zu, up), zc[k], zd, dn);
            if (Op::relax(w[k], zc[k], cand)) now |= 1u << k;
        }
#pragma unroll
        for (int k = STRIP - 2; k >= 0; --k) {  // up: only the cell below is news
            const V cand = Op::join(Op::none(), zc[k], zc[k + 1], w[k + 1]);
            if (Op::relax(w[k], zc[k], cand)) now |= 1u << k;
        }
        fell |= now;
        if (!__syncthreads_or(now != 0)) break; // every read of this iteration is done
        ever = true;
        if (++it == CAP) { pending = true; break; }
        // ---- write phase
        if (now) {
#pragma unroll
            for (int k = 0; k < STRIP; ++k) vt[1 + r0 + k][1 + lane] = w[k];
        }
        __syncthreads();
    }
    if (!ever) return;

    unsigned n = 0;
#pragma unroll
    for (int k = 0; k < STRIP; ++k) {
        const bool mine = (fell >> k) & 1u;
        const long i = i0 + r0 + k;
        if (mine && col_ok && i < rows) plane[i * cols + j] = w[k];
        n += (unsigned)__popcll(__ballot(mine));
    }
    if (lane == 0 && n != 0) atomicAdd(head + ((tile * 4u + (unsigned)(t >> 6)) & (SLOTS - 1)) * SLOT_STRIDE, n);
    if (t < 9) {
        const int di = t / 3 - 1, dj = t % 3 - 1;
        const long ni = (long)ti + di, nj = (long)tj + dj;
        if ((di != 0 || dj != 0 || pending) && ni >= 0 && ni < (long)tiles_y && nj >= 0 && nj < (long)tiles_x)
            atomicOr(flags + ni * tiles_x + nj, 1u);
    }
}

// ------------------------------------------------------------------ first and last launches
template <typename T>
__device__ __forceinline__ bool rim_cell(const T *__restrict__ z, long i, long j, long rows, long cols) {
    if (i == 0 || j == 0 || i == rows - 1 || j == cols - 1) return true;
    bool rim = false;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
            const T v = z[(i + di) * cols + (j + dj)];
            rim |= v != v;
        }
    return rim;
}

template <typename T>
__global__ void __launch_bounds__(THREADS) fill_init_kernel(const T *__restrict__ z, T *__restrict__ out, long rows, long cols) {
    const long u = (long)blockIdx.x * THREADS + threadIdx.x;
    if (u >= rows * cols) return;
    const long i = (long)((unsigned)u / (unsigned)cols), j = u - i * cols;      // (cells and cols fit 32 bits)
    const T zc = z[u];
    out[u] = (zc != zc || rim_cell(z, i, j, rows, cols)) ? zc : inf_of<T>();
}

template <typename T>
__global__ void __launch_bounds__(THREADS) flat_init_kernel(const T *__restrict__ z, const float *__restrict__ code, unsigned *__restrict__ d,
                                                            long rows, long cols) {
    const long u = (long)blockIdx.x * THREADS + threadIdx.x;
    if (u >= rows * cols) return;
    const long i = (long)((unsigned)u / (unsigned)cols), j = u - i * cols;
    const T zc = z[u];
    unsigned v = INF;                                                    // NaN cells: never equal to a neighbour
    if (zc == zc && (code[u] != 0.0f || rim_cell(z, i, j, rows, cols))) v = 0u;
    d[u] = v;
}

// a flat cell with a finite count takes the first neighbour of its elevation that is one step nearer
template <typename T>
__global__ void __launch_bounds__(THREADS) flat_codes_kernel(const T *__restrict__ z, const unsigned *__restrict__ d, float *__restrict__ code,
                                                             long rows, long cols) {
    const long u = (long)blockIdx.x * THREADS + threadIdx.x;
    if (u >= rows * cols) return;
    const unsigned dc = d[u];
    if (dc == 0u || dc == INF) return;
    const long i = (long)((unsigned)u / (unsigned)cols), j = u - i * cols;
    const T zc = z[u];
    const int dr[8] = {0, 1, 1, 1, 0, -1, -1, -1}, dq[8] = {1, 1, 0, -1, -1, -1, 0, 1};
    int c = 0;
#pragma unroll
    for (int k = 7; k >= 0; --k) {                                       // backwards, so that the first in the order stays
        const long r = i + dr[k], q = j + dq[k];
        if (r >= 0 && r < rows && q >= 0 && q < cols) {
            const long v = r * cols + q;
            if (z[v] == zc && d[v] == dc - 1u) c = 1 << k;
        }
    }
    code[u] = (float)c;
}

struct Work {
    RoundWork rounds;
    unsigned *d;
    size_t total;
};
Work carve(void *base, size_t rows, size_t cols, bool with_d) {
    Carver c(base);
    Work w = {};
    w.rounds = carve_rounds(c, rows, cols);
    if (with_d) w.d = c.take<unsigned>(rows * cols);
    w.total = c.at();
    return w;
}

// the rounds of tile_rounds.h with relax_kernel<Op> as the launch of a colour
template <typename Op>
int run_rounds(const char *what, const typename Op::Z *z, typename Op::V *plane, long rows, long cols, const Work &wk, int64_t *status,
               bool timed, hipStream_t s) {
    return run_tile_rounds(what, rows, cols, wk.rounds, status, timed, s,
                           [&](int colour, unsigned blocks, unsigned across, unsigned tiles_y, unsigned tiles_x, const unsigned *list) {
                               hipLaunchKernelGGL((relax_kernel<Op>), dim3(blocks), dim3(THREADS), 0, s, z, plane, rows, cols, tiles_y, tiles_x,
                                                  colour, across, list, wk.rounds.flags, wk.rounds.head);
                           });
}

int check_call(const char *what, const void *z, int dtype, int64_t rows, int64_t cols, const void *plane, const void *work, int64_t *status,
               int flags, bool *empty) {
    *empty = true;
    if (rows < 0 || cols < 0) return fail("%s: negative shape", what);
    if (!dtype_in(DT_FLOATS, dtype)) return fail("%s: unsupported dtype code %d (float32 or float64)", what, dtype);
    if (flags & ~XRS_FILL_TIMED) return fail("%s: unknown flags %d", what, flags);
    if (!status) return fail("%s: null status pointer", what);
    for (int w = 0; w < XRS_FILL_STATUS_WORDS; ++w) status[w] = 0;
    if (rows == 0 || cols == 0) return 0;
    if ((uint64_t)rows > XRS_FLOW_MAX_CELLS / (uint64_t)cols)
        return fail("%s: more than 2^32 - 2 cells (%lld x %lld)", what, (long long)rows, (long long)cols);
    if (!z || !plane || !work) return fail("%s: null pointer", what);
    if (z == plane) return fail("%s: the result cannot overwrite the elevations", what);
    *empty = false;
    return 0;
}

template <typename T>
int fill_typed(const T *z, long rows, long cols, T *out, void *work, int64_t *status, bool timed, hipStream_t s) {
    const unsigned grid = (unsigned)(((uint64_t)rows * (uint64_t)cols + THREADS - 1) / THREADS);   // < 2^24 blocks
    int64_t t0 = 0;
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); t0 = now_ns(); }
    hipLaunchKernelGGL((fill_init_kernel<T>), dim3(grid), dim3(THREADS), 0, s, z, out, rows, cols);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status[2] = now_ns() - t0; }
    if (rows < 3 || cols < 3) return 0;                                  // every cell is a rim cell
    return run_rounds<FillOp<T>>("xrs_fill", z, out, rows, cols, carve(work, (size_t)rows, (size_t)cols, false), status, timed, s);
}

template <typename T>
int flats_typed(const T *z, long rows, long cols, float *code, void *work, int64_t *status, bool timed, hipStream_t s) {
    if (rows < 3 || cols < 3) return 0;                                  // every cell is a rim cell: all drained
    const Work wk = carve(work, (size_t)rows, (size_t)cols, true);
    const unsigned grid = (unsigned)(((uint64_t)rows * (uint64_t)cols + THREADS - 1) / THREADS);
    int64_t t0 = 0;
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); t0 = now_ns(); }
    hipLaunchKernelGGL((flat_init_kernel<T>), dim3(grid), dim3(THREADS), 0, s, z, (const float *)code, wk.d, rows, cols);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status[2] = now_ns() - t0; }
    if (int rc = run_rounds<FlatOp<T>>("xrs_flow_flats", z, wk.d, rows, cols, wk, status, timed, s)) return rc;
    if (timed) t0 = now_ns();
    hipLaunchKernelGGL((flat_codes_kernel<T>), dim3(grid), dim3(THREADS), 0, s, z, (const unsigned *)wk.d, code, rows, cols);
    XRS_LAUNCH_CHECK();
    if (timed) { XRS_HIP(hipStreamSynchronize(s)); status[3] = now_ns() - t0; }
    return 0;
}

int workspace_size(const char *what, int64_t rows, int64_t cols, bool with_d, uint64_t *bytes_out) {
    if (!bytes_out) return fail("%s: null pointer", what);
    *bytes_out = 0;
    if (rows <= 0 || cols <= 0 || (uint64_t)rows > XRS_FLOW_MAX_CELLS / (uint64_t)cols) return 0;
    *bytes_out = carve(nullptr, (size_t)rows, (size_t)cols, with_d).total;
    return 0;
}

}  // namespace

extern "C" {

int xrs_fill_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out) {
    return workspace_size("xrs_fill_workspace_size", rows, cols, false, bytes_out);
}

int xrs_fill(const void *z_dev, int dtype, int64_t rows, int64_t cols, void *out_dev, void *work_dev, int64_t *status_host, int flags,
             void *stream) {
    bool empty;
    if (int rc = check_call("xrs_fill", z_dev, dtype, rows, cols, out_dev, work_dev, status_host, flags, &empty)) return rc;
    if (empty) return 0;
    const bool timed = flags & XRS_FILL_TIMED;
    int rc = 0;
    with_dtype<DT_FLOATS>(dtype, [&](auto t) {                    // check_call refused every other code
        using T = dtype_of<decltype(t)>;
        rc = fill_typed(static_cast<const T *>(z_dev), (long)rows, (long)cols, static_cast<T *>(out_dev), work_dev, status_host, timed,
                        as_stream(stream));
    });
    return rc;
}

int xrs_flow_flats_workspace_size(int64_t rows, int64_t cols, uint64_t *bytes_out) {
    return workspace_size("xrs_flow_flats_workspace_size", rows, cols, true, bytes_out);
}

int xrs_flow_flats(const void *z_dev, int dtype, int64_t rows, int64_t cols, float *code_dev, void *work_dev, int64_t *status_host, int flags,
                   void *stream) {
    bool empty;
    if (int rc = check_call("xrs_flow_flats", z_dev, dtype, rows, cols, code_dev, work_dev, status_host, flags, &empty)) return rc;
    if (empty) return 0;
    const bool timed = flags & XRS_FILL_TIMED;
    int rc = 0;
    with_dtype<DT_FLOATS>(dtype, [&](auto t) {                    // check_call refused every other code
        rc = flats_typed(static_cast<const dtype_of<decltype(t)> *>(z_dev), (long)rows, (long)cols, code_dev, work_dev, status_host, timed,
                         as_stream(stream));
    });
    return rc;
}

}  // extern "C"

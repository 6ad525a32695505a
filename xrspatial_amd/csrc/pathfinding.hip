// a_star_search: the shortest 4- or 8-connected path between two cells of a raster.
//
// Reference: xrspatial/pathfinding.py:145-230 `_a_star_search`, an A* whose open list is scanned whole at every pop.  Its
// heuristic is admissible, so what it returns is a shortest path; what is computed here is the shortest-distance field of the
// grid graph from the GOAL and one walk along it from the start:
//   crossable  a cell that is not NaN and equals no barrier value (value_match.h, as proximity's target_values);
//   D(c)       the exact shortest distance goal -> c as the integer pair (a, b): a steps of 1.0 and b steps of sqrt(2).  One
//              64-bit word per cell, a in the high half and b in the low half; all-ones = not reached, all-ones - 1 = not
//              crossable.  Two distances compare in integers (sqrt(2) is irrational, so the pair of a shortest path is
//              unique): the sign of da + db sqrt(2) follows from the signs of da and db and, when they oppose, from da^2
//              against 2 db^2 -- at most 2^30 cells keep both inside int64.  Never a lexicographic compare of the word.
//   walk       from the start, at every cell the first neighbour n in the reference's neighbour order with
//              D(n) + step == D(cur) exactly; exactly a + b steps; out = the float64 running sum g = g + (1.0 or
//              1.4142135623730951) in walk order, the arithmetic of the reference's d_from_start; NaN everywhere else.
// Launches: init (field, NaN plane), snap partials (only when asked for), setup (snap result, flags, the goal's 0 and the
// dirty marks around it), relax repeated, walk.
//   relax    one workgroup per 64 x 32 tile, and NO communication between workgroups inside a launch: a tile that is not
//            marked dirty returns at once; a dirty one loads itself and a one-cell halo into LDS (relaxed 64-bit atomic loads at
//            agent scope: a neighbour may lower a halo word during the same launch; every value ever stored is the length of a
//            real path, so whatever is read is a valid upper bound) and iterates pull-style, every cell the exact minimum of
//            itself and neighbour + step, between two LDS buffers (read one, write the other, one barrier: nothing can tear and
//            the result does not depend on the order of the waves), at most 64 * 32 times -- after k rounds every cell whose
//            best path inside the tile has k hops is final, and no path inside a tile has more than 64 * 32 - 1.  A tile that
//            lowered a cell writes its words back, marks itself and its eight neighbours in the NEXT pass's dirty array and
//            sets the pass's `changed` word.  A tile's cells are written by its own workgroup only.
//   passes   launched in groups; after a group the host reads the group's `changed` words and stops at the first pass that
//            changed nothing.  Launch boundaries make every word visible to the next pass.  While the field is not final, take
//            the cell c with the smallest true distance among the non-final ones: its predecessor p is final; the pass that
//            made p final marked c's tile dirty, so the next pass reads p and makes c final (had p and c shared a tile, the
//            tile's own iteration would have done so already).  So every pass but the last makes one more cell final: at most
//            rows * cols + 2 passes, and beyond that the call fails instead of looping.
// No floating point but the walk's sum, and that is an add of literals: nothing here can be contracted.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "value_match.h"
#include "wave_reduce.h"
#include "workspace.h"

#include <cmath>
#include <type_traits>

using namespace xrs;

namespace {

constexpr int TW = 64, TH = 32, NT = 256;              // the tile of regions.hip, four waves
constexpr int CELLS_PER_THREAD = TW * TH / NT;
constexpr uint64_t UNREACHED = ~0ull, BLOCKED = ~0ull - 1;      // every word >= BLOCKED holds no distance
constexpr uint64_t STEP_STRAIGHT = 1ull << 32, STEP_DIAGONAL = 1ull;
constexpr int MAX_GROUP = 64, DEFAULT_GROUP = 8;       // passes per host round trip (profiles/pathfinding/)
constexpr int SNAP_BLOCKS = 1024;
constexpr long long NO_KEY = 0x7fffffffffffffffLL;
// device status words (int64): the eight of `status_host` (the last one is filled in by the host) the walk's error word and the
// number of tiles the passes loaded
constexpr int ST_START_ROW = 0, ST_START_COL = 1, ST_GOAL_ROW = 2, ST_FLAGS = 4, ST_A = 5, ST_B = 6, ST_ERROR = 8, ST_VISITS = 9;
constexpr int ST_WORDS = 16;

struct Work {
    uint64_t *field;
    int *dirty[2], *changed;
    long long *st, *partial;
    size_t zero_bytes, total;       // zero_bytes from dirty[0]: both dirty arrays, changed, status -- cleared per call
    long tiles_x, tiles_y;
};
Work carve(void *base, size_t rows, size_t cols) {
    Carver c(base);
    Work w = {};
    w.tiles_x = (long)((cols + TW - 1) / TW);
    w.tiles_y = (long)((rows + TH - 1) / TH);
    const size_t tiles = (size_t)w.tiles_x * (size_t)w.tiles_y;
    w.field = c.take<uint64_t>(rows * cols);
    const size_t zero_from = c.at();
    w.dirty[0] = c.take<int>(tiles);
    w.dirty[1] = c.take<int>(tiles);
    w.changed = c.take<int>(MAX_GROUP);
    w.st = c.take<long long>(ST_WORDS);
    w.zero_bytes = c.at() - zero_from;
    w.partial = c.take<long long>((size_t)SNAP_BLOCKS * 4);
    w.total = c.at();
    return w;
}

// is a < b for two distances (a1, b1), (a2, b2) packed as above?  Exact.
__device__ __forceinline__ bool shorter(uint64_t x, uint64_t y) {
    const long long da = (long long)(x >> 32) - (long long)(y >> 32);
    const long long db = (long long)(x & 0xffffffffull) - (long long)(y & 0xffffffffull);
    if (da <= 0 && db <= 0) return (da | db) != 0;
    if (da >= 0 && db >= 0) return false;
    const long long p = da * da, q = 2 * db * db;                        // da + db sqrt(2) < 0 ?
    return da < 0 ? p > q : p < q;
}

template <typename T>
__global__ void __launch_bounds__(NT) astar_init_kernel(const T *__restrict__ data, long n, const void *__restrict__ barriers, int kind,
                                                        int n_barriers, uint64_t *__restrict__ field, double *__restrict__ out) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const T v = data[i];
    bool blocked = false;
    if constexpr (std::is_floating_point<T>::value) blocked = v != v;
    if (!blocked && n_barriers > 0) blocked = matches_any<T>(v, barriers, kind, n_barriers);
    field[i] = blocked ? BLOCKED : UNREACHED;
    out[i] = __longlong_as_double(0x7ff8000000000000LL);
}

// `_find_nearest_pixel` of the start (which = 0) and the goal (which = 1): per block the smallest (d^2, row-major index) over
// the crossable cells, into partial[block * 4 + 2 * which + {0, 1}]
__global__ void __launch_bounds__(NT) astar_snap_kernel(const uint64_t *__restrict__ field, long rows, long cols, long pr0, long pc0,
                                                        long pr1, long pc1, long long *__restrict__ partial) {
    __shared__ long long part[4][4];
    const long n = rows * cols;
    const long stride = (long)gridDim.x * NT;
    long long d2[2] = {NO_KEY, NO_KEY}, at[2] = {NO_KEY, NO_KEY};
    const long rounds = (n + stride - 1) / stride;
    for (long k = 0; k < rounds; ++k) {
        const long i = k * stride + (long)blockIdx.x * NT + threadIdx.x;   // ascending per thread: the first of equals stays
        if (i >= n || field[i] == BLOCKED) continue;
        const long r = i / cols, c = i - r * cols;
        const long long e0 = (r - pr0) * (r - pr0) + (c - pc0) * (c - pc0), e1 = (r - pr1) * (r - pr1) + (c - pc1) * (c - pc1);
        if (e0 < d2[0]) { d2[0] = e0; at[0] = i; }
        if (e1 < d2[1]) { d2[1] = e1; at[1] = i; }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const long long m = wave_reduce<WrMin>(d2[w]);
        const long long first = wave_reduce<WrMin>(d2[w] == m ? at[w] : NO_KEY);
        if (lane == 0) { part[wave][2 * w] = m; part[wave][2 * w + 1] = first; }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int w = threadIdx.x;
        long long m = NO_KEY, first = NO_KEY;
        for (int k = 0; k < 4; ++k) {
            const long long pm = part[k][2 * w], pf = part[k][2 * w + 1];
            if (pm < m || (pm == m && pf < first)) { m = pm; first = pf; }
        }
        partial[(long)blockIdx.x * 4 + 2 * w] = m;
        partial[(long)blockIdx.x * 4 + 2 * w + 1] = first;
    }
}

// one wave: the snapped cells, the flags, the goal's distance 0 and the dirty marks of its tile and the eight around it
__global__ void __launch_bounds__(64) astar_setup_kernel(uint64_t *__restrict__ field, long rows, long cols, long pr0, long pc0, long pr1,
                                                         long pc1, int snap_flags, const long long *__restrict__ partial, int n_partial,
                                                         long tiles_x, long tiles_y, int *__restrict__ dirty, long long *__restrict__ st) {
    const int lane = threadIdx.x;
    const long n = rows * cols;
    long cell[2] = {pr0 * cols + pc0, pr1 * cols + pc1};
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        if (!(snap_flags & (1 << w)) || field[cell[w]] != BLOCKED) continue;             // (wave-uniform)
        long long m = NO_KEY, first = NO_KEY;
        for (int k = lane; k < n_partial; k += 64) {
            const long long pm = partial[(long)k * 4 + 2 * w], pf = partial[(long)k * 4 + 2 * w + 1];
            if (pm < m || (pm == m && pf < first)) { m = pm; first = pf; }
        }
        const long long best = wave_reduce<WrMin>(m);
        const long long at = wave_reduce<WrMin>(m == best ? first : NO_KEY);
        // the reference starts from min_distance = the raster's diagonal and keeps what is strictly nearer
        cell[w] = (best != NO_KEY && best < (rows - 1) * (rows - 1) + (cols - 1) * (cols - 1)) ? (long)at : -1;
    }
    if (lane != 0) return;
    // the reference's warnings look at data[row, col] after snapping, and (-1, -1) is the raster's last cell to NumPy
    const bool start_ok = field[cell[0] >= 0 ? cell[0] : n - 1] != BLOCKED, goal_ok = field[cell[1] >= 0 ? cell[1] : n - 1] != BLOCKED;
    for (int w = 0; w < 2; ++w) {
        st[2 * w] = cell[w] >= 0 ? cell[w] / cols : -1;
        st[2 * w + 1] = cell[w] >= 0 ? cell[w] % cols : -1;
    }
    st[ST_FLAGS] = (start_ok ? XRS_ASTAR_START_CROSSABLE : 0) | (goal_ok ? XRS_ASTAR_GOAL_CROSSABLE : 0);
    st[ST_A] = st[ST_B] = -1;
    st[7] = 0;
    st[ST_ERROR] = 0;
    if (cell[0] >= 0 && cell[1] >= 0 && start_ok && goal_ok) {
        field[cell[1]] = 0;
        // the goal's word is lowered here, not by a relaxation: mark what a relaxation would have marked
        const long ty = cell[1] / cols / TH, tx = (cell[1] % cols) / TW;
        for (int k = 0; k < 9; ++k) {
            const long ny = ty + k / 3 - 1, nx = tx + k % 3 - 1;
            if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x) dirty[ny * tiles_x + nx] = 1;
        }
    }
}

__device__ __forceinline__ uint64_t load_word(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_word(uint64_t *p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool EIGHT>
__global__ void __launch_bounds__(NT) astar_relax_kernel(uint64_t *__restrict__ field, long rows, long cols, long tiles_x, long tiles_y,
                                                         int *__restrict__ dirty_now, int *__restrict__ dirty_next,
                                                         int *__restrict__ changed, unsigned long long *__restrict__ visits) {
    __shared__ uint64_t buf[2][TH + 2][TW + 2];          // 2 x 34 x 66 words: 35 904 bytes
    __shared__ int go;
    const long tile = blockIdx.x;
    const int t = threadIdx.x;
    if (t == 0) {
        go = dirty_now[tile];
        dirty_now[tile] = 0;                             // this launch consumes the mark; nobody else touches it now
    }
    __syncthreads();
    if (!go) return;
    if (t == 0) atomicAdd(visits, 1ull);                 // (for tools/pathfinding_bench.py: the traffic of a pass)
    const long ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const long r0 = ty * TH, c0 = tx * TW;

    for (int k = t; k < (TH + 2) * (TW + 2); k += NT) {
        const int ly = k / (TW + 2), lx = k - ly * (TW + 2);
        const long r = r0 + ly - 1, c = c0 + lx - 1;
        const uint64_t w = (r >= 0 && r < rows && c >= 0 && c < cols) ? load_word(field + r * cols + c) : BLOCKED;
        buf[0][ly][lx] = w;
        buf[1][ly][lx] = w;
    }
    __syncthreads();

    uint64_t loaded[CELLS_PER_THREAD];
#pragma unroll
    for (int j = 0; j < CELLS_PER_THREAD; ++j) loaded[j] = buf[0][(t >> 6) + 4 * j + 1][(t & 63) + 1];

    int cur = 0;
    for (int round = 0; round < TW * TH; ++round) {
        int lowered = 0;
#pragma unroll
        for (int j = 0; j < CELLS_PER_THREAD; ++j) {
            const int ly = (t >> 6) + 4 * j + 1, lx = (t & 63) + 1;
            const uint64_t me = buf[cur][ly][lx];
            uint64_t best = me;
            if (me != BLOCKED) {
                auto pull = [&](int dy, int dx, uint64_t step) {
                    const uint64_t w = buf[cur][ly + dy][lx + dx];
                    if (w >= BLOCKED) return;
                    const uint64_t cand = w + step;
                    if (best == UNREACHED || shorter(cand, best)) best = cand;
                };
                pull(0, -1, STEP_STRAIGHT);
                pull(-1, 0, STEP_STRAIGHT);
                pull(1, 0, STEP_STRAIGHT);
                pull(0, 1, STEP_STRAIGHT);
                if (EIGHT) {
                    pull(-1, -1, STEP_DIAGONAL);
                    pull(1, -1, STEP_DIAGONAL);
                    pull(-1, 1, STEP_DIAGONAL);
                    pull(1, 1, STEP_DIAGONAL);
                }
            }
            buf[cur ^ 1][ly][lx] = best;
            lowered |= best != me;
        }
        cur ^= 1;
        if (!__syncthreads_or(lowered)) break;
    }

    int wrote = 0;
#pragma unroll
    for (int j = 0; j < CELLS_PER_THREAD; ++j) {
        const int ly = (t >> 6) + 4 * j + 1, lx = (t & 63) + 1;
        const uint64_t w = buf[cur][ly][lx];
        if (w != loaded[j]) {                            // (only cells inside the raster can change)
            store_word(field + (r0 + ly - 1) * cols + (c0 + lx - 1), w);
            wrote = 1;
        }
    }
    if (!__syncthreads_or(wrote)) return;
    if (t < 9) {
        const long ny = ty + t / 3 - 1, nx = tx + t % 3 - 1;
        if (ny >= 0 && ny < tiles_y && nx >= 0 && nx < tiles_x) dirty_next[ny * tiles_x + nx] = 1;
    }
    if (t == 0) *changed = 1;
}

// one wave walks from the start; lanes 0 .. 7 (0 .. 3) look at the neighbours in the reference's order
template <bool EIGHT>
__global__ void __launch_bounds__(64) astar_walk_kernel(const uint64_t *__restrict__ field, long rows, long cols, long long *__restrict__ st,
                                                        double *__restrict__ out) {
    // `_neighborhood_structure`: (dy, dx) per neighbour
    constexpr int DY8[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, DX8[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
    constexpr int DY4[4] = {0, -1, 1, 0}, DX4[4] = {-1, 0, 0, 1};
    const int lane = threadIdx.x;
    if (st[ST_START_ROW] < 0 || st[ST_GOAL_ROW] < 0) return;
    long r = st[ST_START_ROW], c = st[ST_START_COL];
    uint64_t d = field[r * cols + c];
    if (d >= BLOCKED) return;                            // no path (a blocked goal never got its 0)
    const long steps = (long)(d >> 32) + (long)(d & 0xffffffffull);
    if (lane == 0) {
        st[ST_A] = (long long)(d >> 32);
        st[ST_B] = (long long)(d & 0xffffffffull);
        st[ST_FLAGS] |= XRS_ASTAR_PATH_FOUND;
        out[r * cols + c] = 0.0;
    }
    const int n_nb = EIGHT ? 8 : 4;
    const int k = lane < n_nb ? lane : 0;
    const int dy = EIGHT ? DY8[k] : DY4[k], dx = EIGHT ? DX8[k] : DX4[k];
    const uint64_t step = (dy != 0 && dx != 0) ? STEP_DIAGONAL : STEP_STRAIGHT;
    double g = 0.0;
    for (long s = 0; s < steps; ++s) {
        bool hit = false;
        const long nr = r + dy, nc = c + dx;
        if (lane < n_nb && nr >= 0 && nr < rows && nc >= 0 && nc < cols) {
            const uint64_t w = field[nr * cols + nc];
            hit = w < BLOCKED && w + step == d;
        }
        const unsigned long long votes = __ballot(hit);
        if (votes == 0) {                                // cannot happen on a converged field
            if (lane == 0) st[ST_ERROR] = 1;
            return;
        }
        const int pick = __ffsll(votes) - 1;
        const int py = EIGHT ? DY8[pick] : DY4[pick], px = EIGHT ? DX8[pick] : DX4[pick];
        const bool diagonal = py != 0 && px != 0;
        r += py;
        c += px;
        d -= diagonal ? STEP_DIAGONAL : STEP_STRAIGHT;
        g = g + (diagonal ? 1.4142135623730951 : 1.0);
        if (lane == 0) out[r * cols + c] = g;
    }
}

template <typename T>
void launch_init(const void *data, long n, const void *barriers, int kind, int n_barriers, uint64_t *field, double *out, hipStream_t s) {
    hipLaunchKernelGGL((astar_init_kernel<T>), dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, static_cast<const T *>(data), n, barriers,
                       kind, n_barriers, field, out);
}

}  // namespace

extern "C" {

size_t xrs_astar_workspace_bytes(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || rows > XRS_ASTAR_MAX_CELLS || cols > XRS_ASTAR_MAX_CELLS || rows * cols > XRS_ASTAR_MAX_CELLS) return 0;
    return carve(nullptr, (size_t)rows, (size_t)cols).total;
}

int xrs_astar(const void *data_dev, int dtype, int64_t rows, int64_t cols, int64_t start_row, int64_t start_col, int64_t goal_row,
              int64_t goal_col, const void *barriers_dev, int barriers_kind, int n_barriers, int connectivity, int snap_flags,
              void *work_dev, double *out_dev, int64_t *status_host, void *stream) {
    if (rows < 0 || cols < 0) return fail("xrs_astar: negative shape");
    if (connectivity != 4 && connectivity != 8) return fail("xrs_astar: connectivity %d is neither 4 nor 8", connectivity);
    if (!dtype_bytes(dtype)) return fail("xrs_astar: unsupported dtype code %d", dtype);
    if (n_barriers < 0) return fail("xrs_astar: negative number of barrier values");
    if (barriers_kind != XRS_PROX_VALUES_F64 && barriers_kind != XRS_PROX_VALUES_I64 && barriers_kind != XRS_PROX_VALUES_U64)
        return fail("xrs_astar: unknown kind of barrier values %d", barriers_kind);
    if (barriers_kind != XRS_PROX_VALUES_F64 && (dtype == XRS_DT_F32 || dtype == XRS_DT_F64))
        return fail("xrs_astar: a float raster is compared with float64 barrier values");
    const int group = (snap_flags >> XRS_ASTAR_GROUP_SHIFT) & 0xff;
    if (snap_flags & ~(XRS_ASTAR_SNAP_START | XRS_ASTAR_SNAP_GOAL | XRS_ASTAR_NO_WALK | (0xff << XRS_ASTAR_GROUP_SHIFT)) || group > MAX_GROUP)
        return fail("xrs_astar: unknown snap_flags 0x%x", snap_flags);
    if (rows > XRS_ASTAR_MAX_CELLS || cols > XRS_ASTAR_MAX_CELLS || rows * cols > XRS_ASTAR_MAX_CELLS)
        return fail("xrs_astar: raster too large (%lld x %lld): more than 2^30 cells", (long long)rows, (long long)cols);
    if (start_row < 0 || start_row >= rows || start_col < 0 || start_col >= cols) return fail("xrs_astar: start outside the raster");
    if (goal_row < 0 || goal_row >= rows || goal_col < 0 || goal_col >= cols) return fail("xrs_astar: goal outside the raster");
    if (!data_dev || !work_dev || !out_dev || !status_host || (n_barriers > 0 && !barriers_dev)) return fail("xrs_astar: null pointer");

    hipStream_t s = as_stream(stream);
    const long n = rows * cols;
    const Work w = carve(work_dev, (size_t)rows, (size_t)cols);
    const long tiles = w.tiles_x * w.tiles_y;
    XRS_HIP(hipMemsetAsync(w.dirty[0], 0, w.zero_bytes, s));

    with_dtype_f32_last(dtype, [&](auto t) {   // (the code was checked above)
        launch_init<dtype_of<decltype(t)>>(data_dev, n, barriers_dev, barriers_kind, n_barriers, w.field, out_dev, s);
    });
    XRS_LAUNCH_CHECK();
    int n_partial = 0;
    if (snap_flags & (XRS_ASTAR_SNAP_START | XRS_ASTAR_SNAP_GOAL)) {
        n_partial = (int)((n + NT - 1) / NT < SNAP_BLOCKS ? (n + NT - 1) / NT : SNAP_BLOCKS);
        hipLaunchKernelGGL(astar_snap_kernel, dim3((unsigned)n_partial), dim3(NT), 0, s, w.field, (long)rows, (long)cols, (long)start_row,
                           (long)start_col, (long)goal_row, (long)goal_col, w.partial);
        XRS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(astar_setup_kernel, dim3(1), dim3(64), 0, s, w.field, (long)rows, (long)cols, (long)start_row, (long)start_col,
                       (long)goal_row, (long)goal_col, snap_flags, w.partial, n_partial, w.tiles_x, w.tiles_y, w.dirty[0], w.st);
    XRS_LAUNCH_CHECK();

    const long cap = n + 2;                              // Bellman-Ford: every pass but the last makes one more cell final
    const int per_group = group ? group : DEFAULT_GROUP;
    long passes = 0;
    bool settled = false;
    int seen[MAX_GROUP];
    while (!settled) {
        if (passes >= cap) return fail("xrs_astar: the distance field did not settle within %ld passes", cap);
        const int now = (int)(cap - passes < per_group ? cap - passes : per_group);
        XRS_HIP(hipMemsetAsync(w.changed, 0, MAX_GROUP * 4, s));
        for (int i = 0; i < now; ++i) {
            const long p = passes + i;
            if (connectivity == 8)
                hipLaunchKernelGGL((astar_relax_kernel<true>), dim3((unsigned)tiles), dim3(NT), 0, s, w.field, (long)rows, (long)cols, w.tiles_x,
                                   w.tiles_y, w.dirty[p & 1], w.dirty[(p + 1) & 1], w.changed + i,
                                   (unsigned long long *)(w.st + ST_VISITS));
            else
                hipLaunchKernelGGL((astar_relax_kernel<false>), dim3((unsigned)tiles), dim3(NT), 0, s, w.field, (long)rows, (long)cols, w.tiles_x,
                                   w.tiles_y, w.dirty[p & 1], w.dirty[(p + 1) & 1], w.changed + i,
                                   (unsigned long long *)(w.st + ST_VISITS));
            XRS_LAUNCH_CHECK();
        }
        XRS_HIP(hipMemcpyAsync(seen, w.changed, now * 4, hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < now && !settled; ++i) {
            ++passes;
            settled = seen[i] == 0;
        }
    }

    if (!(snap_flags & XRS_ASTAR_NO_WALK)) {
        if (connectivity == 8) hipLaunchKernelGGL((astar_walk_kernel<true>), dim3(1), dim3(64), 0, s, w.field, (long)rows, (long)cols, w.st, out_dev);
        else hipLaunchKernelGGL((astar_walk_kernel<false>), dim3(1), dim3(64), 0, s, w.field, (long)rows, (long)cols, w.st, out_dev);
        XRS_LAUNCH_CHECK();
    }
    long long host_st[ST_WORDS];
    XRS_HIP(hipMemcpyAsync(host_st, w.st, sizeof host_st, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 7; ++i) status_host[i] = host_st[i];
    status_host[7] = passes;
    if (host_st[ST_ERROR]) return fail("xrs_astar: the walk found no neighbour one step nearer the goal (field not settled)");
    return 0;
}

int xrs_astar_tile_visits(const void *work_dev, int64_t rows, int64_t cols, int64_t *visits_host, void *stream) {
    if (!work_dev || !visits_host) return fail("xrs_astar_tile_visits: null pointer");
    if (xrs_astar_workspace_bytes(rows, cols) == 0) return fail("xrs_astar_tile_visits: not the shape of a workspace");
    const Work w = carve(const_cast<void *>(work_dev), (size_t)rows, (size_t)cols);
    long long v = 0;
    XRS_HIP(hipMemcpyAsync(&v, w.st + ST_VISITS, 8, hipMemcpyDeviceToHost, as_stream(stream)));
    XRS_HIP(hipStreamSynchronize(as_stream(stream)));
    *visits_host = v;
    return 0;
}

}  // extern "C"

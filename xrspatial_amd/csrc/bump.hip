// bump (xrspatial/bump.py:12-28 `_finish_bump`): the reference's serial, order-dependent bump loop, bit for bit.  DESIGN.md §6k.
//
// Bump i adds its height to its centre cell and then adds  out[centre] * (d2 / spread^2)  to every cell of its clipped footprint,
// the centre included (weight 0).  What it spreads depends on all that earlier bumps left on its centre, and every cell's float64
// sum is taken in bump order.  The device keeps both:
//
//   events   one 64-bit key  cell << jbits | j  for every cell of every bump's footprint (j: the bump's number in its chunk);
//            a count kernel and an exclusive scan place them, one radix sort over the bits in use orders each cell's events by
//            bump, and the segment heads hand every touched cell to one thread;
//   fold     that thread walks its cell's events in order, accumulator in a register.  The centre's event adds z_j, PUBLISHES
//            v_j (value, then the number of the pass as the flag) and adds v_j * 0.0; any other event needs v_j, and is ready
//            only when v_j was published in an EARLIER pass.  A thread whose next event is not ready stores its cursor, leaves
//            its accumulator in out[cell] and returns: no kernel ever waits on another thread.  The host repeats the pass until
//            the device counter of retired events reaches the total; the pending event with the smallest (bump, centre first)
//            is always ready, so every pass retires at least one -- a pass that retires none is reported as an error.
//
// Because only values of earlier passes are read, the stores are ordered by the kernel boundary alone, and the number of passes
// is a property of the input -- the depth of its dependency chains, the same on every run and in the NumPy model of the tests.
//
// The reference reads out[centre] afresh for every cell of the footprint, in column-major order (nx outer, ny inner), and the
// centre's own `+ v * 0.0` happens in the middle of that walk: cells after the centre see v + v * 0.0, which is v for every
// finite v and NaN for an infinite one.  The reader applies that itself.
//
// No FMA contraction anywhere in this file: the product and the add round separately.
#pragma clang fp contract(off)

#include "xrs_common.h"
#include "workspace.h"

#include <chrono>
#include <hipcub/hipcub.hpp>

namespace {

using xrs::as_stream;
using xrs::Carver;
using xrs::fail;
using u32 = uint32_t;
using u64 = unsigned long long;

constexpr int BLOCK = 256;
constexpr u32 DONE = 0xffffffffu;
constexpr long MAX_CELLS = 1L << 31;            // the cell number takes at most 31 bits of a key
constexpr long MAX_EVENTS = (1L << 31) - 1;     // event positions are uint32, hipCUB's counts are int
constexpr long MAX_SPREAD = 1L << 26;           // spread^2 and d2 stay exact in float64
constexpr long EXACT_FOOTPRINT = 4096;          // above: the bounding box stands for the disc

struct Ctrl {                                   // device words the host reads back
    u32 bad_loc;                                // a location outside the raster was met
    u32 nseg;                                   // touched cells of the chunk
    u64 retired;                                // events folded so far
};

struct Geom {
    long width, height, spread, s;
    int jbits;                                  // bits of a key below the cell number
    int spread_on;                              // spread >= 1: centres publish and add v * 0.0
};

__host__ __device__ inline long isqrt_floor(long r) {
    long m = (long)sqrt((double)r);
    while (m * m > r) --m;
    while ((m + 1) * (m + 1) <= r) ++m;
    return m;
}

int bits_for(long n) {                          // bits that hold 0 .. n - 1, at least 1
    int b = 1;
    while ((1L << b) < n) ++b;
    return b;
}

// most events one bump can have: the disc without its two far points, or its clipped bounding box
long footprint_bound(long width, long height, long spread) {
    if (spread <= 0) return 1;
    const long bw = 2 * spread < width ? 2 * spread : width, bh = 2 * spread < height ? 2 * spread : height;
    const long box = bw * bh;
    if (spread > EXACT_FOOTPRINT) return box;
    const long s = spread * spread;
    long n = 0;
    for (long dx = -spread; dx < spread; ++dx) {
        const long m = isqrt_floor(s - dx * dx);
        n += m + 1 + (m < spread - 1 ? m : spread - 1);       // dy = -m .. min(m, spread - 1)
    }
    return n < box ? n : box;
}

// f(nx, lo, hi): the rows lo .. hi (inclusive) of column nx that belong to the footprint of a bump at (x, y), in the reference's order
template <typename F>
__device__ __forceinline__ void for_columns(long x, long y, const Geom &g, F f) {
    if (!g.spread_on) {
        f(x, y, y);
        return;
    }
    const long x0 = x - g.spread > 0 ? x - g.spread : 0, x1 = x + g.spread < g.width ? x + g.spread : g.width;
    const long y0 = y - g.spread > 0 ? y - g.spread : 0, y1 = y + g.spread < g.height ? y + g.spread : g.height;
    for (long nx = x0; nx < x1; ++nx) {
        const long dx = nx - x;
        const long m = isqrt_floor(g.s - dx * dx);
        const long lo = y - m > y0 ? y - m : y0, hi = y + m < y1 - 1 ? y + m : y1 - 1;
        if (lo <= hi) f(nx, lo, hi);
    }
}

// cnt[t] = events of bump t of the chunk, cnt[nb] = 0 (the scan's last entry becomes the total).  A location outside the raster
// gets no events and raises bad_loc.
__global__ __launch_bounds__(BLOCK) void bump_count_kernel(const ushort2 *__restrict__ locs, u32 nb, Geom g, u32 *__restrict__ cnt,
                                                           Ctrl *__restrict__ ctrl) {
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t > nb) return;
    u32 n = 0;
    if (t < nb) {
        const ushort2 p = locs[t];
        if ((long)p.x >= g.width || (long)p.y >= g.height)
            atomicOr(&ctrl->bad_loc, 1u);
        else
            for_columns((long)p.x, (long)p.y, g, [&](long, long lo, long hi) { n += (u32)(hi - lo + 1); });
    }
    cnt[t] = n;
}

__global__ __launch_bounds__(BLOCK) void bump_emit_kernel(const ushort2 *__restrict__ locs, u32 nb, Geom g,
                                                          const u32 *__restrict__ offs, u64 *__restrict__ keys) {
    const u32 t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nb) return;
    const ushort2 p = locs[t];
    if ((long)p.x >= g.width || (long)p.y >= g.height) return;
    u32 at = offs[t];
    const u32 end = offs[t + 1];
    for_columns((long)p.x, (long)p.y, g, [&](long nx, long lo, long hi) {
        for (long ny = lo; ny <= hi && at < end; ++ny) keys[at++] = ((u64)(ny * g.width + nx) << g.jbits) | t;
    });
}

// every first event of a cell takes a segment slot; a wave asks for its slots with one atomic
__global__ __launch_bounds__(BLOCK) void bump_heads_kernel(const u64 *__restrict__ keys, u32 total, int jbits, u32 *__restrict__ seg_cur,
                                                           Ctrl *__restrict__ ctrl) {
    const u32 e = blockIdx.x * BLOCK + threadIdx.x;
    const bool head = e < total && (e == 0 || (keys[e - 1] >> jbits) != (keys[e] >> jbits));
    const u64 m = __ballot(head);
    if (m == 0) return;                                     // (wave-uniform)
    const int lane = (int)__lane_id(), leader = __ffsll((long long)m) - 1;
    u32 base = 0;
    if (lane == leader) base = atomicAdd(&ctrl->nseg, (u32)__popcll(m));
    base = __shfl(base, leader);
    if (head) seg_cur[base + (u32)__popcll(m & ((1ull << lane) - 1))] = e;
}

// One pass of the fold: thread `slot` walks its cell's events from its cursor on, as far as they are ready.
__global__ __launch_bounds__(BLOCK) void bump_fold_kernel(const u64 *__restrict__ keys, u32 total, u32 *__restrict__ seg_cur, u32 nseg,
                                                          const ushort2 *__restrict__ locs, const double *__restrict__ z,
                                                          double *v, u32 *flag, double *__restrict__ out, Geom g, u32 pass,
                                                          Ctrl *__restrict__ ctrl) {
    __shared__ u32 block_retired;
    if (threadIdx.x == 0) block_retired = 0;
    __syncthreads();
    const u32 slot = blockIdx.x * BLOCK + threadIdx.x;
    u32 n = 0;
    u32 cur = slot < nseg ? seg_cur[slot] : DONE;
    if (cur != DONE) {
        const u64 jmask = (1ull << g.jbits) - 1;
        u64 key = keys[cur];
        const u64 cell = key >> g.jbits;
        const long cy = (long)cell / g.width, cx = (long)cell - cy * g.width;
        double acc = out[cell];
        bool done = false;
        for (;;) {
            const u32 j = (u32)(key & jmask);
            const ushort2 p = locs[j];
            const long dx = cx - (long)p.x, dy = cy - (long)p.y;
            if (dx == 0 && dy == 0) {
                acc = acc + z[j];
                if (g.spread_on) {
                    v[j] = acc;
                    __hip_atomic_store(&flag[j], pass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    acc = acc + acc * 0.0;                  // the centre's own footprint cell: weight 0 / s
                }
            } else {
                const u32 f = __hip_atomic_load(&flag[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (f == 0 || f >= pass) break;             // not published before this pass: come back in the next
                double vi = v[j];
                if (dx > 0 || (dx == 0 && dy > 0)) vi = vi + vi * 0.0;      // walked after the centre
                acc = acc + vi * ((double)(dx * dx + dy * dy) / (double)g.s);
            }
            ++n;
            ++cur;
            if (cur == total) { done = true; break; }
            key = keys[cur];
            if ((key >> g.jbits) != cell) { done = true; break; }
        }
        out[cell] = acc;
        seg_cur[slot] = done ? DONE : cur;
    }
    if (n) atomicAdd(&block_retired, n);
    __syncthreads();
    if (threadIdx.x == 0 && block_retired) atomicAdd(&ctrl->retired, (u64)block_retired);
}

struct Work {
    long cap;               // events a chunk may hold
    long chunk;             // bumps of a chunk
    long footprint;
    u64 *keys[2];
    u32 *seg_cur, *offs, *flag;
    double *v;
    Ctrl *ctrl;
    void *cub;
    size_t cub_bytes, bytes;
};

// nullptr, or why the arguments are refused
const char *carve(void *base, long count, long width, long height, long spread, long max_events, Work &p) {
    if (count < 0 || count > (1L << 32) - 2) return "a count of 0 .. 2^32 - 2 bumps is needed";
    if (width < 1 || height < 1) return "width and height of at least 1 are needed";
    if (width >= MAX_CELLS || height >= MAX_CELLS || width * height > MAX_CELLS) return "at most 2^31 cells";
    if (spread > MAX_SPREAD) return "a spread of at most 2^26";
    if (max_events < 1) return "an event capacity of at least 1 is needed";
    p.footprint = footprint_bound(width, height, spread);
    if (p.footprint > max_events) return "event capacity too small for one bump's footprint";
    const long n = count > 0 ? count : 1;
    long cap = max_events < MAX_EVENTS ? max_events : MAX_EVENTS;
    if (cap / p.footprint >= n) cap = n * p.footprint;
    p.cap = cap;
    p.chunk = cap / p.footprint;
    if (p.chunk > n) p.chunk = n;
    const long segs = cap < width * height ? cap : width * height;
    Carver c(base);
    p.keys[0] = c.take<u64>(cap);
    p.keys[1] = c.take<u64>(cap);
    p.seg_cur = c.take<u32>(segs);
    p.offs = c.take<u32>(p.chunk + 1);
    p.v = c.take<double>(p.chunk);
    p.flag = c.take<u32>(p.chunk);
    p.ctrl = c.take<Ctrl>(1);
    size_t a = 0, b = 0;
    hipcub::DoubleBuffer<u64> dk(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, dk, (int)cap);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (u32 *)nullptr, (u32 *)nullptr, (int)(p.chunk + 1));
    p.cub_bytes = a > b ? a : b;
    p.cub = c.take<char>(p.cub_bytes);
    p.bytes = c.at();
    return nullptr;
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

size_t xrs_bump_workspace_bytes(int64_t count, int64_t width, int64_t height, int64_t spread, int64_t max_events) {
    Work p = {};
    return carve(nullptr, count, width, height, spread, max_events, p) ? 0 : p.bytes;
}

int xrs_bump_f64(const uint16_t *locs_dev, const double *heights_dev, int64_t count, int64_t width, int64_t height, int64_t spread,
                 double *out_dev, void *work_dev, size_t work_bytes, int64_t max_events, int64_t *status, void *stream) {
    Work p = {};
    if (const char *why = carve(work_dev, count, width, height, spread, max_events, p)) {
        if (p.footprint > max_events && max_events >= 1 && width >= 1 && height >= 1)
            return fail("xrs_bump_f64: %s (%ld events, capacity %ld)", why, p.footprint, (long)max_events);
        return fail("xrs_bump_f64: %s (count %ld, %ld x %ld, spread %ld, capacity %ld)", why, (long)count, (long)width, (long)height,
                    (long)spread, (long)max_events);
    }
    if (!out_dev || !work_dev || (count > 0 && (!locs_dev || !heights_dev))) return fail("xrs_bump_f64: null pointer");
    if (work_bytes < p.bytes) return fail("xrs_bump_f64: workspace of %zu bytes, %zu needed", work_bytes, p.bytes);
    hipStream_t s = as_stream(stream);

    Geom g;
    g.width = width;
    g.height = height;
    g.spread = spread;
    g.s = spread * spread;
    g.spread_on = spread >= 1;
    g.jbits = bits_for(p.chunk);
    const int cbits = bits_for(width * height);
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // chunks, events, passes, touched cells (summed over chunks), ns: expand, sort, fold
    double t_expand = 0, t_sort = 0, t_fold = 0;

    XRS_HIP(hipMemsetAsync(out_dev, 0, (size_t)(width * height) * sizeof(double), s));
    for (long b0 = 0; b0 < count; b0 += p.chunk) {
        const u32 nb = (u32)(count - b0 < p.chunk ? count - b0 : p.chunk);
        const ushort2 *locs = reinterpret_cast<const ushort2 *>(locs_dev) + b0;
        const double *z = heights_dev + b0;
        const unsigned bump_blocks = (nb + 1 + BLOCK - 1) / BLOCK;
        auto t0 = std::chrono::steady_clock::now();
        XRS_HIP(hipMemsetAsync(p.ctrl, 0, sizeof(Ctrl), s));
        XRS_HIP(hipMemsetAsync(p.flag, 0, (size_t)nb * sizeof(u32), s));
        hipLaunchKernelGGL(bump_count_kernel, dim3(bump_blocks), dim3(BLOCK), 0, s, locs, nb, g, p.offs, p.ctrl);
        XRS_LAUNCH_CHECK();
        size_t cub_bytes = p.cub_bytes;
        XRS_HIP(hipcub::DeviceScan::ExclusiveSum(p.cub, cub_bytes, p.offs, p.offs, (int)(nb + 1), s));
        u32 total = 0;
        Ctrl seen;
        XRS_HIP(hipMemcpyAsync(&total, p.offs + nb, sizeof(u32), hipMemcpyDeviceToHost, s));
        XRS_HIP(hipMemcpyAsync(&seen, p.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        if (seen.bad_loc)
            return fail("xrs_bump_f64: a location lies outside the %ld x %ld raster (bumps %ld .. %ld)", (long)width, (long)height, b0,
                        b0 + nb - 1);
        if ((long)total > p.cap) return fail("xrs_bump_f64: %u events in a chunk planned for %ld", total, p.cap);
        if (total == 0) continue;                   // (cannot happen: every bump inside the raster has its centre's event)
        hipLaunchKernelGGL(bump_emit_kernel, dim3(bump_blocks), dim3(BLOCK), 0, s, locs, nb, g, p.offs, p.keys[0]);
        XRS_LAUNCH_CHECK();
        XRS_HIP(hipStreamSynchronize(s));
        t_expand += seconds_since(t0);

        t0 = std::chrono::steady_clock::now();
        hipcub::DoubleBuffer<u64> dk(p.keys[0], p.keys[1]);
        cub_bytes = p.cub_bytes;
        XRS_HIP(hipcub::DeviceRadixSort::SortKeys(p.cub, cub_bytes, dk, (int)total, 0, g.jbits + cbits, s));
        const u64 *sorted = dk.Current();
        hipLaunchKernelGGL(bump_heads_kernel, dim3((total + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, sorted, total, g.jbits, p.seg_cur, p.ctrl);
        XRS_LAUNCH_CHECK();
        XRS_HIP(hipMemcpyAsync(&seen, p.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        t_sort += seconds_since(t0);
        const u32 nseg = seen.nseg;
        if (nseg == 0 || nseg > total || (long)nseg > width * height)
            return fail("xrs_bump_f64: %u touched cells for %u events", nseg, total);

        t0 = std::chrono::steady_clock::now();
        u64 retired = 0;
        for (u32 pass = 1; retired < total; ++pass) {
            hipLaunchKernelGGL(bump_fold_kernel, dim3((nseg + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, sorted, total, p.seg_cur, nseg, locs,
                               z, p.v, p.flag, out_dev, g, pass, p.ctrl);
            XRS_LAUNCH_CHECK();
            XRS_HIP(hipMemcpyAsync(&seen, p.ctrl, sizeof(Ctrl), hipMemcpyDeviceToHost, s));
            XRS_HIP(hipStreamSynchronize(s));
            if (seen.retired <= retired || seen.retired > total)
                return fail("xrs_bump_f64: pass %u retired no event (%llu of %u done)", pass, seen.retired, total);
            retired = seen.retired;
            ++st[2];
        }
        t_fold += seconds_since(t0);
        ++st[0];
        st[1] += total;
        st[3] += nseg;
    }
    st[4] = (int64_t)(t_expand * 1e9);
    st[5] = (int64_t)(t_sort * 1e9);
    st[6] = (int64_t)(t_fold * 1e9);
    if (status)
        for (int i = 0; i < 8; ++i) status[i] = st[i];
    return 0;
}

}  // extern "C"

// regions: connected-region labelling (zonal.regions).  Reference: xrspatial/zonal.py:1406-1549 (`_area_connectivity`).
//
// The reference's two serial passes have a closed form that this file computes in parallel:
//   M(c)   the entries of c's clamped 4- / 8-window, in the reference's order, that match c:
//          abs_T(w - v) <= 1e-08 + 1e-05 * abs_T(v)  (difference and abs in T, threshold and comparison in float64);
//   new(c) no entry of M(c) has a smaller linear index;
//   links  the entries of M(c) with one another, and c with them when c is not new;
//   label  1 + (number of new cells before r), r = the smallest linear index of c's linked component.
//
// Three launches and a scan:
//   link_kernel   one 64 x 32 tile per workgroup, tile + one-cell halo in LDS; the predicate per cell, the new flags as
//                 one 64-bit ballot per tile row (64 consecutive linear indices), the links whose ends both lie in the
//                 tile by union-find in LDS (root = smallest index), parent[] = global index of each cell's tile root;
//   ExclusiveSum  of the per-word popcounts (hipCUB); its last element is the number of new cells, which the host
//                 checks against the output dtype before anything else is written;
//   merge_kernel  the tile-border cells again: every star of links with an end outside its tile, by union-find on
//                 parent[] with device-scope CAS (why no flag, fence or grid barrier is needed);
//   label_kernel  a new launch: root of every cell, label = prefix count up to the root, converted to T; NaN passes.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "union_find.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

using namespace xrs;

namespace {

constexpr int TW = 64, TH = 32, THREADS = 256, WAVES = THREADS / 64;
constexpr int HW = TW + 2, HH = TH + 2;                                   // the tile and its one-cell halo

template <typename T> __device__ __forceinline__ bool is_nan(T) { return false; }
template <> __device__ __forceinline__ bool is_nan<float>(float v) { return __builtin_isnan(v); }
template <> __device__ __forceinline__ bool is_nan<double>(double v) { return __builtin_isnan(v); }

// abs_T(x) as float64, with the reference's Numba typing: integers in their own width, so abs(int_min) == int_min
template <typename T> __device__ __forceinline__ double abs_t(T x) {
    if constexpr (!std::is_integral<T>::value) {
        return (double)__builtin_fabs(x);
    } else if constexpr (std::is_unsigned<T>::value) {
        return (double)x;
    } else {
        using U = typename std::make_unsigned<T>::type;
        return (double)(x < 0 ? (T)(U)(U(0) - (U)x) : x);                 // two's-complement negation, wraps at T_min
    }
}
// w - v in T: integers wrap as NumPy's do
template <typename T> __device__ __forceinline__ T sub_t(T w, T v) {
    if constexpr (!std::is_integral<T>::value) {
        return w - v;
    } else {
        using U = typename std::make_unsigned<T>::type;
        return (T)(U)((U)w - (U)v);
    }
}

// (threshold(): atol + rtol * abs(v) as a multiply, then an add -- union_find.h)
template <typename T> __device__ __forceinline__ bool match(T w, T v, double thr) { return abs_t(sub_t(w, v)) <= thr; }

// The window of cell (y, x): the reference's clamped neighbours, in its order (self and duplicates included)
template <bool N8>
__device__ __forceinline__ int window(uint32_t y, uint32_t x, uint32_t rows, uint32_t cols, uint32_t *wy, uint32_t *wx) {
    const uint32_t ym = y > 0 ? y - 1 : 0, yp = y + 1 < rows ? y + 1 : y;
    const uint32_t xm = x > 0 ? x - 1 : 0, xp = x + 1 < cols ? x + 1 : x;
    if (N8) {
        const uint32_t ys[8] = {ym, y, yp, ym, yp, ym, y, yp}, xs[8] = {xm, xm, xm, x, x, xp, xp, xp};
#pragma unroll
        for (int k = 0; k < 8; ++k) wy[k] = ys[k], wx[k] = xs[k];
        return 8;
    }
    const uint32_t ys[4] = {y, ym, yp, y}, xs[4] = {xm, x, x, xp};
#pragma unroll
    for (int k = 0; k < 4; ++k) wy[k] = ys[k], wx[k] = xs[k];
    return 4;
}

// (union-find with root = smallest index, in LDS and on parent[] with device-scope CAS: union_find.h)

struct Grid {
    uint32_t rows, cols, tiles_x;
};

// ------------------------------------------------------------------ link: predicate, new flags, in-tile unions
template <typename T, bool N8>
__global__ void __launch_bounds__(THREADS) link_kernel(const T *__restrict__ in, Grid g, uint32_t *__restrict__ parent,
                                                       unsigned long long *__restrict__ mask, uint32_t *__restrict__ cnt) {
    __shared__ T val[HH * HW];
    __shared__ uint32_t par[TH * TW];
    const uint32_t tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
    const uint32_t x0 = tx * TW, y0 = ty * TH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int k = tid; k < HH * HW; k += THREADS) {
        const int hy = k / HW, hx = k - hy * HW;
        const long gy = (long)y0 + hy - 1, gx = (long)x0 + hx - 1;
        if (gy >= 0 && gy < g.rows && gx >= 0 && gx < g.cols) val[k] = in[(size_t)gy * g.cols + gx];
    }
    for (int k = tid; k < TH * TW; k += THREADS) par[k] = k;
    __syncthreads();

    for (int ly = wave; ly < TH; ly += WAVES) {
        const uint32_t y = y0 + ly, x = x0 + lane;
        bool fresh = false;
        if (y < g.rows && x < g.cols) {
            const T v = val[(ly + 1) * HW + lane + 1];
            if (!is_nan(v)) {
                const double thr = threshold(abs_t(v));
                uint32_t wy[8], wx[8];
                const int n = window<N8>(y, x, g.rows, g.cols, wy, wx);
                bool m[8];
                T w[8];
                bool before = false;
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    w[k] = val[(wy[k] - y0 + 1) * HW + (wx[k] - x0 + 1)];
                    m[k] = match(w[k], v, thr);
                    before |= m[k] && (wy[k] < y || (wy[k] == y && wx[k] < x));
                }
                fresh = !before;
                const uint32_t self = ly * TW + lane;
                uint32_t anchor = fresh ? ~0u : self;
#pragma unroll
                for (int k = 0; k < n; ++k) {
                    if (!m[k] || wy[k] < y0 || wy[k] >= y0 + TH || wx[k] < x0 || wx[k] >= x0 + TW) continue;
                    const uint32_t li = (wy[k] - y0) * TW + (wx[k] - x0);
                    // c -- d for a later neighbour d that matches c back: d is then not new, its star is anchored at d
                    // and holds c, so d makes this link itself (a clamped entry is c or a true neighbour, and the
                    // neighbourhood is symmetric, so c lies in d's window)
                    if (anchor == self && li > self && match(v, w[k], threshold(abs_t(w[k])))) continue;
                    if (anchor == ~0u) anchor = li;
                    else if (li != anchor) lds_union(par, anchor, li);
                }
            }
        }
        const unsigned long long b = __ballot(fresh);
        if (lane == 0 && y < g.rows) {
            const size_t w = (size_t)y * g.tiles_x + tx;
            mask[w] = b;
            cnt[w] = (uint32_t)__popcll(b);
        }
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
// One wave per tile side (top row, bottom row, left column, right column), a lane per border cell.  A link (a, e)
// is made as union(parent[a], parent[e]): both tile roots are in the sets of a and e, and sets never split, so any value
// of parent[] read here, stale or not, names the same sets.  A lane skips a root pair that it, or the lane before it for
// the same window entry, already covers: along a seam crossed by one region the 64 links of a side collapse to one.
template <typename T, bool N8>
__global__ void __launch_bounds__(THREADS) merge_kernel(const T *__restrict__ in, Grid g, uint32_t *parent) {
    const uint32_t tx = blockIdx.x % g.tiles_x, ty = blockIdx.x / g.tiles_x;
    const uint32_t x0 = tx * TW, y0 = ty * TH;
    const uint32_t th = min((uint32_t)TH, g.rows - y0), tw = min((uint32_t)TW, g.cols - x0);
    const uint32_t lane = threadIdx.x & 63, side = threadIdx.x >> 6;
    uint32_t ly, lx;
    bool on;
    if (side < 2) {
        ly = side == 0 ? 0 : th - 1;
        lx = lane;
        on = lx < tw && (side == 0 || th > 1);
    } else {
        lx = side == 2 ? 0 : tw - 1;
        ly = lane;
        on = ly < th && (side == 2 || tw > 1);
    }
    const uint32_t y = y0 + ly, x = x0 + lx, c = y * g.cols + x;
    constexpr int K = N8 ? 8 : 4;
    uint32_t wy[8], wx[8];
    bool m[8], out_of_tile[8];
    uint32_t anchor = ~0u;
#pragma unroll
    for (int j = 0; j < K; ++j) m[j] = out_of_tile[j] = false;
    if (on) {
        const T v = in[c];
        if (!is_nan(v)) {
            const double thr = threshold(abs_t(v));
            window<N8>(y, x, g.rows, g.cols, wy, wx);
            bool before = false;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                m[j] = match(in[wy[j] * g.cols + wx[j]], v, thr);
                out_of_tile[j] = wy[j] < y0 || wy[j] >= y0 + th || wx[j] < x0 || wx[j] >= x0 + tw;
                before |= m[j] && (wy[j] < y || (wy[j] == y && wx[j] < x));
            }
            // the star's anchor: c when it belongs to the star, else an in-tile member, else the first member
            if (before) anchor = c;
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (m[j] && !out_of_tile[j] && anchor == ~0u) anchor = wy[j] * g.cols + wx[j];
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (m[j] && anchor == ~0u) anchor = wy[j] * g.cols + wx[j];
        }
    }
    // in-tile members were joined to an in-tile anchor by link_kernel; what is left: every out-of-tile member
    // (and, with an out-of-tile anchor, no in-tile member exists)
    const uint32_t pa = anchor != ~0u ? parent[anchor] : ~0u;
    uint32_t seen[8];
    int n_seen = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool need = anchor != ~0u && m[j] && out_of_tile[j] && wy[j] * g.cols + wx[j] != anchor;
        const uint32_t pe = need ? parent[wy[j] * g.cols + wx[j]] : ~0u;
        const uint32_t prev_pa = __shfl_up(pa, 1), prev_pe = __shfl_up(pe, 1);
        const bool prev_need = __shfl_up((int)need, 1) != 0;
        if (!need) continue;
        if (lane > 0 && prev_need && prev_pa == pa && prev_pe == pe) continue;   // the lane before covers this pair
        bool dup = pe == pa;
        for (int q = 0; q < n_seen; ++q) dup |= seen[q] == pe;
        if (dup) continue;
        seen[n_seen++] = pe;
        g_union(parent, pa, pe);
    }
}

// ------------------------------------------------------------------ label: prefix count of new cells up to the root
template <typename T>
__global__ void __launch_bounds__(THREADS) label_kernel(const T *__restrict__ in, T *__restrict__ out, Grid g, uint32_t n,
                                                        uint32_t *parent, const unsigned long long *__restrict__ mask,
                                                        const uint32_t *__restrict__ pre) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const T v = in[i];
    if (is_nan(v)) {
        out[i] = v;
        return;
    }
    // find with halving by plain stores: no union runs in this launch, so every value stored is an ancestor of x
    uint32_t x = i, p = parent[i];
    while (p != x) {
        const uint32_t gp = parent[p];
        if (gp != p) parent[x] = gp;
        x = gp;
        p = parent[x];
    }
    const uint32_t ry = x / g.cols, rx = x - ry * g.cols;
    const size_t w = (size_t)ry * g.tiles_x + (rx >> 6);
    const uint32_t label = pre[w] + (uint32_t)__popcll(mask[w] & (~0ull >> (63 - (rx & 63))));
    out[i] = (T)label;
}

// ------------------------------------------------------------------ workspace
struct Work {
    uint32_t *parent, *cnt;         // cnt[words] is the total; after the scan cnt holds the prefix sums
    unsigned long long *mask;
    void *cub;
    size_t words, cub_bytes, total;
};
Work carve(void *base, uint64_t rows, uint64_t cols) {
    Carver c(base);
    Work w{};
    const uint64_t tiles_x = (cols + TW - 1) / TW;
    w.words = rows * tiles_x;
    w.parent = c.take<uint32_t>(rows * cols);
    w.mask = c.take<unsigned long long>(w.words);
    w.cnt = c.take<uint32_t>(w.words + 1);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, w.cub_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                           (size_t)(w.words + 1));
    w.cub = c.take<char>(w.cub_bytes > 0 ? w.cub_bytes : 1);
    w.total = c.at();
    return w;
}

int check_args(const char *fn, const void *data_dev, int dtype, int64_t rows, int64_t cols, int neighborhood,
               const void *work_dev) {
    if (rows < 0 || cols < 0) return fail("%s: negative shape", fn);
    if ((uint64_t)rows * (uint64_t)cols > 0xFFFFFFFFull || (cols > 0 && (uint64_t)rows > 0xFFFFFFFFull / (uint64_t)cols))
        return fail("%s: %lld x %lld cells exceed the 32-bit cell index (at most 2^32 - 1 cells)", fn, (long long)rows,
                    (long long)cols);
    if (neighborhood != 4 && neighborhood != 8) return fail("%s: neighborhood must be 4 or 8, got %d", fn, neighborhood);
    if (!dtype_bytes(dtype)) return fail("%s: unsupported dtype code %d", fn, dtype);
    if (rows * cols > 0 && (!data_dev || !work_dev)) return fail("%s: null pointer", fn);
    return 0;
}

template <typename T>
int link_impl(const T *in, int64_t rows, int64_t cols, int n8, void *work, uint64_t *n_new, hipStream_t s) {
    const Work w = carve(work, rows, cols);
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)((cols + TW - 1) / TW)};
    const size_t tiles = (size_t)g.tiles_x * ((rows + TH - 1) / TH);
    XRS_HIP(hipMemsetAsync(w.cnt + w.words, 0, 4, s));
    if (n8)
        hipLaunchKernelGGL((link_kernel<T, true>), dim3((unsigned)tiles), dim3(THREADS), 0, s, in, g, w.parent, w.mask, w.cnt);
    else
        hipLaunchKernelGGL((link_kernel<T, false>), dim3((unsigned)tiles), dim3(THREADS), 0, s, in, g, w.parent, w.mask, w.cnt);
    XRS_LAUNCH_CHECK();
    size_t cub_bytes = w.cub_bytes;
    XRS_HIP(hipcub::DeviceScan::ExclusiveSum(w.cub, cub_bytes, w.cnt, w.cnt, (size_t)(w.words + 1), s));
    uint32_t total = 0;
    XRS_HIP(hipMemcpyAsync(&total, w.cnt + w.words, 4, hipMemcpyDeviceToHost, s));
    XRS_HIP(hipStreamSynchronize(s));
    *n_new = total;
    return 0;
}

template <typename T>
int label_impl(const T *in, T *out, int64_t rows, int64_t cols, int n8, void *work, hipStream_t s) {
    const Work w = carve(work, rows, cols);
    const Grid g{(uint32_t)rows, (uint32_t)cols, (uint32_t)((cols + TW - 1) / TW)};
    const size_t tiles = (size_t)g.tiles_x * ((rows + TH - 1) / TH);
    if (n8)
        hipLaunchKernelGGL((merge_kernel<T, true>), dim3((unsigned)tiles), dim3(THREADS), 0, s, in, g, w.parent);
    else
        hipLaunchKernelGGL((merge_kernel<T, false>), dim3((unsigned)tiles), dim3(THREADS), 0, s, in, g, w.parent);
    XRS_LAUNCH_CHECK();
    const uint64_t n = (uint64_t)rows * cols;
    hipLaunchKernelGGL(label_kernel<T>, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, in, out, g,
                       (uint32_t)n, w.parent, (const unsigned long long *)w.mask, w.cnt);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t xrs_regions_workspace_bytes(int64_t rows, int64_t cols) {
    if (rows < 0 || cols < 0) return 0;
    return carve(nullptr, (uint64_t)rows, (uint64_t)cols).total;
}

int xrs_regions_link(const void *data_dev, int dtype, int64_t rows, int64_t cols, int neighborhood, void *work_dev,
                     uint64_t *n_new, void *stream) {
    if (int rc = check_args("xrs_regions_link", data_dev, dtype, rows, cols, neighborhood, work_dev)) return rc;
    if (!n_new) return fail("xrs_regions_link: null pointer");
    *n_new = 0;
    if (rows * cols == 0) return 0;
    hipStream_t s = as_stream(stream);
    const int n8 = neighborhood == 8;
    int rc = 0;
    with_dtype(dtype, [&](auto t) {                               // check_args refused every other code
        using T = dtype_of<decltype(t)>;
        rc = link_impl<T>((const T *)data_dev, rows, cols, n8, work_dev, n_new, s);
    });
    return rc;
}

int xrs_regions_label(const void *data_dev, int dtype, int64_t rows, int64_t cols, int neighborhood, void *work_dev,
                      void *out_dev, void *stream) {
    if (int rc = check_args("xrs_regions_label", data_dev, dtype, rows, cols, neighborhood, work_dev)) return rc;
    if (rows * cols == 0) return 0;
    if (!out_dev) return fail("xrs_regions_label: null pointer");
    hipStream_t s = as_stream(stream);
    const int n8 = neighborhood == 8;
    int rc = 0;
    with_dtype(dtype, [&](auto t) {                               // check_args refused every other code
        using T = dtype_of<decltype(t)>;
        rc = label_impl<T>((const T *)data_dev, (T *)out_dev, rows, cols, n8, work_dev, s);
    });
    return rc;
}

}  // extern "C"

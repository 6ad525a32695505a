// Shared helpers for libxrs_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/xrs_hip.h"

namespace xrs {

// Per-thread last-error text: the only mutable state in the library.
inline char *err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

inline int fail(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return 1;
}

// Route witness (xrs_debug_window_route): which launch groups served the thread's last focal / convolve_2d window call, in
// launch order, and the tiling the strip walkers chose.  A plain per-thread record: cleared at the top of the three ABI
// entries, written by the host launch functions once their kernels are enqueued.  Host code only.
struct RouteItem {
    const char *name;             // static text: a walker entry's name, or a branch tag of kxk.hip
    int R, RI;                    // radius and inner radius; -1 = none
    int wave_cols, wg_cols;       // columns of a wave tile and of a workgroup; 0 = the launch reports no geometry
    int tile_rows;
    long wgs_x, wgs_y;            // workgroups across and down
};
struct Route {
    int n;
    RouteItem item[8];
};
inline Route &route() {
    static thread_local Route r = {};
    return r;
}
inline void route_clear() { route().n = 0; }
inline void route_note(const char *name, int R = -1, int RI = -1, int wave_cols = 0, int wg_cols = 0, int tile_rows = 0,
                       long wgs_x = 0, long wgs_y = 0) {
    Route &r = route();
    if (r.n >= 8) return;
    if (!strncmp(name, "try_launch_", 11)) name += 11;
    r.item[r.n++] = RouteItem{name, R, RI, wave_cols, wg_cols, tile_rows, wgs_x, wgs_y};
}
#define XRS_STR_(x) #x
#define XRS_STR(x) XRS_STR_(x)

#define XRS_HIP(call)                                                                  \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess)                                                          \
            return ::xrs::fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),  \
                               __FILE__, __LINE__);                                    \
    } while (0)

#define XRS_LAUNCH_CHECK()                                                             \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess)                                                          \
            return ::xrs::fail("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                               __FILE__, __LINE__);                                    \
    } while (0)

// Run-time options of the library (xrs_set_option / xrs_get_option, include/xrs_hip.h): process-wide, relaxed atomics.
int option_value(int key);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// blockIdx -> tile index.  Workgroups are dealt round-robin to the 8 XCDs (block b -> XCD b % 8, observed, used for
// speed only).  Tiles are numbered row-major and handed out in groups of `unit` consecutive tiles -- one tile ROW for
// the 2-D kernels (unit = tiles_x): XCD k takes tile rows k, k + 8, ...  All eight XCDs then walk through the same
// few rows of the raster at the same time (one dense stream through DRAM), and the halo COLUMNS a tile re-reads were
// fetched into its own L2 by its left / right neighbours; the halo ROWS between tile rows are fetched by two L2s
// (2 rows in 16 for the 3x3 strip kernels: +6 % traffic at the L2 <-> fabric counters).  Round 1 gave every XCD one
// contiguous band of the raster instead (all halos in one L2, traffic == algorithmic bytes) -- eight streams 1/8 of the
// raster apart, and 4-7 % slower on every strip kernel (experiments/strip_floor.hip: 0.352 vs 0.328 ms for the loading
// pattern of the 3x3 kernels; groups of 2 / 4 / 8+ tile rows: 0.332 / 0.340 / 0.35).  unit = 1: launch order.
// Returns -1 for the surplus blocks of the padded grid.
// unit = 0: the round-1 order, one contiguous band of tiles per XCD -- kept for the column walkers (circle_walk.h,
// wide_impl.h: tall tiles, 100+ rows each; same-box A/B 3-6 % faster in bands) and, unmeasured, the
// LDS-tile kernels.
__device__ __forceinline__ long xcd_tile(long block, long n_tiles, long unit) {
    if (unit == 0) {
        const long per_xcd = (n_tiles + 7) >> 3;
        const long t = (block & 7) * per_xcd + (block >> 3);
        return ((block >> 3) < per_xcd && t < n_tiles) ? t : -1;
    }
    const unsigned xcd = (unsigned)block & 7u, j = (unsigned)(block >> 3), u = (unsigned)unit;
    const unsigned grp = j / u, within = j - grp * u;
    const long t = ((long)grp * 8 + xcd) * unit + within;
    return t < n_tiles ? t : -1;
}
inline long xcd_grid(long n_tiles, long unit) {
    if (unit == 0) return ((n_tiles + 7) >> 3) << 3;
    const long groups = (n_tiles + unit - 1) / unit;
    return (((groups + 7) >> 3) << 3) * unit;
}
// which order a kernel family uses (compile-time, the same expression on the host and in the kernel)
#ifndef XRS_XCD_WALK
#define XRS_XCD_WALK 0          // column walkers: bands
#endif
#ifndef XRS_XCD_LDS
#define XRS_XCD_LDS 0           // LDS-tile window kernels, run kernels, geodesic: bands (as measured in round 1)
#endif
#define XCD_UNIT(rows, tiles_x) ((rows) ? (long)(tiles_x) : 0L)

__device__ __forceinline__ float nan_f32() { return __int_as_float(0x7fc00000); }

// max(a, |b|, |c|) in one v_max3_f32 (no canonicalising moves; a NaN operand is skipped, which is what the guard below
// wants: NaN cells are caught through the sums they poison)
__device__ __forceinline__ float amax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}


// 16-byte global accesses at DWORD alignment (global_load/store_dwordx4 only need 4-byte alignment on gfx9+): rasters
// whose width or pitch is not a multiple of 4 cells -- an SRTM tile is 3601 wide -- keep the one-instruction-per-lane
// row accesses of the strip kernels instead of dropping to one-cell-per-thread kernels.
struct __attribute__((packed, aligned(4))) xrs_f4u { float x, y, z, w; };
struct __attribute__((packed, aligned(8))) xrs_d2u { double x, y; };
__device__ __forceinline__ xrs_f4u load_f4u(const float *p) { return *reinterpret_cast<const xrs_f4u *>(p); }

// Streaming ("nt") cache policy for planes that are read or written exactly once per launch (copy, per-cell indices,
// zonal reductions).  On a 1 GiB + 1 GiB copy on this chip nt loads + nt stores measured 6 290 GB/s against 5 870 with
// the default policy (experiments/copy_sweep.hip); ndvi / evi / savi gain 4-5 %.  NOT for the stencil kernels' input:
// their halo rows and columns are re-read by neighbouring strips out of L2, and streaming loads cost them 4-35 %
// (profiles/r01/nt_ab_r01.log).
typedef float xrs_v4f __attribute__((ext_vector_type(4)));
typedef float xrs_v4fu __attribute__((ext_vector_type(4), aligned(4)));
typedef int xrs_v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ldg_stream(const float4 *p) {
    const xrs_v4f v = __builtin_nontemporal_load(reinterpret_cast<const xrs_v4f *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ int4 ldg_stream(const int4 *p) {
    const xrs_v4i v = __builtin_nontemporal_load(reinterpret_cast<const xrs_v4i *>(p));
    return make_int4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void stg_stream(float4 *p, const float4 v) {
    xrs_v4f q; q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w;
    __builtin_nontemporal_store(q, reinterpret_cast<xrs_v4f *>(p));
}
__device__ __forceinline__ xrs_f4u load_f4u_stream(const float *p) {       // dword-aligned 16 bytes
    const xrs_v4fu v = __builtin_nontemporal_load(reinterpret_cast<const xrs_v4fu *>(p));
    xrs_f4u r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
    return r;
}
// Results are written once and not read again by the launch that produces them: streaming ("nt") stores.  Same-box A/B
// (profiles/r01/ntst_ab_r01.log): hillshade 0.386 -> 0.366 ms, slope 0.422 -> 0.400, curvature 0.388 -> 0.361,
// 5x5 convolve 0.556 -> 0.438, four terrain products 1.147 -> 1.070.
typedef double xrs_v2du_st __attribute__((ext_vector_type(2), aligned(8)));
template <typename T>
__device__ __forceinline__ void st_stream(T *p, const T v) {          // one scalar result per lane
    __builtin_nontemporal_store(v, p);
}
__device__ __forceinline__ void store_d2u(double *p, double x, double y) {    // two doubles at 8-byte alignment
    xrs_v2du_st q; q.x = x; q.y = y;
    __builtin_nontemporal_store(q, reinterpret_cast<xrs_v2du_st *>(p));
}
// A wave's 256 adjacent float64 results (4 per lane, lane l owns columns 4l .. 4l+3) as TWO store instructions that
// each write 1 KiB of consecutive bytes: lane pairs are transposed through ds_bpermute first.  Every lane storing its own
// 32 bytes as two 16-byte halves makes each store instruction touch 64 x 16 B at a 32-byte stride -- two instructions
// writing alternate halves of the same 2 KiB -- and costs a third of the bandwidth (experiments/f64_store.hip: 0.856 ->
// 0.584 ms for a float32 -> float64 plane).  `row` = address of the wave's first result; ALL 64 lanes must be active
// (wave-uniform control flow).
__device__ __forceinline__ void store_wave_row_d4(double *row, int lane, double x, double y, double z, double w) {
    const bool odd = lane & 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        // store k writes doubles [128 k + 2 lane, + 2): columns (2 lane, 2 lane + 1) of half k, owned by lane 32 k + lane / 2
        const int src = 32 * k + (lane >> 1);
        const double a0 = __shfl(x, src), a1 = __shfl(y, src), a2 = __shfl(z, src), a3 = __shfl(w, src);
        store_d2u(row + 128 * k + 2 * lane, odd ? a2 : a0, odd ? a3 : a1);
    }
}
// the same for float32 results that leave as float64 (converted after the exchange: half the shuffles)
__device__ __forceinline__ void store_wave_row_f4_as_d(double *row, int lane, float x, float y, float z, float w) {
    const bool odd = lane & 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int src = 32 * k + (lane >> 1);
        const float a0 = __shfl(x, src), a1 = __shfl(y, src), a2 = __shfl(z, src), a3 = __shfl(w, src);
        store_d2u(row + 128 * k + 2 * lane, (double)(odd ? a2 : a0), (double)(odd ? a3 : a1));
    }
}
typedef float xrs_v4fu_st __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ void store_f4u(float *p, float x, float y, float z, float w) {
    xrs_v4fu_st q; q.x = x; q.y = y; q.z = z; q.w = w;
    __builtin_nontemporal_store(q, reinterpret_cast<xrs_v4fu_st *>(p));
}

// runtime.hip: compute units of the current device (256 if the runtime will not say); asked once per thread
int device_cu_count();

// (the window walkers' entry points: window_call.h)
// kxk_big.hip: focal statistics / convolve_2d for windows beyond the tiled kernels' 63 x 63 (one thread per cell, window from
// global memory, mask / weights from a device copy of the kernel in `work_dev`)
int launch_window_any_size(bool conv, const float *in, float *const *outs, long rows, long cols, long ld_in, long ld_out,
                           const double *kernel, int krows, int kcols, void *work_dev, int halo_top, int halo_bot,
                           hipStream_t s);
// pass.hip: is this mask one of the compile-time masks of raster_pass_kernel (circle_kernel(1, 1, 2), np.ones((3, 3)))?
bool pass_has_compile_time_mask(const double *kernel, int krows, int kcols);
// boxsep.hip: the separable fast walk for np.ones((krows, kcols)) -- mean / var / std / sum sets WITH var or std (for the
// mean or the sum alone it measured no faster than the wide row walker: 0.53 vs 0.55 ms at 25x25, 0.68 vs 0.47 at 11x11) --
// in front of a fall-back kernel whose workgroup tiles (fb_group_cols x fb_tile_rows cells, fb_groups_x per tile row) it
// marks in `todo` where it cannot stand for its results.  0 = launched, -1 = not for this walk (the caller runs its kernel
// everywhere), > 0 = error.  `todo`: WorkspaceLayout::todo_off (window_call.h).
int launch_box_sep(const float *in, float *out_sum, float *out_mean, float *out_var, float *out_std,
                   long rows, long cols, long ld_in, long ld_out, int krows, int kcols, int halo_top, int halo_bot,
                   unsigned char *todo, long fb_groups_x, int fb_tile_rows, int fb_group_cols, hipStream_t s);

}  // namespace xrs

// perlin / generate_terrain: every octave of lattice noise in one launch, each cell written once, and the finishing pass.
//
// Reference: xrspatial/perlin.py `_perlin` (:51-74) under `_perlin_numpy` (:77-91), and xrspatial/terrain.py `_gen_terrain`
// (:36-61) under `_terrain_numpy` (:64-80) -- the NumPy path, whose typing this file follows:
//   coordinates   np.linspace(a, b, n, endpoint=False, dtype=float32)[j] = float32(float64(j) * ((b - a) / n) + a), the
//                 multiply and the add rounded separately; terrain octave i scales them by 2^i in float32 (exact);
//   _perlin       xi = trunc(x) (>= 0 here), xf = x - xi in float64, and fade, gradient and the three lerps in float64;
//   perlin        the float64 noise stored in the output dtype;
//   terrain       h = T(float64(h) + noise_i * 2^-i) for i = 0 .. n - 1 in that order, h = h / T(1.97), h = h * h * h.
// Contraction is off for the whole file: NumPy rounds every multiply and add on its own.
//
// The reference's GPU path is 16 launches that each read, modify and write the whole plane, then seven more full-plane
// passes; here a thread owns one column of a 256 x 64 tile and walks down its rows with the column's part of every octave
// in registers (xf, fade(xf), p[xi], p[xi + 1]); the rows' part (yi, yf, fade(yf)) is computed once per tile into LDS and
// read back as broadcasts.  The table of an octave is the 2^20-entry permutation; the reference doubles it so that
// p[xi] + yi + 1 needs no wrap, here the index is masked instead (p2[k] == p[k - 2^20]), which also keeps every table read
// inside the table whatever the arguments are.  A wave stores 64 adjacent cells per row.  The plane's min and max
// leave through wave reductions, one LDS round per block and one pair of float64 atomics per block.
#include "wave_reduce.h"
#include "xrs_common.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr int MAX_OCT = 16, TABLE_BITS = 20, TABLE_MASK = (1 << TABLE_BITS) - 1;
constexpr int TILE_COLS = 256, TILE_ROWS = 64;
constexpr int MODE_PERLIN = 0, MODE_TERRAIN = 1;

struct Tables {
    const int32_t *p[MAX_OCT];
};

__device__ __forceinline__ double fade(double t) {          // 6 t^5 - 15 t^4 + 10 t^3
    const double t3 = t * t * t, t4 = t3 * t, t5 = t4 * t;
    return 6.0 * t5 - 15.0 * t4 + 10.0 * t3;
}

// vectors[h % 4] . (x, y) with vectors (0, 1), (0, -1), (1, 0), (-1, 0).  0.0 - s: a zero keeps the sign the reference's
// 0 * x + (-1) * y gives wherever it reaches the result.
__device__ __forceinline__ double gradient(int h, double x, double y) {
    const double s = (h & 2) ? x : y;
    return (h & 1) ? 0.0 - s : s;
}

__device__ __forceinline__ double lerp(double a, double b, double t) { return a + t * (b - a); }

// a / b correctly rounded in T (float through float64: innocuous double rounding for a quotient)
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ double div_rn(double a, double b) { return a / b; }
// h ** 3 (float: the float64 product of three floats, rounded once more)
__device__ __forceinline__ float cube(float h) { const double d = (double)h; return (float)(d * d * d); }
__device__ __forceinline__ double cube(double h) { return h * h * h; }

// np.linspace(start, start + n * step, n, endpoint=False, dtype=float32)[j]
__device__ __forceinline__ float lin_f32(long j, double step, double start) { return (float)((double)j * step + start); }

template <typename T, int MODE, int NOCT>
__global__ void __launch_bounds__(TILE_COLS) noise_raw_kernel(T *__restrict__ out, long rows, long cols, long row0, long tiles_x,
                                                             double xstart, double xstep, double ystart, double ystep, Tables tab,
                                                             int n_oct, double divisor, double *__restrict__ minmax) {
    __shared__ double s_yf[NOCT][TILE_ROWS], s_v[NOCT][TILE_ROWS];
    __shared__ int s_yi[NOCT][TILE_ROWS];
    __shared__ double s_mn[TILE_COLS / 64], s_mx[TILE_COLS / 64];
    const long tile_y = (long)blockIdx.x / tiles_x, tile_x = (long)blockIdx.x - tile_y * tiles_x;
    const long r0 = tile_y * TILE_ROWS;
    const int nr = (int)(rows - r0 < TILE_ROWS ? rows - r0 : TILE_ROWS);

    // the rows' part of every octave
    for (int e = threadIdx.x; e < NOCT * TILE_ROWS; e += TILE_COLS) {
        const int o = e / TILE_ROWS, r = e - o * TILE_ROWS;
        const float y = lin_f32(row0 + r0 + r, ystep, ystart) * (float)(1 << o);
        const int yi = (int)y;
        const double yf = (double)y - (double)yi;
        s_yi[o][r] = yi;
        s_yf[o][r] = yf;
        s_v[o][r] = fade(yf);
    }

    // this thread's column (the surplus threads of the last tile redo the last column and store nothing)
    const long col_raw = tile_x * TILE_COLS + threadIdx.x;
    const bool live = col_raw < cols;
    const long col = live ? col_raw : cols - 1;
    const float x = lin_f32(col, xstep, xstart);
    double xf[NOCT], u[NOCT];
    int a0[NOCT], a1[NOCT];
#pragma unroll
    for (int o = 0; o < NOCT; ++o) {
        xf[o] = u[o] = 0.0;
        a0[o] = a1[o] = 0;
        if (o < n_oct) {
            const float xo = x * (float)(1 << o);
            const int xi = (int)xo;
            xf[o] = (double)xo - (double)xi;
            u[o] = fade(xf[o]);
            a0[o] = tab.p[o][xi & TABLE_MASK];
            a1[o] = tab.p[o][(xi + 1) & TABLE_MASK];
        }
    }
    __syncthreads();

    const T div_t = (T)divisor;
    T mn = (T)__builtin_inf(), mx = -(T)__builtin_inf();
    T *dst = out + r0 * cols + col;
    for (int r = 0; r < nr; ++r, dst += cols) {
        T h = T(0);
#pragma unroll
        for (int o = 0; o < NOCT; ++o) {
            if (o < n_oct) {
                const int yi = s_yi[o][r];
                const double yf = s_yf[o][r], v = s_v[o][r];
                const int32_t *__restrict__ p = tab.p[o];
                const int h00 = p[(a0[o] + yi) & TABLE_MASK], h01 = p[(a0[o] + yi + 1) & TABLE_MASK];
                const int h11 = p[(a1[o] + yi + 1) & TABLE_MASK], h10 = p[(a1[o] + yi) & TABLE_MASK];
                const double xm = xf[o] - 1.0, ym = yf - 1.0;
                const double n00 = gradient(h00, xf[o], yf), n01 = gradient(h01, xf[o], ym);
                const double n11 = gradient(h11, xm, ym), n10 = gradient(h10, xm, yf);
                const double a = lerp(lerp(n00, n10, u[o]), lerp(n01, n11, u[o]), v);
                if (MODE == MODE_PERLIN) h = (T)a;
                else h = (T)((double)h + a * (1.0 / (double)(1 << o)));
            }
        }
        if (MODE == MODE_TERRAIN) h = cube(div_rn(h, div_t));
        if (live) {
            st_stream(dst, h);
            mn = h < mn ? h : mn;
            mx = h > mx ? h : mx;
        }
    }

    // every lane is here: wave -> block -> one pair of atomics
    const double wmn = wave_reduce<WrMin>((double)mn), wmx = wave_reduce<WrMax>((double)mx);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mn[wave] = wmn; s_mx[wave] = wmx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bmn = s_mn[0], bmx = s_mx[0];
        for (int w = 1; w < TILE_COLS / 64; ++w) { bmn = fmin(bmn, s_mn[w]); bmx = fmax(bmx, s_mx[w]); }
        atomicMin(minmax, bmn);
        atomicMax(minmax + 1, bmx);
    }
}

// (v - min) / (max - min) in T, then the optional water line and the optional scale
constexpr int FIN_PER = 4;
template <typename T>
__global__ void __launch_bounds__(256) noise_finish_kernel(T *__restrict__ data, long n, T mn, T ptp, int has_thr, T thr, int has_scale,
                                                          T scale) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * FIN_PER;
#pragma unroll
    for (int j = 0; j < FIN_PER; ++j) {
        const long i = i0 + j;
        if (i >= n) return;
        T v = div_rn((T)(data[i] - mn), ptp);
        if (has_thr && v < thr) v = T(0);
        if (has_scale) v = v * scale;
        data[i] = v;
    }
}

// largest and smallest float32 coordinate of linspace(a, b, n, endpoint=False): its two ends (it is monotone)
inline void lin_ends(double a, double b, long n, double *lo, double *hi) {
    const double step = (b - a) / (double)n;
    const float first = (float)a, last = (float)((double)(n - 1) * step + a);
    *lo = first < last ? first : last;
    *hi = first < last ? last : first;
}

template <typename T>
int raw_impl(T *out, long rows, long cols, long row0, long total_rows, double x0, double x1, double y0, double y1,
             const int32_t *const *tables, int n_oct, int mode, double *minmax, hipStream_t s) {
    if (rows < 0 || cols < 0 || row0 < 0 || total_rows < 0) return fail("xrs_noise_raw: negative size");
    if (row0 + rows > total_rows) return fail("xrs_noise_raw: rows [%ld, %ld) outside a raster of %ld rows", row0, row0 + rows, total_rows);
    if (mode != MODE_PERLIN && mode != MODE_TERRAIN) return fail("xrs_noise_raw: unknown mode %d", mode);
    if (n_oct < 1 || n_oct > MAX_OCT || (mode == MODE_PERLIN && n_oct != 1))
        return fail("xrs_noise_raw: %d octaves (perlin: 1, terrain: 1 .. %d)", n_oct, MAX_OCT);
    if (!minmax || !tables) return fail("xrs_noise_raw: null pointer");
    Tables tab{};
    for (int o = 0; o < n_oct; ++o) {
        if (!tables[o]) return fail("xrs_noise_raw: null table %d", o);
        tab.p[o] = tables[o];
    }
    for (int o = n_oct; o < MAX_OCT; ++o) tab.p[o] = tables[0];
    const double init[2] = {__builtin_inf(), -__builtin_inf()};
    if (rows == 0 || cols == 0) {
        XRS_HIP(hipMemcpyAsync(minmax, init, sizeof init, hipMemcpyHostToDevice, s));
        return 0;
    }
    if (!out) return fail("xrs_noise_raw: null pointer");
    if (!(std::isfinite(x0) && std::isfinite(x1) && std::isfinite(y0) && std::isfinite(y1)))
        return fail("xrs_noise_raw: non-finite coordinate range");
    // every lattice index in [0, 2^20 - 1)
    double xlo, xhi, ylo, yhi;
    lin_ends(x0, x1, cols, &xlo, &xhi);
    lin_ends(y0, y1, total_rows, &ylo, &yhi);
    const double top = (double)(1 << (n_oct - 1));
    if (xlo < 0.0 || ylo < 0.0 || !(xhi * top < (double)TABLE_MASK) || !(yhi * top < (double)TABLE_MASK))
        return fail("xrs_noise_raw: lattice coordinates [%g, %g] x [%g, %g] (octave %d) leave [0, 2^20 - 1)", xlo * top, xhi * top,
                    ylo * top, yhi * top, n_oct - 1);
    const long tiles_x = (cols + TILE_COLS - 1) / TILE_COLS, tiles_y = (rows + TILE_ROWS - 1) / TILE_ROWS;
    if (tiles_x * tiles_y >= (1L << 31)) return fail("xrs_noise_raw: plane too large for one call (%ld x %ld)", rows, cols);
    XRS_HIP(hipMemcpyAsync(minmax, init, sizeof init, hipMemcpyHostToDevice, s));
    const double xstep = (x1 - x0) / (double)cols, ystep = (y1 - y0) / (double)total_rows;
    const double divisor = 1.00 + 0.50 + 0.25 + 0.13 + 0.06 + 0.03;         // terrain.py:59, summed in its order
    const dim3 grid((unsigned)(tiles_x * tiles_y)), block(TILE_COLS);
    if (mode == MODE_PERLIN)
        hipLaunchKernelGGL((noise_raw_kernel<T, MODE_PERLIN, 1>), grid, block, 0, s, out, rows, cols, row0, tiles_x, x0, xstep, y0,
                           ystep, tab, n_oct, divisor, minmax);
    else
        hipLaunchKernelGGL((noise_raw_kernel<T, MODE_TERRAIN, MAX_OCT>), grid, block, 0, s, out, rows, cols, row0, tiles_x, x0, xstep,
                           y0, ystep, tab, n_oct, divisor, minmax);
    XRS_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int finish_impl(T *data, long n, double mn, double mx, int has_thr, double thr, int has_scale, double scale, hipStream_t s) {
    if (n < 0) return fail("xrs_noise_finish: negative size");
    if (n == 0) return 0;
    if (!data) return fail("xrs_noise_finish: null pointer");
    const T ptp = (T)((T)mx - (T)mn);
    hipLaunchKernelGGL((noise_finish_kernel<T>), dim3((unsigned)((n + 256L * FIN_PER - 1) / (256L * FIN_PER))), dim3(256), 0, s, data, n,
                       (T)mn, ptp, has_thr, (T)thr, has_scale, (T)scale);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

#define XRS_NOISE(SUF, T)                                                                                                      \
    int xrs_noise_raw_##SUF(T *out_dev, int64_t rows, int64_t cols, int64_t row0, int64_t total_rows, double x0, double x1,   \
                            double y0, double y1, const int32_t *const *tables, int n_octaves, int mode, double *minmax_dev,  \
                            void *stream) {                                                                                    \
        return raw_impl<T>(out_dev, rows, cols, row0, total_rows, x0, x1, y0, y1, tables, n_octaves, mode, minmax_dev,        \
                           as_stream(stream));                                                                                 \
    }                                                                                                                          \
    int xrs_noise_finish_##SUF(T *data_dev, int64_t n, double min, double max, int has_threshold, double threshold,           \
                               int has_scale, double scale, void *stream) {                                                    \
        return finish_impl<T>(data_dev, n, min, max, has_threshold, threshold, has_scale, scale, as_stream(stream));          \
    }
XRS_NOISE(f32, float)
XRS_NOISE(f64, double)

}  // extern "C"

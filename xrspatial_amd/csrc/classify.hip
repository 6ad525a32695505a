// classify: reclassify / binary (per-cell) and the device statistics behind the data-driven classifiers.
//
// Reference: xrspatial/classify.py, CPU path.  _cpu_binary (:31-41) -> binary_kernel; _cpu_bin (:153-187) -> bin_kernel;
// the host formulas of equal_interval / quantile / percentiles / box_plot / std_mean / head_tail_breaks /
// maximum_breaks take their inputs from the reductions, the radix select and the maximum-breaks pipeline below.
//
// bin_kernel: `mode` picks one of three searches that give the SAME bin for the bins they are used with:
//   LITERAL  the reference loop, line for line (floor division, bins[mid - 1] with mid == 0 reading bins[n - 1],
//            the value of `mid` after a loop that ends without `break`): any bins, NaN-carrying and unsorted included;
//   COUNT    bins non-decreasing and NaN-free: bin = #{b : bins[b] < v} (searchsorted-left), a branch-free count over
//            wave-uniform bins (scalar loads); the argument that the reference loop computes this is in DESIGN.md §classify;
//   SEARCH   the same bins, many of them: lower_bound by bisection.
// Every comparison is in float64, as Numba compares a float32 / integer cell with float64 bins.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

using namespace xrs;

namespace {

constexpr int BIN_LITERAL = 0, BIN_COUNT = 1, BIN_SEARCH = 2;

template <typename T> __device__ __forceinline__ bool finite_of(T v) { return true; }
template <> __device__ __forceinline__ bool finite_of<float>(float v) { return isfinite(v); }
template <> __device__ __forceinline__ bool finite_of<double>(double v) { return isfinite(v); }

template <int MODE>
__device__ __forceinline__ int find_bin(double v, bool fin, const double *__restrict__ bins, int nb) {
    if (!fin) return -1;
    if (MODE == BIN_COUNT) {
        if (!(v <= bins[nb - 1])) return -1;
        int c = 0;
        for (int b = 0; b < nb; ++b) c += bins[b] < v ? 1 : 0;      // uniform address: scalar loads
        return c;
    } else if (MODE == BIN_SEARCH) {
        if (!(v <= bins[nb - 1])) return -1;
        int lo = 0, hi = nb - 1;                                      // first b with v <= bins[b]; exists
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (bins[mid] < v) lo = mid + 1; else hi = mid;
        }
        return lo;
    } else {
        if (v <= bins[0]) return 0;
        if (!(v <= bins[nb - 1])) return -1;
        int start = 0, end = nb - 1;
        int mid = (end + start) >> 1;                                 // arithmetic shift = Python's floor division
        while (start <= end) {
            if (bins[mid] < v) {
                start = mid + 1;
            } else if (v > bins[mid == 0 ? nb - 1 : mid - 1]) {       // Numba wraps index -1 to the last bin
                break;
            } else {
                end = mid - 1;
            }
            mid = (end + start) >> 1;
        }
        return mid;                                                   // -1 possible: (0 + -1) // 2
    }
}

constexpr int PER = 4;          // cells per thread

template <typename T, int MODE>
__global__ void __launch_bounds__(256) bin_kernel(const T *__restrict__ in, float *__restrict__ out, long n,
                                                  const double *__restrict__ bins, const double *__restrict__ nv, int nb) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * PER;
    if (i0 >= n) return;
    T v[PER];
    const bool whole = i0 + PER <= n;
    if (whole) {
#pragma unroll
        for (int j = 0; j < PER; ++j) v[j] = __builtin_nontemporal_load(in + i0 + j);
    } else {
        for (int j = 0; j < PER; ++j) v[j] = i0 + j < n ? in[i0 + j] : T(0);
    }
    float r[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int b = find_bin<MODE>((double)v[j], finite_of(v[j]), bins, nb);
        r[j] = b > -1 ? (float)nv[b] : __builtin_nanf("");
    }
    if (whole) {
#pragma unroll
        for (int j = 0; j < PER; ++j) __builtin_nontemporal_store(r[j], out + i0 + j);
    } else {
        for (int j = 0; j < PER && i0 + j < n; ++j) out[i0 + j] = r[j];
    }
}

// _cpu_binary: 1 where the cell equals one of `values` (compared in float64), else 0 for a finite cell, NaN otherwise
template <typename T>
__global__ void __launch_bounds__(256) binary_kernel(const T *__restrict__ in, T *__restrict__ out, long n,
                                                     const double *__restrict__ vals, int nv) {
    const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * PER;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const long i = i0 + j;
        if (i >= n) return;
        const T x = in[i];
        const double d = (double)x;
        bool hit = false;
        for (int k = 0; k < nv; ++k) hit |= d == vals[k];
        if constexpr (sizeof(T) >= 4 && T(0.5) != T(0))
            out[i] = hit ? T(1) : (isfinite(x) ? T(0) : T(__builtin_nan("")));
        else
            out[i] = hit ? T(1) : T(0);                               // an integer cell is always finite
    }
}

template <typename S>
__global__ void to_f64_kernel(const S *__restrict__ in, double *__restrict__ out, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

// ------------------------------------------------------------------ reductions over the finite cells
constexpr int RED_BLOCKS = 1024, RED_THREADS = 256;

struct Part {            // one block's partial: count, min, max, sum (or sum of squared deviations)
    double cnt, mn, mx, s;
};

__device__ __forceinline__ Part combine(Part a, Part b) {
    return Part{a.cnt + b.cnt, fmin(a.mn, b.mn), fmax(a.mx, b.mx), a.s + b.s};
}

__device__ Part block_reduce(Part p) {
    __shared__ Part sh[RED_THREADS];
    sh[threadIdx.x] = p;
    __syncthreads();
    for (int off = RED_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] = combine(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
    return sh[0];
}

// OP 0: count / min / max / sum of finite cells; 1: sum of (x - c)^2 over finite cells; 2: count / sum of finite x > c
template <typename T, int OP>
__global__ void __launch_bounds__(RED_THREADS) reduce_kernel(const T *__restrict__ in, long n, double c, Part *parts) {
    Part p{0.0, __builtin_inf(), -__builtin_inf(), 0.0};
    for (long i = (long)blockIdx.x * RED_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * RED_THREADS) {
        const T x = in[i];
        if (!isfinite(x)) continue;
        const double d = (double)x;
        if (OP == 0) { p.cnt += 1.0; p.mn = fmin(p.mn, d); p.mx = fmax(p.mx, d); p.s += d; }
        if (OP == 1) { const double e = d - c; p.cnt += 1.0; p.s += e * e; }
        if (OP == 2 && d > c) { p.cnt += 1.0; p.s += d; }
    }
    p = block_reduce(p);
    if (threadIdx.x == 0) parts[blockIdx.x] = p;
}

__global__ void __launch_bounds__(RED_THREADS) reduce_final_kernel(const Part *parts, int np, double *out) {
    Part p{0.0, __builtin_inf(), -__builtin_inf(), 0.0};
    for (int i = threadIdx.x; i < np; i += RED_THREADS) p = combine(p, parts[i]);
    p = block_reduce(p);
    if (threadIdx.x == 0) {
        const bool none = p.cnt == 0.0;
        out[0] = p.cnt;
        out[1] = none ? __builtin_nan("") : p.mn;
        out[2] = none ? __builtin_nan("") : p.mx;
        out[3] = p.s;
    }
}

// ------------------------------------------------------------------ order-preserving keys
template <typename T> struct Key;
template <> struct Key<float> {
    using K = unsigned;
    static constexpr int BITS = 32;
    static __device__ __forceinline__ K enc(float v) {
        const unsigned b = __float_as_uint(v);
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    static __device__ __forceinline__ float dec(K k) {
        return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
    }
};
template <> struct Key<double> {
    using K = unsigned long long;
    static constexpr int BITS = 64;
    static __device__ __forceinline__ K enc(double v) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double dec(K k) {
        return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
    }
};

// ------------------------------------------------------------------ exact order statistics: MSB-first radix select
// Every rank walks down the key from the top digit.  Ranks are sorted, so after each digit the ranks' prefixes are
// non-decreasing and the distinct ones are disjoint: a cell matches at most one of them.  One pass per digit:
//   hist     every block counts the digits of its cells that match a distinct prefix, in LDS (8 prefixes per sweep),
//            and adds the non-zero bins to the global histogram;
//   scan     one block per rank: prefix sum over that rank's histogram row, the digit whose bucket holds the rank,
//            the rank within that bucket;
//   dedupe   one thread: the distinct prefixes of the next digit.
constexpr int MAX_RANKS = 64, DIGIT_BITS = 11, NBUCKET = 1 << DIGIT_BITS, GROUP = 8;
constexpr int SEL_THREADS = 512, SEL_MAX_BLOCKS = 1024;

struct SelState {
    unsigned long long prefix[MAX_RANKS];     // key bits decided so far (right-aligned)
    unsigned long long resid[MAX_RANKS];      // rank within the cells carrying that prefix
    unsigned long long dprefix[MAX_RANKS];    // distinct prefixes, ascending
    int dp[MAX_RANKS];                         // rank -> its distinct prefix
    int n_dp;
};

template <int KB> __host__ __device__ constexpr int n_digits() { return (KB + DIGIT_BITS - 1) / DIGIT_BITS; }
// digit d covers key bits [lo, lo + width): widths 11, 11, 10 (32-bit keys) / 11 x 4, 10, 10 (64-bit keys)
template <int KB> __host__ __device__ inline int digit_width(int d) {
    const int nd = n_digits<KB>(), extra = nd * DIGIT_BITS - KB;       // the last `extra` digits are 1 bit narrower
    return d >= nd - extra ? DIGIT_BITS - 1 : DIGIT_BITS;
}
template <int KB> __host__ __device__ inline int digit_lo(int d) {
    int hi = KB;
    for (int j = 0; j <= d; ++j) hi -= digit_width<KB>(j);
    return hi;
}

__global__ void sel_init_kernel(SelState *st, const long long *ranks, int nr) {
    const int r = threadIdx.x;
    if (r < nr) {
        st->prefix[r] = 0;
        st->resid[r] = (unsigned long long)ranks[r];
        st->dp[r] = 0;
    }
    if (r == 0) { st->dprefix[0] = 0; st->n_dp = 1; }
}

template <typename T>
__global__ void __launch_bounds__(SEL_THREADS) sel_hist_kernel(const T *__restrict__ in, long n, const SelState *st, int d,
                                                               unsigned *__restrict__ hist) {
    using KK = Key<T>;
    constexpr int KB = KK::BITS;
    __shared__ unsigned lh[GROUP * NBUCKET];
    const int lo = digit_lo<KB>(d), w = digit_width<KB>(d), hi = lo + w;
    const unsigned mask = (1u << w) - 1u;
    const int ndp = st->n_dp;
    const long per = (n + gridDim.x - 1) / gridDim.x;
    const long a = (long)blockIdx.x * per, b = a + per < n ? a + per : n;
    for (int g0 = 0; g0 < ndp; g0 += GROUP) {
        const int ng = ndp - g0 < GROUP ? ndp - g0 : GROUP;
        unsigned long long pre[GROUP];
#pragma unroll
        for (int j = 0; j < GROUP; ++j) pre[j] = j < ng ? st->dprefix[g0 + j] : ~0ull;
        for (int i = threadIdx.x; i < ng * NBUCKET; i += SEL_THREADS) lh[i] = 0;
        __syncthreads();
        for (long i = a + threadIdx.x; i < b; i += SEL_THREADS) {
            const T x = in[i];
            if (!isfinite(x)) continue;
            const unsigned long long k = (unsigned long long)KK::enc(x);
            const unsigned long long top = hi >= 64 ? 0ull : (k >> hi);
            int slot = -1;
#pragma unroll
            for (int j = 0; j < GROUP; ++j) slot = (j < ng && top == pre[j]) ? j : slot;
            if (slot >= 0) atomicAdd(&lh[slot * NBUCKET + (unsigned)((k >> lo) & mask)], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ng * NBUCKET; i += SEL_THREADS) {
            const unsigned c = lh[i];
            if (c) atomicAdd(&hist[(long)(g0 + i / NBUCKET) * NBUCKET + (i % NBUCKET)], c);
        }
        __syncthreads();
    }
}

template <int KB>
__global__ void __launch_bounds__(256) sel_scan_kernel(SelState *st, int d, const unsigned *__restrict__ hist) {
    const int r = blockIdx.x;
    const int w = digit_width<KB>(d);
    const int nbk = 1 << w, per = nbk / 256;          // 8 or 4 buckets per thread
    const unsigned *row = hist + (long)st->dp[r] * NBUCKET;
    const unsigned long long want = st->resid[r];
    unsigned long long mine = 0;
    for (int j = 0; j < per; ++j) mine += row[threadIdx.x * per + j];
    __shared__ unsigned long long sc[256];
    sc[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // inclusive Hillis-Steele scan
        const unsigned long long add = (int)threadIdx.x >= off ? sc[threadIdx.x - off] : 0ull;
        __syncthreads();
        sc[threadIdx.x] += add;
        __syncthreads();
    }
    const unsigned long long incl = sc[threadIdx.x], excl = incl - mine;
    if (want >= excl && want < incl) {
        unsigned long long run = excl;
        for (int j = 0; j < per; ++j) {
            const unsigned c = row[threadIdx.x * per + j];
            if (want < run + c) {
                st->prefix[r] = (st->prefix[r] << w) | (unsigned long long)(threadIdx.x * per + j);
                st->resid[r] = want - run;
                break;
            }
            run += c;
        }
    }
}

__global__ void sel_dedupe_kernel(SelState *st, int nr) {
    if (threadIdx.x != 0) return;
    int nd = 0;
    for (int r = 0; r < nr; ++r) {
        if (nd == 0 || st->prefix[r] != st->dprefix[nd - 1]) st->dprefix[nd++] = st->prefix[r];
        st->dp[r] = nd - 1;
    }
    st->n_dp = nd;
}

template <typename T>
__global__ void sel_decode_kernel(const SelState *st, int nr, double *out) {
    const int r = threadIdx.x;
    if (r < nr) out[r] = (double)Key<T>::dec((typename Key<T>::K)st->prefix[r]);
}

struct SelWork {
    SelState *st;
    unsigned *hist;
    size_t hist_bytes, total;
};
inline SelWork carve_select(void *base) {
    Carver c(base);
    SelWork w = {};
    w.st = c.take<SelState>(1);
    w.hist_bytes = (size_t)MAX_RANKS * NBUCKET * 4;
    w.hist = c.take_bytes<unsigned>(w.hist_bytes);
    w.total = c.at();
    return w;
}
inline unsigned sel_blocks(long n) {
    const long b = (n + SEL_THREADS * 16L - 1) / (SEL_THREADS * 16L);
    return (unsigned)(b < 1 ? 1 : (b > SEL_MAX_BLOCKS ? SEL_MAX_BLOCKS : b));
}

template <typename T>
int select_impl(const T *in, long n, const long long *ranks, int nr, void *work, size_t work_bytes, double *out,
                hipStream_t s) {
    constexpr int KB = Key<T>::BITS;
    if (n < 0 || nr < 0) return fail("xrs_classify_select: negative size");
    if (nr == 0) return 0;
    if (nr > MAX_RANKS) return fail("xrs_classify_select: at most %d ranks per call (%d)", MAX_RANKS, nr);
    if (n >= (1L << 32)) return fail("xrs_classify_select: at most 2^32-1 cells per call");
    if (!in || !ranks || !work || !out) return fail("xrs_classify_select: null pointer");
    const SelWork w = carve_select(work);
    if (work_bytes < w.total) return fail("xrs_classify_select: workspace too small (%zu)", work_bytes);
    hipLaunchKernelGGL(sel_init_kernel, dim3(1), dim3(MAX_RANKS), 0, s, w.st, ranks, nr);
    XRS_LAUNCH_CHECK();
    for (int d = 0; d < n_digits<KB>(); ++d) {
        XRS_HIP(hipMemsetAsync(w.hist, 0, w.hist_bytes, s));
        hipLaunchKernelGGL((sel_hist_kernel<T>), dim3(sel_blocks(n)), dim3(SEL_THREADS), 0, s, in, n, w.st, d, w.hist);
        XRS_LAUNCH_CHECK();
        hipLaunchKernelGGL((sel_scan_kernel<KB>), dim3(nr), dim3(256), 0, s, w.st, d, w.hist);
        XRS_LAUNCH_CHECK();
        hipLaunchKernelGGL(sel_dedupe_kernel, dim3(1), dim3(64), 0, s, w.st, nr);
        XRS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((sel_decode_kernel<T>), dim3(1), dim3(MAX_RANKS), 0, s, w.st, nr, out);
    XRS_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ maximum_breaks
// finite cells -> keys (-0.0 folded into +0.0: np.unique keeps one zero) -> vendor radix sort -> run heads -> the
// unique values uv[0..M) -> gaps uv[i+1] - uv[i] in the input dtype -> the top n_top gaps by (gap, index), one
// device-wide arg-max per gap (the set np.argsort(diffs, kind='stable')[-n_top:] picks).
template <typename T>
__global__ void mb_keys_kernel(const T *__restrict__ in, long n, typename Key<T>::K *keys) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    T v = in[i];
    if (v == T(0)) v = T(0);
    keys[i] = isfinite(v) ? Key<T>::enc(v) : ~(typename Key<T>::K)0;
}

template <typename K>
__global__ void mb_heads_kernel(const K *keys, long n, unsigned char *flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = (keys[i] != ~(K)0 && (i == 0 || keys[i] != keys[i - 1])) ? 1 : 0;
}

struct Arg {             // (gap, index), ordered lexicographically; index -1 = none
    double g;
    long long i;
};
__device__ __forceinline__ bool arg_less(Arg a, Arg b) { return a.g < b.g || (a.g == b.g && a.i < b.i); }

constexpr int MB_BLOCKS = 512;

// arg-max of (gap, index) over the gaps below `bound` (the previous pick), per block
template <typename T>
__global__ void __launch_bounds__(256) mb_argmax_kernel(const typename Key<T>::K *uk, const unsigned *m_p, const Arg *bound,
                                                        Arg *parts) {
    const long m = (long)*m_p;
    const Arg bd = *bound;
    Arg best{-__builtin_inf(), -1};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i + 1 < m; i += (long)gridDim.x * 256) {
        const T g = Key<T>::dec(uk[i + 1]) - Key<T>::dec(uk[i]);        // np.diff in the input dtype
        const Arg a{(double)g, i};
        if ((bd.i < 0 || arg_less(a, bd)) && (best.i < 0 || arg_less(best, a))) best = a;
    }
    __shared__ Arg sh[256];
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const Arg o = sh[threadIdx.x + off];
            if (o.i >= 0 && (sh[threadIdx.x].i < 0 || arg_less(sh[threadIdx.x], o))) sh[threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) parts[blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(256) mb_pick_kernel(const Arg *parts, int np, Arg *bound, long long *picked) {
    __shared__ Arg sh[256];
    Arg best{-__builtin_inf(), -1};
    for (int i = threadIdx.x; i < np; i += 256) {
        const Arg o = parts[i];
        if (o.i >= 0 && (best.i < 0 || arg_less(best, o))) best = o;
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const Arg o = sh[threadIdx.x + off];
            if (o.i >= 0 && (sh[threadIdx.x].i < 0 || arg_less(sh[threadIdx.x], o))) sh[threadIdx.x] = o;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *picked = sh[0].i;
        if (sh[0].i >= 0) *bound = sh[0];
        else bound->i = -2;          // nothing left: later passes find nothing below (-2 never matches)
    }
}

// out: [M, (idx_j, uv[idx_j], uv[idx_j + 1]) for j < n_top, uv[M - 1], uv[0 .. n_top]] ; n_top < 0: [M, uv[0 .. M)]
template <typename T>
__global__ void mb_gather_kernel(const typename Key<T>::K *uk, const unsigned *m_p, const long long *picked, int n_top,
                                 double *out) {
    const long m = (long)*m_p;
    const double nan = __builtin_nan("");
    if (n_top < 0) {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < m; i += (long)gridDim.x * 256)
            out[1 + i] = (double)Key<T>::dec(uk[i]);
        if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (double)m;
        return;
    }
    if (blockIdx.x != 0) return;
    const int t = threadIdx.x;
    if (t == 0) {
        out[0] = (double)m;
        out[1 + 3 * n_top] = m > 0 ? (double)Key<T>::dec(uk[m - 1]) : nan;
    }
    for (int j = t; j < n_top; j += 256) {
        const long long i = picked[j];
        out[1 + 3 * j] = (double)i;
        out[2 + 3 * j] = i >= 0 ? (double)Key<T>::dec(uk[i]) : nan;
        out[3 + 3 * j] = i >= 0 ? (double)Key<T>::dec(uk[i + 1]) : nan;
    }
    for (int j = t; j <= n_top; j += 256) out[2 + 3 * n_top + j] = j < m ? (double)Key<T>::dec(uk[j]) : nan;
}

template <typename T>
struct MbWork {
    using K = typename Key<T>::K;
    K *k[2], *uk;
    unsigned char *flags;
    unsigned *m;
    Arg *parts, *bound;
    long long *picked;
    void *cub;
    size_t cub_bytes, total;
};
template <typename T>
MbWork<T> carve_max_breaks(void *base, long n, int n_top) {
    using K = typename Key<T>::K;
    Carver c(base);
    MbWork<T> w = {};
    for (int i = 0; i < 2; ++i) w.k[i] = c.take<K>(n);
    w.uk = c.take<K>(n);
    w.flags = c.take<unsigned char>(n);
    w.m = c.take_bytes<unsigned>(256);
    w.parts = c.take<Arg>(MB_BLOCKS);
    w.bound = c.take_bytes<Arg>(256);
    w.picked = c.take<long long>(n_top > 0 ? n_top : 1);
    size_t t1 = 0, t2 = 0;
    hipcub::DoubleBuffer<K> dk(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, t1, dk, (int)n);
    (void)hipcub::DeviceSelect::Flagged(nullptr, t2, (const K *)nullptr, (const unsigned char *)nullptr, (K *)nullptr,
                                        (unsigned *)nullptr, (int)n);
    w.cub_bytes = up256(t1 > t2 ? t1 : t2) + 256;
    w.cub = c.take_bytes(w.cub_bytes);
    w.total = c.at();
    return w;
}

template <typename T>
int max_breaks_impl(const T *in, long n, int n_top, void *work, size_t work_bytes, double *out, hipStream_t s) {
    using K = typename Key<T>::K;
    if (n <= 0) return fail("xrs_classify_max_breaks: no cells");
    if (n >= (1L << 31)) return fail("xrs_classify_max_breaks: at most 2^31-1 cells per call");
    if (!in || !work || !out) return fail("xrs_classify_max_breaks: null pointer");
    const MbWork<T> w = carve_max_breaks<T>(work, n, n_top);
    if (work_bytes < w.total) return fail("xrs_classify_max_breaks: workspace too small (%zu < %zu)", work_bytes, w.total);
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((mb_keys_kernel<T>), dim3(grid), dim3(256), 0, s, in, n, w.k[0]);
    XRS_LAUNCH_CHECK();
    hipcub::DoubleBuffer<K> dk(w.k[0], w.k[1]);
    size_t cb = w.cub_bytes;
    XRS_HIP(hipcub::DeviceRadixSort::SortKeys(w.cub, cb, dk, (int)n, 0, (int)sizeof(K) * 8, s));
    hipLaunchKernelGGL((mb_heads_kernel<K>), dim3(grid), dim3(256), 0, s, dk.Current(), n, w.flags);
    XRS_LAUNCH_CHECK();
    cb = w.cub_bytes;
    XRS_HIP(hipcub::DeviceSelect::Flagged(w.cub, cb, dk.Current(), w.flags, w.uk, w.m, (int)n, s));
    if (n_top < 0) {
        hipLaunchKernelGGL((mb_gather_kernel<T>), dim3(grid), dim3(256), 0, s, w.uk, w.m, w.picked, n_top, out);
        XRS_LAUNCH_CHECK();
        return 0;
    }
    const Arg none{0.0, -1};
    XRS_HIP(hipMemcpyAsync(w.bound, &none, sizeof(Arg), hipMemcpyHostToDevice, s));
    const unsigned mb = grid < (unsigned)MB_BLOCKS ? grid : (unsigned)MB_BLOCKS;
    for (int j = 0; j < n_top; ++j) {
        hipLaunchKernelGGL((mb_argmax_kernel<T>), dim3(mb), dim3(256), 0, s, w.uk, w.m, w.bound, w.parts);
        XRS_LAUNCH_CHECK();
        hipLaunchKernelGGL(mb_pick_kernel, dim3(1), dim3(256), 0, s, w.parts, (int)mb, w.bound, w.picked + j);
        XRS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((mb_gather_kernel<T>), dim3(1), dim3(256), 0, s, w.uk, w.m, w.picked, n_top, out);
    XRS_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------ launch helpers
template <typename T>
int bin_impl(const T *in, float *out, long n, const double *bins, const double *nv, int nb, int mode, hipStream_t s) {
    if (n < 0 || nb < 0) return fail("xrs_classify_bin: negative size");
    if (n == 0) return 0;
    if (!in || !out) return fail("xrs_classify_bin: null pointer");
    if (nb == 0) return fail("xrs_classify_bin: no bins");
    if (!bins || !nv) return fail("xrs_classify_bin: null bins");
    const unsigned grid = (unsigned)((n + 256L * PER - 1) / (256L * PER));
    if (mode == BIN_COUNT)
        hipLaunchKernelGGL((bin_kernel<T, BIN_COUNT>), dim3(grid), dim3(256), 0, s, in, out, n, bins, nv, nb);
    else if (mode == BIN_SEARCH)
        hipLaunchKernelGGL((bin_kernel<T, BIN_SEARCH>), dim3(grid), dim3(256), 0, s, in, out, n, bins, nv, nb);
    else if (mode == BIN_LITERAL)
        hipLaunchKernelGGL((bin_kernel<T, BIN_LITERAL>), dim3(grid), dim3(256), 0, s, in, out, n, bins, nv, nb);
    else
        return fail("xrs_classify_bin: unknown mode %d", mode);
    XRS_LAUNCH_CHECK();
    return 0;
}

template <typename T>
int binary_impl(const T *in, T *out, long n, const double *vals, int nv, hipStream_t s) {
    if (n < 0 || nv < 0) return fail("xrs_classify_binary: negative size");
    if (n == 0) return 0;
    if (!in || !out || (nv && !vals)) return fail("xrs_classify_binary: null pointer");
    hipLaunchKernelGGL((binary_kernel<T>), dim3((unsigned)((n + 256L * PER - 1) / (256L * PER))), dim3(256), 0, s, in, out, n,
                       vals, nv);
    XRS_LAUNCH_CHECK();
    return 0;
}

template <typename T, int OP>
int reduce_impl(const T *in, long n, double c, void *work, double *out, hipStream_t s) {
    if (n < 0) return fail("xrs_classify reduction: negative size");
    if (!work || !out || (n && !in)) return fail("xrs_classify reduction: null pointer");
    long b = (n + RED_THREADS * 8L - 1) / (RED_THREADS * 8L);
    const int grid = (int)(b < 1 ? 1 : (b > RED_BLOCKS ? RED_BLOCKS : b));
    Part *parts = static_cast<Part *>(work);
    hipLaunchKernelGGL((reduce_kernel<T, OP>), dim3(grid), dim3(RED_THREADS), 0, s, in, n, c, parts);
    XRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(RED_THREADS), 0, s, parts, grid, out);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t xrs_classify_workspace_bytes(int64_t n, int values_f64) {
    const long m = n > 0 ? n : 1;
    size_t a = carve_select(nullptr).total;
    const size_t r = up256(RED_BLOCKS * sizeof(Part));
    const size_t mb = values_f64 ? carve_max_breaks<double>(nullptr, m, MAX_RANKS).total
                                 : carve_max_breaks<float>(nullptr, m, MAX_RANKS).total;
    a = a > r ? a : r;
    return a > mb ? a : mb;
}

int xrs_classify_to_f64(const void *in_dev, int dtype_code, double *out_dev, int64_t n, void *stream) {
    if (n < 0) return fail("xrs_classify_to_f64: negative size");
    if (n == 0) return 0;
    if (!in_dev || !out_dev) return fail("xrs_classify_to_f64: null pointer");
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    hipStream_t s = as_stream(stream);
    const bool known = with_dtype<DT_NO_F64>(dtype_code, [&](auto t) {
        using T = dtype_of<decltype(t)>;
        hipLaunchKernelGGL(to_f64_kernel<T>, g, b, 0, s, (const T *)in_dev, out_dev, n);
    });
    if (!known) return fail("xrs_classify_to_f64: unsupported dtype code %d", dtype_code);
    XRS_LAUNCH_CHECK();
    return 0;
}

#define XRS_CLASSIFY_BIN(SUF, T)                                                                                         \
    int xrs_classify_bin_##SUF(const T *in_dev, float *out_dev, int64_t n, const double *bins_dev,                       \
                               const double *new_values_dev, int n_bins, int mode, void *stream) {                       \
        return bin_impl<T>(in_dev, out_dev, n, bins_dev, new_values_dev, n_bins, mode, as_stream(stream));               \
    }
XRS_CLASSIFY_BIN(f32, float)
XRS_CLASSIFY_BIN(f64, double)
XRS_CLASSIFY_BIN(i32, int32_t)
XRS_CLASSIFY_BIN(i64, int64_t)

#define XRS_CLASSIFY_BINARY(SUF, T)                                                                                      \
    int xrs_classify_binary_##SUF(const T *in_dev, T *out_dev, int64_t n, const double *values_dev, int n_values,        \
                                  void *stream) {                                                                        \
        return binary_impl<T>(in_dev, out_dev, n, values_dev, n_values, as_stream(stream));                              \
    }
XRS_CLASSIFY_BINARY(f32, float)
XRS_CLASSIFY_BINARY(f64, double)
XRS_CLASSIFY_BINARY(i8, int8_t)
XRS_CLASSIFY_BINARY(u8, uint8_t)
XRS_CLASSIFY_BINARY(i16, int16_t)
XRS_CLASSIFY_BINARY(u16, uint16_t)
XRS_CLASSIFY_BINARY(i32, int32_t)
XRS_CLASSIFY_BINARY(u32, uint32_t)
XRS_CLASSIFY_BINARY(i64, int64_t)
XRS_CLASSIFY_BINARY(u64, uint64_t)

#define XRS_CLASSIFY_FLOAT(SUF, T)                                                                                       \
    int xrs_classify_finite_stats_##SUF(const T *in_dev, int64_t n, void *work_dev, double *out4_dev, void *stream) {   \
        return reduce_impl<T, 0>(in_dev, n, 0.0, work_dev, out4_dev, as_stream(stream));                                \
    }                                                                                                                    \
    int xrs_classify_sqdev_##SUF(const T *in_dev, int64_t n, double center, void *work_dev, double *out4_dev,           \
                                 void *stream) {                                                                         \
        return reduce_impl<T, 1>(in_dev, n, center, work_dev, out4_dev, as_stream(stream));                             \
    }                                                                                                                    \
    int xrs_classify_above_##SUF(const T *in_dev, int64_t n, double threshold, void *work_dev, double *out4_dev,        \
                                 void *stream) {                                                                         \
        return reduce_impl<T, 2>(in_dev, n, threshold, work_dev, out4_dev, as_stream(stream));                          \
    }                                                                                                                    \
    int xrs_classify_select_##SUF(const T *in_dev, int64_t n, const int64_t *ranks_dev, int n_ranks, void *work_dev,    \
                                  size_t work_bytes, double *values_dev, void *stream) {                                 \
        return select_impl<T>(in_dev, n, (const long long *)ranks_dev, n_ranks, work_dev, work_bytes, values_dev,       \
                              as_stream(stream));                                                                        \
    }                                                                                                                    \
    int xrs_classify_max_breaks_##SUF(const T *in_dev, int64_t n, int n_top, void *work_dev, size_t work_bytes,         \
                                      double *out_dev, void *stream) {                                                   \
        return max_breaks_impl<T>(in_dev, n, n_top, work_dev, work_bytes, out_dev, as_stream(stream));                   \
    }
XRS_CLASSIFY_FLOAT(f32, float)
XRS_CLASSIFY_FLOAT(f64, double)

}  // extern "C"

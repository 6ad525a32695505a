// local: statistics, frequencies, positions, rank, popularity and combine across the variables of a Dataset, cell by cell.
//
// Reference: xrspatial/local.py, which builds a Python tuple per cell and calls NumPy on it.  The rule computed here is
// written out in xrspatial_amd/local.py and DESIGN.md §6f.  Every per-cell function reads N planes once, each in its own
// dtype, widens in registers to the working type (int64 when every plane is an integer and the function allows it, else
// float64) and writes one 8-byte plane.  The plane pointers and dtype codes travel in the kernel's argument block (64 x 8
// + 64 bytes): no upload, no device pointer table.
//
//   streaming  max, min, sum, mean, std, the three frequencies, the two positions: two cells per thread, no per-cell array;
//              sum / mean / std keep NumPy's eight pairwise accumulators; std reads the planes a second time (from L2).
//   values     median, rank, popularity: one cell per thread; N <= 4 / 8 / 16 in registers through a bitonic network with
//              compile-time indices (padded with the largest value, which sorts behind every cell value or equal to it),
//              17 <= N <= 64 by insertion into a column of LDS per thread (column-major: lane l of a wave reads word l).
//   combine    exact and without hashing: one plane at a time the cells are stably radix-sorted (rocPRIM via hipCUB) by the
//              plane's canonical value and then by the class they had so far; runs of (class, value) become the new dense
//              classes.  Equal tuples never change their relative order, so the first cell of a final run is the tuple's
//              first occurrence in row-major order; sorting the classes by that cell gives the reference's ids.
#include "xrs_common.h"
#include "dtype_dispatch.h"
#include "workspace.h"

#include <hipcub/hipcub.hpp>

#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

constexpr int MAXP = XRS_LOCAL_MAX_PLANES;

struct LocalArgs {
    const void *p[MAXP];
    unsigned char dt[MAXP];
};

typedef long long i64;
typedef unsigned long long u64;

struct __attribute__((packed, aligned(4))) f2u { float x, y; };
struct __attribute__((packed, aligned(4))) i2u { int x, y; };
struct __attribute__((packed, aligned(4))) u2u { unsigned x, y; };
struct __attribute__((packed, aligned(8))) l2u { i64 x, y; };

template <typename W> __device__ __forceinline__ bool is_nan(W v) {
    if constexpr (std::is_same<W, double>::value) return v != v;
    return false;
}
template <typename W> __device__ __forceinline__ W largest() {
    if constexpr (std::is_same<W, double>::value) return __longlong_as_double(0x7ff0000000000000ll);
    else return (W)0x7fffffffffffffffll;
}

// One cell of a plane, widened, is load_as<W, DT_NO_U64> (dtype_dispatch.h).
// cells i and i + 1 of a plane (i even): one 8- or 16-byte load for the 4- and 8-byte dtypes
template <typename W> __device__ __forceinline__ void ld2(const void *p, int dt, long i, bool two, W &a, W &b) {
    if (!two) { a = load_as<W, DT_NO_U64>(p, dt, i); b = a; return; }
    switch (dt) {
    case XRS_DT_F32: { const f2u v = *reinterpret_cast<const f2u *>(static_cast<const float *>(p) + i); a = (W)v.x; b = (W)v.y; return; }
    case XRS_DT_F64: { const xrs_d2u v = *reinterpret_cast<const xrs_d2u *>(static_cast<const double *>(p) + i); a = (W)v.x; b = (W)v.y; return; }
    case XRS_DT_I32: { const i2u v = *reinterpret_cast<const i2u *>(static_cast<const int32_t *>(p) + i); a = (W)v.x; b = (W)v.y; return; }
    case XRS_DT_U32: { const u2u v = *reinterpret_cast<const u2u *>(static_cast<const uint32_t *>(p) + i); a = (W)v.x; b = (W)v.y; return; }
    case XRS_DT_I64: { const l2u v = *reinterpret_cast<const l2u *>(static_cast<const int64_t *>(p) + i); a = (W)v.x; b = (W)v.y; return; }
    default: a = load_as<W, DT_NO_U64>(p, dt, i); b = load_as<W, DT_NO_U64>(p, dt, i + 1); return;
    }
}

__device__ __forceinline__ double nan_f64() { return __longlong_as_double(0x7ff8000000000000ll); }

// ------------------------------------------------------------------ streaming functions
// NumPy's pairwise block over the values get(j), j = 0 .. n - 1, of two cells at once (n <= 64 < its recursion threshold)
template <typename G> __device__ __forceinline__ void pairwise2(int n, G get, double &s0, double &s1) {
    if (n < 8) {
        double r0 = 0.0, r1 = 0.0;
        for (int j = 0; j < n; ++j) {
            double a, b;
            get(j, a, b);
            r0 += a;
            r1 += b;
        }
        s0 = r0;
        s1 = r1;
        return;
    }
    double a0[8], a1[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) get(k, a0[k], a1[k]);
    int j = 8;
    for (; j + 8 <= n; j += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            double a, b;
            get(j + k, a, b);
            a0[k] += a;
            a1[k] += b;
        }
    }
    double r0 = ((a0[0] + a0[1]) + (a0[2] + a0[3])) + ((a0[4] + a0[5]) + (a0[6] + a0[7]));
    double r1 = ((a1[0] + a1[1]) + (a1[2] + a1[3])) + ((a1[4] + a1[5]) + (a1[6] + a1[7]));
    for (; j < n; ++j) {
        double a, b;
        get(j, a, b);
        r0 += a;
        r1 += b;
    }
    s0 = r0;
    s1 = r1;
}

template <typename W> __device__ __forceinline__ double as_out(W r, int out_i64) {
    if constexpr (std::is_same<W, double>::value) return r;
    else return out_i64 ? __longlong_as_double(r) : (double)r;
}

template <int OP, typename W>
__global__ void __launch_bounds__(256) local_stream_kernel(const LocalArgs args, int np, const void *ref, int ref_dt, long n,
                                                          double *out, int out_i64) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i >= n) return;
    const bool two = i + 1 < n;
    double o0, o1;
    if constexpr (OP == XRS_LOCAL_SUM && !std::is_same<W, double>::value) {
        u64 s0 = 0, s1 = 0;                                                   // wraps as NumPy's int64 sum does
#pragma unroll 4
        for (int j = 0; j < np; ++j) {
            i64 a, b;
            ld2<i64>(args.p[j], args.dt[j], i, two, a, b);
            s0 += (u64)a;
            s1 += (u64)b;
        }
        o0 = as_out<i64>((i64)s0, out_i64);
        o1 = as_out<i64>((i64)s1, out_i64);
    } else if constexpr (OP == XRS_LOCAL_SUM || OP == XRS_LOCAL_MEAN || OP == XRS_LOCAL_STD) {
        auto get = [&](int j, double &a, double &b) { ld2<double>(args.p[j], args.dt[j], i, two, a, b); };
        double s0, s1;
        pairwise2(np, get, s0, s1);
        if constexpr (OP != XRS_LOCAL_SUM) {
            const double cnt = (double)np;
            s0 = s0 / cnt;
            s1 = s1 / cnt;
        }
        if constexpr (OP == XRS_LOCAL_STD) {
            const double m0 = s0, m1 = s1;
            auto dev = [&](int j, double &a, double &b) {
                ld2<double>(args.p[j], args.dt[j], i, two, a, b);
                a = a - m0;
                b = b - m1;
                a = a * a;
                b = b * b;
            };
            pairwise2(np, dev, s0, s1);
            s0 = sqrt(s0 / (double)np);
            s1 = sqrt(s1 / (double)np);
        }
        o0 = s0;
        o1 = s1;
    } else if constexpr (OP == XRS_LOCAL_MAX || OP == XRS_LOCAL_MIN || OP == XRS_LOCAL_LOWEST || OP == XRS_LOCAL_HIGHEST) {
        constexpr bool UP = OP == XRS_LOCAL_MAX || OP == XRS_LOCAL_HIGHEST;
        W b0, b1;
        ld2<W>(args.p[0], args.dt[0], i, two, b0, b1);
        bool bad0 = is_nan(b0), bad1 = is_nan(b1);
        int at0 = 1, at1 = 1;
#pragma unroll 4                                                              // (several planes' loads in flight)
        for (int j = 1; j < np; ++j) {
            W a, b;
            ld2<W>(args.p[j], args.dt[j], i, two, a, b);
            bad0 |= is_nan(a);
            bad1 |= is_nan(b);
            if (UP ? a > b0 : a < b0) { b0 = a; at0 = j + 1; }                 // strict: the first of equal values keeps its place
            if (UP ? b > b1 : b < b1) { b1 = b; at1 = j + 1; }
        }
        if constexpr (OP == XRS_LOCAL_LOWEST || OP == XRS_LOCAL_HIGHEST) {
            o0 = bad0 ? nan_f64() : as_out<i64>(at0, out_i64);
            o1 = bad1 ? nan_f64() : as_out<i64>(at1, out_i64);
        } else {
            o0 = bad0 ? nan_f64() : as_out<W>(b0, out_i64);
            o1 = bad1 ? nan_f64() : as_out<W>(b1, out_i64);
        }
    } else {                                                                  // the three frequencies
        W r0, r1;
        ld2<W>(ref, ref_dt, i, two, r0, r1);
        const bool in_f32 = ref_dt == XRS_DT_F32;                             // a float32 scalar against a Python number: float32
        bool bad0 = false, bad1 = false;
        int c0 = 0, c1 = 0;
#pragma unroll 4
        for (int j = 0; j < np; ++j) {
            W a, b;
            ld2<W>(args.p[j], args.dt[j], i, two, a, b);
            bad0 |= is_nan(a);
            bad1 |= is_nan(b);
            if constexpr (std::is_same<W, double>::value) {
                if (in_f32) {
                    a = (double)(float)a;
                    b = (double)(float)b;
                }
            }
            c0 += OP == XRS_LOCAL_LESSER ? r0 > a : OP == XRS_LOCAL_EQUAL ? r0 == a : r0 < a;
            c1 += OP == XRS_LOCAL_LESSER ? r1 > b : OP == XRS_LOCAL_EQUAL ? r1 == b : r1 < b;
        }
        o0 = bad0 ? nan_f64() : as_out<i64>(c0, out_i64);
        o1 = bad1 ? nan_f64() : as_out<i64>(c1, out_i64);
    }
    if (two) store_d2u(out + i, o0, o1);
    else st_stream(out + i, o0);
}

// ------------------------------------------------------------------ functions that need the cell's values
// `ref - 1` as the reference computes it: in the dtype of ref_var, wrapping
__device__ __forceinline__ i64 ref_minus_one(i64 r, int dt) {
    const u64 k = (u64)r - 1u;
    switch (dt) {
    case XRS_DT_I8: return (int8_t)k;
    case XRS_DT_U8: return (uint8_t)k;
    case XRS_DT_I16: return (int16_t)k;
    case XRS_DT_U16: return (uint16_t)k;
    case XRS_DT_I32: return (int32_t)k;
    case XRS_DT_U32: return (uint32_t)k;
    default: return (i64)k;
    }
}

template <typename W, int N> __device__ __forceinline__ void bitonic(W (&v)[N]) {
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const W a = v[i], b = v[l];
                    const bool swap = ((i & k) == 0) ? (a > b) : (a < b);
                    v[i] = swap ? b : a;
                    v[l] = swap ? a : b;
                }
            }
        }
    }
}

// the sorted values of one cell: registers (N > 0) or the thread's LDS column (N == 0)
template <typename W, int N> struct Sorted {
    W v[N];
    __device__ __forceinline__ W at(int k) const {
        u64 bits = 0;                                          // (OR of masked words: a chain of selects on the values is turned
#pragma unroll                                                 //  back into an indexed load from scratch at N = 16)
        for (int j = 0; j < N; ++j) bits |= j == k ? word(v[j]) : 0ull;
        if constexpr (std::is_same<W, double>::value) return __longlong_as_double((i64)bits);
        else return (W)bits;
    }
    static __device__ __forceinline__ u64 word(W x) {
        if constexpr (std::is_same<W, double>::value) return (u64)__double_as_longlong(x);
        else return (u64)x;
    }
    __device__ __forceinline__ bool fill(const LocalArgs &args, int np, long i, W *) {
        bool bad = false;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            v[j] = largest<W>();
            if (j < np) {
                v[j] = load_as<W, DT_NO_U64>(args.p[j], args.dt[j], i);
                bad |= is_nan(v[j]);
            }
        }
        bitonic<W, N>(v);
        return bad;
    }
};
constexpr int LDS_THREADS = 128;
template <typename W> struct Sorted<W, 0> {
    W *col;                                                    // col[j * LDS_THREADS]: consecutive lanes, consecutive words
    __device__ __forceinline__ W at(int k) const { return col[k * LDS_THREADS]; }
    __device__ __forceinline__ bool fill(const LocalArgs &args, int np, long i, W *lds) {
        col = lds + threadIdx.x;
        bool bad = false;
        for (int j = 0; j < np; ++j) {
            const W x = load_as<W, DT_NO_U64>(args.p[j], args.dt[j], i);
            bad |= is_nan(x);
            int k = j;
            while (k > 0) {
                const W y = col[(k - 1) * LDS_THREADS];
                if (!(y > x)) break;
                col[k * LDS_THREADS] = y;
                --k;
            }
            col[k * LDS_THREADS] = x;
        }
        return bad;
    }
};

template <int OP, typename W, int N>
__global__ void __launch_bounds__(N ? 256 : LDS_THREADS) local_values_kernel(const LocalArgs args, int np, const void *ref, int ref_dt,
                                                                            long n, double *out) {
    extern __shared__ double lds_raw[];
    const long i = (long)blockIdx.x * (N ? 256 : LDS_THREADS) + threadIdx.x;
    if (i >= n) return;                                        // (no barrier below: a column belongs to one thread)
    Sorted<W, N> s;
    const bool bad = s.fill(args, np, i, reinterpret_cast<W *>(lds_raw));
    double r = nan_f64();
    if constexpr (OP == XRS_LOCAL_MEDIAN) {
        const int h = np >> 1;
        if (!bad) r = (np & 1) ? (double)s.at(h) : ((double)s.at(h - 1) + (double)s.at(h)) / 2.0;
    } else {
        i64 k = ref_minus_one(load_as<i64, DT_NO_U64>(ref, ref_dt, i), ref_dt);
        if constexpr (OP == XRS_LOCAL_RANK) {
            if (k < 0) k += np;                                // Python's wrap; below it the reference raises IndexError: NaN here
            if (!bad && k >= 0 && k < np) r = (double)s.at((int)k);
        } else {                                               // popularity
            int u = 1;
            if constexpr (N > 0) {
#pragma unroll
                for (int j = 1; j < N; ++j) u += (j < np && s.v[j] != s.v[j - 1]) ? 1 : 0;
            } else {
                for (int j = 1; j < np; ++j) u += s.at(j) != s.at(j - 1) ? 1 : 0;
            }
            if (!bad && u < np) {
                if (u == 1) {
                    r = (double)s.at(0);
                } else {
                    if (k < 0) k += u;
                    if (k >= 0 && k < u) {
                        int d = 0;                             // index of the distinct value at hand
                        W pick = s.at(0);
                        if constexpr (N > 0) {
#pragma unroll
                            for (int j = 1; j < N; ++j) {
                                d += (j < np && s.v[j] != s.v[j - 1]) ? 1 : 0;
                                pick = (j < np && d == (int)k && s.v[j] != s.v[j - 1]) ? s.v[j] : pick;
                            }
                        } else {
                            for (int j = 1; j < np && d < (int)k; ++j) {
                                const W x = s.at(j);
                                if (x != s.at(j - 1)) { ++d; pick = x; }
                            }
                        }
                        r = (double)pick;
                    }
                }
            }
        }
    }
    st_stream(out + i, r);
}

inline bool dtype_float(int dt) { return dtype_in(DT_FLOATS, dt); }

int fill_args(const char *who, const void *const *planes, const int *dtypes, int n_planes, LocalArgs &args, bool &any_float) {
    if (!planes || !dtypes) return fail("%s: null pointer", who);
    if (n_planes < 1 || n_planes > MAXP) return fail("%s: n_planes = %d is outside 1 .. %d", who, n_planes, MAXP);
    memset(&args, 0, sizeof(args));
    any_float = false;
    for (int j = 0; j < n_planes; ++j) {
        if (!planes[j]) return fail("%s: null pointer (plane %d)", who, j);
        if (!dtype_in(DT_NO_U64, dtypes[j])) return fail("%s: plane %d has unsupported dtype code %d", who, j, dtypes[j]);
        args.p[j] = planes[j];
        args.dt[j] = (unsigned char)dtypes[j];
        any_float |= dtype_float(dtypes[j]);
    }
    return 0;
}

template <int OP, typename W>
void launch_stream(const LocalArgs &args, int np, const void *ref, int ref_dt, long n, double *out, int out_i64, hipStream_t s) {
    hipLaunchKernelGGL((local_stream_kernel<OP, W>), dim3((unsigned)((n + 511) / 512)), dim3(256), 0, s, args, np, ref, ref_dt, n, out,
                       out_i64);
}

template <int OP, typename W>
void launch_values(const LocalArgs &args, int np, const void *ref, int ref_dt, long n, double *out, hipStream_t s) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (np <= 4) hipLaunchKernelGGL((local_values_kernel<OP, W, 4>), grid, dim3(256), 0, s, args, np, ref, ref_dt, n, out);
    else if (np <= 8) hipLaunchKernelGGL((local_values_kernel<OP, W, 8>), grid, dim3(256), 0, s, args, np, ref, ref_dt, n, out);
    else if (np <= 16) hipLaunchKernelGGL((local_values_kernel<OP, W, 16>), grid, dim3(256), 0, s, args, np, ref, ref_dt, n, out);
    else
        hipLaunchKernelGGL((local_values_kernel<OP, W, 0>), dim3((unsigned)((n + LDS_THREADS - 1) / LDS_THREADS)), dim3(LDS_THREADS),
                           (size_t)np * LDS_THREADS * 8, s, args, np, ref, ref_dt, n, out);
}

// ------------------------------------------------------------------ combine
// what `==` looks at, as a bit pattern in the low 8 * itemsize bits: -0.0 is 0.0, integers are their own pattern
__device__ __forceinline__ u64 canon(const void *p, int dt, long i) {
    switch (dt) {
    case XRS_DT_I8: case XRS_DT_U8: return static_cast<const uint8_t *>(p)[i];
    case XRS_DT_I16: case XRS_DT_U16: return static_cast<const uint16_t *>(p)[i];
    case XRS_DT_I32: case XRS_DT_U32: return static_cast<const uint32_t *>(p)[i];
    case XRS_DT_F32: { const float v = static_cast<const float *>(p)[i]; return v == 0.0f ? 0u : __float_as_uint(v); }
    case XRS_DT_F64: { const double v = static_cast<const double *>(p)[i]; return v == 0.0 ? 0ull : (u64)__double_as_longlong(v); }
    default: return static_cast<const u64 *>(p)[i];
    }
}

__global__ void __launch_bounds__(256) combine_mask_kernel(const LocalArgs args, int np, long n, unsigned char *bad, unsigned *idx,
                                                          unsigned *cls, unsigned *any_bad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool b = false;
    for (int j = 0; j < np; ++j) {
        const int dt = args.dt[j];
        if (dt == XRS_DT_F32) { const float v = static_cast<const float *>(args.p[j])[i]; b |= v != v; }
        else if (dt == XRS_DT_F64) { const double v = static_cast<const double *>(args.p[j])[i]; b |= v != v; }
    }
    bad[i] = b;
    idx[i] = (unsigned)i;
    cls[i] = b;                                                // the NaN cells are one class of their own, valued 0 in every plane
    if (b) *any_bad = 1u;
}

__global__ void __launch_bounds__(256) combine_key_kernel(const void *plane, int dt, const unsigned *idx, const unsigned char *bad, long n,
                                                         u64 *key) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const unsigned c = idx[t];
    key[t] = bad[c] ? 0ull : canon(plane, dt, c);
}

__global__ void __launch_bounds__(256) combine_class_key_kernel(const unsigned *cls, const unsigned *idx, long n, unsigned *ckey) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < n) ckey[t] = cls[idx[t]];
}

__global__ void __launch_bounds__(256) combine_flag_kernel(const void *plane, int dt, const unsigned *idx, const unsigned char *bad,
                                                          const unsigned *ckey, long n, unsigned *flag) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    unsigned f = 1;
    if (t > 0) {
        const unsigned c = idx[t], d = idx[t - 1];
        const u64 v = bad[c] ? 0ull : canon(plane, dt, c), w = bad[d] ? 0ull : canon(plane, dt, d);
        f = (ckey[t] != ckey[t - 1] || v != w) ? 1u : 0u;
    }
    flag[t] = f;
}

__global__ void __launch_bounds__(256) combine_scatter_kernel(const unsigned *idx, const unsigned *scan, long n, unsigned *cls,
                                                             unsigned *count) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    cls[idx[t]] = scan[t] - 1u;
    if (t == n - 1) *count = scan[t];
}

__global__ void __launch_bounds__(256) combine_first_kernel(const unsigned *idx, const unsigned *scan, const unsigned char *bad, long n,
                                                           unsigned *first, unsigned *cid) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    if (t == 0 || scan[t] != scan[t - 1]) {
        const unsigned c = scan[t] - 1u, cell = idx[t];
        first[c] = bad[cell] ? 0xffffffffu : cell;             // the NaN class goes behind every other
        cid[c] = c;
    }
}

__global__ void __launch_bounds__(256) combine_rank_kernel(const unsigned *cid_sorted, long n_classes, unsigned *rank) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r < n_classes) rank[cid_sorted[r]] = (unsigned)r;
}

__global__ void __launch_bounds__(256) combine_out_kernel(const unsigned *cls, const unsigned char *bad, const unsigned *rank, long n,
                                                         double *out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    st_stream(out + i, bad[i] ? nan_f64() : (double)(rank[cls[i]] + 1u));
}

// the cells' values for the key: 8 bytes per (cell, plane), int64 for an integer plane and float64 for a floating one
__global__ void __launch_bounds__(256) local_gather_kernel(const LocalArgs args, int np, const unsigned *cells, long n_cells, long n,
                                                          u64 *out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_cells) return;
    const unsigned c = cells[t];
    for (int j = 0; j < np; ++j) {
        const int dt = args.dt[j];
        u64 bits = 0;
        if ((long)c < n) {
            if (dt == XRS_DT_F32 || dt == XRS_DT_F64) bits = (u64)__double_as_longlong(load_as<double, DT_NO_U64>(args.p[j], dt, c));
            else bits = (u64)load_as<i64, DT_NO_U64>(args.p[j], dt, c);
        }
        out[t * np + j] = bits;
    }
}

struct CombineWork {
    unsigned *idx[2], *cls, *scan, *small;
    u64 *key[2];
    unsigned *half[2][2];           // key[i] seen again, once the value keys are done with: two arrays of n words each
    unsigned char *bad;
    void *cub;
    size_t cub_bytes, total;
};
CombineWork carve_combine(void *base, long n) {
    Carver c(base);
    CombineWork w = {};
    for (int i = 0; i < 2; ++i) w.idx[i] = c.take<unsigned>(n);
    for (int i = 0; i < 2; ++i) {
        Carver halves(c.take_bytes(up256((size_t)n * 8) + 256));   // (256 more: the second half is 256-aligned too)
        w.key[i] = halves.take<u64>(0);
        for (int h = 0; h < 2; ++h) w.half[i][h] = halves.take<unsigned>(n);
    }
    w.cls = c.take<unsigned>(n);
    w.scan = c.take<unsigned>(n);                                   // later: the classes' ranks
    w.bad = c.take<unsigned char>(n);
    w.small = c.take_bytes<unsigned>(256);                          // { class count, any NaN cell }
    size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    hipcub::DoubleBuffer<u64> dk(nullptr, nullptr);
    hipcub::DoubleBuffer<unsigned> dc(nullptr, nullptr), di(nullptr, nullptr);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t1, dk, di, (int)n);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t2, dc, di, (int)n);
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, t3, (unsigned *)nullptr, (unsigned *)nullptr, (int)n);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t4, (const unsigned *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr,
                                             (unsigned *)nullptr, (int)n);
    size_t m = t1 > t2 ? t1 : t2;
    m = m > t3 ? m : t3;
    m = m > t4 ? m : t4;
    w.cub_bytes = up256(m) + 256;
    w.cub = c.take_bytes(w.cub_bytes);
    w.total = c.at();
    return w;
}

}  // namespace

extern "C" {

int xrs_local_cells(int op, const void *const *planes, const int *dtypes, int n_planes, const void *ref_dev, int ref_dtype, int64_t n,
                    void *out_dev, int out_is_i64, void *stream) {
    LocalArgs args;
    bool any_float;
    if (int rc = fill_args("xrs_local_cells", planes, dtypes, n_planes, args, any_float)) return rc;
    if (op < XRS_LOCAL_MAX || op > XRS_LOCAL_POPULARITY) return fail("xrs_local_cells: unknown op %d", op);
    if (!out_dev) return fail("xrs_local_cells: null pointer (out)");
    const bool needs_ref = op == XRS_LOCAL_LESSER || op == XRS_LOCAL_EQUAL || op == XRS_LOCAL_GREATER || op == XRS_LOCAL_RANK ||
                           op == XRS_LOCAL_POPULARITY;
    if (needs_ref) {
        if (!ref_dev) return fail("xrs_local_cells: null pointer (ref)");
        if (!dtype_in(DT_NO_U64, ref_dtype)) return fail("xrs_local_cells: ref has unsupported dtype code %d", ref_dtype);
        if ((op == XRS_LOCAL_RANK || op == XRS_LOCAL_POPULARITY) && dtype_float(ref_dtype))
            return fail("xrs_local_cells: rank and popularity need an integer ref");
        any_float |= dtype_float(ref_dtype);
    }
    const bool float_op = op == XRS_LOCAL_MEAN || op == XRS_LOCAL_STD || op == XRS_LOCAL_MEDIAN;
    const bool w_i64 = !any_float && !float_op;
    if (out_is_i64 && !w_i64)
        return fail("xrs_local_cells: an int64 result needs integer planes and a function other than mean, median and std");
    if (out_is_i64 && (op == XRS_LOCAL_RANK || op == XRS_LOCAL_POPULARITY))
        return fail("xrs_local_cells: rank and popularity can give NaN: their result is float64");
    if (n < 0) return fail("xrs_local_cells: negative size");
    if (n == 0) return 0;
    hipStream_t s = as_stream(stream);
    double *out = static_cast<double *>(out_dev);
#define XRS_STREAM_OP(OPC)                                                                                      \
    case OPC:                                                                                                   \
        if (w_i64) launch_stream<OPC, i64>(args, n_planes, ref_dev, ref_dtype, n, out, out_is_i64, s);          \
        else launch_stream<OPC, double>(args, n_planes, ref_dev, ref_dtype, n, out, 0, s);                      \
        break;
    switch (op) {
        XRS_STREAM_OP(XRS_LOCAL_MAX)
        XRS_STREAM_OP(XRS_LOCAL_MIN)
        XRS_STREAM_OP(XRS_LOCAL_SUM)
        XRS_STREAM_OP(XRS_LOCAL_LESSER)
        XRS_STREAM_OP(XRS_LOCAL_EQUAL)
        XRS_STREAM_OP(XRS_LOCAL_GREATER)
        XRS_STREAM_OP(XRS_LOCAL_LOWEST)
        XRS_STREAM_OP(XRS_LOCAL_HIGHEST)
    case XRS_LOCAL_MEAN: launch_stream<XRS_LOCAL_MEAN, double>(args, n_planes, ref_dev, ref_dtype, n, out, 0, s); break;
    case XRS_LOCAL_STD: launch_stream<XRS_LOCAL_STD, double>(args, n_planes, ref_dev, ref_dtype, n, out, 0, s); break;
    case XRS_LOCAL_MEDIAN: launch_values<XRS_LOCAL_MEDIAN, double>(args, n_planes, ref_dev, ref_dtype, n, out, s); break;
    case XRS_LOCAL_RANK:
        if (w_i64) launch_values<XRS_LOCAL_RANK, i64>(args, n_planes, ref_dev, ref_dtype, n, out, s);
        else launch_values<XRS_LOCAL_RANK, double>(args, n_planes, ref_dev, ref_dtype, n, out, s);
        break;
    default:
        if (w_i64) launch_values<XRS_LOCAL_POPULARITY, i64>(args, n_planes, ref_dev, ref_dtype, n, out, s);
        else launch_values<XRS_LOCAL_POPULARITY, double>(args, n_planes, ref_dev, ref_dtype, n, out, s);
        break;
    }
#undef XRS_STREAM_OP
    XRS_LAUNCH_CHECK();
    return 0;
}

size_t xrs_local_combine_workspace_bytes(int64_t n, int n_planes) {
    (void)n_planes;
    if (n <= 0 || n >= (1LL << 31)) return 256;
    return carve_combine(nullptr, n).total;
}

int xrs_local_combine(const void *const *planes, const int *dtypes, int n_planes, int64_t n, void *work_dev, size_t work_bytes,
                      double *out_dev, unsigned *first_cells_dev, int64_t first_capacity, int64_t *n_classes, void *stream) {
    const char *who = "xrs_local_combine";
    LocalArgs args;
    bool any_float;
    if (int rc = fill_args(who, planes, dtypes, n_planes, args, any_float)) return rc;
    if (!n_classes) return fail("%s: null pointer (n_classes)", who);
    if (n < 0) return fail("%s: negative size", who);
    if (n >= (1LL << 31)) return fail("%s: at most 2^31-1 cells per call", who);
    if (n == 0) { *n_classes = 0; return 0; }
    if (!work_dev) return fail("%s: null pointer (workspace)", who);
    const CombineWork w = carve_combine(work_dev, n);
    if (work_bytes < w.total) return fail("%s: workspace too small (%zu < %zu)", who, work_bytes, w.total);
    hipStream_t s = as_stream(stream);
    if (first_cells_dev) {                                     // second call: the list the first call left in the workspace
        if (*n_classes < 0 || *n_classes > first_capacity || *n_classes > n) return fail("%s: room for %lld first cells, %lld classes", who, (long long)first_capacity, (long long)*n_classes);
        if (*n_classes) XRS_HIP(hipMemcpyAsync(first_cells_dev, w.half[0][1], (size_t)*n_classes * 4, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    if (!out_dev) return fail("%s: null pointer (out)", who);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    XRS_HIP(hipMemsetAsync(w.small, 0, 256, s));
    hipLaunchKernelGGL(combine_mask_kernel, grid, block, 0, s, args, n_planes, (long)n, w.bad, w.idx[0], w.cls, w.small + 1);
    XRS_LAUNCH_CHECK();
    hipcub::DoubleBuffer<unsigned> di(w.idx[0], w.idx[1]);
    unsigned host_small[2] = {2u, 0u};                         // classes so far: the valid cells and the NaN cells
    for (int j = 0; j < n_planes; ++j) {
        hipLaunchKernelGGL(combine_key_kernel, grid, block, 0, s, args.p[j], (int)args.dt[j], di.Current(), w.bad, (long)n, w.key[0]);
        XRS_LAUNCH_CHECK();
        hipcub::DoubleBuffer<u64> dk(w.key[0], w.key[1]);
        size_t cb = w.cub_bytes;
        XRS_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cb, dk, di, (int)n, 0, 8 * dtype_bytes(args.dt[j]), s));
        unsigned *ck[2] = {w.half[0][0], w.half[1][0]};                                // (the value keys are done with)
        hipLaunchKernelGGL(combine_class_key_kernel, grid, block, 0, s, w.cls, di.Current(), (long)n, ck[0]);
        XRS_LAUNCH_CHECK();
        int cbits = 1;
        while (cbits < 32 && (1ull << cbits) < (u64)host_small[0]) ++cbits;
        hipcub::DoubleBuffer<unsigned> dc(ck[0], ck[1]);
        cb = w.cub_bytes;
        XRS_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cb, dc, di, (int)n, 0, cbits, s));
        hipLaunchKernelGGL(combine_flag_kernel, grid, block, 0, s, args.p[j], (int)args.dt[j], di.Current(), w.bad, dc.Current(), (long)n, w.scan);
        XRS_LAUNCH_CHECK();
        cb = w.cub_bytes;
        XRS_HIP(hipcub::DeviceScan::InclusiveSum(w.cub, cb, w.scan, w.scan, (int)n, s));
        hipLaunchKernelGGL(combine_scatter_kernel, grid, block, 0, s, di.Current(), w.scan, (long)n, w.cls, w.small);
        XRS_LAUNCH_CHECK();
        XRS_HIP(hipMemcpyAsync(host_small, w.small, 8, hipMemcpyDeviceToHost, s));
        XRS_HIP(hipStreamSynchronize(s));
        if (host_small[0] < 1 || (int64_t)host_small[0] > n) return fail("%s: internal error: %u classes of %lld cells", who, host_small[0], (long long)n);
    }
    const long total = host_small[0];
    unsigned *first = w.half[0][0], *first_sorted = w.half[0][1], *cid = w.half[1][0], *cid_sorted = w.half[1][1];
    hipLaunchKernelGGL(combine_first_kernel, grid, block, 0, s, di.Current(), w.scan, w.bad, (long)n, first, cid);
    XRS_LAUNCH_CHECK();
    size_t cb = w.cub_bytes;
    XRS_HIP(hipcub::DeviceRadixSort::SortPairs(w.cub, cb, (const unsigned *)first, first_sorted, (const unsigned *)cid, cid_sorted, (int)total, 0, 32, s));
    hipLaunchKernelGGL(combine_rank_kernel, dim3((unsigned)((total + 255) / 256)), block, 0, s, cid_sorted, total, w.scan);
    XRS_LAUNCH_CHECK();
    hipLaunchKernelGGL(combine_out_kernel, grid, block, 0, s, w.cls, w.bad, w.scan, (long)n, out_dev);
    XRS_LAUNCH_CHECK();
    XRS_HIP(hipStreamSynchronize(s));
    *n_classes = total - (host_small[1] ? 1 : 0);
    return 0;
}

int xrs_local_gather(const void *const *planes, const int *dtypes, int n_planes, int64_t n, const unsigned *cells_dev, int64_t n_cells,
                     void *out_dev, void *stream) {
    LocalArgs args;
    bool any_float;
    if (int rc = fill_args("xrs_local_gather", planes, dtypes, n_planes, args, any_float)) return rc;
    if (n < 0 || n_cells < 0) return fail("xrs_local_gather: negative size");
    if (n_cells == 0) return 0;
    if (!cells_dev || !out_dev) return fail("xrs_local_gather: null pointer");
    hipLaunchKernelGGL(local_gather_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, as_stream(stream), args, n_planes,
                       cells_dev, (long)n_cells, (long)n, static_cast<u64 *>(out_dev));
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

// natural_breaks (xrspatial/classify.py:508-564 `_run_numpy_jenks_matrices`): the two tables of the Jenks dynamic programme,
// and the typed gather that fetches its sample.  DESIGN.md §6j.
//
// The reference's loop nest runs row by row (l), walks m = 0 .. l-1 down the sorted sample and updates every class column j
// inside.  What it computes is  V[l][j] = min over i4 = l-1-m >= 1 of ( var(data[i4 .. l-1]) + V[i4][j-1] ):  column j reads
// column j-1 only, and the rows of a column do not read one another.  So: one launch per column, one thread per row, and each
// thread walks its own m in the reference's order with the reference's types -- float64 running sums of float32 values (the
// square rounded to float32 first), one IEEE float64 division per step, the running minimum kept in float32 and replaced on
// `>=`, so that the later m wins a tie.  Every rounding and every tie then falls as in the reference's loop.
//
// No FMA contraction anywhere in this file: `sum_squares - (sum * sum) / w` and `variance + V` must round after every operation.
#pragma clang fp contract(off)

#include "xrs_common.h"
#include "workspace.h"

#include <cmath>

namespace {

using xrs::as_stream;
using xrs::fail;
using xrs::up256;

constexpr int BLOCK = 64;               // one wave per workgroup: the ~n / 64 waves of a column spread over all CUs
constexpr long N_MAX = 1L << 24;        // the lower class limits are float32 row numbers: exact below 2^24

// the reference's initial tables, and rows 0 and 1 of both working columns (V[0][j] is never read, V[1][j] = 0)
__global__ __launch_bounds__(256) void jenks_init_kernel(float *__restrict__ limits, float *__restrict__ var, float *__restrict__ col_a,
                                                         float *__restrict__ col_b, long n, int k) {
    const long cells = (n + 1) * (long)(k + 1);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < 2) {
        col_a[i] = 0.0f;
        col_b[i] = 0.0f;
    }
    if (i >= cells) return;
    const long l = i / (k + 1);
    const int j = (int)(i - l * (k + 1));
    limits[i] = (l == 1 && j >= 1) ? 1.0f : 0.0f;
    var[i] = (l >= 2 && j >= 1) ? INFINITY : 0.0f;
}

// Column j of both tables.  Thread t of block b owns row l = n - (64 b + t): the longest walks start first, the rows of a wave
// are consecutive (the loads of `sorted` and of the previous column are coalesced, and the lanes of a wave differ by at most
// 63 steps).  `prev` is column j-1 of V, contiguous (entries 1 .. n); `cur` receives column j.
template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void jenks_column_kernel(const float *__restrict__ sorted, const float *__restrict__ prev,
                                                            float *__restrict__ cur, float *__restrict__ limits,
                                                            float *__restrict__ var, int n, int k, int j) {
    const long l = (long)n - ((long)blockIdx.x * BLOCK + threadIdx.x);
    if (l < 2) return;
    const float *data = sorted + (l - 1);           // data[-m] is the reference's data[i4], i4 = l - 1 - m
    const float *vcol = prev + (l - 1);             // vcol[-m] is V[i4][j - 1]
    double sum = 0.0, sum_squares = 0.0, w = 0.0, variance = 0.0;
    float best = INFINITY, limit = 0.0f;
    const int last = (int)l - 1;                    // m = l - 1 is i4 == 0: the sums move, no class starts there
#pragma unroll 4
    for (int m = 0; m < last; ++m) {
        const float val = data[-m];
        w += 1.0;
        sum += (double)val;
        sum_squares += (double)(val * val);
        variance = sum_squares - (sum * sum) / w;
        if (!FIRST) {
            const double cand = variance + (double)vcol[-m];
            if ((double)best >= cand) {
                best = (float)cand;
                limit = (float)((int)l - m);
            }
        }
    }
    if (FIRST) {                                    // column 1: one class, the variance of data[0 .. l-1]
        const float val = data[-last];
        w += 1.0;
        sum += (double)val;
        sum_squares += (double)(val * val);
        variance = sum_squares - (sum * sum) / w;
        best = (float)variance;
        limit = 1.0f;
    }
    cur[l] = best;
    const long at = l * (long)(k + 1) + j;
    limits[at] = limit;
    var[at] = best;
}

template <typename T>
__global__ __launch_bounds__(256) void gather_kernel(const T *__restrict__ in, long n, const unsigned *__restrict__ idx, long n_idx,
                                                     T *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_idx) return;
    const unsigned at = idx[i];
    out[i] = (long)at < n ? in[at] : T(0);
}

template <typename T>
void launch_gather(const void *in, long n, const unsigned *idx, long n_idx, void *out, hipStream_t s) {
    hipLaunchKernelGGL((gather_kernel<T>), dim3((unsigned)((n_idx + 255) / 256)), dim3(256), 0, s, static_cast<const T *>(in), n, idx,
                       n_idx, static_cast<T *>(out));
}

}  // namespace

extern "C" {

size_t xrs_jenks_workspace_bytes(int64_t n, int k) {
    if (n < 1 || n >= N_MAX || k < 1) return 0;
    return 2 * up256((size_t)(n + 1) * sizeof(float));
}

int xrs_jenks_matrices_f32(const float *sorted_dev, int64_t n, int k, float *lower_class_limits_dev, float *var_combinations_dev,
                           void *work_dev, size_t work_bytes, void *stream) {
    if (n < 1) return fail("xrs_jenks_matrices_f32: a sample of at least 1 value is needed, got %ld", (long)n);
    if (n >= N_MAX) return fail("xrs_jenks_matrices_f32: at most 2^24 - 1 sample values (%ld): the class limits are float32", (long)n);
    if (k < 1) return fail("xrs_jenks_matrices_f32: at least 1 class is needed, got %d", k);
    if ((n + 1) * ((long)k + 1) >= (1L << 40)) return fail("xrs_jenks_matrices_f32: tables too large (%ld x %d)", (long)n + 1, k + 1);
    if (!sorted_dev || !lower_class_limits_dev || !var_combinations_dev || !work_dev)
        return fail("xrs_jenks_matrices_f32: null pointer");
    if (work_bytes < xrs_jenks_workspace_bytes(n, k))
        return fail("xrs_jenks_matrices_f32: workspace of %zu bytes, %zu needed", work_bytes, xrs_jenks_workspace_bytes(n, k));
    hipStream_t s = as_stream(stream);
    float *col[2] = {static_cast<float *>(work_dev),
                     reinterpret_cast<float *>(static_cast<char *>(work_dev) + up256((size_t)(n + 1) * sizeof(float)))};
    const long cells = (n + 1) * ((long)k + 1);
    hipLaunchKernelGGL(jenks_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, lower_class_limits_dev,
                       var_combinations_dev, col[0], col[1], (long)n, k);
    XRS_LAUNCH_CHECK();
    if (n < 2) return 0;
    const unsigned blocks = (unsigned)((n - 1 + BLOCK - 1) / BLOCK);        // rows 2 .. n
    for (int j = 1; j <= k; ++j) {
        const float *prev = col[(j - 1) & 1];
        float *cur = col[j & 1];
        if (j == 1)
            hipLaunchKernelGGL((jenks_column_kernel<true>), dim3(blocks), dim3(BLOCK), 0, s, sorted_dev, prev, cur,
                               lower_class_limits_dev, var_combinations_dev, (int)n, k, j);
        else
            hipLaunchKernelGGL((jenks_column_kernel<false>), dim3(blocks), dim3(BLOCK), 0, s, sorted_dev, prev, cur,
                               lower_class_limits_dev, var_combinations_dev, (int)n, k, j);
        XRS_LAUNCH_CHECK();
    }
    return 0;
}

int xrs_gather_elems(const void *in_dev, int elem_size, int64_t n, const uint32_t *idx_dev, int64_t n_idx, void *out_dev,
                     void *stream) {
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8)
        return fail("xrs_gather_elems: elements of 1, 2, 4 or 8 bytes, got %d", elem_size);
    if (n < 0 || n_idx < 0) return fail("xrs_gather_elems: negative size");
    if (n > (1L << 32)) return fail("xrs_gather_elems: at most 2^32 elements (%ld): the indices are uint32", (long)n);
    if (n_idx >= (1L << 39)) return fail("xrs_gather_elems: too many indices (%ld)", (long)n_idx);
    if (n_idx == 0) return 0;
    if (!in_dev || !idx_dev || !out_dev) return fail("xrs_gather_elems: null pointer");
    hipStream_t s = as_stream(stream);
    switch (elem_size) {
    case 1: launch_gather<uint8_t>(in_dev, n, idx_dev, n_idx, out_dev, s); break;
    case 2: launch_gather<uint16_t>(in_dev, n, idx_dev, n_idx, out_dev, s); break;
    case 4: launch_gather<uint32_t>(in_dev, n, idx_dev, n_idx, out_dev, s); break;
    default: launch_gather<uint64_t>(in_dev, n, idx_dev, n_idx, out_dev, s); break;
    }
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

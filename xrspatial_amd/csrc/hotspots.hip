// focal.hotspots (Getis-Ord Gi*) support kernels: global NaN-skipping moments and the z-score classifier.
//
// Reference: _hotspots_numpy (xrspatial/focal.py:914-934): mean_array = convolve_2d(data, kernel/kernel.sum());
// z = (mean_array - nanmean(data)) / nanstd(data); _calc_hotspots_numpy (:881-911) maps z to
// {0, +-90, +-95, +-99}.  The convolution is xrs_convolve2d_f32; here:
//   xrs_nan_moments_f32   ONE streaming pass over shifted values (count, sum, sum of squares in float64):
//                         wave64 DPP reductions, one atomic per wave;
//   xrs_hotspots_classify_f32   z in float32 exactly as the reference forms it, compared with the thresholds as float64
//                         values (classify() below), int8 out (4 B in + 1 B out per cell).
#include "xrs_common.h"

#include "wave_reduce.h"

using namespace xrs;

namespace {

struct Moments {                 // device-resident, 32 bytes
    unsigned long long count;
    double sum, ssd, mean;
};

// Single streaming pass: count, sum and sum of squares of the values SHIFTED by `m->mean` (set beforehand to the mean
// of a small sample, so the shifted values are centred to within a few standard deviations and the one-pass
// variance  (S2 - S1^2/n)/n  is well conditioned in float64; the reference's own float32 np.nanmean / np.nanstd carry
// ~1e-6 relative error).  Each workgroup streams ONE contiguous chunk (chunks dealt to XCDs in contiguous runs), the
// pattern that measured 1.3x faster than a grid-strided comb on the per-cell kernels.
__global__ void moments_sample_kernel(const float *x, long n, Moments *m) {
    __shared__ double ssum[256];
    __shared__ unsigned scnt[256];
    const long take = n < 4096 ? n : 4096;          // (a shift within a few sigma of the mean is all that is needed)
    double acc = 0.0;
    unsigned cnt = 0;
    for (long i = threadIdx.x; i < take; i += 256)
        if (isfinite(x[i])) { acc += (double)x[i]; ++cnt; }
    ssum[threadIdx.x] = acc; scnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { ssum[threadIdx.x] += ssum[threadIdx.x + o]; scnt[threadIdx.x] += scnt[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        m->count = 0ull; m->sum = 0.0; m->ssd = 0.0;
        m->mean = scnt[0] ? ssum[0] / (double)scnt[0] : 0.0;           // the shift
    }
}

__global__ void __launch_bounds__(256) moments_kernel(const float *x, long n, Moments *m, const int vec) {
    const double shift = m->mean;
    double s1 = 0.0, s2 = 0.0;
    unsigned cnt = 0;
    const long n4 = vec ? n >> 2 : 0;                   // 16-byte loads only when the plane is 16-byte aligned
    const long n_chunks = gridDim.x;                    // a multiple of 8
    const long my_chunk = ((long)blockIdx.x & 7) * (n_chunks >> 3) + ((long)blockIdx.x >> 3);
    const long per_chunk = ((n4 + n_chunks - 1) / n_chunks + 1023) & ~1023L;
    const long c_begin = my_chunk * per_chunk;
    const long c_end = c_begin + per_chunk < n4 ? c_begin + per_chunk : n4;
    constexpr int U = 4;                                // 16-byte loads in flight per lane
    for (long i0 = c_begin + threadIdx.x; i0 < c_end; i0 += 256 * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = i0 + 256 * u;
            v[u] = i < c_end ? ldg_stream(reinterpret_cast<const float4 *>(x) + i) : make_float4(nan_f32(), nan_f32(), nan_f32(), nan_f32());
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float e[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = !isnan(e[k]);
                const double d = ok ? (double)e[k] - shift : 0.0;
                s1 += d;
                s2 = fma(d, d, s2);
                cnt += ok ? 1u : 0u;
            }
        }
    }
    const long stride = (long)gridDim.x * 256;
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        if (!isnan(x[i])) {
            const double d = (double)x[i] - shift;
            s1 += d;
            s2 = fma(d, d, s2);
            ++cnt;
        }
    s1 = wave_reduce<WrSum>(s1);                       // (wave_reduce.h: DPP row folds + v_readlane)
    s2 = wave_reduce<WrSum>(s2);
    cnt = wave_reduce<WrSum>(cnt);
    // one set of atomics per workgroup (three addresses shared by the whole grid)
    __shared__ double w1[4], w2[4];
    __shared__ unsigned wc[4];
    if ((threadIdx.x & 63) == 0) { w1[threadIdx.x >> 6] = s1; w2[threadIdx.x >> 6] = s2; wc[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned c = wc[0] + wc[1] + wc[2] + wc[3];
        if (c) {
            atomicAdd(&m->sum, (w1[0] + w1[1]) + (w1[2] + w1[3]));
            atomicAdd(&m->ssd, (w2[0] + w2[1]) + (w2[2] + w2[3]));
            atomicAdd(&m->count, (unsigned long long)c);
        }
    }
}

__global__ void moments_final_kernel(Moments *m) {
    const double n = (double)m->count, s1 = m->sum, s2 = m->ssd, shift = m->mean;
    if (m->count) {
        const double md = s1 / n;
        const double ssd = s2 - s1 * md;
        m->mean = shift + md;
        m->ssd = ssd < 0.0 ? 0.0 : ssd;            // rounding guard only: a NaN (inf cells: inf - inf) stays NaN, like np.nanstd
        m->sum = m->mean * n;
    } else {
        m->mean = nan(""); m->ssd = 0.0; m->sum = 0.0;
    }
}

// The reference's Numba loop compares the float32 z-score with the Python literals 2.33, 1.65, ... in FLOAT64 (Numba unifies
// float32 with a float64 constant to float64).  For a float32 `a` and a double `t`,  (double)a >= t  is  a >= the smallest
// float32 not below t,  and  (double)a > t  is  a > the largest float32 not above t:  so the ladder stays in float32 with
// these constants.  Rounding t to float32 instead differs at one magnitude, a == 1.96f (which lies above 1.96: 95, not 90).
constexpr bool ceil32_of(float c, double t, float ulp) { return (double)c >= t && (double)(c - ulp) < t; }
constexpr bool floor32_of(float c, double t, float ulp) { return (double)c <= t && (double)(c + ulp) > t; }
constexpr float GE_1_29 = 0x1.4a3d72p+0f, GE_1_65 = 0x1.a66668p+0f, GE_2_33 = 0x1.2a3d72p+1f;
constexpr float GT_1_65 = 0x1.a66666p+0f, GT_1_96 = 0x1.f5c28ep+0f, GT_2_58 = 0x1.4a3d70p+1f;
static_assert(ceil32_of(GE_1_29, 1.29, 0x1p-23f) && ceil32_of(GE_1_65, 1.65, 0x1p-23f) && ceil32_of(GE_2_33, 2.33, 0x1p-22f),
              "not the smallest float32 at or above the reference's thresholds");
static_assert(floor32_of(GT_1_65, 1.65, 0x1p-23f) && floor32_of(GT_1_96, 1.96, 0x1p-23f) && floor32_of(GT_2_58, 2.58, 0x1p-22f),
              "not the largest float32 at or below the reference's thresholds");

__device__ __forceinline__ signed char classify(float z) {
    // focal.py:889-909
    const float a = fabsf(z);
    float p = 1.0f;
    if (a >= GE_2_33) p = 0.0099f;
    else if (a >= GE_1_65) p = 0.0495f;
    else if (a >= GE_1_29) p = 0.0985f;
    int conf = 0;
    if (a > GT_2_58 && p < 0.01f) conf = 99;
    else if (a > GT_1_96 && p < 0.05f) conf = 95;
    else if (a > GT_1_65 && p < 0.1f) conf = 90;
    const int hot = z > 0.0f ? 1 : (z < 0.0f ? -1 : 0);
    return (signed char)(hot * conf);
}

// 4 cells per lane and trip (one 16-byte load, one 4-byte store of four int8 classes), contiguous chunk per workgroup.
__global__ void __launch_bounds__(256) classify_kernel(const float *mean_array, signed char *out, long n, float gmean,
                                                       float gstd, const int vec) {
    const long n4 = vec ? n >> 2 : 0;
    const long n_chunks = gridDim.x;                    // a multiple of 8
    const long my_chunk = ((long)blockIdx.x & 7) * (n_chunks >> 3) + ((long)blockIdx.x >> 3);
    const long per_chunk = ((n4 + n_chunks - 1) / n_chunks + 1023) & ~1023L;
    const long c_begin = my_chunk * per_chunk;
    const long c_end = c_begin + per_chunk < n4 ? c_begin + per_chunk : n4;
    constexpr int U = 4;
    for (long i0 = c_begin + threadIdx.x; i0 < c_end; i0 += 256 * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + 256 * u < c_end) v[u] = ldg_stream(reinterpret_cast<const float4 *>(mean_array) + i0 + 256 * u);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (i0 + 256 * u < c_end) {
                const unsigned b0 = (unsigned char)classify((v[u].x - gmean) / gstd);
                const unsigned b1 = (unsigned char)classify((v[u].y - gmean) / gstd);
                const unsigned b2 = (unsigned char)classify((v[u].z - gmean) / gstd);
                const unsigned b3 = (unsigned char)classify((v[u].w - gmean) / gstd);
                st_stream(reinterpret_cast<unsigned *>(out) + i0 + 256 * u, b0 | (b1 << 8) | (b2 << 16) | (b3 << 24));
            }
    }
    const long stride = (long)gridDim.x * 256;
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        out[i] = classify((mean_array[i] - gmean) / gstd);
}

}  // namespace

extern "C" {

int xrs_nan_moments_f32(const float *in_dev, int64_t n, void *moments32_dev, void *stream) {
    if (n < 0) return fail("xrs_nan_moments_f32: negative size");
    if (!moments32_dev || (n && !in_dev)) return fail("xrs_nan_moments_f32: null pointer");
    Moments *m = static_cast<Moments *>(moments32_dev);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(moments_sample_kernel, dim3(1), dim3(256), 0, s, in_dev, (long)n, m);
    const int vec = aligned16(in_dev) ? 1 : 0;
    if (n) {
        long g = (n / 4 + 255) / 256;
        g = g > 2048 ? 2048 : (g < 1 ? 1 : g);
        hipLaunchKernelGGL(moments_kernel, dim3((unsigned)xcd_grid(g, 1)), dim3(256), 0, s, in_dev, (long)n, m, vec);
    }
    hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(1), 0, s, m);
    XRS_LAUNCH_CHECK();
    return 0;
}

int xrs_hotspots_classify_f32(const float *mean_array_dev, signed char *out_dev, int64_t n, float global_mean,
                              float global_std, void *stream) {
    if (n < 0) return fail("xrs_hotspots_classify_f32: negative size");
    if (n == 0) return 0;
    if (!mean_array_dev || !out_dev) return fail("xrs_hotspots_classify_f32: null pointer");
    long g = (n / 4 + 255) / 256;
    g = g > 2048 ? 2048 : (g < 1 ? 1 : g);
    const int vec = aligned16(mean_array_dev) && (reinterpret_cast<uintptr_t>(out_dev) & 3u) == 0;
    hipLaunchKernelGGL(classify_kernel, dim3((unsigned)xcd_grid(g, 1)), dim3(256), 0, as_stream(stream), mean_array_dev,
                       out_dev, (long)n, global_mean, global_std, vec);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"

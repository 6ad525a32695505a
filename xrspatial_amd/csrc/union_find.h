// Union-find with root = smallest index, in LDS (workgroup scope) and in global memory (agent scope), and the float64
// tolerance threshold of the reference's `isclose`-style predicates.  Shared by regions.hip and polygonize.hip.
#pragma once
#include "xrs_common.h"

namespace xrs {

// atol + rtol * abs(v): a multiply, then an add -- hipcc at -O3 would fuse them into one v_fma_f64, which rounds once
__device__ __forceinline__ double threshold(double abs_v) {
#pragma clang fp contract(off)
    const double scaled = 1e-05 * abs_v;
    return 1e-08 + scaled;
}

// ------------------------------------------------------------------ union-find, root = smallest index
// Every entry satisfies p[x] <= x, equality exactly at a root.  A root's entry changes only by CAS(x -> smaller root),
// so sets only ever merge; a non-root entry is only lowered (atomicMin) to an ancestor, which stays in its set.  Every
// loop follows a strictly decreasing index, or retries a CAS that failed because another union took a root away.
__device__ __forceinline__ uint32_t lds_ld(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

static __device__ uint32_t lds_find(uint32_t *par, uint32_t x) {
    uint32_t p = lds_ld(par + x);
    while (p != x) {
        const uint32_t g = lds_ld(par + p);
        if (g != p) __hip_atomic_fetch_min(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // halve
        x = g;
        p = lds_ld(par + x);
    }
    return x;
}

static __device__ void lds_union(uint32_t *par, uint32_t a, uint32_t b) {
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        uint32_t expect = b;
        if (__hip_atomic_compare_exchange_strong(par + b, &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP))
            return;
    }
}

// a global parent[] while unions run: agent-scope relaxed loads (L2, never a stale L1 line) and agent-scope RMWs
__device__ __forceinline__ uint32_t g_ld(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

static __device__ uint32_t g_find(uint32_t *par, uint32_t x) {
    uint32_t p = g_ld(par + x);
    while (p != x) {
        const uint32_t g = g_ld(par + p);
        if (g != p) __hip_atomic_fetch_min(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // x is no root
        x = g;
        p = g_ld(par + x);
    }
    return x;
}

static __device__ void g_union(uint32_t *par, uint32_t a, uint32_t b) {
    for (;;) {
        a = g_find(par, a);
        b = g_find(par, b);
        if (a == b) return;
        if (a > b) { const uint32_t t = a; a = b; b = t; }
        uint32_t expect = b;
        if (__hip_atomic_compare_exchange_strong(par + b, &expect, a, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
}

}  // namespace xrs

// Does a cell equal one of n 8-byte values under NumPy's == ?  Shared by proximity (target_values) and pathfinding (barriers).
// `kind` says how the values are read (XRS_PROX_VALUES_*): int64 / uint64 for integer rasters, compared as integers so that
// values beyond 2^53 stay apart; float64 otherwise, the cell converted to float64 (NumPy's promotion).  NaN equals nothing.
#pragma once
#include "xrs_common.h"

#include <type_traits>

namespace xrs {

template <typename T>
__device__ __forceinline__ bool matches_any(T v, const void *__restrict__ values, int kind, int n) {
    bool hit = false;
    if constexpr (std::is_integral<T>::value) {
        if (kind == XRS_PROX_VALUES_I64) {
            const int64_t *q = static_cast<const int64_t *>(values);
            for (int k = 0; k < n; ++k) {
                if constexpr (std::is_unsigned<T>::value) hit |= q[k] >= 0 && (uint64_t)q[k] == (uint64_t)v;
                else hit |= (int64_t)v == q[k];
            }
            return hit;
        }
        if (kind == XRS_PROX_VALUES_U64) {
            const uint64_t *q = static_cast<const uint64_t *>(values);
            for (int k = 0; k < n; ++k) {
                if constexpr (std::is_unsigned<T>::value) hit |= (uint64_t)v == q[k];
                else hit |= v >= 0 && (uint64_t)v == q[k];
            }
            return hit;
        }
    }
    const double *q = static_cast<const double *>(values);
    for (int k = 0; k < n; ++k) hit |= (double)v == q[k];
    return hit;
}

}  // namespace xrs

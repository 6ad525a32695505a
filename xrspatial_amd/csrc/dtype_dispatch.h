// XRS_DT_* codes (include/xrs_hip.h) to C++ types: the one table behind every entry point that takes a raster in its own
// dtype as (const void *, int dtype).  An unknown code, or one outside the caller's set, is refused -- never read as some type.
#pragma once

#include "xrs_common.h"

namespace xrs {

template <typename T> struct tag { using type = T; };
template <typename Tag> using dtype_of = typename Tag::type;   // in a with_dtype callback: using T = dtype_of<decltype(t)>;

// sets of codes, one bit each
constexpr unsigned dt_bit(int code) { return 1u << code; }
constexpr unsigned DT_ALL = (1u << 10) - 1;
constexpr unsigned DT_F32 = dt_bit(XRS_DT_F32);
constexpr unsigned DT_NO_F32 = DT_ALL & ~DT_F32;
constexpr unsigned DT_NO_F64 = DT_ALL & ~dt_bit(XRS_DT_F64);
constexpr unsigned DT_NO_U64 = DT_ALL & ~dt_bit(XRS_DT_U64);
constexpr unsigned DT_FLOATS = dt_bit(XRS_DT_F32) | dt_bit(XRS_DT_F64);

namespace detail {
template <unsigned MASK, int CODE, typename T, typename F> inline bool call_if(F &f) {
    if constexpr ((MASK >> CODE) & 1u) { f(tag<T>{}); return true; }
    else return false;
}
}  // namespace detail

// f(tag<T>{}) for the type of `code`; false, and no call, for a code that is unknown or outside MASK.  f is instantiated for
// the types in MASK only: a caller without a kernel for some type leaves it out and gains none.  The instantiations, and so
// the kernels in the unit's code object, come in the order of the cases below.
template <unsigned MASK = DT_ALL, typename F> inline bool with_dtype(int code, F &&f) {
    switch (code) {
    case XRS_DT_I8: return detail::call_if<MASK, XRS_DT_I8, int8_t>(f);
    case XRS_DT_U8: return detail::call_if<MASK, XRS_DT_U8, uint8_t>(f);
    case XRS_DT_I16: return detail::call_if<MASK, XRS_DT_I16, int16_t>(f);
    case XRS_DT_U16: return detail::call_if<MASK, XRS_DT_U16, uint16_t>(f);
    case XRS_DT_I32: return detail::call_if<MASK, XRS_DT_I32, int32_t>(f);
    case XRS_DT_U32: return detail::call_if<MASK, XRS_DT_U32, uint32_t>(f);
    case XRS_DT_I64: return detail::call_if<MASK, XRS_DT_I64, int64_t>(f);
    case XRS_DT_U64: return detail::call_if<MASK, XRS_DT_U64, uint64_t>(f);
    case XRS_DT_F32: return detail::call_if<MASK, XRS_DT_F32, float>(f);
    case XRS_DT_F64: return detail::call_if<MASK, XRS_DT_F64, double>(f);
    default: return false;
    }
}

// with_dtype over all ten codes with float32 instantiated last: composite, proximity and pathfinding have always had their
// float32 kernel behind the float64 one, and this keeps their code objects as they were, byte for byte.
template <typename F> inline bool with_dtype_f32_last(int code, F &&f) {
    return with_dtype<DT_NO_F32>(code, f) || with_dtype<DT_F32>(code, f);
}

// item size of a code; 0 for an unknown one, so `!dtype_bytes(code)` is the test for "not a dtype code"
inline int dtype_bytes(int code) {
    int bytes = 0;
    with_dtype(code, [&](auto t) { bytes = (int)sizeof(dtype_of<decltype(t)>); });
    return bytes;
}

// whether `code` is one of the codes in `mask`
inline bool dtype_in(unsigned mask, int code) { return dtype_bytes(code) && ((mask >> code) & 1u); }

// Device side: cell i of a plane of dtype `dt`, widened to W.  The host refused every code outside MASK before the launch,
// so float32, which every caller's set holds, takes what is left.
template <typename W, unsigned MASK = DT_ALL> __device__ __forceinline__ W load_as(const void *p, int dt, long i) {
    switch (dt) {
    case XRS_DT_I8: return (W) static_cast<const int8_t *>(p)[i];
    case XRS_DT_U8: return (W) static_cast<const uint8_t *>(p)[i];
    case XRS_DT_I16: return (W) static_cast<const int16_t *>(p)[i];
    case XRS_DT_U16: return (W) static_cast<const uint16_t *>(p)[i];
    case XRS_DT_I32: return (W) static_cast<const int32_t *>(p)[i];
    case XRS_DT_U32: return (W) static_cast<const uint32_t *>(p)[i];
    case XRS_DT_I64: return (W) static_cast<const int64_t *>(p)[i];
    case XRS_DT_F64: return (W) static_cast<const double *>(p)[i];
    case XRS_DT_U64:
        if constexpr (MASK & dt_bit(XRS_DT_U64)) return (W) static_cast<const uint64_t *>(p)[i];
        [[fallthrough]];
    default: return (W) static_cast<const float *>(p)[i];
    }
}

}  // namespace xrs

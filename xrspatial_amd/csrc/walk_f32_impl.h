// Float32 statistics (row-major sum, max, min, range) of focal_stats / focal.apply through the column walker of
// circle_walk.h, for one mask shape (XRS_WALK_SHAPE) and radius 2..12 cells.  For radius <= 3 the float64 moments ride
// along in the same kernel (one read of the raster for all seven statistics).  The tap-by-tap walk of kxk.hip this
// replaces spends 6 VALU + 6 SALU instructions per tap on a 25x25 mask (profiles/r01/pmc_focal25_sum.json).
// Included by kxk_circle.hip and kxk_box.hip, which define XRS_WALK_SHAPE / XRS_WALK_KERNEL / XRS_WALK_ENTRY.
#include "circle_walk.h"

using namespace xrs;

namespace {

template <int R, bool WANT_SUM, bool WANT_MM, bool F64>
__global__ void __launch_bounds__(256) XRS_WALK_KERNEL(const WalkGeom g, const WalkOuts o) {
    walk_tile<R, XRS_WALK_SHAPE, true, WANT_SUM, WANT_MM, F64>(g, o);
}

template <int R, bool WANT_SUM, bool WANT_MM, bool F64>
int launch(WalkGeom &g, const WalkOuts &o, hipStream_t s) {
    long grid;
    if (int rc = walk_grid(g, &grid)) return rc;
    hipLaunchKernelGGL((XRS_WALK_KERNEL<R, WANT_SUM, WANT_MM, F64>), dim3((unsigned)grid), dim3(256), 0, s, g, o);
    XRS_LAUNCH_CHECK();
    route_note(XRS_STR(XRS_WALK_ENTRY), R);
    return 0;
}

template <int R>
int dispatch(WalkGeom &g, const WalkOuts &o, bool with_moments, hipStream_t s) {
    const bool ws = o.sum, wm = o.max || o.min || o.range;
    if (with_moments) {
        if constexpr (R <= 3) return launch<R, true, true, true>(g, o, s);
        else return -1;
    }
    if (ws && wm) return launch<R, true, true, false>(g, o, s);
    if (ws) return launch<R, true, false, false>(g, o, s);
    return launch<R, false, true, false>(g, o, s);
}

}  // namespace

namespace xrs {

// 0 = launched, -1 = not the shape / a radius this file is instantiated for (caller walks the taps), > 0 = error.
// Mean / var / std among the outputs: all seven statistics in one kernel (radius 2 and 3 only).
int XRS_WALK_ENTRY(const WindowCall &c) {
    if (c.mask.kind != ShapeKind<XRS_WALK_SHAPE>::kind) return -1;
    float *const *out = c.out;
    const bool moments = out[XRS_STAT_MEAN] || out[XRS_STAT_VAR] || out[XRS_STAT_STD];
    if (!out[XRS_STAT_SUM] && !out[XRS_STAT_MAX] && !out[XRS_STAT_MIN] && !out[XRS_STAT_RANGE] && !moments) return 0;
    WalkGeom g;
    memset(&g, 0, sizeof(g));
    fill_geom(g, c);
    const WalkOuts o = {out[XRS_STAT_SUM], out[XRS_STAT_MAX], out[XRS_STAT_MIN], out[XRS_STAT_RANGE],
                        out[XRS_STAT_MEAN], out[XRS_STAT_VAR], out[XRS_STAT_STD]};
    hipStream_t s = c.s;
    switch (c.mask.R) {
        case 2: return dispatch<2>(g, o, moments, s);
        case 3: return dispatch<3>(g, o, moments, s);
        case 4: return dispatch<4>(g, o, moments, s);
        case 5: return dispatch<5>(g, o, moments, s);
        case 6: return dispatch<6>(g, o, moments, s);
        case 7: return dispatch<7>(g, o, moments, s);
        case 8: return dispatch<8>(g, o, moments, s);
        case 9: return dispatch<9>(g, o, moments, s);
        case 10: return dispatch<10>(g, o, moments, s);
        case 11: return dispatch<11>(g, o, moments, s);
        case 12: return dispatch<12>(g, o, moments, s);
        default: return -1;
    }
}

}  // namespace xrs

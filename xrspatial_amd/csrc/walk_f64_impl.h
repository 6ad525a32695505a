// Float64 statistics (mean, var, std) of focal_stats / focal.apply through the column walker of circle_walk.h, for
// one mask shape (XRS_WALK_SHAPE) and radius 2..12 cells.  Included by kxk_circle64.hip and kxk_box64.hip.
#include "circle_walk.h"

using namespace xrs;

namespace {

template <int R, bool WANT_VAR>
__global__ void __launch_bounds__(256) XRS_WALK_KERNEL(const WalkGeom g, const WalkOuts o) {
    walk_tile<R, XRS_WALK_SHAPE, false, false, false, true, WANT_VAR>(g, o);
}

template <int R>
int launch64(WalkGeom &g, const WalkOuts &o, hipStream_t s) {
    long grid;
    if (int rc = walk_grid(g, &grid)) return rc;
    if (o.var || o.std)
        hipLaunchKernelGGL((XRS_WALK_KERNEL<R, true>), dim3((unsigned)grid), dim3(256), 0, s, g, o);
    else
        hipLaunchKernelGGL((XRS_WALK_KERNEL<R, false>), dim3((unsigned)grid), dim3(256), 0, s, g, o);
    XRS_LAUNCH_CHECK();
    route_note(XRS_STR(XRS_WALK_ENTRY), R);
    return 0;
}

}  // namespace

namespace xrs {

// 0 = launched, -1 = not a circle this file is instantiated for, > 0 = error
int XRS_WALK_ENTRY(const WindowCall &c) {
    if (c.mask.kind != ShapeKind<XRS_WALK_SHAPE>::kind) return -1;
    if (!c.out[XRS_STAT_MEAN] && !c.out[XRS_STAT_VAR] && !c.out[XRS_STAT_STD]) return 0;
    WalkGeom g;
    memset(&g, 0, sizeof(g));
    fill_geom(g, c);
    const WalkOuts o = {nullptr, nullptr, nullptr, nullptr, c.out[XRS_STAT_MEAN], c.out[XRS_STAT_VAR], c.out[XRS_STAT_STD]};
    hipStream_t s = c.s;
    switch (c.mask.R) {
        case 2: return launch64<2>(g, o, s);
        case 3: return launch64<3>(g, o, s);
        case 4: return launch64<4>(g, o, s);
        case 5: return launch64<5>(g, o, s);
        case 6: return launch64<6>(g, o, s);
        case 7: return launch64<7>(g, o, s);
        case 8: return launch64<8>(g, o, s);
        case 9: return launch64<9>(g, o, s);
        case 10: return launch64<10>(g, o, s);
        case 11: return launch64<11>(g, o, s);
        case 12: return launch64<12>(g, o, s);
        default: return -1;
    }
}

}  // namespace xrs

// One record for a focal / convolve_2d window call, as it travels from the C ABI (kxk.hip) to the walkers' translation units:
// the planes and their geometry, the mask as it was recognised ONCE for the call, the pieces of the caller's workspace, the
// stream.  Every walker entry is `int entry(const WindowCall &)`: 0 = launched, -1 = not mine (another shape, a radius the unit is
// not instantiated for, an output set it does not serve), > 0 = error (xrs::fail).  Host code only.
#pragma once
#include "xrs_common.h"

#include <cassert>

namespace xrs {

// Mask shapes the walkers are instantiated for: every row of the (2R+1)^2 mask is ONE run centred on the kernel's
// centre column, with a compile-time half-width hw(R, |dy|).
struct CircleShape {      // circle_kernel on square cells: largest dx with dx^2 + dy^2 <= R^2 (convolution.py:144)
    static constexpr int hw(int R, int dy) {
        int h = 0;
        while ((h + 1) * (h + 1) + dy * dy <= R * R) ++h;
        return h;
    }
    static constexpr int hwi(int, int) { return -1; }      // no hole
};
struct BoxShape {         // np.ones((2R+1, 2R+1))
    static constexpr int hw(int R, int) { return R; }
    static constexpr int hwi(int, int) { return -1; }
};
// annulus_kernel(1, 1, R, RI) = circle_kernel(R) - circle_kernel(RI) (convolution.py:199-259): a row at offset dy is the
// centred run of half-width hw(dy) WITHOUT the centred run of half-width hwi(dy) (-1: no hole in this row) -- two runs,
// but every sum over them is a difference of two centred-run sums, and every extremum one over a "shell" of cell pairs.
constexpr int annulus_hole_hw(int RI, int dy) { return dy <= RI ? CircleShape::hw(RI, dy) : -1; }
template <int RI>
struct AnnulusShape {
    static constexpr int hw(int R, int dy) { return CircleShape::hw(R, dy); }
    static constexpr int hwi(int, int dy) { return annulus_hole_hw(RI, dy); }
};

// What recognise_mask (kxk.hip) found: the one definition of "this mask is that shape", from the row formulas above.
struct WindowMask {
    enum Kind { OTHER, CIRCLE, BOX, ANNULUS };
    Kind kind;
    int R, RI;            // radius = krows / 2 (0 for OTHER); inner radius (ANNULUS only, 1 <= RI < R; else -1)
    double weight;        // the value on the shape's cells: 1.0 for focal statistics, the one weight of a convolve_2d mask
    bool hole_zero;       // ANNULUS: the centre row's hole cells are exactly 0.0, not merely "not selected" (recognise_mask)
};
template <typename Shape> struct ShapeKind;
template <> struct ShapeKind<CircleShape> { static constexpr WindowMask::Kind kind = WindowMask::CIRCLE; };
template <> struct ShapeKind<BoxShape> { static constexpr WindowMask::Kind kind = WindowMask::BOX; };

// The caller's workspace (xrs_focal_workspace_bytes): kernel copy, tile map of the separable box walk (boxsep.hip), work-list
// of the moments / wide kernels' slow wave tiles ([0] count, [2..] tiles; a wave tile is at least 64 columns x 16 rows), and
// behind it the bands the moments rescue launch hands on to the float64 walker's own launch ([0] count, 16-byte entries
// from byte 16 on, read and written as uint4).
struct WorkspaceLayout {
    size_t kernel_off, todo_off, worklist_off, exact_off, bytes;
    size_t worklist_bytes;      // of the work-list region alone
    unsigned exact_cap;         // entries of the band list
};
inline WorkspaceLayout workspace_layout(long rows, long cols, int krows, int kcols) {
    const auto up = [](size_t n, size_t a) { return (n + a - 1) & ~(a - 1); };
    const size_t wave_tiles = (size_t)(cols / 64 + 2) * (size_t)(rows / 16 + 2);
    WorkspaceLayout w;
    w.kernel_off = 0;
    w.todo_off = up((size_t)krows * kcols * sizeof(double), 256);
    w.worklist_off = w.todo_off + up((size_t)(cols / 512 + 2) * (size_t)(rows / 64 + 2), 256);
    w.worklist_bytes = up(256 + 4 * wave_tiles, 16);
    w.exact_off = w.worklist_off + w.worklist_bytes;
    w.exact_cap = (unsigned)(2 * wave_tiles + 8192);
    w.bytes = w.exact_off + 16 + 16 * (size_t)w.exact_cap;
    assert(w.kernel_off % 16 == 0 && w.todo_off % 16 == 0 && w.worklist_off % 16 == 0 && w.exact_off % 16 == 0);
    return w;
}

struct WindowCall {
    const float *in;
    long rows, cols, ld_in, ld_out;
    int halo_top, halo_bot;
    float *out[XRS_NUM_STATS];      // focal statistics, XRS_STAT_* order; NULL = not wanted
    float *out_conv;                // convolve_2d
    const double *weights_dev;      // convolve_2d: the kernel as float64 in device memory
    const double *kernel;           // host, krows x kcols
    int krows, kcols;
    WindowMask mask;
    // pieces of the caller's workspace; NULL when it brought none or too small a one
    unsigned char *box_todo;        // tile map of the separable box walk
    unsigned *worklist;             // work-list of slow wave tiles, `worklist_bytes` long
    size_t worklist_bytes;
    unsigned *exact;                // band list behind it, `exact_cap` entries
    unsigned exact_cap;
    hipStream_t s;
};

// the call with only the statistics of `keep` (bits 1 << XRS_STAT_*) left as outputs
inline WindowCall with_outputs(WindowCall c, unsigned keep) {
    for (int i = 0; i < XRS_NUM_STATS; ++i) if (!(keep >> i & 1)) c.out[i] = nullptr;
    return c;
}

// Walker entries, one per translation unit (kxk_*.hip name theirs with XRS_*_ENTRY).  Each answers -1 outside its own range of
// radii: strip walker 2-3, wide 3-12, extrema and moments 4-12, column walkers 2-12.
typedef int WindowEntryFn(const WindowCall &);
// kxk_runs.hip: prefix-sum mean, and mean / var / std, for large run-structured masks of any shape
WindowEntryFn try_launch_focal_mean_runs, try_launch_focal_meanvar_runs;
// kxk_circle.hip / kxk_box.hip: float32 sum / max / min / range (column walker); with mean / var / std among the outputs all
// seven statistics from one kernel (radius 2, 3 only).  kxk_circle64.hip / kxk_box64.hip: float64 mean / var / std.
WindowEntryFn try_launch_focal_circle_f32, try_launch_focal_box_f32, try_launch_focal_circle_f64, try_launch_focal_box_f64;
// kxk_sw_*.hip (sw_impl.h): any of the seven statistics from one pass of the strip walker
WindowEntryFn try_launch_focal_sw_circle, try_launch_focal_sw_box;
// kxk_wide_*.hip (wide_impl.h): mean and / or sum, float32 on shifted values with a guarded fall-back to the float64 walker;
// convolve_2d with one weight value (out_conv).  The annulus units serve the mean alone or the convolution, exactly one of the two.
WindowEntryFn try_launch_focal_wide_circle, try_launch_focal_wide_box, try_launch_conv_wide_circle, try_launch_conv_wide_box;
WindowEntryFn try_launch_wide_annulus4, try_launch_wide_annulus5, try_launch_wide_annulus6, try_launch_wide_annulus7, try_launch_wide_annulus8,
    try_launch_wide_annulus9, try_launch_wide_annulus10, try_launch_wide_annulus11, try_launch_wide_annulus12;
// kxk_ext_*.hip (ext_impl.h): max / min / range, two input rows per step; annuli in three units by outer radius (4-9, 10-11, 12)
WindowEntryFn try_launch_focal_ext_circle, try_launch_focal_ext_box;
WindowEntryFn try_launch_focal_ext_annulus_a, try_launch_focal_ext_annulus_b, try_launch_focal_ext_annulus_c;
// kxk_mom_*.hip (mom_impl.h): mean / var / std / sum, float32 sums about a shift that trails the walk, guarded; exact float64
// walker for the tiles that fail the guard.  The box unit runs the separable walk of boxsep.hip first when the call has `box_todo`.
WindowEntryFn try_launch_focal_mom_circle, try_launch_focal_mom_box;
WindowEntryFn try_launch_focal_mom_annulus4, try_launch_focal_mom_annulus5, try_launch_focal_mom_annulus6, try_launch_focal_mom_annulus7,
    try_launch_focal_mom_annulus8, try_launch_focal_mom_annulus9, try_launch_focal_mom_annulus10, try_launch_focal_mom_annulus11,
    try_launch_focal_mom_annulus12;

}  // namespace xrs

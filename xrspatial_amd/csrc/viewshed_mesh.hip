// viewshed(method='mesh'): line of sight over the reference's triangle mesh, one bounded ray walk per cell.
//
// Reference: xrspatial/gpu_rtx/viewshed.py and mesh_utils.py -- the raster becomes a triangle mesh, one camera ray per cell
// finds the cell's surface point, and one ray per cell is traced through OptiX from that point towards the observer with
// tmin = 0, tmax = the distance; the cell is visible iff it hits nothing.  Here the result is a rule evaluated per cell, all
// float64 (heights are the reference's float32 vertices, widened):
//   prepare  mesh_walk.h's pass: zv[h, w] = (float)((double)value * scale) and the table of block maxima.
//   walk     per cell (i, j), border rows and columns included: the surface point S under the float32 camera origin
//            (j +- 1e-3, i +- 1e-3: minus on the last column / row) on the triangle of cell (min(i, H - 2), min(j, W - 2)) that
//            holds it, the unit normal n with n_z > 0 there; the same for the viewpoint, recomputed by every thread from four
//            loads; P = S(viewpoint) + (0, 0, observer_elev * scale); the ray from S + n * 1e-3 + (0, 0, target_elev * scale)
//            along (P - S) * (1 / L), L = |P - S|; the verdict "some triangle of the mesh is hit with 0 <= t <= L" by
//            mesh_walk.h's bounded walk.  One thread per cell, a wave on an 8 x 8 patch of a 16 x 16 tile: the rays of a patch
//            converge on one point, so its lanes gather nearly the same cells and end within a few steps of each other.
//   value    -1 where hit; 180 at the viewpoint (no ray); else `_get_vertical_ang` of the UNSCALED heights and the distance in
//            the raster's resolutions, as float32.
// Contraction is off for the whole file: the tests ask for the brute-force evaluation of the rule bit for bit.
#pragma clang fp contract(off)

#include "mesh_walk.h"

namespace {

constexpr int TILE = 16;                       // a workgroup is 16 x 16 cells: four waves of 8 x 8
// the block level the API walks with: 32 x 32 cells (generate_terrain 8192^2, observer 10 above the centre / a corner: 56.3 / 63.6 ms
// against 57.1 / 75.9 with 16 x 16 and 68.2 / 103.7 with 8 x 8; at 4096^2 12.8 / 15.2 against 12.3 / 15.7 and 13.2 / 18.9:
// profiles/viewshed_mesh/viewshed_mesh_bench.txt)
constexpr int BSHIFT_API = BSHIFT_DEFAULT;

struct Surface {
    double x, y, z, nx, ny, nz;
};

// rule 2: the point under the float32 camera origin of cell (i, j), on the triangle that holds it, and the normal there
XRS_HD Surface surface_point(const float *__restrict__ zv, long rows, long cols, long i, long j) {
    Surface s;
    s.x = (double)(float)(j == cols - 1 ? (double)j - EPS : (double)j + EPS);
    s.y = (double)(float)(i == rows - 1 ? (double)i - EPS : (double)i + EPS);
    const long ci = i < rows - 2 ? i : rows - 2, cj = j < cols - 2 ? j : cols - 2;
    const double fx = s.x - (double)cj, fy = s.y - (double)ci;
    const float *__restrict__ p = zv + ci * cols + cj;
    const double C = (double)p[0], D = (double)p[1], A = (double)p[cols], B = (double)p[cols + 1];
    const bool t0 = fy >= fx;
    const double gx = t0 ? B - A : D - C, gy = t0 ? A - C : B - D;
    s.z = C + fx * gx + fy * gy;
    const double len = sqrt(gx * gx + gy * gy + 1.0);
    s.nx = -gx / len, s.ny = -gy / len, s.nz = 1.0 / len;
    return s;
}

// rule 6: `_get_vertical_ang` (gpu_rtx/viewshed.py:58-68)
XRS_HD double vertical_angle(double diff, double dist) {
    if (diff == 0.0) return 90.0;
    if (diff > 0.0) return atan(dist / diff) * 180.0 / 3.141592653589793;
    return atan(-diff / dist) * 180.0 / 3.141592653589793 + 90.0;
}

// rules 2 to 6 for cell (i, j); host and device, so that a CPU build can be held against the brute force
template <typename T, bool COUNT>
XRS_HD float viewshed_cell(const T *__restrict__ z, const float *__restrict__ zv, const float *__restrict__ bmax, long rows, long cols,
                           long blocks_x, int bshift, long i, long j, long vr, long vc, double oe, double te, double oe_scaled,
                           double te_scaled, double ew_res, double ns_res, double zmin, double zmax, unsigned &n_cells,
                           unsigned &n_blocks) {
    if (i == vr && j == vc) return 180.0f;
    const Surface s = surface_point(zv, rows, cols, i, j), v = surface_point(zv, rows, cols, vr, vc);
    const double px = v.x, py = v.y, pz = v.z + oe_scaled;
    const double dx = px - s.x, dy = py - s.y, dz = pz - s.z;
    const double len = sqrt(dx * dx + dy * dy + dz * dz), inv = 1.0 / len;
    Ray ray;
    ray.ox = s.x + s.nx * EPS, ray.oy = s.y + s.ny * EPS, ray.oz = s.z + s.nz * EPS + te_scaled;
    ray.dx = dx * inv, ray.dy = dy * inv, ray.dz = dz * inv, ray.len = len;
    const double slack0 = SLACK * (1.0 + fmax(fabs(zmin), fabs(zmax)));
    if (ray_shadowed<RAY_BOUNDED, COUNT>(zv, bmax, rows, cols, blocks_x, bshift, ray, zmin, zmax, slack0, n_cells, n_blocks)) return -1.0f;
    const double diff = ((double)z[vr * cols + vc] + oe) - ((double)z[i * cols + j] + te);
    const double ry = (double)(vr - i) * ns_res, rx = (double)(vc - j) * ew_res;
    return (float)vertical_angle(diff, sqrt(rx * rx + ry * ry));
}

template <typename T, bool COUNT>
__global__ void __launch_bounds__(TILE * TILE) viewshed_mesh_kernel(const T *__restrict__ z, const float *__restrict__ zv,
                                                                    const float *__restrict__ bmax, long rows, long cols, long tiles_x,
                                                                    long blocks_x, int bshift, long vr, long vc, double oe, double te,
                                                                    double oe_scaled, double te_scaled, double ew_res, double ns_res,
                                                                    double zmin, double zmax, float *__restrict__ out,
                                                                    unsigned long long *__restrict__ counts) {
    const long tile_y = (long)blockIdx.x / tiles_x, tile_x = (long)blockIdx.x - tile_y * tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long i = tile_y * TILE + (wave >> 1) * 8 + (lane >> 3), j = tile_x * TILE + (wave & 1) * 8 + (lane & 7);
    if (i >= rows || j >= cols) return;
    unsigned n_cells = 0, n_blocks = 0;
    out[i * cols + j] = viewshed_cell<T, COUNT>(z, zv, bmax, rows, cols, blocks_x, bshift, i, j, vr, vc, oe, te, oe_scaled, te_scaled,
                                                ew_res, ns_res, zmin, zmax, n_cells, n_blocks);
    if (COUNT) {                                                   // { sum, max } of cells, { sum, max } of blocks
        atomicAdd(counts + 0, (unsigned long long)n_cells);
        atomicMax(counts + 1, (unsigned long long)n_cells);
        atomicAdd(counts + 2, (unsigned long long)n_blocks);
        atomicMax(counts + 3, (unsigned long long)n_blocks);
    }
}

template <typename T>
int viewshed_mesh_impl(const T *z, long rows, long cols, double scale, double zmin, double zmax, long vr, long vc, double oe, double te,
                       double ew_res, double ns_res, int block, void *work, float *out, unsigned long long *counts, hipStream_t s) {
    if (rows < 2 || cols < 2) return fail("xrs_viewshed_mesh: a raster of at least 2 x 2 cells is needed, got %ld x %ld", rows, cols);
    if (rows >= (1L << 30) || cols >= (1L << 30)) return fail("xrs_viewshed_mesh: raster too large (%ld x %ld)", rows, cols);
    if (!z || !work || !out) return fail("xrs_viewshed_mesh: null pointer");
    if (vr < 0 || vr >= rows || vc < 0 || vc >= cols)
        return fail("xrs_viewshed_mesh: the viewpoint (%ld, %ld) is outside the %ld x %ld raster", vr, vc, rows, cols);
    if (!(std::isfinite(scale) && scale > 0.0)) return fail("xrs_viewshed_mesh: scale must be finite and positive");
    if (!(std::isfinite(zmin) && std::isfinite(zmax) && zmin <= zmax))
        return fail("xrs_viewshed_mesh: the height bounds must be finite and ordered");
    if (!(std::isfinite(oe) && std::isfinite(te) && std::isfinite(oe * scale) && std::isfinite(te * scale)))
        return fail("xrs_viewshed_mesh: observer_elev and target_elev must be finite");
    if (!(std::isfinite(ew_res) && std::isfinite(ns_res))) return fail("xrs_viewshed_mesh: the resolutions must be finite");
    int bshift = 0;
    if (block == 8) bshift = 3;
    else if (block == 16) bshift = 4;
    else if (block == 32) bshift = 5;
    else if (block != 0) return fail("xrs_viewshed_mesh: block must be 0 (no block level), 8, 16 or 32, got %d", block);
    const int table_shift = bshift ? bshift : BSHIFT_DEFAULT;      // the plain walk's prepare pass still writes a table
    const long tiles_x = (cols + TILE - 1) / TILE, tiles_y = (rows + TILE - 1) / TILE;
    const long blocks_x = (cols - 1 + (1L << table_shift) - 1) >> table_shift, blocks_y = (rows - 1 + (1L << table_shift) - 1) >> table_shift;
    if (tiles_x * tiles_y >= (1L << 31) || blocks_x * blocks_y >= (1L << 31))
        return fail("xrs_viewshed_mesh: raster too large for one call (%ld x %ld)", rows, cols);
    float *zv = static_cast<float *>(work);
    float *bmax = reinterpret_cast<float *>(static_cast<char *>(work) + up256((size_t)rows * (size_t)cols * sizeof(float)));
    // the vertex heights as the kernels see them: float32 of the scaled bounds (the rounding is monotonic)
    const double vmin = (double)(float)(zmin * scale), vmax = (double)(float)(zmax * scale);
    hipLaunchKernelGGL((shadow_prepare_kernel<T>), dim3((unsigned)(blocks_x * blocks_y)), dim3(256), 0, s, z, rows, cols, scale, table_shift,
                       blocks_x, blocks_y, zv, bmax);
    XRS_LAUNCH_CHECK();
    if (counts)
        hipLaunchKernelGGL((viewshed_mesh_kernel<T, true>), dim3((unsigned)(tiles_x * tiles_y)), dim3(TILE * TILE), 0, s, z, zv, bmax, rows,
                           cols, tiles_x, blocks_x, bshift, vr, vc, oe, te, oe * scale, te * scale, ew_res, ns_res, vmin, vmax, out, counts);
    else
        hipLaunchKernelGGL((viewshed_mesh_kernel<T, false>), dim3((unsigned)(tiles_x * tiles_y)), dim3(TILE * TILE), 0, s, z, zv, bmax, rows,
                           cols, tiles_x, blocks_x, bshift, vr, vc, oe, te, oe * scale, te * scale, ew_res, ns_res, vmin, vmax, out, counts);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t xrs_viewshed_mesh_workspace_bytes(int64_t rows, int64_t cols) { return mesh_workspace_bytes(rows, cols); }

#define XRS_VIEWSHED_MESH(SUF, T)                                                                                                  \
    int xrs_viewshed_mesh_##SUF(const T *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,             \
                                int64_t view_row, int64_t view_col, double observer_elev, double target_elev, double ew_res,       \
                                double ns_res, void *work_dev, float *out_dev, void *stream) {                                     \
        return viewshed_mesh_impl<T>(data_dev, rows, cols, scale, zmin, zmax, view_row, view_col, observer_elev, target_elev,      \
                                     ew_res, ns_res, 1 << BSHIFT_API, work_dev, out_dev, nullptr, as_stream(stream));              \
    }                                                                                                                              \
    int xrs_viewshed_mesh_probe_##SUF(const T *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,       \
                                      int64_t view_row, int64_t view_col, double observer_elev, double target_elev,                \
                                      double ew_res, double ns_res, int block, void *work_dev, float *out_dev,                     \
                                      uint64_t *counts4_dev, void *stream) {                                                       \
        return viewshed_mesh_impl<T>(data_dev, rows, cols, scale, zmin, zmax, view_row, view_col, observer_elev, target_elev,      \
                                     ew_res, ns_res, block, work_dev, out_dev, reinterpret_cast<unsigned long long *>(counts4_dev), \
                                     as_stream(stream));                                                                           \
    }
XRS_VIEWSHED_MESH(f32, float)
XRS_VIEWSHED_MESH(f64, double)

}  // extern "C"

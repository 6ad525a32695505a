// hillshade(shadows=True): cast shadows by one ray walk per cell over the reference's triangle mesh.
//
// Reference: xrspatial/gpu_rtx/hillshade.py and mesh_utils.py -- the raster becomes a triangle mesh, one camera ray per cell
// and one shadow ray towards the sun are traced on NVIDIA RT cores through OptiX, and Lambert's law on the hit triangle's
// normal is halved where the shadow ray hits anything.  The mesh is a height field and every shadow ray has the same direction,
// so here the result is a rule evaluated per cell, all float64 (heights are the reference's float32 vertices, widened):
//   prepare  zv[h, w] = (float)((double)value * scale), and per block of B x B cells the maximum of the (B + 1) x (B + 1)
//            vertices its triangles use.  One workgroup per block.
//   walk     per interior cell (i, j): the point under the float32 camera origin (j + 1e-3, i + 1e-3) on the cell's own
//            triangle, the unit normal n with n_z > 0 there, the origin o = point + n * 1e-3, and the verdict "some triangle of
//            the mesh is hit by o + t * sun with t > 1e-3" by Moller-Trumbore in the order written in tri_hit().  The verdict
//            is an OR over triangles, so any set of triangles that holds every accepted one gives the brute-force verdict:
//            the xy projection of the ray is stepped cell column by cell column along its major axis (blocks first: a block
//            column whose blocks all lie below the ray is jumped over), and a cell's two triangles get the test unless the
//            ray stays above the cell's four corners.  One thread per cell, a wave on an 8 x 8 patch: all rays are parallel,
//            so neighbouring lanes gather neighbouring cells.
//   shade    (sun . n + 1) / 2, halved in shadow, clamped to [0, 1], float32; NaN on the border rows and columns.
// Contraction is off for the whole file: the tests ask for the brute-force evaluation of the rule bit for bit.
// The walk itself, the guard argument that it skips nothing the rule accepts, and the prepare pass are in mesh_walk.h, shared with
// viewshed_mesh.hip; the shadow rays are its unbounded kind (t > 1e-3).
#pragma clang fp contract(off)

#include "mesh_walk.h"

namespace {

constexpr int TILE = 16;                       // a workgroup is 16 x 16 cells: four waves of 8 x 8

// rules 3 to 5 for interior cell (i, j); host and device, so that a CPU build can be held against the brute force
template <bool COUNT>
XRS_HD float shade_cell(const float *__restrict__ zv, const float *__restrict__ bmax, long rows, long cols, long blocks_x, int bshift,
                        long i, long j, double sun_x, double sun_y, double sun_z, double zmin, double zmax, int shadows,
                        unsigned &n_cells, unsigned &n_blocks) {
    // rule 3: the point under the float32 camera origin, on the cell's own triangle
    const double x0 = (double)(float)((double)j + EPS), y0 = (double)(float)((double)i + EPS);
    const double fx = x0 - (double)j, fy = y0 - (double)i;
    const float *__restrict__ p = zv + i * cols + j;
    const double C = (double)p[0], D = (double)p[1], A = (double)p[cols], B = (double)p[cols + 1];
    const bool t0 = fy >= fx;
    const double gx = t0 ? B - A : D - C, gy = t0 ? A - C : B - D;
    const double zh = C + fx * gx + fy * gy;
    const double len = sqrt(gx * gx + gy * gy + 1.0);
    const double nx = -gx / len, ny = -gy / len, nz = 1.0 / len;
    bool shadow = false;
    if (shadows) {
        Ray ray;
        ray.ox = x0 + nx * EPS, ray.oy = y0 + ny * EPS, ray.oz = zh + nz * EPS;
        ray.dx = sun_x, ray.dy = sun_y, ray.dz = sun_z, ray.len = 0.0;
        const double slack0 = SLACK * (1.0 + fmax(fabs(zmin), fabs(zmax)));
        shadow = ray_shadowed<RAY_UNBOUNDED, COUNT>(zv, bmax, rows, cols, blocks_x, bshift, ray, zmin, zmax, slack0, n_cells, n_blocks);
    }
    // rule 5
    double temp = (sun_x * nx + sun_y * ny + sun_z * nz + 1.0) / 2.0;
    if (shadow) temp = temp / 2.0;
    if (temp > 1.0) temp = 1.0;
    else if (temp < 0.0) temp = 0.0;
    return (float)temp;
}

template <bool COUNT>
__global__ void __launch_bounds__(TILE * TILE) shadow_walk_kernel(const float *__restrict__ zv, const float *__restrict__ bmax, long rows,
                                                                  long cols, long tiles_x, long blocks_x, int bshift, double sun_x,
                                                                  double sun_y, double sun_z, double zmin, double zmax, int shadows,
                                                                  float *__restrict__ out, unsigned long long *__restrict__ counts) {
    const long tile_y = (long)blockIdx.x / tiles_x, tile_x = (long)blockIdx.x - tile_y * tiles_x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long i = tile_y * TILE + (wave >> 1) * 8 + (lane >> 3), j = tile_x * TILE + (wave & 1) * 8 + (lane & 7);
    if (i >= rows || j >= cols) return;
    if (i == 0 || j == 0 || i == rows - 1 || j == cols - 1) {
        out[i * cols + j] = nan_f32();
        return;
    }
    unsigned n_cells = 0, n_blocks = 0;
    out[i * cols + j] = shade_cell<COUNT>(zv, bmax, rows, cols, blocks_x, bshift, i, j, sun_x, sun_y, sun_z, zmin, zmax, shadows, n_cells,
                                          n_blocks);
    if (COUNT && shadows) {                                        // { sum, max } of cells, { sum, max } of blocks
        atomicAdd(counts + 0, (unsigned long long)n_cells);
        atomicMax(counts + 1, (unsigned long long)n_cells);
        atomicAdd(counts + 2, (unsigned long long)n_blocks);
        atomicMax(counts + 3, (unsigned long long)n_blocks);
    }
}

template <typename T>
int shadow_impl(const T *z, long rows, long cols, double scale, double zmin, double zmax, double sun_x, double sun_y, double sun_z,
                int shadows, int block, void *work, float *out, unsigned long long *counts, hipStream_t s) {
    if (rows < 1 || cols < 1) return fail("xrs_hillshade_shadow: a raster of at least 1 x 1 cells is needed, got %ld x %ld", rows, cols);
    if (rows >= (1L << 30) || cols >= (1L << 30)) return fail("xrs_hillshade_shadow: raster too large (%ld x %ld)", rows, cols);
    if (!z || !work || !out) return fail("xrs_hillshade_shadow: null pointer");
    if (!(std::isfinite(scale) && scale > 0.0)) return fail("xrs_hillshade_shadow: scale must be finite and positive");
    if (!(std::isfinite(zmin) && std::isfinite(zmax) && zmin <= zmax))
        return fail("xrs_hillshade_shadow: the height bounds must be finite and ordered");
    if (!(std::isfinite(sun_x) && std::isfinite(sun_y) && std::isfinite(sun_z)) || (sun_x == 0.0 && sun_y == 0.0 && sun_z == 0.0))
        return fail("xrs_hillshade_shadow: the sun vector must be finite and non-zero");
    int bshift = 0;
    if (block == 8) bshift = 3;
    else if (block == 16) bshift = 4;
    else if (block == 32) bshift = 5;
    else if (block != 0) return fail("xrs_hillshade_shadow: block must be 0 (no block level), 8, 16 or 32, got %d", block);
    const int table_shift = bshift ? bshift : BSHIFT_DEFAULT;      // the plain walk's prepare pass still writes a table
    const long tiles_x = (cols + TILE - 1) / TILE, tiles_y = (rows + TILE - 1) / TILE;
    const long blocks_x = (cols - 1 + (1L << table_shift) - 1) >> table_shift, blocks_y = (rows - 1 + (1L << table_shift) - 1) >> table_shift;
    if (tiles_x * tiles_y >= (1L << 31) || blocks_x * blocks_y >= (1L << 31))
        return fail("xrs_hillshade_shadow: raster too large for one call (%ld x %ld)", rows, cols);
    float *zv = static_cast<float *>(work);
    float *bmax = reinterpret_cast<float *>(static_cast<char *>(work) + up256((size_t)rows * (size_t)cols * sizeof(float)));
    // the vertex heights as the kernels see them: float32 of the scaled bounds (the rounding is monotonic)
    const double vmin = (double)(float)(zmin * scale), vmax = (double)(float)(zmax * scale);
    if (rows >= 3 && cols >= 3) {                                  // (else every cell is a border cell and no height is read)
        hipLaunchKernelGGL((shadow_prepare_kernel<T>), dim3((unsigned)(blocks_x * blocks_y)), dim3(256), 0, s, z, rows, cols, scale,
                           table_shift, blocks_x, blocks_y, zv, bmax);
        XRS_LAUNCH_CHECK();
    }
    if (counts)
        hipLaunchKernelGGL((shadow_walk_kernel<true>), dim3((unsigned)(tiles_x * tiles_y)), dim3(TILE * TILE), 0, s, zv, bmax, rows, cols,
                           tiles_x, blocks_x, bshift, sun_x, sun_y, sun_z, vmin, vmax, shadows, out, counts);
    else
        hipLaunchKernelGGL((shadow_walk_kernel<false>), dim3((unsigned)(tiles_x * tiles_y)), dim3(TILE * TILE), 0, s, zv, bmax, rows, cols,
                           tiles_x, blocks_x, bshift, sun_x, sun_y, sun_z, vmin, vmax, shadows, out, counts);
    XRS_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

size_t xrs_hillshade_shadow_workspace_bytes(int64_t rows, int64_t cols) {
    return mesh_workspace_bytes(rows, cols);
}

#define XRS_HILLSHADE_SHADOW(SUF, T)                                                                                               \
    int xrs_hillshade_shadow_##SUF(const T *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,          \
                                   double sun_x, double sun_y, double sun_z, int shadows, void *work_dev, float *out_dev,          \
                                   void *stream) {                                                                                 \
        return shadow_impl<T>(data_dev, rows, cols, scale, zmin, zmax, sun_x, sun_y, sun_z, shadows, 1 << BSHIFT_DEFAULT, work_dev, \
                              out_dev, nullptr, as_stream(stream));                                                                \
    }                                                                                                                              \
    int xrs_hillshade_shadow_probe_##SUF(const T *data_dev, int64_t rows, int64_t cols, double scale, double zmin, double zmax,    \
                                         double sun_x, double sun_y, double sun_z, int block, void *work_dev, float *out_dev,      \
                                         uint64_t *counts4_dev, void *stream) {                                                    \
        return shadow_impl<T>(data_dev, rows, cols, scale, zmin, zmax, sun_x, sun_y, sun_z, 1, block, work_dev, out_dev,           \
                              reinterpret_cast<unsigned long long *>(counts4_dev), as_stream(stream));                             \
    }
XRS_HILLSHADE_SHADOW(f32, float)
XRS_HILLSHADE_SHADOW(f64, double)

}  // extern "C"

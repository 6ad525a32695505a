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
//
// Why the walk skips nothing the rule accepts.  A triangle's barycentric u, v are, up to sign and offset, the x and y of the hit
// point inside its cell, whatever t is.  If the projected ray (run backwards by GUARD as well) stays GUARD = 2^-10 cells clear
// of a cell's square, the exact u, v or u + v of both its triangles violate their bound by GUARD for every t; the rule's own u,
// v carry the relative rounding error of three float64 sums over det's, a few 2^-53 of the sums' terms over |det|, so the
// rule rejects such a triangle as long as |det| is not smaller than 2^-40 of its own terms (a sun ray within 1e-12 rad of a
// face's plane; below that the rule's quotients are noise and no cover short of every triangle is a proof).  The walk's own
// coordinates are float64 of magnitude < 2^30, good to 2^-22, far inside GUARD.  The height rejects compare the ray's lowest
// z over the GUARD-widened crossing with the largest vertex: an accepted hit lies on the ray and on the triangle's plane at
// barycentrics within the error above of [0, 1], so at most that error times the triangle's height range above its highest
// vertex; the ray's z is two roundings of magnitudes below |oz| + |z|.  SLACK = 2^-20 of (1 + the largest |height| + |z|)
// covers both with thirty bits to spare and costs nothing measurable: it only widens what is tested.
#include "xrs_common.h"
#include "wave_reduce.h"

#include <cmath>

#pragma clang fp contract(off)

using namespace xrs;

namespace {

#define XRS_HD __host__ __device__ __forceinline__

constexpr int TILE = 16;                       // a workgroup is 16 x 16 cells: four waves of 8 x 8
constexpr double EPS = 1e-3;                   // the reference's origin offsets and tmin
constexpr double GUARD = 0.0009765625;         // 2^-10 cells
constexpr double SLACK = 9.5367431640625e-07;  // 2^-20
// tables over 8 x 8 cells are the largest; the API walks with 32 x 32 (8192^2 terrain, sun at 60 / 25 / 5 degrees: 35.9 / 34.7 /
// 33.6 ms against 39.8 / 35.6 / 33.9 with 16 x 16 and 56.7 / 45.5 / 41.7 with 8 x 8: profiles/hillshade_shadows/block_size_trial.txt)
constexpr int BSHIFT_MIN = 3, BSHIFT_DEFAULT = 5;

// ---------------------------------------------------------------------------------------------------------------- prepare
template <typename T>
__global__ void __launch_bounds__(256) shadow_prepare_kernel(const T *__restrict__ z, long rows, long cols, double scale, int bshift,
                                                            long blocks_x, long blocks_y, float *__restrict__ zv,
                                                            float *__restrict__ bmax) {
    __shared__ float part[4];
    const long by = (long)blockIdx.x / blocks_x, bx = (long)blockIdx.x - by * blocks_x;
    const int B = 1 << bshift, side = B + 1;
    const long r0 = by << bshift, c0 = bx << bshift;
    const bool last_y = by == blocks_y - 1, last_x = bx == blocks_x - 1;    // the last blocks own their far vertex row / column
    float m = -INFINITY;
    for (int i = threadIdx.x; i < side * side; i += 256) {
        const int rr = i / side, cc = i - rr * side;
        const long r = r0 + rr, c = c0 + cc;
        if (r >= rows || c >= cols) continue;
        const float v = (float)((double)z[r * cols + c] * scale);
        m = fmaxf(m, v);
        if ((rr < B || last_y) && (cc < B || last_x)) zv[r * cols + c] = v;
    }
    m = wave_reduce<WrMax>(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) bmax[blockIdx.x] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

// ------------------------------------------------------------------------------------------------------------------- walk
// rule 4, in its order: e1, e2, p = d x e2, det = e1 . p, s = o - v0, u, q = s x e1, v, t; sums left to right.  The early
// returns change no verdict: every condition is one of the rule's conjuncts (a NaN quotient fails its comparison here as there).
XRS_HD bool tri_hit(double ox, double oy, double oz, double dx, double dy, double dz, double v0x, double v0y,
                                        double v0z, double v1x, double v1y, double v1z, double v2x, double v2y, double v2z) {
    const double e1x = v1x - v0x, e1y = v1y - v0y, e1z = v1z - v0z;
    const double e2x = v2x - v0x, e2y = v2y - v0y, e2z = v2z - v0z;
    const double px = dy * e2z - dz * e2y, py = dz * e2x - dx * e2z, pz = dx * e2y - dy * e2x;
    const double det = e1x * px + e1y * py + e1z * pz;
    if (det == 0.0) return false;
    const double sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
    const double u = (sx * px + sy * py + sz * pz) / det;
    if (!(u >= 0.0)) return false;
    const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    const double v = (dx * qx + dy * qy + dz * qz) / det;
    if (!(v >= 0.0) || !(u + v <= 1.0)) return false;
    const double t = (e2x * qx + e2y * qy + e2z * qz) / det;
    return t > EPS;
}

struct Ray {
    double ox, oy, oz, dx, dy, dz;
};

// the two triangles of cell (r, c) against the ray, unless the ray's lowest height over the cell clears its corners
XRS_HD bool cell_hit(const float *__restrict__ zv, long cols, long r, long c, const Ray &ray, double zlo,
                                         double slack0) {
    const float *__restrict__ p = zv + r * cols + c;
    const double C = (double)p[0], D = (double)p[1], A = (double)p[cols], B = (double)p[cols + 1];
    if (zlo - fmax(fmax(C, D), fmax(A, B)) > slack0 + SLACK * fabs(zlo)) return false;
    const double x = (double)c, y = (double)r, x1 = (double)(c + 1), y1 = (double)(r + 1);
    // T0 = [(r + 1, c), (r + 1, c + 1), (r, c)], T1 = [(r + 1, c + 1), (r, c + 1), (r, c)]
    return tri_hit(ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, x, y1, A, x1, y1, B, x, y, C) ||
           tri_hit(ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, x1, y1, B, x1, y, D, x, y, C);
}

XRS_HD long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the verdict of rule 4 for one ray.  bshift = 0: the plain cell walk; else blocks of 2^bshift cells are tested first.
// counts (COUNT only): cells visited (corners loaded) and blocks tested by this ray.
template <bool COUNT>
XRS_HD bool ray_shadowed(const float *__restrict__ zv, const float *__restrict__ bmax, long rows, long cols,
                                             long blocks_x, int bshift, const Ray &ray, double zmin, double zmax, double slack0,
                                             unsigned &n_cells, unsigned &n_blocks) {
    const long ncx = cols - 1, ncy = rows - 1;                     // cells along x and y
    if (ray.dx == 0.0 && ray.dy == 0.0) {                          // a vertical projection: the cells around the origin
        const long c_lo = clampl((long)floor(ray.ox - GUARD), 0, ncx - 1), c_hi = clampl((long)floor(ray.ox + GUARD), 0, ncx - 1);
        const long r_lo = clampl((long)floor(ray.oy - GUARD), 0, ncy - 1), r_hi = clampl((long)floor(ray.oy + GUARD), 0, ncy - 1);
        const double zlo = ray.dz >= 0.0 ? ray.oz : -INFINITY;
        for (long r = r_lo; r <= r_hi; ++r)                        // at most 2 x 2 cells
            for (long c = c_lo; c <= c_hi; ++c) {
                if (COUNT) ++n_cells;
                if (cell_hit(zv, cols, r, c, ray, zlo, slack0)) return true;
            }
        return false;
    }
    // m: the major axis of the projection, n: the minor one; |slope| <= 1
    const bool by_x = fabs(ray.dx) >= fabs(ray.dy);
    const double dm = by_x ? ray.dx : ray.dy, dn = by_x ? ray.dy : ray.dx;
    const double om = by_x ? ray.ox : ray.oy, on = by_x ? ray.oy : ray.ox;
    const long nm = by_x ? ncx : ncy, nn = by_x ? ncy : ncx;
    const int sg = dm > 0.0 ? 1 : -1;
    const double slope = dn / dm, zs = ray.dz / dm;                // per unit of m
    const bool rising = ray.dz >= 0.0, falling = ray.dz <= 0.0;
    long c = clampl((long)floor(om - sg * GUARD), 0, nm - 1);
    long blk = -1, b_lo = 0;                                       // the block column being crossed, its first block row
    unsigned mask = 7u;                                            // which of block rows b_lo .. b_lo + 2 the ray may hit
    for (long it = 0; it < nm && c >= 0 && c < nm; ++it) {         // every turn leaves at least one cell column behind
        if (bshift && (c >> bshift) != blk) {                      // entering a block column
            blk = c >> bshift;
            const long first = blk << bshift, past = first + (1L << bshift) < nm ? first + (1L << bshift) : nm;
            const double lo = (double)first - GUARD, hi = (double)past + GUARD;
            double da = (sg > 0 ? lo : hi) - om;
            const double db = (sg > 0 ? hi : lo) - om;
            const double na = on + da * slope, nb = on + db * slope;
            if (da * sg < 0.0) da = 0.0;                           // the ray starts at t = 0
            const double za = ray.oz + da * zs, zb = ray.oz + db * zs, zlo = rising ? za : zb;
            const long r_lo = (long)floor(fmin(na, nb) - GUARD), r_hi = (long)floor(fmax(na, nb) + GUARD);
            mask = 0u;
            if (r_hi >= 0 && r_lo < nn) {
                b_lo = clampl(r_lo, 0, nn - 1) >> bshift;
                const long b_hi = clampl(r_hi, 0, nn - 1) >> bshift;
                for (long b = b_lo; b <= b_hi && b <= b_lo + 2; ++b) {
                    if (COUNT) ++n_blocks;
                    const double top = (double)bmax[by_x ? b * blocks_x + blk : blk * blocks_x + b];
                    if (!(zlo - top > slack0 + SLACK * fabs(zlo))) mask |= 1u << (b - b_lo);
                }
            }
            if (mask == 0u) {                                      // nothing to hit in this block column: over it in one step
                if ((rising && za > zmax + (slack0 + SLACK * fabs(za))) || (falling && za < zmin - (slack0 + SLACK * fabs(za)))) break;
                if (r_hi < 0 || r_lo >= nn) break;                 // the projection has left the grid
                c = sg > 0 ? past : first - 1;
                continue;
            }
        }
        const double lo = (double)c - GUARD, hi = (double)(c + 1) + GUARD;
        double da = (sg > 0 ? lo : hi) - om;
        const double db = (sg > 0 ? hi : lo) - om;
        const double na = on + da * slope, nb = on + db * slope;
        if (da * sg < 0.0) da = 0.0;
        const double za = ray.oz + da * zs, zb = ray.oz + db * zs, zlo = rising ? za : zb;
        // from here on the ray only rises above every vertex, or only falls below every vertex
        if ((rising && za > zmax + (slack0 + SLACK * fabs(za))) || (falling && za < zmin - (slack0 + SLACK * fabs(za)))) break;
        const long r_lo = (long)floor(fmin(na, nb) - GUARD), r_hi = (long)floor(fmax(na, nb) + GUARD);
        if (r_hi < 0 || r_lo >= nn) break;                         // the projection has left the grid
        const long r_a = r_lo < 0 ? 0 : r_lo, r_b = r_hi > nn - 1 ? nn - 1 : r_hi;
        for (long r = r_a; r <= r_b && r <= r_a + 2; ++r) {        // |slope| <= 1: at most three cells of this column
            if (bshift) {
                const long k = (r >> bshift) - b_lo;
                if (k >= 0 && k <= 2 && !((mask >> k) & 1u)) continue;
            }
            if (COUNT) ++n_cells;
            if (cell_hit(zv, cols, by_x ? r : c, by_x ? c : r, ray, zlo, slack0)) return true;
        }
        c += sg;
    }
    return false;
}

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
        ray.dx = sun_x, ray.dy = sun_y, ray.dz = sun_z;
        const double slack0 = SLACK * (1.0 + fmax(fabs(zmin), fabs(zmax)));
        shadow = ray_shadowed<COUNT>(zv, bmax, rows, cols, blocks_x, bshift, ray, zmin, zmax, slack0, n_cells, n_blocks);
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

size_t table_cells(long rows, long cols, int bshift) {
    const long by = (rows - 1 + (1L << bshift) - 1) >> bshift, bx = (cols - 1 + (1L << bshift) - 1) >> bshift;
    return (size_t)(by > 0 ? by : 0) * (size_t)(bx > 0 ? bx : 0);
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

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
    float *bmax = reinterpret_cast<float *>(static_cast<char *>(work) + align256((size_t)rows * (size_t)cols * sizeof(float)));
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
    if (rows < 1 || cols < 1) return 0;
    return align256((size_t)rows * (size_t)cols * sizeof(float)) + align256((table_cells(rows, cols, BSHIFT_MIN) + 1) * sizeof(float));
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

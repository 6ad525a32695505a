// One ray walk over the reference's triangle mesh: the float32 vertex heights and the table of block
// maxima (prepare), Moller-Trumbore in the rule's order, and the guarded walk over cell columns and block columns that decides
// "some triangle of the mesh is hit by o + t * d" for one ray.  Shared by hillshade_shadow.hip (parallel, unbounded shadow
// rays: t > 1e-3) and viewshed_mesh.hip (rays that converge on the observer and end there: 0 <= t <= L); the ray kind is a
// compile-time parameter, and the unbounded form is the code hillshade_shadow.hip held before, instruction for instruction.
// Everything here has internal linkage: each translation unit that includes this header gets its own kernels.
// Contraction must be off in the including file (#pragma clang fp contract(off) before the include).
//
// Why the walk skips nothing the rule accepts.  A triangle's barycentric u, v are, up to sign and offset, the x and y of the hit
// point inside its cell, whatever t is.  If the projected ray (run backwards by GUARD as well) stays GUARD = 2^-10 cells clear
// of a cell's square, the exact u, v or u + v of both its triangles violate their bound by GUARD for every t; the rule's own u,
// v carry the relative rounding error of three float64 sums over det's, a few 2^-53 of the sums' terms over |det|, so the
// rule rejects such a triangle as long as |det| is not smaller than 2^-40 of its own terms (a ray within 1e-12 rad of a
// face's plane; below that the rule's quotients are noise and no cover short of every triangle is a proof).  The walk's own
// coordinates are float64 of magnitude < 2^30, good to 2^-22, far inside GUARD.  The height rejects compare the ray's lowest
// z over the GUARD-widened crossing with the largest vertex: an accepted hit lies on the ray and on the triangle's plane at
// barycentrics within the error above of [0, 1], so at most that error times the triangle's height range above its highest
// vertex; the ray's z is two roundings of magnitudes below |oz| + |z|.  SLACK = 2^-20 of (1 + the largest |height| + |z|)
// covers both with thirty bits to spare and costs nothing measurable: it only widens what is tested.
//
// The bounded form (a unit direction, 0 <= t <= L) adds one stop and one clip.  An accepted hit has the rule's t in [0, L]; the
// exact t of that hit point differs from it by the same relative error as u and v (one more quotient of a three-term sum over
// the same det), and the hit point's major coordinate is om + dm * t with |dm| <= 1, so it lies inside the projected segment
// [om, om + dm * L] widened by that error at both ends -- under the premise on |det| above less than GUARD, the margin the walk
// already keeps behind the origin.  So a cell column that begins more than GUARD past om + dm * L holds no accepted hit and
// the walk ends there, a block column likewise; and inside the last column the ray's z interval is taken over the segment
// widened by GUARD instead of over the whole crossing, which the SLACK argument covers unchanged (the z of the widened end is
// one more rounding of the same magnitudes).  t = 0 itself is accepted now: the walk starts GUARD behind the origin and takes
// the origin's own z for that stretch, and a hit whose rule t is >= 0 has an exact t above minus the error, a z difference of
// |dz| times that error, inside SLACK.  The exits stay: the projection leaves the grid, the ray is above the global maximum
// and rising or below the global minimum and falling.  Every loop is bounded by max(H, W) - 1 turns.
#pragma once

#include "xrs_common.h"
#include "wave_reduce.h"
#include "workspace.h"

#include <cmath>

namespace {

using namespace xrs;

#define XRS_HD __host__ __device__ __forceinline__

constexpr double EPS = 1e-3;                   // the reference's origin offsets and the shadow rays' tmin
constexpr double GUARD = 0.0009765625;         // 2^-10 cells
constexpr double SLACK = 9.5367431640625e-07;  // 2^-20
// tables over 8 x 8 cells are the largest; hillshade walks with 32 x 32 (8192^2 terrain, sun at 60 / 25 / 5 degrees: 35.9 / 34.7 /
// 33.6 ms against 39.8 / 35.6 / 33.9 with 16 x 16 and 56.7 / 45.5 / 41.7 with 8 x 8: profiles/hillshade_shadows/block_size_trial.txt)
constexpr int BSHIFT_MIN = 3, BSHIFT_DEFAULT = 5;

enum RayKind { RAY_UNBOUNDED = 0,              // accepted: t > 1e-3 (a shadow ray; `len` is not read)
               RAY_BOUNDED = 1 };              // accepted: 0 <= t <= len, the direction a unit vector (a sight line)

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
// §6i rule 4, in its order: e1, e2, p = d x e2, det = e1 . p, s = o - v0, u, q = s x e1, v, t; sums left to right.  The early
// returns change no verdict: every condition is one of the rule's conjuncts (a NaN quotient fails its comparison here as there).
template <RayKind KIND>
XRS_HD bool tri_hit(double ox, double oy, double oz, double dx, double dy, double dz, double len, double v0x, double v0y,
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
    if (KIND == RAY_BOUNDED) return t >= 0.0 && t <= len;
    return t > EPS;
}

struct Ray {
    double ox, oy, oz, dx, dy, dz;
    double len;                                // RAY_BOUNDED only
};

// the two triangles of cell (r, c) against the ray, unless the ray's lowest height over the cell clears its corners
template <RayKind KIND>
XRS_HD bool cell_hit(const float *__restrict__ zv, long cols, long r, long c, const Ray &ray, double zlo, double slack0) {
    const float *__restrict__ p = zv + r * cols + c;
    const double C = (double)p[0], D = (double)p[1], A = (double)p[cols], B = (double)p[cols + 1];
    if (zlo - fmax(fmax(C, D), fmax(A, B)) > slack0 + SLACK * fabs(zlo)) return false;
    const double x = (double)c, y = (double)r, x1 = (double)(c + 1), y1 = (double)(r + 1);
    // T0 = [(r + 1, c), (r + 1, c + 1), (r, c)], T1 = [(r + 1, c + 1), (r, c + 1), (r, c)]
    return tri_hit<KIND>(ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, ray.len, x, y1, A, x1, y1, B, x, y, C) ||
           tri_hit<KIND>(ray.ox, ray.oy, ray.oz, ray.dx, ray.dy, ray.dz, ray.len, x1, y1, B, x1, y, D, x, y, C);
}

XRS_HD long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the verdict for one ray: is any triangle of the mesh hit.  bshift = 0: the plain cell walk; else blocks of 2^bshift cells
// are tested first.  counts (COUNT only): cells visited (corners loaded) and blocks tested by this ray.
template <RayKind KIND, bool COUNT>
XRS_HD bool ray_shadowed(const float *__restrict__ zv, const float *__restrict__ bmax, long rows, long cols, long blocks_x, int bshift,
                         const Ray &ray, double zmin, double zmax, double slack0, unsigned &n_cells, unsigned &n_blocks) {
    const long ncx = cols - 1, ncy = rows - 1;                     // cells along x and y
    if (ray.dx == 0.0 && ray.dy == 0.0) {                          // a vertical projection: the cells around the origin
        const long c_lo = clampl((long)floor(ray.ox - GUARD), 0, ncx - 1), c_hi = clampl((long)floor(ray.ox + GUARD), 0, ncx - 1);
        const long r_lo = clampl((long)floor(ray.oy - GUARD), 0, ncy - 1), r_hi = clampl((long)floor(ray.oy + GUARD), 0, ncy - 1);
        const double zlo = ray.dz >= 0.0 ? ray.oz : -INFINITY;
        for (long r = r_lo; r <= r_hi; ++r)                        // at most 2 x 2 cells
            for (long c = c_lo; c <= c_hi; ++c) {
                if (COUNT) ++n_cells;
                if (cell_hit<KIND>(zv, cols, r, c, ray, zlo, slack0)) return true;
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
    // RAY_BOUNDED: how far along m, from om, a hit can lie (the segment's end and GUARD past it), as sg * distance >= 0
    const double reach = KIND == RAY_BOUNDED ? fabs(dm) * ray.len + GUARD : 0.0;
    long c = clampl((long)floor(om - sg * GUARD), 0, nm - 1);
    long blk = -1, b_lo = 0;                                       // the block column being crossed, its first block row
    unsigned mask = 7u;                                            // which of block rows b_lo .. b_lo + 2 the ray may hit
    for (long it = 0; it < nm && c >= 0 && c < nm; ++it) {         // every turn leaves at least one cell column behind
        if (bshift && (c >> bshift) != blk) {                      // entering a block column
            blk = c >> bshift;
            const long first = blk << bshift, past = first + (1L << bshift) < nm ? first + (1L << bshift) : nm;
            const double lo = (double)first - GUARD, hi = (double)past + GUARD;
            double da = (sg > 0 ? lo : hi) - om;
            double db = (sg > 0 ? hi : lo) - om;
            const double na = on + da * slope, nb = on + db * slope;
            if (da * sg < 0.0) da = 0.0;                           // the ray starts at t = 0
            if (KIND == RAY_BOUNDED) {
                if (da * sg > reach) break;                        // the segment ends before this block column
                if (db * sg > reach) db = sg * reach;
            }
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
        double db = (sg > 0 ? hi : lo) - om;
        const double na = on + da * slope, nb = on + db * slope;
        if (da * sg < 0.0) da = 0.0;
        if (KIND == RAY_BOUNDED) {
            if (da * sg > reach) break;                            // the segment ends before this cell column
            if (db * sg > reach) db = sg * reach;
        }
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
            if (cell_hit<KIND>(zv, cols, by_x ? r : c, by_x ? c : r, ray, zlo, slack0)) return true;
        }
        c += sg;
    }
    return false;
}

// ---------------------------------------------------------------------------------------------------------- the workspace
size_t table_cells(long rows, long cols, int bshift) {
    const long by = (rows - 1 + (1L << bshift) - 1) >> bshift, bx = (cols - 1 + (1L << bshift) - 1) >> bshift;
    return (size_t)(by > 0 ? by : 0) * (size_t)(bx > 0 ? bx : 0);
}

// the float32 vertex heights, then the largest table of block maxima
size_t mesh_workspace_bytes(long rows, long cols) {
    if (rows < 1 || cols < 1) return 0;
    return up256((size_t)rows * (size_t)cols * sizeof(float)) + up256((table_cells(rows, cols, BSHIFT_MIN) + 1) * sizeof(float));
}

}  // namespace

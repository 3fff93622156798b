/* dexr_mesh_sdf.h -- signed distances of points, or of a whole regular grid of samples, to ONE triangle mesh: the stage in front of
 * dexr_sdf_grid.h, which turns an object model into the samples that a signed-distance grid is made of.  C ABI.  Brute force: every
 * point meets every triangle, the cost is points x triangles pairs and nothing is culled; one kernel, in float32 and in float64.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; P == 0 is a no-op returning 0.  Everything is validated before the first HIP call.  The library reads
 * no environment variable.
 *
 * THE MESH.  V vertices (V, 3) float64 and T triangles (T, 3) int32 of vertex indices, corners a_t, b_t, c_t.  At creation every
 * triangle becomes one record, computed in float64 and kept on the device in float64 and rounded to float32:
 *
 *   a,   ab = b - a,   ac = c - a
 *
 * DEFINITION.  For a point p, in the arithmetic type of the kernel, per triangle t with ap = p - a:
 *
 *   d1 = ab.ap   d2 = ac.ap   d3 = ab.(ap - ab)   d4 = ac.(ap - ab)   d5 = ab.(ap - ac)   d6 = ac.(ap - ac)
 *   vc = d1 d4 - d3 d2      vb = d5 d2 - d1 d6      va = d3 d6 - d5 d4
 *
 * and the closest point of the triangle is a + v ab + w ac, with (v, w) from the FIRST of these seven regions, in this order, whose
 * test holds:
 *
 *   1 vertex a   d1 <= 0 and d2 <= 0                          v = 0                 w = 0
 *   2 vertex b   d3 >= 0 and d4 <= d3                         v = 1                 w = 0
 *   3 edge ab    vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3)    w = 0
 *   4 vertex c   d6 >= 0 and d5 <= d6                         v = 0                 w = 1
 *   5 edge ac    vb <= 0 and d2 >= 0 and d6 <= 0              v = 0                 w = d2 / (d2 - d6)
 *   6 edge bc    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),  v = 1 - w
 *   7 face       otherwise                                    v = vb / (va + vb + vc)   w = vc / (va + vb + vc)
 *
 *   e_t = ap - v ab - w ac,      u(p) = sqrt(min_t e_t.e_t)
 *
 * This is the exact closest point of a triangle (vertex / edge / face), not a projection onto its plane.  The minimum is taken with
 * `candidate < best`: among equal distances the earlier triangle stands, a candidate that is a NaN never wins.
 *
 * THE SIGN is that of the generalised winding number.  With A = a - p, B = A + ab, C = A + ac and their lengths:
 *
 *   Omega_t = 2 atan2(A.(B x C),  |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|)        the solid angle of triangle t seen from p
 *   w(p)    = (1 / 4 pi) sum_t Omega_t
 *   sdf(p)  = w(p) >= 0.5 ? -u(p) : u(p)
 *
 * Each Omega_t is evaluated in the kernel's arithmetic type; the sum is accumulated in float64, in triangle order, in both
 * precisions, and compared with 0.5 as a float64.  For a closed mesh whose triangles are oriented with their normals (b - a) x (c - a)
 * pointing outwards, w is 0 outside and 1 inside (and 1/2 on the surface, where u = 0).  A mesh that is inside out gives 0 and -1:
 * every sample positive.  An open mesh gives a fractional w, and the sign is only a majority vote of the triangles' solid angles:
 * it degrades smoothly around a hole where a ray count would flip along whole rays.  Nothing is preprocessed: no adjacency, no
 * pseudonormals.  Neither the nearest triangle (ties make it ambiguous) nor a gradient (the grid's interpolant supplies one) is
 * returned.
 *
 * EVERY entry of every output is written.  A point with a coordinate that is a NaN or infinite gives a NaN in its own entry of
 * both outputs and touches no other entry.  A point's result is produced by one thread that walks all triangles in table order:
 * there are no atomics and no sums across threads, so that its bits do not depend on P, on where the point sits in the batch, or
 * on whether it came from an array or was generated as a grid sample.
 *
 * THE GRID entry points evaluate sample (ix, iy, iz) of n = (nx, ny, nz) samples in C order (iz the fastest) at
 * origin + (ix, iy, iz) * spacing, the product and the sum each rounded once in float64 (no fused multiply-add), and in the
 * float32 kernel the result rounded once to float32.  The rules for n, origin and spacing are those of dexr_sdf_grid.h, by its
 * macros DEXR_SDF_GRID_MIN_DIM, DEXR_SDF_GRID_MAX_DIM and DEXR_SDF_GRID_MAX_SAMPLES.
 *
 * BOUNDED LAUNCHES.  The work can reach 2^44 pairs, so no launch does more than DEXR_MESH_PAIRS_PER_LAUNCH of them: an entry point
 * enqueues consecutive ranges of
 *
 *   max(1, (DEXR_MESH_PAIRS_PER_LAUNCH / T) / DEXR_MESH_BLOCK_POINTS) * DEXR_MESH_BLOCK_POINTS
 *
 * points, one launch each, on the caller's stream: a whole number of blocks, one at least (at the largest mesh a block is
 * DEXR_MESH_BLOCK_POINTS << 20 pairs, still below the figure).  The constant is chosen from the measured float64 pair rate so that a
 * launch stays under about a quarter of a second: docs/experiments/mesh_sdf.md.
 */
#ifndef DEXR_MESH_SDF_H
#define DEXR_MESH_SDF_H

#include "dexr_sdf_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_MESH_MAX_VERTICES (1 << 20)
#define DEXR_MESH_MAX_TRIANGLES (1 << 20)
#define DEXR_MESH_TILE 256                      /* triangles staged through LDS at a time */
#define DEXR_MESH_BLOCK_POINTS 512              /* points of one block: 256 threads, two points each */
#define DEXR_MESH_PAIRS_PER_LAUNCH (1ll << 34)  /* point-triangle pairs of one launch, see above */

typedef struct dexr_mesh dexr_mesh;

/* vertices (n_vertex, 3) float64, faces (n_triangle, 3) int32, host pointers.  DEXR_ERR_INVALID before any HIP call: a null
 * argument; n_vertex or n_triangle below 1 or above DEXR_MESH_MAX_VERTICES / DEXR_MESH_MAX_TRIANGLES; a face index outside
 * 0 .. n_vertex - 1; a vertex coordinate that is not finite; a triangle whose cross product (b - a) x (c - a), evaluated in float64
 * without fused multiply-add, is exactly zero in all three components (two equal indices among them).  A well-formed input needs a
 * device (the records are uploaded once, in both precisions): DEXR_ERR_HIP without one. */
int dexr_mesh_create(int32_t n_vertex, const double* vertices, int32_t n_triangle, const int32_t* faces, dexr_mesh** out);
void dexr_mesh_destroy(dexr_mesh* m);
/* n_vertex, n_triangle, bounds (6: the smallest, then the largest coordinate of all vertices per axis): each may be NULL */
int dexr_mesh_info(const dexr_mesh* m, int32_t* n_vertex, int32_t* n_triangle, double* bounds);

/* DEXR_ERR_INVALID before any launch: a null mesh, P < 0, a null points or dist_out (where P > 0); for the grids a null n, origin,
 * spacing or values_out, a dimension or a sample count out of range, a spacing that is not finite or not > 0, an origin that is
 * not finite. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * points (P, 3) -> dist_out (P) = sdf, winding_out (P) = w rounded to float32, or NULL. */
int dexr_mesh_distances_dev(const dexr_mesh* m, int64_t P, const float* points, float* dist_out, float* winding_out, void* stream);
/* Host pointers, float64 in and out, float64 arithmetic on the device: copy, run, synchronise. */
int dexr_mesh_distances(const dexr_mesh* m, int64_t P, const double* points, double* dist_out, double* winding_out);

/* n (3) int32, origin (3) and spacing (3) float64 on the host; values_out (n[0] n[1] n[2]) float32 in C order.
 * The _dev form: values_out a device pointer, float32 arithmetic, enqueued on `stream`; never synchronises, never allocates. */
int dexr_mesh_sample_grid_dev(const dexr_mesh* m, const int32_t n[3], const double origin[3], const double spacing[3], float* values_out,
                              void* stream);
/* values_out a host pointer; float64 arithmetic on the device, rounded to float32 at the store: copy, run, synchronise. */
int dexr_mesh_sample_grid(const dexr_mesh* m, const int32_t n[3], const double origin[3], const double spacing[3], float* values_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_MESH_SDF_H */

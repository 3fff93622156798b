/* dexr_sdf_grid.h -- collision of a robot's sphere approximation (dexr_spheres.h) against ONE sampled signed-distance field
 * outside the robot: batched signed distances of every sphere to the field, their vector-Jacobian product, and a fused penalty
 * that returns the energy, its gradient in x and the wrench on the obstacle from ONE launch, in which neither distances nor
 * forces nor normals reach memory.  C ABI.  It is the sibling of dexr_obstacles.h for shapes that no handful of primitives
 * describes -- meshes, scans, depth fusions: a sphere costs one trilinear lookup however complex the shape is.  The robot side
 * is an existing dexr_sphere_model, whose pair list is ignored here; the obstacle side is a handle of its own, a dexr_sdf_grid,
 * that any sphere model may be used with.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * THE GRID.  n = (nx, ny, nz) float32 samples V[ix][iy][iz] in C order (iz the fastest); sample (ix, iy, iz) sits at
 * origin + (ix hx, iy hy, iz hz) of the obstacle frame, spacing = (hx, hy, hz) > 0 and allowed to differ per axis.  Every
 * dimension is DEXR_SDF_GRID_MIN_DIM .. DEXR_SDF_GRID_MAX_DIM and the product at most DEXR_SDF_GRID_MAX_SAMPLES (64 MB), which
 * keeps every 32-bit sample offset exact.
 *
 * Per frame the obstacle frame has a world pose as in dexr_obstacles.h: obstacle_pos (B, 3) and obstacle_rot (B, 3, 3)
 * row-major.  Either may be NULL: zero translation, identity rotation (the same bits as explicit zeros / identities).
 *
 * THE DISTANCE of a point y of the obstacle frame, per axis a:
 *
 *   u_a  = (y_a - origin_a) / h_a               (computed as (y_a - origin_a) * (1 / h_a))
 *   uc_a = clamp(u_a, 0, n_a - 1)               a NaN of u_a clamps to 0, and the NaN reaches the outputs through e
 *   i_a  = min(floor(uc_a), n_a - 2),  t_a = uc_a - i_a     (0 <= t_a <= 1; on the last sample i = n - 2 and t = 1)
 *   v    = the trilinear interpolation of the eight samples V[i + {0,1}^3] at t
 *   e_a  = (u_a - uc_a) h_a                     zero inside the grid's box
 *   sdf(y)  = v + |e|
 *   grad_a  = (u_a == uc_a ? dv/dt_a / h_a : 0) + (|e| > 0 ? e_a / |e| : 0)
 *
 * dv/dt_a is the exact derivative of the interpolant in its cell: the bilinear interpolation of the four sample differences
 * along a.  Inside the grid this is the value and the gradient of one piecewise-trilinear function; outside it is that function
 * at the nearest point of the box plus the distance to the box.  It is continuous everywhere, its gradient jumps across cell
 * faces and the planes of the box.  Far from the grid it grows like a distance: a far grid contributes exact zeros.
 *
 * DEFINITION.  With c_s the world centre of sphere s and r_s its radius (dexr_spheres.h), p_o, R_o the frame's obstacle pose:
 *
 *   y_s = R_o^T (c_s - p_o),   d_s = sdf(y_s) - r_s,   n_s = R_o grad(y_s)
 *
 *   distances      dist[b,s] = d_s                                                              (s: the caller's sphere index)
 *   distance VJP   grad_x[b,c] = sum_s grad_dist[b,s] n_s . Jpt_s[:,c]                           (Jpt_s of dexr_spheres.h)
 *   penalty        h_s = max(0, margin - d_s),   E[b] = sum_s h_s^2,   f_s = -2 h_s n_s
 *                  grad_x[b,c] = sum_s f_s . Jpt_s[:,c]
 *                  wrench[b] = (-sum_s f_s,  -sum_s (c_s - p_o) x f_s)
 *
 * wrench (B, 6) is dE/d(obstacle translation) and dE/d(a world-aligned small rotation of the obstacle about its origin).
 * margin >= 0 and finite.
 *
 * The rest is the contract of dexr_obstacles.h: mimic joints land on the column of their source with their multiplier; joints
 * driven by `fixed` or by a constant move the geometry and receive no gradient; columns no joint reads are exact zeros.  EVERY
 * entry of every output is written.  A non-finite input spoils its own frame only, and no input -- NaN, infinities, huge values
 * in x, fixed, obstacle_pos or obstacle_rot -- makes a kernel read outside the samples.  The outputs of a frame do not depend on
 * B or on where the frame sits in the batch, bit for bit: every sum has a fixed order (per column its joints in walk order and
 * their spheres in table order, the energy and each component of the wrench as sixteen partial sums added in order) and there
 * are no atomics.
 *
 * The per-frame working set and the frames per block are those of dexr_obstacles.h (12 n_slot + 3 n_sphere + 13 values for the
 * distances, 12 n_slot + 6 n_jx + 6 n_sphere + 125 values for the gradient forms); a model whose working set does not fit the
 * 64 KB of LDS of a block of one frame is refused with DEXR_ERR_UNSUPPORTED (none within the limits is).
 */
#ifndef DEXR_SDF_GRID_H
#define DEXR_SDF_GRID_H

#include "dexr_spheres.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_SDF_GRID_MIN_DIM 2               /* samples along an axis: one cell at least */
#define DEXR_SDF_GRID_MAX_DIM 1024            /* samples along an axis */
#define DEXR_SDF_GRID_MAX_SAMPLES (1 << 24)   /* samples of a grid: 64 MB of float32 */

typedef struct dexr_sdf_grid dexr_sdf_grid;

/* n (3) int32, origin (3) and spacing (3) float64, values (n[0] n[1] n[2]) float32 in C order.  Everything is validated before
 * the first HIP call: a null argument, a dimension or a product out of range, a spacing that is not finite or not > 0, an
 * origin that is not finite, a sample that is not finite are DEXR_ERR_INVALID.  A well-formed input needs a device (the samples
 * are uploaded, once, as float32; the float64 kernels widen them on load): DEXR_ERR_HIP without one. */
int dexr_sdf_grid_create(const int32_t n[3], const double origin[3], const double spacing[3], const float* values, dexr_sdf_grid** out);
void dexr_sdf_grid_destroy(dexr_sdf_grid* g);
/* n (3), origin (3), spacing (3): each may be NULL */
int dexr_sdf_grid_info(const dexr_sdf_grid* g, int32_t* n, double* origin, double* spacing);

/* DEXR_ERR_INVALID before any launch: a null sphere model or grid, B < 0, x / fixed NULL where the table reads them, a NULL
 * dist_out of the distances, a NULL grad_dist or grad_x_out (where n_in > 0) of the VJP, a margin that is negative or not
 * finite, every output of the penalty NULL. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * x (B, n_in), fixed (B, n_fixed) or NULL when n_fixed == 0, obstacle_pos (B, 3) or NULL, obstacle_rot (B, 3, 3) or NULL
 * -> dist_out (B, n_sphere). */
int dexr_grid_distances_dev(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const float* x, const float* fixed,
                            const float* obstacle_pos, const float* obstacle_rot, float* dist_out, void* stream);
/* grad_dist (B, n_sphere) -> grad_x_out (B, n_in).  The kinematics, the cell and its gradient are recomputed. */
int dexr_grid_distances_vjp_dev(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const float* x, const float* fixed,
                                const float* obstacle_pos, const float* obstacle_rot, const float* grad_dist, float* grad_x_out,
                                void* stream);
/* -> energy_out (B), grad_x_out (B, n_in), wrench_out (B, 6): each may be NULL, not all three. */
int dexr_grid_penalty_dev(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const float* x, const float* fixed,
                          const float* obstacle_pos, const float* obstacle_rot, float margin, float* energy_out, float* grad_x_out,
                          float* wrench_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device, the float32 samples widened): copy, run, synchronise. */
int dexr_grid_distances(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const double* x, const double* fixed,
                        const double* obstacle_pos, const double* obstacle_rot, double* dist_out);
int dexr_grid_distances_vjp(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const double* x, const double* fixed,
                            const double* obstacle_pos, const double* obstacle_rot, const double* grad_dist, double* grad_x_out);
int dexr_grid_penalty(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const double* x, const double* fixed,
                      const double* obstacle_pos, const double* obstacle_rot, double margin, double* energy_out, double* grad_x_out,
                      double* wrench_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_SDF_GRID_H */

/* dexr_obstacles.h -- collision of a robot's sphere approximation (dexr_spheres.h) against posed primitives outside the robot:
 * batched signed distances of every sphere to the nearest primitive, their vector-Jacobian product, and a fused penalty that
 * returns the energy, its gradient in x and the wrench on the obstacle from ONE launch, in which neither distances nor forces
 * nor normals reach memory.  C ABI.  The robot side is an existing dexr_sphere_model, whose pair list is ignored here; the
 * obstacle side is a handle of its own, a dexr_obstacle_set, that any sphere model may be used with.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * OBSTACLE SET.  1 .. DEXR_OBSTACLE_MAX primitives in an obstacle frame, each a kind and DEXR_OBSTACLE_PARAMS float64
 * parameters (the unused ones are ignored; pass 0).  The signed distance of a point y of the obstacle frame:
 *
 *   DEXR_OBSTACLE_SPHERE     c (3), r                    |y - c| - r
 *   DEXR_OBSTACLE_CAPSULE    a (3), b (3), r             |y - (a + t (b - a))| - r,  t = clamp((y - a).(b - a) / |b - a|^2, 0, 1);
 *                                                        a == b gives t = 0
 *   DEXR_OBSTACLE_BOX        c (3), half extents h (3),  u = R^T (y - c), q = |u| - h (per axis):
 *                            R (9, row-major, box axes     max_i q_i <= 0   max_i q_i, the normal along the first largest axis
 *                            -> obstacle frame)            otherwise        |max(q, 0)|
 *   DEXR_OBSTACLE_HALFSPACE  n (3, unit), offset         n . y - offset
 *
 * Per frame the obstacle frame has a world pose: obstacle_pos (B, 3) and obstacle_rot (B, 3, 3) row-major.  Either may be
 * NULL: zero translation, identity rotation (the same bits as explicit zeros / identities).  A shared scene leaves both out, a
 * held object has one pose per frame.
 *
 * DEFINITION.  With c_s the world centre of sphere s and r_s its radius (dexr_spheres.h), p_o, R_o the frame's obstacle pose:
 *
 *   y_s  = R_o^T (c_s - p_o)
 *   d_sm = sdf_m(y_s) - r_s
 *   n_sm = R_o grad sdf_m(y_s)                  (zero where there is no direction: y_s on a sphere's centre or a capsule's axis)
 *
 *   distances      dist[b,s] = min_m d_sm       nearest[b,s] = the first m that attains it      (s: the caller's sphere index)
 *   distance VJP   grad_x[b,c] = sum_s grad_dist[b,s] n_{s,nearest} . Jpt_s[:,c]                 (Jpt_s of dexr_spheres.h)
 *   penalty        h_sm = max(0, margin - d_sm),   E[b] = sum_s sum_m w_m h_sm^2
 *                  f_s = sum_m -2 w_m h_sm n_sm,   grad_x[b,c] = sum_s f_s . Jpt_s[:,c]
 *                  wrench[b] = (-sum_s f_s,  -sum_s (c_s - p_o) x f_s)
 *
 * wrench (B, 6) is dE/d(obstacle translation) and dE/d(a world-aligned small rotation of the obstacle about its origin).
 * margin >= 0 and finite.  w (n_prim) is shared by the batch and must be >= 0 (not checked); NULL means 1.
 *
 * The rest is the sphere family's contract: mimic joints land on the column of their source with their multiplier; joints
 * driven by `fixed` or by a constant move the geometry and receive no gradient; columns no joint reads are exact zeros.  EVERY
 * entry of every output is written.  A non-finite input spoils its own frame only.  The outputs of a frame do not depend on B
 * or on where the frame sits in the batch, bit for bit: every sum has a fixed order (per sphere its primitives in set order,
 * per column its joints in walk order and their spheres in table order, the energy and each component of the wrench as sixteen
 * partial sums added in order) and there are no atomics.
 *
 * A model whose per-frame working set (12 n_slot + 3 n_sphere + 13 values for the distances, 12 n_slot + 6 n_jx + 6 n_sphere +
 * 125 values for the gradient forms, n_jx the joints driven by x) does not fit the 64 KB of LDS of a block of one frame is
 * refused with DEXR_ERR_UNSUPPORTED (none within the limits is: 8 slots, 64 joints and 128 spheres need 10 984 B per frame in
 * float64, four frames per block).
 */
#ifndef DEXR_OBSTACLES_H
#define DEXR_OBSTACLES_H

#include "dexr_spheres.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_OBSTACLE_MAX 64    /* primitives per set */
#define DEXR_OBSTACLE_PARAMS 16 /* float64 parameters per primitive */

#define DEXR_OBSTACLE_SPHERE 0
#define DEXR_OBSTACLE_CAPSULE 1
#define DEXR_OBSTACLE_BOX 2
#define DEXR_OBSTACLE_HALFSPACE 3

typedef struct dexr_obstacle_set dexr_obstacle_set;

/* kind (n_prim) int32, param (n_prim, DEXR_OBSTACLE_PARAMS) float64.  Everything is validated before the first HIP call: a
 * count out of range, a null argument, an unknown kind, a non-finite parameter (the unused ones included), a negative radius, a
 * half extent that is not positive, a box rotation that is not orthonormal or a half-space normal that is not unit, each to
 * 1e-6, are DEXR_ERR_INVALID.  A well-formed input needs a device (the tables are uploaded): DEXR_ERR_HIP without one. */
int dexr_obstacle_set_create(int32_t n_prim, const int32_t* kind, const double* param, dexr_obstacle_set** out);
void dexr_obstacle_set_destroy(dexr_obstacle_set* o);
int dexr_obstacle_set_info(const dexr_obstacle_set* o, int32_t* n_prim);

/* DEXR_ERR_INVALID before any launch: a null sphere model or obstacle set, B < 0, x / fixed NULL where the table reads them,
 * a NULL grad_dist or grad_x_out (where n_in > 0) of the VJP, a margin that is negative or not finite, every output of a call
 * NULL. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * x (B, n_in), fixed (B, n_fixed) or NULL when n_fixed == 0, obstacle_pos (B, 3) or NULL, obstacle_rot (B, 3, 3) or NULL
 * -> dist_out (B, n_sphere) and / or nearest_out (B, n_sphere) int32: either may be NULL, not both. */
int dexr_obstacle_distances_dev(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const float* x, const float* fixed,
                                const float* obstacle_pos, const float* obstacle_rot, float* dist_out, int32_t* nearest_out,
                                void* stream);
/* grad_dist (B, n_sphere) -> grad_x_out (B, n_in).  The kinematics, the nearest primitive and its normal are recomputed. */
int dexr_obstacle_distances_vjp_dev(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const float* x,
                                    const float* fixed, const float* obstacle_pos, const float* obstacle_rot, const float* grad_dist,
                                    float* grad_x_out, void* stream);
/* prim_weight (n_prim) or NULL -> energy_out (B), grad_x_out (B, n_in), wrench_out (B, 6): each may be NULL, not all three. */
int dexr_obstacle_penalty_dev(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const float* x, const float* fixed,
                              const float* obstacle_pos, const float* obstacle_rot, float margin, const float* prim_weight,
                              float* energy_out, float* grad_x_out, float* wrench_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_obstacle_distances(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const double* x, const double* fixed,
                            const double* obstacle_pos, const double* obstacle_rot, double* dist_out, int32_t* nearest_out);
int dexr_obstacle_distances_vjp(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const double* x,
                                const double* fixed, const double* obstacle_pos, const double* obstacle_rot, const double* grad_dist,
                                double* grad_x_out);
int dexr_obstacle_penalty(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const double* x, const double* fixed,
                          const double* obstacle_pos, const double* obstacle_rot, double margin, const double* prim_weight,
                          double* energy_out, double* grad_x_out, double* wrench_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_OBSTACLES_H */

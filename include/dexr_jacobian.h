/* dexr_jacobian.h -- batched link Jacobians J = d(pose)/dx and link velocities J xdot on a pose table (dexr_pose.h): C ABI.
 * No table format of its own: every function takes the dexr_pose_model of a list of links.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  For a pose table with inputs x (B, n_in) and fixed (B, n_fixed), link l and input column c
 *
 *   Jlin[b,l,:,c] = sum_k mult_k * ( a_k x (p_l - o_k)   revolute  |  a_k   prismatic )
 *   Jang[b,l,:,c] = sum_k mult_k * ( a_k                 revolute  |  0     prismatic )
 *
 * summed over the joints k with src_kind == DEXR_POSE_SRC_X, src_col == c and k on the chain of link l; a_k is the world
 * axis and o_k the world origin of joint k, p_l the world origin of link l, all at (x, fixed).  Mimic joints therefore land
 * on the column of their source with their multiplier applied (the fold of dexr_link_poses_vjp).  Columns no joint feeds
 * are exact zeros; joints driven by `fixed` or by a constant, and links on the fixed base, contribute nothing.  EVERY entry
 * of an output is written: the caller pre-zeroes nothing.
 *
 * Frames: DEXR_JAC_WORLD_ALIGNED is the formula above (velocity of the link origin and angular velocity in world axes,
 * pinocchio's LOCAL_WORLD_ALIGNED); DEXR_JAC_LOCAL multiplies both blocks on the left by R_l^T (the link's own axes,
 * pinocchio's LOCAL: rows 0-2 linear, 3-5 angular of a 6 x n frame Jacobian).
 *
 * Link velocities are the same contraction without the matrix: lin[b,l] = Jlin[b,l] xdot[b], ang[b,l] = Jang[b,l] xdot[b].
 */
#ifndef DEXR_JACOBIAN_H
#define DEXR_JACOBIAN_H

#include "dexr_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_JAC_WORLD_ALIGNED 0
#define DEXR_JAC_LOCAL 1

/* DEXR_ERR_INVALID before any launch: a null model, B < 0, an unknown frame, both outputs NULL, x / fixed / xdot NULL
 * where the table reads them. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * jlin_out / jang_out (B, n_link, 3, n_in): either may be NULL, not both. */
int dexr_link_jacobians_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, int32_t frame,
                            float* jlin_out, float* jang_out, void* stream);
/* xdot (B, n_in) -> lin_out (B, n_link, 3), ang_out (B, n_link, 3): either may be NULL, not both. */
int dexr_link_velocities_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, const float* xdot,
                             int32_t frame, float* lin_out, float* ang_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_link_jacobians(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, int32_t frame,
                        double* jlin_out, double* jang_out);
int dexr_link_velocities(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, const double* xdot,
                         int32_t frame, double* lin_out, double* ang_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_JACOBIAN_H */

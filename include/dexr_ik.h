/* dexr_ik.h -- one damped least-squares (Levenberg-Marquardt) inverse-kinematics step on a pose table (dexr_pose.h), batched:
 * the normal equations of the link Jacobians of dexr_jacobian.h built, factorised and solved inside one kernel.  C ABI; no
 * table format of its own: every function takes the dexr_pose_model of a list of links.  Neither a Jacobian nor the normal
 * matrix is written to memory.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  With Jlin, Jang (B, n_link, 3, n_in) of dexr_jacobian.h in the asked frame and damping = lambda > 0,
 *
 *   dx[b] = argmin_d  1/2 sum_l ( w_lin[b,l] |Jlin[b,l] d - e_lin[b,l]|^2 + w_ang[b,l] |Jang[b,l] d - e_ang[b,l]|^2 ) + 1/2 lambda |d|^2
 *         = H^-1 g,     H = sum_l w_lin Jlin^T Jlin + w_ang Jang^T Jang + lambda I,     g = sum_l w_lin Jlin^T e_lin + w_ang Jang^T e_ang
 *
 * e_lin, e_ang (B, n_link, 3) are the desired displacement of each link origin and a small rotation vector, in world axes at
 * the link origin (DEXR_JAC_WORLD_ALIGNED) or in the link's own axes (DEXR_JAC_LOCAL).  Either may be NULL: its rows are then
 * absent from the sum.  w_lin, w_ang (B, n_link) must be >= 0 (not checked); NULL means 1.
 *
 * Closed form, per joint j driven by x (a_j world axis, o_j world origin, mult_j its multiplier, col_j its column) and link l
 * below it (p_l world origin, R_l rotation):
 *
 *   c_jl = a_j x (p_l - o_j)   revolute   |   a_j   prismatic            (a column of Jlin in world axes, before mult_j)
 *   f_l  = w_lin e_lin (world frame)  |  w_lin R_l e_lin (local frame)    m_l likewise from w_ang, e_ang
 *
 *   H[col_j, col_k] += mult_j mult_k sum_{l below j and k} ( w_lin_l c_jl . c_kl  +  w_ang_l a_j . a_k [j, k both revolute] )
 *   g[col_j]        += mult_j        sum_{l below j}       ( c_jl . f_l           +  a_j . m_l         [j revolute]         )
 *
 * The local frame multiplies both blocks of a link by R_l^T on the left; with one scalar weight per block the rotation
 * cancels in J^T J, so H is the same matrix in both frames and only f_l = R_l e_lin, m_l = R_l e_ang differ.  H is symmetric
 * positive definite because lambda > 0: it is factorised by a Cholesky decomposition without pivoting, over the columns of x
 * that some joint reads (at most 64, whatever n_in is); two triangular solves give dx.
 *
 * Mimic joints fold onto the column of their source with their multiplier (the fold of dexr_link_poses_vjp).  Joints driven
 * by `fixed` or by a constant move the geometry and have no column; links on the fixed base contribute nothing; a link
 * listed twice counts twice.  Columns of x no joint reads are exact zeros in dx.  EVERY entry of dx_out is written.  A frame
 * with a non-finite input gives non-finite values in its own row only.  The row of a frame does not depend on B, on where
 * the frame sits in the batch, or on the other frames, bit for bit: every sum has a fixed order and there are no atomics.
 *
 * A table whose per-frame working set does not fit the 64 KB of LDS of a block of one frame is refused with
 * DEXR_ERR_UNSUPPORTED.  No table within the limits of dexr_pose.h is: 64 active columns, 64 links and 8 slots need
 * 8 * (96 + 384 + 704 + 2080 + 192 + 1) = 27 656 B per frame in float64.
 */
#ifndef DEXR_IK_H
#define DEXR_IK_H

#include "dexr_jacobian.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DEXR_ERR_INVALID before any launch: a null model, B < 0, an unknown frame, err_lin and err_ang both NULL, dx_out NULL,
 * x / fixed NULL where the table reads them, damping not finite or <= 0, w_lin given while err_lin is NULL, w_ang given
 * while err_ang is NULL. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * err_lin / err_ang (B, n_link, 3), w_lin / w_ang (B, n_link) or NULL -> dx_out (B, n_in). */
int dexr_link_ik_step_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, int32_t frame,
                          const float* err_lin, const float* err_ang, const float* w_lin, const float* w_ang,
                          float damping, float* dx_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_link_ik_step(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, int32_t frame,
                      const double* err_lin, const double* err_ang, const double* w_lin, const double* w_ang,
                      double damping, double* dx_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_IK_H */

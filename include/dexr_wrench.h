/* dexr_wrench.h -- J^T on a pose table (dexr_pose.h): batched link wrenches tau = J^T (force, torque) and the vector-Jacobian
 * product of the link velocities of dexr_jacobian.h in x and in xdot.  C ABI; no table format of its own: every function
 * takes the dexr_pose_model of a list of links.  No Jacobian matrix is formed.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  With Jlin, Jang (B, n_link, 3, n_in) of dexr_jacobian.h in the asked frame,
 *
 *   tau[b,c]       = sum_l  Jlin[b,l,:,c] . force[b,l]  +  Jang[b,l,:,c] . torque[b,l]                         (link wrenches)
 *   grad_xdot[b,c] = the same sum with (grad_lin, grad_ang) for (force, torque)       = dL/dxdot of L(lin, ang)  (velocity VJP)
 *   grad_x[b,c]    = sum_l  grad_lin[b,l] . d lin[b,l]/dx[b,c]  +  grad_ang[b,l] . d ang[b,l]/dx[b,c]     = dL/dx
 *
 * for lin = Jlin xdot, ang = Jang xdot (dexr_link_velocities).  Closed form, per joint j driven by x (a_j world axis, o_j
 * world origin, qd_j = mult_j xdot[col_j]; (V_j, W_j) the twist of joint j's body taken at o_j after joint j's own advance;
 * (v_l, w_l) the world-aligned velocity of link l, R_l its rotation, p_l its origin):
 *
 *   world frame:  f_l = g_lin_l        m_l = g_ang_l        A_l = v_l x f_l + w_l x m_l
 *   local frame:  f_l = R_l g_lin_l    m_l = R_l g_ang_l    A_l = 0   (the derivative of R_l^T cancels it exactly)
 *
 *   F = sum f_l,  G = sum m_l,  T0 = sum p_l x f_l,  A = sum A_l     over the links below joint j
 *
 *   dL/dqd_j = a_j . (T0 + G - o_j x F)                                       revolute       a_j . F             prismatic
 *   dL/dq_j  = a_j . (A - V_j x F - W_j x G) + (W_j x a_j) . (T0 - o_j x F)   revolute       (W_j x a_j) . F     prismatic
 *
 *   grad_xdot[col_j] += mult_j dL/dqd_j        grad_x[col_j] += mult_j dL/dq_j
 *
 * Mimic joints land on the column of their source with their multiplier (the fold of dexr_link_poses_vjp).  Joints driven by
 * `fixed` or by a constant carry no rate and receive no gradient, but move the geometry; links on the fixed base contribute
 * nothing.  Columns no joint reads are exact zeros.  EVERY entry of an output is written: the caller pre-zeroes nothing.
 * There is no gradient with respect to `fixed`.
 *
 * Frames: DEXR_JAC_WORLD_ALIGNED / DEXR_JAC_LOCAL of dexr_jacobian.h: the frame the forces and torques, or the cotangents of
 * the velocities, are expressed in (world axes at the link origin, or the link's own axes).
 *
 * A table whose per-frame working set does not fit the 64 KB of LDS of a block of 8 frames is refused with
 * DEXR_ERR_UNSUPPORTED (no table within the limits of dexr_pose.h is).
 */
#ifndef DEXR_WRENCH_H
#define DEXR_WRENCH_H

#include "dexr_jacobian.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DEXR_ERR_INVALID before any launch: a null model, B < 0, an unknown frame, both inputs NULL, every output NULL, x / fixed
 * NULL where the table reads them, xdot NULL where grad_x_out is asked for (the rate gradient alone does not read xdot). */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * force / torque (B, n_link, 3): either may be NULL, not both -> tau_out (B, n_in). */
int dexr_link_wrenches_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, int32_t frame,
                           const float* force, const float* torque, float* tau_out, void* stream);
/* grad_lin / grad_ang (B, n_link, 3): either may be NULL, not both -> grad_x_out, grad_xdot_out (B, n_in): either may be
 * NULL, not both.  grad_xdot_out holds the bits dexr_link_wrenches_dev gives for the same cotangents, and a NULL grad_x_out
 * costs what that call costs. */
int dexr_link_velocities_vjp_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, const float* xdot,
                                 int32_t frame, const float* grad_lin, const float* grad_ang, float* grad_x_out,
                                 float* grad_xdot_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_link_wrenches(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, int32_t frame,
                       const double* force, const double* torque, double* tau_out);
int dexr_link_velocities_vjp(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, const double* xdot,
                             int32_t frame, const double* grad_lin, const double* grad_ang, double* grad_x_out,
                             double* grad_xdot_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_WRENCH_H */

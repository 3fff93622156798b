/* dexr_ik_solve.h -- batched inverse kinematics to link pose targets on a pose table (dexr_pose.h): the damped least-squares
 * step of dexr_ik.h iterated inside ONE kernel, with joint limits.  Every iterate, the normal matrix and its factor stay on
 * chip; one launch takes start configurations and world targets and returns the solved configurations, the iterations each
 * frame used and its final error.  C ABI; no table format of its own: every function takes the dexr_pose_model of a list of
 * links.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  World axes only: the targets are world poses, there is no frame argument.  Per frame, x_0 is the start as given.
 * For k = 0, 1, ...:
 *
 *   1. forward kinematics at x_k: p_l, R_l of every link of the table.
 *   2. e_lin_l = tgt_pos_l - p_l.   With M = tgt_rot_l R_l^T, v = 1/2 vee(M - M^T), c = (tr M - 1) / 2, s = |v|:
 *      e_ang_l = v * (s > 1e-6 ? atan2(s, c) / s : 1), the rotation vector, in world axes, that takes the link to its target.
 *      A rotation error of angle pi is OUTSIDE THE CONTRACT: s is near 0 there and the error reads as 0.
 *      A NULL tgt_pos or tgt_rot removes its rows, as in dexr_ik.h.
 *   3. E_k = sum_l ( w_lin |e_lin_l|^2 + w_ang |e_ang_l|^2 ), summed over the links in table order.  If E_k <= tol^2 the frame
 *      stops: iters = k, x_out = x_k, err_out = sqrt(E_k).  If k == max_iters it stops the same way with iters = max_iters.
 *   4. g and H exactly as dexr_ik.h defines them, in the world frame (DEXR_JAC_WORLD_ALIGNED).  Column i is FROZEN when
 *      (x_i <= lo_i and g_i < 0) or (x_i >= hi_i and g_i > 0): the step would push it out of its bounds.  The row and the
 *      column of H of a frozen column become those of the identity and g_i = 0, so dx_i = 0 exactly.
 *   5. dx = H^-1 g by the Cholesky factorisation and the two triangular solves of dexr_ik.h.
 *   6. if max_step > 0: with m = max_i |dx_i|, dx *= max_step / m where m > max_step.
 *   7. x_{k+1,i} = v < lo_i ? lo_i : (v > hi_i ? hi_i : v) with v = x_{k,i} + dx_i: comparisons, so that a NaN stays a NaN.
 *
 * lo, hi (n_in) are shared by the batch: both NULL (no bounds, nothing is ever frozen or clamped) or both given.  Columns of
 * x no joint reads are copied from the start unchanged, with no clamp.  Mimic joints, fixed joints, links on the fixed base and
 * links listed twice behave as in dexr_ik.h (a link on the fixed base moves with no column but its error counts in E_k).
 * w_lin, w_ang (B, n_link) must be >= 0 (not checked); NULL means 1.  Forward kinematics is evaluated iters + 1 times per
 * frame.  EVERY entry of every output is written.  A non-finite input spoils its own frame only; that frame runs to max_iters.
 * The outputs of a frame do not depend on B, on where the frame sits in the batch, or on when the frames beside it stop, bit
 * for bit: every sum has a fixed order and there are no atomics.
 *
 * A table whose per-frame working set does not fit the 64 KB of LDS of a block of one frame is refused with
 * DEXR_ERR_UNSUPPORTED.  64 active columns of 64, 64 links and 8 slots need 8 * (96 + 384 + 704 + 2080 + 192 + 64 + 1) + 136 =
 * 28 304 B per frame in float64: two frames per block.
 */
#ifndef DEXR_IK_SOLVE_H
#define DEXR_IK_SOLVE_H

#include "dexr_ik.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DEXR_ERR_INVALID before any launch: a null model, B < 0, tgt_pos and tgt_rot both NULL, w_lin given while tgt_pos is NULL,
 * w_ang given while tgt_rot is NULL, damping not finite or <= 0, x0 / fixed NULL where the table reads them, x_out NULL, only
 * one of lo / hi given, max_iters outside 1..256, tol or max_step negative or not finite (max_step == 0: no limit). */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * x0 (B, n_in), fixed (B, n_fixed), tgt_pos (B, n_link, 3), tgt_rot (B, n_link, 3, 3) row-major, w_lin / w_ang (B, n_link) or
 * NULL, lo / hi (n_in) or NULL -> x_out (B, n_in), iters_out (B) int32 or NULL, err_out (B) or NULL.  x_out may alias x0. */
int dexr_link_ik_solve_dev(const dexr_pose_model* m, int64_t B, const float* x0, const float* fixed, const float* tgt_pos,
                           const float* tgt_rot, const float* w_lin, const float* w_ang, const float* lo, const float* hi,
                           float damping, float max_step, float tol, int32_t max_iters, float* x_out, int32_t* iters_out,
                           float* err_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_link_ik_solve(const dexr_pose_model* m, int64_t B, const double* x0, const double* fixed, const double* tgt_pos,
                       const double* tgt_rot, const double* w_lin, const double* w_ang, const double* lo, const double* hi,
                       double damping, double max_step, double tol, int32_t max_iters, double* x_out, int32_t* iters_out,
                       double* err_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_IK_SOLVE_H */

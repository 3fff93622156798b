/* dexr_resolve.h -- collision-aware posture solve on a sphere model (dexr_spheres.h): a damped Gauss-Newton iteration with an
 * accept / reject rule that projects a posture out of self-penetration, stays near a reference posture and keeps chosen links at
 * world targets, iterated inside ONE kernel.  Every iterate, the forces, the list of active pairs, the normal matrix, its factor
 * and the per-frame damping stay on chip; one launch takes start postures and returns the resolved postures, the trial steps each
 * frame took, the three energies at the answer and a status word.  C ABI; no handle of its own: every function takes a
 * dexr_sphere_model.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  Per frame the variables are x (n_in of them).  With p_l, R_l the world pose of link l and d_p, w_p, n_p of
 * dexr_spheres.h:
 *
 *   E(x)   = E_pose + E_post + E_col
 *   E_pose = sum over the target links  w_pos |t_pos - p_l|^2 + w_rot |log(T_rot R_l^T)|^2       the terms of dexr_ik_solve.h
 *   E_post = sum_c u_c (x_c - xref_c)^2                                                           over ALL n_in columns, in order
 *   E_col  = w_col sum_p w_p h_p^2,   h_p = max(0, margin - d_p)
 *
 *   g = -1/2 grad E = J^T W e + u (xref - x) + w_col sum_p w_p h_p grad d_p
 *   H (Gauss-Newton) = J^T W J + diag(u) + w_col sum over the curvature pairs of w_p (grad d_p)(grad d_p)^T
 *
 * The TARGET LINKS are the first n_target rows of the model's link list (0 .. n_link); rows may carry no sphere.  The ACTIVE
 * PAIRS of a frame (h_p > 0) form a list in pair-index order; energy and gradient use every one of them, the curvature the
 * first DEXR_RESOLVE_MAXACTIVE of the list.  grad d_p in column a is n_p . (Jpt_i - Jpt_j) of dexr_spheres.h, each joint of the
 * column counting for the spheres below it.
 *
 *   x <- x0;  E <- E(x);  lam <- damping;  iters <- 0;  rejects <- 0;  status <- 0
 *   while iters < max_iters:
 *     g, H at x.  Column i is FROZEN when (x_i <= lo_i and g_i < 0) or (x_i >= hi_i and g_i > 0): its row and column of H become
 *       the identity's and g_i = 0, exactly as in dexr_ik_solve.h.
 *     (H + lam I) dx = g (lam on the columns that are not frozen), by the Cholesky factorisation of dexr_ik.h.
 *     if max_step > 0: with m = max_i |dx_i|, dx *= max_step / m where m > max_step.
 *     xt_i = clamp(x_i + dx_i, lo_i, hi_i) on the columns some joint reads (comparisons: a NaN stays a NaN);  iters += 1;  Et = E(xt)
 *     if Et <= E   (a comparison: a NaN rejects):
 *       step = max_i |xt_i - x_i|;  x, E <- xt, Et;  lam <- max(lam / DEXR_RESOLVE_LAM_DOWN, damping);  rejects <- 0
 *       if step <= tol: status |= DEXR_RESOLVE_CONVERGED, stop
 *     else:
 *       lam <- DEXR_RESOLVE_LAM_UP lam;  rejects += 1
 *       if rejects == DEXR_RESOLVE_MAXREJECT: status |= DEXR_RESOLVE_STALLED, stop
 *
 * The answer is always an accepted point: E(x_out) <= E(x0) in the kernel's own arithmetic.  iters counts trial steps.  If any
 * evaluated point (x0 or a trial) has more than DEXR_RESOLVE_MAXACTIVE active pairs, status |= DEXR_RESOLVE_TRUNCATED; the
 * accept / reject rule keeps the descent property.  The two factors are powers of two, so lam takes the same values in float32
 * and in float64.  A rejected trial leaves x where it was, so g and H are those of the last accepted point: the kernel keeps
 * them (before the damping) and only adds the new lam -- a rejection costs neither a second walk nor a pass.
 *
 * x_ref (B, n_in) NULL means x0.  posture_weight u (n_in) >= 0 (not checked) is shared by the batch, NULL means 0.  pos_weight,
 * rot_weight (B, n_target) >= 0 (not checked), NULL means 1.  pair_weight (n_pair) as in dexr_spheres.h.  lo, hi (n_in) are
 * shared by the batch: both NULL (nothing is ever frozen or clamped) or both given.  Columns of x no joint reads are copied from
 * the start unchanged, with no clamp.  Mimic joints fold onto their source's column, joints driven by `fixed` or by a constant
 * move the geometry and are no variables.
 *
 * EVERY entry of every output is written.  A non-finite input spoils its own frame only; that frame ends within max_iters
 * trial steps.  The outputs of a frame do not depend on B, on where the frame sits in the batch, or on when the frames beside it
 * stop, bit for bit: every sum is taken by one thread in table order and there are no atomics.
 *
 * A model whose per-frame working set does not fit the 64 KB of LDS of a block of one frame is refused with
 * DEXR_ERR_UNSUPPORTED.  The largest model within the limits (64 links and active columns, 128 spheres, 8128 pairs, 256 columns,
 * 8 slots) needs 64 608 B in float64: one frame per block.
 */
#ifndef DEXR_RESOLVE_H
#define DEXR_RESOLVE_H

#include "dexr_spheres.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_RESOLVE_MAXACTIVE 256 /* active pairs of a frame that enter the curvature */
#define DEXR_RESOLVE_LAM_UP 8      /* lam *= this after a rejected trial */
#define DEXR_RESOLVE_LAM_DOWN 4    /* lam /= this after an accepted trial, never below `damping` */
#define DEXR_RESOLVE_MAXREJECT 12  /* rejections in a row that end a frame */

#define DEXR_RESOLVE_CONVERGED 1 /* an accepted step moved no variable by more than tol */
#define DEXR_RESOLVE_STALLED 2   /* DEXR_RESOLVE_MAXREJECT rejections in a row */
#define DEXR_RESOLVE_TRUNCATED 4 /* some evaluated point had more than DEXR_RESOLVE_MAXACTIVE active pairs */

/* DEXR_ERR_INVALID before any launch: a null model, B < 0, margin / collision_weight / tol / max_step negative or not finite
 * (max_step == 0: no limit), damping not finite or <= 0, max_iters outside 1..256, only one of lo / hi given, n_target outside
 * 0..n_link, n_target > 0 with target_pos and target_rot both NULL, pos_weight given while target_pos is NULL, rot_weight given
 * while target_rot is NULL, a target or weight array given while n_target == 0, x_out NULL, x0 / fixed NULL where the table
 * reads them. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * x0 (B, n_in), fixed (B, n_fixed) or NULL, x_ref (B, n_in) or NULL, posture_weight (n_in) or NULL, target_pos (B, n_target, 3),
 * target_rot (B, n_target, 3, 3) row-major, pos_weight / rot_weight (B, n_target) or NULL, pair_weight (n_pair) or NULL, lo / hi
 * (n_in) or NULL -> x_out (B, n_in), iters_out (B) int32 or NULL, energy_out (B, 3): E_pose, E_post, E_col at x_out, or NULL,
 * status_out (B) int32 or NULL.  x_out may alias x0. */
int dexr_sphere_resolve_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                            const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                            const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                            const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                            int32_t max_iters, float* x_out, int32_t* iters_out, float* energy_out, int32_t* status_out,
                            void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_sphere_resolve(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                        const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                        const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                        const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                        int32_t max_iters, double* x_out, int32_t* iters_out, double* energy_out, int32_t* status_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_RESOLVE_H */

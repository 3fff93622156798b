/* dexr_resolve_cross.h -- the collision-aware posture solve of dexr_resolve.h against a SECOND POSED ROBOT: robot A's posture is
 * the variable, robot B is held at a given posture with a given pose per frame in A's root frame and acts as a body made of B's
 * spheres (the two-robot term of dexr_cross.h inside the resident loop) -- two hands that interpenetrate after retargeting, a hand
 * against an arm.  One launch projects A's postures out of self-penetration AND out of B: one energy, one descent.  Every iterate,
 * B's centres, the forces, both contact lists, the normal matrix, its factor and the per-frame damping stay on chip.  C ABI; no
 * handle of its own: every function takes two dexr_sphere_model handles, A and B, which may be the same handle.  B's pair list is
 * ignored.  A solve over both robots' columns at once is not offered: n_act_a + n_act_b would exceed the 64 active columns the
 * factor code of dexr_ik.h is built for; alternate two calls instead.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  Everything of dexr_resolve.h holds unchanged for A: the variables, the freeze rule, the damping factors, the step
 * limit, the clamp, the stop rules, iters, "the answer is an accepted point", the NULL rules, x_out may alias x0.  B's inputs are
 * x_b (B, n_in_b), fixed_b (B, n_fixed_b), other_pos (B, 3) and other_rot (B, 3, 3) row-major; the last two follow the NULL rule of
 * dexr_obstacles.h: NULL is zero translation / the identity, with the same bits as explicit zeros / identities.  B's posture and
 * pose are fixed during the solve.  With c_s the centre of a sphere in its robot's root frame and r_s its radius (dexr_spheres.h),
 *
 *   C^A_s = c^A_s(x)          C^B_t = other_pos + other_rot c^B_t(x_b)          (both in A's root frame)
 *   D_st = C^A_s - C^B_t,  s_st = |D_st|,  d_st = s_st - (r_s + r_t),  n_st = s_st > 0 ? D_st / s_st : 0        (as in dexr_cross.h)
 *
 *   E      = ((E_pose + E_post) + E_col) + E_x            (this order of addition)
 *   E_x    = w_x sum_s sum_t w_st h_st^2,   h_st = max(0, margin_x - d_st)
 *   g     += w_x sum over ALL active contacts of w_st h_st grad d_st,        grad d_st [c] = n_st . Jpt^A_s[:, c]     (B does not move)
 *   H     += w_x sum over the CURVATURE contacts of w_st (grad d_st)(grad d_st)^T
 *
 * margin_x >= 0 and w_x >= 0, both finite.  cross_weight (S_a, S_b), indexed by the callers' sphere indices, is shared by the batch
 * and must be >= 0 (not checked); NULL means 1, a zero masks a pair: the pair adds exact zeros to E_x, g and H (it still counts as
 * a contact below while h_st > 0).
 *
 * The ACTIVE CONTACTS of a frame are the (s, t) with h_st > 0, ordered by the CALLER's sphere index of A, then by the CALLER's
 * sphere index of B.  Energy and gradient use every one of them, the curvature the first DEXR_RESOLVE_MAXCONTACT (256) of that
 * order.  If any evaluated point (x0 or a trial) has more, status |= DEXR_RESOLVE_CONTACTS_TRUNCATED; both constants are those of
 * dexr_resolve_obstacles.h.  The pair side keeps its own list, its own cap (DEXR_RESOLVE_MAXACTIVE) and its own bit
 * (DEXR_RESOLVE_TRUNCATED).  Coincident centres follow the rule of dexr_cross.h: no direction and no NaN; such a contact counts in
 * E_x with h = margin_x + r_s + r_t and adds neither force nor curvature.
 *
 * OUTPUTS, each of which may be NULL except x_out: x_out (B, n_in_a), iters_out (B) int32, energy_out (B, 4): E_pose, E_post, E_col,
 * E_x at x_out, status_out (B) int32.  EVERY entry of every output is written.  A non-finite input (x_b, fixed_b and B's pose
 * included) spoils its own frame only; that frame ends within max_iters trial steps.  The outputs of a frame do not depend on B, on
 * where the frame sits in the batch, or on when the frames beside it stop, bit for bit: there are no atomics and every sum is taken
 * by one thread in a fixed order --
 *   the force on a sphere of A   w_col times its pair force (dexr_resolve.h) first, then fma(w_x, f_x, .), where f_x = sum_t w_st h_st
 *                                n_st runs over B's spheres in B's TABLE order (the order dexr_sphere_model_create sorted them into:
 *                                by their link's position in the walk, ties by the caller's index);
 *   E_x                          sixteen partial sums, partial k holding A's table spheres k, k + 16, ... (each over B in table
 *                                order), added in order, then multiplied by w_x: the order dexr_cross.h counts its E in;
 *   a column of g, an entry of H as in dexr_resolve.h; the curvature rows in the order of the contact list above, behind the pairs'.
 *
 * LDS.  A block holds 16 frames, halved until its working set fits 64 KB.  With v = 4 (float32) or 8 (float64) bytes a value, for A
 * n_jx the joints driven by x, n_act the active columns, n_tri = n_act (n_act + 1) / 2, L = 11 n_link with targets, else 0, and S_a,
 * S_b the spheres and n_slot_a, n_slot_b the fork slots of the two tables, one frame needs
 *
 *   values = (6 n_jx + L + 6 S_a + 16 + max(n_tri, 16 n_act + 16) + n_tri + 4 n_act + 2 n_in + 8 + 3 S_b + 12 + 16) | 1
 *   bytes  = 128 + 16 S_a + v (12 (n_slot_a + n_slot_b) + values) + 4 (DEXR_RESOLVE_MAXACTIVE + 22) + 4 * 17
 *            + 2 DEXR_RESOLVE_MAXCONTACT + ((n_pair_a + 3) & ~3)
 *
 * (dexr_resolve.h's working set; B's centres in A's root frame, B's parked pose, sixteen more partial energies, B's fork slots, a
 * 128-bit contact mask per sphere of A, the contact list, 16 bits an entry, and its counts).  A pair of models whose one frame
 * does not fit is refused with DEXR_ERR_UNSUPPORTED and the message states `bytes`.
 */
#ifndef DEXR_RESOLVE_CROSS_H
#define DEXR_RESOLVE_CROSS_H

#include "dexr_cross.h"
#include "dexr_resolve_obstacles.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DEXR_ERR_INVALID before any launch: every rule of dexr_resolve.h, a null `other`, x_b / fixed_b NULL where B's table reads them,
 * a margin_x or w_x that is negative or not finite.  The null models and the scalar rules are checked at B == 0 too, as the scene
 * header does: B == 0 is the no-op returning 0 for a call that passes them (NULL x0, fixed, x_b, fixed_b and outputs included). */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.  The arguments of
 * dexr_sphere_resolve_dev up to max_iters, then B's handle `other`, x_b, fixed_b, other_pos or NULL, other_rot or NULL, margin_x,
 * w_x, cross_weight (S_a, S_b) or NULL -> the outputs above.  x_out may alias x0. */
int dexr_sphere_resolve_cross_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                  const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                  const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                  const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                                  int32_t max_iters, const dexr_sphere_model* other, const float* x_b, const float* fixed_b,
                                  const float* other_pos, const float* other_rot, float margin_x, float w_x, const float* cross_weight,
                                  float* x_out, int32_t* iters_out, float* energy_out, int32_t* status_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_sphere_resolve_cross(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                              const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                              const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                              const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                              int32_t max_iters, const dexr_sphere_model* other, const double* x_b, const double* fixed_b,
                              const double* other_pos, const double* other_rot, double margin_x, double w_x, const double* cross_weight,
                              double* x_out, int32_t* iters_out, double* energy_out, int32_t* status_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_RESOLVE_CROSS_H */

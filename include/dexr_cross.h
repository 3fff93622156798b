/* dexr_cross.h -- collision between TWO posed robots, each a sphere approximation (dexr_spheres.h) with its own x and its own
 * base pose per frame: batched signed distances of every sphere of either robot to the nearest sphere of the other, their
 * vector-Jacobian product, and a fused penalty that returns the energy, its gradient in both robots' x and the wrench on
 * either base from ONE launch, in which neither distances nor forces nor normals reach memory.  C ABI.  Both sides are existing
 * dexr_sphere_model handles, A and B, whose pair lists are ignored here; they may be the same handle (a hand against its own
 * copy elsewhere).
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * INPUTS PER FRAME.  x_a (B, n_in_a) and fixed_a (B, n_fixed_a), x_b (B, n_in_b) and fixed_b (B, n_fixed_b), and a base pose
 * per robot: pos_a, pos_b (B, 3) and rot_a, rot_b (B, 3, 3) row-major.  Each of the four pose arguments may be NULL: zero
 * translation, identity rotation (the same bits as explicit zeros / identities).
 *
 * DEFINITION.  With c_s(x) the centre of sphere s in its robot's own root frame and r_s its radius (dexr_spheres.h):
 *
 *   C^A_s = pos_a + rot_a c^A_s(x_a)        C^B_t = pos_b + rot_b c^B_t(x_b)
 *   D_st = C^A_s - C^B_t,  s_st = |D_st|,  d_st = s_st - (r_s + r_t),  n_st = s_st > 0 ? D_st / s_st : 0
 *
 *   distances      dist_a[b,s] = min_t d_st      nearest_a[b,s] = the first t that attains it
 *                  dist_b[b,t] = min_s d_st      nearest_b[b,t] = the first s that attains it      (s, t: the callers' indices)
 *   penalty        h_st = max(0, margin - d_st),   E[b] = sum_s sum_t w_st h_st^2
 *                  F^A_s = sum_t -2 w_st h_st n_st  (= dE/dC^A_s)       F^B_t = -sum_s -2 w_st h_st n_st  (= dE/dC^B_t)
 *                  grad_xa[b,c] = sum_s F^A_s . rot_a Jpt^A_s[:,c]      grad_xb[b,c] = sum_t F^B_t . rot_b Jpt^B_t[:,c]
 *                  wrench_a[b] = (sum_s F^A_s,  sum_s (C^A_s - pos_a) x F^A_s)       wrench_b likewise over F^B and pos_b
 *   distance VJP   with ga = grad_dist_a, gb = grad_dist_b (NULL: zeros), na = nearest_a, nb = nearest_b (recomputed):
 *                  F^A_s = ga[s] n_{s,na(s)} + sum over t with nb(t) = s of gb[t] n_st
 *                  F^B_t = -gb[t] n_{nb(t),t} - sum over s with na(s) = t of ga[s] n_st
 *                  grad_xa, grad_xb, wrench_a, wrench_b from F^A, F^B as in the penalty
 *
 * Jpt_s is the point Jacobian of dexr_spheres.h in the robot's root frame.  The first half of a wrench is dE/d(translation of
 * that base), its second half dE/d(a world-aligned small rotation of that base about its origin).  margin >= 0 and finite.
 * w (S_a, S_b), indexed by the callers' sphere indices, is shared by the batch and must be >= 0 (not checked); NULL means 1, a
 * zero masks a pair.
 *
 * The rest is the sphere family's contract: mimic joints land on the column of their source with their multiplier; joints
 * driven by `fixed` or by a constant move the geometry and receive no gradient; columns no joint reads are exact zeros.  EVERY
 * entry of every output is written.  A non-finite input spoils its own frame only.  Coincident centres give no direction and
 * no NaN: such a pair counts in E with h = margin + r_s + r_t and adds no force.  The outputs of a frame do not depend on B or
 * on where the frame sits in the batch, bit for bit: there are no atomics and every sum has a fixed order --
 *   a force        its own cotangent's term first (VJP), then the other robot's spheres in that robot's TABLE order (the order
 *                  dexr_sphere_model_create sorted them into: by their link's position in the walk, ties by the caller's index);
 *   a column       its joints in walk order and their spheres in table order;
 *   E, a wrench    sixteen partial sums added in order, partial k holding the spheres k, k + 16, ... of the table, E counted from
 *                  A's side (per sphere of A the spheres of B in table order).
 * A pair is evaluated from both of its ends; C^A_s - C^B_t is the exact negative of C^B_t - C^A_s, so both ends see the same
 * bits of s_st, d_st and h_st.  Swapping the two robots therefore swaps dist_a with dist_b and nearest_a with nearest_b bit for
 * bit; E and the gradients change in the order of their sums only.
 *
 * LIMITS.  A block holds up to 16 frames; a frame's working set in LDS, in values of the arithmetic type (n_slot the fork
 * slots of a pose table, n_jx its joints driven by x, S the spheres):
 *
 *   distances      12 (n_slot_a + n_slot_b) + 3 (S_a + S_b) + 24                                       the two base poses: 24
 *   penalty        12 (n_slot_a + n_slot_b) + 9 (S_a + S_b) + 24 + 16 + 192 + 6 (n_jx_a + n_jx_b)      world centres, forces, root-frame
 *   distance VJP   the penalty's + S_a + S_b                                                           centres: 9 S; the nearest indices
 *
 * (16 partial energies, 2 x 6 x 16 partial wrench sums, an axis and an origin per joint driven by x), rounded up to an odd
 * count.  The frames per block are halved until the block fits 64 KB.  The largest pair of models within the table limits, 128
 * spheres against 128 with 64 joints and 8 fork slots each, needs 3 497 values for the penalty (27 976 B in float64: two frames
 * per block; 13 988 B in float32: four) and 3 753 for the VJP (30 024 B in float64: two frames per block); a frame that does
 * not fit a block alone would be refused with DEXR_ERR_UNSUPPORTED and the byte count (none within the limits is).
 */
#ifndef DEXR_CROSS_H
#define DEXR_CROSS_H

#include "dexr_spheres.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_CROSS_FRAMES 16   /* most frames of a block */
#define DEXR_CROSS_LDS 65536   /* bytes of LDS a block may use */

/* DEXR_ERR_INVALID before any launch: a null model; B < 0; x_a / fixed_a / x_b / fixed_b NULL where that robot's table reads
 * them; a margin that is negative or not finite; every output of a call NULL (distances, penalty); a NULL grad_xa_out or
 * grad_xb_out of the VJP where that robot's n_in > 0. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * -> dist_a_out (B, S_a), nearest_a_out (B, S_a) int32, dist_b_out (B, S_b), nearest_b_out (B, S_b) int32: each may be NULL,
 * not all four. */
int dexr_cross_distances_dev(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const float* x_a, const float* fixed_a,
                             const float* x_b, const float* fixed_b, const float* pos_a, const float* rot_a, const float* pos_b,
                             const float* rot_b, float* dist_a_out, int32_t* nearest_a_out, float* dist_b_out, int32_t* nearest_b_out,
                             void* stream);
/* grad_dist_a (B, S_a) or NULL, grad_dist_b (B, S_b) or NULL -> grad_xa_out (B, n_in_a), grad_xb_out (B, n_in_b), and
 * wrench_a_out, wrench_b_out (B, 6), either or both of which may be NULL.  The kinematics, the nearest spheres and their
 * normals are recomputed. */
int dexr_cross_distances_vjp_dev(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const float* x_a, const float* fixed_a,
                                 const float* x_b, const float* fixed_b, const float* pos_a, const float* rot_a, const float* pos_b,
                                 const float* rot_b, const float* grad_dist_a, const float* grad_dist_b, float* grad_xa_out,
                                 float* grad_xb_out, float* wrench_a_out, float* wrench_b_out, void* stream);
/* pair_weight (S_a, S_b) or NULL -> energy_out (B), grad_xa_out (B, n_in_a), grad_xb_out (B, n_in_b), wrench_a_out (B, 6),
 * wrench_b_out (B, 6): each may be NULL, not all five. */
int dexr_cross_penalty_dev(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const float* x_a, const float* fixed_a,
                           const float* x_b, const float* fixed_b, const float* pos_a, const float* rot_a, const float* pos_b,
                           const float* rot_b, float margin, const float* pair_weight, float* energy_out, float* grad_xa_out,
                           float* grad_xb_out, float* wrench_a_out, float* wrench_b_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_cross_distances(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const double* x_a, const double* fixed_a,
                         const double* x_b, const double* fixed_b, const double* pos_a, const double* rot_a, const double* pos_b,
                         const double* rot_b, double* dist_a_out, int32_t* nearest_a_out, double* dist_b_out, int32_t* nearest_b_out);
int dexr_cross_distances_vjp(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const double* x_a, const double* fixed_a,
                             const double* x_b, const double* fixed_b, const double* pos_a, const double* rot_a, const double* pos_b,
                             const double* rot_b, const double* grad_dist_a, const double* grad_dist_b, double* grad_xa_out,
                             double* grad_xb_out, double* wrench_a_out, double* wrench_b_out);
int dexr_cross_penalty(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const double* x_a, const double* fixed_a,
                       const double* x_b, const double* fixed_b, const double* pos_a, const double* rot_a, const double* pos_b,
                       const double* rot_b, double margin, const double* pair_weight, double* energy_out, double* grad_xa_out,
                       double* grad_xb_out, double* wrench_a_out, double* wrench_b_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_CROSS_H */

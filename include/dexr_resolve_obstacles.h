/* dexr_resolve_obstacles.h -- the collision-aware posture solve of dexr_resolve.h with one more energy term: the robot's spheres
 * against the posed primitives of an obstacle set of dexr_obstacles.h.  One launch projects postures out of self-penetration AND
 * out of a held object or a scene, stays near a reference posture and keeps chosen links at world targets; every iterate, the
 * forces, both contact lists, the normal matrix, its factor and the per-frame damping stay on chip.  C ABI; no handle of its own:
 * every function takes a dexr_sphere_model and a dexr_obstacle_set.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  Everything of dexr_resolve.h holds unchanged: the variables, the freeze rule, the damping factors, the step limit,
 * the clamp, the stop rules, iters, and "the answer is an accepted point".  One term is added, with d_sm, n_sm, w_m of
 * dexr_obstacles.h (s a sphere, m a primitive of the set):
 *
 *   E      = ((E_pose + E_post) + E_col) + E_obs            (this order of addition)
 *   E_obs  = w_obs sum_s sum_m w_m h_sm^2,   h_sm = max(0, obstacle_margin - d_sm)
 *   g     += w_obs sum_{s,m} w_m h_sm grad d_sm,            grad d_sm [c] = n_sm . Jpt_s[:, c]
 *   H     += w_obs sum over the curvature contacts of w_m (grad d_sm)(grad d_sm)^T
 *
 * The ACTIVE CONTACTS of a frame are the (s, m) with h_sm > 0, ordered by the CALLER's sphere index, then by the primitive's index
 * in the set.  Energy and gradient use every one of them, the curvature the first DEXR_RESOLVE_MAXCONTACT of that order.  If any
 * evaluated point (x0 or a trial) has more, status |= DEXR_RESOLVE_CONTACTS_TRUNCATED.  The pair side keeps its own list, its own
 * cap (DEXR_RESOLVE_MAXACTIVE) and its own bit (DEXR_RESOLVE_TRUNCATED).  A contact without a direction (n_sm = 0: the centre of a
 * sphere on a sphere primitive's centre or on a capsule's axis) contributes energy only.
 *
 * The obstacle pose of a frame is fixed during the solve.  obstacle_pos (B, 3) and obstacle_rot (B, 3, 3) follow the NULL rules of
 * dexr_obstacles.h: NULL is zero translation / the identity, with the same bits as explicit zeros / identities.  prim_weight
 * (n_prim) >= 0 (not checked) is shared by the batch, NULL means 1.
 *
 * EVERY entry of every output is written.  A non-finite input (an obstacle pose included) spoils its own frame only; that frame
 * ends within max_iters trial steps.  The outputs of a frame do not depend on B, on where the frame sits in the batch, or on when
 * the frames beside it stop, bit for bit: every sum is taken by one thread in a fixed order and there are no atomics.
 *
 * LDS.  A block holds 16 frames, halved until its working set fits 64 KB.  With v = 4 (float32) or 8 (float64) bytes a value,
 * n_jx the joints driven by x, n_act the active columns, n_tri = n_act (n_act + 1) / 2 and L = 11 n_link with targets, else 0,
 * one frame needs
 *
 *   values = (6 n_jx + L + 6 n_sphere + 16 + max(n_tri, 16 n_act + 16) + n_tri + 4 n_act + 2 n_in + 8 + 12 + 16) | 1
 *   bytes  = 128 + 8 n_sphere + v (12 n_slot + values) + 4 (DEXR_RESOLVE_MAXACTIVE + 22) + 4 * 17 + 2 DEXR_RESOLVE_MAXCONTACT
 *            + ((n_pair + 3) & ~3)
 *
 * (dexr_resolve.h's working set, a parked obstacle pose, sixteen more partial energies, a 64-bit contact mask per sphere, the
 * contact list and its counts).  A model whose one frame does not fit is refused with DEXR_ERR_UNSUPPORTED and the message states
 * `bytes`.  The largest model within the table limits, which dexr_resolve.h holds in 64 608 B in float64, needs 66 436 B here and
 * is refused in float64; in float32 it needs 38 704 B (one frame per block).
 */
#ifndef DEXR_RESOLVE_OBSTACLES_H
#define DEXR_RESOLVE_OBSTACLES_H

#include "dexr_obstacles.h"
#include "dexr_resolve.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_RESOLVE_MAXCONTACT 256 /* active (sphere, primitive) contacts of a frame that enter the curvature */

#define DEXR_RESOLVE_CONTACTS_TRUNCATED 8 /* some evaluated point had more than DEXR_RESOLVE_MAXCONTACT active contacts */

/* DEXR_ERR_INVALID before any launch: every rule of dexr_resolve.h, a null obstacle set, an obstacle_margin or obstacle_weight
 * that is negative or not finite. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.  The arguments of
 * dexr_sphere_resolve_dev, then the obstacle set, obstacle_pos (B, 3) or NULL, obstacle_rot (B, 3, 3) row-major or NULL,
 * obstacle_margin, obstacle_weight (w_obs), prim_weight (n_prim) or NULL -> x_out (B, n_in), iters_out (B) int32 or NULL,
 * energy_out (B, 4): E_pose, E_post, E_col, E_obs at x_out, or NULL, status_out (B) int32 or NULL.  x_out may alias x0. */
int dexr_sphere_resolve_obstacles_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                      const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                      const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                      const float* pair_weight, const float* lo, const float* hi, float damping, float max_step,
                                      float tol, int32_t max_iters, const dexr_obstacle_set* obstacles, const float* obstacle_pos,
                                      const float* obstacle_rot, float obstacle_margin, float obstacle_weight, const float* prim_weight,
                                      float* x_out, int32_t* iters_out, float* energy_out, int32_t* status_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_sphere_resolve_obstacles(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                                  const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                                  const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                                  const double* pair_weight, const double* lo, const double* hi, double damping, double max_step,
                                  double tol, int32_t max_iters, const dexr_obstacle_set* obstacles, const double* obstacle_pos,
                                  const double* obstacle_rot, double obstacle_margin, double obstacle_weight, const double* prim_weight,
                                  double* x_out, int32_t* iters_out, double* energy_out, int32_t* status_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_RESOLVE_OBSTACLES_H */

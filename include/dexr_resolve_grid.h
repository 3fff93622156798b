/* dexr_resolve_grid.h -- the collision-aware posture solve of dexr_resolve.h with one more energy term: the robot's spheres against
 * one sampled signed-distance field of dexr_sdf_grid.h -- a mesh, a scan, a depth fusion.  One launch projects postures out of
 * self-penetration AND out of that object or scene, stays near a reference posture and keeps chosen links at world targets; every
 * iterate, the forces, both contact lists, the normal matrix, its factor and the per-frame damping stay on chip; the samples stay
 * in global memory, one trilinear lookup per sphere and evaluated point.  C ABI; no handle of its own: every function takes a
 * dexr_sphere_model and a dexr_sdf_grid.  It is the sibling of dexr_resolve_obstacles.h, whose primitives a grid replaces.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  Everything of dexr_resolve.h holds unchanged: the variables, the freeze rule, the damping factors, the step limit,
 * the clamp, the stop rules, iters, and "the answer is an accepted point".  One term is added, with d_s and n_s of dexr_sdf_grid.h
 * (s a sphere: d_s = sdf(R_o^T (c_s - p_o)) - r_s, n_s = R_o grad sdf, the clamped continuation outside the grid's box included):
 *
 *   E      = ((E_pose + E_post) + E_col) + E_obs            (this order of addition)
 *   E_obs  = w_obs sum_s h_s^2,              h_s = max(0, obstacle_margin - d_s)
 *   g     += w_obs sum_s h_s grad d_s,                      grad d_s [c] = n_s . Jpt_s[:, c]
 *   H     += w_obs sum over the active spheres of (grad d_s)(grad d_s)^T
 *
 * The ACTIVE CONTACTS of a frame are the spheres with h_s > 0, in the CALLER's sphere order.  A sphere has at most ONE contact with
 * a grid and a model at most DEXR_SPHERE_MAX = 128 spheres: energy, gradient AND curvature use every contact, there is no cap, and
 * DEXR_RESOLVE_CONTACTS_TRUNCATED of dexr_resolve_obstacles.h is never set.  status uses DEXR_RESOLVE_CONVERGED, DEXR_RESOLVE_STALLED
 * and DEXR_RESOLVE_TRUNCATED (the pair side keeps its list, its cap DEXR_RESOLVE_MAXACTIVE and its bit) only.  A contact without a
 * direction (n_s = 0: a flat spot of the samples) contributes energy only.  The gradient of a trilinear field jumps across cell
 * faces and the planes of the grid's box; E stays continuous, and the accept / reject rule holds the descent as it does anywhere.
 *
 * The obstacle pose of a frame is fixed during the solve.  obstacle_pos (B, 3) and obstacle_rot (B, 3, 3) follow the NULL rules of
 * dexr_sdf_grid.h: NULL is zero translation / the identity, with the same bits as explicit zeros / identities.
 *
 * EVERY entry of every output is written.  A non-finite input (an obstacle pose included) spoils its own frame only; that frame
 * ends within max_iters trial steps, and no input makes a load leave the samples.  The outputs of a frame do not depend on B, on
 * where the frame sits in the batch, or on when the frames beside it stop, bit for bit: every sum is taken by one thread in a
 * fixed order and there are no atomics.
 *
 * LDS.  A block holds 16 frames, halved until its working set fits 64 KB.  With v = 4 (float32) or 8 (float64) bytes a value,
 * n_jx the joints driven by x, n_act the active columns, n_tri = n_act (n_act + 1) / 2 and L = 11 n_link with targets, else 0,
 * one frame needs
 *
 *   values = (6 n_jx + L + 6 n_sphere + 16 + max(n_tri, 16 n_act + 16) + n_tri + 4 n_act + 2 n_in + 8 + 12 + 16) | 1
 *   bytes  = 128 + v (12 n_slot + values) + 4 (DEXR_RESOLVE_MAXACTIVE + 22) + 4 * 17 + 2 ((n_sphere + 3) & ~3)
 *            + ((n_pair + 3) & ~3)
 *
 * (dexr_resolve.h's working set, a parked obstacle pose, sixteen more partial energies, the contact counts, and per sphere one
 * byte of active flag and one byte of contact list: the normal of a contact is recomputed from the parked centre, not parked).  A
 * model whose one frame does not fit is refused with DEXR_ERR_UNSUPPORTED and the message states `bytes`.  No model within the table
 * limits is refused: the largest one (128 spheres, 8 128 pairs), which dexr_resolve.h holds in 64 608 B in float64 and
 * dexr_resolve_obstacles.h refuses there, needs 65 156 B here in float64 and 37 424 B in float32 (one frame per block).
 */
#ifndef DEXR_RESOLVE_GRID_H
#define DEXR_RESOLVE_GRID_H

#include "dexr_sdf_grid.h"
#include "dexr_resolve.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DEXR_ERR_INVALID before any launch: every rule of dexr_resolve.h, a null grid, an obstacle_margin or obstacle_weight that is
 * negative or not finite. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.  The arguments of
 * dexr_sphere_resolve_dev up to max_iters, then the grid, obstacle_pos (B, 3) or NULL, obstacle_rot (B, 3, 3) row-major or NULL,
 * obstacle_margin, obstacle_weight (w_obs) -> x_out (B, n_in), iters_out (B) int32 or NULL, energy_out (B, 4): E_pose, E_post,
 * E_col, E_obs at x_out, or NULL, status_out (B) int32 or NULL.  x_out may alias x0. */
int dexr_sphere_resolve_grid_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                 const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                 const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                 const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                                 int32_t max_iters, const dexr_sdf_grid* grid, const float* obstacle_pos, const float* obstacle_rot,
                                 float obstacle_margin, float obstacle_weight, float* x_out, int32_t* iters_out, float* energy_out,
                                 int32_t* status_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device, the float32 samples widened on load): copy, run,
 * synchronise. */
int dexr_sphere_resolve_grid(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                             const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                             const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                             const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                             int32_t max_iters, const dexr_sdf_grid* grid, const double* obstacle_pos, const double* obstacle_rot,
                             double obstacle_margin, double obstacle_weight, double* x_out, int32_t* iters_out, double* energy_out,
                             int32_t* status_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_RESOLVE_GRID_H */

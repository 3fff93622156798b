/* dexr_resolve_scene.h -- the collision-aware posture solve of dexr_resolve.h against a SCENE: up to DEXR_SCENE_MAXBODY bodies, each
 * an obstacle set of dexr_obstacles.h or a sampled signed-distance field of dexr_sdf_grid.h, each with a pose per frame (or none), a
 * margin and a weight of its own -- a hand holding an object that sits on a table, a world-fixed fixture together with a held
 * object, primitives and a scanned mesh together.  One launch projects postures out of self-penetration AND out of every body at
 * once: one energy, one descent; the single-body solves of dexr_resolve_obstacles.h and dexr_resolve_grid.h run one after the other
 * each push the hand back into the body they do not know.  Every iterate, the forces, both contact lists, the normal matrix, its
 * factor and the per-frame damping stay on chip.  C ABI; no handle of its own: every function takes a dexr_sphere_model and the
 * bodies' dexr_obstacle_set / dexr_sdf_grid handles.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * DEFINITION.  Everything of dexr_resolve.h holds unchanged: the variables, the freeze rule, the damping factors, the step limit,
 * the clamp, the stop rules, iters, and "the answer is an accepted point".  A scene is n_body bodies, 1 <= n_body <=
 * DEXR_SCENE_MAXBODY; body b has its own obstacle_pos_b (B, 3) and obstacle_rot_b (B, 3, 3) with the NULL rules of dexr_obstacles.h
 * (NULL is zero translation / the identity, with the same bits as explicit zeros / identities), margin_b >= 0, weight_b >= 0 and,
 * a set alone, prim_weight_b (n_prim) or NULL (weights of 1):
 *
 *   E      = ((E_pose + E_post) + E_col) + E_obs            (this order of addition)
 *   E_obs  = (((E_0 + E_1) + E_2) + E_3)                    (body order, as many as there are)
 *   E_b    = weight_b sum of w_m h^2 over body b: exactly the E_obs of dexr_resolve_obstacles.h (a set) or of dexr_resolve_grid.h
 *            (a grid) with obstacle_margin = margin_b, w_obs = weight_b and the pose of body b
 *   g, H  += the same bodies' terms, as those two headers define them
 *
 * The ACTIVE CONTACTS of a frame are ordered by the CALLER's sphere index, then by the body index, then by the primitive's index
 * inside a set; a grid has one contact per sphere at most.  Energy and gradient use every one of them, the curvature the first
 * DEXR_RESOLVE_MAXCONTACT (256) of that order OVER ALL BODIES TOGETHER.  If any evaluated point (x0 or a trial) has more, status |=
 * DEXR_RESOLVE_CONTACTS_TRUNCATED.  GRIDS TAKE PART IN THIS CAP HERE: four grids and 128 spheres can make 512 contacts.  This
 * differs from dexr_resolve_grid.h, whose one grid has at most DEXR_SPHERE_MAX contacts, no cap and never sets the bit.  The pair
 * side keeps its own list, its own cap (DEXR_RESOLVE_MAXACTIVE) and its own bit (DEXR_RESOLVE_TRUNCATED).  A contact without a
 * direction (a zero normal) contributes energy only.
 *
 * The pose of every body of a frame is fixed during the solve.
 *
 * OUTPUTS, each of which may be NULL except x_out: x_out (B, n_in), iters_out (B) int32, energy_out (B, 4): E_pose, E_post, E_col,
 * E_obs at x_out, body_energy_out (B, n_body): E_b at x_out, status_out (B) int32.  EVERY entry of every output is written.  A
 * non-finite input (any body's pose included) spoils its own frame only; that frame ends within max_iters trial steps, and no
 * input makes a load leave a grid's samples.  The outputs of a frame do not depend on B, on where the frame sits in the batch, or
 * on when the frames beside it stop, bit for bit: every sum is taken by one thread in a fixed order and there are no atomics.
 *
 * LDS.  A block holds 16 frames, halved until its working set fits 64 KB.  With v = 4 (float32) or 8 (float64) bytes a value,
 * n_jx the joints driven by x, n_act the active columns, n_tri = n_act (n_act + 1) / 2 and L = 11 n_link with targets, else 0,
 * one frame needs
 *
 *   values = (6 n_jx + L + 6 n_sphere + 16 + max(n_tri, 16 n_act + 16) + n_tri + 4 n_act + 2 n_in + 8 + 30 n_body) | 1
 *   bytes  = 128 + 8 n_body n_sphere + v (12 n_slot + values) + 4 (DEXR_RESOLVE_MAXACTIVE + 22) + 4 * 17
 *            + 2 DEXR_RESOLVE_MAXCONTACT + ((n_pair + 3) & ~3)
 *
 * (dexr_resolve.h's working set; per body a parked pose, sixteen partial energies, its energy at the trial and at the accepted
 * point, and a 64-bit contact mask per sphere; the contact list, 16 bits an entry, and its counts).  A one-body scene needs 8 B
 * (float32) or 16 B (float64) more than dexr_resolve_obstacles.h.  A model whose one frame does not fit is refused with
 * DEXR_ERR_UNSUPPORTED and the message states `bytes`.  The largest model within the table limits (128 spheres, 8 128 pairs), which
 * dexr_resolve.h holds in 64 608 B in float64, is refused in float64 with any scene (one body: 66 452 B, four bodies: 70 244 B); in
 * float32 it needs 38 712 B with one body and 42 144 B with four (one frame per block).
 */
#ifndef DEXR_RESOLVE_SCENE_H
#define DEXR_RESOLVE_SCENE_H

#include "dexr_resolve_obstacles.h"
#include "dexr_sdf_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_SCENE_MAXBODY 4 /* bodies of a scene */

typedef struct dexr_scene_body {
  const dexr_obstacle_set* set; /* exactly one of set / grid is non-NULL */
  const dexr_sdf_grid* grid;
  const void* pos;         /* (B, 3) or NULL;    float32 device (the _dev entry point) / float64 host (the host twin) */
  const void* rot;         /* (B, 3, 3) row-major or NULL */
  const void* prim_weight; /* (n_prim) or NULL; NULL for a grid */
  double margin, weight;   /* margin_b, weight_b: finite and >= 0 */
} dexr_scene_body;

/* DEXR_ERR_INVALID before any launch: every rule of dexr_resolve.h, n_body outside 1..DEXR_SCENE_MAXBODY, a NULL `bodies`, a body
 * with both or neither of set / grid, a prim_weight on a grid, a margin or weight that is negative or not finite.  The scene's
 * rules and the scalar rules of dexr_resolve.h are checked at B == 0 too, as the single-body entry points check their obstacle
 * there: B == 0 is the no-op returning 0 for a call that passes them (NULL x0, fixed and outputs included); B == 0 with a NULL
 * `bodies` is DEXR_ERR_INVALID. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.  The arguments of
 * dexr_sphere_resolve_dev up to max_iters, then n_body and `bodies`, a HOST array of n_body records read during the call (their
 * pos, rot and prim_weight are device pointers, float32) -> the outputs above.  x_out may alias x0. */
int dexr_sphere_resolve_scene_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                  const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                  const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                  const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                                  int32_t max_iters, int32_t n_body, const dexr_scene_body* bodies, float* x_out, int32_t* iters_out,
                                  float* energy_out, float* body_energy_out, int32_t* status_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device, a grid's float32 samples widened on load; the bodies' pos,
 * rot and prim_weight are host pointers, float64): copy, run, synchronise. */
int dexr_sphere_resolve_scene(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                              const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                              const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                              const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                              int32_t max_iters, int32_t n_body, const dexr_scene_body* bodies, double* x_out, int32_t* iters_out,
                              double* energy_out, double* body_energy_out, int32_t* status_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_RESOLVE_SCENE_H */

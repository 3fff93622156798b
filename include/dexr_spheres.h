/* dexr_spheres.h -- self-collision of a sphere approximation on a pose table (dexr_pose.h): batched signed distances of sphere
 * pairs, their vector-Jacobian product, and a fused penalty that returns the energy and its gradient in x from ONE launch, in
 * which neither distances nor forces nor normals reach memory.  C ABI.  A sphere model is a handle of its own: it owns the
 * dexr_pose_model of its link list and the sphere and pair tables beside it.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h; B == 0 is a no-op returning 0.  The library reads no environment variable.
 *
 * SPHERE MODEL.  A pose table (its links are the rows 0 .. n_link-1 of the caller's link list) and
 *
 *   n_sphere spheres, 1 .. DEXR_SPHERE_MAX:    sphere_link[s]  a row of the link list
 *                                              center[s]       3 values, in that link's frame
 *                                              radius[s]       >= 0
 *   n_pair pairs (i, j) of sphere indices, 1 .. DEXR_SPHERE_MAXPAIR (128 spheres with every pair, 8128, fit): i != j; a pair
 *   listed twice counts twice.
 *
 * DEFINITION.  Per frame, with p_l, R_l the world pose of link l (dexr_link_poses):
 *
 *   c_s = p_l(s) + R_l(s) center_s
 *   D = c_i - c_j,   s_p = |D|,   d_p = s_p - (r_i + r_j),   n_p = s_p > 0 ? D / s_p : 0     (coincident centres: no direction, no NaN)
 *   dd_p/dx_c = n_p . (Jpt_i[:,c] - Jpt_j[:,c]),    Jpt_s[:,c] = Jlin_l[:,c] + Jang_l[:,c] x (c_s - p_l)
 *                                                   (Jlin, Jang of dexr_jacobian.h, DEXR_JAC_WORLD_ALIGNED)
 *
 *   distances      dist[b,p] = d_p                                   centers[b,s] = c_s   (optional output)
 *   distance VJP   grad_x[b,c] = sum_p grad_dist[b,p] dd_p/dx_c
 *   penalty        h_p = max(0, margin - d_p),   E[b] = sum_p w_p h_p^2,   grad_x[b,c] = sum_p (-2 w_p h_p) dd_p/dx_c
 *
 * margin >= 0 and finite.  w (n_pair) is shared by the batch and must be >= 0 (not checked); NULL means 1.  The hinge is
 * squared on purpose: E is C1, so a pair that float32 rounding puts on one side or the other of the margin changes neither E
 * nor the gradient by more than rounding.
 *
 * No Jacobian is formed.  With f_s = sum over the pairs at sphere s of g_p (c_s - c_other) / s_p (g_p = grad_dist[b,p], or
 * -2 w_p h_p), the force on sphere s, a joint k driven by x (world axis a_k, world origin o_k) takes
 *
 *   dL/dq_k = sum over the spheres s below joint k of   a_k . ((c_s - o_k) x f_s)   revolute      a_k . f_s   prismatic
 *   grad_x[col_k] += mult_k dL/dq_k
 *
 * The rest is dexr_wrench.h's: mimic joints land on the column of their source with their multiplier; joints driven by `fixed`
 * or by a constant move the geometry and receive no gradient; a sphere on the fixed base moves with nothing, but its pairs
 * count; columns no joint reads are exact zeros.  EVERY entry of every output is written.  A non-finite input spoils its own
 * frame only.  The outputs of a frame do not depend on B or on where the frame sits in the batch, bit for bit: every sum has a
 * fixed order (per sphere its pairs in list order, per column its joints in walk order and their spheres in table order, the
 * energy as sixteen partial sums added in order) and there are no atomics.  The penalty's gradient agrees with the VJP fed
 * with -2 w h to rounding, not bit for bit.
 *
 * A model whose per-frame working set (12 n_slot + 6 n_jx + 6 n_sphere + 17 values, n_jx the joints driven by x) does not fit
 * the 64 KB of LDS of a block of one frame is refused with DEXR_ERR_UNSUPPORTED (none within the limits is: 8 slots, 64 joints
 * and 128 spheres need 10 120 B per frame in float64, four frames per block).
 */
#ifndef DEXR_SPHERES_H
#define DEXR_SPHERES_H

#include "dexr_pose.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_SPHERE_MAX 128      /* spheres per model */
#define DEXR_SPHERE_MAXPAIR 8192 /* pairs per model */

typedef struct dexr_sphere_model dexr_sphere_model;

/* pose_blob / nbytes: a pose table as dexr_pose_model_create takes it (the model builds and owns its pose model).
 * sphere_link (n_sphere) int32, center (n_sphere, 3) and radius (n_sphere) float64, pair (n_pair, 2) int32.  The blob, then
 * the sphere and the pair arrays are validated before the first HIP call: a malformed blob, a count out of range, a link row
 * or a sphere index out of range, i == j, a non-finite centre, a non-finite or negative radius and a null argument are
 * DEXR_ERR_INVALID.  A well-formed input needs a device (the tables are uploaded): DEXR_ERR_HIP without one. */
int dexr_sphere_model_create(const void* pose_blob, size_t nbytes, int32_t n_sphere, const int32_t* sphere_link,
                             const double* center, const double* radius, int32_t n_pair, const int32_t* pair,
                             dexr_sphere_model** out);
void dexr_sphere_model_destroy(dexr_sphere_model* m);
int dexr_sphere_model_info(const dexr_sphere_model* m, int32_t* n_in, int32_t* n_fixed, int32_t* n_sphere, int32_t* n_pair);

/* DEXR_ERR_INVALID before any launch: a null model, B < 0, x / fixed NULL where the table reads them, a NULL dist_out /
 * grad_dist / grad_x_out (where n_in > 0), a margin that is negative or not finite, energy_out and grad_x_out both NULL. */

/* Device pointers, float32, C-contiguous; enqueued on `stream`; never synchronise, never allocate.
 * x (B, n_in), fixed (B, n_fixed) or NULL when n_fixed == 0 -> dist_out (B, n_pair), center_out (B, n_sphere, 3) or NULL. */
int dexr_sphere_distances_dev(const dexr_sphere_model* m, int64_t B, const float* x, const float* fixed, float* dist_out,
                              float* center_out /* may be NULL */, void* stream);
/* grad_dist (B, n_pair) -> grad_x_out (B, n_in).  The kinematics are recomputed from x. */
int dexr_sphere_distances_vjp_dev(const dexr_sphere_model* m, int64_t B, const float* x, const float* fixed,
                                  const float* grad_dist, float* grad_x_out, void* stream);
/* pair_weight (n_pair) or NULL -> energy_out (B) and / or grad_x_out (B, n_in): either may be NULL, not both. */
int dexr_sphere_penalty_dev(const dexr_sphere_model* m, int64_t B, const float* x, const float* fixed, float margin,
                            const float* pair_weight, float* energy_out, float* grad_x_out, void* stream);

/* Host pointers, float64 in and out (float64 arithmetic on the device): copy, run, synchronise. */
int dexr_sphere_distances(const dexr_sphere_model* m, int64_t B, const double* x, const double* fixed, double* dist_out,
                          double* center_out);
int dexr_sphere_distances_vjp(const dexr_sphere_model* m, int64_t B, const double* x, const double* fixed,
                              const double* grad_dist, double* grad_x_out);
int dexr_sphere_penalty(const dexr_sphere_model* m, int64_t B, const double* x, const double* fixed, double margin,
                        const double* pair_weight, double* energy_out, double* grad_x_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_SPHERES_H */

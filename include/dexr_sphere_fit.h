/* dexr_sphere_fit.h -- a few spheres inside a body, chosen from the samples of its signed-distance field: the stage behind
 * dexr_mesh_sdf.h (a mesh -> a grid of samples) and in front of dexr_spheres.h (spheres on links -> distances, penalties, solves).
 * A greedy set cover: every round takes the inscribed sphere that covers the most interior samples no earlier sphere covers.
 * Several bodies (the links of a hand) are fitted by one call.  C ABI.
 *
 * Conventions of dexr.h: every function but dexr_sphere_fit_workspace_bytes returns DEXR_OK (0) or a negative DEXR_ERR_* code, the
 * message is read through dexr_last_error of dexr.h.  Everything is validated before the first HIP call.  The library reads no
 * environment variable.
 *
 * A BODY is a grid of float32 samples v of shape (nx, ny, nz) in C order (iz the fastest) with ONE spacing h for its three axes,
 * each dimension DEXR_SPHERE_FIT_MIN_DIM .. DEXR_SPHERE_FIT_MAX_DIM.  Where the samples sit in space does not matter here: a sphere
 * is returned as the flat index of the sample at its centre.  Everything compared is an integer:
 *
 *   interior    v < 0 (a NaN is not interior)
 *   candidate   an interior sample with (double)(-v) >= min_radius
 *   reach       t = ((double)(-v) + inflate) / h,   m = floor(t * t)      float64, each operation rounded once, the product a
 *               single product (nothing to fuse); m is an integer, and a value above 2^31 - 1 counts as 2^31 - 1 (the squared
 *               distance of two samples of a grid is below 2^14: such a sphere covers the grid either way)
 *   coverage    candidate c covers interior sample j  iff  |i_j - i_c|^2 <= m_c, the integer squared distance of the index triples
 *
 * that is "sample j lies in the ball of radius -v_c + inflate about sample c" without a floating comparison per pair.  With
 * inflate = 0 and v the exact distance to the surface the ball lies wholly inside the body; with inflate > 0 it protrudes by at
 * most inflate.
 *
 * THE ROUNDS of a body, k = 0 .. K - 1 with K its sphere count (1 .. DEXR_SPHERE_MAX):
 *
 *   1 stop before the round when  n_covered >= ceil(coverage * n_interior)  (a float64 product, then ceil)
 *   2 gain_c = the number of interior samples not yet covered that c covers (c itself among them, while it is uncovered)
 *   3 the winner has the largest gain; among equal gains the larger m; among those the lower flat index
 *   4 stop when the winner's gain is 0; otherwise record its flat index and its gain and mark its samples covered
 *
 * OUTPUTS, all int32 and every entry written: index_out and gain_out (n_body, k_max) with k_max = the largest K of the call, unused
 * slots -1 and 0; count_out (n_body, 3) = (n_interior, n_covered, n_spheres).  A body without an interior sample gives no sphere and
 * is no error.  Centres (origin + index * h) and radii (-v + inflate) are the caller's to form, in float64, from the indices.
 *
 * THE KERNELS.  The uncovered interior samples of a body are a bit mask: one 64-bit word per (ix, iy) row, bit iz; at most 32 KB.
 * It lives in the workspace between launches and in LDS inside the gain kernel.  One launch builds mask, m and the candidate flag of
 * all bodies; then every round is two launches for all bodies at once, on the caller's stream, with nothing read back in between:
 *
 *   gain    blocks (chunk of DEXR_SPHERE_FIT_CHUNK samples, body).  A block copies its body's mask into LDS; a thread owns
 *           candidates and for each walks the rows (dx, dy) with dx^2 + dy^2 <= m that lie in the grid: the half width
 *           w = isqrt(m - dx^2 - dy^2) (an integer square root corrected by comparison), the row's word, the bits iz - w .. iz + w
 *           clipped to the grid, a population count.  The block's largest (gain, m, ~index) goes to the block's slot.
 *   apply   one block per body: the largest of the slots is the winner; the stop rules; the outputs; the winner's bits are cleared
 *           from the mask in the workspace by the same row arithmetic.
 *
 * A body that has stopped costs its blocks one load.  There are no atomics and no sums whose order could vary: the outputs are a
 * function of the inputs alone, and a body's do not depend on which bodies share its call.
 */
#ifndef DEXR_SPHERE_FIT_H
#define DEXR_SPHERE_FIT_H

#include <stddef.h>
#include <stdint.h>

#include "dexr_spheres.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_SPHERE_FIT_MIN_DIM 2
#define DEXR_SPHERE_FIT_MAX_DIM 64    /* per axis: a row of samples along z is one 64-bit word */
#define DEXR_SPHERE_FIT_MAX_BODIES 64 /* the link limit of a sphere set */
#define DEXR_SPHERE_FIT_CHUNK 1024    /* samples of one block of the gain kernel: 256 threads, four samples each */

/* Bytes of workspace a call on n_body bodies of dims (n_body, 3) needs; 0 (and a message) where n_body or a dimension is out of
 * range or dims is NULL.  Never touches a device. */
size_t dexr_sphere_fit_workspace_bytes(int32_t n_body, const int32_t* dims);

/* HOST arrays: dims (n_body, 3) int32; spacing (n_body) float64; offset (n_body) int64, body b's samples start at values + offset[b];
 * k (n_body) int32, the sphere count of each body.  Scalars for all bodies: min_radius, inflate, coverage.
 * DEVICE pointers: values (n_values) float32; index_out, gain_out (n_body, max k) int32; count_out (n_body, 3) int32; workspace of
 * workspace_bytes >= dexr_sphere_fit_workspace_bytes(n_body, dims) bytes, 16-byte aligned, contents irrelevant and reusable by the
 * next call on the same stream.  Enqueued on `stream`; never synchronises, never allocates.
 *
 * DEXR_ERR_INVALID before any launch: a null pointer; n_body outside 1 .. DEXR_SPHERE_FIT_MAX_BODIES; a dimension out of range; a
 * spacing that is not finite or not > 0; an offset below 0 or a body that ends past n_values; k outside 1 .. DEXR_SPHERE_MAX;
 * min_radius or inflate not finite or below 0; coverage outside 0 .. 1 (a NaN included); a workspace too small or misaligned. */
int dexr_sphere_fit_dev(int32_t n_body, const int32_t* dims, const double* spacing, const int64_t* offset, const int32_t* k, double min_radius,
                        double inflate, double coverage, int64_t n_values, const float* values, int32_t* index_out, int32_t* gain_out,
                        int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same with values and the three outputs on the host: copy, run, synchronise; allocates its own workspace. */
int dexr_sphere_fit(int32_t n_body, const int32_t* dims, const double* spacing, const int64_t* offset, const int32_t* k, double min_radius,
                    double inflate, double coverage, int64_t n_values, const float* values, int32_t* index_out, int32_t* gain_out,
                    int32_t* count_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_SPHERE_FIT_H */

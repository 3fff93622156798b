/* dexr_sdf_grid_dev.h -- a dexr_sdf_grid of dexr_sdf_grid.h whose samples are produced ON the device: the handle is created around
 * device memory of its own, a producer writes the samples through a device pointer on a stream of its own ordering, and every
 * consumer of a dexr_sdf_grid -- the distances, their VJP, the fused penalty, the posture solves against a grid and against a scene --
 * takes the handle as it takes one made from host samples.  No kernel of those is changed.  C ABI, the conventions of dexr.h.
 *
 * The handle is destroyed with the destroy function of dexr_sdf_grid.h and described by its info function.  (The three entry points
 * live in a header of their own so that dexr_sdf_grid.h stays exactly the list of symbols it was.)
 *
 * THE CONTRACT OF THE SAMPLES.  The create function of dexr_sdf_grid.h refuses a sample that is not finite, because the grid kernels
 * promise that no finite input produces a non-finite output.  Samples written through dexr_sdf_grid_values_dev are never inspected:
 * keeping every one of them finite is the CALLER's contract.  The distance-transform entries of dexr_distance_transform.h always
 * honour it (their clamp to max_distance makes every sample finite whatever the input).  A grid created with values_dev == NULL
 * holds zeros.
 *
 * ORDERING.  Nothing here synchronises but dexr_sdf_grid_download.  A consumer enqueued on the stream on which the producer wrote
 * the samples sees them; across streams the ordering is the caller's to establish.  A consumer reads the samples at the time its
 * kernel runs, not at the time it is enqueued.
 */
#ifndef DEXR_SDF_GRID_DEV_H
#define DEXR_SDF_GRID_DEV_H

#include "dexr_sdf_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n (3) int32, origin (3) and spacing (3) float64 on the host, the rules of dexr_sdf_grid.h (DEXR_ERR_INVALID before the first HIP
 * call: a null n, origin, spacing or out; a dimension or a product out of range; a spacing that is not finite or not > 0; an origin
 * that is not finite).  values_dev: a DEVICE pointer to n[0] n[1] n[2] float32 in C order, copied device-to-device on `stream`, or
 * NULL: the samples are set to zero on `stream`.  Allocates the samples on the current device; never synchronises. */
int dexr_sdf_grid_create_dev(const int32_t n[3], const double origin[3], const double spacing[3], const float* values_dev, void* stream,
                             dexr_sdf_grid** out);

/* The device pointer to the n[0] n[1] n[2] float32 samples of ANY dexr_sdf_grid, NULL for a null handle.  It stays valid until the
 * handle is destroyed. */
float* dexr_sdf_grid_values_dev(dexr_sdf_grid* g);

/* The samples as they are once everything enqueued on `stream` before this call has run: copied to the HOST array values_out on
 * `stream`, then that stream is synchronised.  DEXR_ERR_INVALID for a null handle or array. */
int dexr_sdf_grid_download(const dexr_sdf_grid* g, float* values_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_SDF_GRID_DEV_H */

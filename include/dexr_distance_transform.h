/* dexr_distance_transform.h -- the samples of a distance grid from a point cloud or from a voxel occupancy map: the exact Euclidean
 * distance transform on the device, a stage in front of dexr_sdf_grid.h beside dexr_mesh_sdf.h.  Where the mesh sampler costs
 * samples x triangles and needs a closed surface, this costs three one-dimensional passes over the grid whatever the number of
 * points, and needs no faces, no winding and no closed surface: a depth camera's cloud, an occupancy map.  C ABI.
 *
 * Conventions of dexr.h: every function returns DEXR_OK (0) or a negative DEXR_ERR_* code, the message is read through
 * dexr_last_error of dexr.h.  Everything is validated before the first HIP call.  The library reads no environment variable.
 *
 * THE GRID.  n = (nx, ny, nz) samples in C order (iz the fastest), sample (ix, iy, iz) at origin + (ix, iy, iz) h: ONE spacing h for
 * the three axes, because everything between the voxelisation and the last step is then an integer.  The limits are those of
 * dexr_sdf_grid.h by its macros: DEXR_SDF_GRID_MIN_DIM .. DEXR_SDF_GRID_MAX_DIM samples per axis, DEXR_SDF_GRID_MAX_SAMPLES in all.
 *
 * VOXELISATION OF A CLOUD.  points (N, 3) float32, 0 <= N <= DEXR_EDT_MAX_POINTS.  Per axis a, in float64, every operation rounded
 * on its own (no fused multiply-add), the division a multiplication by the reciprocal as in dexr_sdf_grid.h:
 *
 *   u_a = ((double)p_a - origin_a) * (1 / h),      i_a = floor(u_a + 0.5)
 *
 * A point with a coordinate that is not finite, or with an i_a outside 0 .. n_a - 1, is DROPPED: it touches nothing.  Every other
 * point adds one to count[ix][iy][iz], an int32, with an integer atomic add -- integer sums do not depend on their order.  A count
 * saturates at 2^31 - 1; with N <= DEXR_EDT_MAX_POINTS = 2^26 it never gets there.  A voxel is OCCUPIED when
 * count >= min_points (min_points >= 1; a threshold above 1 rejects the isolated points of depth noise).
 *
 * OCCUPANCY GIVEN DIRECTLY.  occ (nx, ny, nz) uint8 in C order: nonzero is occupied.
 *
 * THE TRANSFORM.  For every sample i, in index units, int32:
 *
 *   d2[i] = min over occupied voxels j of  (ix - jx)^2 + (iy - jy)^2 + (iz - jz)^2,        DEXR_EDT_NONE where no voxel is occupied
 *
 * DEXR_EDT_NONE = 2^30 is larger than any squared distance of a grid (3 * 1023^2) and stays below 2^31 after 1023^2 has been added
 * to it three times.  The kernels compute d2 as three one-dimensional passes, z then y then x, each the minimum along its axis of
 * "previous value + squared offset"; all of it is integer arithmetic without rounding, so the result IS the brute-force minimum
 * above, bit for bit, and a row whose samples are all DEXR_EDT_NONE stays so.
 *
 * THE SAMPLES.  Everything after d2 is float64, every operation rounded on its own, and rounded to float32 once, at the store.
 * With D(d2) = max_distance where d2 == DEXR_EDT_NONE and min(h * sqrt((double)d2), max_distance) otherwise:
 *
 *   unsigned (a cloud; an occupancy map with is_signed == 0)      v = (float)(D(d2) - radius)
 *   signed (an occupancy map with is_signed != 0; radius == 0)    a free sample      v = (float)(+D(d2 to occupied) - h / 2)
 *                                                                 an occupied one    v = (float)(-D(d2 to free) + h / 2)
 *
 * radius >= 0 thickens every kept point into a ball.  With radius = h sqrt(3) / 2, half the diagonal of a voxel, the unsigned field
 * never exceeds the true distance to the nearest kept point (a point is at most that far from the centre of its voxel), which is
 * the safe side for a collision term; with radius = 0 it is the raw distance between voxel centres and lies within h sqrt(3) / 2 of
 * the distance to the nearest kept point.  The signed form is two transforms -- to the occupied voxels and to the free ones -- and
 * puts the surface halfway between a free voxel and an occupied neighbour.  max_distance is finite and > 0; because of the clamp
 * EVERY sample is finite whatever the input (an empty cloud: max_distance - radius everywhere), so a grid written by these entry
 * points always satisfies the "samples finite" rule of dexr_sdf_grid.h.
 *
 * DETERMINISM.  EVERY entry of every output is written.  The outputs are a function of the SET of points: they do not depend on the
 * order of the points (the only read-modify-write is the integer count), and they do not depend on the launch shape (the passes are
 * integer minima, the last step is one thread's arithmetic per sample).  There is no floating-point sum anywhere.
 *
 * THE KERNELS.  Voxelisation: one thread per point.  The z pass: a block stages consecutive z rows in LDS and one thread per row
 * makes two sweeps, the nearest occupied sample below and the nearest above.  The y and the x pass: a block takes a tile of (the whole
 * row along the pass axis) x (a run of consecutive addresses), at most DEXR_EDT_TILE_BYTES of int32 in LDS, so that consecutive
 * lanes read consecutive addresses although the row itself is strided; every output sample scans its row in LDS (n operations per
 * sample, n^2 per row).  A last kernel turns d2 into the float32 samples.  docs/experiments/distance_transform.md has the
 * measurements.
 */
#ifndef DEXR_DISTANCE_TRANSFORM_H
#define DEXR_DISTANCE_TRANSFORM_H

#include <stddef.h>
#include <stdint.h>

#include "dexr_sdf_grid_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DEXR_EDT_NONE (1 << 30)        /* d2 where no voxel is occupied */
#define DEXR_EDT_MAX_POINTS (1 << 26)  /* points of one cloud */
#define DEXR_EDT_TILE_BYTES 65536      /* LDS of a block of the y and x passes: a 1024-sample row x 16 columns of int32 */

/* Bytes of workspace a transform on a grid of n (3) needs (three int32 per sample: the counts and two d2 arrays); *bytes_out = 0 and
 * DEXR_ERR_INVALID where n or bytes_out is NULL or a dimension or the product is out of range.  Never touches a device. */
int dexr_edt_workspace_bytes(const int32_t n[3], size_t* bytes_out);

/* DEXR_ERR_INVALID before any HIP call: a null n, origin, values_out or workspace; points or occ NULL (points may be NULL where
 * N == 0); N < 0 or above DEXR_EDT_MAX_POINTS; a dimension or the product out of range; h not finite or not > 0, or 1 / h not finite;
 * an origin that is not finite; min_points < 1; radius not finite or < 0, or not 0 where is_signed; max_distance not finite or not
 * > 0; a workspace smaller than dexr_edt_workspace_bytes says or not 16-byte aligned. */

/* DEVICE pointers: points (N, 3) float32; values_out (nx, ny, nz) float32; d2_out (nx, ny, nz) int32 or NULL; count_out (nx, ny, nz)
 * int32 or NULL; workspace, contents irrelevant and reusable by the next call on the same stream.  n (3) int32 and origin (3) float64
 * on the host.  Enqueued on `stream`; never synchronises, never allocates.  N == 0 is an empty cloud and no error. */
int dexr_edt_points_dev(const float* points, int64_t N, const int32_t n[3], const double origin[3], double h, int32_t min_points, double radius,
                        double max_distance, float* values_out, int32_t* d2_out, int32_t* count_out, void* workspace, size_t workspace_bytes,
                        void* stream);

/* DEVICE pointers: occ (nx, ny, nz) uint8; values_out; d2_out or NULL (signed: the d2 to the OCCUPIED voxels); workspace. */
int dexr_edt_occupancy_dev(const uint8_t* occ, const int32_t n[3], double h, int32_t is_signed, double radius, double max_distance,
                           float* values_out, int32_t* d2_out, void* workspace, size_t workspace_bytes, void* stream);

/* The same with points / occ and every output on the HOST: copy, run, synchronise; they allocate their own workspace. */
int dexr_edt_points(const float* points, int64_t N, const int32_t n[3], const double origin[3], double h, int32_t min_points, double radius,
                    double max_distance, float* values_out, int32_t* d2_out, int32_t* count_out);
int dexr_edt_occupancy(const uint8_t* occ, const int32_t n[3], double h, int32_t is_signed, double radius, double max_distance,
                       float* values_out, int32_t* d2_out);

#ifdef __cplusplus
}
#endif
#endif /* DEXR_DISTANCE_TRANSFORM_H */

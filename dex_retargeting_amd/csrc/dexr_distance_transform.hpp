// dexr_distance_transform.hpp -- distance grids from point clouds and occupancy maps, the exact Euclidean distance transform
// (include/dexr_distance_transform.h), and the grid handle whose samples live on the device (include/dexr_sdf_grid_dev.h): a fragment
// of dexr_pose.hip, which includes it once, after the grid fragment whose handle it fills.  It shares nothing with the robot kernels
// but DevBuf / POSE_HIP, finite_d and the error channel.
//
// Four kernels, all integer but the last:
//
//   edt_voxel_kernel   one thread per point: the voxel of the point in float64, one integer atomicAdd into the count grid.  The only
//                      read-modify-write of the fragment; an integer sum does not depend on its order.
//   edt_z_kernel       a z row is contiguous.  A block stages EDT_Z_ROWS consecutive rows in LDS (consecutive threads on consecutive
//                      words, the row stride odd so that the sweeping threads start in different banks), thread r sweeps row r twice
//                      -- the nearest occupied sample below, the nearest above -- and the block writes the squares back as it read.
//   edt_axis_kernel    the y and the x pass.  A row is strided, so a block takes (the whole row) x (cw consecutive addresses): the
//                      loads and the stores of consecutive lanes are consecutive words.  The tile sits in LDS as int32; every output
//                      scans its row there (the plain n-per-sample form: lanes of one column read one word, a broadcast, lanes of
//                      different columns consecutive words, no bank conflict) and is stored in place -- the block owns its tile and
//                      reads it from memory only before the barrier.
//   edt_finish_kernel  d2 -> the float32 sample, float64 arithmetic rounded once at the store, one thread per sample.
//
// A DEXR_EDT_NONE entry needs no branch in the scan: NONE + offset^2 >= NONE > any real squared distance, so the minimum is clamped
// back to NONE once, after the loop.
#include "dexr_distance_transform.h"

#define EDT_THREADS 256
#define EDT_Z_LDS 32768        // bytes of LDS of a block of the z pass
#define EDT_AXIS_MAX_RUN 32    // consecutive addresses of a tile of the y / x pass at most: 128 B per row segment

static_assert(DEXR_EDT_NONE > 3 * (DEXR_SDF_GRID_MAX_DIM - 1) * (DEXR_SDF_GRID_MAX_DIM - 1), "the sentinel is above every squared distance");
static_assert((long long)DEXR_EDT_NONE + 3ll * (DEXR_SDF_GRID_MAX_DIM - 1) * (DEXR_SDF_GRID_MAX_DIM - 1) < (1ll << 31), "the sentinel survives three passes");
static_assert(DEXR_EDT_TILE_BYTES <= 65536 && DEXR_EDT_TILE_BYTES / 4 / DEXR_SDF_GRID_MAX_DIM >= 1, "a tile holds the longest row");
static_assert(EDT_Z_LDS / 4 >= (DEXR_SDF_GRID_MAX_DIM | 1), "a block of the z pass holds the longest row");

namespace {

struct EdtGrid {
  int32_t n[3];
  double origin[3], inv_h;
};

__global__ void __launch_bounds__(EDT_THREADS) edt_voxel_kernel(const float* __restrict__ points, int64_t N, EdtGrid G, int32_t* __restrict__ count) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * EDT_THREADS + threadIdx.x;
  if (i >= N) return;
  int32_t idx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double d = (double)points[i * 3 + a] - G.origin[a];
    const double u = d * G.inv_h;
    const double f = floor(u + 0.5);
    if (!(f >= 0.0 && f < (double)G.n[a])) return;  // (a NaN and both infinities fail the comparison: the point is dropped)
    idx[a] = (int32_t)f;
  }
  int32_t* slot = count + ((int64_t)idx[0] * G.n[1] + idx[1]) * G.n[2] + idx[2];
  // (saturation at 2^31 - 1 cannot come into play: a call holds at most DEXR_EDT_MAX_POINTS points)
  atomicAdd(slot, 1);
}

// occupied = ((int)src >= thr) != invert.  src: the int32 counts against min_points, or the uint8 occupancy against 1; invert: the
// transform to the FREE voxels of the signed form.
template <typename S>
__global__ void __launch_bounds__(EDT_THREADS) edt_z_kernel(const S* __restrict__ src, int32_t thr, int32_t invert, int32_t* __restrict__ d2, int32_t n_rows,
                                                            int32_t nz, int32_t rows_per_block) {
  extern __shared__ int32_t edt_lds[];
  const int tid = threadIdx.x;
  const int stride = nz | 1;
  const int32_t row0 = (int32_t)blockIdx.x * rows_per_block;
  const int nr = n_rows - row0 < rows_per_block ? n_rows - row0 : rows_per_block;
  const int64_t base = (int64_t)row0 * nz;
  const int cnt = nr * nz;
  for (int e = tid; e < cnt; e += EDT_THREADS) {
    const int r = e / nz, k = e - r * nz;
    const bool occupied = ((int32_t)src[base + e] >= thr) != (invert != 0);
    edt_lds[r * stride + k] = occupied ? 0 : DEXR_EDT_NONE;
  }
  __syncthreads();
  if (tid < nr) {
    int32_t* row = edt_lds + tid * stride;
    int32_t d = DEXR_EDT_NONE;  // samples to the nearest occupied one below, NONE: there is none
    for (int k = 0; k < nz; ++k) {
      d = row[k] == 0 ? 0 : (d == DEXR_EDT_NONE ? d : d + 1);
      row[k] = d;
    }
    d = DEXR_EDT_NONE;
    for (int k = nz - 1; k >= 0; --k) {
      const int32_t f = row[k];
      d = f == 0 ? 0 : (d == DEXR_EDT_NONE ? d : d + 1);
      const int32_t m = f < d ? f : d;
      row[k] = m == DEXR_EDT_NONE ? DEXR_EDT_NONE : m * m;
    }
  }
  __syncthreads();
  for (int e = tid; e < cnt; e += EDT_THREADS) {
    const int r = e / nz, k = e - r * nz;
    d2[base + e] = edt_lds[r * stride + k];
  }
}

// in place on d2.  n samples along the pass axis, `stride` words apart; a block owns the columns c0 .. c0 + cw - 1 of outer slab o,
// `run` of them at most, of the `inner` consecutive words of that slab.
__global__ void __launch_bounds__(EDT_THREADS) edt_axis_kernel(int32_t* __restrict__ d2, int32_t n, int32_t stride, int32_t inner, int32_t outer_stride,
                                                               int32_t run, int32_t tiles_per_outer) {
  extern __shared__ int32_t edt_lds[];
  const int tid = threadIdx.x;
  const int32_t o = (int32_t)blockIdx.x / tiles_per_outer, c0 = ((int32_t)blockIdx.x - o * tiles_per_outer) * run;
  const int cw = inner - c0 < run ? inner - c0 : run;
  int32_t* tile = d2 + (int64_t)o * outer_stride + c0;
  const int cnt = n * cw;
  for (int e = tid; e < cnt; e += EDT_THREADS) {
    const int j = e / cw, c = e - j * cw;
    edt_lds[e] = tile[(int64_t)j * stride + c];
  }
  __syncthreads();
  for (int e = tid; e < cnt; e += EDT_THREADS) {
    const int i = e / cw, c = e - i * cw;
    const int32_t* col = edt_lds + c;
    int32_t best = DEXR_EDT_NONE;
    int32_t off = i;  // i - j
    for (int j = 0; j < n; ++j, --off) {
      const int32_t v = col[j * cw] + off * off;
      best = v < best ? v : best;
    }
    tile[(int64_t)i * stride + c] = best;  // (v >= NONE never wins against the initial NONE: a row without an entry stays NONE)
  }
}

// occ == nullptr: the unsigned form of to_occ.  Otherwise the signed form: to_occ where the sample is free, to_free where it is occupied.
__global__ void __launch_bounds__(EDT_THREADS) edt_finish_kernel(const int32_t* __restrict__ to_occ, const int32_t* __restrict__ to_free,
                                                                 const uint8_t* __restrict__ occ, int32_t total, double h, double radius, double max_distance,
                                                                 float* __restrict__ values) {
#pragma clang fp contract(off)
  const int32_t i = (int32_t)blockIdx.x * EDT_THREADS + threadIdx.x;
  if (i >= total) return;
  const bool inside = occ && occ[i] != 0;
  const int32_t q = inside ? to_free[i] : to_occ[i];
  double D = max_distance;
  if (q < DEXR_EDT_NONE) {
    const double r = sqrt((double)q);
    const double t = h * r;
    D = t < max_distance ? t : max_distance;
  }
  const double sub = occ ? h * 0.5 : radius;
  const double v = D - sub;
  values[i] = (float)(inside ? -v : v);
}

struct EdtSpec {
  int32_t n[3];
  int64_t total;
  double h;
};

int check_edt_grid(const int32_t* n, EdtSpec* S) {
  if (!n) return dexr_set_error(DEXR_ERR_INVALID, "null dimension array");
  S->total = 1;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < DEXR_SDF_GRID_MIN_DIM || n[a] > DEXR_SDF_GRID_MAX_DIM)
      return dexr_set_error(DEXR_ERR_INVALID, "grid dimension %d is %d (%d..%d)", a, n[a], DEXR_SDF_GRID_MIN_DIM, DEXR_SDF_GRID_MAX_DIM);
    S->n[a] = n[a];
    S->total *= n[a];
  }
  if (S->total > DEXR_SDF_GRID_MAX_SAMPLES)
    return dexr_set_error(DEXR_ERR_INVALID, "the grid has %lld samples (at most %d)", (long long)S->total, DEXR_SDF_GRID_MAX_SAMPLES);
  return 0;
}

// the rules shared by the four transform entries; ws_needed: the _dev forms
int check_edt_call(const int32_t* n, double h, double radius, double max_distance, bool is_signed, const void* values_out, bool ws_needed,
                   const void* workspace, size_t workspace_bytes, EdtSpec* S) {
  const int c = check_edt_grid(n, S);
  if (c) return c;
  if (!finite_d(h) || !(h > 0.0) || !finite_d(1.0 / h)) return dexr_set_error(DEXR_ERR_INVALID, "the spacing must be finite and > 0, got %g", h);
  S->h = h;
  if (!finite_d(radius) || radius < 0.0) return dexr_set_error(DEXR_ERR_INVALID, "radius must be finite and >= 0, got %g", radius);
  if (is_signed && radius != 0.0) return dexr_set_error(DEXR_ERR_INVALID, "the signed form has no radius (its offset is h / 2), got %g", radius);
  if (!finite_d(max_distance) || !(max_distance > 0.0)) return dexr_set_error(DEXR_ERR_INVALID, "max_distance must be finite and > 0, got %g", max_distance);
  if (!values_out) return dexr_set_error(DEXR_ERR_INVALID, "values_out is NULL");
  if (ws_needed) {
    if (!workspace) return dexr_set_error(DEXR_ERR_INVALID, "workspace is NULL");
    if (((uintptr_t)workspace & 15) != 0) return dexr_set_error(DEXR_ERR_INVALID, "the workspace is not 16-byte aligned");
    if (workspace_bytes < (size_t)S->total * 3 * sizeof(int32_t))
      return dexr_set_error(DEXR_ERR_INVALID, "the workspace has %zu bytes, the transform needs %zu", workspace_bytes, (size_t)S->total * 3 * sizeof(int32_t));
  }
  return 0;
}

int check_edt_points(const void* points, int64_t N, const double* origin, int32_t min_points) {
  if (N < 0 || N > DEXR_EDT_MAX_POINTS) return dexr_set_error(DEXR_ERR_INVALID, "the cloud has %lld points (0..%d)", (long long)N, DEXR_EDT_MAX_POINTS);
  if (N > 0 && !points) return dexr_set_error(DEXR_ERR_INVALID, "points is NULL");
  if (!origin) return dexr_set_error(DEXR_ERR_INVALID, "null origin");
  for (int a = 0; a < 3; ++a)
    if (!finite_d(origin[a])) return dexr_set_error(DEXR_ERR_INVALID, "grid origin %d is not finite", a);
  if (min_points < 1) return dexr_set_error(DEXR_ERR_INVALID, "min_points must be >= 1, got %d", min_points);
  return 0;
}

#define EDT_LAUNCHED(what)                                                                                                  \
  do {                                                                                                                      \
    const hipError_t e_ = hipGetLastError();                                                                                \
    if (e_ != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "distance transform: %s failed: %s", what, hipGetErrorString(e_)); \
  } while (0)

// the three passes of one transform into d2 (in place after the z pass)
template <typename S>
int launch_edt_passes(const EdtSpec& G, const S* src, int32_t thr, int32_t invert, int32_t* d2, hipStream_t st) {
  const int32_t nx = G.n[0], ny = G.n[1], nz = G.n[2];
  {
    const int32_t n_rows = nx * ny, stride = nz | 1;
    int32_t rows = (EDT_Z_LDS / 4) / stride;
    rows = rows > EDT_THREADS ? EDT_THREADS : rows;
    rows = rows > n_rows ? n_rows : rows;
    const dim3 grid((unsigned)((n_rows + rows - 1) / rows)), block(EDT_THREADS);
    hipLaunchKernelGGL((edt_z_kernel<S>), grid, block, (size_t)rows * stride * sizeof(int32_t), st, src, thr, invert, d2, n_rows, nz, rows);
    EDT_LAUNCHED("the z pass");
  }
  // y: rows of ny samples nz words apart, nz consecutive words per slab ix; x: rows of nx samples ny nz words apart, one slab
  const int32_t len[2] = {ny, nx}, stride[2] = {nz, ny * nz}, inner[2] = {nz, ny * nz}, outer[2] = {nx, 1}, outer_stride[2] = {ny * nz, 0};
  for (int p = 0; p < 2; ++p) {
    int32_t run = (DEXR_EDT_TILE_BYTES / 4) / len[p];
    run = run > EDT_AXIS_MAX_RUN ? EDT_AXIS_MAX_RUN : run;
    run = run > inner[p] ? inner[p] : run;
    const int32_t tiles = (inner[p] + run - 1) / run;
    const dim3 grid((unsigned)((int64_t)outer[p] * tiles)), block(EDT_THREADS);
    hipLaunchKernelGGL(edt_axis_kernel, grid, block, (size_t)len[p] * run * sizeof(int32_t), st, d2, len[p], stride[p], inner[p], outer_stride[p], run, tiles);
    EDT_LAUNCHED(p == 0 ? "the y pass" : "the x pass");
  }
  return DEXR_OK;
}

int launch_edt_finish(const EdtSpec& G, const int32_t* to_occ, const int32_t* to_free, const uint8_t* occ, double radius, double max_distance, float* values,
                      hipStream_t st) {
  const dim3 grid((unsigned)((G.total + EDT_THREADS - 1) / EDT_THREADS)), block(EDT_THREADS);
  hipLaunchKernelGGL(edt_finish_kernel, grid, block, 0, st, to_occ, to_free, occ, (int32_t)G.total, G.h, radius, max_distance, values);
  EDT_LAUNCHED("the finishing kernel");
  return DEXR_OK;
}

// workspace: three int32 per sample -- the counts, d2 to the occupied voxels, d2 to the free ones
int run_edt_points(const EdtSpec& G, const float* points, int64_t N, const double* origin, int32_t min_points, double radius, double max_distance,
                   float* values, int32_t* d2_out, int32_t* count_out, int32_t* ws, hipStream_t st) {
  int32_t* count = count_out ? count_out : ws;
  int32_t* d2 = d2_out ? d2_out : ws + G.total;
  const hipError_t e = hipMemsetAsync(count, 0, (size_t)G.total * sizeof(int32_t), st);
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "distance transform: clearing the counts failed: %s", hipGetErrorString(e));
  if (N > 0) {
    EdtGrid V;
    for (int a = 0; a < 3; ++a) {
      V.n[a] = G.n[a];
      V.origin[a] = origin[a];
    }
    V.inv_h = 1.0 / G.h;
    const dim3 grid((unsigned)((N + EDT_THREADS - 1) / EDT_THREADS)), block(EDT_THREADS);
    hipLaunchKernelGGL(edt_voxel_kernel, grid, block, 0, st, points, N, V, count);
    EDT_LAUNCHED("the voxelisation");
  }
  const int rc = launch_edt_passes<int32_t>(G, count, min_points, 0, d2, st);
  if (rc) return rc;
  return launch_edt_finish(G, d2, nullptr, nullptr, radius, max_distance, values, st);
}

int run_edt_occupancy(const EdtSpec& G, const uint8_t* occ, bool is_signed, double radius, double max_distance, float* values, int32_t* d2_out,
                      int32_t* ws, hipStream_t st) {
  int32_t* d2 = d2_out ? d2_out : ws + G.total;
  int rc = launch_edt_passes<uint8_t>(G, occ, 1, 0, d2, st);
  if (rc) return rc;
  if (!is_signed) return launch_edt_finish(G, d2, nullptr, nullptr, radius, max_distance, values, st);
  int32_t* to_free = ws + 2 * G.total;
  rc = launch_edt_passes<uint8_t>(G, occ, 1, 1, to_free, st);
  if (rc) return rc;
  return launch_edt_finish(G, d2, to_free, occ, 0.0, max_distance, values, st);
}

}  // namespace

extern "C" {

int dexr_edt_workspace_bytes(const int32_t n[3], size_t* bytes_out) {
  if (!bytes_out) return dexr_set_error(DEXR_ERR_INVALID, "null argument");
  *bytes_out = 0;
  EdtSpec G;
  const int c = check_edt_grid(n, &G);
  if (c) return c;
  *bytes_out = (size_t)G.total * 3 * sizeof(int32_t);
  return DEXR_OK;
}

int dexr_edt_points_dev(const float* points, int64_t N, const int32_t n[3], const double origin[3], double h, int32_t min_points, double radius,
                        double max_distance, float* values_out, int32_t* d2_out, int32_t* count_out, void* workspace, size_t workspace_bytes,
                        void* stream) {
  EdtSpec G;
  int c = check_edt_call(n, h, radius, max_distance, false, values_out, true, workspace, workspace_bytes, &G);
  if (!c) c = check_edt_points(points, N, origin, min_points);
  if (c) return c;
  return run_edt_points(G, points, N, origin, min_points, radius, max_distance, values_out, d2_out, count_out, (int32_t*)workspace, (hipStream_t)stream);
}

int dexr_edt_occupancy_dev(const uint8_t* occ, const int32_t n[3], double h, int32_t is_signed, double radius, double max_distance,
                           float* values_out, int32_t* d2_out, void* workspace, size_t workspace_bytes, void* stream) {
  EdtSpec G;
  const int c = check_edt_call(n, h, radius, max_distance, is_signed != 0, values_out, true, workspace, workspace_bytes, &G);
  if (c) return c;
  if (!occ) return dexr_set_error(DEXR_ERR_INVALID, "occ is NULL");
  return run_edt_occupancy(G, occ, is_signed != 0, radius, max_distance, values_out, d2_out, (int32_t*)workspace, (hipStream_t)stream);
}

int dexr_edt_points(const float* points, int64_t N, const int32_t n[3], const double origin[3], double h, int32_t min_points, double radius,
                    double max_distance, float* values_out, int32_t* d2_out, int32_t* count_out) {
  EdtSpec G;
  int c = check_edt_call(n, h, radius, max_distance, false, values_out, false, nullptr, 0, &G);
  if (!c) c = check_edt_points(points, N, origin, min_points);
  if (c) return c;
  const size_t nb = (size_t)G.total * sizeof(int32_t);
  DevBuf dp, dv, dw;
  POSE_HIP(dp.put(points, (size_t)N * 3 * sizeof(float)));
  POSE_HIP(dv.put(nullptr, (size_t)G.total * sizeof(float)));
  POSE_HIP(dw.put(nullptr, 3 * nb));
  int32_t* ws = (int32_t*)dw.p;
  const int rc = run_edt_points(G, (const float*)dp.p, N, origin, min_points, radius, max_distance, (float*)dv.p, nullptr, nullptr, ws, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  POSE_HIP(hipMemcpy(values_out, dv.p, (size_t)G.total * sizeof(float), hipMemcpyDeviceToHost));
  if (count_out) POSE_HIP(hipMemcpy(count_out, ws, nb, hipMemcpyDeviceToHost));
  if (d2_out) POSE_HIP(hipMemcpy(d2_out, ws + G.total, nb, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

int dexr_edt_occupancy(const uint8_t* occ, const int32_t n[3], double h, int32_t is_signed, double radius, double max_distance,
                       float* values_out, int32_t* d2_out) {
  EdtSpec G;
  const int c = check_edt_call(n, h, radius, max_distance, is_signed != 0, values_out, false, nullptr, 0, &G);
  if (c) return c;
  if (!occ) return dexr_set_error(DEXR_ERR_INVALID, "occ is NULL");
  const size_t nb = (size_t)G.total * sizeof(int32_t);
  DevBuf dc, dv, dw;
  POSE_HIP(dc.put(occ, (size_t)G.total));
  POSE_HIP(dv.put(nullptr, (size_t)G.total * sizeof(float)));
  POSE_HIP(dw.put(nullptr, 3 * nb));
  int32_t* ws = (int32_t*)dw.p;
  const int rc = run_edt_occupancy(G, (const uint8_t*)dc.p, is_signed != 0, radius, max_distance, (float*)dv.p, nullptr, ws, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  POSE_HIP(hipMemcpy(values_out, dv.p, (size_t)G.total * sizeof(float), hipMemcpyDeviceToHost));
  if (d2_out) POSE_HIP(hipMemcpy(d2_out, ws + G.total, nb, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

// ---- include/dexr_sdf_grid_dev.h: a grid handle around samples that a producer writes on the device -----------------------------

int dexr_sdf_grid_create_dev(const int32_t n[3], const double origin[3], const double spacing[3], const float* values_dev, void* stream,
                             dexr_sdf_grid** out) {
  if (!out) return dexr_set_error(DEXR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!origin || !spacing) return dexr_set_error(DEXR_ERR_INVALID, "null dimension, origin or spacing");
  EdtSpec G;
  const int c = check_edt_grid(n, &G);
  if (c) return c;
  for (int a = 0; a < 3; ++a) {
    if (!finite_d(spacing[a]) || !(spacing[a] > 0.0) || !finite_d(1.0 / spacing[a]))
      return dexr_set_error(DEXR_ERR_INVALID, "grid spacing %d must be finite and > 0, got %g", a, spacing[a]);
    if (!finite_d(origin[a])) return dexr_set_error(DEXR_ERR_INVALID, "grid origin %d is not finite", a);
  }
  dexr_sdf_grid* g = new (std::nothrow) dexr_sdf_grid();
  if (!g) return dexr_set_error(DEXR_ERR_INVALID, "out of host memory");
  for (int a = 0; a < 3; ++a) {
    g->n[a] = n[a];
    g->origin[a] = origin[a];
    g->spacing[a] = spacing[a];
  }
  fill_grid_desc<float>(g, &g->f32);
  fill_grid_desc<double>(g, &g->f64);
  const size_t nb = (size_t)G.total * sizeof(float);
  hipError_t e = hipMalloc((void**)&g->values, nb);
  if (e == hipSuccess)
    e = values_dev ? hipMemcpyAsync(g->values, values_dev, nb, hipMemcpyDeviceToDevice, (hipStream_t)stream)
                   : hipMemsetAsync(g->values, 0, nb, (hipStream_t)stream);
  if (e != hipSuccess) {
    dexr_sdf_grid_destroy(g);
    return dexr_set_error(DEXR_ERR_HIP, "creating the device sdf grid failed: %s", hipGetErrorString(e));
  }
  *out = g;
  return DEXR_OK;
}

float* dexr_sdf_grid_values_dev(dexr_sdf_grid* g) { return g ? g->values : nullptr; }

int dexr_sdf_grid_download(const dexr_sdf_grid* g, float* values_out, void* stream) {
  if (!g || !values_out) return dexr_set_error(DEXR_ERR_INVALID, "null sdf grid or value array");
  const size_t nb = (size_t)g->n[0] * g->n[1] * g->n[2] * sizeof(float);
  POSE_HIP(hipMemcpyAsync(values_out, g->values, nb, hipMemcpyDeviceToHost, (hipStream_t)stream));
  POSE_HIP(hipStreamSynchronize((hipStream_t)stream));
  return DEXR_OK;
}

}  // extern "C"

// dexr_mesh_sdf.hpp -- signed distances of points or of a grid of samples to a triangle mesh (include/dexr_mesh_sdf.h): a fragment of
// dexr_pose.hip, which includes it once, last.  It shares nothing with the robot kernels but DevBuf / POSE_HIP, finite_d and
// the error channel.
//
// mesh_sdf_kernel<T, O, GRID>: a block of MESH_THREADS threads, each owning MESH_PPT points (thread t of block k owns the points
// k * DEXR_MESH_BLOCK_POINTS + j * MESH_THREADS + t, j < MESH_PPT: consecutive lanes read consecutive points).  With GRID the point
// is generated from that linear sample index in C order.  Every thread walks ALL triangles in table order, so a point's result is
// one thread's and its bits do not depend on the batch; there is no reduction across lanes and no read-modify-write on memory.
//
// The triangle records (a, ab, ac; 12 values, every fourth a pad, so that a record is three 16-byte or six 16-byte reads) are
// staged through LDS DEXR_MESH_TILE at a time: the block copies a tile with consecutive threads on consecutive words, and in the
// loop over the tile every lane reads the SAME address at the same time: a broadcast, no bank conflicts, and one read serves the
// MESH_PPT points of the lane.  Threads of a ragged last block whose points do not exist take part in the loads and the barriers
// (they park on the last point) and skip only the store.
//
// MESH_PPT = 2: docs/experiments/mesh_sdf.md has the register report behind it.
#include "dexr_mesh_sdf.h"

#define MESH_THREADS 256
#define MESH_PPT (DEXR_MESH_BLOCK_POINTS / MESH_THREADS)
#define MESH_REC 12  // values of a record: a, pad, ab, pad, ac, pad

static_assert(DEXR_MESH_BLOCK_POINTS % MESH_THREADS == 0 && MESH_PPT >= 2 && MESH_PPT <= 4, "a thread owns 2 to 4 points");
static_assert(DEXR_MESH_PAIRS_PER_LAUNCH >= (long long)DEXR_MESH_BLOCK_POINTS, "a launch holds one block at least");

namespace {

// where the points come from and where the results go; uniform data, by value
template <typename T, typename O>
struct MeshJob {
  const T* rec;      // (n_tri, MESH_REC)
  int32_t n_tri;
  const T* points;   // (P, 3), or nullptr with GRID
  int64_t first, P;  // this launch covers the points first .. P - 1 as far as its blocks reach
  int32_t nyz, nz;   // GRID: ny * nz and nz
  double origin[3], spacing[3];
  O* dist;
  T* winding;  // or nullptr
};

// origin + i * spacing, each operation rounded once in float64
__device__ __forceinline__ double mesh_sample_coord(double origin, int32_t i, double spacing) {
#pragma clang fp contract(off)
  const double s = (double)i * spacing;
  return origin + s;
}

// a.b with the products fused in a fixed order
template <typename T>
__device__ __forceinline__ T mesh_dot(const T x[3], const T y[3]) {
  return fma(x[2], y[2], fma(x[1], y[1], x[0] * y[0]));
}

// one triangle against one point: the squared distance to the closest point and the solid angle (include/dexr_mesh_sdf.h).
// THE ARITHMETIC IS WRITTEN OUT: contraction is off in this function and every fused multiply-add is an fma() of the source.  Left
// to the compiler, the two unrolled copies of this body (a thread's two points) were contracted differently, and the winding
// number of one point differed in its last bits with the slot that held it: the bits of a result must not depend on the batch.
template <typename T>
__device__ __forceinline__ void mesh_pair(const T a[3], const T ab[3], const T ac[3], const T p[3], T& best, double& wsum) {
#pragma clang fp contract(off)
  const T ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const T bp[3] = {ap[0] - ab[0], ap[1] - ab[1], ap[2] - ab[2]};
  const T cp[3] = {ap[0] - ac[0], ap[1] - ac[1], ap[2] - ac[2]};
  const T d1 = mesh_dot(ab, ap), d2 = mesh_dot(ac, ap), d3 = mesh_dot(ab, bp), d4 = mesh_dot(ac, bp), d5 = mesh_dot(ab, cp), d6 = mesh_dot(ac, cp);
  const T vc = fma(d1, d4, -(d3 * d2)), vb = fma(d5, d2, -(d1 * d6)), va = fma(d3, d6, -(d5 * d4));
  const T e43 = d4 - d3, e56 = d5 - d6;
  T v, w;
  if (d1 <= T(0) && d2 <= T(0)) {
    v = T(0), w = T(0);
  } else if (d3 >= T(0) && d4 <= d3) {
    v = T(1), w = T(0);
  } else if (vc <= T(0) && d1 >= T(0) && d3 <= T(0)) {
    v = d1 / (d1 - d3), w = T(0);
  } else if (d6 >= T(0) && d5 <= d6) {
    v = T(0), w = T(1);
  } else if (vb <= T(0) && d2 >= T(0) && d6 <= T(0)) {
    v = T(0), w = d2 / (d2 - d6);
  } else if (va <= T(0) && e43 >= T(0) && e56 >= T(0)) {
    w = e43 / (e43 + e56), v = T(1) - w;
  } else {
    const T den = va + vb + vc;
    v = vb / den, w = vc / den;
  }
  const T e[3] = {fma(-w, ac[0], fma(-v, ab[0], ap[0])), fma(-w, ac[1], fma(-v, ab[1], ap[1])), fma(-w, ac[2], fma(-v, ab[2], ap[2]))};
  const T q = mesh_dot(e, e);
  if (q < best) best = q;  // (a NaN never wins, the earlier of two equal ones stands)
  // the solid angle: A = a - p = -ap, B = A + ab = -bp, C = A + ac = -cp; the lengths and the pairwise products do not see the
  // signs, the triple product changes its own
  const T la = sqrt(mesh_dot(ap, ap)), lb = sqrt(mesh_dot(bp, bp)), lc = sqrt(mesh_dot(cp, cp));
  const T cr[3] = {fma(bp[1], cp[2], -(bp[2] * cp[1])), fma(bp[2], cp[0], -(bp[0] * cp[2])), fma(bp[0], cp[1], -(bp[1] * cp[0]))};
  const T det = -mesh_dot(ap, cr);
  const T den = fma(mesh_dot(cp, ap), lb, fma(mesh_dot(bp, cp), la, fma(mesh_dot(ap, bp), lc, la * lb * lc)));
  wsum += (double)(T(2) * atan2(det, den));
}

template <typename T, typename O, bool GRID>
__global__ void __launch_bounds__(MESH_THREADS) mesh_sdf_kernel(MeshJob<T, O> J) {
  __shared__ __attribute__((aligned(16))) T tile[DEXR_MESH_TILE * MESH_REC];
  const int tid = threadIdx.x;
  const int64_t base = J.first + (int64_t)blockIdx.x * DEXR_MESH_BLOCK_POINTS + tid;
  T p[MESH_PPT][3], best[MESH_PPT];
  double wsum[MESH_PPT];
  bool ok[MESH_PPT];
#pragma unroll
  for (int j = 0; j < MESH_PPT; ++j) {
    const int64_t i = base + (int64_t)j * MESH_THREADS;
    const int64_t ic = i < J.P ? i : J.P - 1;  // ragged tail: idle threads park on the last point
    if (GRID) {
      const int32_t s = (int32_t)ic;  // (at most DEXR_SDF_GRID_MAX_SAMPLES)
      const int32_t ix = s / J.nyz, r = s - ix * J.nyz, iy = r / J.nz, iz = r - iy * J.nz;
      p[j][0] = (T)mesh_sample_coord(J.origin[0], ix, J.spacing[0]);
      p[j][1] = (T)mesh_sample_coord(J.origin[1], iy, J.spacing[1]);
      p[j][2] = (T)mesh_sample_coord(J.origin[2], iz, J.spacing[2]);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) p[j][k] = J.points[ic * 3 + k];
    }
    const T big = sizeof(T) == 4 ? T(3.4028234663852886e38) : T(1.7976931348623157e308);
    ok[j] = fabs(p[j][0]) <= big && fabs(p[j][1]) <= big && fabs(p[j][2]) <= big;  // (a NaN fails the comparison)
    best[j] = T(INFINITY);
    wsum[j] = 0.0;
  }
  for (int t0 = 0; t0 < J.n_tri; t0 += DEXR_MESH_TILE) {
    const int nt = J.n_tri - t0 < DEXR_MESH_TILE ? J.n_tri - t0 : DEXR_MESH_TILE;
    const T* src = J.rec + (size_t)t0 * MESH_REC;
    __syncthreads();  // the previous tile has been read by every thread
    for (int k = tid; k < nt * MESH_REC; k += MESH_THREADS) tile[k] = src[k];
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const T* r = tile + t * MESH_REC;  // the same address in every lane: a broadcast
      const T a[3] = {r[0], r[1], r[2]}, ab[3] = {r[4], r[5], r[6]}, ac[3] = {r[8], r[9], r[10]};
#pragma unroll
      for (int j = 0; j < MESH_PPT; ++j) mesh_pair<T>(a, ab, ac, p[j], best[j], wsum[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < MESH_PPT; ++j) {
    const int64_t i = base + (int64_t)j * MESH_THREADS;
    if (i >= J.P) continue;
    const double w = wsum[j] * 0.07957747154594767;  // 1 / (4 pi)
    const T u = sqrt(best[j]);
    const T spoilt = T(NAN);
    J.dist[i] = (O)(ok[j] ? (w >= 0.5 ? -u : u) : spoilt);
    if (J.winding) J.winding[i] = ok[j] ? (T)w : spoilt;
  }
}

}  // namespace

struct dexr_mesh {
  int32_t n_vertex = 0, n_triangle = 0;
  double bounds[6] = {0, 0, 0, 0, 0, 0};
  float* rec32 = nullptr;   // device (n_triangle, MESH_REC)
  double* rec64 = nullptr;  // device (n_triangle, MESH_REC)
};

namespace {

template <typename T>
const T* mesh_rec_of(const dexr_mesh* m);
template <>
const float* mesh_rec_of<float>(const dexr_mesh* m) { return m->rec32; }
template <>
const double* mesh_rec_of<double>(const dexr_mesh* m) { return m->rec64; }

struct MeshGridSpec {
  int32_t n[3];
  double origin[3], spacing[3];
};

// the launches of one call: consecutive point ranges, each of at most DEXR_MESH_PAIRS_PER_LAUNCH pairs (a block at least)
template <typename T, typename O>
int launch_mesh(const dexr_mesh* m, int64_t P, const T* points, const MeshGridSpec* G, O* dist, T* winding, hipStream_t st) {
  MeshJob<T, O> J;
  J.rec = mesh_rec_of<T>(m);
  J.n_tri = m->n_triangle;
  J.points = points;
  J.P = P;
  J.nyz = G ? G->n[1] * G->n[2] : 1;
  J.nz = G ? G->n[2] : 1;
  for (int a = 0; a < 3; ++a) {
    J.origin[a] = G ? G->origin[a] : 0.0;
    J.spacing[a] = G ? G->spacing[a] : 0.0;
  }
  J.dist = dist;
  J.winding = winding;
  int64_t blocks_per = ((int64_t)DEXR_MESH_PAIRS_PER_LAUNCH / m->n_triangle) / DEXR_MESH_BLOCK_POINTS;
  if (blocks_per < 1) blocks_per = 1;
  if (blocks_per > 0x7fffffffLL) blocks_per = 0x7fffffffLL;
  const int64_t per = blocks_per * DEXR_MESH_BLOCK_POINTS;
  for (int64_t first = 0; first < P; first += per) {
    const int64_t left = P - first < per ? P - first : per;
    const dim3 grid((unsigned)((left + DEXR_MESH_BLOCK_POINTS - 1) / DEXR_MESH_BLOCK_POINTS)), block(MESH_THREADS);
    J.first = first;
    if (G) hipLaunchKernelGGL((mesh_sdf_kernel<T, O, true>), grid, block, 0, st, J);
    else hipLaunchKernelGGL((mesh_sdf_kernel<T, O, false>), grid, block, 0, st, J);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "mesh distance kernel launch failed: %s", hipGetErrorString(e));
  }
  return DEXR_OK;
}

// checks of the two point entries: < 0 error, 1 nothing to do, 0 go on
int check_mesh_points(const dexr_mesh* m, int64_t P, const void* points, const void* dist_out) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null mesh");
  if (P < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative point count");
  if (P == 0) return 1;
  if (!points) return dexr_set_error(DEXR_ERR_INVALID, "points is NULL");
  if (!dist_out) return dexr_set_error(DEXR_ERR_INVALID, "dist_out is NULL");
  return 0;
}

// checks of the two grid entries, the rules of include/dexr_sdf_grid.h; fills G and the sample count
int check_mesh_grid(const dexr_mesh* m, const int32_t* n, const double* origin, const double* spacing, const void* values_out, MeshGridSpec* G,
                    int64_t* total) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null mesh");
  if (!n || !origin || !spacing || !values_out) return dexr_set_error(DEXR_ERR_INVALID, "null dimension, origin, spacing or value array");
  *total = 1;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < DEXR_SDF_GRID_MIN_DIM || n[a] > DEXR_SDF_GRID_MAX_DIM)
      return dexr_set_error(DEXR_ERR_INVALID, "grid dimension %d is %d (%d..%d)", a, n[a], DEXR_SDF_GRID_MIN_DIM, DEXR_SDF_GRID_MAX_DIM);
    *total *= n[a];
  }
  if (*total > DEXR_SDF_GRID_MAX_SAMPLES)
    return dexr_set_error(DEXR_ERR_INVALID, "the grid has %lld samples (at most %d)", (long long)*total, DEXR_SDF_GRID_MAX_SAMPLES);
  for (int a = 0; a < 3; ++a) {
    if (!finite_d(spacing[a]) || !(spacing[a] > 0.0) || !finite_d(1.0 / spacing[a]))
      return dexr_set_error(DEXR_ERR_INVALID, "grid spacing %d must be finite and > 0, got %g", a, spacing[a]);
    if (!finite_d(origin[a])) return dexr_set_error(DEXR_ERR_INVALID, "grid origin %d is not finite", a);
    G->n[a] = n[a];
    G->origin[a] = origin[a];
    G->spacing[a] = spacing[a];
  }
  return 0;
}

// (b - a) x (c - a) in float64, every operation rounded on its own: the zero test of a degenerate triangle must not depend on
// whether the host compiler fuses
bool mesh_triangle_is_degenerate(const double* a, const double* b, const double* c) {
#pragma clang fp contract(off)
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double p0 = ab[1] * ac[2], q0 = ab[2] * ac[1], p1 = ab[2] * ac[0], q1 = ab[0] * ac[2], p2 = ab[0] * ac[1], q2 = ab[1] * ac[0];
  return p0 - q0 == 0.0 && p1 - q1 == 0.0 && p2 - q2 == 0.0;
}

}  // namespace

extern "C" {

int dexr_mesh_create(int32_t n_vertex, const double* vertices, int32_t n_triangle, const int32_t* faces, dexr_mesh** out) {
  if (!out) return dexr_set_error(DEXR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!vertices || !faces) return dexr_set_error(DEXR_ERR_INVALID, "null vertex or face array");
  if (n_vertex < 1 || n_vertex > DEXR_MESH_MAX_VERTICES)
    return dexr_set_error(DEXR_ERR_INVALID, "the mesh has %d vertices (1..%d)", n_vertex, DEXR_MESH_MAX_VERTICES);
  if (n_triangle < 1 || n_triangle > DEXR_MESH_MAX_TRIANGLES)
    return dexr_set_error(DEXR_ERR_INVALID, "the mesh has %d triangles (1..%d)", n_triangle, DEXR_MESH_MAX_TRIANGLES);
  for (int64_t i = 0; i < (int64_t)n_triangle * 3; ++i)
    if (faces[i] < 0 || faces[i] >= n_vertex)
      return dexr_set_error(DEXR_ERR_INVALID, "triangle %lld: vertex index %d out of range (0..%d)", (long long)(i / 3), faces[i], n_vertex - 1);
  for (int64_t i = 0; i < (int64_t)n_vertex * 3; ++i)
    if (!finite_d(vertices[i])) return dexr_set_error(DEXR_ERR_INVALID, "vertex %lld is not finite", (long long)(i / 3));
  for (int32_t t = 0; t < n_triangle; ++t)
    if (mesh_triangle_is_degenerate(vertices + 3 * (size_t)faces[3 * t], vertices + 3 * (size_t)faces[3 * t + 1], vertices + 3 * (size_t)faces[3 * t + 2]))
      return dexr_set_error(DEXR_ERR_INVALID, "triangle %d has no area: (b - a) x (c - a) is exactly zero", t);
  dexr_mesh* m = new (std::nothrow) dexr_mesh();
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "out of host memory");
  m->n_vertex = n_vertex;
  m->n_triangle = n_triangle;
  for (int k = 0; k < 3; ++k) m->bounds[k] = m->bounds[3 + k] = vertices[k];
  for (int64_t i = 0; i < n_vertex; ++i)
    for (int k = 0; k < 3; ++k) {
      const double v = vertices[3 * i + k];
      if (v < m->bounds[k]) m->bounds[k] = v;
      if (v > m->bounds[3 + k]) m->bounds[3 + k] = v;
    }
  std::vector<double> r64((size_t)n_triangle * MESH_REC, 0.0);
  std::vector<float> r32((size_t)n_triangle * MESH_REC, 0.f);
  for (int32_t t = 0; t < n_triangle; ++t) {
    const double *a = vertices + 3 * (size_t)faces[3 * t], *b = vertices + 3 * (size_t)faces[3 * t + 1], *c = vertices + 3 * (size_t)faces[3 * t + 2];
    double* r = r64.data() + (size_t)t * MESH_REC;
    for (int k = 0; k < 3; ++k) {
      r[k] = a[k];
      r[4 + k] = b[k] - a[k];
      r[8 + k] = c[k] - a[k];
    }
    for (int k = 0; k < MESH_REC; ++k) r32[(size_t)t * MESH_REC + k] = (float)r[k];
  }
  hipError_t e = hipMalloc((void**)&m->rec32, r32.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&m->rec64, r64.size() * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(m->rec32, r32.data(), r32.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->rec64, r64.data(), r64.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    dexr_mesh_destroy(m);
    return dexr_set_error(DEXR_ERR_HIP, "uploading the mesh failed: %s", hipGetErrorString(e));
  }
  *out = m;
  return DEXR_OK;
}

void dexr_mesh_destroy(dexr_mesh* m) {
  if (!m) return;
  if (m->rec32) (void)hipFree(m->rec32);
  if (m->rec64) (void)hipFree(m->rec64);
  delete m;
}

int dexr_mesh_info(const dexr_mesh* m, int32_t* n_vertex, int32_t* n_triangle, double* bounds) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null mesh");
  if (n_vertex) *n_vertex = m->n_vertex;
  if (n_triangle) *n_triangle = m->n_triangle;
  if (bounds)
    for (int k = 0; k < 6; ++k) bounds[k] = m->bounds[k];
  return DEXR_OK;
}

int dexr_mesh_distances_dev(const dexr_mesh* m, int64_t P, const float* points, float* dist_out, float* winding_out, void* stream) {
  const int c = check_mesh_points(m, P, points, dist_out);
  if (c) return c < 0 ? c : DEXR_OK;
  return launch_mesh<float, float>(m, P, points, nullptr, dist_out, winding_out, (hipStream_t)stream);
}

int dexr_mesh_distances(const dexr_mesh* m, int64_t P, const double* points, double* dist_out, double* winding_out) {
  const int c = check_mesh_points(m, P, points, dist_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const size_t np = (size_t)P * sizeof(double);
  DevBuf dp, dd, dw;
  POSE_HIP(dp.put(points, 3 * np));
  POSE_HIP(dd.put(nullptr, np));
  if (winding_out) POSE_HIP(dw.put(nullptr, np));
  const int rc = launch_mesh<double, double>(m, P, (const double*)dp.p, nullptr, (double*)dd.p, (double*)dw.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  POSE_HIP(hipMemcpy(dist_out, dd.p, np, hipMemcpyDeviceToHost));
  if (winding_out) POSE_HIP(hipMemcpy(winding_out, dw.p, np, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

int dexr_mesh_sample_grid_dev(const dexr_mesh* m, const int32_t n[3], const double origin[3], const double spacing[3], float* values_out,
                              void* stream) {
  MeshGridSpec G;
  int64_t total = 0;
  const int c = check_mesh_grid(m, n, origin, spacing, values_out, &G, &total);
  if (c) return c;
  return launch_mesh<float, float>(m, total, nullptr, &G, values_out, nullptr, (hipStream_t)stream);
}

int dexr_mesh_sample_grid(const dexr_mesh* m, const int32_t n[3], const double origin[3], const double spacing[3], float* values_out) {
  MeshGridSpec G;
  int64_t total = 0;
  const int c = check_mesh_grid(m, n, origin, spacing, values_out, &G, &total);
  if (c) return c;
  DevBuf dv;
  POSE_HIP(dv.put(nullptr, (size_t)total * sizeof(float)));
  const int rc = launch_mesh<double, float>(m, total, nullptr, &G, (float*)dv.p, nullptr, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  POSE_HIP(hipMemcpy(values_out, dv.p, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
  return DEXR_OK;
}

}  // extern "C"

// dexr_sdf_grid.hpp -- the robot's spheres against one sampled signed-distance field (include/dexr_sdf_grid.h): a fragment of
// dexr_pose.hip, which includes it once after dexr_resolve_obstacles.hpp.  It is pose_obstacle_kernel
// (dexr_obstacles.hpp) with another phase B: the same three-phase block, per-frame LDS layout and frames per block.  What that
// family has as functions is used as it is -- joint_step, link_pose, sphere_centre, resolve_force_entry, cross_fma, obstacle_point
// and obstacle_to_world of dexr_resolve_obstacles.hpp, ObstacleArgs, check_call, check_margin, DevBuf / POSE_HIP.  Phases A and C
// are written inline in pose_obstacle_kernel; they are functions here (grid_walk, grid_columns), operation by operation those
// phases, and pose_obstacle_kernel is left as it is: calling them from it changes its code object.
//
// Phase B (pose_grid_kernel<T, MODE>, 16 threads per frame): thread t owns the spheres t, t + 16, ...; a sphere moves its
// centre into the obstacle frame once, y = R_o^T (c - p_o), and does ONE cell lookup (grid_sdf): per axis the cell coordinate is
// clamped in floating point by comparisons that send a NaN to 0, converted, and the integer clamped to [0, n - 2] again, so
// that whatever the inputs hold -- NaN, infinities, 1e30 -- the eight offsets lie inside the samples and there is no branch
// around the loads: a sphere outside the grid reads the boundary cell, and what it lacks comes from e, the vector from the box
// to the point.  All eight offsets are formed and all eight loads issued before the first use: one wait covers them.
//
// THE DESCRIPTOR IS UNIFORM DATA: dims, strides, origin, spacing and inverse spacing travel by value as a kernel argument
// (GridD<T>) and live in scalar registers, as the primitive table's records do in the sibling.  The samples stay in global memory
// behind a const float* __restrict__ in C order, one float32 copy for both precisions (the float64 kernels widen on load); the
// eight addresses differ per lane: vector loads.  The two samples that differ in iz alone are adjacent words; they are written
// as two loads of one float each, nothing asks for more than 4-byte alignment.
#include "dexr_sdf_grid.h"

namespace {

template <typename T>
struct GridD {
  int32_t n[3];    // samples per axis
  int32_t sx, sy;  // strides of ix and iy in samples (iz: 1)
  T origin[3], h[3], inv[3];  // spacing and 1 / spacing
};

// offsets into a frame's region, those of pose_obstacle_kernel: all from n_sphere alone, the a, o records last
struct GridLayout {
  int fbase, ebase, wbase, obase, abase;
};

__device__ __forceinline__ GridLayout grid_layout(int n_sphere, bool dist_form) {
  GridLayout Y;
  Y.fbase = 3 * n_sphere;
  Y.ebase = Y.fbase + 3 * n_sphere;
  Y.wbase = Y.ebase + SPH_FANOUT;
  Y.obase = dist_form ? Y.fbase : Y.wbase + 6 * SPH_FANOUT;
  Y.abase = Y.obase + OBS_POSE;
  return Y;
}

// phase A of one lane (lane = frame): the frame's obstacle pose (zeros and the identity where the caller left them out), the
// sphere centres and, with GRAD, a_k, o_k of every joint driven by x, into the frame's region pk
template <typename T, bool GRAD>
__device__ __forceinline__ void grid_walk(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links, const PoseArgs<T>& P,
                                          const SphereD<T>* __restrict__ spheres, const SphereIndex& S, const T* __restrict__ x,
                                          const T* __restrict__ fixed, const ObstacleArgs<T>& A, T* slots, int nl, int lane, int64_t first, T* pk,
                                          const GridLayout& Y) {
  T* cen = pk;
  const int64_t b = first + lane < P.B ? first + lane : P.B - 1;  // ragged tail: idle lanes park the last frame again
  T* po = pk + Y.obase;
#pragma unroll
  for (int i = 0; i < 3; ++i) po[i] = A.opos ? A.opos[b * 3 + i] : T(0);
#pragma unroll
  for (int i = 0; i < 9; ++i) po[3 + i] = A.orot ? A.orot[b * 9 + i] : ((i % 4 == 0) ? T(1) : T(0));
  for (int l = 0; l < P.n_base; ++l) {  // spheres on the fixed base: constant centres
    const LinkD<T>& L = links[l];
    for (int s = S.link_sph[l]; s < S.link_sph[l + 1]; ++s) sphere_centre(L.R, L.p, spheres[s], cen + 3 * s);
  }
  Xf<T> t;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.R[i] = (i % 4 == 0) ? T(1) : T(0);
  t.p[0] = t.p[1] = t.p[2] = T(0);
  int xi = 0;
  for (int k = 0; k < P.n_joint; ++k) {
    const JointD<T>& J = joints[k];
    T a[3];
    joint_step(J, P, x, fixed, b, slots, nl, lane, t, a);
    if (GRAD && J.src_kind == DEXR_POSE_SRC_X) {
      T* d = pk + Y.abase + 6 * xi;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        d[i] = a[i];
        d[3 + i] = t.p[i];
      }
      ++xi;
    }
    for (int l = J.link_begin; l < J.link_end; ++l) {
      const int s0 = S.link_sph[l], s1 = S.link_sph[l + 1];
      if (s0 == s1) continue;
      T R[9], p[3];
      link_pose(links[l], t, R, p);
      for (int s = s0; s < s1; ++s) sphere_centre(R, p, spheres[s], cen + 3 * s);
    }
  }
}

// phase C (behind the barrier that ends phase B): a thread per active column through resolve_force_entry, then the columns no
// joint reads; with PENALTY thread 0 adds the sixteen partial energies in order, threads 10 .. 15 each one component of the wrench
template <typename T, bool PENALTY>
__device__ __forceinline__ void grid_columns(const PoseArgs<T>& P, const SphereIndex& S, const JacEnt* __restrict__ ents,
                                             const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col,
                                             const int32_t* __restrict__ col_act, int n_act, const T* pk, const GridLayout& Y, int t, bool live,
                                             int64_t b, const ObstacleArgs<T>& A) {
  if (A.gx) {
    for (int i = t; i < n_act; i += SPH_FANOUT) {
      const T g = resolve_force_entry(act_rng[i], ents, S.link_sph, pk + Y.abase, pk, pk + Y.fbase);
      if (live) A.gx[b * P.n_in + act_col[i]] = g;
    }
    if (live) {
      T* o = A.gx + b * P.n_in;
      for (int c = t; c < P.n_in; c += SPH_FANOUT)
        if (col_act[c] < 0) o[c] = T(0);
    }
  }
  if (PENALTY && live) {
    if (A.e_out && t == 0) {
      T E = pk[Y.ebase];
      for (int i = 1; i < SPH_FANOUT; ++i) E += pk[Y.ebase + i];
      A.e_out[b] = E;
    }
    if (A.wrench && t >= SPH_FANOUT - 6) {
      const int c = t - (SPH_FANOUT - 6);
      const T* w = pk + Y.wbase + c * SPH_FANOUT;
      T W = w[0];
      for (int i = 1; i < SPH_FANOUT; ++i) W += w[i];
      A.wrench[b * 6 + c] = W;
    }
  }
}

// sdf(y) of include/dexr_sdf_grid.h and its gradient g in the obstacle frame.  No input makes an offset leave the samples.
template <typename T, bool GRAD>
__device__ __forceinline__ T grid_sdf(const GridD<T>& G, const float* __restrict__ V, const T y[3], T g[3]) {
  int i[3];
  T t[3], e[3];
  bool in[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const T top = T(G.n[a] - 1);
    const T u = (y[a] - G.origin[a]) * G.inv[a];
    const T uc = u > T(0) ? (u < top ? u : top) : T(0);  // (comparisons: a NaN goes to 0)
    int k = (int)uc;                                      // 0 <= uc <= n - 1, finite: the conversion is floor
    k = k < 0 ? 0 : (k > G.n[a] - 2 ? G.n[a] - 2 : k);    // ... and whatever it gave, the cell is one of the grid's
    i[a] = k;
    t[a] = uc - T(k);
    in[a] = u == uc;
    // exact zero inside the box, by the comparison and not by the subtraction: the compiler may contract u - uc with the product
    // that made u, which leaves that product's rounding error and, divided by its own length, a direction.  A NaN of u stays one
    e[a] = in[a] ? T(0) : (u - uc) * G.h[a];
  }
  const int o00 = i[0] * G.sx + i[1] * G.sy + i[2], o01 = o00 + G.sy, o10 = o00 + G.sx, o11 = o10 + G.sy;
  const float f000 = V[o00], f001 = V[o00 + 1], f010 = V[o01], f011 = V[o01 + 1];
  const float f100 = V[o10], f101 = V[o10 + 1], f110 = V[o11], f111 = V[o11 + 1];
  // along x, then y, then z: c = V0 + t (V1 - V0); the differences are the interpolant's exact derivatives
  const T dx00 = T(f100) - T(f000), dx01 = T(f101) - T(f001), dx10 = T(f110) - T(f010), dx11 = T(f111) - T(f011);
  const T c00 = fma(t[0], dx00, T(f000)), c01 = fma(t[0], dx01, T(f001)), c10 = fma(t[0], dx10, T(f010)), c11 = fma(t[0], dx11, T(f011));
  const T dy0 = c10 - c00, dy1 = c11 - c01;
  const T c0 = fma(t[1], dy0, c00), c1 = fma(t[1], dy1, c01);
  const T dz = c1 - c0;
  const T v = fma(t[2], dz, c0);
  const T len = sqrt(fma(e[2], e[2], fma(e[1], e[1], e[0] * e[0])));
  if (GRAD) {
    const T ex0 = fma(t[1], dx10 - dx00, dx00), ex1 = fma(t[1], dx11 - dx01, dx01);
    const T dv[3] = {fma(t[2], ex1 - ex0, ex0), fma(t[2], dy1 - dy0, dy0), dz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const T out = len > T(0) ? e[a] / len : len * T(0);  // (a NaN of e stays one)
      g[a] = (in[a] ? dv[a] * G.inv[a] : T(0)) + out;
    }
  }
  return v + len;
}

template <typename T, int MODE>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES) pose_grid_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                           PoseArgs<T> P, const SphereD<T>* __restrict__ spheres, SphereIndex S,
                                                                           GridD<T> G, const float* __restrict__ V, const JacEnt* __restrict__ ents,
                                                                           const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col,
                                                                           const int32_t* __restrict__ col_act, int n_act, int stride,
                                                                           const T* __restrict__ x, const T* __restrict__ fixed, ObstacleArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* park = slots + (size_t)P.n_slot * 12 * nl;
  const GridLayout Y = grid_layout(S.n_sphere, MODE == OBS_DIST);
  const int64_t first = (int64_t)blockIdx.x * nl;
  if (tid < nl)  // phase A: lane = frame
    grid_walk<T, MODE != OBS_DIST>(joints, links, P, spheres, S, x, fixed, A, slots, nl, tid, first, park + (size_t)tid * stride, Y);
  __syncthreads();
  // phase B: SPH_FANOUT threads per frame, a thread per sphere, one cell lookup per sphere
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  T* pk = park + (size_t)fr * stride;
  const T* cen = pk;
  const bool live = first + fr < P.B;
  const int64_t b = live ? first + fr : P.B - 1;
  const T* po = pk + Y.obase;  // p_o (3), R_o (9)
  T e = T(0), wr[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  for (int s = t; s < S.n_sphere; s += SPH_FANOUT) {
    T y[3], go[3];
    obstacle_point(po, cen + 3 * s, y);
    const T d = grid_sdf<T, MODE != OBS_DIST>(G, V, y, go) - spheres[s].r;
    if (MODE == OBS_DIST) {
      if (live) A.dist[b * S.n_sphere + S.sph_out[s]] = d;
    } else {
      T k;
      if (MODE == OBS_VJP) {
        k = A.gdist[b * S.n_sphere + S.sph_out[s]];
      } else {
        T h = A.margin - d;
        if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
        e = fma(h, h, e);
        k = T(-2) * h;
      }
      T n[3], f[3];
      obstacle_to_world(po, go, n);
#pragma unroll
      for (int i = 0; i < 3; ++i) f[i] = k * n[i];
      if (MODE == OBS_PENALTY) {
        const T arm[3] = {cen[3 * s] - po[0], cen[3 * s + 1] - po[1], cen[3 * s + 2] - po[2]};  // c_s - p_o
        T tq[3];
        cross_fma(arm, f, tq);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          wr[i] -= f[i];
          wr[3 + i] -= tq[i];
        }
      }
      T* fs = pk + Y.fbase + 3 * s;
      fs[0] = f[0];
      fs[1] = f[1];
      fs[2] = f[2];
    }
  }
  if (MODE == OBS_DIST) return;  // (no barrier follows in this form)
  if (MODE == OBS_PENALTY) {
    pk[Y.ebase + t] = e;
#pragma unroll
    for (int i = 0; i < 6; ++i) pk[Y.wbase + i * SPH_FANOUT + t] = wr[i];
  }
  __syncthreads();
  grid_columns<T, MODE == OBS_PENALTY>(P, S, ents, act_rng, act_col, col_act, n_act, pk, Y, t, live, b, A);
}

}  // namespace

struct dexr_sdf_grid {
  int32_t n[3] = {0, 0, 0};
  double origin[3] = {0, 0, 0}, spacing[3] = {0, 0, 0};
  GridD<float> f32;
  GridD<double> f64;
  float* values = nullptr;  // device, C order: the one copy of the samples
};

namespace {

template <typename T>
const GridD<T>& grid_desc_of(const dexr_sdf_grid* g);
template <>
const GridD<float>& grid_desc_of<float>(const dexr_sdf_grid* g) { return g->f32; }
template <>
const GridD<double>& grid_desc_of<double>(const dexr_sdf_grid* g) { return g->f64; }

// checks shared by the six entry points: < 0 error, 1 nothing to do, 0 go on
int check_grid_call(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const void* x, const void* fixed) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (!g) return dexr_set_error(DEXR_ERR_INVALID, "null sdf grid");
  return check_call(m->pose, B, x, fixed);
}

template <typename T>
int launch_grid(const dexr_sphere_model* sm, const dexr_sdf_grid* gr, int mode, int64_t B, const T* x, const T* fixed, const ObstacleArgs<T>& A,
                hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  // the sibling's region, frames per block and refusals (launch_obstacle): an odd stride, so that the frames of a wave start in
  // different banks
  const int stride = (mode == OBS_DIST ? 3 * sm->n_sphere + OBS_POSE : 6 * sm->n_sphere + 7 * SPH_FANOUT + OBS_POSE + 6 * m->n_jx) | 1;
  const size_t per_frame = ((size_t)m->h.n_slot * 12 + (size_t)stride) * sizeof(T);
  int nl = SPH_FRAMES;
  while (nl > 1 && per_frame * nl > 64 * 1024) nl /= 2;
  if (per_frame * nl > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the sphere model needs %zu B of LDS per frame: one frame does not fit a block", per_frame);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  const JointD<T>* js = tables_of<T>(m).joints;
  const LinkD<T>* ls = tables_of<T>(m).links;
  const SphereD<T>* sp = sphere_tables_of<T>(sm).spheres;
  const dim3 grid((unsigned)blocks), block(nl * SPH_FANOUT);
  const size_t lds = per_frame * nl;
#define GRID_LAUNCH(MODE)                                                                                                                   \
  hipLaunchKernelGGL((pose_grid_kernel<T, MODE>), grid, block, lds, st, js, ls, args_of<T>(m, B), sp, S, grid_desc_of<T>(gr),              \
                     (const float*)gr->values, (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col,    \
                     (const int32_t*)m->ik_col_act, m->n_act, stride, x, fixed, A)
  if (mode == OBS_DIST) GRID_LAUNCH(OBS_DIST);
  else if (mode == OBS_VJP) GRID_LAUNCH(OBS_VJP);
  else GRID_LAUNCH(OBS_PENALTY);
#undef GRID_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "sdf grid collision kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// the float64 host twin of all three forms: copy, run, synchronise
int host_grid(const dexr_sphere_model* sm, const dexr_sdf_grid* gr, int mode, int64_t B, const double* x, const double* fixed, const double* opos,
              const double* orot, const double* gdist, double margin, double* dist_out, double* e_out, double* gx_out, double* wr_out) {
  const dexr_pose_model* m = sm->pose;
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t ns = (size_t)B * sm->n_sphere * sizeof(double), nb = (size_t)B * sizeof(double);
  DevBuf dx, dfix, dp, dr, dg, dd, de, dgx, dwr;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (opos) POSE_HIP(dp.put(opos, 3 * nb));
  if (orot) POSE_HIP(dr.put(orot, 9 * nb));
  if (gdist) POSE_HIP(dg.put(gdist, ns));
  if (dist_out) POSE_HIP(dd.put(nullptr, ns));
  if (e_out) POSE_HIP(de.put(nullptr, nb));
  if (gx_out) POSE_HIP(dgx.put(nullptr, nx));
  if (wr_out) POSE_HIP(dwr.put(nullptr, 6 * nb));
  const ObstacleArgs<double> A = {(const double*)dp.p, (const double*)dr.p, (const double*)dg.p, margin,         (double*)dd.p,
                                  nullptr,             (double*)de.p,       (double*)dgx.p,      (double*)dwr.p};
  const int rc = launch_grid<double>(sm, gr, mode, B, (const double*)dx.p, (const double*)dfix.p, A, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (dist_out) POSE_HIP(hipMemcpy(dist_out, dd.p, ns, hipMemcpyDeviceToHost));
  if (e_out) POSE_HIP(hipMemcpy(e_out, de.p, nb, hipMemcpyDeviceToHost));
  if (gx_out && nx) POSE_HIP(hipMemcpy(gx_out, dgx.p, nx, hipMemcpyDeviceToHost));
  if (wr_out) POSE_HIP(hipMemcpy(wr_out, dwr.p, 6 * nb, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

template <typename T>
void fill_grid_desc(const dexr_sdf_grid* g, GridD<T>* D) {
  for (int a = 0; a < 3; ++a) {
    D->n[a] = g->n[a];
    D->origin[a] = (T)g->origin[a];
    D->h[a] = (T)g->spacing[a];
    D->inv[a] = (T)(1.0 / g->spacing[a]);
  }
  D->sy = g->n[2];
  D->sx = g->n[1] * g->n[2];
}

}  // namespace

extern "C" {

int dexr_sdf_grid_create(const int32_t n[3], const double origin[3], const double spacing[3], const float* values, dexr_sdf_grid** out) {
  if (!out) return dexr_set_error(DEXR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!n || !origin || !spacing || !values) return dexr_set_error(DEXR_ERR_INVALID, "null dimension, origin, spacing or value array");
  int64_t total = 1;
  for (int a = 0; a < 3; ++a) {
    if (n[a] < DEXR_SDF_GRID_MIN_DIM || n[a] > DEXR_SDF_GRID_MAX_DIM)
      return dexr_set_error(DEXR_ERR_INVALID, "grid dimension %d is %d (%d..%d)", a, n[a], DEXR_SDF_GRID_MIN_DIM, DEXR_SDF_GRID_MAX_DIM);
    total *= n[a];
  }
  if (total > DEXR_SDF_GRID_MAX_SAMPLES)
    return dexr_set_error(DEXR_ERR_INVALID, "the grid has %lld samples (at most %d)", (long long)total, DEXR_SDF_GRID_MAX_SAMPLES);
  for (int a = 0; a < 3; ++a) {
    if (!finite_d(spacing[a]) || !(spacing[a] > 0.0) || !finite_d(1.0 / spacing[a]))
      return dexr_set_error(DEXR_ERR_INVALID, "grid spacing %d must be finite and > 0, got %g", a, spacing[a]);
    if (!finite_d(origin[a])) return dexr_set_error(DEXR_ERR_INVALID, "grid origin %d is not finite", a);
  }
  for (int64_t i = 0; i < total; ++i)
    if (!finite_d((double)values[i])) return dexr_set_error(DEXR_ERR_INVALID, "grid sample %lld is not finite", (long long)i);
  dexr_sdf_grid* g = new (std::nothrow) dexr_sdf_grid();
  if (!g) return dexr_set_error(DEXR_ERR_INVALID, "out of host memory");
  for (int a = 0; a < 3; ++a) {
    g->n[a] = n[a];
    g->origin[a] = origin[a];
    g->spacing[a] = spacing[a];
  }
  fill_grid_desc<float>(g, &g->f32);
  fill_grid_desc<double>(g, &g->f64);
  hipError_t e = hipMalloc((void**)&g->values, (size_t)total * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(g->values, values, (size_t)total * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    dexr_sdf_grid_destroy(g);
    return dexr_set_error(DEXR_ERR_HIP, "uploading the sdf grid failed: %s", hipGetErrorString(e));
  }
  *out = g;
  return DEXR_OK;
}

void dexr_sdf_grid_destroy(dexr_sdf_grid* g) {
  if (!g) return;
  if (g->values) (void)hipFree(g->values);
  delete g;
}

int dexr_sdf_grid_info(const dexr_sdf_grid* g, int32_t* n, double* origin, double* spacing) {
  if (!g) return dexr_set_error(DEXR_ERR_INVALID, "null sdf grid");
  for (int a = 0; a < 3; ++a) {
    if (n) n[a] = g->n[a];
    if (origin) origin[a] = g->origin[a];
    if (spacing) spacing[a] = g->spacing[a];
  }
  return DEXR_OK;
}

int dexr_grid_distances_dev(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const float* x, const float* fixed,
                            const float* obstacle_pos, const float* obstacle_rot, float* dist_out, void* stream) {
  const int c = check_grid_call(m, g, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_out) return dexr_set_error(DEXR_ERR_INVALID, "dist_out is NULL");
  const ObstacleArgs<float> A = {obstacle_pos, obstacle_rot, nullptr, 0.f, dist_out, nullptr, nullptr, nullptr, nullptr};
  return launch_grid<float>(m, g, OBS_DIST, B, x, fixed, A, (hipStream_t)stream);
}

int dexr_grid_distances_vjp_dev(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const float* x, const float* fixed,
                                const float* obstacle_pos, const float* obstacle_rot, const float* grad_dist, float* grad_x_out,
                                void* stream) {
  const int c = check_grid_call(m, g, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_dist) return dexr_set_error(DEXR_ERR_INVALID, "grad_dist is NULL");
  if (!grad_x_out && m->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  const ObstacleArgs<float> A = {obstacle_pos, obstacle_rot, grad_dist, 0.f, nullptr, nullptr, nullptr, grad_x_out, nullptr};
  return launch_grid<float>(m, g, OBS_VJP, B, x, fixed, A, (hipStream_t)stream);
}

int dexr_grid_penalty_dev(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const float* x, const float* fixed,
                          const float* obstacle_pos, const float* obstacle_rot, float margin, float* energy_out, float* grad_x_out,
                          float* wrench_out, void* stream) {
  if (m && g && check_margin((double)margin)) return DEXR_ERR_INVALID;
  const int c = check_grid_call(m, g, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_x_out && !wrench_out) return dexr_set_error(DEXR_ERR_INVALID, "energy_out, grad_x_out and wrench_out are all NULL");
  const ObstacleArgs<float> A = {obstacle_pos, obstacle_rot, nullptr, margin, nullptr, nullptr, energy_out, grad_x_out, wrench_out};
  return launch_grid<float>(m, g, OBS_PENALTY, B, x, fixed, A, (hipStream_t)stream);
}

int dexr_grid_distances(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const double* x, const double* fixed,
                        const double* obstacle_pos, const double* obstacle_rot, double* dist_out) {
  const int c = check_grid_call(m, g, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_out) return dexr_set_error(DEXR_ERR_INVALID, "dist_out is NULL");
  return host_grid(m, g, OBS_DIST, B, x, fixed, obstacle_pos, obstacle_rot, nullptr, 0.0, dist_out, nullptr, nullptr, nullptr);
}

int dexr_grid_distances_vjp(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const double* x, const double* fixed,
                            const double* obstacle_pos, const double* obstacle_rot, const double* grad_dist, double* grad_x_out) {
  const int c = check_grid_call(m, g, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_dist) return dexr_set_error(DEXR_ERR_INVALID, "grad_dist is NULL");
  if (!grad_x_out && m->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  return host_grid(m, g, OBS_VJP, B, x, fixed, obstacle_pos, obstacle_rot, grad_dist, 0.0, nullptr, nullptr, grad_x_out, nullptr);
}

int dexr_grid_penalty(const dexr_sphere_model* m, const dexr_sdf_grid* g, int64_t B, const double* x, const double* fixed,
                      const double* obstacle_pos, const double* obstacle_rot, double margin, double* energy_out, double* grad_x_out,
                      double* wrench_out) {
  if (m && g && check_margin(margin)) return DEXR_ERR_INVALID;
  const int c = check_grid_call(m, g, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_x_out && !wrench_out) return dexr_set_error(DEXR_ERR_INVALID, "energy_out, grad_x_out and wrench_out are all NULL");
  return host_grid(m, g, OBS_PENALTY, B, x, fixed, obstacle_pos, obstacle_rot, nullptr, margin, nullptr, energy_out, grad_x_out, wrench_out);
}

}  // extern "C"

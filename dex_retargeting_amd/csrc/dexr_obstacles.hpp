// dexr_obstacles.hpp -- the robot's spheres against posed primitives (include/dexr_obstacles.h): a fragment of dexr_pose.hip,
// which includes it once at its end, after dexr_resolve.hpp (it shares the sphere model, sphere_centre, the block shape of
// pose_sphere_kernel, resolve_force_entry -- phase C of the sphere kernel as a function -- and DevBuf / POSE_HIP).
//
// One kernel, three forms (pose_obstacle_kernel<T, MODE>), the three-phase block of pose_sphere_kernel:
//   phase A (lane = frame, the first nl <= 16 lanes)   the forward walk of pose_sphere_kernel, restated: the sphere centres, and
//                                                      for the gradient forms a_k, o_k of every joint driven by x, go to the
//                                                      frame's region of LDS; the lane also parks the frame's obstacle pose
//                                                      (p_o, R_o; zeros and the identity where the caller left them out, so that
//                                                      both ways run the same arithmetic);
//   phase B (16 threads per frame)                     thread t owns the spheres t, t + 16, ...: it moves the centre into the
//                                                      obstacle frame once, y = R_o^T (c - p_o), and loops over the primitives in
//                                                      set order.  The distance form keeps the smallest d and the first m that
//                                                      attains it, the VJP form also that primitive's normal, the penalty form
//                                                      sums the force in the obstacle frame; the force goes back to the world
//                                                      frame (f = R_o f_obs) and into the frame's region.  Energy and wrench are
//                                                      per-thread partial sums, parked;
//   phase C (gradient forms)                           a thread per active column through resolve_force_entry (the arithmetic of
//                                                      pose_sphere_kernel's phase C), the columns no joint reads zeroed; thread 0
//                                                      adds the sixteen partial energies in order, threads 10 .. 15 each one
//                                                      component of the wrench, its sixteen partial sums in order.
//
// THE PRIMITIVE TABLE IS UNIFORM DATA: every thread of the launch reads primitive m at the same time.  It stays in global memory
// and is read through the scalar load path: the table pointer is a const __restrict__ kernel argument and the index is the
// loop counter alone, which the compiler proves uniform, so the record of a primitive (64 B in float32) arrives by s_load_dwordx4 /
// x8 in scalar registers that the vector instructions then read as operands -- no vector register, no LDS and no barrier is
// spent on it, and the 4 KB of a full set stay in the scalar cache.  A staged copy in LDS would cost every block a 4 KB copy and
// a barrier for data the scalar cache already holds, and LDS is what limits the frames per block of the large models.
//
// A frame's region of LDS is [frame][stride] with an odd stride, behind the fork slots ([value][lane]):
//   distance form   centres, 3 per sphere | obstacle pose, 12                                              3 n_sphere + 12
//   gradient forms  centres | forces, 3 per sphere | 16 partial energies | 16 x 6 partial wrenches |
//                   obstacle pose, 12 | a, o per joint driven by x                               6 n_sphere + 124 + 6 n_jx
// Every barrier is reached by every thread; every sum has a fixed order that does not depend on the frames per block.
#include "dexr_obstacles.h"

namespace {

constexpr int OBS_DIST = 0, OBS_VJP = 1, OBS_PENALTY = 2;
constexpr int OBS_POSE = 12;  // values of a parked obstacle pose: p_o (3), R_o (9, row-major)

// one primitive: the caller's sixteen parameters, v[15] replaced by 1 / |b - a|^2 of a capsule (0 where a == b: t = 0).  A table
// is DEXR_OBSTACLE_MAX records whatever the set holds, with the int32 kinds behind them (obstacle_kinds): one pointer for both, which
// the kernel has to keep in scalar registers across the whole of phase A
template <typename T>
struct ObstacleD {
  T v[DEXR_OBSTACLE_PARAMS];
};

template <typename T>
__host__ __device__ __forceinline__ const int32_t* obstacle_kinds(const ObstacleD<T>* table) {
  return reinterpret_cast<const int32_t*>(table + DEXR_OBSTACLE_MAX);
}

template <typename T>
struct ObstacleArgs {
  const T* opos;   // (B, 3) or NULL
  const T* orot;   // (B, 3, 3) or NULL
  const T* gdist;  // (B, n_sphere), the VJP form
  T margin;
  T* dist;           // (B, n_sphere) or NULL
  int32_t* nearest;  // (B, n_sphere) or NULL
  T* e_out;          // (B) or NULL
  T* gx;             // (B, n_in) or NULL
  T* wrench;         // (B, 6) or NULL
};

// sdf_m(y) and its gradient g in the obstacle frame (zero where there is no direction).  A NaN of y stays a NaN.
template <typename T>
__device__ __forceinline__ T obstacle_sdf(int kind, const ObstacleD<T>& Q, const T y[3], T g[3]) {
  const T* v = Q.v;
  if (kind == DEXR_OBSTACLE_HALFSPACE) {
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = v[i];
    return fma(v[2], y[2], fma(v[1], y[1], v[0] * y[0])) - v[3];
  }
  if (kind == DEXR_OBSTACLE_BOX) {
    const T d[3] = {y[0] - v[0], y[1] - v[1], y[2] - v[2]};
    T u[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // u = R^T (y - c)
      u[i] = fma(v[12 + i], d[2], fma(v[9 + i], d[1], v[6 + i] * d[0]));
      q[i] = fabs(u[i]) - v[3 + i];
    }
    int ax = 0;  // the first largest axis
    T mx = q[0];
    if (q[1] > mx) mx = q[1], ax = 1;
    if (q[2] > mx) mx = q[2], ax = 2;
    T gu[3], sdf;
    if (mx <= T(0)) {  // inside: the nearest face
      sdf = mx;
#pragma unroll
      for (int i = 0; i < 3; ++i) gu[i] = i == ax ? (u[i] < T(0) ? T(-1) : T(1)) : T(0);
    } else {  // (a comparison that keeps a NaN: q <= 0 ? 0 : q)
      const T m[3] = {q[0] <= T(0) ? T(0) : q[0], q[1] <= T(0) ? T(0) : q[1], q[2] <= T(0) ? T(0) : q[2]};
      sdf = sqrt(fma(m[2], m[2], fma(m[1], m[1], m[0] * m[0])));
#pragma unroll
      for (int i = 0; i < 3; ++i) gu[i] = (u[i] < T(0) ? -m[i] : m[i]) / sdf;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = fma(v[6 + 3 * i + 2], gu[2], fma(v[6 + 3 * i + 1], gu[1], v[6 + 3 * i] * gu[0]));
    return sdf;
  }
  // a capsule; a sphere is the capsule with a == b (its b and 1 / |b - a|^2 are zeros: t = 0)
  const bool cap = kind == DEXR_OBSTACLE_CAPSULE;
  const T ab[3] = {cap ? v[3] - v[0] : T(0), cap ? v[4] - v[1] : T(0), cap ? v[5] - v[2] : T(0)};
  const T r = cap ? v[6] : v[3], inv = cap ? v[15] : T(0);
  T d[3] = {y[0] - v[0], y[1] - v[1], y[2] - v[2]};
  T t = fma(d[2], ab[2], fma(d[1], ab[1], d[0] * ab[0])) * inv;
  t = t < T(0) ? T(0) : (t > T(1) ? T(1) : t);
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = fma(-t, ab[i], d[i]);
  const T s = sqrt(fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])));
  const T k = s > T(0) ? T(1) / s : s * T(0);  // on the centre or the axis: no direction (a NaN of s stays one)
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = k * d[i];
  return s - r;
}

template <typename T, int MODE>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES) pose_obstacle_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                               PoseArgs<T> P, const SphereD<T>* __restrict__ spheres, SphereIndex S,
                                                                               const ObstacleD<T>* __restrict__ prims, const T* __restrict__ pw,
                                                                               int n_prim, const JacEnt* __restrict__ ents,
                                                                               const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col,
                                                                               const int32_t* __restrict__ col_act, int n_act, int stride,
                                                                               const T* __restrict__ x, const T* __restrict__ fixed, ObstacleArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* park = slots + (size_t)P.n_slot * 12 * nl;
  // offsets into a frame's region: all from n_sphere alone, the a, o records last (nothing derived from n_jx has to be kept)
  const int fbase = 3 * S.n_sphere, ebase = fbase + 3 * S.n_sphere, wbase = ebase + SPH_FANOUT;
  const int obase = MODE == OBS_DIST ? fbase : wbase + 6 * SPH_FANOUT, abase = obase + OBS_POSE;
  const int64_t first = (int64_t)blockIdx.x * nl;
  if (tid < nl) {  // phase A: lane = frame
    const int lane = tid;
    T* pk = park + (size_t)lane * stride;
    T* cen = pk;
    const int64_t b = first + lane < P.B ? first + lane : P.B - 1;  // ragged tail: idle lanes park the last frame again
    T* po = pk + obase;
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
      if (MODE != OBS_DIST && J.src_kind == DEXR_POSE_SRC_X) {
        T* d = pk + abase + 6 * xi;
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
  __syncthreads();
  // phase B: SPH_FANOUT threads per frame, a thread per sphere, the primitives in set order
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  T* pk = park + (size_t)fr * stride;
  const T* cen = pk;
  const bool live = first + fr < P.B;
  const int64_t b = live ? first + fr : P.B - 1;
  T po[3], Ro[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) po[i] = pk[obase + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) Ro[i] = pk[obase + 3 + i];
  const int32_t* kinds = obstacle_kinds(prims);
  T e = T(0), wr[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  for (int s = t; s < S.n_sphere; s += SPH_FANOUT) {
    const T arm[3] = {cen[3 * s] - po[0], cen[3 * s + 1] - po[1], cen[3 * s + 2] - po[2]};  // c_s - p_o
    T y[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = fma(Ro[6 + i], arm[2], fma(Ro[3 + i], arm[1], Ro[i] * arm[0]));  // R_o^T (c_s - p_o)
    const T rs = spheres[s].r;
    T fo[3] = {T(0), T(0), T(0)};  // the force (or the nearest normal) in the obstacle frame
    T best = T(0);
    int near = 0;
    for (int m = 0; m < n_prim; ++m) {
      T g[3];
      const T d = obstacle_sdf(kinds[m], prims[m], y, g) - rs;
      if (MODE == OBS_PENALTY) {
        T h = A.margin - d;
        if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
        const T wh = pw ? pw[m] * h : h;
        e = fma(wh, h, e);
        const T k = T(-2) * wh;
#pragma unroll
        for (int i = 0; i < 3; ++i) fo[i] = fma(k, g[i], fo[i]);
      } else if (m == 0 || d < best) {  // the first that attains the minimum (a NaN of the first d stays)
        best = d;
        near = m;
        if (MODE == OBS_VJP) {
#pragma unroll
          for (int i = 0; i < 3; ++i) fo[i] = g[i];
        }
      }
    }
    if (MODE == OBS_DIST) {
      if (live) {
        const int64_t o = b * S.n_sphere + S.sph_out[s];
        if (A.dist) A.dist[o] = best;
        if (A.nearest) A.nearest[o] = near;
      }
    } else {
      T f[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) f[i] = fma(Ro[3 * i + 2], fo[2], fma(Ro[3 * i + 1], fo[1], Ro[3 * i] * fo[0]));  // R_o f_obs
      if (MODE == OBS_VJP) {
        const T gd = A.gdist[b * S.n_sphere + S.sph_out[s]];
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i] *= gd;
      } else {
        T tq[3];
        cross_fma(arm, f, tq);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          wr[i] -= f[i];
          wr[3 + i] -= tq[i];
        }
      }
      T* fs = pk + fbase + 3 * s;
      fs[0] = f[0];
      fs[1] = f[1];
      fs[2] = f[2];
    }
  }
  if (MODE == OBS_DIST) return;  // (no barrier follows in this form)
  if (MODE == OBS_PENALTY) {
    pk[ebase + t] = e;
#pragma unroll
    for (int i = 0; i < 6; ++i) pk[wbase + i * SPH_FANOUT + t] = wr[i];
  }
  __syncthreads();
  // phase C: a thread per active column, then the columns no joint reads
  if (A.gx) {
    const T* frc = pk + fbase;
    for (int i = t; i < n_act; i += SPH_FANOUT) {
      const T g = resolve_force_entry(act_rng[i], ents, S.link_sph, pk + abase, cen, frc);
      if (live) A.gx[b * P.n_in + act_col[i]] = g;
    }
    if (live) {
      T* o = A.gx + b * P.n_in;
      for (int c = t; c < P.n_in; c += SPH_FANOUT)
        if (col_act[c] < 0) o[c] = T(0);
    }
  }
  if (MODE == OBS_PENALTY && live) {
    if (A.e_out && t == 0) {
      T E = pk[ebase];
      for (int i = 1; i < SPH_FANOUT; ++i) E += pk[ebase + i];
      A.e_out[b] = E;
    }
    if (A.wrench && t >= SPH_FANOUT - 6) {
      const int c = t - (SPH_FANOUT - 6);
      const T* w = pk + wbase + c * SPH_FANOUT;
      T W = w[0];
      for (int i = 1; i < SPH_FANOUT; ++i) W += w[i];
      A.wrench[b * 6 + c] = W;
    }
  }
}

}  // namespace

struct dexr_obstacle_set {
  int n_prim = 0;
  ObstacleD<float>* f32 = nullptr;  // each: DEXR_OBSTACLE_MAX records, then DEXR_OBSTACLE_MAX kinds
  ObstacleD<double>* f64 = nullptr;
};

namespace {

template <typename T>
const ObstacleD<T>* obstacle_table_of(const dexr_obstacle_set* o);
template <>
const ObstacleD<float>* obstacle_table_of<float>(const dexr_obstacle_set* o) { return o->f32; }
template <>
const ObstacleD<double>* obstacle_table_of<double>(const dexr_obstacle_set* o) { return o->f64; }

// checks shared by the six entry points: < 0 error, 1 nothing to do, 0 go on
int check_obstacle_call(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const void* x, const void* fixed) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (!o) return dexr_set_error(DEXR_ERR_INVALID, "null obstacle set");
  return check_call(m->pose, B, x, fixed);
}

template <typename T>
int launch_obstacle(const dexr_sphere_model* sm, const dexr_obstacle_set* os, int mode, int64_t B, const T* x, const T* fixed, const T* pw,
                    const ObstacleArgs<T>& A, hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  // values of a frame's region (the list at the head of this file); odd, so that the frames of a wave start in different banks
  const int stride = (mode == OBS_DIST ? 3 * sm->n_sphere + OBS_POSE : 6 * sm->n_sphere + 7 * SPH_FANOUT + OBS_POSE + 6 * m->n_jx) | 1;
  const size_t per_frame = ((size_t)m->h.n_slot * 12 + (size_t)stride) * sizeof(T);
  int nl = SPH_FRAMES;
  while (nl > 1 && per_frame * nl > 64 * 1024) nl /= 2;  // (float64, 8 slots, 64 joints, 128 spheres: 4 frames)
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
#define OBS_LAUNCH(MODE)                                                                                                                     \
  hipLaunchKernelGGL((pose_obstacle_kernel<T, MODE>), grid, block, lds, st, js, ls, args_of<T>(m, B), sp, S, obstacle_table_of<T>(os),        \
                     pw, os->n_prim, (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng,                  \
                     (const int32_t*)m->ik_act_col, (const int32_t*)m->ik_col_act, m->n_act, stride, x, fixed, A)
  if (mode == OBS_DIST) OBS_LAUNCH(OBS_DIST);
  else if (mode == OBS_VJP) OBS_LAUNCH(OBS_VJP);
  else OBS_LAUNCH(OBS_PENALTY);
#undef OBS_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "obstacle collision kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// the float64 host twin of all three forms: copy, run, synchronise
int host_obstacle(const dexr_sphere_model* sm, const dexr_obstacle_set* os, int mode, int64_t B, const double* x, const double* fixed,
                  const double* opos, const double* orot, const double* gdist, double margin, const double* pw, double* dist_out,
                  int32_t* near_out, double* e_out, double* gx_out, double* wr_out) {
  const dexr_pose_model* m = sm->pose;
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t ns = (size_t)B * sm->n_sphere * sizeof(double), ni = (size_t)B * sm->n_sphere * sizeof(int32_t), nb = (size_t)B * sizeof(double);
  DevBuf dx, dfix, dp, dr, dg, dw, dd, dn, de, dgx, dwr;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (opos) POSE_HIP(dp.put(opos, 3 * nb));
  if (orot) POSE_HIP(dr.put(orot, 9 * nb));
  if (gdist) POSE_HIP(dg.put(gdist, ns));
  if (pw) POSE_HIP(dw.put(pw, (size_t)os->n_prim * sizeof(double)));
  if (dist_out) POSE_HIP(dd.put(nullptr, ns));
  if (near_out) POSE_HIP(dn.put(nullptr, ni));
  if (e_out) POSE_HIP(de.put(nullptr, nb));
  if (gx_out) POSE_HIP(dgx.put(nullptr, nx));
  if (wr_out) POSE_HIP(dwr.put(nullptr, 6 * nb));
  const ObstacleArgs<double> A = {(const double*)dp.p, (const double*)dr.p, (const double*)dg.p, margin,         (double*)dd.p,
                                  (int32_t*)dn.p,      (double*)de.p,       (double*)dgx.p,      (double*)dwr.p};
  const int rc = launch_obstacle<double>(sm, os, mode, B, (const double*)dx.p, (const double*)dfix.p, (const double*)dw.p, A, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (dist_out) POSE_HIP(hipMemcpy(dist_out, dd.p, ns, hipMemcpyDeviceToHost));
  if (near_out) POSE_HIP(hipMemcpy(near_out, dn.p, ni, hipMemcpyDeviceToHost));
  if (e_out) POSE_HIP(hipMemcpy(e_out, de.p, nb, hipMemcpyDeviceToHost));
  if (gx_out && nx) POSE_HIP(hipMemcpy(gx_out, dgx.p, nx, hipMemcpyDeviceToHost));
  if (wr_out) POSE_HIP(hipMemcpy(wr_out, dwr.p, 6 * nb, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

template <typename T>
hipError_t upload_obstacle_table(const std::vector<ObstacleD<double>>& prims, const std::vector<int32_t>& kinds, ObstacleD<T>** out) {
  const size_t rec = DEXR_OBSTACLE_MAX * sizeof(ObstacleD<T>), all = rec + DEXR_OBSTACLE_MAX * sizeof(int32_t);
  std::vector<unsigned char> image(all, 0);
  ObstacleD<T>* p = reinterpret_cast<ObstacleD<T>*>(image.data());
  for (size_t i = 0; i < prims.size(); ++i)
    for (int k = 0; k < DEXR_OBSTACLE_PARAMS; ++k) p[i].v[k] = (T)prims[i].v[k];
  memcpy(image.data() + rec, kinds.data(), kinds.size() * sizeof(int32_t));
  hipError_t e = hipMalloc((void**)out, all);
  if (e == hipSuccess) e = hipMemcpy(*out, image.data(), all, hipMemcpyHostToDevice);
  return e;
}

}  // namespace

extern "C" {

int dexr_obstacle_set_create(int32_t n_prim, const int32_t* kind, const double* param, dexr_obstacle_set** out) {
  if (!out) return dexr_set_error(DEXR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (n_prim < 1 || n_prim > DEXR_OBSTACLE_MAX)
    return dexr_set_error(DEXR_ERR_INVALID, "obstacle set has %d primitives (1..%d)", n_prim, DEXR_OBSTACLE_MAX);
  if (!kind || !param) return dexr_set_error(DEXR_ERR_INVALID, "null kind or parameter array");
  const double tol = 1e-6;
  std::vector<ObstacleD<double>> prims(n_prim);
  std::vector<int32_t> kinds(kind, kind + n_prim);
  for (int m = 0; m < n_prim; ++m) {
    const double* v = param + (size_t)m * DEXR_OBSTACLE_PARAMS;
    if (kind[m] < DEXR_OBSTACLE_SPHERE || kind[m] > DEXR_OBSTACLE_HALFSPACE)
      return dexr_set_error(DEXR_ERR_INVALID, "primitive %d: unknown kind %d", m, kind[m]);
    for (int k = 0; k < DEXR_OBSTACLE_PARAMS; ++k)
      if (!finite_d(v[k])) return dexr_set_error(DEXR_ERR_INVALID, "primitive %d: parameter %d is not finite", m, k);
    for (int k = 0; k < DEXR_OBSTACLE_PARAMS; ++k) prims[m].v[k] = v[k];
    if (kind[m] == DEXR_OBSTACLE_SPHERE || kind[m] == DEXR_OBSTACLE_CAPSULE) {
      const double r = v[kind[m] == DEXR_OBSTACLE_SPHERE ? 3 : 6];
      if (r < 0.0) return dexr_set_error(DEXR_ERR_INVALID, "primitive %d: radius must be >= 0, got %g", m, r);
      prims[m].v[15] = 0.0;
      if (kind[m] == DEXR_OBSTACLE_CAPSULE) {
        double l2 = 0.0;
        for (int i = 0; i < 3; ++i) l2 += (v[3 + i] - v[i]) * (v[3 + i] - v[i]);
        if (l2 > 0.0 && finite_d(1.0 / l2)) prims[m].v[15] = 1.0 / l2;
      }
    } else if (kind[m] == DEXR_OBSTACLE_BOX) {
      for (int i = 0; i < 3; ++i)
        if (!(v[3 + i] > 0.0)) return dexr_set_error(DEXR_ERR_INVALID, "primitive %d: half extent %d must be > 0, got %g", m, i, v[3 + i]);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {  // R^T R = I
          double s = i == j ? -1.0 : 0.0;
          for (int k = 0; k < 3; ++k) s += v[6 + 3 * k + i] * v[6 + 3 * k + j];
          if (!(s <= tol && s >= -tol)) return dexr_set_error(DEXR_ERR_INVALID, "primitive %d: the box rotation is not orthonormal to %g", m, tol);
        }
    } else {
      const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
      const double d = (n2 < 0.0 ? 0.0 : __builtin_sqrt(n2)) - 1.0;
      if (!(d <= tol && d >= -tol)) return dexr_set_error(DEXR_ERR_INVALID, "primitive %d: the half-space normal is not unit to %g", m, tol);
    }
  }
  dexr_obstacle_set* o = new (std::nothrow) dexr_obstacle_set();
  if (!o) return dexr_set_error(DEXR_ERR_INVALID, "out of host memory");
  o->n_prim = n_prim;
  hipError_t e = upload_obstacle_table<float>(prims, kinds, &o->f32);
  if (e == hipSuccess) e = upload_obstacle_table<double>(prims, kinds, &o->f64);
  if (e != hipSuccess) {
    dexr_obstacle_set_destroy(o);
    return dexr_set_error(DEXR_ERR_HIP, "uploading obstacle tables failed: %s", hipGetErrorString(e));
  }
  *out = o;
  return DEXR_OK;
}

void dexr_obstacle_set_destroy(dexr_obstacle_set* o) {
  if (!o) return;
  if (o->f32) (void)hipFree(o->f32);
  if (o->f64) (void)hipFree(o->f64);
  delete o;
}

int dexr_obstacle_set_info(const dexr_obstacle_set* o, int32_t* n_prim) {
  if (!o) return dexr_set_error(DEXR_ERR_INVALID, "null obstacle set");
  if (n_prim) *n_prim = o->n_prim;
  return DEXR_OK;
}

int dexr_obstacle_distances_dev(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const float* x, const float* fixed,
                                const float* obstacle_pos, const float* obstacle_rot, float* dist_out, int32_t* nearest_out, void* stream) {
  const int c = check_obstacle_call(m, o, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_out && !nearest_out) return dexr_set_error(DEXR_ERR_INVALID, "dist_out and nearest_out are both NULL");
  const ObstacleArgs<float> A = {obstacle_pos, obstacle_rot, nullptr, 0.f, dist_out, nearest_out, nullptr, nullptr, nullptr};
  return launch_obstacle<float>(m, o, OBS_DIST, B, x, fixed, nullptr, A, (hipStream_t)stream);
}

int dexr_obstacle_distances_vjp_dev(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const float* x, const float* fixed,
                                    const float* obstacle_pos, const float* obstacle_rot, const float* grad_dist, float* grad_x_out,
                                    void* stream) {
  const int c = check_obstacle_call(m, o, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_dist) return dexr_set_error(DEXR_ERR_INVALID, "grad_dist is NULL");
  if (!grad_x_out && m->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  const ObstacleArgs<float> A = {obstacle_pos, obstacle_rot, grad_dist, 0.f, nullptr, nullptr, nullptr, grad_x_out, nullptr};
  return launch_obstacle<float>(m, o, OBS_VJP, B, x, fixed, nullptr, A, (hipStream_t)stream);
}

int dexr_obstacle_penalty_dev(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const float* x, const float* fixed,
                              const float* obstacle_pos, const float* obstacle_rot, float margin, const float* prim_weight,
                              float* energy_out, float* grad_x_out, float* wrench_out, void* stream) {
  if (m && o && check_margin((double)margin)) return DEXR_ERR_INVALID;
  const int c = check_obstacle_call(m, o, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_x_out && !wrench_out) return dexr_set_error(DEXR_ERR_INVALID, "energy_out, grad_x_out and wrench_out are all NULL");
  const ObstacleArgs<float> A = {obstacle_pos, obstacle_rot, nullptr, margin, nullptr, nullptr, energy_out, grad_x_out, wrench_out};
  return launch_obstacle<float>(m, o, OBS_PENALTY, B, x, fixed, prim_weight, A, (hipStream_t)stream);
}

int dexr_obstacle_distances(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const double* x, const double* fixed,
                            const double* obstacle_pos, const double* obstacle_rot, double* dist_out, int32_t* nearest_out) {
  const int c = check_obstacle_call(m, o, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_out && !nearest_out) return dexr_set_error(DEXR_ERR_INVALID, "dist_out and nearest_out are both NULL");
  return host_obstacle(m, o, OBS_DIST, B, x, fixed, obstacle_pos, obstacle_rot, nullptr, 0.0, nullptr, dist_out, nearest_out, nullptr, nullptr,
                       nullptr);
}

int dexr_obstacle_distances_vjp(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const double* x, const double* fixed,
                                const double* obstacle_pos, const double* obstacle_rot, const double* grad_dist, double* grad_x_out) {
  const int c = check_obstacle_call(m, o, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_dist) return dexr_set_error(DEXR_ERR_INVALID, "grad_dist is NULL");
  if (!grad_x_out && m->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  return host_obstacle(m, o, OBS_VJP, B, x, fixed, obstacle_pos, obstacle_rot, grad_dist, 0.0, nullptr, nullptr, nullptr, nullptr, grad_x_out,
                       nullptr);
}

int dexr_obstacle_penalty(const dexr_sphere_model* m, const dexr_obstacle_set* o, int64_t B, const double* x, const double* fixed,
                          const double* obstacle_pos, const double* obstacle_rot, double margin, const double* prim_weight,
                          double* energy_out, double* grad_x_out, double* wrench_out) {
  if (m && o && check_margin(margin)) return DEXR_ERR_INVALID;
  const int c = check_obstacle_call(m, o, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_x_out && !wrench_out) return dexr_set_error(DEXR_ERR_INVALID, "energy_out, grad_x_out and wrench_out are all NULL");
  return host_obstacle(m, o, OBS_PENALTY, B, x, fixed, obstacle_pos, obstacle_rot, nullptr, margin, prim_weight, nullptr, nullptr, energy_out,
                       grad_x_out, wrench_out);
}

}  // extern "C"

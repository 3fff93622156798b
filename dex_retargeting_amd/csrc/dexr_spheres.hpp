// dexr_spheres.hpp -- sphere-pair self-collision on a pose table (include/dexr_spheres.h): the last part of dexr_pose.hip, which
// includes it once at its end (it shares joint_step, link_pose, the fork slots, JacEnt and the active-column index of the IK
// kernels, and parse_pose_blob / upload_pose_model).
//
// One kernel, three forms (pose_sphere_kernel<T, MODE>), the two-phase block of the IK kernels with a third phase:
//   phase A (lane = frame, the first nl <= 16 lanes)   the forward walk; per link at its sorted position the centres of its
//                                                      spheres (sorted by their link's sorted position at create time) go to the
//                                                      frame's region of LDS; the gradient forms also park a_k, o_k of every
//                                                      joint driven by x;
//   phase B (16 threads per frame)                     thread t owns the spheres t, t + 16, ...: per sphere it walks the
//                                                      sphere's incident pairs (a CSR list sphere -> other sphere, pair,
//                                                      first-end flag), so a pair is evaluated from both of its ends -- D, s_p and
//                                                      d_p are the same bits from either end, c_i - c_j being the exact
//                                                      negative of c_j - c_i -- and sums the force f_s = sum g_p (c_s - c_other) /
//                                                      s_p in registers, then parks it.  The end listed first stores dist and
//                                                      adds to the thread's partial energy;
//   phase C (gradient forms)                           one thread per active column: over the joints of the column and the
//                                                      contiguous sphere range below each, mult_k a_k . ((c_s - o_k) x f_s)
//                                                      (revolute) or mult_k a_k . f_s (prismatic); the columns no joint reads
//                                                      are zeroed from the active-column index; thread 0 adds the sixteen
//                                                      partial energies in order.
// A frame's region of LDS is [frame][stride] with an odd stride, behind the fork slots ([value][lane]), as in the IK kernels:
//   a, o per joint driven by x (gradient forms) | centres, 3 per sphere | forces, 3 per sphere | 16 partial energies.
// Every barrier is reached by every thread; every sum has a fixed order that does not depend on the frames per block.
#include "dexr_spheres.h"

namespace {

constexpr int SPH_FANOUT = 16;  // threads of a block per frame it holds
constexpr int SPH_FRAMES = 16;  // most frames of a block (256 threads)
constexpr int SPH_DIST = 0, SPH_VJP = 1, SPH_PENALTY = 2;

// incidence entry of a sphere: the other sphere (sorted index) | first-end flag << 7 | pair (caller's index) << 8
constexpr uint32_t SPH_FIRST = 1u << 7;

template <typename T>
struct SphereD {
  T c[3], r;  // centre in the link's frame; the radius fills the record to four values (the kernels read r_i + r_j per pair: rsum)
};

template <typename T>
struct SphereTables {
  SphereD<T>* spheres = nullptr;  // (n_sphere), sorted by the sorted position of their link
  T* rsum = nullptr;              // (n_pair): r_i + r_j
};

struct SphereIndex {
  const int32_t* link_sph;  // (n_link + 1): the spheres of sorted link l are [link_sph[l], link_sph[l + 1])
  const int32_t* sph_out;   // (n_sphere): the caller's index of a sorted sphere
  const int32_t* inc_ptr;   // (n_sphere + 1)
  const uint32_t* inc;      // (2 n_pair)
  int32_t n_sphere, n_pair;
};

// c = p + R v
template <typename T>
__device__ __forceinline__ void sphere_centre(const T R[9], const T p[3], const SphereD<T>& S, T* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = fma(R[3 * i + 2], S.c[2], fma(R[3 * i + 1], S.c[1], fma(R[3 * i], S.c[0], p[i])));
}

template <typename T, int MODE>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES) pose_sphere_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                             PoseArgs<T> P, const SphereD<T>* __restrict__ spheres,
                                                                             const T* __restrict__ rsum, SphereIndex S,
                                                                             const JacEnt* __restrict__ ents, const uint32_t* __restrict__ act_rng,
                                                                             const int32_t* __restrict__ act_col, const int32_t* __restrict__ col_act,
                                                                             int n_jx, int n_act, int stride, const T* __restrict__ x,
                                                                             const T* __restrict__ fixed, const T* __restrict__ gdist, T margin,
                                                                             const T* __restrict__ pw, T* __restrict__ dist, T* __restrict__ cen_out,
                                                                             T* __restrict__ e_out, T* __restrict__ gx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* park = slots + (size_t)P.n_slot * 12 * nl;
  const int cbase = MODE == SPH_DIST ? 0 : 6 * n_jx, fbase = cbase + 3 * S.n_sphere, ebase = fbase + 3 * S.n_sphere;
  const int64_t first = (int64_t)blockIdx.x * nl;
  if (tid < nl) {  // phase A: lane = frame
    const int lane = tid;
    T* pk = park + (size_t)lane * stride;
    T* cen = pk + cbase;
    const int64_t b = first + lane < P.B ? first + lane : P.B - 1;  // ragged tail: idle lanes park the last frame again
    for (int l = 0; l < P.n_base; ++l) {                            // spheres on the fixed base: constant centres
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
      if (MODE != SPH_DIST && J.src_kind == DEXR_POSE_SRC_X) {
        T* d = pk + 6 * xi;
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
  // phase B: SPH_FANOUT threads per frame, a thread per sphere
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  T* pk = park + (size_t)fr * stride;
  const T* cen = pk + cbase;
  const bool live = first + fr < P.B;
  const int64_t b = live ? first + fr : P.B - 1;
  T e = T(0);
  for (int s = t; s < S.n_sphere; s += SPH_FANOUT) {
    const T c0 = cen[3 * s], c1 = cen[3 * s + 1], c2 = cen[3 * s + 2];
    T f0 = T(0), f1 = T(0), f2 = T(0);
    const int i1 = S.inc_ptr[s + 1];
    for (int i = S.inc_ptr[s]; i < i1; ++i) {
      const uint32_t u = S.inc[i];
      const int o = u & 127, p = u >> 8;
      const bool head = (u & SPH_FIRST) != 0;
      const T d0 = c0 - cen[3 * o], d1 = c1 - cen[3 * o + 1], d2 = c2 - cen[3 * o + 2];
      const T sp = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)));
      const T d = sp - rsum[p];
      if (MODE == SPH_DIST) {
        if (head && live) dist[b * S.n_pair + p] = d;
      } else {
        T g;
        if (MODE == SPH_VJP) {
          g = gdist[b * S.n_pair + p];
        } else {
          T h = margin - d;
          if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
          const T wh = pw ? pw[p] * h : h;
          if (head) e = fma(wh, h, e);
          g = T(-2) * wh;
        }
        const T k = sp > T(0) ? g / sp : g * (sp * T(0));  // coincident centres: no direction (a NaN of g or of sp stays one)
        f0 = fma(k, d0, f0);
        f1 = fma(k, d1, f1);
        f2 = fma(k, d2, f2);
      }
    }
    if (MODE == SPH_DIST) {
      if (cen_out && live) {
        T* co = cen_out + (b * S.n_sphere + S.sph_out[s]) * 3;
        co[0] = c0;
        co[1] = c1;
        co[2] = c2;
      }
    } else {
      T* f = pk + fbase + 3 * s;
      f[0] = f0;
      f[1] = f1;
      f[2] = f2;
    }
  }
  if (MODE == SPH_DIST) return;  // (no barrier follows in this form)
  if (MODE == SPH_PENALTY) pk[ebase + t] = e;
  __syncthreads();
  // phase C: a thread per active column, then the columns no joint reads
  if (gx) {
    const T* frc = pk + fbase;
    for (int i = t; i < n_act; i += SPH_FANOUT) {
      const uint32_t r = act_rng[i];
      T g = T(0);
      for (int ii = r & 255; ii < (int)(r >> 8); ++ii) {
        const JacEnt A = ents[ii];
        const T* a = pk + 6 * A.xi;  // a[0..2] world axis, a[3..5] world origin
        const bool rev = A.type == DEXR_POSE_REVOLUTE;
        const int s1 = S.link_sph[A.sub_end];
        T sl = T(0);
        for (int s = S.link_sph[A.link_begin]; s < s1; ++s) {
          const T f[3] = {frc[3 * s], frc[3 * s + 1], frc[3 * s + 2]};
          const T ax[3] = {a[0], a[1], a[2]};
          if (rev) {
            const T d[3] = {cen[3 * s] - a[3], cen[3 * s + 1] - a[4], cen[3 * s + 2] - a[5]};
            T m[3];
            cross_fma(d, f, m);
            sl += dot_fma(ax, m);
          } else {
            sl += dot_fma(ax, f);
          }
        }
        g = fma(mult_of(A, T(0)), sl, g);
      }
      if (live) gx[b * P.n_in + act_col[i]] = g;
    }
    if (live) {
      T* o = gx + b * P.n_in;
      for (int c = t; c < P.n_in; c += SPH_FANOUT)
        if (col_act[c] < 0) o[c] = T(0);
    }
  }
  if (MODE == SPH_PENALTY && e_out && t == 0 && live) {
    T E = pk[ebase];
    for (int i = 1; i < SPH_FANOUT; ++i) E += pk[ebase + i];
    e_out[b] = E;
  }
}

}  // namespace

struct dexr_sphere_model {
  dexr_pose_model* pose = nullptr;
  int n_sphere = 0, n_pair = 0;
  SphereTables<float> f32;
  SphereTables<double> f64;
  int32_t* link_sph = nullptr;
  int32_t* sph_out = nullptr;
  int32_t* inc_ptr = nullptr;
  uint32_t* inc = nullptr;
  uint32_t* pair_sph = nullptr;  // (n_pair): the two spheres of a pair by sorted index, first | second << 7 (dexr_resolve.hpp)
  int32_t* sph_in = nullptr;     // (n_sphere): the sorted index of the caller's sphere, the inverse of sph_out (dexr_resolve_obstacles.hpp)
};

namespace {

template <typename T>
const SphereTables<T>& sphere_tables_of(const dexr_sphere_model* m);
template <>
const SphereTables<float>& sphere_tables_of<float>(const dexr_sphere_model* m) { return m->f32; }
template <>
const SphereTables<double>& sphere_tables_of<double>(const dexr_sphere_model* m) { return m->f64; }

template <typename T>
hipError_t upload_sphere_tables(const std::vector<SphereD<double>>& sph, const std::vector<double>& rsum, SphereTables<T>& out) {
  std::vector<SphereD<T>> s(sph.size());
  std::vector<T> r(rsum.size());
  for (size_t i = 0; i < sph.size(); ++i) {
    for (int k = 0; k < 3; ++k) s[i].c[k] = (T)sph[i].c[k];
    s[i].r = (T)sph[i].r;
  }
  for (size_t i = 0; i < rsum.size(); ++i) r[i] = (T)rsum[i];
  hipError_t e = hipMalloc((void**)&out.spheres, s.size() * sizeof(SphereD<T>));
  if (e == hipSuccess) e = hipMalloc((void**)&out.rsum, r.size() * sizeof(T));
  if (e == hipSuccess) e = hipMemcpy(out.spheres, s.data(), s.size() * sizeof(SphereD<T>), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(out.rsum, r.data(), r.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

template <typename V>
hipError_t upload_vector(const std::vector<V>& v, V** out) {
  hipError_t e = hipMalloc((void**)out, (v.size() + 1) * sizeof(V));
  if (e == hipSuccess && !v.empty()) e = hipMemcpy(*out, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice);
  return e;
}

// checks shared by the six entry points: < 0 error, 1 nothing to do, 0 go on
int check_sphere_call(const dexr_sphere_model* m, int64_t B, const void* x, const void* fixed) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  return check_call(m->pose, B, x, fixed);
}

int check_margin(double margin) {
  if (!(margin >= 0.0) || margin > 1.7976931348623157e308) return dexr_set_error(DEXR_ERR_INVALID, "margin must be finite and >= 0, got %g", margin);
  return 0;
}

template <typename T>
int launch_sphere(const dexr_sphere_model* sm, int mode, int64_t B, const T* x, const T* fixed, const T* gdist, T margin, const T* pw, T* dist,
                  T* cen, T* e_out, T* gx, hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  // values of a frame's region: a, o per joint driven by x | centres | forces | sixteen partial energies (the distance form:
  // the centres alone); odd, so that the frames of a wave start in different banks
  const int stride = (mode == SPH_DIST ? 3 * sm->n_sphere : 6 * m->n_jx + 6 * sm->n_sphere + SPH_FANOUT) | 1;
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
  const T* rs = sphere_tables_of<T>(sm).rsum;
  const dim3 grid((unsigned)blocks), block(nl * SPH_FANOUT);
  const size_t lds = per_frame * nl;
#define SPH_LAUNCH(MODE)                                                                                                                        \
  hipLaunchKernelGGL((pose_sphere_kernel<T, MODE>), grid, block, lds, st, js, ls, args_of<T>(m, B), sp, rs, S, (const JacEnt*)m->jac_ents,     \
                     (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col, (const int32_t*)m->ik_col_act, m->n_jx, m->n_act, stride, x, \
                     fixed, gdist, margin, pw, dist, cen, e_out, gx)
  if (mode == SPH_DIST) SPH_LAUNCH(SPH_DIST);
  else if (mode == SPH_VJP) SPH_LAUNCH(SPH_VJP);
  else SPH_LAUNCH(SPH_PENALTY);
#undef SPH_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "sphere collision kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// the float64 host twin of all three forms: copy, run, synchronise
int host_sphere(const dexr_sphere_model* sm, int mode, int64_t B, const double* x, const double* fixed, const double* gdist, double margin,
                const double* pw, double* dist_out, double* cen_out, double* e_out, double* gx_out) {
  const dexr_pose_model* m = sm->pose;
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t np = (size_t)B * sm->n_pair * sizeof(double), nc = (size_t)B * sm->n_sphere * 3 * sizeof(double);
  DevBuf dx, dfix, dg, dw, dd, dc, de, dgx;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (gdist) POSE_HIP(dg.put(gdist, np));
  if (pw) POSE_HIP(dw.put(pw, (size_t)sm->n_pair * sizeof(double)));
  if (dist_out) POSE_HIP(dd.put(nullptr, np));
  if (cen_out) POSE_HIP(dc.put(nullptr, nc));
  if (e_out) POSE_HIP(de.put(nullptr, (size_t)B * sizeof(double)));
  if (gx_out) POSE_HIP(dgx.put(nullptr, nx));
  const int rc = launch_sphere<double>(sm, mode, B, (const double*)dx.p, (const double*)dfix.p, (const double*)dg.p, margin, (const double*)dw.p,
                                       (double*)dd.p, (double*)dc.p, (double*)de.p, (double*)dgx.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (dist_out) POSE_HIP(hipMemcpy(dist_out, dd.p, np, hipMemcpyDeviceToHost));
  if (cen_out) POSE_HIP(hipMemcpy(cen_out, dc.p, nc, hipMemcpyDeviceToHost));
  if (e_out) POSE_HIP(hipMemcpy(e_out, de.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost));
  if (gx_out && nx) POSE_HIP(hipMemcpy(gx_out, dgx.p, nx, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

inline bool finite_d(double v) { return v == v && v <= 1.7976931348623157e308 && v >= -1.7976931348623157e308; }

}  // namespace

extern "C" {

int dexr_sphere_model_create(const void* pose_blob, size_t nbytes, int32_t n_sphere, const int32_t* sphere_link, const double* center,
                             const double* radius, int32_t n_pair, const int32_t* pair, dexr_sphere_model** out) {
  if (!pose_blob || !out) return dexr_set_error(DEXR_ERR_INVALID, "null argument");
  *out = nullptr;
  PoseParsed parsed;
  int rc = parse_pose_blob(pose_blob, nbytes, parsed);
  if (rc) return rc;
  if (n_sphere < 1 || n_sphere > DEXR_SPHERE_MAX) return dexr_set_error(DEXR_ERR_INVALID, "sphere model has %d spheres (1..%d)", n_sphere, DEXR_SPHERE_MAX);
  if (n_pair < 1 || n_pair > DEXR_SPHERE_MAXPAIR) return dexr_set_error(DEXR_ERR_INVALID, "sphere model has %d pairs (1..%d)", n_pair, DEXR_SPHERE_MAXPAIR);
  if (!sphere_link || !center || !radius || !pair) return dexr_set_error(DEXR_ERR_INVALID, "null sphere or pair array");
  const int n_link = parsed.h.n_link;
  for (int s = 0; s < n_sphere; ++s) {
    if (sphere_link[s] < 0 || sphere_link[s] >= n_link) return dexr_set_error(DEXR_ERR_INVALID, "sphere %d: link row %d out of range (%d links)", s, sphere_link[s], n_link);
    for (int k = 0; k < 3; ++k)
      if (!finite_d(center[3 * s + k])) return dexr_set_error(DEXR_ERR_INVALID, "sphere %d: centre is not finite", s);
    if (!finite_d(radius[s]) || radius[s] < 0.0) return dexr_set_error(DEXR_ERR_INVALID, "sphere %d: radius must be finite and >= 0, got %g", s, radius[s]);
  }
  for (int p = 0; p < n_pair; ++p) {
    const int i = pair[2 * p], j = pair[2 * p + 1];
    if (i < 0 || i >= n_sphere || j < 0 || j >= n_sphere) return dexr_set_error(DEXR_ERR_INVALID, "pair %d: sphere index out of range (%d, %d; %d spheres)", p, i, j, n_sphere);
    if (i == j) return dexr_set_error(DEXR_ERR_INVALID, "pair %d: pairs sphere %d with itself", p, i);
  }
  // spheres sorted by the sorted position of their link (stable: the caller's order within a link)
  std::vector<int32_t> sorted_of(n_link, 0), order(n_sphere), pos_of(n_sphere), link_sph(n_link + 1, 0);
  for (int l = 0; l < n_link; ++l) sorted_of[parsed.ls[l].out] = l;
  for (int s = 0; s < n_sphere; ++s) order[s] = s;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return sorted_of[sphere_link[a]] < sorted_of[sphere_link[b]]; });
  std::vector<SphereD<double>> sph(n_sphere);
  for (int k = 0; k < n_sphere; ++k) {
    const int s = order[k];
    pos_of[s] = k;
    for (int i = 0; i < 3; ++i) sph[k].c[i] = center[3 * s + i];
    sph[k].r = radius[s];
    ++link_sph[sorted_of[sphere_link[s]] + 1];
  }
  for (int l = 0; l < n_link; ++l) link_sph[l + 1] += link_sph[l];
  // incidence lists: per sorted sphere its pairs in list order, from either end
  std::vector<int32_t> inc_ptr(n_sphere + 1, 0);
  std::vector<double> rsum(n_pair);
  for (int p = 0; p < n_pair; ++p) {
    ++inc_ptr[pos_of[pair[2 * p]] + 1];
    ++inc_ptr[pos_of[pair[2 * p + 1]] + 1];
    rsum[p] = radius[pair[2 * p]] + radius[pair[2 * p + 1]];
  }
  for (int s = 0; s < n_sphere; ++s) inc_ptr[s + 1] += inc_ptr[s];
  std::vector<uint32_t> inc((size_t)2 * n_pair);
  std::vector<int32_t> fill(inc_ptr.begin(), inc_ptr.end() - 1);
  std::vector<uint32_t> pair_sph(n_pair);
  for (int p = 0; p < n_pair; ++p) {
    const int a = pos_of[pair[2 * p]], b = pos_of[pair[2 * p + 1]];
    pair_sph[p] = (uint32_t)a | ((uint32_t)b << 7);
    inc[fill[a]++] = (uint32_t)b | SPH_FIRST | ((uint32_t)p << 8);
    inc[fill[b]++] = (uint32_t)a | ((uint32_t)p << 8);
  }

  dexr_sphere_model* m = new (std::nothrow) dexr_sphere_model();
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "out of host memory");
  m->n_sphere = n_sphere;
  m->n_pair = n_pair;
  rc = upload_pose_model(parsed, &m->pose);
  if (rc) {
    dexr_sphere_model_destroy(m);
    return rc;
  }
  hipError_t e = upload_sphere_tables<float>(sph, rsum, m->f32);
  if (e == hipSuccess) e = upload_sphere_tables<double>(sph, rsum, m->f64);
  if (e == hipSuccess) e = upload_vector(link_sph, &m->link_sph);
  if (e == hipSuccess) e = upload_vector(order, &m->sph_out);
  if (e == hipSuccess) e = upload_vector(inc_ptr, &m->inc_ptr);
  if (e == hipSuccess) e = upload_vector(inc, &m->inc);
  if (e == hipSuccess) e = upload_vector(pair_sph, &m->pair_sph);
  if (e == hipSuccess) e = upload_vector(pos_of, &m->sph_in);
  if (e != hipSuccess) {
    dexr_sphere_model_destroy(m);
    return dexr_set_error(DEXR_ERR_HIP, "uploading sphere tables failed: %s", hipGetErrorString(e));
  }
  *out = m;
  return DEXR_OK;
}

void dexr_sphere_model_destroy(dexr_sphere_model* m) {
  if (!m) return;
  dexr_pose_model_destroy(m->pose);
  if (m->f32.spheres) (void)hipFree(m->f32.spheres);
  if (m->f32.rsum) (void)hipFree(m->f32.rsum);
  if (m->f64.spheres) (void)hipFree(m->f64.spheres);
  if (m->f64.rsum) (void)hipFree(m->f64.rsum);
  if (m->link_sph) (void)hipFree(m->link_sph);
  if (m->sph_out) (void)hipFree(m->sph_out);
  if (m->inc_ptr) (void)hipFree(m->inc_ptr);
  if (m->inc) (void)hipFree(m->inc);
  if (m->pair_sph) (void)hipFree(m->pair_sph);
  if (m->sph_in) (void)hipFree(m->sph_in);
  delete m;
}

int dexr_sphere_model_info(const dexr_sphere_model* m, int32_t* n_in, int32_t* n_fixed, int32_t* n_sphere, int32_t* n_pair) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (n_in) *n_in = m->pose->h.n_in;
  if (n_fixed) *n_fixed = m->pose->h.n_fixed;
  if (n_sphere) *n_sphere = m->n_sphere;
  if (n_pair) *n_pair = m->n_pair;
  return DEXR_OK;
}

int dexr_sphere_distances_dev(const dexr_sphere_model* m, int64_t B, const float* x, const float* fixed, float* dist_out, float* center_out,
                              void* stream) {
  const int c = check_sphere_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_out) return dexr_set_error(DEXR_ERR_INVALID, "dist_out is NULL");
  return launch_sphere<float>(m, SPH_DIST, B, x, fixed, nullptr, 0.f, nullptr, dist_out, center_out, nullptr, nullptr, (hipStream_t)stream);
}

int dexr_sphere_distances_vjp_dev(const dexr_sphere_model* m, int64_t B, const float* x, const float* fixed, const float* grad_dist,
                                  float* grad_x_out, void* stream) {
  const int c = check_sphere_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_dist) return dexr_set_error(DEXR_ERR_INVALID, "grad_dist is NULL");
  if (!grad_x_out && m->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  return launch_sphere<float>(m, SPH_VJP, B, x, fixed, grad_dist, 0.f, nullptr, nullptr, nullptr, nullptr, grad_x_out, (hipStream_t)stream);
}

int dexr_sphere_penalty_dev(const dexr_sphere_model* m, int64_t B, const float* x, const float* fixed, float margin, const float* pair_weight,
                            float* energy_out, float* grad_x_out, void* stream) {
  if (m && check_margin((double)margin)) return DEXR_ERR_INVALID;
  const int c = check_sphere_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_x_out) return dexr_set_error(DEXR_ERR_INVALID, "energy_out and grad_x_out are both NULL");
  return launch_sphere<float>(m, SPH_PENALTY, B, x, fixed, nullptr, margin, pair_weight, nullptr, nullptr, energy_out, grad_x_out,
                              (hipStream_t)stream);
}

int dexr_sphere_distances(const dexr_sphere_model* m, int64_t B, const double* x, const double* fixed, double* dist_out, double* center_out) {
  const int c = check_sphere_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_out) return dexr_set_error(DEXR_ERR_INVALID, "dist_out is NULL");
  return host_sphere(m, SPH_DIST, B, x, fixed, nullptr, 0.0, nullptr, dist_out, center_out, nullptr, nullptr);
}

int dexr_sphere_distances_vjp(const dexr_sphere_model* m, int64_t B, const double* x, const double* fixed, const double* grad_dist,
                              double* grad_x_out) {
  const int c = check_sphere_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_dist) return dexr_set_error(DEXR_ERR_INVALID, "grad_dist is NULL");
  if (!grad_x_out && m->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  return host_sphere(m, SPH_VJP, B, x, fixed, grad_dist, 0.0, nullptr, nullptr, nullptr, nullptr, grad_x_out);
}

int dexr_sphere_penalty(const dexr_sphere_model* m, int64_t B, const double* x, const double* fixed, double margin, const double* pair_weight,
                        double* energy_out, double* grad_x_out) {
  if (m && check_margin(margin)) return DEXR_ERR_INVALID;
  const int c = check_sphere_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_x_out) return dexr_set_error(DEXR_ERR_INVALID, "energy_out and grad_x_out are both NULL");
  return host_sphere(m, SPH_PENALTY, B, x, fixed, nullptr, margin, pair_weight, nullptr, nullptr, energy_out, grad_x_out);
}

}  // extern "C"

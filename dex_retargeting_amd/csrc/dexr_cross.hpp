// dexr_cross.hpp -- the spheres of one posed robot against the spheres of another (include/dexr_cross.h): a fragment of
// dexr_pose.hip, which includes it once behind dexr_resolve_scene.hpp.  Two dexr_sphere_model handles, each with its own x and its own base pose
// per frame.  What the family has as functions is used as it is -- joint_step, link_pose, sphere_centre, resolve_force_entry,
// cross_fma, check_call, check_margin, DevBuf / POSE_HIP; the walk and the column phase are this fragment's own
// (cross_walk, cross_columns), so that no existing kernel changes.
//
// One kernel, three forms (pose_cross_kernel<T, MODE>), the block of pose_sphere_kernel: 16 threads per frame, up to 16 frames:
//   phase A (lane = frame)            the forward walk of BOTH robots, A's in the first nl lanes of the block, B's in the first nl
//                                     lanes of its second wave (a block of one wave: the nl lanes behind A's), so that the two
//                                     serial walks run side by side where the block has two waves.  A lane parks its robot's
//                                     base pose (zeros and the identity where the caller left them out: both ways run the same
//                                     arithmetic) and puts every centre into the WORLD frame as it parks it, C = pos + rot c; the
//                                     gradient forms also park the root-frame centre and a_k, o_k of every joint driven by x;
//   phase B (16 threads per frame)    every pair from both of its ends (cross_pass): thread t owns the spheres t, t + 16, ... of
//                                     A and runs over all of B in table order, then owns the spheres t, t + 16, ... of B and
//                                     runs over all of A.  C^A_s - C^B_t is the exact negative of C^B_t - C^A_s, so both ends
//                                     see the same s_st, d_st, h_st and every force is summed in registers.  The index of the
//                                     other robot's sphere is the loop counter alone: its radius and its caller's index come
//                                     through the scalar path, its centre from LDS as a broadcast.  The distance form keeps the
//                                     smallest d and the first caller's index that attains it; the VJP form does that in a first
//                                     pass, parks the nearest (table) indices of both sides and, behind a barrier, forms the
//                                     forces in a second pass that knows which t chose s; the penalty form sums the force and
//                                     (from A's side only) the energy.  The force goes to the frame's region pulled back into
//                                     the robot's root frame, rot^T F: F . rot Jpt = (rot^T F) . Jpt whatever rot holds, so phase C
//                                     is the sphere kernel's on root-frame centres, axes and origins.  The energy and the two
//                                     wrenches (world frame) go to per-thread partial sums, parked;
//   phase C (gradient forms)          a thread per active column of A, then of B, through resolve_force_entry, the columns no
//                                     joint reads zeroed; thread 0 adds the sixteen partial energies in order, threads 10 .. 15
//                                     each one component of wrench_a, threads 4 .. 9 each one of wrench_b.
//
// A frame's region of LDS is [frame][stride] with an odd stride, behind the fork slots of A and of B ([value][lane] each):
//   world centres of A, of B (3 per sphere) | pose of A, of B (12 each) | forces of A, of B | root-frame centres of A, of B |
//   16 partial energies | 16 x 6 partial wrench sums of A, of B | a, o per joint driven by x of A, of B | nearest of A, of B
//   (VJP, one value each)
// (the distance form ends behind the poses).  Every barrier is reached by every thread; every sum has a fixed order that does
// not depend on the frames per block.
#include "dexr_cross.h"

namespace {

constexpr int CRS_DIST = 0, CRS_VJP = 1, CRS_PENALTY = 2;
constexpr int CRS_POSE = 12;  // values of a parked base pose: pos (3), rot (9, row-major)

static_assert(DEXR_CROSS_FRAMES == SPH_FRAMES, "dexr_cross.h states the frames of a block");

// offsets into a frame's region (the centres of A are at 0) and its stride; made on the host (cross_layout)
struct CrossLayout {
  int cen_b, pose_a, pose_b, frc_a, frc_b, root_a, root_b, ebase, wr_a, wr_b, ao_a, ao_b, near_a, near_b, stride;
};

template <typename T>
struct CrossArgs {
  const T *pos_a, *rot_a, *pos_b, *rot_b;  // (B, 3), (B, 3, 3) or NULL
  const T *gdist_a, *gdist_b;              // (B, S_a), (B, S_b) or NULL: the VJP form
  const T* pw;                             // (S_a, S_b) or NULL
  T margin;
  T* dist_a;  // (B, S_a) or NULL ...
  int32_t* near_a;
  T* dist_b;
  int32_t* near_b;
  T* e_out;          // (B) or NULL
  T *gx_a, *gx_b;    // (B, n_in) or NULL
  T *wr_a, *wr_b;    // (B, 6) or NULL
};

// w = p + R v
template <typename T>
__device__ __forceinline__ void cross_place(const T* po, const T v[3], T* w) {
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = fma(po[3 + 3 * i + 2], v[2], fma(po[3 + 3 * i + 1], v[1], fma(po[3 + 3 * i], v[0], po[i])));
}

// phase A of one lane (lane = frame) for one robot: its base pose into park_pose, its world centres into cen and, with GRAD, its
// root-frame centres into root and a_k, o_k of every joint driven by x into ao
template <typename T, bool GRAD>
__device__ __forceinline__ void cross_walk(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links, const PoseArgs<T>& P,
                                           const SphereD<T>* __restrict__ spheres, const SphereIndex& S, const T* __restrict__ x,
                                           const T* __restrict__ fixed, const T* __restrict__ pos, const T* __restrict__ rot, T* slots, int nl,
                                           int lane, int64_t first, T* cen, T* park_pose, T* root, T* ao) {
  const int64_t b = first + lane < P.B ? first + lane : P.B - 1;  // ragged tail: idle lanes park the last frame again
  T po[CRS_POSE];
#pragma unroll
  for (int i = 0; i < 3; ++i) po[i] = pos ? pos[b * 3 + i] : T(0);
#pragma unroll
  for (int i = 0; i < 9; ++i) po[3 + i] = rot ? rot[b * 9 + i] : ((i % 4 == 0) ? T(1) : T(0));
#pragma unroll
  for (int i = 0; i < CRS_POSE; ++i) park_pose[i] = po[i];
  for (int l = 0; l < P.n_base; ++l) {  // spheres on the fixed base: constant in the root frame
    const LinkD<T>& L = links[l];
    for (int s = S.link_sph[l]; s < S.link_sph[l + 1]; ++s) {
      T c[3];
      sphere_centre(L.R, L.p, spheres[s], c);
      cross_place(po, c, cen + 3 * s);
      if (GRAD) root[3 * s] = c[0], root[3 * s + 1] = c[1], root[3 * s + 2] = c[2];
    }
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
      T* d = ao + 6 * xi;
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
      for (int s = s0; s < s1; ++s) {
        T c[3];
        sphere_centre(R, p, spheres[s], c);
        cross_place(po, c, cen + 3 * s);
        if (GRAD) root[3 * s] = c[0], root[3 * s + 1] = c[1], root[3 * s + 2] = c[2];
      }
    }
  }
}

// D = c - cu and d = |D| - (r + ru); sd receives |D|.  From the other end D is the exact negative and sd, d the same bits
template <typename T>
__device__ __forceinline__ T cross_gap(const T c[3], T r, const T* cu, T ru, T D[3], T& sd) {
#pragma unroll
  for (int i = 0; i < 3; ++i) D[i] = c[i] - cu[i];
  sd = sqrt(fma(D[2], D[2], fma(D[1], D[1], D[0] * D[0])));
  return sd - (r + ru);
}

// 1 / |D|, or 0 where the centres coincide (no direction; a NaN of sd stays one)
template <typename T>
__device__ __forceinline__ T cross_inv(T sd) {
  return sd > T(0) ? T(1) / sd : sd * T(0);
}

// the other robot's sphere nearest to the sphere (c, r): its table index, with its caller's index in near_out and d in best.
// Among equal distances the smallest caller's index wins (a NaN of the first d stays)
template <typename T>
__device__ __forceinline__ int cross_nearest(const T c[3], T r, const T* oth, int n_oth, const SphereD<T>* __restrict__ sph_oth,
                                             const int32_t* __restrict__ out_oth, T& best, int& near_out) {
  int near = 0;
  best = T(0);
  near_out = 0;
  for (int u = 0; u < n_oth; ++u) {
    T D[3], sd;
    const T d = cross_gap(c, r, oth + 3 * u, sph_oth[u].r, D, sd);
    const int o = out_oth[u];
    if (u == 0 || d < best || (d == best && o < near_out)) {
      best = d;
      near = u;
      near_out = o;
    }
  }
  return near;
}

// phase B from one end: thread t owns the spheres t, t + 16, ... of `own` and runs over all n_oth spheres of the other robot.
//   CRS_DIST      dist / nearest rows of the frame (caller's indices)
//   CRS_VJP       FIRST: the nearest table index of every own sphere into near_own; else the forces, with both sides' indices
//   CRS_PENALTY   the forces, and with ENERGY the thread's partial energy
// The gradient forms add the force of every own sphere to the thread's partial wrench about the base (po: pos, rot) and park it,
// pulled back into the root frame (rot^T F), in frc.
template <typename T, int MODE, bool FIRST, bool ENERGY>
__device__ __forceinline__ void cross_pass(const T* cen, const T* oth, int n_own, int n_oth, const SphereD<T>* __restrict__ sph_own,
                                           const SphereD<T>* __restrict__ sph_oth, const int32_t* __restrict__ out_own,
                                           const int32_t* __restrict__ out_oth, const T* po, const T* __restrict__ pw, int w_own, int w_oth,
                                           T margin, const T* __restrict__ g_own, const T* __restrict__ g_oth, int32_t* near_own,
                                           const int32_t* near_oth, T* frc, T* __restrict__ dist_row, int32_t* __restrict__ near_row, bool live,
                                           int t, T& e, T wr[6]) {
  for (int s = t; s < n_own; s += SPH_FANOUT) {
    const T c[3] = {cen[3 * s], cen[3 * s + 1], cen[3 * s + 2]};
    const T r = sph_own[s].r;
    const int so = out_own[s];
    if (MODE == CRS_DIST || (MODE == CRS_VJP && FIRST)) {
      T best;
      int near_out;
      const int near = cross_nearest(c, r, oth, n_oth, sph_oth, out_oth, best, near_out);
      if (MODE == CRS_VJP) {
        near_own[s] = near;
      } else if (live) {
        if (dist_row) dist_row[so] = best;
        if (near_row) near_row[so] = near_out;
      }
      continue;
    }
    T f[3] = {T(0), T(0), T(0)};
    if (MODE == CRS_VJP) {
      T D[3], sd;
      const int u0 = near_own[s];
      cross_gap(c, r, oth + 3 * u0, sph_oth[u0].r, D, sd);
      const T k = (g_own ? g_own[so] : T(0)) * cross_inv(sd);
#pragma unroll
      for (int i = 0; i < 3; ++i) f[i] = k * D[i];
      for (int u = 0; u < n_oth; ++u) {
        if (near_oth[u] != s) continue;
        cross_gap(c, r, oth + 3 * u, sph_oth[u].r, D, sd);
        const T ku = (g_oth ? g_oth[out_oth[u]] : T(0)) * cross_inv(sd);
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i] = fma(ku, D[i], f[i]);
      }
    } else {
      const T* wrow = pw ? pw + (size_t)so * w_own : nullptr;
      for (int u = 0; u < n_oth; ++u) {
        T D[3], sd;
        const T d = cross_gap(c, r, oth + 3 * u, sph_oth[u].r, D, sd);
        const T h = margin - d;
        if (h <= T(0)) continue;  // (a comparison: a NaN goes on and stays a NaN)
        const T wh = wrow ? wrow[(size_t)out_oth[u] * w_oth] * h : h;
        if (ENERGY) e = fma(wh, h, e);
        const T k = T(-2) * wh * cross_inv(sd);
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i] = fma(k, D[i], f[i]);
      }
    }
    const T arm[3] = {c[0] - po[0], c[1] - po[1], c[2] - po[2]};  // C_s - pos
    T tq[3];
    cross_fma(arm, f, tq);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      wr[i] += f[i];
      wr[3 + i] += tq[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) frc[3 * s + i] = fma(po[3 + 6 + i], f[2], fma(po[3 + 3 + i], f[1], po[3 + i] * f[0]));  // rot^T F
  }
}

// phase C for one robot (behind the barrier that ends phase B): a thread per active column through resolve_force_entry, then the
// columns no joint reads; threads w0 .. w0 + 5 each add the sixteen partial sums of one component of the wrench in order
template <typename T>
__device__ __forceinline__ void cross_columns(const PoseArgs<T>& P, const SphereIndex& S, const JacEnt* __restrict__ ents,
                                              const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col,
                                              const int32_t* __restrict__ col_act, int n_act, const T* ao, const T* cen, const T* frc,
                                              const T* wpart, int w0, int t, bool live, int64_t b, T* __restrict__ gx, T* __restrict__ wrench) {
  if (gx) {
    for (int i = t; i < n_act; i += SPH_FANOUT) {
      const T g = resolve_force_entry(act_rng[i], ents, S.link_sph, ao, cen, frc);
      if (live) gx[b * P.n_in + act_col[i]] = g;
    }
    if (live) {
      T* o = gx + b * P.n_in;
      for (int c = t; c < P.n_in; c += SPH_FANOUT)
        if (col_act[c] < 0) o[c] = T(0);
    }
  }
  if (wrench && live && t >= w0 && t < w0 + 6) {
    const T* w = wpart + (t - w0) * SPH_FANOUT;
    T W = w[0];
    for (int i = 1; i < SPH_FANOUT; ++i) W += w[i];
    wrench[b * 6 + (t - w0)] = W;
  }
}

template <typename T, int MODE>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES)
    pose_cross_kernel(const JointD<T>* __restrict__ joints_a, const LinkD<T>* __restrict__ links_a, PoseArgs<T> Pa,
                      const SphereD<T>* __restrict__ spheres_a, SphereIndex Sa, const JacEnt* __restrict__ ents_a,
                      const uint32_t* __restrict__ act_rng_a, const int32_t* __restrict__ act_col_a, const int32_t* __restrict__ col_act_a,
                      int n_act_a, const T* __restrict__ x_a, const T* __restrict__ fixed_a, const JointD<T>* __restrict__ joints_b,
                      const LinkD<T>* __restrict__ links_b, PoseArgs<T> Pb, const SphereD<T>* __restrict__ spheres_b, SphereIndex Sb,
                      const JacEnt* __restrict__ ents_b, const uint32_t* __restrict__ act_rng_b, const int32_t* __restrict__ act_col_b,
                      const int32_t* __restrict__ col_act_b, int n_act_b, const T* __restrict__ x_b, const T* __restrict__ fixed_b,
                      CrossLayout Y, CrossArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  T* slots_a = reinterpret_cast<T*>(pose_lds);
  T* slots_b = slots_a + (size_t)Pa.n_slot * 12 * nl;
  T* park = slots_b + (size_t)Pb.n_slot * 12 * nl;
  const int64_t first = (int64_t)blockIdx.x * nl;
  const int lane_b = tid - (blockDim.x > 64 ? 64 : nl);  // B's walk: the second wave where the block has one
  if (tid < nl) {
    T* pk = park + (size_t)tid * Y.stride;
    cross_walk<T, MODE != CRS_DIST>(joints_a, links_a, Pa, spheres_a, Sa, x_a, fixed_a, A.pos_a, A.rot_a, slots_a, nl, tid, first, pk,
                                    pk + Y.pose_a, pk + Y.root_a, pk + Y.ao_a);
  } else if (lane_b >= 0 && lane_b < nl) {
    T* pk = park + (size_t)lane_b * Y.stride;
    cross_walk<T, MODE != CRS_DIST>(joints_b, links_b, Pb, spheres_b, Sb, x_b, fixed_b, A.pos_b, A.rot_b, slots_b, nl, lane_b, first,
                                    pk + Y.cen_b, pk + Y.pose_b, pk + Y.root_b, pk + Y.ao_b);
  }
  __syncthreads();
  // phase B: SPH_FANOUT threads per frame, every pair from both ends
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  T* pk = park + (size_t)fr * Y.stride;
  const T *cen_a = pk, *cen_b = pk + Y.cen_b;
  const bool live = first + fr < Pa.B;
  const int64_t b = live ? first + fr : Pa.B - 1;
  const int na = Sa.n_sphere, nb = Sb.n_sphere;
  int32_t* near_a = reinterpret_cast<int32_t*>(pk + Y.near_a);
  int32_t* near_b = reinterpret_cast<int32_t*>(pk + Y.near_b);
  T e = T(0), wa[6] = {T(0), T(0), T(0), T(0), T(0), T(0)}, wb[6] = {T(0), T(0), T(0), T(0), T(0), T(0)};
  if (MODE == CRS_DIST) {
    if (A.dist_a || A.near_a)
      cross_pass<T, CRS_DIST, true, false>(cen_a, cen_b, na, nb, spheres_a, spheres_b, Sa.sph_out, Sb.sph_out, nullptr, nullptr, 0, 0, T(0),
                                           nullptr, nullptr, nullptr, nullptr, nullptr, A.dist_a ? A.dist_a + b * na : nullptr,
                                           A.near_a ? A.near_a + b * na : nullptr, live, t, e, wa);
    if (A.dist_b || A.near_b)
      cross_pass<T, CRS_DIST, true, false>(cen_b, cen_a, nb, na, spheres_b, spheres_a, Sb.sph_out, Sa.sph_out, nullptr, nullptr, 0, 0, T(0),
                                           nullptr, nullptr, nullptr, nullptr, nullptr, A.dist_b ? A.dist_b + b * nb : nullptr,
                                           A.near_b ? A.near_b + b * nb : nullptr, live, t, e, wb);
    return;  // (no barrier follows in this form)
  }
  const T* ga = A.gdist_a ? A.gdist_a + b * na : nullptr;
  const T* gb = A.gdist_b ? A.gdist_b + b * nb : nullptr;
  if (MODE == CRS_VJP) {
    cross_pass<T, CRS_VJP, true, false>(cen_a, cen_b, na, nb, spheres_a, spheres_b, Sa.sph_out, Sb.sph_out, nullptr, nullptr, 0, 0, T(0), nullptr,
                                        nullptr, near_a, nullptr, nullptr, nullptr, nullptr, live, t, e, wa);
    cross_pass<T, CRS_VJP, true, false>(cen_b, cen_a, nb, na, spheres_b, spheres_a, Sb.sph_out, Sa.sph_out, nullptr, nullptr, 0, 0, T(0), nullptr,
                                        nullptr, near_b, nullptr, nullptr, nullptr, nullptr, live, t, e, wb);
    __syncthreads();
  }
  // (the weight of the pair (s, t) is pw[s * S_b + t] from either end)
  cross_pass<T, MODE, false, true>(cen_a, cen_b, na, nb, spheres_a, spheres_b, Sa.sph_out, Sb.sph_out, pk + Y.pose_a, A.pw, nb, 1, A.margin, ga,
                                   gb, near_a, near_b, pk + Y.frc_a, nullptr, nullptr, live, t, e, wa);
  cross_pass<T, MODE, false, false>(cen_b, cen_a, nb, na, spheres_b, spheres_a, Sb.sph_out, Sa.sph_out, pk + Y.pose_b, A.pw, 1, nb, A.margin, gb,
                                    ga, near_b, near_a, pk + Y.frc_b, nullptr, nullptr, live, t, e, wb);
  pk[Y.ebase + t] = e;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    pk[Y.wr_a + i * SPH_FANOUT + t] = wa[i];
    pk[Y.wr_b + i * SPH_FANOUT + t] = wb[i];
  }
  __syncthreads();
  // phase C: the columns of A, the columns of B, the energy and the two wrenches
  cross_columns(Pa, Sa, ents_a, act_rng_a, act_col_a, col_act_a, n_act_a, pk + Y.ao_a, pk + Y.root_a, pk + Y.frc_a, pk + Y.wr_a, SPH_FANOUT - 6, t, live,
                b, A.gx_a, A.wr_a);
  cross_columns(Pb, Sb, ents_b, act_rng_b, act_col_b, col_act_b, n_act_b, pk + Y.ao_b, pk + Y.root_b, pk + Y.frc_b, pk + Y.wr_b, SPH_FANOUT - 12, t, live,
                b, A.gx_b, A.wr_b);
  if (MODE == CRS_PENALTY && live && A.e_out && t == 0) {
    T E = pk[Y.ebase];
    for (int i = 1; i < SPH_FANOUT; ++i) E += pk[Y.ebase + i];
    A.e_out[b] = E;
  }
}

// the region of a frame (the list at the head of this file); an odd stride, so that the frames of a wave start in different banks
CrossLayout cross_layout(const dexr_sphere_model* a, const dexr_sphere_model* b, int mode) {
  CrossLayout Y;
  const int sa = a->n_sphere, sb = b->n_sphere;
  Y.cen_b = 3 * sa;
  Y.pose_a = Y.cen_b + 3 * sb;
  Y.pose_b = Y.pose_a + CRS_POSE;
  Y.frc_a = Y.pose_b + CRS_POSE;
  Y.frc_b = Y.frc_a + 3 * sa;
  Y.root_a = Y.frc_b + 3 * sb;
  Y.root_b = Y.root_a + 3 * sa;
  Y.ebase = Y.root_b + 3 * sb;
  Y.wr_a = Y.ebase + SPH_FANOUT;
  Y.wr_b = Y.wr_a + 6 * SPH_FANOUT;
  Y.ao_a = Y.wr_b + 6 * SPH_FANOUT;
  Y.ao_b = Y.ao_a + 6 * a->pose->n_jx;
  Y.near_a = Y.ao_b + 6 * b->pose->n_jx;
  Y.near_b = Y.near_a + sa;
  const int end = mode == CRS_DIST ? Y.frc_a : (mode == CRS_PENALTY ? Y.near_a : Y.near_b + sb);
  Y.stride = end | 1;
  return Y;
}

// checks shared by the six entry points: < 0 error, 1 nothing to do, 0 go on
int check_cross_call(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const void* x_a, const void* fixed_a, const void* x_b,
                     const void* fixed_b) {
  if (!a || !b) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  const int c = check_call(a->pose, B, x_a, fixed_a);
  if (c) return c;
  return check_call(b->pose, B, x_b, fixed_b);
}

template <typename T>
int launch_cross(const dexr_sphere_model* a, const dexr_sphere_model* b, int mode, int64_t B, const T* x_a, const T* fixed_a, const T* x_b,
                 const T* fixed_b, const CrossArgs<T>& A, hipStream_t st) {
  const dexr_pose_model *ma = a->pose, *mb = b->pose;
  const CrossLayout Y = cross_layout(a, b, mode);
  const size_t per_frame = ((size_t)(ma->h.n_slot + mb->h.n_slot) * 12 + (size_t)Y.stride) * sizeof(T);
  int nl = SPH_FRAMES;
  while (nl > 1 && per_frame * nl > DEXR_CROSS_LDS) nl /= 2;  // (float64, 128 spheres against 128, 64 joints each: 2 frames)
  if (per_frame * nl > DEXR_CROSS_LDS)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the two sphere models need %zu B of LDS per frame: one frame does not fit a block", per_frame);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  const SphereIndex Sa = {a->link_sph, a->sph_out, a->inc_ptr, a->inc, a->n_sphere, a->n_pair};
  const SphereIndex Sb = {b->link_sph, b->sph_out, b->inc_ptr, b->inc, b->n_sphere, b->n_pair};
  const dim3 grid((unsigned)blocks), block(nl * SPH_FANOUT);
  const size_t lds = per_frame * nl;
#define CRS_LAUNCH(MODE)                                                                                                                     \
  hipLaunchKernelGGL((pose_cross_kernel<T, MODE>), grid, block, lds, st, (const JointD<T>*)tables_of<T>(ma).joints,                           \
                     (const LinkD<T>*)tables_of<T>(ma).links, args_of<T>(ma, B), (const SphereD<T>*)sphere_tables_of<T>(a).spheres, Sa,       \
                     (const JacEnt*)ma->jac_ents, (const uint32_t*)ma->ik_act_rng, (const int32_t*)ma->ik_act_col,                            \
                     (const int32_t*)ma->ik_col_act, ma->n_act, x_a, fixed_a, (const JointD<T>*)tables_of<T>(mb).joints,                     \
                     (const LinkD<T>*)tables_of<T>(mb).links, args_of<T>(mb, B), (const SphereD<T>*)sphere_tables_of<T>(b).spheres, Sb,       \
                     (const JacEnt*)mb->jac_ents, (const uint32_t*)mb->ik_act_rng, (const int32_t*)mb->ik_act_col,                            \
                     (const int32_t*)mb->ik_col_act, mb->n_act, x_b, fixed_b, Y, A)
  if (mode == CRS_DIST) CRS_LAUNCH(CRS_DIST);
  else if (mode == CRS_VJP) CRS_LAUNCH(CRS_VJP);
  else CRS_LAUNCH(CRS_PENALTY);
#undef CRS_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "cross collision kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

struct CrossHost {
  const double *x_a, *fixed_a, *x_b, *fixed_b, *pos_a, *rot_a, *pos_b, *rot_b, *gdist_a, *gdist_b, *pw;
  double margin;
  double* dist_a;
  int32_t* near_a;
  double* dist_b;
  int32_t* near_b;
  double *e, *gx_a, *gx_b, *wr_a, *wr_b;
};

// the float64 host twin of all three forms: copy, run, synchronise
int host_cross(const dexr_sphere_model* a, const dexr_sphere_model* b, int mode, int64_t B, const CrossHost& H) {
  const dexr_pose_model *ma = a->pose, *mb = b->pose;
  const size_t d8 = sizeof(double), nb = (size_t)B * d8;
  const size_t nxa = (size_t)B * ma->h.n_in * d8, nfa = (size_t)B * ma->h.n_fixed * d8, nxb = (size_t)B * mb->h.n_in * d8;
  const size_t nfb = (size_t)B * mb->h.n_fixed * d8, nsa = (size_t)B * a->n_sphere, nsb = (size_t)B * b->n_sphere;
  DevBuf dxa, dfa, dxb, dfb, dpa, dra, dpb, drb, dga, dgb, dw, dda, dna, ddb, dnb, de, dgxa, dgxb, dwa, dwb;
  POSE_HIP(dxa.put(H.x_a, nxa));
  POSE_HIP(dfa.put(H.fixed_a, nfa));
  POSE_HIP(dxb.put(H.x_b, nxb));
  POSE_HIP(dfb.put(H.fixed_b, nfb));
  if (H.pos_a) POSE_HIP(dpa.put(H.pos_a, 3 * nb));
  if (H.rot_a) POSE_HIP(dra.put(H.rot_a, 9 * nb));
  if (H.pos_b) POSE_HIP(dpb.put(H.pos_b, 3 * nb));
  if (H.rot_b) POSE_HIP(drb.put(H.rot_b, 9 * nb));
  if (H.gdist_a) POSE_HIP(dga.put(H.gdist_a, nsa * d8));
  if (H.gdist_b) POSE_HIP(dgb.put(H.gdist_b, nsb * d8));
  if (H.pw) POSE_HIP(dw.put(H.pw, (size_t)a->n_sphere * b->n_sphere * d8));
  if (H.dist_a) POSE_HIP(dda.put(nullptr, nsa * d8));
  if (H.near_a) POSE_HIP(dna.put(nullptr, nsa * sizeof(int32_t)));
  if (H.dist_b) POSE_HIP(ddb.put(nullptr, nsb * d8));
  if (H.near_b) POSE_HIP(dnb.put(nullptr, nsb * sizeof(int32_t)));
  if (H.e) POSE_HIP(de.put(nullptr, nb));
  if (H.gx_a) POSE_HIP(dgxa.put(nullptr, nxa));
  if (H.gx_b) POSE_HIP(dgxb.put(nullptr, nxb));
  if (H.wr_a) POSE_HIP(dwa.put(nullptr, 6 * nb));
  if (H.wr_b) POSE_HIP(dwb.put(nullptr, 6 * nb));
  CrossArgs<double> A;
  A.pos_a = (const double*)dpa.p, A.rot_a = (const double*)dra.p, A.pos_b = (const double*)dpb.p, A.rot_b = (const double*)drb.p;
  A.gdist_a = (const double*)dga.p, A.gdist_b = (const double*)dgb.p, A.pw = (const double*)dw.p, A.margin = H.margin;
  A.dist_a = (double*)dda.p, A.near_a = (int32_t*)dna.p, A.dist_b = (double*)ddb.p, A.near_b = (int32_t*)dnb.p;
  A.e_out = (double*)de.p, A.gx_a = (double*)dgxa.p, A.gx_b = (double*)dgxb.p, A.wr_a = (double*)dwa.p, A.wr_b = (double*)dwb.p;
  const int rc = launch_cross<double>(a, b, mode, B, (const double*)dxa.p, (const double*)dfa.p, (const double*)dxb.p, (const double*)dfb.p, A,
                                      nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (H.dist_a) POSE_HIP(hipMemcpy(H.dist_a, dda.p, nsa * d8, hipMemcpyDeviceToHost));
  if (H.near_a) POSE_HIP(hipMemcpy(H.near_a, dna.p, nsa * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (H.dist_b) POSE_HIP(hipMemcpy(H.dist_b, ddb.p, nsb * d8, hipMemcpyDeviceToHost));
  if (H.near_b) POSE_HIP(hipMemcpy(H.near_b, dnb.p, nsb * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (H.e) POSE_HIP(hipMemcpy(H.e, de.p, nb, hipMemcpyDeviceToHost));
  if (H.gx_a && nxa) POSE_HIP(hipMemcpy(H.gx_a, dgxa.p, nxa, hipMemcpyDeviceToHost));
  if (H.gx_b && nxb) POSE_HIP(hipMemcpy(H.gx_b, dgxb.p, nxb, hipMemcpyDeviceToHost));
  if (H.wr_a) POSE_HIP(hipMemcpy(H.wr_a, dwa.p, 6 * nb, hipMemcpyDeviceToHost));
  if (H.wr_b) POSE_HIP(hipMemcpy(H.wr_b, dwb.p, 6 * nb, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

template <typename T>
CrossArgs<T> cross_args(const T* pos_a, const T* rot_a, const T* pos_b, const T* rot_b) {
  CrossArgs<T> A;
  memset(&A, 0, sizeof(A));
  A.pos_a = pos_a, A.rot_a = rot_a, A.pos_b = pos_b, A.rot_b = rot_b;
  return A;
}

int check_cross_vjp_outputs(const dexr_sphere_model* a, const dexr_sphere_model* b, const void* gx_a, const void* gx_b) {
  if (!gx_a && a->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_xa_out is NULL");
  if (!gx_b && b->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_xb_out is NULL");
  return 0;
}

}  // namespace

extern "C" {

int dexr_cross_distances_dev(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const float* x_a, const float* fixed_a,
                             const float* x_b, const float* fixed_b, const float* pos_a, const float* rot_a, const float* pos_b,
                             const float* rot_b, float* dist_a_out, int32_t* nearest_a_out, float* dist_b_out, int32_t* nearest_b_out,
                             void* stream) {
  const int c = check_cross_call(a, b, B, x_a, fixed_a, x_b, fixed_b);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_a_out && !nearest_a_out && !dist_b_out && !nearest_b_out) return dexr_set_error(DEXR_ERR_INVALID, "every output is NULL");
  CrossArgs<float> A = cross_args<float>(pos_a, rot_a, pos_b, rot_b);
  A.dist_a = dist_a_out, A.near_a = nearest_a_out, A.dist_b = dist_b_out, A.near_b = nearest_b_out;
  return launch_cross<float>(a, b, CRS_DIST, B, x_a, fixed_a, x_b, fixed_b, A, (hipStream_t)stream);
}

int dexr_cross_distances_vjp_dev(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const float* x_a, const float* fixed_a,
                                 const float* x_b, const float* fixed_b, const float* pos_a, const float* rot_a, const float* pos_b,
                                 const float* rot_b, const float* grad_dist_a, const float* grad_dist_b, float* grad_xa_out,
                                 float* grad_xb_out, float* wrench_a_out, float* wrench_b_out, void* stream) {
  const int c = check_cross_call(a, b, B, x_a, fixed_a, x_b, fixed_b);
  if (c) return c < 0 ? c : DEXR_OK;
  if (check_cross_vjp_outputs(a, b, grad_xa_out, grad_xb_out)) return DEXR_ERR_INVALID;
  CrossArgs<float> A = cross_args<float>(pos_a, rot_a, pos_b, rot_b);
  A.gdist_a = grad_dist_a, A.gdist_b = grad_dist_b;
  A.gx_a = grad_xa_out, A.gx_b = grad_xb_out, A.wr_a = wrench_a_out, A.wr_b = wrench_b_out;
  return launch_cross<float>(a, b, CRS_VJP, B, x_a, fixed_a, x_b, fixed_b, A, (hipStream_t)stream);
}

int dexr_cross_penalty_dev(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const float* x_a, const float* fixed_a,
                           const float* x_b, const float* fixed_b, const float* pos_a, const float* rot_a, const float* pos_b,
                           const float* rot_b, float margin, const float* pair_weight, float* energy_out, float* grad_xa_out,
                           float* grad_xb_out, float* wrench_a_out, float* wrench_b_out, void* stream) {
  if (a && b && check_margin((double)margin)) return DEXR_ERR_INVALID;
  const int c = check_cross_call(a, b, B, x_a, fixed_a, x_b, fixed_b);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_xa_out && !grad_xb_out && !wrench_a_out && !wrench_b_out) return dexr_set_error(DEXR_ERR_INVALID, "every output is NULL");
  CrossArgs<float> A = cross_args<float>(pos_a, rot_a, pos_b, rot_b);
  A.margin = margin, A.pw = pair_weight;
  A.e_out = energy_out, A.gx_a = grad_xa_out, A.gx_b = grad_xb_out, A.wr_a = wrench_a_out, A.wr_b = wrench_b_out;
  return launch_cross<float>(a, b, CRS_PENALTY, B, x_a, fixed_a, x_b, fixed_b, A, (hipStream_t)stream);
}

int dexr_cross_distances(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const double* x_a, const double* fixed_a,
                         const double* x_b, const double* fixed_b, const double* pos_a, const double* rot_a, const double* pos_b,
                         const double* rot_b, double* dist_a_out, int32_t* nearest_a_out, double* dist_b_out, int32_t* nearest_b_out) {
  const int c = check_cross_call(a, b, B, x_a, fixed_a, x_b, fixed_b);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!dist_a_out && !nearest_a_out && !dist_b_out && !nearest_b_out) return dexr_set_error(DEXR_ERR_INVALID, "every output is NULL");
  const CrossHost H = {x_a,     fixed_a, x_b,     fixed_b,    pos_a,         rot_a,      pos_b,         rot_b,   nullptr, nullptr, nullptr,
                       0.0,     dist_a_out, nearest_a_out, dist_b_out, nearest_b_out, nullptr, nullptr, nullptr, nullptr, nullptr};
  return host_cross(a, b, CRS_DIST, B, H);
}

int dexr_cross_distances_vjp(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const double* x_a, const double* fixed_a,
                             const double* x_b, const double* fixed_b, const double* pos_a, const double* rot_a, const double* pos_b,
                             const double* rot_b, const double* grad_dist_a, const double* grad_dist_b, double* grad_xa_out,
                             double* grad_xb_out, double* wrench_a_out, double* wrench_b_out) {
  const int c = check_cross_call(a, b, B, x_a, fixed_a, x_b, fixed_b);
  if (c) return c < 0 ? c : DEXR_OK;
  if (check_cross_vjp_outputs(a, b, grad_xa_out, grad_xb_out)) return DEXR_ERR_INVALID;
  const CrossHost H = {x_a, fixed_a, x_b,     fixed_b, pos_a,   rot_a,       pos_b,       rot_b,        grad_dist_a, grad_dist_b, nullptr,
                       0.0, nullptr, nullptr, nullptr, nullptr, nullptr, grad_xa_out, grad_xb_out, wrench_a_out, wrench_b_out};
  return host_cross(a, b, CRS_VJP, B, H);
}

int dexr_cross_penalty(const dexr_sphere_model* a, const dexr_sphere_model* b, int64_t B, const double* x_a, const double* fixed_a,
                       const double* x_b, const double* fixed_b, const double* pos_a, const double* rot_a, const double* pos_b,
                       const double* rot_b, double margin, const double* pair_weight, double* energy_out, double* grad_xa_out,
                       double* grad_xb_out, double* wrench_a_out, double* wrench_b_out) {
  if (a && b && check_margin(margin)) return DEXR_ERR_INVALID;
  const int c = check_cross_call(a, b, B, x_a, fixed_a, x_b, fixed_b);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!energy_out && !grad_xa_out && !grad_xb_out && !wrench_a_out && !wrench_b_out) return dexr_set_error(DEXR_ERR_INVALID, "every output is NULL");
  const CrossHost H = {x_a,    fixed_a, x_b,     fixed_b, pos_a,   rot_a,      pos_b,       rot_b,       nullptr,      nullptr,     pair_weight,
                       margin, nullptr, nullptr, nullptr, nullptr, energy_out, grad_xa_out, grad_xb_out, wrench_a_out, wrench_b_out};
  return host_cross(a, b, CRS_PENALTY, B, H);
}

}  // extern "C"

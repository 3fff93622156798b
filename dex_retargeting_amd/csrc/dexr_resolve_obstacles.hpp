// dexr_resolve_obstacles.hpp -- the collision-aware posture solve against obstacles (include/dexr_resolve_obstacles.h): a fragment
// of dexr_pose.hip, which includes it once after dexr_obstacles.hpp.  It owns two things:
//   resolve_contact_loop<T, Src>  the resident loop of the two contact kernels, made of the phases of dexr_resolve.hpp (whose
//                                 layout, arguments and resolve_* helpers it uses) and of a contact source Src for what an obstacle
//                                 term adds; pose_resolve_grid_kernel (dexr_resolve_grid.hpp) is its other instantiation;
//   ObstacleContacts<T>           the contact source of a primitive table (obstacle_sdf of dexr_obstacles.hpp), with
//                                 pose_resolve_obstacle_kernel<T>, its launcher and its two entry points.
//
// What a pass of resolve_contact_loop does beyond pose_resolve_kernel:
//   A  pass 0 also parks the frame's obstacle pose (p_o, R_o; zeros and the identity where the caller left them out);
//   B  after the pair forces of a sphere the thread moves the centre into the obstacle frame once, y = R_o^T (c - p_o), and asks
//      the source for the sphere's obstacle term: the force sum w h grad sdf in that frame, w h^2 onto a second set of sixteen
//      partial energies, and the sphere's active contacts in LDS at the CALLER's index of the sphere.  The sphere's force becomes
//      w_col f_pairs + w_obs R_o f_obstacle, so that g needs no new code;
//   C  thread t has the source count the contacts of its contiguous slice of caller indices; thread 0 adds the sixteen partial
//      obstacle energies in order and decides on E = ((E_pose + E_post) + E_col) + E_obs;
//   D  the source appends the thread's contacts to the frame's contact list at a prefix over the sixteen counts: caller's sphere
//      order, no atomics.  After the pair chunks the contact curvature goes through the same rank-16 staging: the source recomputes
//      a contact's normal from the parked centre and pose, the row goes through resolve_row_entry with one sphere.
// Kept system, phase E, factor / solve and the outputs are those of pose_resolve_kernel; energy_out has four columns.
// The rule's constants are the header's, read where the rule stands and nowhere as numbers of this file's own: lam times
// DEXR_RESOLVE_LAM_UP on a rejection, over DEXR_RESOLVE_LAM_DOWN on an accepted trial, DEXR_RESOLVE_MAXREJECT rejections in a row
// end a frame (resolve_decide); the first DEXR_RESOLVE_MAXACTIVE active pairs enter the curvature (resolve_pair_total,
// resolve_list_pairs).
//
// A contact source is a small struct with: head_words(n_sphere) and tail_bytes(n_sphere), the LDS it adds per frame (64-bit words
// behind the frozen masks, bytes behind the contact counts); place(L, own, n_sphere), which takes its frame's share; term, count,
// capped, append and contact, the five things above.  ObstacleContacts: a loop over the primitives in set order -- the table is
// uniform data read through the scalar load path, the index is the loop counter alone -- and ONE 64-bit mask per sphere
// (n_prim <= 64: 8 B per sphere instead of a byte per contact); counts by popcount; list entries sorted sphere | primitive << 7
// (16 bits), sphere order then set order, capped at DEXR_RESOLVE_MAXCONTACT with DEXR_RESOLVE_CONTACTS_TRUNCATED.
//
// LDS of a block: sixteen 64-bit partial frozen masks per frame | a 64-bit contact mask per sphere and frame | the fork slots | per
// frame a region [frame][stride], odd stride (ResolveLayout, then the obstacle pose and the sixteen partial obstacle energies) |
// per frame the active pairs, sixteen counts, six words of state, sixteen contact counts, the curvature contacts | per frame the
// contact list (16 bits each) | per frame one byte per pair.  include/dexr_resolve_obstacles.h states the bytes.
#include "dexr_resolve_obstacles.h"

namespace {

template <typename T>
struct ResolveObstacleArgs {
  const T* opos;  // (B, 3) or NULL
  const T* orot;  // (B, 3, 3) or NULL
  T omargin, wobs;
};

// the obstacle frame's view of a world point: R_o^T (c - p_o); po = p_o (3), R_o (9, row-major)
template <typename T>
__device__ __forceinline__ void obstacle_point(const T* po, const T* c, T y[3]) {
  const T arm[3] = {c[0] - po[0], c[1] - po[1], c[2] - po[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = fma(po[9 + i], arm[2], fma(po[6 + i], arm[1], po[3 + i] * arm[0]));
}

// R_o v
template <typename T>
__device__ __forceinline__ void obstacle_to_world(const T* po, const T v[3], T w[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = fma(po[3 + 3 * i + 2], v[2], fma(po[3 + 3 * i + 1], v[1], po[3 + 3 * i] * v[0]));
}

// bytes per frame of the counts every contact source has: sixteen contact counts and the curvature contacts
constexpr int RESOLVE_CONTACT_COUNTS = (SPH_FANOUT + 1) * (int)sizeof(int32_t);

template <typename T>
struct ObstacleContacts {
  const ObstacleD<T>* prims;
  const int32_t* kinds;
  const T* ow;  // (n_prim) or NULL
  int n_prim;
  unsigned long long* msk;  // [n_sphere] the frame's contact masks, by the caller's sphere index
  uint16_t* clst;           // [DEXR_RESOLVE_MAXCONTACT] the frame's contact list

  static __host__ __device__ int head_words(int n_sphere) { return n_sphere; }
  static __host__ __device__ int tail_bytes(int) { return DEXR_RESOLVE_MAXCONTACT * (int)sizeof(uint16_t); }

  __device__ __forceinline__ void place(const ResolveLds<T>& L, unsigned char* own, int n_sphere) {
    msk = L.head + L.fr * n_sphere;
    clst = reinterpret_cast<uint16_t*>(own) + L.fr * DEXR_RESOLVE_MAXCONTACT;
  }

  // the term of the sphere of radius rs at yo (obstacle frame), c its caller's index: sum_m w_m h grad sdf_m into fo, w_m h^2 onto eo
  __device__ __forceinline__ void term(const ResolveObstacleArgs<T>& O, const T yo[3], T rs, int c, T& eo, T fo[3]) const {
    fo[0] = fo[1] = fo[2] = T(0);
    unsigned long long bits = 0;
    for (int m = 0; m < n_prim; ++m) {
      T gm[3];
      const T d = obstacle_sdf(kinds[m], prims[m], yo, gm) - rs;
      T h = O.omargin - d;
      if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
      const T wh = ow ? ow[m] * h : h;
      eo = fma(wh, h, eo);
      if (h > T(0)) bits |= 1ull << m;
#pragma unroll
      for (int i = 0; i < 3; ++i) fo[i] = fma(wh, gm[i], fo[i]);
    }
    msk[c] = bits;
  }

  __device__ __forceinline__ int count(int c0, int c1) const {
    int n = 0;
    for (int c = c0; c < c1; ++c) n += __popcll(msk[c]);
    return n;
  }

  __device__ __forceinline__ bool capped(int& ctotal) const {
    if (ctotal <= DEXR_RESOLVE_MAXCONTACT) return false;
    ctotal = DEXR_RESOLVE_MAXCONTACT;
    return true;
  }

  // the contacts of the caller's spheres [c0, c1) from entry coff on: the caller's sphere order, then set order
  __device__ __forceinline__ void append(int c0, int c1, int coff, const int32_t* __restrict__ sph_in) const {
    for (int c = c0; c < c1 && coff < DEXR_RESOLVE_MAXCONTACT; ++c) {
      unsigned long long bits = msk[c];
      const uint32_t s = (uint32_t)sph_in[c];
      while (bits != 0 && coff < DEXR_RESOLVE_MAXCONTACT) {
        const uint32_t m = (uint32_t)__ffsll((long long)bits) - 1u;
        clst[coff++] = (uint16_t)(s | (m << 7));
        bits &= bits - 1;
      }
    }
  }

  // the q-th contact of the list: its sorted sphere, its world normal and its weight
  __device__ __forceinline__ void contact(const ResolveObstacleArgs<T>& O, const T* po, const T* cen, int q, int& si, T n[3], T& w) const {
    const uint32_t cm = clst[q];
    const int m = cm >> 7;
    si = cm & 127;
    T yo[3], gm[3];
    obstacle_point(po, cen + 3 * si, yo);
    (void)obstacle_sdf(kinds[m], prims[m], yo, gm);
    obstacle_to_world(po, gm, n);
    w = ow ? O.wobs * ow[m] : O.wobs;
  }
};

// The resident loop of a contact kernel: the skeleton of pose_resolve_kernel (dexr_resolve.hpp, where the reasons why THE LOOP
// CANNOT HANG are written down; here both chunk counts are the block's largest, read by every thread from LDS after a barrier)
// with the contact source C in it.  obase, oebase: the obstacle pose and the sixteen partial obstacle energies in a frame's region.
template <typename T, typename Src>
__device__ __forceinline__ void resolve_contact_loop(unsigned char* pose_lds, const ResolveModel<T>& M, const PoseArgs<T>& P,
                                                     const int32_t* __restrict__ sph_in, const ResolveLayout Y, int obase, int oebase, int fstride,
                                                     const ResolveArgs<T> A, const ResolveObstacleArgs<T>& O, Src C) {
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  const SphereIndex& S = M.S;
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  const ResolveLds<T> L = resolve_lds<T>(pose_lds, nl, fr, t, Y, P.n_slot, M.n_act, S.n_pair, fstride, Src::head_words(S.n_sphere),
                                         RESOLVE_CONTACT_COUNTS + Src::tail_bytes(S.n_sphere));
  int32_t* ccnt = reinterpret_cast<int32_t*>(L.tail);  // [nl][SPH_FANOUT]: contacts of a thread's slice of spheres
  int32_t* ncon = ccnt + nl * SPH_FANOUT;              // [nl]: curvature contacts
  C.place(L, reinterpret_cast<unsigned char*>(ncon + nl), S.n_sphere);
  const int64_t first = (int64_t)blockIdx.x * nl;
  const bool inb = first + fr < P.B;
  const T* po = L.pk + obase;  // the frame's obstacle pose
  const T* xr = A.xref + (inb ? first + fr : 0) * P.n_in;  // (read by working frames alone)
  const int schunk = (S.n_sphere + SPH_FANOUT - 1) / SPH_FANOUT;  // thread t owns the caller's spheres [t schunk, (t + 1) schunk)
  const int c0 = t * schunk < S.n_sphere ? t * schunk : S.n_sphere, c1 = c0 + schunk < S.n_sphere ? c0 + schunk : S.n_sphere;
  resolve_start(L, A, P.n_in, first + fr, inb);
  if (t == 0) ncon[fr] = 0;
  __syncthreads();
  for (int k = 0; k <= A.max_iters; ++k) {
    if (tid < nl && L.stopf[tid] == 0) {  // phase A; pass 0: the obstacle pose
      if (k == 0) {
        const int64_t b = first + tid;
        T* oa = L.park + tid * Y.stride + obase;
#pragma unroll
        for (int i = 0; i < 3; ++i) oa[i] = O.opos ? O.opos[b * 3 + i] : T(0);
#pragma unroll
        for (int i = 0; i < 9; ++i) oa[3 + i] = O.orot ? O.orot[b * 9 + i] : ((i % 4 == 0) ? T(1) : T(0));
      }
      resolve_walk(L, M.joints, M.links, M.spheres, S, P, Y, A, tid, first);
    }
    __syncthreads();
    const bool work = L.stopf[fr] == 0;
    if (work) {  // phase B: a thread per sphere; its pair forces, then its obstacle term: forces, energies, both kinds of active flag
      T e = T(0), eo = T(0);
      for (int s = t; s < S.n_sphere; s += SPH_FANOUT) {
        const T cs[3] = {L.cen[3 * s], L.cen[3 * s + 1], L.cen[3 * s + 2]};
        T f[3], yo[3], fo[3], fw[3];
        resolve_pair_forces(L, M, A, s, cs, e, f);
        obstacle_point(po, cs, yo);
        C.term(O, yo, M.spheres[s].r, S.sph_out[s], eo, fo);
        obstacle_to_world(po, fo, fw);
        L.frc[3 * s] = fma(O.wobs, fw[0], A.wcol * f[0]);
        L.frc[3 * s + 1] = fma(O.wobs, fw[1], A.wcol * f[1]);
        L.frc[3 * s + 2] = fma(O.wobs, fw[2], A.wcol * f[2]);
      }
      L.pk[Y.pebase + t] = e;
      L.pk[oebase + t] = eo;
    }
    __syncthreads();
    if (work) {  // phase C: the counts of both lists, and the decision
      resolve_count_pairs(L);
      ccnt[fr * SPH_FANOUT + t] = C.count(c0, c1);
      if (t == 0) resolve_decide<true>(L, M, A, k, resolve_sum16(L.pk + Y.pebase) * A.wcol, resolve_sum16(L.pk + oebase) * O.wobs);
    }
    __syncthreads();
    if (work && t == 0) {  // (stat, nact and ncon of a frame are its thread 0's alone until the next barrier)
      const int total = resolve_pair_total(L);
      int ctotal = 0;
      for (int u = 0; u < SPH_FANOUT; ++u) ctotal += ccnt[fr * SPH_FANOUT + u];
      if (C.capped(ctotal)) L.stat[fr] |= DEXR_RESOLVE_CONTACTS_TRUNCATED;
      const bool keep = L.accf[fr] != 0 && L.stopf[fr] == 0;
      L.nact[fr] = keep ? total : 0;
      ncon[fr] = keep ? ctotal : 0;
    }
    if (resolve_all_stopped(L)) break;
    const bool go = L.stopf[fr] == 0;          // the frame goes on: it needs a next trial
    const bool build = go && L.accf[fr] != 0;  // ... from a new point: its lists, g and H are formed and kept
    if (build) {  // phase D: both lists in their orders, then g
      resolve_list_pairs(L);
      int coff = 0;
      for (int u = 0; u < t; ++u) coff += ccnt[fr * SPH_FANOUT + u];
      C.append(c0, c1, coff, sph_in);
      resolve_gradient<true>(L, M, Y, A, xr);
    }
    __syncthreads();
    const unsigned long long frozen = resolve_frozen(L);
    if (build) resolve_base_h(L, M, Y, A, frozen);
    int nmax = 0, cmax = 0;  // the block's largest lists: the same in every thread
    for (int f = 0; f < nl; ++f) {
      nmax = L.nact[f] > nmax ? L.nact[f] : nmax;
      cmax = ncon[f] > cmax ? ncon[f] : cmax;
    }
    const int mine_n = L.nact[fr], mine_c = ncon[fr];  // (0 unless `build`)
    nmax = (nmax + SPH_FANOUT - 1) / SPH_FANOUT * SPH_FANOUT;  // whole chunks: the contacts start at a chunk boundary of their own
    for (int base = 0; base < nmax + cmax; base += SPH_FANOUT) {  // the curvature, sixteen rows at a time: the pairs' grad d_p, then
      const bool pairs = base < nmax;                               // the contacts' grad d (the same choice in every thread)
      const int at = pairs ? base : base - nmax;
      const int have = pairs ? mine_n : mine_c;
      if (at + t < have) {
        T n[3], w;
        int si, sj;
        if (pairs) {
          resolve_pair_contact(L, M, A, at + t, si, sj, n, w);
        } else {
          sj = -1;
          C.contact(O, po, L.cen, at + t, si, n, w);
        }
        resolve_stage_row(L, M, frozen, si, sj, n, w);
      }
      __syncthreads();
      const int nk = have - at < SPH_FANOUT ? have - at : SPH_FANOUT;
      if (nk > 0) resolve_rank16(L, M, nk);
      __syncthreads();
    }
    if (go) resolve_damp(L, M, frozen);  // phase E
    __syncthreads();
    ik_factor_solve(L.H, L.g, L.y, L.dg, M.n_act, t, go);
    if (go) resolve_step(L, M, A);
    __syncthreads();
  }
  if (inb) resolve_output(L, A, P.n_in, first + fr, 4);
}

template <typename T>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES)
    pose_resolve_obstacle_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links, PoseArgs<T> P,
                                 const SphereD<T>* __restrict__ spheres, const T* __restrict__ rsum, SphereIndex S,
                                 const int32_t* __restrict__ sph_in, const uint32_t* __restrict__ pair_sph, const JacEnt* __restrict__ ents,
                                 const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col, const uint2* __restrict__ tri,
                                 const ObstacleD<T>* __restrict__ prims, const T* __restrict__ ow, int n_prim, int n_jx, int n_act,
                                 ResolveLayout Y, int obase, int oebase, int fstride, ResolveArgs<T> A, ResolveObstacleArgs<T> O) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const ResolveModel<T> M = {joints, links, spheres, rsum, S, pair_sph, ents, act_rng, act_col, tri, n_act, n_act * (n_act + 1) / 2};
  const ObstacleContacts<T> C = {prims, obstacle_kinds(prims), ow, n_prim, nullptr, nullptr};
  resolve_contact_loop<T>(pose_lds, M, P, sph_in, Y, obase, oebase, fstride, A, O, C);
}

// the argument rules of the four contact entry points: the obstacle side's, then those of check_resolve_call; < 0 error, 1 nothing
// to do, 0 go on.  obstacle: the set or the grid, no_obstacle: what to say where it is NULL
int check_resolve_contact_call(const dexr_sphere_model* sm, const void* obstacle, const char* no_obstacle, double omargin, double wobs, int64_t B,
                               const void* x0, const void* fixed, int32_t n_target, const void* tp, const void* tr, const void* wl, const void* wa,
                               double margin, double wcol, const void* lo, const void* hi, double damping, double max_step, double tol,
                               int32_t max_iters, const void* x_out) {
  const double big = 1.7976931348623157e308;
  if (!sm) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (!obstacle) return dexr_set_error(DEXR_ERR_INVALID, "%s", no_obstacle);
  if (!(omargin >= 0.0) || omargin > big) return dexr_set_error(DEXR_ERR_INVALID, "obstacle_margin must be finite and >= 0, got %g", omargin);
  if (!(wobs >= 0.0) || wobs > big) return dexr_set_error(DEXR_ERR_INVALID, "obstacle_weight must be finite and >= 0, got %g", wobs);
  return check_resolve_call(sm, B, x0, fixed, n_target, tp, tr, wl, wa, margin, wcol, lo, hi, damping, max_step, tol, max_iters, x_out);
}

// the layout of a contact kernel's frame: behind the scalars of ResolveLayout the obstacle pose, then sixteen partial energies
template <typename T>
ResolveLayout resolve_contact_layout(const dexr_sphere_model* sm, int n_target, int* obase, int* oebase) {
  ResolveLayout Y = resolve_layout<T>(sm, n_target);
  *obase = Y.sbase + RSV_SCALARS, *oebase = *obase + OBS_POSE;
  Y.stride = (*oebase + SPH_FANOUT) | 1;
  return Y;
}

template <typename T>
int launch_resolve_obstacles(const dexr_sphere_model* sm, const dexr_obstacle_set* os, int64_t B, ResolveArgs<T> A, const ResolveObstacleArgs<T>& O,
                             const T* ow, hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  int obase, oebase;
  const ResolveLayout Y = resolve_contact_layout<T>(sm, A.n_target, &obase, &oebase);
  // (the formula of include/dexr_resolve_obstacles.h)
  const size_t per_frame = resolve_lds_bytes<T>(sm, Y, ObstacleContacts<T>::head_words(sm->n_sphere),
                                                RESOLVE_CONTACT_COUNTS + ObstacleContacts<T>::tail_bytes(sm->n_sphere));
  int nl;
  int64_t blocks;
  if (const int rc = resolve_launch_shape(per_frame, B, &nl, &blocks)) return rc;
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  if (!A.xref) A.xref = A.x0;
  hipLaunchKernelGGL(pose_resolve_obstacle_kernel<T>, dim3((unsigned)blocks), dim3(nl * SPH_FANOUT), per_frame * nl, st,
                     (const JointD<T>*)tables_of<T>(m).joints, (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B),
                     (const SphereD<T>*)sphere_tables_of<T>(sm).spheres, (const T*)sphere_tables_of<T>(sm).rsum, S, (const int32_t*)sm->sph_in,
                     (const uint32_t*)sm->pair_sph, (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col,
                     (const uint2*)m->ik_tri, obstacle_table_of<T>(os), ow, os->n_prim, m->n_jx, m->n_act, Y, obase, oebase,
                     (sm->n_pair + 3) & ~3, A, O);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "obstacle resolve kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

}  // namespace

extern "C" {

int dexr_sphere_resolve_obstacles_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                      const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                      const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                      const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                                      int32_t max_iters, const dexr_obstacle_set* obstacles, const float* obstacle_pos, const float* obstacle_rot,
                                      float obstacle_margin, float obstacle_weight, const float* prim_weight, float* x_out, int32_t* iters_out,
                                      float* energy_out, int32_t* status_out, void* stream) {
  const int c = check_resolve_contact_call(m, obstacles, "null obstacle set", (double)obstacle_margin, (double)obstacle_weight, B, x0, fixed,
                                           n_target, target_pos, target_rot, pos_weight, rot_weight, (double)margin, (double)collision_weight, lo,
                                           hi, (double)damping, (double)max_step, (double)tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const ResolveArgs<float> A = {x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi,
                                margin, collision_weight, damping, max_step, tol, n_target, max_iters, x_out, iters_out, energy_out, status_out};
  const ResolveObstacleArgs<float> O = {obstacle_pos, obstacle_rot, obstacle_margin, obstacle_weight};
  return launch_resolve_obstacles<float>(m, obstacles, B, A, O, prim_weight, (hipStream_t)stream);
}

int dexr_sphere_resolve_obstacles(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                                  const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                                  const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                                  const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                                  int32_t max_iters, const dexr_obstacle_set* obstacles, const double* obstacle_pos, const double* obstacle_rot,
                                  double obstacle_margin, double obstacle_weight, const double* prim_weight, double* x_out, int32_t* iters_out,
                                  double* energy_out, int32_t* status_out) {
  const int c = check_resolve_contact_call(m, obstacles, "null obstacle set", obstacle_margin, obstacle_weight, B, x0, fixed, n_target,
                                           target_pos, target_rot, pos_weight, rot_weight, margin, collision_weight, lo, hi, damping, max_step,
                                           tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  ResolveRoundTrip D;
  ResolveArgs<double> A;
  if (const int rc = D.up(m, B, x0, fixed, x_ref, posture_weight, n_target, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi))
    return rc;
  DevBuf dop, dor, dow;
  if (obstacle_pos) POSE_HIP(dop.put(obstacle_pos, (size_t)B * 3 * sizeof(double)));
  if (obstacle_rot) POSE_HIP(dor.put(obstacle_rot, (size_t)B * 9 * sizeof(double)));
  if (prim_weight) POSE_HIP(dow.put(prim_weight, (size_t)obstacles->n_prim * sizeof(double)));
  if (const int rc = D.out(B, 4, margin, collision_weight, damping, max_step, tol, n_target, max_iters, &A)) return rc;
  const ResolveObstacleArgs<double> O = {(const double*)dop.p, (const double*)dor.p, obstacle_margin, obstacle_weight};
  if (const int rc = launch_resolve_obstacles<double>(m, obstacles, B, A, O, (const double*)dow.p, nullptr)) return rc;
  return D.down(x_out, iters_out, energy_out, status_out);
}

}  // extern "C"

// dexr_resolve_cross.hpp -- the collision-aware posture solve against a second posed robot (include/dexr_resolve_cross.h): a
// fragment of dexr_pose.hip, which includes it once after dexr_cross.hpp.  The loop has a home of its own here,
// resolve_cross_loop<T>: the skeleton of resolve_scene_loop (dexr_resolve_scene.hpp) made of the same resolve_* phases of
// dexr_resolve.hpp, with robot B's spheres where that one asks its bodies.  The pair arithmetic is dexr_cross.hpp's as it stands:
// cross_walk places B's centres (pos + rot c), cross_gap and cross_inv give D, s, d and 1 / s.
//
// B'S TABLE IS UNIFORM DATA: CrossBodyD<T> travels by value as a kernel argument -- B's joint, link and sphere tables, its x and
// fixed rows, its pose pointers, the pair weights, margin_x and w_x.  B's sphere count is the same in every thread of a block; no
// barrier stands under a condition that differs inside a block.
//
// What a pass does beyond pose_resolve_kernel:
//   A  pass 0 also walks B ONCE, in lanes that A's walk leaves idle (the first nl lanes of the block's second wave; a block of one
//      wave: the nl lanes behind A's), and parks B's centres in A's root frame, 3 S_b values per frame; B does not move after that;
//   B  the thread's spheres get their pair forces times w_col first; then every sphere s of the thread runs over all of B in B's
//      table order (radius and caller's index by uniform loads, the centre an LDS broadcast): a pair outside the margin costs the
//      distance and one compare, the reciprocal and the force sit behind the branch.  w_st h_st^2 goes onto the thread's partial
//      E_x, the force becomes fma(w_x, f_x, w_col f_pairs), and a 128-bit active mask goes to LDS per caller's sphere index of A (two
//      64-bit words, bit = caller's sphere index of B);
//   C  thread t counts the contacts (popcounts) of its contiguous slice of A's caller indices; thread 0 adds the sixteen partial
//      energies in order, weighs them and decides on E = ((E_pose + E_post) + E_col) + E_x;
//   D  the contacts go into ONE list at a prefix over the sixteen counts, no atomics: A's caller index, then B's caller index; an
//      entry is 16 bits, A's sorted sphere (7) | B's table sphere << 7 (7).  The list is capped at DEXR_RESOLVE_MAXCONTACT with
//      DEXR_RESOLVE_CONTACTS_TRUNCATED.  After the pair chunks the contact curvature goes through the same rank-16 staging: a
//      contact's normal is recomputed from the two parked centres through the functions of phase B (the same bits).
// Kept system, phase E, factor / solve and the outputs are those of pose_resolve_kernel; energy_out has four columns.  The rule's
// constants are the headers', read where the rule stands: DEXR_RESOLVE_LAM_UP, DEXR_RESOLVE_LAM_DOWN and DEXR_RESOLVE_MAXREJECT in
// resolve_decide, DEXR_RESOLVE_MAXACTIVE in resolve_pair_total and resolve_list_pairs (dexr_resolve.hpp), DEXR_RESOLVE_MAXCONTACT and
// DEXR_RESOLVE_CONTACTS_TRUNCATED here.
//
// LDS of a block: sixteen 64-bit partial frozen masks per frame | two 64-bit contact words per sphere of A and frame | the fork
// slots of A, then of B ([value][lane] each) | per frame a region [frame][stride], odd stride (ResolveLayout, then B's centres, B's
// parked pose, sixteen partial energies) | per frame the active pairs, sixteen counts, six words of state, sixteen contact counts,
// the curvature contacts | per frame the contact list (16 bits each) | per frame one byte per pair.
// include/dexr_resolve_cross.h states the bytes.
#include "dexr_resolve_cross.h"

namespace {

static_assert(DEXR_SPHERE_MAX <= 128, "a contact is 7 + 7 bits and a sphere's mask two 64-bit words");

template <typename T>
struct CrossBodyD {
  const JointD<T>* joints;
  const LinkD<T>* links;
  PoseArgs<T> P;
  const SphereD<T>* spheres;
  SphereIndex S;
  const int32_t* sph_in;  // (S_b): B's table index of B's caller's sphere
  const T* x;             // (B, n_in_b)
  const T* fixed;         // (B, n_fixed_b) or NULL
  const T* opos;          // (B, 3) or NULL
  const T* orot;          // (B, 3, 3) or NULL
  const T* xw;            // (S_a, S_b) or NULL
  T xmargin, wx;
};

// offsets (in values) into a frame's region behind the scalars of ResolveLayout: B's centres, B's parked pose, sixteen partial E_x
struct CrossResolveLayout {
  int cbbase, pbbase, xebase;
};

constexpr int XRS_MASK_WORDS = 2;  // 64-bit words of a sphere's active mask

// the term of B on A's sorted sphere at cs (radius rs, caller's index so): f = sum_t w_st h_st n_st over B in table order, w_st
// h_st^2 onto ex, the active spheres of B (caller's indices) into the two words of m
template <typename T>
__device__ __forceinline__ void cross_resolve_term(const CrossBodyD<T>& Q, const T* cenb, const T cs[3], T rs, int so, T& ex, T f[3],
                                                   unsigned long long m[XRS_MASK_WORDS]) {
  const int nb = Q.S.n_sphere;
  const T* wrow = Q.xw ? Q.xw + (size_t)so * nb : nullptr;
  unsigned long long m0 = 0, m1 = 0;
  T f0 = T(0), f1 = T(0), f2 = T(0);
  for (int u = 0; u < nb; ++u) {
    T D[3], sd;
    const T d = cross_gap(cs, rs, cenb + 3 * u, Q.spheres[u].r, D, sd);
    const T h = Q.xmargin - d;
    if (h <= T(0)) continue;  // (a comparison: a NaN goes on and stays a NaN)
    const int ob = Q.S.sph_out[u];
    const T wh = wrow ? wrow[ob] * h : h;
    ex = fma(wh, h, ex);
    if (h > T(0)) {  // (a NaN is no contact)
      const unsigned long long bit = 1ull << (ob & 63);
      if (ob < 64) m0 |= bit;
      else m1 |= bit;
    }
    const T k = wh * cross_inv(sd);
    f0 = fma(k, D[0], f0);
    f1 = fma(k, D[1], f1);
    f2 = fma(k, D[2], f2);
  }
  f[0] = f0, f[1] = f1, f[2] = f2;
  m[0] = m0, m[1] = m1;
}

// the q-th contact of the list: A's sorted sphere, its normal and its weight, from the two parked centres through the functions of
// phase B
template <typename T>
__device__ __forceinline__ void cross_resolve_contact(const CrossBodyD<T>& Q, const SphereD<T>* __restrict__ spheres_a,
                                                      const int32_t* __restrict__ out_a, const uint16_t* clst, const T* cen, const T* cenb,
                                                      int q, int& si, T n[3], T& w) {
  const uint32_t cm = clst[q];
  const int ub = (cm >> 7) & 127;
  si = cm & 127;
  T D[3], sd;
  (void)cross_gap(cen + 3 * si, spheres_a[si].r, cenb + 3 * ub, Q.spheres[ub].r, D, sd);
  const T inv = cross_inv(sd);
#pragma unroll
  for (int i = 0; i < 3; ++i) n[i] = D[i] * inv;
  w = Q.xw ? Q.wx * Q.xw[(size_t)out_a[si] * Q.S.n_sphere + Q.S.sph_out[ub]] : Q.wx;
}

// The resident loop of the two-robot kernel.  THE LOOP CANNOT HANG, for the reasons written down at pose_resolve_kernel
// (dexr_resolve.hpp) and re-checked here: it runs k = 0 .. max_iters at most; every __syncthreads() stands in the body of the k
// loop or of the chunk loop, outside every condition that differs between the threads of a block -- B's walk in pass 0 sits beside
// A's under the same lane test, in front of the barrier that ends phase A, and the loop over B's spheres in phases B and D holds
// no barrier, its trip count S_b a kernel argument; both chunk counts of the curvature loop (nmax, cmax) are the block's largest,
// read by every thread from LDS (nact, ncon of all frames) after the barrier that follows their last write, and not written again
// before the barrier that ends phase E; a frame that has stopped (or an idle lane of a ragged last block: stopped from the start)
// does no work and writes nothing but walks through the same barriers; the one early exit is taken on the AND of all stop flags,
// read by every thread after the same barrier, and at k == max_iters every flag is set.  Every sum is taken by one thread in
// table order: a frame's bits do not depend on the batch or on its neighbours.
template <typename T>
__device__ __forceinline__ void resolve_cross_loop(unsigned char* pose_lds, const ResolveModel<T>& M, const PoseArgs<T>& P,
                                                   const int32_t* __restrict__ sph_in, const ResolveLayout Y, const CrossResolveLayout Z,
                                                   int fstride, const ResolveArgs<T> A, const CrossBodyD<T>& Q) {
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  const SphereIndex& S = M.S;
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  const int ns = S.n_sphere;
  const ResolveLds<T> L = resolve_lds<T>(pose_lds, nl, fr, t, Y, P.n_slot + Q.P.n_slot, M.n_act, S.n_pair, fstride, XRS_MASK_WORDS * ns,
                                         RESOLVE_CONTACT_COUNTS + DEXR_RESOLVE_MAXCONTACT * (int)sizeof(uint16_t));
  int32_t* ccnt = reinterpret_cast<int32_t*>(L.tail);  // [nl][SPH_FANOUT]: contacts of a thread's slice of spheres
  int32_t* ncon = ccnt + nl * SPH_FANOUT;              // [nl]: curvature contacts
  uint16_t* clst = reinterpret_cast<uint16_t*>(ncon + nl) + fr * DEXR_RESOLVE_MAXCONTACT;  // the frame's contact list
  unsigned long long* msk = L.head + fr * (XRS_MASK_WORDS * ns);  // [n_sphere][2] the frame's contact masks, by A's caller's sphere index
  T* slots_b = L.slots + P.n_slot * 12 * nl;                      // B's fork slots behind A's
  const int64_t first = (int64_t)blockIdx.x * nl;
  const bool inb = first + fr < P.B;
  const T* cenb = L.pk + Z.cbbase;  // B's centres in A's root frame
  const T* xr = A.xref + (inb ? first + fr : 0) * P.n_in;  // (read by working frames alone)
  const int schunk = (ns + SPH_FANOUT - 1) / SPH_FANOUT;  // thread t owns A's caller's spheres [t schunk, (t + 1) schunk)
  const int c0 = t * schunk < ns ? t * schunk : ns, c1 = c0 + schunk < ns ? c0 + schunk : ns;
  const int lane_b = tid - (blockDim.x > 64 ? 64 : nl);  // B's walk: the second wave where the block has one
  resolve_start(L, A, P.n_in, first + fr, inb);
  if (t == 0) ncon[fr] = 0;
  __syncthreads();
  for (int k = 0; k <= A.max_iters; ++k) {
    if (tid < nl) {  // phase A
      if (L.stopf[tid] == 0) resolve_walk(L, M.joints, M.links, M.spheres, S, P, Y, A, tid, first);
    } else if (k == 0 && lane_b >= 0 && lane_b < nl && L.stopf[lane_b] == 0) {  // pass 0: B, once, beside A's walk
      T* pb = L.park + lane_b * Y.stride;
      cross_walk<T, false>(Q.joints, Q.links, Q.P, Q.spheres, Q.S, Q.x, Q.fixed, Q.opos, Q.orot, slots_b, nl, lane_b, first, pb + Z.cbbase,
                           pb + Z.pbbase, nullptr, nullptr);
    }
    __syncthreads();
    const bool work = L.stopf[fr] == 0;
    if (work) {  // phase B: a thread per sphere of A; its pair forces, then B's term: force, energy, active mask
      T e = T(0), ex = T(0);
      for (int s = t; s < ns; s += SPH_FANOUT) {
        const T cs[3] = {L.cen[3 * s], L.cen[3 * s + 1], L.cen[3 * s + 2]};
        T f[3], fx[3];
        resolve_pair_forces(L, M, A, s, cs, e, f);
        const int so = S.sph_out[s];
        unsigned long long m[XRS_MASK_WORDS];
        cross_resolve_term(Q, cenb, cs, M.spheres[s].r, so, ex, fx, m);
        msk[XRS_MASK_WORDS * so] = m[0];
        msk[XRS_MASK_WORDS * so + 1] = m[1];
        L.frc[3 * s] = fma(Q.wx, fx[0], A.wcol * f[0]);
        L.frc[3 * s + 1] = fma(Q.wx, fx[1], A.wcol * f[1]);
        L.frc[3 * s + 2] = fma(Q.wx, fx[2], A.wcol * f[2]);
      }
      L.pk[Y.pebase + t] = e;
      L.pk[Z.xebase + t] = ex;
    }
    __syncthreads();
    if (work) {  // phase C: the counts of both lists, and the decision
      resolve_count_pairs(L);
      int n = 0;
      for (int c = XRS_MASK_WORDS * c0; c < XRS_MASK_WORDS * c1; ++c) n += __popcll(msk[c]);
      ccnt[fr * SPH_FANOUT + t] = n;
      if (t == 0) resolve_decide<true>(L, M, A, k, resolve_sum16(L.pk + Y.pebase) * A.wcol, resolve_sum16(L.pk + Z.xebase) * Q.wx);
    }
    __syncthreads();
    if (work && t == 0) {  // (stat, nact and ncon of a frame are its thread 0's alone until the next barrier)
      const int total = resolve_pair_total(L);
      int ctotal = 0;
      for (int u = 0; u < SPH_FANOUT; ++u) ctotal += ccnt[fr * SPH_FANOUT + u];
      if (ctotal > DEXR_RESOLVE_MAXCONTACT) {
        L.stat[fr] |= DEXR_RESOLVE_CONTACTS_TRUNCATED;
        ctotal = DEXR_RESOLVE_MAXCONTACT;
      }
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
      for (int c = c0; c < c1 && coff < DEXR_RESOLVE_MAXCONTACT; ++c) {  // A's caller's sphere order, then B's caller's sphere order
        const uint32_t s = (uint32_t)sph_in[c];
        for (int wd = 0; wd < XRS_MASK_WORDS; ++wd) {
          unsigned long long bits = msk[XRS_MASK_WORDS * c + wd];
          while (bits != 0 && coff < DEXR_RESOLVE_MAXCONTACT) {
            const int ob = __ffsll((long long)bits) - 1 + 64 * wd;
            clst[coff++] = (uint16_t)(s | ((uint32_t)Q.sph_in[ob] << 7));
            bits &= bits - 1;
          }
        }
      }
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
          cross_resolve_contact(Q, M.spheres, S.sph_out, clst, L.cen, cenb, at + t, si, n, w);
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
    pose_resolve_cross_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links, PoseArgs<T> P,
                              const SphereD<T>* __restrict__ spheres, const T* __restrict__ rsum, SphereIndex S,
                              const int32_t* __restrict__ sph_in, const uint32_t* __restrict__ pair_sph, const JacEnt* __restrict__ ents,
                              const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col, const uint2* __restrict__ tri, int n_jx,
                              int n_act, ResolveLayout Y, CrossResolveLayout Z, int fstride, ResolveArgs<T> A, CrossBodyD<T> Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const ResolveModel<T> M = {joints, links, spheres, rsum, S, pair_sph, ents, act_rng, act_col, tri, n_act, n_act * (n_act + 1) / 2};
  resolve_cross_loop<T>(pose_lds, M, P, sph_in, Y, Z, fstride, A, Q);
}

// the two-robot argument rules, then those of check_resolve_call and B's of check_call; < 0 error, 1 nothing to do, 0 go on
int check_resolve_cross_call(const dexr_sphere_model* sm, const dexr_sphere_model* other, int64_t B, const void* x0, const void* fixed,
                             int32_t n_target, const void* tp, const void* tr, const void* wl, const void* wa, double margin, double wcol,
                             const void* lo, const void* hi, double damping, double max_step, double tol, int32_t max_iters, const void* x_b,
                             const void* fixed_b, double margin_x, double w_x, const void* x_out) {
  const double big = 1.7976931348623157e308;
  if (!sm) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (!other) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model of the other robot");
  if (!(margin_x >= 0.0) || margin_x > big) return dexr_set_error(DEXR_ERR_INVALID, "margin_x must be finite and >= 0, got %g", margin_x);
  if (!(w_x >= 0.0) || w_x > big) return dexr_set_error(DEXR_ERR_INVALID, "w_x must be finite and >= 0, got %g", w_x);
  const int c = check_resolve_call(sm, B, x0, fixed, n_target, tp, tr, wl, wa, margin, wcol, lo, hi, damping, max_step, tol, max_iters, x_out);
  if (c) return c;
  if (!x_b && other->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "x_b is NULL");
  if (!fixed_b && other->pose->h.n_fixed > 0)
    return dexr_set_error(DEXR_ERR_INVALID, "the other robot's table reads %d fixed columns: fixed_b must not be NULL", other->pose->h.n_fixed);
  return 0;
}

// the layout of the two-robot kernel's frame: behind the scalars of ResolveLayout B's centres, B's parked pose, sixteen energies
template <typename T>
ResolveLayout resolve_cross_layout(const dexr_sphere_model* sm, const dexr_sphere_model* other, int n_target, CrossResolveLayout* Z) {
  ResolveLayout Y = resolve_layout<T>(sm, n_target);
  Z->cbbase = Y.sbase + RSV_SCALARS;
  Z->pbbase = Z->cbbase + 3 * other->n_sphere;
  Z->xebase = Z->pbbase + CRS_POSE;
  Y.stride = (Z->xebase + SPH_FANOUT) | 1;
  static_assert(CRS_POSE + SPH_FANOUT == 28, "include/dexr_resolve_cross.h states 3 S_b + 12 + 16");
  return Y;
}

template <typename T>
int launch_resolve_cross(const dexr_sphere_model* sm, const dexr_sphere_model* other, int64_t B, ResolveArgs<T> A, const T* x_b,
                         const T* fixed_b, const T* opos, const T* orot, T xmargin, T wx, const T* xw, hipStream_t st) {
  const dexr_pose_model *m = sm->pose, *mb = other->pose;
  CrossResolveLayout Z;
  const ResolveLayout Y = resolve_cross_layout<T>(sm, other, A.n_target, &Z);
  // (the formula of include/dexr_resolve_cross.h: B's fork slots stand behind A's)
  const size_t per_frame = resolve_lds_bytes<T>(sm, Y, (size_t)XRS_MASK_WORDS * sm->n_sphere,
                                                RESOLVE_CONTACT_COUNTS + DEXR_RESOLVE_MAXCONTACT * sizeof(uint16_t)) +
                           (size_t)mb->h.n_slot * 12 * sizeof(T);
  int nl;
  int64_t blocks;
  if (per_frame > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the two sphere models need %zu B of LDS per frame: one frame does not fit a block", per_frame);
  if (const int rc = resolve_launch_shape(per_frame, B, &nl, &blocks)) return rc;
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  CrossBodyD<T> Q;
  Q.joints = (const JointD<T>*)tables_of<T>(mb).joints, Q.links = (const LinkD<T>*)tables_of<T>(mb).links, Q.P = args_of<T>(mb, B);
  Q.spheres = (const SphereD<T>*)sphere_tables_of<T>(other).spheres;
  Q.S = {other->link_sph, other->sph_out, other->inc_ptr, other->inc, other->n_sphere, other->n_pair};
  Q.sph_in = (const int32_t*)other->sph_in;
  Q.x = x_b, Q.fixed = fixed_b, Q.opos = opos, Q.orot = orot, Q.xw = xw, Q.xmargin = xmargin, Q.wx = wx;
  if (!A.xref) A.xref = A.x0;
  hipLaunchKernelGGL(pose_resolve_cross_kernel<T>, dim3((unsigned)blocks), dim3(nl * SPH_FANOUT), per_frame * nl, st,
                     (const JointD<T>*)tables_of<T>(m).joints, (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B),
                     (const SphereD<T>*)sphere_tables_of<T>(sm).spheres, (const T*)sphere_tables_of<T>(sm).rsum, S, (const int32_t*)sm->sph_in,
                     (const uint32_t*)sm->pair_sph, (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col,
                     (const uint2*)m->ik_tri, m->n_jx, m->n_act, Y, Z, (sm->n_pair + 3) & ~3, A, Q);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "two-robot resolve kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

}  // namespace

extern "C" {

int dexr_sphere_resolve_cross_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                  const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                  const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                  const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                                  int32_t max_iters, const dexr_sphere_model* other, const float* x_b, const float* fixed_b,
                                  const float* other_pos, const float* other_rot, float margin_x, float w_x, const float* cross_weight,
                                  float* x_out, int32_t* iters_out, float* energy_out, int32_t* status_out, void* stream) {
  const int c = check_resolve_cross_call(m, other, B, x0, fixed, n_target, target_pos, target_rot, pos_weight, rot_weight, (double)margin,
                                         (double)collision_weight, lo, hi, (double)damping, (double)max_step, (double)tol, max_iters, x_b,
                                         fixed_b, (double)margin_x, (double)w_x, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const ResolveArgs<float> A = {x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi,
                                margin, collision_weight, damping, max_step, tol, n_target, max_iters, x_out, iters_out, energy_out, status_out};
  return launch_resolve_cross<float>(m, other, B, A, x_b, fixed_b, other_pos, other_rot, margin_x, w_x, cross_weight, (hipStream_t)stream);
}

int dexr_sphere_resolve_cross(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                              const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                              const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                              const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                              int32_t max_iters, const dexr_sphere_model* other, const double* x_b, const double* fixed_b,
                              const double* other_pos, const double* other_rot, double margin_x, double w_x, const double* cross_weight,
                              double* x_out, int32_t* iters_out, double* energy_out, int32_t* status_out) {
  const int c = check_resolve_cross_call(m, other, B, x0, fixed, n_target, target_pos, target_rot, pos_weight, rot_weight, margin,
                                         collision_weight, lo, hi, damping, max_step, tol, max_iters, x_b, fixed_b, margin_x, w_x, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  ResolveRoundTrip D;
  ResolveArgs<double> A;
  if (const int rc = D.up(m, B, x0, fixed, x_ref, posture_weight, n_target, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi))
    return rc;
  const dexr_pose_model* mb = other->pose;
  DevBuf dxb, dfb, dop, dor, dxw;
  POSE_HIP(dxb.put(x_b, (size_t)B * mb->h.n_in * sizeof(double)));
  POSE_HIP(dfb.put(fixed_b, (size_t)B * mb->h.n_fixed * sizeof(double)));
  if (other_pos) POSE_HIP(dop.put(other_pos, (size_t)B * 3 * sizeof(double)));
  if (other_rot) POSE_HIP(dor.put(other_rot, (size_t)B * 9 * sizeof(double)));
  if (cross_weight) POSE_HIP(dxw.put(cross_weight, (size_t)m->n_sphere * other->n_sphere * sizeof(double)));
  if (const int rc = D.out(B, 4, margin, collision_weight, damping, max_step, tol, n_target, max_iters, &A)) return rc;
  if (const int rc = launch_resolve_cross<double>(m, other, B, A, (const double*)dxb.p, (const double*)dfb.p, (const double*)dop.p,
                                                  (const double*)dor.p, margin_x, w_x, (const double*)dxw.p, nullptr))
    return rc;
  return D.down(x_out, iters_out, energy_out, status_out);
}

}  // extern "C"

// dexr_resolve.hpp -- the collision-aware posture solve (include/dexr_resolve.h): a fragment of dexr_pose.hip, which includes it
// once after dexr_spheres.hpp.  It is the ONE home of the resident loop's phases: the resolve_* helpers below are what
// pose_resolve_kernel<T> (here) and the contact kernels (resolve_contact_loop of dexr_resolve_obstacles.hpp, instantiated for
// primitives there and for a grid in dexr_resolve_grid.hpp) are made of, and the host helpers at the end (ResolveRoundTrip,
// resolve_launch_shape, resolve_lds_bytes, check_resolve_call) serve all three pairs of entry points.  The loop is the resident
// loop of pose_ik_solve_kernel with the phases of pose_sphere_kernel inside it, an accept / reject rule and a per-frame damping.
//
// One pass of the loop evaluates ONE point per frame (pass 0 the start, pass k the k-th trial) and, where the frame goes on, ends
// with the next trial in LDS:
//   A  (lane = frame)        the forward walk at the trial: a, o per joint driven by x, the IK_LINK record of every link (targets
//                            through ik_link_target, weights 0 on the links that carry none), the sphere centres, E_pose, E_post;
//   B  (16 threads a frame)  thread t owns the spheres t, t + 16, ...: their incidence lists give the forces f_s = sum w_p h_p n_p
//                            and sixteen partial energies; the first end of a pair also writes the pair's active flag (a byte);
//   C                        thread t counts the flags of its slice of the pair list; thread 0 of the frame adds the energies in
//                            order and takes the accept / reject decision, moves x, lam, the reject count and the stop flag;
//      the block's vote      the one early exit, on the AND of the stop flags;
//   D  (accepted trials)     the active list from the sixteen counts (a prefix in thread order: pair-index order, no atomics), g
//                            with the freeze masks, then H without the damping: ik_h_entry + the posture diagonal + the pair
//                            curvature, the rows grad d_p staged sixteen pairs at a time in LDS and applied as a rank-16 update;
//                            g and H are KEPT: a rejected trial leaves x where it was, so its next system is the kept one with a
//                            larger lam -- no second walk and no pass is spent on a rejection;
//   E                        H + lam I, ik_factor_solve unchanged, the step limit, the move and the clamp: the next trial.
// A helper holds no barrier: every __syncthreads() stands in the body of a loop, outside every divergent condition.  The helpers
// take ResolveArgs and ResolveLayout by value and form LDS offsets in 32 bits: both keep the kernels' registers where they were
// (docs/experiments/collision_resolve_shared.md).
//
// Two things differ between the plain kernel and the contact kernels, by the compile-time parameter OBS of the helper concerned:
// the plain kernel keeps unweighted pair forces and gives them w_col in g, and decides on (E_pose + E_post) + E_col; the contact
// kernels' forces carry w_col and w_obs already, and they decide on ((E_pose + E_post) + E_col) + E_obs.
//
// LDS of a block (resolve_lds): sixteen 64-bit partial frozen masks per frame | a contact source's 64-bit words | the fork slots |
// per frame a region [frame][stride], odd stride (ResolveLayout) | per frame the active list (DEXR_RESOLVE_MAXACTIVE pair
// indices), sixteen counts, six words of state | a contact source's bytes | per frame one byte per pair.  The plain kernel has no
// contact source.  The staged rows of the curvature share the place of the working copy of H, which is formed after them.
#include "dexr_resolve.h"

namespace {

// a frame's scalars: E, lam, the trial's E_pose and E_post, then the terms of E at the accepted point (RSV_OBS: the contact kernels')
constexpr int RSV_E = 0, RSV_LAM = 1, RSV_TPOSE = 2, RSV_TPOST = 3, RSV_POSE = 4, RSV_POST = 5, RSV_COL = 6, RSV_OBS = 7, RSV_SCALARS = 8;

// offsets (in values) into a frame's region
struct ResolveLayout {
  int lbase;   // IK_LINK per sorted link (none without targets)
  int cbase;   // centres, 3 per sphere
  int fbase;   // forces, 3 per sphere
  int pebase;  // sixteen partial energies
  int hbase;   // H + lam I, then its factor; before that the sixteen staged rows (n_act each) and their sixteen weights
  int hsbase;  // H of the last accepted point, before the damping
  int gbase, gsbase, ybase, dbase;  // g (later dx) | g of the last accepted point | y | the factor's diagonal
  int xbase;   // the trial (all n_in columns): what the walk reads
  int xsbase;  // the last accepted point
  int sbase;   // RSV_SCALARS scalars
  int stride;
};

template <typename T>
struct ResolveArgs {
  const T* x0;
  const T* fixed;
  const T* xref;  // never NULL: x0 where the caller gave none
  const T* u;
  const T* tp;
  const T* tr;
  const T* wl;
  const T* wa;
  const T* pw;
  const T* lo;
  const T* hi;
  T margin, wcol, damping, max_step, tol;
  int32_t n_target, max_iters;
  T* x_out;
  int32_t* iters_out;
  T* e_out;
  int32_t* status_out;
};

// the model's tables as a kernel got them: bundled for the helpers, taken apart again by the compiler
template <typename T>
struct ResolveModel {
  const JointD<T>* joints;
  const LinkD<T>* links;
  const SphereD<T>* spheres;
  const T* rsum;
  const SphereIndex& S;
  const uint32_t* pair_sph;
  const JacEnt* ents;
  const uint32_t* act_rng;
  const int32_t* act_col;
  const uint2* tri;
  int n_act, n_tri;
};

// a thread's view of its block's LDS and of its frame's share of it
template <typename T>
struct ResolveLds {
  int nl, fr, t;             // frames of this block | the thread's frame, and its place among the frame's SPH_FANOUT threads
  unsigned long long* part;  // [nl][SPH_FANOUT] partial frozen masks
  unsigned long long* head;  // [nl][head] a contact source's words
  T* slots;
  T* park;                   // [nl][Y.stride]
  int32_t* cnt;              // [nl][SPH_FANOUT] active pairs of a thread's slice
  int32_t *stopf, *itv, *accf, *stat, *rej, *nact;  // [nl] each: stop flag, trial steps, accepted?, status, rejections in a row, curvature pairs
  unsigned char* tail;       // [nl][tail] a contact source's bytes
  T* pk;                     // the frame's region, and its parts:
  const T* cen;
  T *frc, *H, *Hs, *g, *gs, *y, *dg, *xt, *xs, *sc;
  T *rows, *rw;              // [SPH_FANOUT][n_act] staged rows in the place of H, then SPH_FANOUT weights
  uint32_t* lst;             // the frame's active pairs
  unsigned char* fl;         // the frame's pair flags
  int p0, p1;                // thread t owns the pairs [p0, p1) = [t pchunk, (t + 1) pchunk)
};

// head: 64-bit words per frame behind the frozen masks, tail: bytes per frame behind the state words (a contact source's; 0, 0 in
// the plain kernel).  The formula of resolve_lds_bytes.
template <typename T>
__device__ __forceinline__ ResolveLds<T> resolve_lds(unsigned char* lds, int nl, int fr, int t, const ResolveLayout Y, int n_slot, int n_act,
                                                     int n_pair, int fstride, int head, int tail) {
  ResolveLds<T> L;
  L.nl = nl, L.fr = fr, L.t = t;
  L.part = reinterpret_cast<unsigned long long*>(lds);
  L.head = L.part + nl * SPH_FANOUT;
  L.slots = reinterpret_cast<T*>(L.head + nl * head);
  L.park = L.slots + n_slot * 12 * nl;
  uint32_t* lists = reinterpret_cast<uint32_t*>(L.park + nl * Y.stride);  // [nl][DEXR_RESOLVE_MAXACTIVE]
  L.cnt = reinterpret_cast<int32_t*>(lists + nl * DEXR_RESOLVE_MAXACTIVE);
  L.stopf = L.cnt + nl * SPH_FANOUT;
  L.itv = L.stopf + nl;
  L.accf = L.itv + nl;
  L.stat = L.accf + nl;
  L.rej = L.stat + nl;
  L.nact = L.rej + nl;
  L.tail = reinterpret_cast<unsigned char*>(L.nact + nl);
  unsigned char* flags = L.tail + nl * tail;  // [nl][fstride]
  L.pk = L.park + L.fr * Y.stride;
  L.cen = L.pk + Y.cbase;
  L.frc = L.pk + Y.fbase;
  L.H = L.pk + Y.hbase;
  L.Hs = L.pk + Y.hsbase;
  L.g = L.pk + Y.gbase;
  L.gs = L.pk + Y.gsbase;
  L.y = L.pk + Y.ybase;
  L.dg = L.pk + Y.dbase;
  L.xt = L.pk + Y.xbase;
  L.xs = L.pk + Y.xsbase;
  L.sc = L.pk + Y.sbase;
  L.rows = L.H;
  L.rw = L.rows + SPH_FANOUT * n_act;
  L.lst = lists + L.fr * DEXR_RESOLVE_MAXACTIVE;
  L.fl = flags + L.fr * fstride;
  const int pchunk = (n_pair + SPH_FANOUT - 1) / SPH_FANOUT;
  L.p0 = L.t * pchunk < n_pair ? L.t * pchunk : n_pair;
  L.p1 = L.p0 + pchunk < n_pair ? L.p0 + pchunk : n_pair;
  return L;
}

// phase A's share of one link: a target row (the first n_target rows of the caller's list) through ik_link_target, any other
// link its position with weights of 0
template <typename T>
__device__ __forceinline__ T resolve_link(const T R[9], const T p[3], int out, int64_t b, const ResolveArgs<T> A, T* d) {
  if (out < A.n_target) return ik_link_target(R, p, b * A.n_target + out, A.tp, A.tr, A.wl, A.wa, d);
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = p[i];
#pragma unroll
  for (int i = 3; i < IK_LINK; ++i) d[i] = T(0);
  return T(0);
}

// sum over the joints of the active column whose entries are r of mult_k a_k . ((c_s - o_k) x f_s) (revolute) or mult_k a_k . f_s
// (prismatic) over the spheres below joint k: phase C of pose_sphere_kernel
template <typename T>
__device__ __forceinline__ T resolve_force_entry(uint32_t r, const JacEnt* __restrict__ ents, const int32_t* __restrict__ link_sph, const T* pk,
                                                 const T* cen, const T* frc) {
  T g = T(0);
  for (int ii = r & 255; ii < (int)(r >> 8); ++ii) {
    const JacEnt A = ents[ii];
    const T* a = pk + 6 * A.xi;
    const bool rev = A.type == DEXR_POSE_REVOLUTE;
    const int s1 = link_sph[A.sub_end];
    const T ax[3] = {a[0], a[1], a[2]};
    T sl = T(0);
    for (int s = link_sph[A.link_begin]; s < s1; ++s) {
      const T f[3] = {frc[3 * s], frc[3 * s + 1], frc[3 * s + 2]};
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
  return g;
}

// grad d_p in the active column whose entries are r, for the pair of the sorted spheres si (first) and sj with unit normal n:
// n . (Jpt_si - Jpt_sj), each joint of the column counting for the spheres below it
template <typename T>
__device__ __forceinline__ T resolve_row_entry(uint32_t r, const JacEnt* __restrict__ ents, const int32_t* __restrict__ link_sph, const T* pk,
                                               const T* cen, int si, int sj, const T n[3]) {
  T s = T(0);
  for (int ii = r & 255; ii < (int)(r >> 8); ++ii) {
    const JacEnt A = ents[ii];
    const int s0 = link_sph[A.link_begin], s1 = link_sph[A.sub_end];
    const bool ini = si >= s0 && si < s1, inj = sj >= s0 && sj < s1;
    if (!ini && !inj) continue;
    const T* a = pk + 6 * A.xi;
    const bool rev = A.type == DEXR_POSE_REVOLUTE;
    T v[3] = {T(0), T(0), T(0)}, c[3];
    if (ini) {
      ik_column(a, rev, cen + 3 * si, c);
#pragma unroll
      for (int i = 0; i < 3; ++i) v[i] = c[i];
    }
    if (inj) {
      ik_column(a, rev, cen + 3 * sj, c);
#pragma unroll
      for (int i = 0; i < 3; ++i) v[i] -= c[i];
    }
    s = fma(mult_of(A, T(0)), dot_fma(n, v), s);
  }
  return s;
}

// ---- the phases, each once --------------------------------------------------------------------------------------------------
// the start of a frame (row: its index in the batch): x0 into the trial and the accepted point, the state words, lam
template <typename T>
__device__ __forceinline__ void resolve_start(const ResolveLds<T>& L, const ResolveArgs<T> A, int n_in, int64_t row, bool inb) {
  for (int c = L.t; c < n_in; c += SPH_FANOUT) {
    const T v = inb ? A.x0[row * n_in + c] : T(0);
    L.xt[c] = v;
    L.xs[c] = v;
  }
  L.part[L.fr * SPH_FANOUT + L.t] = 0;
  if (L.t == 0) {
    L.stopf[L.fr] = inb ? 0 : 1;  // idle lanes of a ragged last block never start
    L.itv[L.fr] = L.accf[L.fr] = L.stat[L.fr] = L.rej[L.fr] = L.nact[L.fr] = 0;
    for (int i = 0; i < RSV_SCALARS; ++i) L.sc[i] = T(0);
    L.sc[RSV_LAM] = A.damping;
  }
}

// phase A, lane = frame: the walk at the trial, E_pose and E_post
template <typename T>
__device__ __forceinline__ void resolve_walk(const ResolveLds<T>& L, const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                             const SphereD<T>* __restrict__ spheres, const SphereIndex& S, const PoseArgs<T>& P,
                                             const ResolveLayout Y, const ResolveArgs<T> A, int lane, int64_t first) {
  const bool targets = A.n_target > 0;
  PoseArgs<T> PL = P;  // the walk's view of x: the frames' trial rows in LDS
  PL.n_in = Y.stride;
  const T* xl = L.park + Y.xbase;
  const T* fixl = A.fixed + first * P.n_fixed;
  T* pa = L.park + lane * Y.stride;
  T* ca = pa + Y.cbase;
  const int64_t b = first + lane;
  T Ep = T(0);
  for (int l = 0; l < P.n_base; ++l) {  // links on the fixed base: below no joint, but their error and their spheres count
    const LinkD<T>& K = links[l];
    if (targets) Ep += resolve_link(K.R, K.p, K.out, b, A, pa + Y.lbase + IK_LINK * l);
    for (int s = S.link_sph[l]; s < S.link_sph[l + 1]; ++s) sphere_centre(K.R, K.p, spheres[s], ca + 3 * s);
  }
  Xf<T> tf;
#pragma unroll
  for (int i = 0; i < 9; ++i) tf.R[i] = (i % 4 == 0) ? T(1) : T(0);
  tf.p[0] = tf.p[1] = tf.p[2] = T(0);
  int xi = 0;
  for (int j = 0; j < P.n_joint; ++j) {
    const JointD<T>& J = joints[j];
    T a[3];
    joint_step(J, PL, xl, fixl, (int64_t)lane, L.slots, L.nl, lane, tf, a);
    if (J.src_kind == DEXR_POSE_SRC_X) {
      T* d = pa + 6 * xi;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        d[i] = a[i];
        d[3 + i] = tf.p[i];
      }
      ++xi;
    }
    for (int l = J.link_begin; l < J.link_end; ++l) {
      const int s0 = S.link_sph[l], s1 = S.link_sph[l + 1];
      if (!targets && s0 == s1) continue;
      const LinkD<T>& K = links[l];
      T R[9], p[3];
      link_pose(K, tf, R, p);
      if (targets) Ep += resolve_link(R, p, K.out, b, A, pa + Y.lbase + IK_LINK * l);
      for (int s = s0; s < s1; ++s) sphere_centre(R, p, spheres[s], ca + 3 * s);
    }
  }
  T Eq = T(0);
  if (A.u) {
    const T* xa = pa + Y.xbase;
    const T* ra = A.xref + b * P.n_in;
    for (int c = 0; c < P.n_in; ++c) {
      const T d = xa[c] - ra[c];
      Eq = fma(A.u[c] * d, d, Eq);
    }
  }
  pa[Y.sbase + RSV_TPOSE] = Ep;
  pa[Y.sbase + RSV_TPOST] = Eq;
}

// phase B, the pairs of the sorted sphere s at cs: its force with g_p = w_p h_p (g = -1/2 grad E) into f, the energies of the
// pairs it is the first end of onto e, and those pairs' active flags
template <typename T>
__device__ __forceinline__ void resolve_pair_forces(const ResolveLds<T>& L, const ResolveModel<T>& M, const ResolveArgs<T> A, int s,
                                                    const T cs[3], T& e, T f[3]) {
  T f0 = T(0), f1 = T(0), f2 = T(0);
  const int i1 = M.S.inc_ptr[s + 1];
  for (int i = M.S.inc_ptr[s]; i < i1; ++i) {
    const uint32_t u = M.S.inc[i];
    const int o = u & 127, p = u >> 8;
    const T d0 = cs[0] - L.cen[3 * o], d1 = cs[1] - L.cen[3 * o + 1], d2 = cs[2] - L.cen[3 * o + 2];
    const T sp = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)));
    T h = A.margin - (sp - M.rsum[p]);
    if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
    const T wh = A.pw ? A.pw[p] * h : h;
    if (u & SPH_FIRST) {
      e = fma(wh, h, e);
      L.fl[p] = h > T(0) ? 1 : 0;
    }
    const T q = sp > T(0) ? wh / sp : wh * (sp * T(0));  // coincident centres: no direction
    f0 = fma(q, d0, f0);
    f1 = fma(q, d1, f1);
    f2 = fma(q, d2, f2);
  }
  f[0] = f0, f[1] = f1, f[2] = f2;
}

// sixteen partial energies, added in order
template <typename T>
__device__ __forceinline__ T resolve_sum16(const T* pe) {
  T E = pe[0];
  for (int i = 1; i < SPH_FANOUT; ++i) E += pe[i];
  return E;
}

// phase C, every thread: the active pairs of its slice
template <typename T>
__device__ __forceinline__ void resolve_count_pairs(const ResolveLds<T>& L) {
  int n = 0;
  for (int p = L.p0; p < L.p1; ++p) n += L.fl[p];
  L.cnt[L.fr * SPH_FANOUT + L.t] = n;
}

// phase C, thread 0 of a frame: the accept / reject decision on the trial's weighted terms Ec (and Eo with OBS); it moves the
// accepted point, lam, the reject count, the status and the stop flag
template <bool OBS, typename T>
__device__ __forceinline__ void resolve_decide(const ResolveLds<T>& L, const ResolveModel<T>& M, const ResolveArgs<T> A, int k, T Ec, T Eo) {
  const int fr = L.fr;
  T* sc = L.sc;
  T Et = (sc[RSV_TPOSE] + sc[RSV_TPOST]) + Ec;
  if constexpr (OBS) Et = Et + Eo;
  const bool acc = k == 0 || Et <= sc[RSV_E];  // (a comparison: a NaN rejects)
  int st = L.stat[fr];
  bool stop = false;
  if (acc) {
    T step = T(0);
    for (int i = 0; i < M.n_act; ++i) {
      const int c = M.act_col[i];
      const T d = fabs(L.xt[c] - L.xs[c]);
      step = d > step ? d : step;
      L.xs[c] = L.xt[c];
    }
    sc[RSV_E] = Et;
    sc[RSV_POSE] = sc[RSV_TPOSE];
    sc[RSV_POST] = sc[RSV_TPOST];
    sc[RSV_COL] = Ec;
    if constexpr (OBS) sc[RSV_OBS] = Eo;
    if (k > 0) {
      const T l = sc[RSV_LAM] / T(DEXR_RESOLVE_LAM_DOWN);
      sc[RSV_LAM] = l > A.damping ? l : A.damping;
      L.rej[fr] = 0;
      if (step <= A.tol) {
        st |= DEXR_RESOLVE_CONVERGED;
        stop = true;
      }
    }
  } else {
    sc[RSV_LAM] *= T(DEXR_RESOLVE_LAM_UP);
    if (++L.rej[fr] == DEXR_RESOLVE_MAXREJECT) {
      st |= DEXR_RESOLVE_STALLED;
      stop = true;
    }
  }
  L.itv[fr] = k;
  L.accf[fr] = acc ? 1 : 0;
  L.stat[fr] = st;
  if (stop || k == A.max_iters) L.stopf[fr] = 1;
}

// after the decision, thread 0 of a frame: the pairs of the curvature, capped (stat of a frame is its thread 0's alone until the
// next barrier)
template <typename T>
__device__ __forceinline__ int resolve_pair_total(const ResolveLds<T>& L) {
  int total = 0;
  for (int u = 0; u < SPH_FANOUT; ++u) total += L.cnt[L.fr * SPH_FANOUT + u];
  if (total > DEXR_RESOLVE_MAXACTIVE) {
    L.stat[L.fr] |= DEXR_RESOLVE_TRUNCATED;
    total = DEXR_RESOLVE_MAXACTIVE;
  }
  return total;
}

// the block's vote, the same in every thread
template <typename T>
__device__ __forceinline__ bool resolve_all_stopped(const ResolveLds<T>& L) {
  bool all = true;
  for (int f = 0; f < L.nl; ++f) all = all && L.stopf[f] != 0;
  return all;
}

// phase D: the active list in pair-index order, by a prefix over the sixteen counts
template <typename T>
__device__ __forceinline__ void resolve_list_pairs(const ResolveLds<T>& L) {
  int off = 0;
  for (int u = 0; u < L.t; ++u) off += L.cnt[L.fr * SPH_FANOUT + u];
  for (int p = L.p0; p < L.p1 && off < DEXR_RESOLVE_MAXACTIVE; ++p)
    if (L.fl[p]) L.lst[off++] = (uint32_t)p;
}

// phase D: g of the accepted point with the freeze test of its columns, and the thread's partial frozen mask.  OBS: the forces
// carry w_col and w_obs already
template <bool OBS, typename T>
__device__ __forceinline__ void resolve_gradient(const ResolveLds<T>& L, const ResolveModel<T>& M, const ResolveLayout Y, const ResolveArgs<T> A,
                                                 const T* xr) {
  const bool targets = A.n_target > 0;
  unsigned long long mine = 0;
  for (int i = L.t; i < M.n_act; i += SPH_FANOUT) {
    const int c = M.act_col[i];
    const uint32_t r = M.act_rng[i];
    T s = targets ? ik_g_entry(r, M.ents, L.pk, Y.lbase) : T(0);
    if (A.u) s = fma(A.u[c], xr[c] - L.xs[c], s);
    if constexpr (OBS)
      s += resolve_force_entry(r, M.ents, M.S.link_sph, L.pk, L.cen, L.frc);
    else
      s = fma(A.wcol, resolve_force_entry(r, M.ents, M.S.link_sph, L.pk, L.cen, L.frc), s);
    if (A.lo) {
      const T xc = L.xs[c];
      if ((xc <= A.lo[c] && s < T(0)) || (xc >= A.hi[c] && s > T(0))) {
        mine |= 1ull << i;
        s = T(0);
      }
    }
    L.gs[i] = s;
  }
  L.part[L.fr * SPH_FANOUT + L.t] = mine;
}

// the frozen columns of the last accepted point: a frame that rejected keeps its partial masks
template <typename T>
__device__ __forceinline__ unsigned long long resolve_frozen(const ResolveLds<T>& L) {
  unsigned long long frozen = 0;
  for (int u = 0; u < SPH_FANOUT; ++u) frozen |= L.part[L.fr * SPH_FANOUT + u];
  return frozen;
}

// phase D: H without damping and curvature; a frozen column's row and column of H are the identity's
template <typename T>
__device__ __forceinline__ void resolve_base_h(const ResolveLds<T>& L, const ResolveModel<T>& M, const ResolveLayout Y, const ResolveArgs<T> A,
                                               unsigned long long frozen) {
  const bool targets = A.n_target > 0;
  for (int e = L.t; e < M.n_tri; e += SPH_FANOUT) {
    const uint2 d = M.tri[e];
    const int i = d.x & 63, j = d.x >> 6;
    T h;
    if (((frozen >> i) | (frozen >> j)) & 1ull) {
      h = i == j ? T(1) : T(0);
    } else {
      h = targets ? ik_h_entry(d, M.ents, L.pk, Y.lbase) : T(0);
      if (i == j && A.u) h += A.u[M.act_col[i]];
    }
    L.Hs[e] = h;
  }
}

// what the q-th active pair gives the curvature: its sorted spheres, its unit normal (none between coincident centres), its weight
template <typename T>
__device__ __forceinline__ void resolve_pair_contact(const ResolveLds<T>& L, const ResolveModel<T>& M, const ResolveArgs<T> A, int q, int& si,
                                                     int& sj, T n[3], T& w) {
  const uint32_t p = L.lst[q], ps = M.pair_sph[p];
  si = ps & 127, sj = (ps >> 7) & 127;
  const T* cen = L.cen;
  const T d[3] = {cen[3 * si] - cen[3 * sj], cen[3 * si + 1] - cen[3 * sj + 1], cen[3 * si + 2] - cen[3 * sj + 2]};
  const T sp = sqrt(fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])));
  const T inv = sp > T(0) ? T(1) / sp : T(0);
#pragma unroll
  for (int i = 0; i < 3; ++i) n[i] = d[i] * inv;
  w = A.pw ? A.wcol * A.pw[p] : A.wcol;
}

// thread t stages row t of a rank-16 chunk: grad d over the active columns (0 in a frozen one) for the spheres si and sj (-1: one
// sphere alone, no link holds sphere -1) with normal n, and the row's weight
template <typename T>
__device__ __forceinline__ void resolve_stage_row(const ResolveLds<T>& L, const ResolveModel<T>& M, unsigned long long frozen, int si, int sj,
                                                  const T n[3], T w) {
  T* row = L.rows + L.t * M.n_act;
  for (int i = 0; i < M.n_act; ++i)
    row[i] = ((frozen >> i) & 1ull) ? T(0) : resolve_row_entry(M.act_rng[i], M.ents, M.S.link_sph, L.pk, L.cen, si, sj, n);
  L.rw[L.t] = w;
}

// Hs += sum over the nk staged rows of w_q row_q row_q^T, every entry by one thread in row order
template <typename T>
__device__ __forceinline__ void resolve_rank16(const ResolveLds<T>& L, const ResolveModel<T>& M, int nk) {
  for (int e = L.t; e < M.n_tri; e += SPH_FANOUT) {
    const uint2 dd = M.tri[e];
    const int i = dd.x & 63, j = dd.x >> 6;
    T h = L.Hs[e];
    for (int q = 0; q < nk; ++q) h = fma(L.rw[q] * L.rows[q * M.n_act + i], L.rows[q * M.n_act + j], h);
    L.Hs[e] = h;
  }
}

// phase E, before ik_factor_solve: the kept system with the frame's lam
template <typename T>
__device__ __forceinline__ void resolve_damp(const ResolveLds<T>& L, const ResolveModel<T>& M, unsigned long long frozen) {
  const T lam = L.sc[RSV_LAM];
  for (int e = L.t; e < M.n_tri; e += SPH_FANOUT) {
    const uint2 d = M.tri[e];
    const int i = d.x & 63, j = d.x >> 6;
    L.H[e] = (i == j && !((frozen >> i) & 1ull)) ? L.Hs[e] + lam : L.Hs[e];
  }
  for (int i = L.t; i < M.n_act; i += SPH_FANOUT) L.g[i] = L.gs[i];
}

// phase E, after it: limit the step, move, clamp -- by comparisons, a NaN stays a NaN
template <typename T>
__device__ __forceinline__ void resolve_step(const ResolveLds<T>& L, const ResolveModel<T>& M, const ResolveArgs<T> A) {
  T scale = T(1);
  if (A.max_step > T(0)) {
    T m = T(0);
    for (int i = 0; i < M.n_act; ++i) {
      const T a = fabs(L.g[i]);
      m = a > m ? a : m;
    }
    if (m > A.max_step) scale = A.max_step / m;
  }
  for (int i = L.t; i < M.n_act; i += SPH_FANOUT) {
    const int c = M.act_col[i];
    T v = L.xs[c] + L.g[i] * scale;
    if (A.lo) {
      const T l = A.lo[c], h = A.hi[c];
      v = v < l ? l : (v > h ? h : v);
    }
    L.xt[c] = v;
  }
}

// what a frame of the batch reports: the accepted point, and by its thread 0 iters, status and the first ecols terms of E
template <typename T>
__device__ __forceinline__ void resolve_output(const ResolveLds<T>& L, const ResolveArgs<T> A, int n_in, int64_t row, int ecols) {
  T* o = A.x_out + row * n_in;
  for (int c = L.t; c < n_in; c += SPH_FANOUT) o[c] = L.xs[c];
  if (L.t == 0) {
    if (A.iters_out) A.iters_out[row] = L.itv[L.fr];
    if (A.status_out) A.status_out[row] = L.stat[L.fr];
    if (A.e_out) {
      T* eo = A.e_out + row * ecols;
      eo[0] = L.sc[RSV_POSE];
      eo[1] = L.sc[RSV_POST];
      eo[2] = L.sc[RSV_COL];
      if (ecols > 3) eo[3] = L.sc[RSV_OBS];
    }
  }
}

// THE LOOP CANNOT HANG (here and in resolve_contact_loop, which has the same skeleton): it runs k = 0 .. max_iters at most; every
// barrier sits outside every condition that differs between the threads of a block (the number of rank-16 chunks is the block's
// largest, read by every thread from LDS after a barrier); a frame that has stopped (or an idle lane of a ragged last block:
// stopped from the start) does no work and writes nothing but walks through the same barriers; the one early exit is taken on
// the AND of all stop flags, and at k == max_iters every flag is set.  Every sum is taken by one thread in table order: a
// frame's bits do not depend on the batch or on its neighbours.
template <typename T>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES) pose_resolve_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                              PoseArgs<T> P, const SphereD<T>* __restrict__ spheres,
                                                                              const T* __restrict__ rsum, SphereIndex S,
                                                                              const uint32_t* __restrict__ pair_sph,
                                                                              const JacEnt* __restrict__ ents, const uint32_t* __restrict__ act_rng,
                                                                              const int32_t* __restrict__ act_col, const uint2* __restrict__ tri,
                                                                              int n_jx, int n_act, ResolveLayout Y, int fstride, ResolveArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  const ResolveModel<T> M = {joints, links, spheres, rsum, S, pair_sph, ents, act_rng, act_col, tri, n_act, n_act * (n_act + 1) / 2};
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  const ResolveLds<T> L = resolve_lds<T>(pose_lds, nl, fr, t, Y, P.n_slot, n_act, S.n_pair, fstride, 0, 0);
  const int64_t first = (int64_t)blockIdx.x * nl;
  const bool inb = first + fr < P.B;
  const T* xr = A.xref + (inb ? first + fr : 0) * P.n_in;  // (read by working frames alone)
  resolve_start(L, A, P.n_in, first + fr, inb);
  __syncthreads();
  for (int k = 0; k <= A.max_iters; ++k) {
    if (tid < nl && L.stopf[tid] == 0) resolve_walk(L, joints, links, spheres, S, P, Y, A, tid, first);  // phase A
    __syncthreads();
    const bool work = L.stopf[fr] == 0;
    if (work) {  // phase B: a thread per sphere; forces, energies, active flags
      T e = T(0);
      for (int s = t; s < S.n_sphere; s += SPH_FANOUT) {
        const T cs[3] = {L.cen[3 * s], L.cen[3 * s + 1], L.cen[3 * s + 2]};
        T f[3];
        resolve_pair_forces(L, M, A, s, cs, e, f);
        L.frc[3 * s] = f[0];
        L.frc[3 * s + 1] = f[1];
        L.frc[3 * s + 2] = f[2];
      }
      L.pk[Y.pebase + t] = e;
    }
    __syncthreads();
    if (work) {  // phase C: the counts of the active list, and the decision
      resolve_count_pairs(L);
      if (t == 0) resolve_decide<false>(L, M, A, k, resolve_sum16(L.pk + Y.pebase) * A.wcol, T(0));
    }
    __syncthreads();
    if (work && t == 0) {
      const int total = resolve_pair_total(L);
      L.nact[fr] = (L.accf[fr] != 0 && L.stopf[fr] == 0) ? total : 0;
    }
    if (resolve_all_stopped(L)) break;
    const bool go = L.stopf[fr] == 0;          // the frame goes on: it needs a next trial
    const bool build = go && L.accf[fr] != 0;  // ... from a new point: its list, g and H are formed and kept
    if (build) {  // phase D
      resolve_list_pairs(L);
      resolve_gradient<false>(L, M, Y, A, xr);
    }
    __syncthreads();
    const unsigned long long frozen = resolve_frozen(L);
    if (build) resolve_base_h(L, M, Y, A, frozen);
    int nmax = 0;  // the block's largest list: the same in every thread
    for (int f = 0; f < nl; ++f) nmax = L.nact[f] > nmax ? L.nact[f] : nmax;
    const int mine_n = L.nact[fr];  // (0 unless `build`)
    for (int base = 0; base < nmax; base += SPH_FANOUT) {  // the pair curvature, sixteen rows grad d_p at a time
      if (base + t < mine_n) {
        T n[3], w;
        int si, sj;
        resolve_pair_contact(L, M, A, base + t, si, sj, n, w);
        resolve_stage_row(L, M, frozen, si, sj, n, w);
      }
      __syncthreads();
      const int nk = mine_n - base < SPH_FANOUT ? mine_n - base : SPH_FANOUT;
      if (nk > 0) resolve_rank16(L, M, nk);
      __syncthreads();
    }
    if (go) resolve_damp(L, M, frozen);  // phase E
    __syncthreads();
    ik_factor_solve(L.H, L.g, L.y, L.dg, n_act, t, go);
    if (go) resolve_step(L, M, A);
    __syncthreads();
  }
  if (inb) resolve_output(L, A, P.n_in, first + fr, 3);
}

template <typename T>
ResolveLayout resolve_layout(const dexr_sphere_model* sm, int n_target) {
  const dexr_pose_model* m = sm->pose;
  const int n_act = m->n_act, n_tri = n_act * (n_act + 1) / 2, staged = SPH_FANOUT * n_act + SPH_FANOUT;
  ResolveLayout Y;
  int o = 6 * m->n_jx;
  Y.lbase = o, o += n_target > 0 ? IK_LINK * m->h.n_link : 0;
  Y.cbase = o, o += 3 * sm->n_sphere;
  Y.fbase = o, o += 3 * sm->n_sphere;
  Y.pebase = o, o += SPH_FANOUT;
  Y.hbase = o, o += n_tri > staged ? n_tri : staged;
  Y.hsbase = o, o += n_tri;
  Y.gbase = o, o += n_act;
  Y.gsbase = o, o += n_act;
  Y.ybase = o, o += n_act;
  Y.dbase = o, o += n_act;
  Y.xbase = o, o += m->h.n_in;
  Y.xsbase = o, o += m->h.n_in;
  Y.sbase = o, o += RSV_SCALARS;
  Y.stride = o | 1;  // odd, so that the frames of a wave start in different banks
  return Y;
}

// the argument rules of both entry points: < 0 error, 1 nothing to do, 0 go on
int check_resolve_call(const dexr_sphere_model* sm, int64_t B, const void* x0, const void* fixed, int32_t n_target, const void* tp, const void* tr,
                       const void* wl, const void* wa, double margin, double wcol, const void* lo, const void* hi, double damping, double max_step,
                       double tol, int32_t max_iters, const void* x_out) {
  const double big = 1.7976931348623157e308;
  if (!sm) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (B < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative batch size");
  if (check_margin(margin)) return DEXR_ERR_INVALID;
  if (!(wcol >= 0.0) || wcol > big) return dexr_set_error(DEXR_ERR_INVALID, "collision_weight must be finite and >= 0, got %g", wcol);
  if (!(damping > 0.0) || damping > big) return dexr_set_error(DEXR_ERR_INVALID, "damping must be finite and > 0, got %g", damping);
  if (!(max_step >= 0.0) || max_step > big) return dexr_set_error(DEXR_ERR_INVALID, "max_step must be finite and >= 0 (0: no limit), got %g", max_step);
  if (!(tol >= 0.0) || tol > big) return dexr_set_error(DEXR_ERR_INVALID, "tol must be finite and >= 0, got %g", tol);
  if (max_iters < 1 || max_iters > 256) return dexr_set_error(DEXR_ERR_INVALID, "max_iters must be in 1..256, got %d", max_iters);
  if ((lo == nullptr) != (hi == nullptr)) return dexr_set_error(DEXR_ERR_INVALID, "lo and hi must both be given or both be NULL");
  if (n_target < 0 || n_target > sm->pose->h.n_link)
    return dexr_set_error(DEXR_ERR_INVALID, "n_target must be in 0..%d (the links of the model), got %d", sm->pose->h.n_link, n_target);
  if (B == 0) return 1;
  if (n_target > 0 && !tp && !tr) return dexr_set_error(DEXR_ERR_INVALID, "n_target is %d but target_pos and target_rot are both NULL", n_target);
  if (n_target == 0 && (tp || tr || wl || wa))
    return dexr_set_error(DEXR_ERR_INVALID, "n_target is 0 but target_pos, target_rot, pos_weight or rot_weight is given");
  if (wl && !tp) return dexr_set_error(DEXR_ERR_INVALID, "pos_weight given without target_pos");
  if (wa && !tr) return dexr_set_error(DEXR_ERR_INVALID, "rot_weight given without target_rot");
  if (!x_out) return dexr_set_error(DEXR_ERR_INVALID, "x_out is NULL");
  if (!x0 && sm->pose->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "x0 is NULL");
  return check_call(sm->pose, B, x0, fixed);
}

// LDS bytes of one frame for the layout Y: the formula of include/dexr_resolve.h, and with a contact source's head words and tail
// bytes those of include/dexr_resolve_obstacles.h and include/dexr_resolve_grid.h (resolve_lds places the same parts)
template <typename T>
size_t resolve_lds_bytes(const dexr_sphere_model* sm, const ResolveLayout Y, size_t head, size_t tail) {
  return SPH_FANOUT * sizeof(unsigned long long) + head * sizeof(unsigned long long) +
         ((size_t)sm->pose->h.n_slot * 12 + (size_t)Y.stride) * sizeof(T) + (DEXR_RESOLVE_MAXACTIVE + SPH_FANOUT + 6) * sizeof(int32_t) + tail +
         (size_t)((sm->n_pair + 3) & ~3);
}

// the launch shape of B frames of per_frame bytes of LDS each: the frames of a block (halved until they fit; the largest model in
// float64: one frame) and the blocks
int resolve_launch_shape(size_t per_frame, int64_t B, int* nl_out, int64_t* blocks_out) {
  int nl = SPH_FRAMES;
  while (nl > 1 && per_frame * nl > 64 * 1024) nl /= 2;
  if (per_frame * nl > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the sphere model needs %zu B of LDS per frame: one frame does not fit a block", per_frame);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  *nl_out = nl, *blocks_out = blocks;
  return DEXR_OK;
}

template <typename T>
int launch_resolve(const dexr_sphere_model* sm, int64_t B, ResolveArgs<T> A, hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  const ResolveLayout Y = resolve_layout<T>(sm, A.n_target);
  const size_t per_frame = resolve_lds_bytes<T>(sm, Y, 0, 0);
  int nl;
  int64_t blocks;
  if (const int rc = resolve_launch_shape(per_frame, B, &nl, &blocks)) return rc;
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  if (!A.xref) A.xref = A.x0;
  hipLaunchKernelGGL(pose_resolve_kernel<T>, dim3((unsigned)blocks), dim3(nl * SPH_FANOUT), per_frame * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), (const SphereD<T>*)sphere_tables_of<T>(sm).spheres,
                     (const T*)sphere_tables_of<T>(sm).rsum, S, (const uint32_t*)sm->pair_sph, (const JacEnt*)m->jac_ents,
                     (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col, (const uint2*)m->ik_tri, m->n_jx, m->n_act, Y,
                     (sm->n_pair + 3) & ~3, A);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "collision resolve kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// The float64 entry points' round trip through the device: `up` uploads what all three take; after the caller's own uploads `out`
// allocates the four outputs (energy: ecols columns) and gives the ResolveArgs over all of them; after the launch `down` waits
// and copies back the outputs the caller wants.  The buffers live as long as the object.
struct ResolveRoundTrip {
  DevBuf dx, dfix, dref, du, dp, dr, dwl, dwa, dpw, dlo, dhi, dout, dit, den, dst;
  size_t nx = 0, ni = 0, ne = 0;

  int up(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref, const double* posture_weight,
         int32_t n_target, const double* target_pos, const double* target_rot, const double* pos_weight, const double* rot_weight,
         const double* pair_weight, const double* lo, const double* hi) {
    const dexr_pose_model* pm = m->pose;
    const size_t nf = (size_t)B * pm->h.n_fixed * sizeof(double), nw = (size_t)B * n_target * sizeof(double);
    const size_t nb = (size_t)pm->h.n_in * sizeof(double);
    nx = (size_t)B * pm->h.n_in * sizeof(double);
    POSE_HIP(dx.put(x0, nx));
    POSE_HIP(dfix.put(fixed, nf));
    if (x_ref) POSE_HIP(dref.put(x_ref, nx));
    if (posture_weight) POSE_HIP(du.put(posture_weight, nb));
    if (target_pos) POSE_HIP(dp.put(target_pos, 3 * nw));
    if (target_rot) POSE_HIP(dr.put(target_rot, 9 * nw));
    if (pos_weight) POSE_HIP(dwl.put(pos_weight, nw));
    if (rot_weight) POSE_HIP(dwa.put(rot_weight, nw));
    if (pair_weight) POSE_HIP(dpw.put(pair_weight, (size_t)m->n_pair * sizeof(double)));
    if (lo) POSE_HIP(dlo.put(lo, nb));
    if (hi) POSE_HIP(dhi.put(hi, nb));
    return DEXR_OK;
  }

  int out(int64_t B, int ecols, double margin, double collision_weight, double damping, double max_step, double tol, int32_t n_target,
          int32_t max_iters, ResolveArgs<double>* A) {
    ni = (size_t)B * sizeof(int32_t), ne = (size_t)B * ecols * sizeof(double);
    POSE_HIP(dout.put(nullptr, nx));
    POSE_HIP(dit.put(nullptr, ni));
    POSE_HIP(den.put(nullptr, ne));
    POSE_HIP(dst.put(nullptr, ni));
    *A = {(const double*)dx.p,  (const double*)dfix.p, (const double*)dref.p, (const double*)du.p,  (const double*)dp.p,
          (const double*)dr.p,  (const double*)dwl.p,  (const double*)dwa.p,  (const double*)dpw.p, (const double*)dlo.p,
          (const double*)dhi.p, margin,                collision_weight,      damping,              max_step,
          tol,                  n_target,              max_iters,             (double*)dout.p,      (int32_t*)dit.p,
          (double*)den.p,       (int32_t*)dst.p};
    return DEXR_OK;
  }

  int down(double* x_out, int32_t* iters_out, double* energy_out, int32_t* status_out) {
    POSE_HIP(hipDeviceSynchronize());
    if (nx) POSE_HIP(hipMemcpy(x_out, dout.p, nx, hipMemcpyDeviceToHost));
    if (iters_out) POSE_HIP(hipMemcpy(iters_out, dit.p, ni, hipMemcpyDeviceToHost));
    if (energy_out) POSE_HIP(hipMemcpy(energy_out, den.p, ne, hipMemcpyDeviceToHost));
    if (status_out) POSE_HIP(hipMemcpy(status_out, dst.p, ni, hipMemcpyDeviceToHost));
    return DEXR_OK;
  }
};

}  // namespace

extern "C" {

int dexr_sphere_resolve_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                            const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                            const float* pos_weight, const float* rot_weight, float margin, float collision_weight, const float* pair_weight,
                            const float* lo, const float* hi, float damping, float max_step, float tol, int32_t max_iters, float* x_out,
                            int32_t* iters_out, float* energy_out, int32_t* status_out, void* stream) {
  const int c = check_resolve_call(m, B, x0, fixed, n_target, target_pos, target_rot, pos_weight, rot_weight, (double)margin,
                                   (double)collision_weight, lo, hi, (double)damping, (double)max_step, (double)tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const ResolveArgs<float> A = {x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi,
                                margin, collision_weight, damping, max_step, tol, n_target, max_iters, x_out, iters_out, energy_out, status_out};
  return launch_resolve<float>(m, B, A, (hipStream_t)stream);
}

int dexr_sphere_resolve(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                        const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                        const double* pos_weight, const double* rot_weight, double margin, double collision_weight, const double* pair_weight,
                        const double* lo, const double* hi, double damping, double max_step, double tol, int32_t max_iters, double* x_out,
                        int32_t* iters_out, double* energy_out, int32_t* status_out) {
  const int c = check_resolve_call(m, B, x0, fixed, n_target, target_pos, target_rot, pos_weight, rot_weight, margin, collision_weight, lo, hi,
                                   damping, max_step, tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  ResolveRoundTrip D;
  ResolveArgs<double> A;
  if (const int rc = D.up(m, B, x0, fixed, x_ref, posture_weight, n_target, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi))
    return rc;
  if (const int rc = D.out(B, 3, margin, collision_weight, damping, max_step, tol, n_target, max_iters, &A)) return rc;
  if (const int rc = launch_resolve<double>(m, B, A, nullptr)) return rc;
  return D.down(x_out, iters_out, energy_out, status_out);
}

}  // extern "C"

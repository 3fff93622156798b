// dexr_resolve.hpp -- the collision-aware posture solve (include/dexr_resolve.h): a fragment of dexr_pose.hip, which includes it
// once after dexr_spheres.hpp.  pose_resolve_kernel<T> is the resident loop of pose_ik_solve_kernel with the phases of
// pose_sphere_kernel inside it, an accept / reject rule and a per-frame damping.
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
//
// THE LOOP CANNOT HANG: it runs k = 0 .. max_iters at most; every barrier sits outside every condition that differs between the
// threads of a block (the number of rank-16 chunks is the block's largest, read by every thread from LDS after a barrier); a frame
// that has stopped (or an idle lane of a ragged last block: stopped from the start) does no work and writes nothing but walks
// through the same barriers; the one early exit is taken on the AND of all stop flags, and at k == max_iters every flag is set.
// Every sum is taken by one thread in table order: a frame's bits do not depend on the batch or on its neighbours.
//
// LDS of a block: sixteen 64-bit partial frozen masks per frame | the fork slots | per frame a region [frame][stride], odd stride
// (ResolveLayout) | per frame the active list (DEXR_RESOLVE_MAXACTIVE pair indices), sixteen counts, six words of state | per
// frame one byte per pair.  The staged rows of the curvature share the place of the working copy of H, which is formed after them.
#include "dexr_resolve.h"

// 1: form the pair curvature entry by entry from the active list instead of the staged rank-16 update (a developer build for
// tools/resolve_probe.py; docs/experiments/collision_resolve.md has the two timings)
#ifndef DEXR_RESOLVE_CURVATURE_WALK
#define DEXR_RESOLVE_CURVATURE_WALK 0
#endif

namespace {

constexpr int RSV_E = 0, RSV_LAM = 1, RSV_TPOSE = 2, RSV_TPOST = 3, RSV_POSE = 4, RSV_POST = 5, RSV_COL = 6, RSV_SCALARS = 8;

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

// phase A's share of one link: a target row (the first n_target rows of the caller's list) through ik_link_target, any other
// link its position with weights of 0
template <typename T>
__device__ __forceinline__ T resolve_link(const T R[9], const T p[3], int out, int64_t b, const ResolveArgs<T>& A, T* d) {
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
  unsigned long long* part = reinterpret_cast<unsigned long long*>(pose_lds);  // [nl][SPH_FANOUT]
  T* slots = reinterpret_cast<T*>(part + nl * SPH_FANOUT);
  T* park = slots + (size_t)P.n_slot * 12 * nl;
  uint32_t* lists = reinterpret_cast<uint32_t*>(park + (size_t)nl * Y.stride);  // [nl][DEXR_RESOLVE_MAXACTIVE]
  int32_t* cnt = reinterpret_cast<int32_t*>(lists + nl * DEXR_RESOLVE_MAXACTIVE);  // [nl][SPH_FANOUT]
  int32_t* stopf = cnt + nl * SPH_FANOUT;  // [nl] each: stop flag, trial steps, accepted?, status, rejections in a row, curvature pairs
  int32_t* itv = stopf + nl;
  int32_t* accf = itv + nl;
  int32_t* stat = accf + nl;
  int32_t* rej = stat + nl;
  int32_t* nact = rej + nl;
  unsigned char* flags = reinterpret_cast<unsigned char*>(nact + nl);  // [nl][fstride]
  const int n_tri = n_act * (n_act + 1) / 2;
  const bool targets = A.n_target > 0;
  const int64_t first = (int64_t)blockIdx.x * nl;
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  const bool inb = first + fr < P.B;
  T* pk = park + (size_t)fr * Y.stride;
  const T* cen = pk + Y.cbase;
  T* frc = pk + Y.fbase;
  T* H = pk + Y.hbase;
  T* Hs = pk + Y.hsbase;
  T* g = pk + Y.gbase;
  T* gs = pk + Y.gsbase;
  T* y = pk + Y.ybase;
  T* dg = pk + Y.dbase;
  T* xt = pk + Y.xbase;
  T* xs = pk + Y.xsbase;
  T* sc = pk + Y.sbase;
  T* rows = H;  // [SPH_FANOUT][n_act], then SPH_FANOUT weights
  T* rw = rows + SPH_FANOUT * n_act;
  uint32_t* lst = lists + fr * DEXR_RESOLVE_MAXACTIVE;
  unsigned char* fl = flags + (size_t)fr * fstride;
  const T* xr = A.xref + (inb ? first + fr : 0) * P.n_in;  // (read by working frames alone)
  const int pchunk = (S.n_pair + SPH_FANOUT - 1) / SPH_FANOUT;  // thread t owns the pairs [t pchunk, (t + 1) pchunk)
  const int p0 = t * pchunk < S.n_pair ? t * pchunk : S.n_pair, p1 = p0 + pchunk < S.n_pair ? p0 + pchunk : S.n_pair;
  for (int c = t; c < P.n_in; c += SPH_FANOUT) {
    const T v = inb ? A.x0[(first + fr) * P.n_in + c] : T(0);
    xt[c] = v;
    xs[c] = v;
  }
  part[fr * SPH_FANOUT + t] = 0;
  if (t == 0) {
    stopf[fr] = inb ? 0 : 1;  // idle lanes of a ragged last block never start
    itv[fr] = accf[fr] = stat[fr] = rej[fr] = nact[fr] = 0;
    for (int i = 0; i < RSV_SCALARS; ++i) sc[i] = T(0);
    sc[RSV_LAM] = A.damping;
  }
  __syncthreads();
  PoseArgs<T> PL = P;  // the walk's view of x: the frames' trial rows in LDS
  PL.n_in = Y.stride;
  const T* xl = park + Y.xbase;
  const T* fixl = A.fixed + first * P.n_fixed;
  for (int k = 0; k <= A.max_iters; ++k) {
    if (tid < nl && stopf[tid] == 0) {  // phase A: lane = frame; the walk at the trial, E_pose and E_post
      const int lane = tid;
      T* pa = park + (size_t)lane * Y.stride;
      T* ca = pa + Y.cbase;
      const int64_t b = first + lane;
      T Ep = T(0);
      for (int l = 0; l < P.n_base; ++l) {  // links on the fixed base: below no joint, but their error and their spheres count
        const LinkD<T>& L = links[l];
        if (targets) Ep += resolve_link(L.R, L.p, L.out, b, A, pa + Y.lbase + IK_LINK * l);
        for (int s = S.link_sph[l]; s < S.link_sph[l + 1]; ++s) sphere_centre(L.R, L.p, spheres[s], ca + 3 * s);
      }
      Xf<T> tf;
#pragma unroll
      for (int i = 0; i < 9; ++i) tf.R[i] = (i % 4 == 0) ? T(1) : T(0);
      tf.p[0] = tf.p[1] = tf.p[2] = T(0);
      int xi = 0;
      for (int j = 0; j < P.n_joint; ++j) {
        const JointD<T>& J = joints[j];
        T a[3];
        joint_step(J, PL, xl, fixl, (int64_t)lane, slots, nl, lane, tf, a);
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
          const LinkD<T>& L = links[l];
          T R[9], p[3];
          link_pose(L, tf, R, p);
          if (targets) Ep += resolve_link(R, p, L.out, b, A, pa + Y.lbase + IK_LINK * l);
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
    __syncthreads();
    const bool work = stopf[fr] == 0;
    if (work) {  // phase B: a thread per sphere; forces with g_p = w_p h_p (g = -1/2 grad E), energies, active flags
      T e = T(0);
      for (int s = t; s < S.n_sphere; s += SPH_FANOUT) {
        const T c0 = cen[3 * s], c1 = cen[3 * s + 1], c2 = cen[3 * s + 2];
        T f0 = T(0), f1 = T(0), f2 = T(0);
        const int i1 = S.inc_ptr[s + 1];
        for (int i = S.inc_ptr[s]; i < i1; ++i) {
          const uint32_t u = S.inc[i];
          const int o = u & 127, p = u >> 8;
          const T d0 = c0 - cen[3 * o], d1 = c1 - cen[3 * o + 1], d2 = c2 - cen[3 * o + 2];
          const T sp = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)));
          T h = A.margin - (sp - rsum[p]);
          if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
          const T wh = A.pw ? A.pw[p] * h : h;
          if (u & SPH_FIRST) {
            e = fma(wh, h, e);
            fl[p] = h > T(0) ? 1 : 0;
          }
          const T q = sp > T(0) ? wh / sp : wh * (sp * T(0));  // coincident centres: no direction
          f0 = fma(q, d0, f0);
          f1 = fma(q, d1, f1);
          f2 = fma(q, d2, f2);
        }
        frc[3 * s] = f0;
        frc[3 * s + 1] = f1;
        frc[3 * s + 2] = f2;
      }
      pk[Y.pebase + t] = e;
    }
    __syncthreads();
    if (work) {  // phase C: the counts of the active list, and the decision
      int n = 0;
      for (int p = p0; p < p1; ++p) n += fl[p];
      cnt[fr * SPH_FANOUT + t] = n;
      if (t == 0) {
        T Ec = pk[Y.pebase];
        for (int i = 1; i < SPH_FANOUT; ++i) Ec += pk[Y.pebase + i];
        Ec *= A.wcol;
        const T Et = (sc[RSV_TPOSE] + sc[RSV_TPOST]) + Ec;
        const bool acc = k == 0 || Et <= sc[RSV_E];  // (a comparison: a NaN rejects)
        int st = stat[fr];
        bool stop = false;
        if (acc) {
          T step = T(0);
          for (int i = 0; i < n_act; ++i) {
            const int c = act_col[i];
            const T d = fabs(xt[c] - xs[c]);
            step = d > step ? d : step;
            xs[c] = xt[c];
          }
          sc[RSV_E] = Et;
          sc[RSV_POSE] = sc[RSV_TPOSE];
          sc[RSV_POST] = sc[RSV_TPOST];
          sc[RSV_COL] = Ec;
          if (k > 0) {
            const T l = sc[RSV_LAM] / T(DEXR_RESOLVE_LAM_DOWN);
            sc[RSV_LAM] = l > A.damping ? l : A.damping;
            rej[fr] = 0;
            if (step <= A.tol) {
              st |= DEXR_RESOLVE_CONVERGED;
              stop = true;
            }
          }
        } else {
          sc[RSV_LAM] *= T(DEXR_RESOLVE_LAM_UP);
          if (++rej[fr] == DEXR_RESOLVE_MAXREJECT) {
            st |= DEXR_RESOLVE_STALLED;
            stop = true;
          }
        }
        itv[fr] = k;
        accf[fr] = acc ? 1 : 0;
        stat[fr] = st;
        if (stop || k == A.max_iters) stopf[fr] = 1;
      }
    }
    __syncthreads();
    if (work && t == 0) {  // (stat and nact of a frame are its thread 0's alone until the next barrier)
      int total = 0;
      for (int u = 0; u < SPH_FANOUT; ++u) total += cnt[fr * SPH_FANOUT + u];
      if (total > DEXR_RESOLVE_MAXACTIVE) {
        stat[fr] |= DEXR_RESOLVE_TRUNCATED;
        total = DEXR_RESOLVE_MAXACTIVE;
      }
      nact[fr] = (accf[fr] != 0 && stopf[fr] == 0) ? total : 0;
    }
    bool all = true;  // the block's vote, the same in every thread
    for (int f = 0; f < nl; ++f) all = all && stopf[f] != 0;
    if (all) break;
    const bool go = stopf[fr] == 0;            // the frame goes on: it needs a next trial
    const bool build = go && accf[fr] != 0;  // ... from a new point: its list, g and H are formed and kept
    if (build) {  // phase D: the active list in pair-index order, then g with the freeze test of its columns
      int off = 0;
      for (int u = 0; u < t; ++u) off += cnt[fr * SPH_FANOUT + u];
      for (int p = p0; p < p1 && off < DEXR_RESOLVE_MAXACTIVE; ++p)
        if (fl[p]) lst[off++] = (uint32_t)p;
      unsigned long long mine = 0;
      for (int i = t; i < n_act; i += SPH_FANOUT) {
        const int c = act_col[i];
        const uint32_t r = act_rng[i];
        T s = targets ? ik_g_entry(r, ents, pk, Y.lbase) : T(0);
        if (A.u) s = fma(A.u[c], xr[c] - xs[c], s);
        s = fma(A.wcol, resolve_force_entry(r, ents, S.link_sph, pk, cen, frc), s);
        if (A.lo) {
          const T xc = xs[c];
          if ((xc <= A.lo[c] && s < T(0)) || (xc >= A.hi[c] && s > T(0))) {
            mine |= 1ull << i;
            s = T(0);
          }
        }
        gs[i] = s;
      }
      part[fr * SPH_FANOUT + t] = mine;
    }
    __syncthreads();
    unsigned long long frozen = 0;  // of the last accepted point: a frame that rejected keeps its partial masks
    for (int u = 0; u < SPH_FANOUT; ++u) frozen |= part[fr * SPH_FANOUT + u];
    if (build) {
      for (int e = t; e < n_tri; e += SPH_FANOUT) {  // a frozen column's row and column of H are the identity's
        const uint2 d = tri[e];
        const int i = d.x & 63, j = d.x >> 6;
        T h;
        if (((frozen >> i) | (frozen >> j)) & 1ull) {
          h = i == j ? T(1) : T(0);
        } else {
          h = targets ? ik_h_entry(d, ents, pk, Y.lbase) : T(0);
          if (i == j && A.u) h += A.u[act_col[i]];
        }
        Hs[e] = h;
      }
    }
    int nmax = 0;  // the block's largest list: the same in every thread
    for (int f = 0; f < nl; ++f) nmax = nact[f] > nmax ? nact[f] : nmax;
    const int mine_n = nact[fr];  // (0 unless `build`)
#if DEXR_RESOLVE_CURVATURE_WALK
    // the other way of forming the pair curvature, kept for tools/resolve_probe.py to time: every entry H[i, j] walks the active
    // list and forms the two gradients it needs itself -- no staging and no barrier, n_act / 2 times the gradient work
    nmax = 0;
    if (mine_n > 0) {
      for (int e = t; e < n_tri; e += SPH_FANOUT) {
        const uint2 dd = tri[e];
        const int i = dd.x & 63, j = dd.x >> 6;
        if (((frozen >> i) | (frozen >> j)) & 1ull) continue;
        T h = Hs[e];
        for (int q = 0; q < mine_n; ++q) {
          const uint32_t p = lst[q], ps = pair_sph[p];
          const int si = ps & 127, sj = (ps >> 7) & 127;
          const T d[3] = {cen[3 * si] - cen[3 * sj], cen[3 * si + 1] - cen[3 * sj + 1], cen[3 * si + 2] - cen[3 * sj + 2]};
          const T sp = sqrt(fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])));
          const T inv = sp > T(0) ? T(1) / sp : T(0);
          const T n[3] = {d[0] * inv, d[1] * inv, d[2] * inv};
          const T gi = resolve_row_entry(act_rng[i], ents, S.link_sph, pk, cen, si, sj, n);
          const T gj = i == j ? gi : resolve_row_entry(act_rng[j], ents, S.link_sph, pk, cen, si, sj, n);
          h = fma((A.pw ? A.wcol * A.pw[p] : A.wcol) * gi, gj, h);
        }
        Hs[e] = h;
      }
    }
#endif
    for (int base = 0; base < nmax; base += SPH_FANOUT) {  // the pair curvature, sixteen rows grad d_p at a time
      if (base + t < mine_n) {
        const uint32_t p = lst[base + t], ps = pair_sph[p];
        const int si = ps & 127, sj = (ps >> 7) & 127;
        const T d[3] = {cen[3 * si] - cen[3 * sj], cen[3 * si + 1] - cen[3 * sj + 1], cen[3 * si + 2] - cen[3 * sj + 2]};
        const T sp = sqrt(fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])));
        const T inv = sp > T(0) ? T(1) / sp : T(0);
        const T n[3] = {d[0] * inv, d[1] * inv, d[2] * inv};
        T* row = rows + t * n_act;
        for (int i = 0; i < n_act; ++i)
          row[i] = ((frozen >> i) & 1ull) ? T(0) : resolve_row_entry(act_rng[i], ents, S.link_sph, pk, cen, si, sj, n);
        rw[t] = A.pw ? A.wcol * A.pw[p] : A.wcol;
      }
      __syncthreads();
      const int nk = mine_n - base < SPH_FANOUT ? mine_n - base : SPH_FANOUT;
      if (nk > 0) {
        for (int e = t; e < n_tri; e += SPH_FANOUT) {
          const uint2 dd = tri[e];
          const int i = dd.x & 63, j = dd.x >> 6;
          T h = Hs[e];
          for (int q = 0; q < nk; ++q) h = fma(rw[q] * rows[q * n_act + i], rows[q * n_act + j], h);
          Hs[e] = h;
        }
      }
      __syncthreads();
    }
    if (go) {  // phase E: the kept system with the frame's lam
      const T lam = sc[RSV_LAM];
      for (int e = t; e < n_tri; e += SPH_FANOUT) {
        const uint2 d = tri[e];
        const int i = d.x & 63, j = d.x >> 6;
        H[e] = (i == j && !((frozen >> i) & 1ull)) ? Hs[e] + lam : Hs[e];
      }
      for (int i = t; i < n_act; i += SPH_FANOUT) g[i] = gs[i];
    }
    __syncthreads();
    ik_factor_solve(H, g, y, dg, n_act, t, go);
    if (go) {  // limit the step, move, clamp: by comparisons, a NaN stays a NaN
      T scale = T(1);
      if (A.max_step > T(0)) {
        T m = T(0);
        for (int i = 0; i < n_act; ++i) {
          const T a = fabs(g[i]);
          m = a > m ? a : m;
        }
        if (m > A.max_step) scale = A.max_step / m;
      }
      for (int i = t; i < n_act; i += SPH_FANOUT) {
        const int c = act_col[i];
        T v = xs[c] + g[i] * scale;
        if (A.lo) {
          const T l = A.lo[c], h = A.hi[c];
          v = v < l ? l : (v > h ? h : v);
        }
        xt[c] = v;
      }
    }
    __syncthreads();
  }
  if (inb) {
    T* o = A.x_out + (first + fr) * P.n_in;
    for (int c = t; c < P.n_in; c += SPH_FANOUT) o[c] = xs[c];
    if (t == 0) {
      if (A.iters_out) A.iters_out[first + fr] = itv[fr];
      if (A.status_out) A.status_out[first + fr] = stat[fr];
      if (A.e_out) {
        T* eo = A.e_out + (first + fr) * 3;
        eo[0] = sc[RSV_POSE];
        eo[1] = sc[RSV_POST];
        eo[2] = sc[RSV_COL];
      }
    }
  }
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

template <typename T>
int launch_resolve(const dexr_sphere_model* sm, int64_t B, ResolveArgs<T> A, hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  const ResolveLayout Y = resolve_layout<T>(sm, A.n_target);
  const int fstride = (sm->n_pair + 3) & ~3;
  const size_t per_frame = SPH_FANOUT * sizeof(unsigned long long) + ((size_t)m->h.n_slot * 12 + (size_t)Y.stride) * sizeof(T) +
                           (DEXR_RESOLVE_MAXACTIVE + SPH_FANOUT + 6) * sizeof(int32_t) + (size_t)fstride;
  int nl = SPH_FRAMES;
  while (nl > 1 && per_frame * nl > 64 * 1024) nl /= 2;  // (the largest model in float64: one frame)
  if (per_frame * nl > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the sphere model needs %zu B of LDS per frame: one frame does not fit a block", per_frame);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  if (!A.xref) A.xref = A.x0;
  hipLaunchKernelGGL(pose_resolve_kernel<T>, dim3((unsigned)blocks), dim3(nl * SPH_FANOUT), per_frame * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), (const SphereD<T>*)sphere_tables_of<T>(sm).spheres,
                     (const T*)sphere_tables_of<T>(sm).rsum, S, (const uint32_t*)sm->pair_sph, (const JacEnt*)m->jac_ents,
                     (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col, (const uint2*)m->ik_tri, m->n_jx, m->n_act, Y, fstride, A);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "collision resolve kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

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
  const dexr_pose_model* pm = m->pose;
  const size_t nx = (size_t)B * pm->h.n_in * sizeof(double), nf = (size_t)B * pm->h.n_fixed * sizeof(double);
  const size_t nw = (size_t)B * n_target * sizeof(double), nb = (size_t)pm->h.n_in * sizeof(double);
  DevBuf dx, dfix, dref, du, dp, dr, dwl, dwa, dpw, dlo, dhi, dout, dit, den, dst;
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
  POSE_HIP(dout.put(nullptr, nx));
  POSE_HIP(dit.put(nullptr, (size_t)B * sizeof(int32_t)));
  POSE_HIP(den.put(nullptr, (size_t)B * 3 * sizeof(double)));
  POSE_HIP(dst.put(nullptr, (size_t)B * sizeof(int32_t)));
  const ResolveArgs<double> A = {(const double*)dx.p,  (const double*)dfix.p, (const double*)dref.p, (const double*)du.p,  (const double*)dp.p,
                                 (const double*)dr.p,  (const double*)dwl.p,  (const double*)dwa.p,  (const double*)dpw.p, (const double*)dlo.p,
                                 (const double*)dhi.p, margin,                collision_weight,      damping,              max_step,
                                 tol,                  n_target,              max_iters,             (double*)dout.p,      (int32_t*)dit.p,
                                 (double*)den.p,       (int32_t*)dst.p};
  const int rc = launch_resolve<double>(m, B, A, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (nx) POSE_HIP(hipMemcpy(x_out, dout.p, nx, hipMemcpyDeviceToHost));
  if (iters_out) POSE_HIP(hipMemcpy(iters_out, dit.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (energy_out) POSE_HIP(hipMemcpy(energy_out, den.p, (size_t)B * 3 * sizeof(double), hipMemcpyDeviceToHost));
  if (status_out) POSE_HIP(hipMemcpy(status_out, dst.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DEXR_OK;
}

}  // extern "C"

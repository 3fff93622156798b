// dexr_resolve_grid.hpp -- the collision-aware posture solve against a sampled signed-distance field (include/dexr_resolve_grid.h):
// a fragment of dexr_pose.hip, which includes it once at its end, after the grid fragment.  pose_resolve_grid_kernel<T> is the
// resident loop of pose_resolve_obstacle_kernel (dexr_resolve_obstacles.hpp) with the cell lookup of pose_grid_kernel in the place
// of the primitive loop.  It shares ResolveLayout, ResolveArgs, resolve_link, resolve_force_entry, resolve_row_entry and the RSV_*
// scalars of dexr_resolve.hpp, ResolveObstacleArgs, RSV_OBS, obstacle_point and obstacle_to_world of dexr_resolve_obstacles.hpp, and
// grid_sdf<T, true> with the GridD<T> descriptor (uniform data, by value) of the grid fragment.  None of those kernels is touched.
//
// What a pass does beyond dexr_resolve.hpp:
//   A  pass 0 also parks the frame's obstacle pose (p_o, R_o; zeros and the identity where the caller left them out);
//   B  after the pair forces of a sphere the thread moves the centre into the grid's frame once, y = R_o^T (c - p_o), and does ONE
//      grid_sdf call: d = sdf - r, h = max(0, obstacle_margin - d).  The sphere's force becomes w_col f_pairs + w_obs R_o (h grad),
//      so that g needs no new code; h^2 goes to a second set of sixteen partial energies; the sphere's active flag is ONE byte in
//      LDS, stored at the CALLER's index of the sphere;
//   C  thread t counts the flags of its contiguous slice of caller indices; thread 0 adds the sixteen partial obstacle energies in
//      order and decides on E = ((E_pose + E_post) + E_col) + E_obs;
//   D  the contact list (sorted sphere indices, a byte each) by a prefix over the sixteen counts, in the caller's sphere order.
//      A sphere has at most one contact with a grid: at most DEXR_SPHERE_MAX entries, nothing is capped and no status bit
//      says so.  After the pair chunks the contact curvature goes through the same rank-16 staging: the thread recomputes
//      the normal of its sphere by grid_sdf from the parked centre and pose (the inputs and the function of phase B: the same
//      bits) and takes the row through resolve_row_entry with one sphere.  A zero gradient gives a zero row: energy only.
// Kept system, phase E, factor / solve and the outputs are those of pose_resolve_kernel; energy_out has four columns.
//
// THE LOOP CANNOT HANG, for the reasons of dexr_resolve.hpp: k = 0 .. max_iters at most, every barrier outside every condition that
// differs between the threads of a block, both chunk counts the block's largest (read by every thread from LDS after a barrier),
// the one early exit on the AND of all stop flags.  Every sum is taken by one thread in a fixed order.  No input makes a load
// leave the samples: every lookup goes through grid_sdf and its clamps.
//
// LDS of a block: sixteen 64-bit partial frozen masks per frame | the fork slots | per frame a region [frame][stride], odd stride
// (ResolveLayout, then the obstacle pose and the sixteen partial obstacle energies) | per frame the active pairs, sixteen counts,
// six words of state, sixteen contact counts, the curvature contacts | per frame the contact list, a byte per sphere | per frame the
// active flags, a byte per sphere | per frame one byte per pair.  include/dexr_resolve_grid.h states the bytes.
#include "dexr_resolve_grid.h"

namespace {

template <typename T>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES)
    pose_resolve_grid_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links, PoseArgs<T> P,
                             const SphereD<T>* __restrict__ spheres, const T* __restrict__ rsum, SphereIndex S,
                             const int32_t* __restrict__ sph_in, const uint32_t* __restrict__ pair_sph, const JacEnt* __restrict__ ents,
                             const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col, const uint2* __restrict__ tri,
                             GridD<T> G, const float* __restrict__ V, int n_jx, int n_act, ResolveLayout Y, int obase, int oebase, int sstride,
                             int fstride, ResolveArgs<T> A, ResolveObstacleArgs<T> O) {
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
  int32_t* ccnt = nact + nl;              // [nl][SPH_FANOUT]: contacts of a thread's slice of spheres
  int32_t* ncon = ccnt + nl * SPH_FANOUT;  // [nl]: curvature contacts
  unsigned char* clists = reinterpret_cast<unsigned char*>(ncon + nl);  // [nl][sstride]: sorted sphere indices, the caller's order
  unsigned char* active = clists + (size_t)nl * sstride;                // [nl][sstride]: by the caller's sphere index
  unsigned char* flags = active + (size_t)nl * sstride;                 // [nl][fstride]
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
  const T* po = pk + obase;  // the frame's obstacle pose
  T* rows = H;  // [SPH_FANOUT][n_act], then SPH_FANOUT weights
  T* rw = rows + SPH_FANOUT * n_act;
  uint32_t* lst = lists + fr * DEXR_RESOLVE_MAXACTIVE;
  unsigned char* clst = clists + (size_t)fr * sstride;
  unsigned char* act = active + (size_t)fr * sstride;
  unsigned char* fl = flags + (size_t)fr * fstride;
  const T* xr = A.xref + (inb ? first + fr : 0) * P.n_in;  // (read by working frames alone)
  const int pchunk = (S.n_pair + SPH_FANOUT - 1) / SPH_FANOUT;  // thread t owns the pairs [t pchunk, (t + 1) pchunk)
  const int p0 = t * pchunk < S.n_pair ? t * pchunk : S.n_pair, p1 = p0 + pchunk < S.n_pair ? p0 + pchunk : S.n_pair;
  const int schunk = (S.n_sphere + SPH_FANOUT - 1) / SPH_FANOUT;  // ... and the caller's spheres [t schunk, (t + 1) schunk)
  const int c0 = t * schunk < S.n_sphere ? t * schunk : S.n_sphere, c1 = c0 + schunk < S.n_sphere ? c0 + schunk : S.n_sphere;
  for (int c = t; c < P.n_in; c += SPH_FANOUT) {
    const T v = inb ? A.x0[(first + fr) * P.n_in + c] : T(0);
    xt[c] = v;
    xs[c] = v;
  }
  part[fr * SPH_FANOUT + t] = 0;
  if (t == 0) {
    stopf[fr] = inb ? 0 : 1;  // idle lanes of a ragged last block never start
    itv[fr] = accf[fr] = stat[fr] = rej[fr] = nact[fr] = ncon[fr] = 0;
    for (int i = 0; i < RSV_SCALARS; ++i) sc[i] = T(0);
    sc[RSV_LAM] = A.damping;
  }
  __syncthreads();
  PoseArgs<T> PL = P;  // the walk's view of x: the frames' trial rows in LDS
  PL.n_in = Y.stride;
  const T* xl = park + Y.xbase;
  const T* fixl = A.fixed + first * P.n_fixed;
  for (int k = 0; k <= A.max_iters; ++k) {
    if (tid < nl && stopf[tid] == 0) {  // phase A: lane = frame; the walk at the trial, E_pose and E_post; pass 0: the obstacle pose
      const int lane = tid;
      T* pa = park + (size_t)lane * Y.stride;
      T* ca = pa + Y.cbase;
      const int64_t b = first + lane;
      if (k == 0) {
        T* oa = pa + obase;
#pragma unroll
        for (int i = 0; i < 3; ++i) oa[i] = O.opos ? O.opos[b * 3 + i] : T(0);
#pragma unroll
        for (int i = 0; i < 9; ++i) oa[3 + i] = O.orot ? O.orot[b * 9 + i] : ((i % 4 == 0) ? T(1) : T(0));
      }
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
    if (work) {  // phase B: a thread per sphere; its pair forces, then its one lookup: force, energy, both kinds of active flag
      T e = T(0), eo = T(0);
      for (int s = t; s < S.n_sphere; s += SPH_FANOUT) {
        const T cs[3] = {cen[3 * s], cen[3 * s + 1], cen[3 * s + 2]};
        T f0 = T(0), f1 = T(0), f2 = T(0);
        const int i1 = S.inc_ptr[s + 1];
        for (int i = S.inc_ptr[s]; i < i1; ++i) {
          const uint32_t u = S.inc[i];
          const int o = u & 127, p = u >> 8;
          const T d0 = cs[0] - cen[3 * o], d1 = cs[1] - cen[3 * o + 1], d2 = cs[2] - cen[3 * o + 2];
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
        T yo[3], gm[3];
        obstacle_point(po, cs, yo);
        const T d = grid_sdf<T, true>(G, V, yo, gm) - spheres[s].r;
        T h = O.omargin - d;
        if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
        eo = fma(h, h, eo);
        const T fo[3] = {h * gm[0], h * gm[1], h * gm[2]};  // h grad sdf in the grid's frame
        T fw[3];
        obstacle_to_world(po, fo, fw);
        frc[3 * s] = fma(O.wobs, fw[0], A.wcol * f0);
        frc[3 * s + 1] = fma(O.wobs, fw[1], A.wcol * f1);
        frc[3 * s + 2] = fma(O.wobs, fw[2], A.wcol * f2);
        act[S.sph_out[s]] = h > T(0) ? 1 : 0;
      }
      pk[Y.pebase + t] = e;
      pk[oebase + t] = eo;
    }
    __syncthreads();
    if (work) {  // phase C: the counts of both lists, and the decision
      int n = 0;
      for (int p = p0; p < p1; ++p) n += fl[p];
      cnt[fr * SPH_FANOUT + t] = n;
      n = 0;
      for (int c = c0; c < c1; ++c) n += act[c];
      ccnt[fr * SPH_FANOUT + t] = n;
      if (t == 0) {
        T Ec = pk[Y.pebase], Eo = pk[oebase];
        for (int i = 1; i < SPH_FANOUT; ++i) Ec += pk[Y.pebase + i];
        for (int i = 1; i < SPH_FANOUT; ++i) Eo += pk[oebase + i];
        Ec *= A.wcol;
        Eo *= O.wobs;
        const T Et = ((sc[RSV_TPOSE] + sc[RSV_TPOST]) + Ec) + Eo;
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
          sc[RSV_OBS] = Eo;
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
    if (work && t == 0) {  // (stat, nact and ncon of a frame are its thread 0's alone until the next barrier)
      int total = 0, ctotal = 0;
      for (int u = 0; u < SPH_FANOUT; ++u) {
        total += cnt[fr * SPH_FANOUT + u];
        ctotal += ccnt[fr * SPH_FANOUT + u];  // (at most n_sphere: nothing to cap)
      }
      if (total > DEXR_RESOLVE_MAXACTIVE) {
        stat[fr] |= DEXR_RESOLVE_TRUNCATED;
        total = DEXR_RESOLVE_MAXACTIVE;
      }
      const bool keep = accf[fr] != 0 && stopf[fr] == 0;
      nact[fr] = keep ? total : 0;
      ncon[fr] = keep ? ctotal : 0;
    }
    bool all = true;  // the block's vote, the same in every thread
    for (int f = 0; f < nl; ++f) all = all && stopf[f] != 0;
    if (all) break;
    const bool go = stopf[fr] == 0;            // the frame goes on: it needs a next trial
    const bool build = go && accf[fr] != 0;  // ... from a new point: its lists, g and H are formed and kept
    if (build) {  // phase D: both lists in their orders, then g with the freeze test of its columns
      int off = 0, coff = 0;
      for (int u = 0; u < t; ++u) {
        off += cnt[fr * SPH_FANOUT + u];
        coff += ccnt[fr * SPH_FANOUT + u];
      }
      for (int p = p0; p < p1 && off < DEXR_RESOLVE_MAXACTIVE; ++p)
        if (fl[p]) lst[off++] = (uint32_t)p;
      for (int c = c0; c < c1; ++c)  // the caller's sphere order; coff stays below the number of flags set: < sstride
        if (act[c]) clst[coff++] = (unsigned char)sph_in[c];
      unsigned long long mine = 0;
      for (int i = t; i < n_act; i += SPH_FANOUT) {
        const int c = act_col[i];
        const uint32_t r = act_rng[i];
        T s = targets ? ik_g_entry(r, ents, pk, Y.lbase) : T(0);
        if (A.u) s = fma(A.u[c], xr[c] - xs[c], s);
        s += resolve_force_entry(r, ents, S.link_sph, pk, cen, frc);  // (the forces carry w_col and w_obs)
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
    int nmax = 0, cmax = 0;  // the block's largest lists: the same in every thread
    for (int f = 0; f < nl; ++f) {
      nmax = nact[f] > nmax ? nact[f] : nmax;
      cmax = ncon[f] > cmax ? ncon[f] : cmax;
    }
    const int mine_n = nact[fr], mine_c = ncon[fr];  // (0 unless `build`)
    nmax = (nmax + SPH_FANOUT - 1) / SPH_FANOUT * SPH_FANOUT;  // whole chunks: the contacts start at a chunk boundary of their own
    for (int base = 0; base < nmax + cmax; base += SPH_FANOUT) {  // the curvature, sixteen rows at a time: the pairs' grad d_p, then
      const bool pairs = base < nmax;                               // the contacts' grad d_s (the same choice in every thread)
      const int at = pairs ? base : base - nmax;
      const int have = pairs ? mine_n : mine_c;
      if (at + t < have) {
        T n[3], w;
        int si, sj;
        if (pairs) {
          const uint32_t p = lst[at + t], ps = pair_sph[p];
          si = ps & 127, sj = (ps >> 7) & 127;
          const T d[3] = {cen[3 * si] - cen[3 * sj], cen[3 * si + 1] - cen[3 * sj + 1], cen[3 * si + 2] - cen[3 * sj + 2]};
          const T sp = sqrt(fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])));
          const T inv = sp > T(0) ? T(1) / sp : T(0);
#pragma unroll
          for (int i = 0; i < 3; ++i) n[i] = d[i] * inv;
          w = A.pw ? A.wcol * A.pw[p] : A.wcol;
        } else {
          si = clst[at + t], sj = -1;  // one sphere: no link holds sphere -1
          T yo[3], gm[3];
          obstacle_point(po, cen + 3 * si, yo);
          (void)grid_sdf<T, true>(G, V, yo, gm);
          obstacle_to_world(po, gm, n);
          w = O.wobs;
        }
        T* row = rows + t * n_act;
        for (int i = 0; i < n_act; ++i)
          row[i] = ((frozen >> i) & 1ull) ? T(0) : resolve_row_entry(act_rng[i], ents, S.link_sph, pk, cen, si, sj, n);
        rw[t] = w;
      }
      __syncthreads();
      const int nk = have - at < SPH_FANOUT ? have - at : SPH_FANOUT;
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
        T* eo = A.e_out + (first + fr) * 4;
        eo[0] = sc[RSV_POSE];
        eo[1] = sc[RSV_POST];
        eo[2] = sc[RSV_COL];
        eo[3] = sc[RSV_OBS];
      }
    }
  }
}

// the argument rules of both entry points: those of check_resolve_call and the grid side's; < 0 error, 1 nothing to do, 0 go on
int check_resolve_grid_call(const dexr_sphere_model* sm, const dexr_sdf_grid* gr, double omargin, double wobs, int64_t B, const void* x0,
                            const void* fixed, int32_t n_target, const void* tp, const void* tr, const void* wl, const void* wa, double margin,
                            double wcol, const void* lo, const void* hi, double damping, double max_step, double tol, int32_t max_iters,
                            const void* x_out) {
  const double big = 1.7976931348623157e308;
  if (!sm) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (!gr) return dexr_set_error(DEXR_ERR_INVALID, "null sdf grid");
  if (!(omargin >= 0.0) || omargin > big) return dexr_set_error(DEXR_ERR_INVALID, "obstacle_margin must be finite and >= 0, got %g", omargin);
  if (!(wobs >= 0.0) || wobs > big) return dexr_set_error(DEXR_ERR_INVALID, "obstacle_weight must be finite and >= 0, got %g", wobs);
  return check_resolve_call(sm, B, x0, fixed, n_target, tp, tr, wl, wa, margin, wcol, lo, hi, damping, max_step, tol, max_iters, x_out);
}

template <typename T>
int launch_resolve_grid(const dexr_sphere_model* sm, const dexr_sdf_grid* gr, int64_t B, ResolveArgs<T> A, const ResolveObstacleArgs<T>& O,
                        hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  ResolveLayout Y = resolve_layout<T>(sm, A.n_target);
  const int obase = Y.sbase + RSV_SCALARS, oebase = obase + OBS_POSE;  // behind the scalars: the pose, sixteen partial energies
  Y.stride = (oebase + SPH_FANOUT) | 1;
  const int sstride = (sm->n_sphere + 3) & ~3, fstride = (sm->n_pair + 3) & ~3;
  // (the formula of include/dexr_resolve_grid.h)
  const size_t per_frame = SPH_FANOUT * sizeof(unsigned long long) + ((size_t)m->h.n_slot * 12 + (size_t)Y.stride) * sizeof(T) +
                           (DEXR_RESOLVE_MAXACTIVE + SPH_FANOUT + 6) * sizeof(int32_t) + (SPH_FANOUT + 1) * sizeof(int32_t) +
                           2 * (size_t)sstride + (size_t)fstride;
  int nl = SPH_FRAMES;
  while (nl > 1 && per_frame * nl > 64 * 1024) nl /= 2;
  if (per_frame * nl > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the sphere model needs %zu B of LDS per frame: one frame does not fit a block", per_frame);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  if (!A.xref) A.xref = A.x0;
  hipLaunchKernelGGL(pose_resolve_grid_kernel<T>, dim3((unsigned)blocks), dim3(nl * SPH_FANOUT), per_frame * nl, st,
                     (const JointD<T>*)tables_of<T>(m).joints, (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B),
                     (const SphereD<T>*)sphere_tables_of<T>(sm).spheres, (const T*)sphere_tables_of<T>(sm).rsum, S, (const int32_t*)sm->sph_in,
                     (const uint32_t*)sm->pair_sph, (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col,
                     (const uint2*)m->ik_tri, grid_desc_of<T>(gr), (const float*)gr->values, m->n_jx, m->n_act, Y, obase, oebase, sstride,
                     fstride, A, O);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "grid resolve kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

}  // namespace

extern "C" {

int dexr_sphere_resolve_grid_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                 const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                 const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                 const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                                 int32_t max_iters, const dexr_sdf_grid* grid, const float* obstacle_pos, const float* obstacle_rot,
                                 float obstacle_margin, float obstacle_weight, float* x_out, int32_t* iters_out, float* energy_out,
                                 int32_t* status_out, void* stream) {
  const int c = check_resolve_grid_call(m, grid, (double)obstacle_margin, (double)obstacle_weight, B, x0, fixed, n_target, target_pos, target_rot,
                                        pos_weight, rot_weight, (double)margin, (double)collision_weight, lo, hi, (double)damping,
                                        (double)max_step, (double)tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const ResolveArgs<float> A = {x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi,
                                margin, collision_weight, damping, max_step, tol, n_target, max_iters, x_out, iters_out, energy_out, status_out};
  const ResolveObstacleArgs<float> O = {obstacle_pos, obstacle_rot, obstacle_margin, obstacle_weight};
  return launch_resolve_grid<float>(m, grid, B, A, O, (hipStream_t)stream);
}

int dexr_sphere_resolve_grid(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                             const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                             const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                             const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                             int32_t max_iters, const dexr_sdf_grid* grid, const double* obstacle_pos, const double* obstacle_rot,
                             double obstacle_margin, double obstacle_weight, double* x_out, int32_t* iters_out, double* energy_out,
                             int32_t* status_out) {
  const int c = check_resolve_grid_call(m, grid, obstacle_margin, obstacle_weight, B, x0, fixed, n_target, target_pos, target_rot, pos_weight,
                                        rot_weight, margin, collision_weight, lo, hi, damping, max_step, tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const dexr_pose_model* pm = m->pose;
  const size_t nx = (size_t)B * pm->h.n_in * sizeof(double), nf = (size_t)B * pm->h.n_fixed * sizeof(double);
  const size_t nw = (size_t)B * n_target * sizeof(double), nb = (size_t)pm->h.n_in * sizeof(double), n1 = (size_t)B * sizeof(double);
  DevBuf dx, dfix, dref, du, dp, dr, dwl, dwa, dpw, dlo, dhi, dop, dor, dout, dit, den, dst;
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
  if (obstacle_pos) POSE_HIP(dop.put(obstacle_pos, 3 * n1));
  if (obstacle_rot) POSE_HIP(dor.put(obstacle_rot, 9 * n1));
  POSE_HIP(dout.put(nullptr, nx));
  POSE_HIP(dit.put(nullptr, (size_t)B * sizeof(int32_t)));
  POSE_HIP(den.put(nullptr, 4 * n1));
  POSE_HIP(dst.put(nullptr, (size_t)B * sizeof(int32_t)));
  const ResolveArgs<double> A = {(const double*)dx.p,  (const double*)dfix.p, (const double*)dref.p, (const double*)du.p,  (const double*)dp.p,
                                 (const double*)dr.p,  (const double*)dwl.p,  (const double*)dwa.p,  (const double*)dpw.p, (const double*)dlo.p,
                                 (const double*)dhi.p, margin,                collision_weight,      damping,              max_step,
                                 tol,                  n_target,              max_iters,             (double*)dout.p,      (int32_t*)dit.p,
                                 (double*)den.p,       (int32_t*)dst.p};
  const ResolveObstacleArgs<double> O = {(const double*)dop.p, (const double*)dor.p, obstacle_margin, obstacle_weight};
  const int rc = launch_resolve_grid<double>(m, grid, B, A, O, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (nx) POSE_HIP(hipMemcpy(x_out, dout.p, nx, hipMemcpyDeviceToHost));
  if (iters_out) POSE_HIP(hipMemcpy(iters_out, dit.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (energy_out) POSE_HIP(hipMemcpy(energy_out, den.p, 4 * n1, hipMemcpyDeviceToHost));
  if (status_out) POSE_HIP(hipMemcpy(status_out, dst.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
  return DEXR_OK;
}

}  // extern "C"

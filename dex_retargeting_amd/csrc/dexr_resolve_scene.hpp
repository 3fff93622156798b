// dexr_resolve_scene.hpp -- the collision-aware posture solve against a scene of several posed bodies
// (include/dexr_resolve_scene.h): a fragment of dexr_pose.hip, which includes it once after dexr_resolve_grid.hpp.  The loop has a
// home of its own here, resolve_scene_loop<T>: the skeleton of resolve_contact_loop (dexr_resolve_obstacles.hpp) made of the same
// resolve_* phases of dexr_resolve.hpp, with a loop over the bodies where that one asks its one contact source.  The per-body terms
// are the single-body kernels' sequences of operations: obstacle_point / obstacle_to_world around obstacle_sdf over the set's
// primitives in set order (a set), or around ONE grid_sdf<T, true> call (a grid).
//
// THE BODY TABLE IS UNIFORM DATA: SceneD<T> travels by value as a kernel argument -- per body the primitive table or the grid's
// descriptor and samples, the pose pointers, the primitive weights, margin_b and weight_b.  The body loop and the choice of kind
// are the same in every thread of a block in phases A to D; no barrier stands under a condition that differs inside a block.
//
// What a pass does beyond pose_resolve_kernel:
//   A  pass 0 also parks the n_body poses of the frame, OBS_POSE values each (zeros and the identity where the caller left them out);
//   B  the thread's spheres get their pair forces times w_col first; then, body by body, every sphere of the thread is moved into
//      the body's frame and gets the body's term: the force w h grad sdf there, w h^2 onto the thread's partial energy OF THAT BODY,
//      and a 64-bit active mask in LDS per (body, caller's sphere index) -- a set: bit m for primitive m, a grid: bit 0.  The force
//      of a sphere becomes fma(weight_b, R_b f_b, acc) in body order on top of w_col f_pairs, so that g needs no new code;
//   C  thread t counts the contacts (popcounts) of its contiguous slice of caller sphere indices over all bodies; thread 0 adds
//      each body's sixteen partial energies in order, weighs them, adds the bodies in order and decides on
//      E = ((E_pose + E_post) + E_col) + E_obs; an accepted trial's body energies become the frame's;
//   D  the contacts go into ONE list at a prefix over the sixteen counts, no atomics: caller's sphere order, then body order, then set
//      order; an entry is 16 bits, sorted sphere (7) | primitive << 7 (6) | body << 13 (2).  The list is capped at
//      DEXR_RESOLVE_MAXCONTACT over all bodies together, with DEXR_RESOLVE_CONTACTS_TRUNCATED -- grids take part in the cap here.  After
//      the pair chunks the contact curvature goes through the same rank-16 staging: a contact's normal is recomputed from the parked
//      centre and the parked pose of its body through the function of phase B (the same bits); the body of a contact differs from
//      thread to thread there, and no barrier stands inside.
// Kept system, phase E, factor / solve and the outputs are those of pose_resolve_kernel; energy_out has four columns and
// body_energy_out one per body.  The rule's constants are the headers', read where the rule stands: DEXR_RESOLVE_LAM_UP,
// DEXR_RESOLVE_LAM_DOWN and DEXR_RESOLVE_MAXREJECT in resolve_decide, DEXR_RESOLVE_MAXACTIVE in resolve_pair_total and
// resolve_list_pairs (dexr_resolve.hpp), DEXR_RESOLVE_MAXCONTACT, DEXR_RESOLVE_CONTACTS_TRUNCATED and DEXR_SCENE_MAXBODY here.
//
// LDS of a block: sixteen 64-bit partial frozen masks per frame | a 64-bit contact mask per body, sphere and frame | the fork slots
// | per frame a region [frame][stride], odd stride (ResolveLayout, then per body the pose, sixteen partial energies, the trial's
// and the accepted point's energy) | per frame the active pairs, sixteen counts, six words of state, sixteen contact counts, the
// curvature contacts | per frame the contact list (16 bits each) | per frame one byte per pair.  include/dexr_resolve_scene.h states
// the bytes.
#include "dexr_resolve_scene.h"

namespace {

static_assert(DEXR_SCENE_MAXBODY <= 4 && DEXR_OBSTACLE_MAX <= 64 && DEXR_SPHERE_MAX <= 128, "a contact is 7 + 6 + 2 bits");

template <typename T>
struct SceneBodyD {
  const ObstacleD<T>* prims;  // a set: its table (the kinds behind it); NULL: a grid
  const T* ow;                // a set: (n_prim) or NULL
  const float* V;             // a grid: its samples
  GridD<T> G;                 // a grid: its descriptor
  const T* opos;              // (B, 3) or NULL
  const T* orot;              // (B, 3, 3) or NULL
  T omargin, wobs;
  int n_prim;
};

template <typename T>
struct SceneD {
  SceneBodyD<T> b[DEXR_SCENE_MAXBODY];
  int n_body;
  T* be_out;  // (B, n_body) or NULL
};

// offsets (in values) into a frame's region behind the scalars of ResolveLayout: per body the pose, sixteen partial energies, the
// energy at the trial and at the accepted point
struct SceneLayout {
  int obase, oebase, tbase, abase;
};

constexpr int SCENE_BODY_VALUES = OBS_POSE + SPH_FANOUT + 2;

// the term of body Bd on the sphere of radius rs at yo (the body's frame): sum_m w_m h grad sdf_m into fo, w_m h^2 onto eo, the active
// primitives into bits -- the operations of ObstacleContacts::term
template <typename T>
__device__ __forceinline__ unsigned long long scene_set_term(const SceneBodyD<T>& Bd, const T yo[3], T rs, T& eo, T fo[3]) {
  const int32_t* kinds = obstacle_kinds(Bd.prims);
  fo[0] = fo[1] = fo[2] = T(0);
  unsigned long long bits = 0;
  for (int m = 0; m < Bd.n_prim; ++m) {
    T gm[3];
    const T d = obstacle_sdf(kinds[m], Bd.prims[m], yo, gm) - rs;
    T h = Bd.omargin - d;
    if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
    const T wh = Bd.ow ? Bd.ow[m] * h : h;
    eo = fma(wh, h, eo);
    if (h > T(0)) bits |= 1ull << m;
#pragma unroll
    for (int i = 0; i < 3; ++i) fo[i] = fma(wh, gm[i], fo[i]);
  }
  return bits;
}

// the same of a grid: ONE lookup, bit 0 -- the operations of GridContacts::term
template <typename T>
__device__ __forceinline__ unsigned long long scene_grid_term(const SceneBodyD<T>& Bd, const T yo[3], T rs, T& eo, T fo[3]) {
  T gm[3];
  const T d = grid_sdf<T, true>(Bd.G, Bd.V, yo, gm) - rs;
  T h = Bd.omargin - d;
  if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
  eo = fma(h, h, eo);
#pragma unroll
  for (int i = 0; i < 3; ++i) fo[i] = h * gm[i];
  return h > T(0) ? 1ull : 0ull;
}

// the q-th contact of the list: its sorted sphere, its world normal and its weight, from the parked centre and the parked pose
// of its body through the function of phase B
template <typename T>
__device__ __forceinline__ void scene_contact(const SceneD<T>& Q, const uint16_t* clst, const T* poses, const T* cen, int q, int& si, T n[3],
                                              T& w) {
  const uint32_t cm = clst[q];
  const int m = (cm >> 7) & 63, b = cm >> 13;
  si = cm & 127;
  const SceneBodyD<T>& Bd = Q.b[b];
  const T* po = poses + OBS_POSE * b;
  T yo[3], gm[3];
  obstacle_point(po, cen + 3 * si, yo);
  if (Bd.prims) {
    (void)obstacle_sdf(obstacle_kinds(Bd.prims)[m], Bd.prims[m], yo, gm);
    w = Bd.ow ? Bd.wobs * Bd.ow[m] : Bd.wobs;
  } else {
    (void)grid_sdf<T, true>(Bd.G, Bd.V, yo, gm);
    w = Bd.wobs;
  }
  obstacle_to_world(po, gm, n);
}

// The resident loop of the scene kernel.  THE LOOP CANNOT HANG, for the reasons written down at pose_resolve_kernel
// (dexr_resolve.hpp) and re-checked here: it runs k = 0 .. max_iters at most; every __syncthreads() stands in the body of the k
// loop or of the chunk loop, outside every condition that differs between the threads of a block -- the body loops of phases A to D
// hold no barrier, and their trip count n_body is a kernel argument; both chunk counts of the curvature loop (nmax, cmax) are the
// block's largest, read by every thread from LDS (nact, ncon of all frames) after the barrier that follows their last write, and
// not written again before the barrier that ends phase E; a frame that has stopped (or an idle lane of a ragged last block:
// stopped from the start) does no work and writes nothing but walks through the same barriers; the one early exit is taken on
// the AND of all stop flags, read by every thread after the same barrier, and at k == max_iters every flag is set.  Every sum is
// taken by one thread in table order: a frame's bits do not depend on the batch or on its neighbours.
template <typename T>
__device__ __forceinline__ void resolve_scene_loop(unsigned char* pose_lds, const ResolveModel<T>& M, const PoseArgs<T>& P,
                                                   const int32_t* __restrict__ sph_in, const ResolveLayout Y, const SceneLayout Z, int fstride,
                                                   const ResolveArgs<T> A, const SceneD<T>& Q) {
  const int nl = blockDim.x / SPH_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  const SphereIndex& S = M.S;
  const int fr = tid / SPH_FANOUT, t = tid % SPH_FANOUT;
  const int nb = Q.n_body, ns = S.n_sphere;
  const ResolveLds<T> L = resolve_lds<T>(pose_lds, nl, fr, t, Y, P.n_slot, M.n_act, S.n_pair, fstride, nb * ns,
                                         RESOLVE_CONTACT_COUNTS + DEXR_RESOLVE_MAXCONTACT * (int)sizeof(uint16_t));
  int32_t* ccnt = reinterpret_cast<int32_t*>(L.tail);  // [nl][SPH_FANOUT]: contacts of a thread's slice of spheres
  int32_t* ncon = ccnt + nl * SPH_FANOUT;              // [nl]: curvature contacts
  uint16_t* clst = reinterpret_cast<uint16_t*>(ncon + nl) + fr * DEXR_RESOLVE_MAXCONTACT;  // the frame's contact list
  unsigned long long* msk = L.head + fr * (nb * ns);   // [n_body][n_sphere] the frame's contact masks, by the caller's sphere index
  const int64_t first = (int64_t)blockIdx.x * nl;
  const bool inb = first + fr < P.B;
  const T* poses = L.pk + Z.obase;  // the frame's body poses
  const T* xr = A.xref + (inb ? first + fr : 0) * P.n_in;  // (read by working frames alone)
  const int schunk = (ns + SPH_FANOUT - 1) / SPH_FANOUT;  // thread t owns the caller's spheres [t schunk, (t + 1) schunk)
  const int c0 = t * schunk < ns ? t * schunk : ns, c1 = c0 + schunk < ns ? c0 + schunk : ns;
  resolve_start(L, A, P.n_in, first + fr, inb);
  if (t == 0) {
    ncon[fr] = 0;
    for (int b = 0; b < nb; ++b) L.pk[Z.tbase + b] = L.pk[Z.abase + b] = T(0);
  }
  __syncthreads();
  for (int k = 0; k <= A.max_iters; ++k) {
    if (tid < nl && L.stopf[tid] == 0) {  // phase A; pass 0: the poses of the bodies
      if (k == 0) {
        const int64_t row = first + tid;
        for (int b = 0; b < nb; ++b) {
          const SceneBodyD<T>& Bd = Q.b[b];
          T* oa = L.park + tid * Y.stride + Z.obase + OBS_POSE * b;
#pragma unroll
          for (int i = 0; i < 3; ++i) oa[i] = Bd.opos ? Bd.opos[row * 3 + i] : T(0);
#pragma unroll
          for (int i = 0; i < 9; ++i) oa[3 + i] = Bd.orot ? Bd.orot[row * 9 + i] : ((i % 4 == 0) ? T(1) : T(0));
        }
      }
      resolve_walk(L, M.joints, M.links, M.spheres, S, P, Y, A, tid, first);
    }
    __syncthreads();
    const bool work = L.stopf[fr] == 0;
    if (work) {  // phase B: a thread per sphere; its pair forces, then body by body its terms: forces, energies, active masks
      T e = T(0);
      for (int s = t; s < ns; s += SPH_FANOUT) {
        const T cs[3] = {L.cen[3 * s], L.cen[3 * s + 1], L.cen[3 * s + 2]};
        T f[3];
        resolve_pair_forces(L, M, A, s, cs, e, f);
        L.frc[3 * s] = A.wcol * f[0];
        L.frc[3 * s + 1] = A.wcol * f[1];
        L.frc[3 * s + 2] = A.wcol * f[2];
      }
      L.pk[Y.pebase + t] = e;
      for (int b = 0; b < nb; ++b) {  // (the same trip count and the same kind in every thread)
        const SceneBodyD<T>& Bd = Q.b[b];
        const T* po = poses + OBS_POSE * b;
        unsigned long long* mb = msk + b * ns;
        const bool set = Bd.prims != nullptr;
        T eo = T(0);
        for (int s = t; s < ns; s += SPH_FANOUT) {
          const T cs[3] = {L.cen[3 * s], L.cen[3 * s + 1], L.cen[3 * s + 2]};
          T yo[3], fo[3], fw[3];
          obstacle_point(po, cs, yo);
          const T rs = M.spheres[s].r;
          mb[S.sph_out[s]] = set ? scene_set_term(Bd, yo, rs, eo, fo) : scene_grid_term(Bd, yo, rs, eo, fo);
          obstacle_to_world(po, fo, fw);
          L.frc[3 * s] = fma(Bd.wobs, fw[0], L.frc[3 * s]);
          L.frc[3 * s + 1] = fma(Bd.wobs, fw[1], L.frc[3 * s + 1]);
          L.frc[3 * s + 2] = fma(Bd.wobs, fw[2], L.frc[3 * s + 2]);
        }
        L.pk[Z.oebase + SPH_FANOUT * b + t] = eo;
      }
    }
    __syncthreads();
    if (work) {  // phase C: the counts of both lists, and the decision
      resolve_count_pairs(L);
      int n = 0;
      for (int c = c0; c < c1; ++c)
        for (int b = 0; b < nb; ++b) n += __popcll(msk[b * ns + c]);
      ccnt[fr * SPH_FANOUT + t] = n;
      if (t == 0) {
        T Eo = T(0);
        for (int b = 0; b < nb; ++b) {  // each body's sixteen in order, then the bodies in order
          const T Eb = resolve_sum16(L.pk + Z.oebase + SPH_FANOUT * b) * Q.b[b].wobs;
          L.pk[Z.tbase + b] = Eb;
          Eo = b == 0 ? Eb : Eo + Eb;
        }
        resolve_decide<true>(L, M, A, k, resolve_sum16(L.pk + Y.pebase) * A.wcol, Eo);
        if (L.accf[fr] != 0)
          for (int b = 0; b < nb; ++b) L.pk[Z.abase + b] = L.pk[Z.tbase + b];
      }
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
      for (int c = c0; c < c1 && coff < DEXR_RESOLVE_MAXCONTACT; ++c) {  // caller's sphere order, then body order, then set order
        const uint32_t s = (uint32_t)sph_in[c];
        for (int b = 0; b < nb; ++b) {
          unsigned long long bits = msk[b * ns + c];
          while (bits != 0 && coff < DEXR_RESOLVE_MAXCONTACT) {
            const uint32_t m = (uint32_t)__ffsll((long long)bits) - 1u;
            clst[coff++] = (uint16_t)(s | (m << 7) | ((uint32_t)b << 13));
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
          scene_contact(Q, clst, poses, L.cen, at + t, si, n, w);
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
  if (inb) {
    resolve_output(L, A, P.n_in, first + fr, 4);
    if (t == 0 && Q.be_out)
      for (int b = 0; b < nb; ++b) Q.be_out[(first + fr) * nb + b] = L.pk[Z.abase + b];
  }
}

template <typename T>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES)
    pose_resolve_scene_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links, PoseArgs<T> P,
                              const SphereD<T>* __restrict__ spheres, const T* __restrict__ rsum, SphereIndex S,
                              const int32_t* __restrict__ sph_in, const uint32_t* __restrict__ pair_sph, const JacEnt* __restrict__ ents,
                              const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col, const uint2* __restrict__ tri, int n_jx,
                              int n_act, ResolveLayout Y, SceneLayout Z, int fstride, ResolveArgs<T> A, SceneD<T> Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const ResolveModel<T> M = {joints, links, spheres, rsum, S, pair_sph, ents, act_rng, act_col, tri, n_act, n_act * (n_act + 1) / 2};
  resolve_scene_loop<T>(pose_lds, M, P, sph_in, Y, Z, fstride, A, Q);
}

// the scene's argument rules, then those of check_resolve_call; < 0 error, 1 nothing to do, 0 go on
int check_resolve_scene_call(const dexr_sphere_model* sm, int32_t n_body, const dexr_scene_body* bodies, int64_t B, const void* x0,
                             const void* fixed, int32_t n_target, const void* tp, const void* tr, const void* wl, const void* wa, double margin,
                             double wcol, const void* lo, const void* hi, double damping, double max_step, double tol, int32_t max_iters,
                             const void* x_out) {
  const double big = 1.7976931348623157e308;
  if (!sm) return dexr_set_error(DEXR_ERR_INVALID, "null sphere model");
  if (n_body < 1 || n_body > DEXR_SCENE_MAXBODY)
    return dexr_set_error(DEXR_ERR_INVALID, "n_body must be in 1..%d, got %d", DEXR_SCENE_MAXBODY, n_body);
  if (!bodies) return dexr_set_error(DEXR_ERR_INVALID, "bodies is NULL");
  for (int b = 0; b < n_body; ++b) {
    const dexr_scene_body& D = bodies[b];
    if ((D.set == nullptr) == (D.grid == nullptr))
      return dexr_set_error(DEXR_ERR_INVALID, "body %d must have exactly one of set and grid, got %s", b, D.set ? "both" : "neither");
    if (D.grid && D.prim_weight) return dexr_set_error(DEXR_ERR_INVALID, "body %d is a grid and has a prim_weight: a grid has no primitives", b);
    if (!(D.margin >= 0.0) || D.margin > big)
      return dexr_set_error(DEXR_ERR_INVALID, "body %d: its margin must be finite and >= 0, got %g", b, D.margin);
    if (!(D.weight >= 0.0) || D.weight > big)
      return dexr_set_error(DEXR_ERR_INVALID, "body %d: its weight must be finite and >= 0, got %g", b, D.weight);
  }
  return check_resolve_call(sm, B, x0, fixed, n_target, tp, tr, wl, wa, margin, wcol, lo, hi, damping, max_step, tol, max_iters, x_out);
}

// the layout of the scene kernel's frame: behind the scalars of ResolveLayout, per body SCENE_BODY_VALUES values
template <typename T>
ResolveLayout resolve_scene_layout(const dexr_sphere_model* sm, int n_target, int n_body, SceneLayout* Z) {
  ResolveLayout Y = resolve_layout<T>(sm, n_target);
  Z->obase = Y.sbase + RSV_SCALARS;
  Z->oebase = Z->obase + OBS_POSE * n_body;
  Z->tbase = Z->oebase + SPH_FANOUT * n_body;
  Z->abase = Z->tbase + n_body;
  Y.stride = (Z->abase + n_body) | 1;
  static_assert(SCENE_BODY_VALUES == 30, "include/dexr_resolve_scene.h states 30 n_body");
  return Y;
}

// the body table of a launch from the caller's records; pos, rot and prim_weight as given there (device pointers of T)
template <typename T>
SceneD<T> scene_table(int32_t n_body, const dexr_scene_body* bodies, T* be_out) {
  SceneD<T> Q = {};
  Q.n_body = n_body, Q.be_out = be_out;
  for (int b = 0; b < n_body; ++b) {
    const dexr_scene_body& D = bodies[b];
    SceneBodyD<T>& Bd = Q.b[b];
    if (D.set) {
      Bd.prims = obstacle_table_of<T>(D.set), Bd.n_prim = D.set->n_prim, Bd.ow = (const T*)D.prim_weight;
    } else {
      Bd.G = grid_desc_of<T>(D.grid), Bd.V = (const float*)D.grid->values;
    }
    Bd.opos = (const T*)D.pos, Bd.orot = (const T*)D.rot, Bd.omargin = (T)D.margin, Bd.wobs = (T)D.weight;
  }
  return Q;
}

template <typename T>
int launch_resolve_scene(const dexr_sphere_model* sm, int64_t B, ResolveArgs<T> A, const SceneD<T>& Q, hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  SceneLayout Z;
  const ResolveLayout Y = resolve_scene_layout<T>(sm, A.n_target, Q.n_body, &Z);
  // (the formula of include/dexr_resolve_scene.h)
  const size_t per_frame = resolve_lds_bytes<T>(sm, Y, (size_t)Q.n_body * sm->n_sphere,
                                                RESOLVE_CONTACT_COUNTS + DEXR_RESOLVE_MAXCONTACT * sizeof(uint16_t));
  int nl;
  int64_t blocks;
  if (const int rc = resolve_launch_shape(per_frame, B, &nl, &blocks)) return rc;
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  if (!A.xref) A.xref = A.x0;
  hipLaunchKernelGGL(pose_resolve_scene_kernel<T>, dim3((unsigned)blocks), dim3(nl * SPH_FANOUT), per_frame * nl, st,
                     (const JointD<T>*)tables_of<T>(m).joints, (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B),
                     (const SphereD<T>*)sphere_tables_of<T>(sm).spheres, (const T*)sphere_tables_of<T>(sm).rsum, S, (const int32_t*)sm->sph_in,
                     (const uint32_t*)sm->pair_sph, (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col,
                     (const uint2*)m->ik_tri, m->n_jx, m->n_act, Y, Z, (sm->n_pair + 3) & ~3, A, Q);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "scene resolve kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

}  // namespace

extern "C" {

int dexr_sphere_resolve_scene_dev(const dexr_sphere_model* m, int64_t B, const float* x0, const float* fixed, const float* x_ref,
                                  const float* posture_weight, int32_t n_target, const float* target_pos, const float* target_rot,
                                  const float* pos_weight, const float* rot_weight, float margin, float collision_weight,
                                  const float* pair_weight, const float* lo, const float* hi, float damping, float max_step, float tol,
                                  int32_t max_iters, int32_t n_body, const dexr_scene_body* bodies, float* x_out, int32_t* iters_out,
                                  float* energy_out, float* body_energy_out, int32_t* status_out, void* stream) {
  const int c = check_resolve_scene_call(m, n_body, bodies, B, x0, fixed, n_target, target_pos, target_rot, pos_weight, rot_weight,
                                         (double)margin, (double)collision_weight, lo, hi, (double)damping, (double)max_step, (double)tol,
                                         max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const ResolveArgs<float> A = {x0, fixed, x_ref, posture_weight, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi,
                                margin, collision_weight, damping, max_step, tol, n_target, max_iters, x_out, iters_out, energy_out, status_out};
  return launch_resolve_scene<float>(m, B, A, scene_table<float>(n_body, bodies, body_energy_out), (hipStream_t)stream);
}

int dexr_sphere_resolve_scene(const dexr_sphere_model* m, int64_t B, const double* x0, const double* fixed, const double* x_ref,
                              const double* posture_weight, int32_t n_target, const double* target_pos, const double* target_rot,
                              const double* pos_weight, const double* rot_weight, double margin, double collision_weight,
                              const double* pair_weight, const double* lo, const double* hi, double damping, double max_step, double tol,
                              int32_t max_iters, int32_t n_body, const dexr_scene_body* bodies, double* x_out, int32_t* iters_out,
                              double* energy_out, double* body_energy_out, int32_t* status_out) {
  const int c = check_resolve_scene_call(m, n_body, bodies, B, x0, fixed, n_target, target_pos, target_rot, pos_weight, rot_weight, margin,
                                         collision_weight, lo, hi, damping, max_step, tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  ResolveRoundTrip D;
  ResolveArgs<double> A;
  if (const int rc = D.up(m, B, x0, fixed, x_ref, posture_weight, n_target, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi))
    return rc;
  DevBuf dop[DEXR_SCENE_MAXBODY], dor[DEXR_SCENE_MAXBODY], dow[DEXR_SCENE_MAXBODY], dbe;
  dexr_scene_body dev[DEXR_SCENE_MAXBODY];
  for (int b = 0; b < n_body; ++b) {
    dev[b] = bodies[b];
    if (dev[b].pos) POSE_HIP(dop[b].put(dev[b].pos, (size_t)B * 3 * sizeof(double)));
    if (dev[b].rot) POSE_HIP(dor[b].put(dev[b].rot, (size_t)B * 9 * sizeof(double)));
    if (dev[b].prim_weight) POSE_HIP(dow[b].put(dev[b].prim_weight, (size_t)dev[b].set->n_prim * sizeof(double)));
    dev[b].pos = dop[b].p, dev[b].rot = dor[b].p, dev[b].prim_weight = dow[b].p;
  }
  const size_t nbe = (size_t)B * n_body * sizeof(double);
  POSE_HIP(dbe.put(nullptr, nbe));
  if (const int rc = D.out(B, 4, margin, collision_weight, damping, max_step, tol, n_target, max_iters, &A)) return rc;
  if (const int rc = launch_resolve_scene<double>(m, B, A, scene_table<double>(n_body, dev, (double*)dbe.p), nullptr)) return rc;
  if (const int rc = D.down(x_out, iters_out, energy_out, status_out)) return rc;
  if (body_energy_out) POSE_HIP(hipMemcpy(body_energy_out, dbe.p, nbe, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

}  // extern "C"

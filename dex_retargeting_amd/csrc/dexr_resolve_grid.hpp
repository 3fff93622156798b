// dexr_resolve_grid.hpp -- the collision-aware posture solve against a sampled signed-distance field (include/dexr_resolve_grid.h):
// a fragment of dexr_pose.hip, which includes it once at its end, after the grid fragment.  The loop is resolve_contact_loop of
// dexr_resolve_obstacles.hpp (the phases of dexr_resolve.hpp with an obstacle term); this file adds GridContacts<T>, the contact
// source of a grid -- grid_sdf<T, true> with the GridD<T> descriptor (uniform data, by value) of the grid fragment --, the kernel
// pose_resolve_grid_kernel<T> that instantiates the loop with it, the launcher and the two entry points.
//
// GridContacts: the obstacle term of a sphere is ONE grid_sdf call, d = sdf - r, h = max(0, obstacle_margin - d), force h grad
// in the grid's frame, h^2 onto the partial energy, and ONE active flag byte in LDS at the CALLER's index of the sphere.  Counts
// are byte sums.  The contact list holds sorted sphere indices, a byte each, in the caller's sphere order: a sphere has at most
// one contact with a grid, so at most DEXR_SPHERE_MAX entries, nothing is capped and no status bit says so.  For the curvature
// the normal of a sphere is recomputed by grid_sdf from the parked centre and pose (the inputs and the function of phase B: the
// same bits); a zero gradient gives a zero row: energy only.  No input makes a load leave the samples: every lookup goes
// through grid_sdf and its clamps.
// The rule's constants are the header's, read in dexr_resolve.hpp where the rule stands: DEXR_RESOLVE_LAM_UP, DEXR_RESOLVE_LAM_DOWN
// and DEXR_RESOLVE_MAXREJECT in resolve_decide, DEXR_RESOLVE_MAXACTIVE in resolve_pair_total and resolve_list_pairs.
//
// LDS of a block: sixteen 64-bit partial frozen masks per frame | the fork slots | per frame a region [frame][stride], odd stride
// (ResolveLayout, then the obstacle pose and the sixteen partial obstacle energies) | per frame the active pairs, sixteen counts,
// six words of state, sixteen contact counts, the curvature contacts | per frame the contact list, a byte per sphere | per frame the
// active flags, a byte per sphere | per frame one byte per pair.  include/dexr_resolve_grid.h states the bytes.
#include "dexr_resolve_grid.h"

namespace {

template <typename T>
struct GridContacts {
  GridD<T> G;
  const float* V;
  unsigned char* clst;  // [sstride] the frame's contact list: sorted sphere indices, the caller's order
  unsigned char* act;   // [sstride] the frame's active flags, by the caller's sphere index

  static __host__ __device__ int sstride(int n_sphere) { return (n_sphere + 3) & ~3; }
  static __host__ __device__ int head_words(int) { return 0; }
  static __host__ __device__ int tail_bytes(int n_sphere) { return 2 * sstride(n_sphere); }

  __device__ __forceinline__ void place(const ResolveLds<T>& L, unsigned char* own, int n_sphere) {
    const int ss = sstride(n_sphere);
    clst = own + L.fr * ss;
    act = own + L.nl * ss + L.fr * ss;
  }

  // the term of the sphere of radius rs at yo (the grid's frame), c its caller's index: h grad sdf into fo, h^2 onto eo
  __device__ __forceinline__ void term(const ResolveObstacleArgs<T>& O, const T yo[3], T rs, int c, T& eo, T fo[3]) const {
    T gm[3];
    const T d = grid_sdf<T, true>(G, V, yo, gm) - rs;
    T h = O.omargin - d;
    if (h <= T(0)) h = T(0);  // (a comparison: a NaN stays a NaN)
    eo = fma(h, h, eo);
#pragma unroll
    for (int i = 0; i < 3; ++i) fo[i] = h * gm[i];
    act[c] = h > T(0) ? 1 : 0;
  }

  __device__ __forceinline__ int count(int c0, int c1) const {
    int n = 0;
    for (int c = c0; c < c1; ++c) n += act[c];
    return n;
  }

  __device__ __forceinline__ bool capped(int&) const { return false; }  // (at most n_sphere: nothing to cap)

  // the contacts of the caller's spheres [c0, c1) from entry coff on; coff stays below the number of flags set: < sstride
  __device__ __forceinline__ void append(int c0, int c1, int coff, const int32_t* __restrict__ sph_in) const {
    for (int c = c0; c < c1; ++c)
      if (act[c]) clst[coff++] = (unsigned char)sph_in[c];
  }

  // the q-th contact of the list: its sorted sphere, its world normal and its weight
  __device__ __forceinline__ void contact(const ResolveObstacleArgs<T>& O, const T* po, const T* cen, int q, int& si, T n[3], T& w) const {
    si = clst[q];
    T yo[3], gm[3];
    obstacle_point(po, cen + 3 * si, yo);
    (void)grid_sdf<T, true>(G, V, yo, gm);
    obstacle_to_world(po, gm, n);
    w = O.wobs;
  }
};

template <typename T>
__global__ void __launch_bounds__(SPH_FANOUT * SPH_FRAMES)
    pose_resolve_grid_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links, PoseArgs<T> P,
                             const SphereD<T>* __restrict__ spheres, const T* __restrict__ rsum, SphereIndex S,
                             const int32_t* __restrict__ sph_in, const uint32_t* __restrict__ pair_sph, const JacEnt* __restrict__ ents,
                             const uint32_t* __restrict__ act_rng, const int32_t* __restrict__ act_col, const uint2* __restrict__ tri,
                             GridD<T> G, const float* __restrict__ V, int n_jx, int n_act, ResolveLayout Y, int obase, int oebase, int fstride,
                             ResolveArgs<T> A, ResolveObstacleArgs<T> O) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const ResolveModel<T> M = {joints, links, spheres, rsum, S, pair_sph, ents, act_rng, act_col, tri, n_act, n_act * (n_act + 1) / 2};
  const GridContacts<T> C = {G, V, nullptr, nullptr};
  resolve_contact_loop<T>(pose_lds, M, P, sph_in, Y, obase, oebase, fstride, A, O, C);
}

template <typename T>
int launch_resolve_grid(const dexr_sphere_model* sm, const dexr_sdf_grid* gr, int64_t B, ResolveArgs<T> A, const ResolveObstacleArgs<T>& O,
                        hipStream_t st) {
  const dexr_pose_model* m = sm->pose;
  int obase, oebase;
  const ResolveLayout Y = resolve_contact_layout<T>(sm, A.n_target, &obase, &oebase);
  // (the formula of include/dexr_resolve_grid.h)
  const size_t per_frame = resolve_lds_bytes<T>(sm, Y, GridContacts<T>::head_words(sm->n_sphere),
                                                RESOLVE_CONTACT_COUNTS + GridContacts<T>::tail_bytes(sm->n_sphere));
  int nl;
  int64_t blocks;
  if (const int rc = resolve_launch_shape(per_frame, B, &nl, &blocks)) return rc;
  const SphereIndex S = {sm->link_sph, sm->sph_out, sm->inc_ptr, sm->inc, sm->n_sphere, sm->n_pair};
  if (!A.xref) A.xref = A.x0;
  hipLaunchKernelGGL(pose_resolve_grid_kernel<T>, dim3((unsigned)blocks), dim3(nl * SPH_FANOUT), per_frame * nl, st,
                     (const JointD<T>*)tables_of<T>(m).joints, (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B),
                     (const SphereD<T>*)sphere_tables_of<T>(sm).spheres, (const T*)sphere_tables_of<T>(sm).rsum, S, (const int32_t*)sm->sph_in,
                     (const uint32_t*)sm->pair_sph, (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_act_col,
                     (const uint2*)m->ik_tri, grid_desc_of<T>(gr), (const float*)gr->values, m->n_jx, m->n_act, Y, obase, oebase,
                     (sm->n_pair + 3) & ~3, A, O);
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
  const int c = check_resolve_contact_call(m, grid, "null sdf grid", (double)obstacle_margin, (double)obstacle_weight, B, x0, fixed, n_target,
                                           target_pos, target_rot, pos_weight, rot_weight, (double)margin, (double)collision_weight, lo, hi,
                                           (double)damping, (double)max_step, (double)tol, max_iters, x_out);
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
  const int c = check_resolve_contact_call(m, grid, "null sdf grid", obstacle_margin, obstacle_weight, B, x0, fixed, n_target, target_pos,
                                           target_rot, pos_weight, rot_weight, margin, collision_weight, lo, hi, damping, max_step, tol,
                                           max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  ResolveRoundTrip D;
  ResolveArgs<double> A;
  if (const int rc = D.up(m, B, x0, fixed, x_ref, posture_weight, n_target, target_pos, target_rot, pos_weight, rot_weight, pair_weight, lo, hi))
    return rc;
  DevBuf dop, dor;
  if (obstacle_pos) POSE_HIP(dop.put(obstacle_pos, (size_t)B * 3 * sizeof(double)));
  if (obstacle_rot) POSE_HIP(dor.put(obstacle_rot, (size_t)B * 9 * sizeof(double)));
  if (const int rc = D.out(B, 4, margin, collision_weight, damping, max_step, tol, n_target, max_iters, &A)) return rc;
  const ResolveObstacleArgs<double> O = {(const double*)dop.p, (const double*)dor.p, obstacle_margin, obstacle_weight};
  if (const int rc = launch_resolve_grid<double>(m, grid, B, A, O, nullptr)) return rc;
  return D.down(x_out, iters_out, energy_out, status_out);
}

}  // extern "C"

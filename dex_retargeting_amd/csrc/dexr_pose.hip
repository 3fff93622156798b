// dexr_pose.hip -- batched link poses (positions AND rotations of any set of links) and their vector-Jacobian product:
// the task-space half of differentiable retargeting (include/dexr_pose.h: table format and C ABI).
//
// MAPPING: one lane per frame, 64 frames per block.  The table (joint and link records, converted once at create time to
// the arithmetic type of the kernel) is read with wave-uniform indices, i.e. through scalar loads; a lane holds the running
// transform [R | p] of the joint it has just passed in registers.  The joints come in depth-first order, so the parent of
// joint k is joint k-1 except where the walk returns to a fork: the table compiler numbers the fork transforms that are alive
// at once (`save` / `restore` slots, children ordered smallest subtree first, so a 64-joint tree needs at most 6), and the
// kernel keeps those slots in LDS, laid out [value][lane] (bank = lane: conflict free).  Nothing is indexed at run time in
// registers, so nothing goes to scratch.
//
// Per joint the create step precomputes A = Rx, Bm = Rx K, C = Rx K^2 (K = skew(axis), Rx the placement's rotation), so that
//   Rx Rot(axis, q) = A + sin q Bm + (1 - cos q) C                               (Rodrigues, 18 fma)
//   R_k = R_parent (A + s Bm + (1 - c) C),   p_k = p_parent + R_parent (px + d xa)      (xa = Rx axis, d = q if prismatic)
//
// VJP (no Jacobian matrix): sweep 1 is the forward walk, and per link it forms the wrench about the world origin,
//   f_l = grad_pos_l,   t_l = p_l x f_l + sum_j R_l[:, j] x grad_rot_l[:, j],
// and parks it in LDS ([value][lane] again) at the link's SORTED position: links are sorted by parent joint and a subtree is
// a contiguous run of joints, hence the links below joint k are the contiguous range [link_begin, sub_link_end).  Sweep 2
// walks the joints again and at joint k sums that range (F, T0) and takes
//   dL/dq_k = a_k . (T0 - o_k x F)   (revolute; a_k world axis, o_k world origin)        a_k . F   (prismatic),
// then grad_x[col_k] (+)= mult_k dL/dq_k with plain loads / stores by the lane that owns the row (the first joint of a column
// stores, later ones -- mimic joints of the same variable -- read, add, store; columns no joint reads are zeroed).
//
// LINK JACOBIANS and LINK VELOCITIES (include/dexr_jacobian.h).  The velocity kernel is the forward walk with the running
// twist of the current joint frame beside the transform: v at the joint origin and w, carried to each new origin with
// w x dp, saved with the transform at a fork (six more values per slot, [value][lane] behind the transform slots), and
// at a joint driven by x advanced by mult xdot[col] a.  The Jacobian kernel has two phases in one block, because its
// output (n_link x 3 x n_in values per frame and block) dwarfs everything else and a lane-per-frame store loop would put
// kilobytes between the addresses of neighbouring lanes:
//   phase A (lane = frame)   walks the joints once and parks a_k, o_k of every joint driven by x and p_l (local frame: and
//                            R_l) of every link in LDS, laid out [lane][value] with an odd per-lane stride: a fixed value
//                            over the lanes hits every bank once, and so do consecutive values of one frame;
//   phase B (lane = element) after the barrier a lane owns the elements e, e + 256, ... of the (n_link, 3, n_in) block (the
//                            block has four threads per frame; three quarters of it sit out phase A); an
//                            element map built at create time gives (sorted link, row, column) of e without a division,
//                            and a CSR list the joints feeding the column.  The lane loops over the frames of the block
//                            (wave-uniform), sums mult (a x (p - o) | a) over the joints with link_begin <= l < sub_link_end
//                            and stores: 64 consecutive floats per instruction.
//
// LINK WRENCHES and the VJP of the LINK VELOCITIES (include/dexr_wrench.h): J^T applied to per-link cotangents, and the
// kinematic Hessian contracted on both sides, again without a matrix.  One kernel, two forms (pose_wrench_kernel<T, VEL>):
//   wrench form (VEL = false)  the pose VJP's two sweeps with other cargo: sweep 1 parks f_l and p_l x f_l + m_l (6 values per
//                              sorted link, [value][lane]), sweep 2 sums the range below each joint and projects it;
//   VJP form    (VEL = true)   both sweeps are the velocity walk (18 values per fork slot); sweep 1 parks f_l, m_l, p_l x f_l and
//                              A_l = v_l x f_l + w_l x m_l (12 values per link; 9 in the local frame, where A_l = 0), sweep 2
//                              takes both gradients of a joint from the five range sums and its own twist.
// The rate gradient of the VJP form is the wrench form's arithmetic operation by operation (rate_grad, cross_fma: explicit
// fma, nothing left to contraction), so the two agree bit for bit.
//
// DAMPED LEAST-SQUARES IK STEP (include/dexr_ik.h): dx = (J^T W J + lambda I)^-1 J^T W e of the Jacobians above, with neither J
// nor the normal matrix written to memory.  One kernel (pose_ik_kernel<T>), two phases in one block like the Jacobian kernel:
//   phase A (lane = frame)          the Jacobian kernel's walk: a_k, o_k per joint driven by x, and per sorted link p_l, the weighted
//                                   errors as a force and a moment in world axes and the two weights, in the frame's region of LDS;
//   phase B (16 threads per frame)  the packed lower triangle of H over the ACTIVE columns (those some joint reads: at most 64
//                                   whatever n_in is) and g, each entry summed by one thread over the joints of its columns and the
//                                   links below both; then a Cholesky factorisation and two triangular solves in LDS, one barrier
//                                   per column, and the scatter to dx with zeros in the columns no joint reads.
// Every sum has a fixed order that does not depend on the frames per block: a frame's row is the same bits at every B.
//
// IK SOLVE TO LINK POSE TARGETS (include/dexr_ik_solve.h): that step iterated inside one kernel (pose_ik_solve_kernel<T>), the same
// block and the same two phases with a loop around them.  A frame's current x lives in LDS and the walk reads it there; phase A
// also forms the errors towards the world targets, their sum E_k and the frame's stop decision; phase B sums g first, freezes the
// columns on a bound that g pushes outward (a 64-bit mask per frame in LDS, one more barrier), then builds H, solves, limits the
// step, moves and clamps.  A stopped frame keeps walking through the barriers without working or writing; the block leaves the
// loop on the AND of its frames' stop flags or at max_iters.  Phase B's sums and the factorisation are helpers both kernels call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "dexr.h"
#include "dexr_math.hpp"
#include "dexr_ik.h"
#include "dexr_ik_solve.h"
#include "dexr_jacobian.h"
#include "dexr_pose.h"
#include "dexr_wrench.h"

int dexr_set_error(int code, const char* fmt, ...);  // dexr_api.hip

namespace {

constexpr int POSE_BLOCK = 64;

template <typename T>
struct JointD {
  int32_t type, src_kind, src_col, restore, save, link_begin, link_end, sub_link_end, first_of_col, pad;
  T mult, off;
  T A[9], Bm[9], C[9], p[3], xa[3];
};

template <typename T>
struct LinkD {
  int32_t parent, out;
  T R[9], p[3];
};

template <typename T>
struct PoseArgs {
  int32_t n_joint, n_link, n_base, n_in, n_fixed, n_slot;
  uint64_t unused_lo, unused_hi, unused_2, unused_3;  // columns of x no joint reads (256 bits)
  int64_t B;
};

__device__ __forceinline__ void sincos_t(float a, float* s, float* c) { sincosf(a, s, c); }
__device__ __forceinline__ void sincos_t(double a, double* s, double* c) { dexr::sincos_f64(a, s, c); }

// running transform of a lane
template <typename T>
struct Xf {
  T R[9], p[3];
};

template <typename T>
__device__ __forceinline__ void slot_store(T* lds, int slot, int nl, int lane, const Xf<T>& t) {
  T* s = lds + (size_t)slot * 12 * nl + lane;
#pragma unroll
  for (int i = 0; i < 9; ++i) s[i * nl] = t.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) s[(9 + i) * nl] = t.p[i];
}

template <typename T>
__device__ __forceinline__ void slot_load(const T* lds, int slot, int nl, int lane, Xf<T>& t) {
  const T* s = lds + (size_t)slot * 12 * nl + lane;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.R[i] = s[i * nl];
#pragma unroll
  for (int i = 0; i < 3; ++i) t.p[i] = s[(9 + i) * nl];
}

// the three parts of one joint of the walk.  joint_restore: t becomes the transform of the joint's parent (the running one,
// the identity, or the fork's from its slot); joint_move: t -> transform of joint k, `a` receives the world axis of the joint
// (its origin is the new t.p); the save of a fork's transform is joint_step's last line
template <typename T>
__device__ __forceinline__ void joint_restore(const JointD<T>& J, const T* slots, int nl, int lane, Xf<T>& t) {
  if (J.restore == DEXR_POSE_ROOT) {
#pragma unroll
    for (int i = 0; i < 9; ++i) t.R[i] = (i % 4 == 0) ? T(1) : T(0);
    t.p[0] = t.p[1] = t.p[2] = T(0);
  } else if (J.restore >= 0) {
    slot_load(slots, J.restore, nl, lane, t);
  }
}

template <typename T>
__device__ __forceinline__ void joint_move(const JointD<T>& J, const PoseArgs<T>& P, const T* __restrict__ x,
                                           const T* __restrict__ fixed, int64_t b, Xf<T>& t, T a[3]) {
  T q = J.off;
  if (J.src_kind == DEXR_POSE_SRC_X) q = fma(J.mult, x[b * P.n_in + J.src_col], J.off);
  else if (J.src_kind == DEXR_POSE_SRC_FIXED) q = fma(J.mult, fixed[b * P.n_fixed + J.src_col], J.off);
  T M[9], pl[3];
  if (J.type == DEXR_POSE_REVOLUTE) {
    T s, c;
    sincos_t(q, &s, &c);
    const T v = T(1) - c;
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = fma(v, J.C[i], fma(s, J.Bm[i], J.A[i]));
#pragma unroll
    for (int i = 0; i < 3; ++i) pl[i] = J.p[i];
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = J.A[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pl[i] = fma(q, J.xa[i], J.p[i]);
  }
  Xf<T> n;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    n.p[i] = fma(t.R[3 * i + 2], pl[2], fma(t.R[3 * i + 1], pl[1], fma(t.R[3 * i], pl[0], t.p[i])));
    a[i] = fma(t.R[3 * i + 2], J.xa[2], fma(t.R[3 * i + 1], J.xa[1], t.R[3 * i] * J.xa[0]));
#pragma unroll
    for (int j = 0; j < 3; ++j)
      n.R[3 * i + j] = fma(t.R[3 * i + 2], M[6 + j], fma(t.R[3 * i + 1], M[3 + j], t.R[3 * i] * M[j]));
  }
  t = n;
}

// one joint of the walk: t (transform of the previous joint, or of the fork this joint hangs off) -> transform of joint k
template <typename T>
__device__ __forceinline__ void joint_step(const JointD<T>& J, const PoseArgs<T>& P, const T* __restrict__ x,
                                           const T* __restrict__ fixed, int64_t b, T* slots, int nl, int lane, Xf<T>& t,
                                           T a[3]) {
  joint_restore(J, slots, nl, lane, t);
  joint_move(J, P, x, fixed, b, t, a);
  if (J.save >= 0) slot_store(slots, J.save, nl, lane, t);
}

// world pose of a link hanging off the joint whose transform is t
template <typename T>
__device__ __forceinline__ void link_pose(const LinkD<T>& L, const Xf<T>& t, T R[9], T p[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p[i] = fma(t.R[3 * i + 2], L.p[2], fma(t.R[3 * i + 1], L.p[1], fma(t.R[3 * i], L.p[0], t.p[i])));
#pragma unroll
    for (int j = 0; j < 3; ++j)
      R[3 * i + j] = fma(t.R[3 * i + 2], L.R[6 + j], fma(t.R[3 * i + 1], L.R[3 + j], t.R[3 * i] * L.R[j]));
  }
}

template <typename T>
__global__ void __launch_bounds__(POSE_BLOCK) pose_forward_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                  PoseArgs<T> P, const T* __restrict__ x, const T* __restrict__ fixed,
                                                                  T* __restrict__ pos, T* __restrict__ rot) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  T* slots = reinterpret_cast<T*>(pose_lds);
  const int nl = blockDim.x, lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * nl + lane;
  const bool live = b0 < P.B;
  const int64_t b = live ? b0 : P.B - 1;  // ragged tail: idle lanes recompute the last frame and store nothing
  for (int l = 0; l < P.n_base; ++l) {    // links on the fixed base: their constant placement
    const LinkD<T>& L = links[l];
    if (live) {
      T* o = pos + (b * P.n_link + L.out) * 3;
#pragma unroll
      for (int i = 0; i < 3; ++i) o[i] = L.p[i];
      if (rot) {
        T* r = rot + (b * P.n_link + L.out) * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) r[i] = L.R[i];
      }
    }
  }
  Xf<T> t;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.R[i] = (i % 4 == 0) ? T(1) : T(0);
  t.p[0] = t.p[1] = t.p[2] = T(0);
  for (int k = 0; k < P.n_joint; ++k) {
    const JointD<T>& J = joints[k];
    T a[3];
    joint_step(J, P, x, fixed, b, slots, nl, lane, t, a);
    for (int l = J.link_begin; l < J.link_end; ++l) {
      const LinkD<T>& L = links[l];
      T R[9], p[3];
      link_pose(L, t, R, p);
      if (live) {
        T* o = pos + (b * P.n_link + L.out) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = p[i];
        if (rot) {
          T* r = rot + (b * P.n_link + L.out) * 9;
#pragma unroll
          for (int i = 0; i < 9; ++i) r[i] = R[i];
        }
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(POSE_BLOCK) pose_vjp_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                              PoseArgs<T> P, const T* __restrict__ x, const T* __restrict__ fixed,
                                                              const T* __restrict__ gpos, const T* __restrict__ grot,
                                                              T* __restrict__ gx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x, lane = threadIdx.x;
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* wr = slots + (size_t)P.n_slot * 12 * nl + lane;  // wrench of sorted link l: wr[(6 l + i) nl]
  const int64_t b0 = (int64_t)blockIdx.x * nl + lane;
  const bool live = b0 < P.B;
  const int64_t b = live ? b0 : P.B - 1;
  Xf<T> t;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.R[i] = (i % 4 == 0) ? T(1) : T(0);
  t.p[0] = t.p[1] = t.p[2] = T(0);
  // sweep 1: link poses -> link wrenches about the world origin
  for (int k = 0; k < P.n_joint; ++k) {
    const JointD<T>& J = joints[k];
    T a[3];
    joint_step(J, P, x, fixed, b, slots, nl, lane, t, a);
    for (int l = J.link_begin; l < J.link_end; ++l) {
      const LinkD<T>& L = links[l];
      T R[9], p[3], f[3] = {T(0), T(0), T(0)}, tq[3] = {T(0), T(0), T(0)};
      link_pose(L, t, R, p);
      if (gpos) {
        const T* g = gpos + (b * P.n_link + L.out) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i] = g[i];
        tq[0] = p[1] * f[2] - p[2] * f[1];
        tq[1] = p[2] * f[0] - p[0] * f[2];
        tq[2] = p[0] * f[1] - p[1] * f[0];
      }
      if (grot) {
        const T* g = grot + (b * P.n_link + L.out) * 9;
        T G[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) G[i] = g[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) {  // column j of R x column j of G
          tq[0] += R[3 + j] * G[6 + j] - R[6 + j] * G[3 + j];
          tq[1] += R[6 + j] * G[j] - R[j] * G[6 + j];
          tq[2] += R[j] * G[3 + j] - R[3 + j] * G[j];
        }
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        wr[(6 * l + i) * nl] = f[i];
        wr[(6 * l + 3 + i) * nl] = tq[i];
      }
    }
  }
  // columns of x that no joint reads: zero gradient
  for (int c = 0; c < P.n_in; ++c) {
    const uint64_t w = c < 64 ? P.unused_lo : (c < 128 ? P.unused_hi : (c < 192 ? P.unused_2 : P.unused_3));
    if (((w >> (c & 63)) & 1ull) && live) gx[b * P.n_in + c] = T(0);
  }
  // sweep 2: per joint the wrench of the links below it, projected on the joint's motion
  for (int k = 0; k < P.n_joint; ++k) {
    const JointD<T>& J = joints[k];
    T a[3];
    joint_step(J, P, x, fixed, b, slots, nl, lane, t, a);
    if (J.src_kind != DEXR_POSE_SRC_X) continue;
    T F[3] = {T(0), T(0), T(0)}, M[3] = {T(0), T(0), T(0)};
    for (int l = J.link_begin; l < J.sub_link_end; ++l) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        F[i] += wr[(6 * l + i) * nl];
        M[i] += wr[(6 * l + 3 + i) * nl];
      }
    }
    T g;
    if (J.type == DEXR_POSE_REVOLUTE) {
      const T* o = t.p;
      const T m0 = M[0] - (o[1] * F[2] - o[2] * F[1]);
      const T m1 = M[1] - (o[2] * F[0] - o[0] * F[2]);
      const T m2 = M[2] - (o[0] * F[1] - o[1] * F[0]);
      g = a[0] * m0 + a[1] * m1 + a[2] * m2;
    } else {
      g = a[0] * F[0] + a[1] * F[1] + a[2] * F[2];
    }
    g *= J.mult;
    if (live) {
      T* dst = gx + b * P.n_in + J.src_col;
      if (J.first_of_col) *dst = g;
      else *dst = *dst + g;
    }
  }
}

// ---- link velocities and link Jacobians (include/dexr_jacobian.h) ------------------------------------------------------
// a joint driven by x as phase B of the Jacobian kernel reads it: one record per (column, joint), grouped by column (CSR)
struct JacEnt {
  int32_t xi;                    // index among the joints driven by x: where phase A parked a, o
  int32_t link_begin, sub_end;   // sorted links below the joint
  int32_t type;
  double mult;
  float multf;
  int32_t pad;
};
__device__ __forceinline__ float mult_of(const JacEnt& e, float) { return e.multf; }
__device__ __forceinline__ double mult_of(const JacEnt& e, double) { return e.mult; }

// v (world axes) -> R^T v (the link's own axes)
template <typename T>
__device__ __forceinline__ void to_local(const T R[9], T v[3]) {
  const T v0 = v[0], v1 = v[1], v2 = v[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] = fma(R[6 + i], v2, fma(R[3 + i], v1, R[i] * v0));
}

template <typename T>
__global__ void __launch_bounds__(POSE_BLOCK) pose_velocity_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                   PoseArgs<T> P, const T* __restrict__ x, const T* __restrict__ fixed,
                                                                   const T* __restrict__ xdot, int frame, T* __restrict__ lin,
                                                                   T* __restrict__ ang) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x, lane = threadIdx.x;
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* tw = slots + (size_t)P.n_slot * 12 * nl + lane;  // twist of the fork in slot s: tw[(6 s + i) nl], v then w
  const int64_t b0 = (int64_t)blockIdx.x * nl + lane;
  const bool live = b0 < P.B;
  const int64_t b = live ? b0 : P.B - 1;
  for (int l = 0; l < P.n_base; ++l) {  // links on the fixed base do not move
    if (live) {
      const int64_t o = (b * P.n_link + links[l].out) * 3;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        if (lin) lin[o + i] = T(0);
        if (ang) ang[o + i] = T(0);
      }
    }
  }
  Xf<T> t;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.R[i] = (i % 4 == 0) ? T(1) : T(0);
  t.p[0] = t.p[1] = t.p[2] = T(0);
  T v[3] = {T(0), T(0), T(0)}, w[3] = {T(0), T(0), T(0)};  // velocity of the running frame's origin, angular velocity
  for (int k = 0; k < P.n_joint; ++k) {
    const JointD<T>& J = joints[k];
    joint_restore(J, slots, nl, lane, t);
    if (J.restore == DEXR_POSE_ROOT) {
      v[0] = v[1] = v[2] = w[0] = w[1] = w[2] = T(0);
    } else if (J.restore >= 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        v[i] = tw[(6 * J.restore + i) * nl];
        w[i] = tw[(6 * J.restore + 3 + i) * nl];
      }
    }
    const T po[3] = {t.p[0], t.p[1], t.p[2]};
    T a[3];
    joint_move(J, P, x, fixed, b, t, a);
    {  // the parent body's velocity at the new origin
      const T d0 = t.p[0] - po[0], d1 = t.p[1] - po[1], d2 = t.p[2] - po[2];
      v[0] += w[1] * d2 - w[2] * d1;
      v[1] += w[2] * d0 - w[0] * d2;
      v[2] += w[0] * d1 - w[1] * d0;
    }
    if (J.src_kind == DEXR_POSE_SRC_X) {
      const T qd = J.mult * xdot[b * P.n_in + J.src_col];
      if (J.type == DEXR_POSE_REVOLUTE) {
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = fma(qd, a[i], w[i]);
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = fma(qd, a[i], v[i]);
      }
    }
    if (J.save >= 0) {
      slot_store(slots, J.save, nl, lane, t);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        tw[(6 * J.save + i) * nl] = v[i];
        tw[(6 * J.save + 3 + i) * nl] = w[i];
      }
    }
    for (int l = J.link_begin; l < J.link_end; ++l) {
      const LinkD<T>& L = links[l];
      T R[9], p[3];
      link_pose(L, t, R, p);
      const T d0 = p[0] - t.p[0], d1 = p[1] - t.p[1], d2 = p[2] - t.p[2];
      T u[3] = {v[0] + (w[1] * d2 - w[2] * d1), v[1] + (w[2] * d0 - w[0] * d2), v[2] + (w[0] * d1 - w[1] * d0)};
      T wl[3] = {w[0], w[1], w[2]};
      if (frame == DEXR_JAC_LOCAL) {
        to_local(R, u);
        to_local(R, wl);
      }
      if (live) {
        const int64_t o = (b * P.n_link + L.out) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (lin) lin[o + i] = u[i];
          if (ang) ang[o + i] = wl[i];
        }
      }
    }
  }
}

// ---- link wrenches and the VJP of the link velocities (include/dexr_wrench.h) ------------------------------------------------
// R v (the link's own axes -> world axes)
template <typename T>
__device__ __forceinline__ void to_world(const T R[9], T v[3]) {
  const T v0 = v[0], v1 = v[1], v2 = v[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] = fma(R[3 * i + 2], v2, fma(R[3 * i + 1], v1, R[3 * i] * v0));
}

// c = a x b with the roundings spelled out (both forms of the kernel must round alike)
template <typename T>
__device__ __forceinline__ void cross_fma(const T a[3], const T b[3], T c[3]) {
  c[0] = fma(a[1], b[2], -(a[2] * b[1]));
  c[1] = fma(a[2], b[0], -(a[0] * b[2]));
  c[2] = fma(a[0], b[1], -(a[1] * b[0]));
}

template <typename T>
__device__ __forceinline__ T dot_fma(const T a[3], const T b[3]) {
  return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]));
}

// dL/dqd of one joint from the sums over the links below it: F = sum f, M = sum (p x f + m); oxF = o x F
template <typename T>
__device__ __forceinline__ T rate_grad(int type, const T a[3], const T F[3], const T M[3], const T oxF[3]) {
  if (type != DEXR_POSE_REVOLUTE) return dot_fma(a, F);
  const T r[3] = {M[0] - oxF[0], M[1] - oxF[1], M[2] - oxF[2]};
  return dot_fma(a, r);
}

// the lane that owns row b adds a joint's share to its column: the first joint of a column stores, later ones (mimic joints
// of the same variable) read, add, store
template <typename T>
__device__ __forceinline__ void column_add(T* __restrict__ row, int col, int first, T g) {
  T* dst = row + col;
  if (first) *dst = g;
  else *dst = *dst + g;
}

// one joint of the velocity walk: joint_step with the twist (v at the running origin, w) carried, advanced and saved along
template <typename T>
__device__ __forceinline__ void joint_step_twist(const JointD<T>& J, const PoseArgs<T>& P, const T* __restrict__ x,
                                                 const T* __restrict__ fixed, const T* __restrict__ xdot, int64_t b, T* slots,
                                                 T* tw, int nl, int lane, Xf<T>& t, T a[3], T v[3], T w[3]) {
  joint_restore(J, slots, nl, lane, t);
  if (J.restore == DEXR_POSE_ROOT) {
    v[0] = v[1] = v[2] = w[0] = w[1] = w[2] = T(0);
  } else if (J.restore >= 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      v[i] = tw[(6 * J.restore + i) * nl];
      w[i] = tw[(6 * J.restore + 3 + i) * nl];
    }
  }
  const T po[3] = {t.p[0], t.p[1], t.p[2]};
  joint_move(J, P, x, fixed, b, t, a);
  const T d[3] = {t.p[0] - po[0], t.p[1] - po[1], t.p[2] - po[2]};
  T wd[3];
  cross_fma(w, d, wd);  // the parent body's velocity at the new origin
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] += wd[i];
  if (J.src_kind == DEXR_POSE_SRC_X) {
    const T qd = J.mult * xdot[b * P.n_in + J.src_col];
    if (J.type == DEXR_POSE_REVOLUTE) {
#pragma unroll
      for (int i = 0; i < 3; ++i) w[i] = fma(qd, a[i], w[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) v[i] = fma(qd, a[i], v[i]);
    }
  }
  if (J.save >= 0) {
    slot_store(slots, J.save, nl, lane, t);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      tw[(6 * J.save + i) * nl] = v[i];
      tw[(6 * J.save + 3 + i) * nl] = w[i];
    }
  }
}

// VEL = false: tau = sum_l Jlin_l^T gl_l + Jang_l^T ga_l -> gxd (xdot and gx are not touched).
// VEL = true:  the VJP of (lin, ang) = link velocities at (x, xdot) for the cotangents (gl, ga): gx (never NULL here: a call
//              that asks for the rate gradient alone is served by the wrench form) and gxd (may be NULL).
template <typename T, bool VEL>
__global__ void __launch_bounds__(POSE_BLOCK) pose_wrench_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                 PoseArgs<T> P, const T* __restrict__ x, const T* __restrict__ fixed,
                                                                 const T* __restrict__ xdot, int frame, const T* __restrict__ gl,
                                                                 const T* __restrict__ ga, T* __restrict__ gx, T* __restrict__ gxd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x, lane = threadIdx.x;
  const bool local = frame == DEXR_JAC_LOCAL;
  const int per_link = VEL ? (local ? 9 : 12) : 6;  // f, then p x f + m (wrench form) | m, p x f, A (VJP form; no A in the local frame)
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* tw = slots + (size_t)P.n_slot * 12 * nl + lane;                     // VJP form: twist of the fork in slot s, v then w
  T* park = slots + (size_t)P.n_slot * (VEL ? 18 : 12) * nl + lane;      // record of sorted link l: park[(per_link l + i) nl]
  const int64_t b0 = (int64_t)blockIdx.x * nl + lane;
  const bool live = b0 < P.B;
  const int64_t b = live ? b0 : P.B - 1;  // ragged tail: idle lanes recompute the last frame and store nothing
  Xf<T> t;
#pragma unroll
  for (int i = 0; i < 9; ++i) t.R[i] = (i % 4 == 0) ? T(1) : T(0);
  t.p[0] = t.p[1] = t.p[2] = T(0);
  T v[3] = {T(0), T(0), T(0)}, w[3] = {T(0), T(0), T(0)};
  // sweep 1: per link the cotangents as a force and a moment in world axes, and what sweep 2 needs of the link beside them
  for (int k = 0; k < P.n_joint; ++k) {
    const JointD<T>& J = joints[k];
    T a[3];
    if (VEL) joint_step_twist(J, P, x, fixed, xdot, b, slots, tw, nl, lane, t, a, v, w);
    else joint_step(J, P, x, fixed, b, slots, nl, lane, t, a);
    for (int l = J.link_begin; l < J.link_end; ++l) {
      const LinkD<T>& L = links[l];
      T R[9], p[3], f[3] = {T(0), T(0), T(0)}, m[3] = {T(0), T(0), T(0)}, c[3];
      link_pose(L, t, R, p);
      const int64_t o = (b * P.n_link + L.out) * 3;
      if (gl) {
#pragma unroll
        for (int i = 0; i < 3; ++i) f[i] = gl[o + i];
        if (local) to_world(R, f);
      }
      if (ga) {
#pragma unroll
        for (int i = 0; i < 3; ++i) m[i] = ga[o + i];
        if (local) to_world(R, m);
      }
      cross_fma(p, f, c);
      T* rec = park + (size_t)per_link * l * nl;
#pragma unroll
      for (int i = 0; i < 3; ++i) rec[i * nl] = f[i];
      if (!VEL) {
#pragma unroll
        for (int i = 0; i < 3; ++i) rec[(3 + i) * nl] = c[i] + m[i];
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          rec[(3 + i) * nl] = m[i];
          rec[(6 + i) * nl] = c[i];
        }
        if (!local) {  // A_l = v_l x f_l + w_l x m_l, v_l the velocity of the link origin
          const T d[3] = {p[0] - t.p[0], p[1] - t.p[1], p[2] - t.p[2]};
          T u[3], uf[3], wm[3];
          cross_fma(w, d, u);
#pragma unroll
          for (int i = 0; i < 3; ++i) u[i] += v[i];
          cross_fma(u, f, uf);
          cross_fma(w, m, wm);
#pragma unroll
          for (int i = 0; i < 3; ++i) rec[(9 + i) * nl] = uf[i] + wm[i];
        }
      }
    }
  }
  // columns of x that no joint reads: zero gradient
  for (int c = 0; c < P.n_in; ++c) {
    const uint64_t u = c < 64 ? P.unused_lo : (c < 128 ? P.unused_hi : (c < 192 ? P.unused_2 : P.unused_3));
    if (((u >> (c & 63)) & 1ull) && live) {
      if (VEL) gx[b * P.n_in + c] = T(0);
      if (gxd) gxd[b * P.n_in + c] = T(0);
    }
  }
  // sweep 2: per joint the sums over the links below it, projected on the joint's motion and on its motion's rate of change
  for (int k = 0; k < P.n_joint; ++k) {
    const JointD<T>& J = joints[k];
    T a[3];
    if (VEL) joint_step_twist(J, P, x, fixed, xdot, b, slots, tw, nl, lane, t, a, v, w);
    else joint_step(J, P, x, fixed, b, slots, nl, lane, t, a);
    if (J.src_kind != DEXR_POSE_SRC_X) continue;
    T F[3] = {T(0), T(0), T(0)}, M[3] = {T(0), T(0), T(0)};                             // sum f, sum (p x f + m)
    T G[3] = {T(0), T(0), T(0)}, C[3] = {T(0), T(0), T(0)}, A[3] = {T(0), T(0), T(0)};  // VJP form: sum m, sum p x f, sum A
    for (int l = J.link_begin; l < J.sub_link_end; ++l) {
      const T* rec = park + (size_t)per_link * l * nl;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        F[i] += rec[i * nl];
        if (!VEL) {
          M[i] += rec[(3 + i) * nl];
        } else {
          const T mi = rec[(3 + i) * nl], ci = rec[(6 + i) * nl];
          M[i] += ci + mi;
          G[i] += mi;
          C[i] += ci;
          if (!local) A[i] += rec[(9 + i) * nl];
        }
      }
    }
    T oxF[3];
    cross_fma(t.p, F, oxF);
    if (gxd) {
      const T g = J.mult * rate_grad(J.type, a, F, M, oxF);
      if (live) column_add(gxd + b * P.n_in, J.src_col, J.first_of_col, g);
    }
    if (VEL) {
      T wa[3], g;
      cross_fma(w, a, wa);
      if (J.type == DEXR_POSE_REVOLUTE) {
        T vf[3], wg[3];
        cross_fma(v, F, vf);
        cross_fma(w, G, wg);
        const T r[3] = {A[0] - vf[0] - wg[0], A[1] - vf[1] - wg[1], A[2] - vf[2] - wg[2]};
        const T arm[3] = {C[0] - oxF[0], C[1] - oxF[1], C[2] - oxF[2]};
        g = dot_fma(a, r) + dot_fma(wa, arm);
      } else {
        g = dot_fma(wa, F);
      }
      g *= J.mult;
      if (live) column_add(gx + b * P.n_in, J.src_col, J.first_of_col, g);
    }
  }
}

// one joint's share of element (sorted link ls, row r) of the two blocks, from the values phase A parked for one frame
// (added to the sums by value: a sum handed down by reference ends up in scratch)
template <typename T>
struct JacShare {
  T lin, ang;
};

template <typename T>
__device__ __forceinline__ JacShare<T> jac_share(const JacEnt& e, const T* pk, int lbase, int lstride, int ls, int r, int frame) {
  JacShare<T> s = {T(0), T(0)};
  if (ls < e.link_begin || ls >= e.sub_end) return s;
  const T* a = pk + 6 * e.xi;               // a[0..2] world axis, a[3..5] world origin
  const T* pl = pk + lbase + ls * lstride;  // p_l, then R_l row-major (local frame only)
  const bool rev = e.type == DEXR_POSE_REVOLUTE;
  T lin, ax;  // a x (p - o) and a, row r in the asked frame
  if (frame == DEXR_JAC_WORLD_ALIGNED) {
    ax = a[r];
    lin = ax;
    if (rev) {
      const int r1 = r == 2 ? 0 : r + 1, r2 = r == 0 ? 2 : r - 1;
      const T d1 = pl[r1] - a[3 + r1], d2 = pl[r2] - a[3 + r2];
      lin = a[r1] * d2 - a[r2] * d1;
    }
  } else {
    const T a0 = a[0], a1 = a[1], a2 = a[2];
    const T R0 = pl[3 + r], R1 = pl[6 + r], R2 = pl[9 + r];  // column r of R_l
    ax = fma(R2, a2, fma(R1, a1, R0 * a0));
    lin = ax;
    if (rev) {
      const T d0 = pl[0] - a[3], d1 = pl[1] - a[4], d2 = pl[2] - a[5];
      lin = fma(R2, a0 * d1 - a1 * d0, fma(R1, a2 * d0 - a0 * d2, R0 * (a1 * d2 - a2 * d1)));
    }
  }
  const T m = mult_of(e, T(0));
  s.lin = m * lin;
  s.ang = rev ? m * ax : T(0);
  return s;
}

// threads of a Jacobian block per frame it holds: phase A runs on the first quarter of the block (lane = frame), phase B on
// all of it -- the LDS a block needs is set by its frames, so the three waves that sit out phase A cost none and are what
// overlaps the LDS reads of phase B
constexpr int JAC_FANOUT = 4;

template <typename T>
__global__ void __launch_bounds__(POSE_BLOCK * JAC_FANOUT) pose_jacobian_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                   PoseArgs<T> P, const int32_t* __restrict__ colptr,
                                                                   const JacEnt* __restrict__ ents, const uint32_t* __restrict__ emap,
                                                                   int n_jx, int stride, int frame, const T* __restrict__ x,
                                                                   const T* __restrict__ fixed, T* __restrict__ jlin, T* __restrict__ jang) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / JAC_FANOUT, lane = threadIdx.x;  // nl: frames of this block
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* park = slots + (size_t)P.n_slot * 12 * nl;  // [lane][stride], stride odd
  const int lstride = frame == DEXR_JAC_LOCAL ? 12 : 3, lbase = 6 * n_jx;
  const int64_t first = (int64_t)blockIdx.x * nl;
  if (lane < nl) {  // phase A: lane = frame
    T* pk = park + (size_t)lane * stride;
    const int64_t b = first + lane < P.B ? first + lane : P.B - 1;  // ragged tail: idle lanes park the last frame again
    for (int l = 0; l < P.n_base; ++l) {
      const LinkD<T>& L = links[l];
      T* d = pk + lbase + l * lstride;
#pragma unroll
      for (int i = 0; i < 3; ++i) d[i] = L.p[i];
      if (frame == DEXR_JAC_LOCAL) {
#pragma unroll
        for (int i = 0; i < 9; ++i) d[3 + i] = L.R[i];
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
      if (J.src_kind == DEXR_POSE_SRC_X) {
        T* d = pk + 6 * xi;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          d[i] = a[i];
          d[3 + i] = t.p[i];
        }
        ++xi;
      }
      for (int l = J.link_begin; l < J.link_end; ++l) {
        const LinkD<T>& L = links[l];
        T R[9], p[3];
        link_pose(L, t, R, p);
        T* d = pk + lbase + l * lstride;
#pragma unroll
        for (int i = 0; i < 3; ++i) d[i] = p[i];
        if (frame == DEXR_JAC_LOCAL) {
#pragma unroll
          for (int i = 0; i < 9; ++i) d[3 + i] = R[i];
        }
      }
    }
  }
  __syncthreads();
  // phase B: lane = element of the (n_link, 3, n_in) block, frames of this block one after the other
  const int E = P.n_link * 3 * P.n_in;
  const int64_t left = P.B - first;
  const int frames = left < nl ? (int)left : nl;
  for (int e = lane; e < E; e += nl * JAC_FANOUT) {
    const uint32_t u = emap[e];
    const int ls = u & 63, r = (u >> 6) & 3, c = u >> 8;
    const int i0 = colptr[c], i1 = colptr[c + 1];
    JacEnt e0 = {0, 0, 0, 0, 0.0, 0.f, 0};  // the first joint of the column stays in registers over the frames (more: mimic joints)
    if (i0 < i1) e0 = ents[i0];
    for (int f = 0; f < frames; ++f) {
      const T* pk = park + (size_t)f * stride;
      const JacShare<T> s0 = jac_share(e0, pk, lbase, lstride, ls, r, frame);
      T sl = s0.lin, sa = s0.ang;
      for (int i = i0 + 1; i < i1; ++i) {
        const JacShare<T> si = jac_share(ents[i], pk, lbase, lstride, ls, r, frame);
        sl += si.lin;
        sa += si.ang;
      }
      const int64_t o = (first + f) * E + e;
      if (jlin) jlin[o] = sl;
      if (jang) jang[o] = sa;
    }
  }
}

// ---- damped least-squares IK step (include/dexr_ik.h) --------------------------------------------------------------------------
// threads of an IK block per frame it holds, and the most frames it holds (256 threads).  Phase A runs on the first
// IK_FRAMES lanes at most (lane = frame), phase B on all of the block: the IK_FANOUT threads of a frame sit in one wave
constexpr int IK_FANOUT = 16;
constexpr int IK_FRAMES = 16;
constexpr int IK_LINK = 11;  // values parked per sorted link: p_l, f_l, m_l (world axes, weighted), w_lin, w_ang

// c = a x (p - o) (revolute) | a (prismatic): the linear column of one joint at one link, world axes, before its multiplier
template <typename T>
__device__ __forceinline__ void ik_column(const T* a, bool rev, const T* p, T c[3]) {
  if (rev) {
    const T d[3] = {p[0] - a[3], p[1] - a[4], p[2] - a[5]};
    const T ax[3] = {a[0], a[1], a[2]};
    cross_fma(ax, d, c);
  } else {
    c[0] = a[0];
    c[1] = a[1];
    c[2] = a[2];
  }
}

// entry (i, j), i >= j, of the packed lower triangle of H before the damping, from what phase A parked for the frame (pk): summed
// over the joints of the two columns and the links below both.  d.x: i | j << 6; d.y: the entries of column i, of column j (both
// empty where no link is below both)
template <typename T>
__device__ __forceinline__ T ik_h_entry(const uint2 d, const JacEnt* __restrict__ ents, const T* pk, int lbase) {
  const int i0 = d.y & 255, i1 = (d.y >> 8) & 255, j0 = (d.y >> 16) & 255, j1 = d.y >> 24;
  T s = T(0);
  for (int ii = i0; ii < i1; ++ii) {
    const JacEnt A = ents[ii];
    const T* a = pk + 6 * A.xi;
    const bool arev = A.type == DEXR_POSE_REVOLUTE;
    for (int jj = j0; jj < j1; ++jj) {
      const JacEnt Bn = ents[jj];
      const int lo = A.link_begin > Bn.link_begin ? A.link_begin : Bn.link_begin;
      const int hi = A.sub_end < Bn.sub_end ? A.sub_end : Bn.sub_end;
      if (lo >= hi) continue;
      const T* c = pk + 6 * Bn.xi;
      const bool brev = Bn.type == DEXR_POSE_REVOLUTE;
      const T mm = mult_of(A, T(0)) * mult_of(Bn, T(0));
      const T aa = (arev && brev) ? dot_fma(a, c) : T(0);
      T sl = T(0);
      for (int l = lo; l < hi; ++l) {
        const T* q = pk + lbase + IK_LINK * l;
        T u[3], v[3];
        ik_column(a, arev, q, u);
        ik_column(c, brev, q, v);
        sl = fma(q[9], dot_fma(u, v), fma(q[10], aa, sl));
      }
      s = fma(mm, sl, s);
    }
  }
  return s;
}

// entry of g of the active column whose entries are r (first | end << 8)
template <typename T>
__device__ __forceinline__ T ik_g_entry(uint32_t r, const JacEnt* __restrict__ ents, const T* pk, int lbase) {
  T s = T(0);
  for (int ii = r & 255; ii < (int)(r >> 8); ++ii) {
    const JacEnt A = ents[ii];
    const T* a = pk + 6 * A.xi;
    const bool arev = A.type == DEXR_POSE_REVOLUTE;
    T sl = T(0);
    for (int l = A.link_begin; l < A.sub_end; ++l) {
      const T* q = pk + lbase + IK_LINK * l;
      T u[3];
      ik_column(a, arev, q, u);
      sl += dot_fma(u, q + 3);
      if (arev) sl += dot_fma(a, q + 6);
    }
    s = fma(mult_of(A, T(0)), sl, s);
  }
  return s;
}

// H (packed lower triangle) -> its Cholesky factor below the diagonal and dg, then L y = g and L^T dx = y: dx takes the place of
// g.  One barrier per column and sweep, 3 n_act in all, reached by every thread of the block whatever `work` is: a frame that
// has nothing to solve passes work = false and only keeps the barriers
template <typename T>
__device__ __forceinline__ void ik_factor_solve(T* H, T* g, T* y, T* dg, int n_act, int t, bool work) {
  // Cholesky, one column per step: every thread of the frame forms the pivot itself (row k is complete), then its rows
  for (int k = 0; k < n_act; ++k) {
    if (work) {
      const T* rk = H + k * (k + 1) / 2;
      T skk = rk[k];
      for (int p = 0; p < k; ++p) skk = fma(-rk[p], rk[p], skk);
      const T d = sqrt(skk);
      if (t == 0) dg[k] = d;
      for (int i = k + 1 + t; i < n_act; i += IK_FANOUT) {
        T* ri = H + i * (i + 1) / 2;
        T s = ri[k];
        for (int p = 0; p < k; ++p) s = fma(-ri[p], rk[p], s);
        ri[k] = s / d;
      }
    }
    __syncthreads();
  }
  // L y = g, by columns
  for (int k = 0; k < n_act; ++k) {
    if (work) {
      const T yk = g[k] / dg[k];
      if (t == 0) y[k] = yk;
      for (int i = k + 1 + t; i < n_act; i += IK_FANOUT) g[i] = fma(-H[i * (i + 1) / 2 + k], yk, g[i]);
    }
    __syncthreads();
  }
  // L^T dx = y, by rows of L from the last; dx takes the place of g
  for (int k = n_act - 1; k >= 0; --k) {
    if (work) {
      const T zk = y[k] / dg[k];
      if (t == 0) g[k] = zk;
      const T* rk = H + k * (k + 1) / 2;
      for (int p = t; p < k; p += IK_FANOUT) y[p] = fma(-rk[p], zk, y[p]);
    }
    __syncthreads();
  }
}

// Per frame one region of LDS, [frame][stride] with an odd stride: a, o per joint driven by x | IK_LINK values per sorted link |
// H, the packed lower triangle over the active columns (row i starts at i (i + 1) / 2), overwritten by its Cholesky factor below
// the diagonal | g (later dx) | y | the factor's diagonal.  Every entry of H and g is summed by one thread in table order, and
// the factorisation and the solves walk the columns in order with one barrier each: no sum depends on the launch shape.
template <typename T>
__global__ void __launch_bounds__(IK_FANOUT * IK_FRAMES) pose_ik_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                       PoseArgs<T> P, const JacEnt* __restrict__ ents,
                                                                       const uint32_t* __restrict__ act_rng,
                                                                       const int32_t* __restrict__ col_act, const uint2* __restrict__ tri,
                                                                       int n_jx, int n_act, int stride, int frame, const T* __restrict__ x,
                                                                       const T* __restrict__ fixed, const T* __restrict__ el,
                                                                       const T* __restrict__ ea, const T* __restrict__ wl,
                                                                       const T* __restrict__ wa, T lambda, T* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / IK_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  T* slots = reinterpret_cast<T*>(pose_lds);
  T* park = slots + (size_t)P.n_slot * 12 * nl;
  const int lbase = 6 * n_jx, n_tri = n_act * (n_act + 1) / 2;
  const int hbase = lbase + IK_LINK * P.n_link, gbase = hbase + n_tri, ybase = gbase + n_act, dbase = ybase + n_act;
  const int64_t first = (int64_t)blockIdx.x * nl;
  if (tid < nl) {  // phase A: lane = frame
    const int lane = tid;
    const bool local = frame == DEXR_JAC_LOCAL;
    T* pk = park + (size_t)lane * stride;
    const int64_t b = first + lane < P.B ? first + lane : P.B - 1;  // ragged tail: idle lanes park the last frame again
    Xf<T> t;
#pragma unroll
    for (int i = 0; i < 9; ++i) t.R[i] = (i % 4 == 0) ? T(1) : T(0);
    t.p[0] = t.p[1] = t.p[2] = T(0);
    int xi = 0;
    for (int k = 0; k < P.n_joint; ++k) {  // (links on the fixed base are below no joint: phase B never reads their records)
      const JointD<T>& J = joints[k];
      T a[3];
      joint_step(J, P, x, fixed, b, slots, nl, lane, t, a);
      if (J.src_kind == DEXR_POSE_SRC_X) {
        T* d = pk + 6 * xi;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          d[i] = a[i];
          d[3 + i] = t.p[i];
        }
        ++xi;
      }
      for (int l = J.link_begin; l < J.link_end; ++l) {
        const LinkD<T>& L = links[l];
        T R[9], p[3], f[3] = {T(0), T(0), T(0)}, m[3] = {T(0), T(0), T(0)}, wf = T(0), wm = T(0);
        link_pose(L, t, R, p);
        const int64_t row = b * P.n_link + L.out;
        if (el) {
          wf = wl ? wl[row] : T(1);
#pragma unroll
          for (int i = 0; i < 3; ++i) f[i] = el[row * 3 + i];
          if (local) to_world(R, f);
#pragma unroll
          for (int i = 0; i < 3; ++i) f[i] *= wf;
        }
        if (ea) {
          wm = wa ? wa[row] : T(1);
#pragma unroll
          for (int i = 0; i < 3; ++i) m[i] = ea[row * 3 + i];
          if (local) to_world(R, m);
#pragma unroll
          for (int i = 0; i < 3; ++i) m[i] *= wm;
        }
        T* d = pk + lbase + IK_LINK * l;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          d[i] = p[i];
          d[3 + i] = f[i];
          d[6 + i] = m[i];
        }
        d[9] = wf;
        d[10] = wm;
      }
    }
  }
  __syncthreads();
  // phase B: IK_FANOUT threads per frame
  const int fr = tid / IK_FANOUT, t = tid % IK_FANOUT;
  T* pk = park + (size_t)fr * stride;
  T* H = pk + hbase;
  T* g = pk + gbase;
  T* y = pk + ybase;
  T* dg = pk + dbase;
  for (int e = t; e < n_tri; e += IK_FANOUT) {  // H[i, j], i >= j: the joints of the two columns, the links below both
    const uint2 d = tri[e];
    const T s = ik_h_entry(d, ents, pk, lbase);
    H[e] = (d.x & 63) == (d.x >> 6) ? s + lambda : s;
  }
  for (int i = t; i < n_act; i += IK_FANOUT) g[i] = ik_g_entry(act_rng[i], ents, pk, lbase);
  __syncthreads();
  ik_factor_solve(H, g, y, dg, n_act, t, true);
  if (first + fr < P.B) {
    T* o = dx + (first + fr) * P.n_in;
    for (int c = t; c < P.n_in; c += IK_FANOUT) {
      const int a = col_act[c];
      o[c] = a >= 0 ? g[a] : T(0);
    }
  }
}

// ---- IK solve to link pose targets (include/dexr_ik_solve.h): the step kernel's two phases inside an iteration loop ------------------
__device__ __forceinline__ float atan2_t(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double atan2_t(double y, double x) { return atan2(y, x); }

// phase A's share of one link at world pose (R, p): its errors towards the target row, parked as the step kernel parks them (d:
// p_l, the weighted errors as a force and a moment in world axes, the two weights); returns w_lin |e_lin|^2 + w_ang |e_ang|^2
template <typename T>
__device__ __forceinline__ T ik_link_target(const T R[9], const T p[3], int64_t row, const T* __restrict__ tp, const T* __restrict__ tr,
                                            const T* __restrict__ wl, const T* __restrict__ wa, T* d) {
  T f[3] = {T(0), T(0), T(0)}, m[3] = {T(0), T(0), T(0)}, wf = T(0), wm = T(0), E = T(0);
  if (tp) {
    wf = wl ? wl[row] : T(1);
    T e[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      e[i] = tp[row * 3 + i] - p[i];
      f[i] = e[i] * wf;
    }
    E = wf * dot_fma(e, e);
  }
  if (tr) {
    wm = wa ? wa[row] : T(1);
    const T* G = tr + row * 9;
    T M[9];  // M = G R^T: the rotation that takes the link to its target, in world axes
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[3 * i + j] = fma(G[3 * i + 2], R[3 * j + 2], fma(G[3 * i + 1], R[3 * j + 1], G[3 * i] * R[3 * j]));
    const T v[3] = {T(0.5) * (M[7] - M[5]), T(0.5) * (M[2] - M[6]), T(0.5) * (M[3] - M[1])};
    const T c = T(0.5) * (M[0] + M[4] + M[8] - T(1)), s = sqrt(dot_fma(v, v));
    const T k = s > T(1e-6) ? atan2_t(s, c) / s : T(1);
    T e[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      e[i] = v[i] * k;
      m[i] = e[i] * wm;
    }
    E = fma(wm, dot_fma(e, e), E);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    d[i] = p[i];
    d[3 + i] = f[i];
    d[6 + i] = m[i];
  }
  d[9] = wf;
  d[10] = wm;
  return E;
}

// LDS of a block: the sixteen partial frozen masks of every frame (64 bits each: thread t holds the bits of the active columns
// t, t + 16, ...; their OR is the frame's mask) | a stop flag and an iteration count per frame | the fork slots | per frame the
// step kernel's region with the frame's current x (all n_in columns) and E behind it.  The walk reads x from LDS through
// joint_move unchanged: row stride `stride`, row index = lane.
//
// THE LOOP CANNOT HANG: it runs k = 0 .. max_iters at most; every barrier sits outside every condition that differs between the
// threads of a block (4 + 3 n_act per iteration); a frame that has stopped (or an idle lane of a ragged last block: stopped from
// the start) does no work and writes nothing but walks through the same barriers; the one early exit is taken on the AND of all
// stop flags of the block, which every thread reads from LDS after the same barrier, and at k == max_iters every flag is set.
template <typename T>
__global__ void __launch_bounds__(IK_FANOUT * IK_FRAMES) pose_ik_solve_kernel(const JointD<T>* __restrict__ joints, const LinkD<T>* __restrict__ links,
                                                                             PoseArgs<T> P, const JacEnt* __restrict__ ents,
                                                                             const uint32_t* __restrict__ act_rng,
                                                                             const int32_t* __restrict__ act_col, const uint2* __restrict__ tri,
                                                                             int n_jx, int n_act, int stride, const T* x0,
                                                                             const T* __restrict__ fixed, const T* __restrict__ tp,
                                                                             const T* __restrict__ tr, const T* __restrict__ wl,
                                                                             const T* __restrict__ wa, const T* __restrict__ lo,
                                                                             const T* __restrict__ hi, T lambda, T max_step, T tol2,
                                                                             int max_iters, T* x_out, int32_t* __restrict__ iters_out,
                                                                             T* __restrict__ err_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pose_lds[];
  const int nl = blockDim.x / IK_FANOUT, tid = threadIdx.x;  // nl: frames of this block
  unsigned long long* part = reinterpret_cast<unsigned long long*>(pose_lds);  // [nl][IK_FANOUT]
  int32_t* stopf = reinterpret_cast<int32_t*>(part + nl * IK_FANOUT);           // [nl]
  int32_t* itv = stopf + nl;                                                    // [nl]
  T* slots = reinterpret_cast<T*>(itv + nl);
  T* park = slots + (size_t)P.n_slot * 12 * nl;
  const int lbase = 6 * n_jx, n_tri = n_act * (n_act + 1) / 2;
  const int hbase = lbase + IK_LINK * P.n_link, gbase = hbase + n_tri, ybase = gbase + n_act, dbase = ybase + n_act;
  const int xbase = dbase + n_act, ebase = xbase + P.n_in;
  const int64_t first = (int64_t)blockIdx.x * nl;
  const int fr = tid / IK_FANOUT, t = tid % IK_FANOUT;
  const bool inb = first + fr < P.B;
  T* pk = park + (size_t)fr * stride;
  T* H = pk + hbase;
  T* g = pk + gbase;
  T* y = pk + ybase;
  T* dg = pk + dbase;
  T* xs = pk + xbase;
  for (int c = t; c < P.n_in; c += IK_FANOUT) xs[c] = inb ? x0[(first + fr) * P.n_in + c] : T(0);
  bool stopped = first + tid >= P.B;  // (read by the walking lanes alone) idle lanes of a ragged last block never start
  if (tid < nl) {
    stopf[tid] = stopped ? 1 : 0;
    itv[tid] = 0;
    park[(size_t)tid * stride + ebase] = T(0);
  }
  __syncthreads();
  PoseArgs<T> PL = P;  // the walk's view of x: the frames' rows in LDS
  PL.n_in = stride;
  const T* xl = park + xbase;
  const T* fixl = fixed + first * P.n_fixed;
  for (int k = 0; k <= max_iters; ++k) {
    if (tid < nl && !stopped) {  // phase A: lane = frame; FK at x_k, the errors, E_k and the stop test
      const int lane = tid;
      T* pa = park + (size_t)lane * stride;
      const int64_t b = first + lane;
      T E = T(0);
      for (int l = 0; l < P.n_base; ++l) {  // links on the fixed base: below no joint, but their error counts
        const LinkD<T>& L = links[l];
        E += ik_link_target(L.R, L.p, b * P.n_link + L.out, tp, tr, wl, wa, pa + lbase + IK_LINK * l);
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
          const LinkD<T>& L = links[l];
          T R[9], p[3];
          link_pose(L, tf, R, p);
          E += ik_link_target(R, p, b * P.n_link + L.out, tp, tr, wl, wa, pa + lbase + IK_LINK * l);
        }
      }
      itv[lane] = k;
      pa[ebase] = E;
      if (E <= tol2 || k == max_iters) {  // (a NaN compares false: a spoiled frame runs to max_iters)
        stopped = true;
        stopf[lane] = 1;
      }
    }
    __syncthreads();
    bool all = true;  // the block's vote, the same in every thread
    for (int f = 0; f < nl; ++f) all = all && stopf[f] != 0;
    if (all) break;
    const bool work = stopf[fr] == 0;
    // phase B: g first, with the freeze test of its columns
    unsigned long long mine = 0;
    if (work) {
      for (int i = t; i < n_act; i += IK_FANOUT) {
        T s = ik_g_entry(act_rng[i], ents, pk, lbase);
        if (lo) {
          const int c = act_col[i];
          const T xc = xs[c];
          if ((xc <= lo[c] && s < T(0)) || (xc >= hi[c] && s > T(0))) {
            mine |= 1ull << i;
            s = T(0);
          }
        }
        g[i] = s;
      }
    }
    part[fr * IK_FANOUT + t] = mine;
    __syncthreads();
    unsigned long long frozen = 0;
    for (int u = 0; u < IK_FANOUT; ++u) frozen |= part[fr * IK_FANOUT + u];
    if (work) {
      for (int e = t; e < n_tri; e += IK_FANOUT) {  // a frozen column's row and column of H are the identity's
        const uint2 d = tri[e];
        const int i = d.x & 63, j = d.x >> 6;
        T h;
        if (((frozen >> i) | (frozen >> j)) & 1ull) {
          h = i == j ? T(1) : T(0);
        } else {
          h = ik_h_entry(d, ents, pk, lbase);
          if (i == j) h += lambda;
        }
        H[e] = h;
      }
    }
    __syncthreads();
    ik_factor_solve(H, g, y, dg, n_act, t, work);
    if (work) {  // limit the step, move, clamp: by comparisons, a NaN stays a NaN
      T scale = T(1);
      if (max_step > T(0)) {
        T m = T(0);
        for (int i = 0; i < n_act; ++i) {
          const T a = fabs(g[i]);
          m = a > m ? a : m;
        }
        if (m > max_step) scale = max_step / m;
      }
      for (int i = t; i < n_act; i += IK_FANOUT) {
        const int c = act_col[i];
        T v = xs[c] + g[i] * scale;
        if (lo) {
          const T l = lo[c], h = hi[c];
          v = v < l ? l : (v > h ? h : v);
        }
        xs[c] = v;
      }
    }
    __syncthreads();
  }
  if (inb) {
    T* o = x_out + (first + fr) * P.n_in;
    for (int c = t; c < P.n_in; c += IK_FANOUT) o[c] = xs[c];
    if (t == 0) {
      if (iters_out) iters_out[first + fr] = itv[fr];
      if (err_out) err_out[first + fr] = sqrt(pk[ebase]);
    }
  }
}

template <typename T>
struct DevTables {
  JointD<T>* joints = nullptr;
  LinkD<T>* links = nullptr;
};

}  // namespace

struct dexr_pose_model {
  dexr_pose_header h;
  int n_base = 0;
  uint64_t unused[4] = {0, 0, 0, 0};
  DevTables<float> f32;
  DevTables<double> f64;
  // index data of the Jacobian kernel, derived from the joint records at create time
  int n_jx = 0;                // joints driven by x
  int32_t* jac_colptr = nullptr;  // (n_in + 1)
  JacEnt* jac_ents = nullptr;     // (n_jx), grouped by column
  uint32_t* jac_emap = nullptr;   // (n_link 3 n_in): sorted link | row << 6 | column << 8 of an output element
  // index data of the IK kernel: the active columns (those some joint reads), in column order
  int n_act = 0;
  uint32_t* ik_act_rng = nullptr;  // (n_act): the entries of active column i in jac_ents, first | end << 8
  int32_t* ik_col_act = nullptr;   // (n_in): active index of column c, -1: no joint reads it
  int32_t* ik_act_col = nullptr;   // (n_act): the column of active index i (the solve kernel's way back)
  uint2* ik_tri = nullptr;         // (n_act (n_act + 1) / 2), packed lower-triangle entry (i, j), i >= j: x = i | j << 6,
                                   // y = the entry ranges of the two columns, first_i | end_i << 8 | first_j << 16 | end_j << 24,
                                   // all 0 where no link is below a joint of each (the entry of H is a structural zero)
};

namespace {

template <typename T>
void build_tables(const dexr_pose_header& h, const std::vector<dexr_pose_joint>& js, const std::vector<dexr_pose_link>& ls,
                  std::vector<JointD<T>>& dj, std::vector<LinkD<T>>& dl) {
  dj.resize(js.size());
  dl.resize(ls.size());
  std::vector<char> seen(DEXR_POSE_MAXIN, 0);
  for (size_t k = 0; k < js.size(); ++k) {
    const dexr_pose_joint& j = js[k];
    JointD<T>& d = dj[k];
    memset(&d, 0, sizeof(d));
    d.type = j.type;
    d.src_kind = j.src_kind;
    d.src_col = j.src_col;
    d.restore = j.restore;
    d.save = j.save;
    d.link_begin = j.link_begin;
    d.link_end = j.link_end;
    d.sub_link_end = j.sub_link_end;
    if (j.src_kind == DEXR_POSE_SRC_X) {
      d.first_of_col = seen[j.src_col] ? 0 : 1;
      seen[j.src_col] = 1;
    }
    d.mult = (T)j.mult;
    d.off = (T)j.off;
    const double* a = j.axis;
    const double K[9] = {0, -a[2], a[1], a[2], 0, -a[0], -a[1], a[0], 0};
    double K2[9], Rx[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        Rx[3 * r + c] = j.X[4 * r + c];
        K2[3 * r + c] = K[3 * r] * K[c] + K[3 * r + 1] * K[3 + c] + K[3 * r + 2] * K[6 + c];
      }
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) {
        d.A[3 * r + c] = (T)Rx[3 * r + c];
        d.Bm[3 * r + c] = (T)(Rx[3 * r] * K[c] + Rx[3 * r + 1] * K[3 + c] + Rx[3 * r + 2] * K[6 + c]);
        d.C[3 * r + c] = (T)(Rx[3 * r] * K2[c] + Rx[3 * r + 1] * K2[3 + c] + Rx[3 * r + 2] * K2[6 + c]);
      }
      d.p[r] = (T)j.X[4 * r + 3];
      d.xa[r] = (T)(Rx[3 * r] * a[0] + Rx[3 * r + 1] * a[1] + Rx[3 * r + 2] * a[2]);
    }
  }
  for (size_t l = 0; l < ls.size(); ++l) {
    dl[l].parent = ls[l].parent;
    dl[l].out = ls[l].out;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) dl[l].R[3 * r + c] = (T)ls[l].X[4 * r + c];
      dl[l].p[r] = (T)ls[l].X[4 * r + 3];
    }
  }
  (void)h;
}

template <typename T>
hipError_t upload(const std::vector<JointD<T>>& dj, const std::vector<LinkD<T>>& dl, DevTables<T>& out) {
  // (one record more than needed: an empty joint list still gets a valid pointer)
  hipError_t e = hipMalloc((void**)&out.joints, (dj.size() + 1) * sizeof(JointD<T>));
  if (e != hipSuccess) return e;
  e = hipMalloc((void**)&out.links, (dl.size() + 1) * sizeof(LinkD<T>));
  if (e != hipSuccess) return e;
  if (!dj.empty()) {
    e = hipMemcpy(out.joints, dj.data(), dj.size() * sizeof(JointD<T>), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
  }
  return hipMemcpy(out.links, dl.data(), dl.size() * sizeof(LinkD<T>), hipMemcpyHostToDevice);
}

template <typename T>
const DevTables<T>& tables_of(const dexr_pose_model* m);
template <>
const DevTables<float>& tables_of<float>(const dexr_pose_model* m) { return m->f32; }
template <>
const DevTables<double>& tables_of<double>(const dexr_pose_model* m) { return m->f64; }

template <typename T>
PoseArgs<T> args_of(const dexr_pose_model* m, int64_t B) {
  PoseArgs<T> P;
  P.n_joint = m->h.n_joint;
  P.n_link = m->h.n_link;
  P.n_base = m->n_base;
  P.n_in = m->h.n_in;
  P.n_fixed = m->h.n_fixed;
  P.n_slot = m->h.n_slot;
  P.unused_lo = m->unused[0];
  P.unused_hi = m->unused[1];
  P.unused_2 = m->unused[2];
  P.unused_3 = m->unused[3];
  P.B = B;
  return P;
}

// lanes per block: 64, fewer only where the per-lane LDS rows of a block would not fit 64 KB (float64 VJP of a 64-link table)
int block_lanes(size_t per_lane) {
  int nl = POSE_BLOCK;
  while (nl > 8 && per_lane * nl > 64 * 1024) nl /= 2;
  return nl;
}

int check_call(const dexr_pose_model* m, int64_t B, const void* x, const void* fixed) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null pose model");
  if (B < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative batch size");
  if (B == 0) return 1;
  if (!x && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "x is NULL");
  if (!fixed && m->h.n_fixed > 0) return dexr_set_error(DEXR_ERR_INVALID, "the table reads %d fixed columns: fixed must not be NULL", m->h.n_fixed);
  return 0;
}

template <typename T>
int launch_forward(const dexr_pose_model* m, int64_t B, const T* x, const T* fixed, T* pos, T* rot, hipStream_t st) {
  const size_t per_lane = (size_t)m->h.n_slot * 12 * sizeof(T);
  const int nl = block_lanes(per_lane);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  hipLaunchKernelGGL(pose_forward_kernel<T>, dim3((unsigned)blocks), dim3(nl), per_lane * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), x, fixed, pos, rot);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "link pose kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

template <typename T>
int launch_vjp(const dexr_pose_model* m, int64_t B, const T* x, const T* fixed, const T* gpos, const T* grot, T* gx, hipStream_t st) {
  const size_t per_lane = ((size_t)m->h.n_slot * 12 + (size_t)m->h.n_link * 6) * sizeof(T);
  const int nl = block_lanes(per_lane);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  hipLaunchKernelGGL(pose_vjp_kernel<T>, dim3((unsigned)blocks), dim3(nl), per_lane * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), x, fixed, gpos, grot, gx);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "link pose VJP kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// the Jacobian kernel's index data: the joints feeding each column of x (CSR, joints in walk order) and, per element of a
// frame's (n_link, 3, n_in) output block, its sorted link, row and column
hipError_t upload_jacobian_index(const dexr_pose_header& h, const std::vector<dexr_pose_joint>& js, const std::vector<dexr_pose_link>& ls,
                                 dexr_pose_model* m) {
  std::vector<int32_t> xi(js.size(), -1), colptr((size_t)h.n_in + 1, 0), sorted_of(ls.size(), 0);
  int n_jx = 0;
  for (size_t k = 0; k < js.size(); ++k)
    if (js[k].src_kind == DEXR_POSE_SRC_X) xi[k] = n_jx++;
  std::vector<JacEnt> ents;
  for (int c = 0; c < h.n_in; ++c) {
    for (size_t k = 0; k < js.size(); ++k) {
      if (js[k].src_kind != DEXR_POSE_SRC_X || js[k].src_col != c) continue;
      JacEnt e = {xi[k], js[k].link_begin, js[k].sub_link_end, js[k].type, js[k].mult, (float)js[k].mult, 0};
      ents.push_back(e);
    }
    colptr[c + 1] = (int32_t)ents.size();
  }
  for (size_t l = 0; l < ls.size(); ++l) sorted_of[ls[l].out] = (int32_t)l;
  std::vector<uint32_t> emap((size_t)h.n_link * 3 * h.n_in);
  for (int lo = 0; lo < h.n_link; ++lo)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < h.n_in; ++c)
        emap[((size_t)lo * 3 + r) * h.n_in + c] = (uint32_t)sorted_of[lo] | ((uint32_t)r << 6) | ((uint32_t)c << 8);
  m->n_jx = n_jx;
  hipError_t e = hipMalloc((void**)&m->jac_colptr, colptr.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m->jac_ents, (ents.size() + 1) * sizeof(JacEnt));
  if (e == hipSuccess) e = hipMalloc((void**)&m->jac_emap, (emap.size() + 1) * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(m->jac_colptr, colptr.data(), colptr.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess && !ents.empty()) e = hipMemcpy(m->jac_ents, ents.data(), ents.size() * sizeof(JacEnt), hipMemcpyHostToDevice);
  if (e == hipSuccess && !emap.empty()) e = hipMemcpy(m->jac_emap, emap.data(), emap.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) return e;
  // the IK kernel's: active columns (n_act <= n_jx <= DEXR_POSE_MAXJ) and the (row, column) of each packed triangle entry
  // (at most DEXR_POSE_MAXJ entries in all, so an index and an end fit eight bits)
  std::vector<int32_t> act_col, col_act((size_t)h.n_in + 1, -1);
  std::vector<uint32_t> act_rng;
  for (int c = 0; c < h.n_in; ++c)
    if (colptr[c + 1] > colptr[c]) {
      col_act[c] = (int32_t)act_col.size();
      act_col.push_back(c);
      act_rng.push_back((uint32_t)colptr[c] | ((uint32_t)colptr[c + 1] << 8));
    }
  std::vector<uint2> tri;
  for (size_t i = 0; i < act_col.size(); ++i)
    for (size_t j = 0; j <= i; ++j) {
      bool shared = false;  // is some link below a joint of column i and a joint of column j?
      for (int a = colptr[act_col[i]]; a < colptr[act_col[i] + 1]; ++a)
        for (int b = colptr[act_col[j]]; b < colptr[act_col[j] + 1]; ++b)
          if (std::max(ents[a].link_begin, ents[b].link_begin) < std::min(ents[a].sub_end, ents[b].sub_end)) shared = true;
      uint2 d;
      d.x = (uint32_t)(i | (j << 6));
      d.y = shared ? (act_rng[i] | (act_rng[j] << 16)) : 0u;
      tri.push_back(d);
    }
  m->n_act = (int)act_col.size();
  e = hipMalloc((void**)&m->ik_act_rng, (act_rng.size() + 1) * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m->ik_col_act, col_act.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m->ik_tri, (tri.size() + 1) * sizeof(uint2));
  if (e == hipSuccess) e = hipMalloc((void**)&m->ik_act_col, (act_col.size() + 1) * sizeof(int32_t));
  if (e == hipSuccess && !act_rng.empty()) e = hipMemcpy(m->ik_act_rng, act_rng.data(), act_rng.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->ik_col_act, col_act.data(), col_act.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess && !tri.empty()) e = hipMemcpy(m->ik_tri, tri.data(), tri.size() * sizeof(uint2), hipMemcpyHostToDevice);
  if (e == hipSuccess && !act_col.empty()) e = hipMemcpy(m->ik_act_col, act_col.data(), act_col.size() * sizeof(int32_t), hipMemcpyHostToDevice);
  return e;
}

// checks shared by the four entry points of dexr_jacobian.h: < 0 error, 1 nothing to do, 0 go on
int check_jacobian_call(const dexr_pose_model* m, int64_t B, const void* x, const void* fixed, int32_t frame, const void* out_a,
                        const void* out_b) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null pose model");
  if (B < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative batch size");
  if (frame != DEXR_JAC_WORLD_ALIGNED && frame != DEXR_JAC_LOCAL) return dexr_set_error(DEXR_ERR_INVALID, "unknown frame %d (0: world aligned, 1: local)", frame);
  if (B == 0) return 1;
  if (!out_a && !out_b) return dexr_set_error(DEXR_ERR_INVALID, "the linear and the angular output are both NULL");
  return check_call(m, B, x, fixed);
}

template <typename T>
int launch_velocities(const dexr_pose_model* m, int64_t B, const T* x, const T* fixed, const T* xdot, int frame, T* lin, T* ang,
                      hipStream_t st) {
  const size_t per_lane = (size_t)m->h.n_slot * 18 * sizeof(T);  // a fork keeps its twist beside its transform
  const int nl = block_lanes(per_lane);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  hipLaunchKernelGGL(pose_velocity_kernel<T>, dim3((unsigned)blocks), dim3(nl), per_lane * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), x, fixed, xdot, frame, lin, ang);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "link velocity kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

template <typename T>
int launch_jacobians(const dexr_pose_model* m, int64_t B, const T* x, const T* fixed, int frame, T* jlin, T* jang, hipStream_t st) {
  // values a lane parks for phase B: a, o per joint driven by x, p (local frame: and R) per link; odd, so that neither phase
  // meets a bank twice
  const int stride = (6 * m->n_jx + (frame == DEXR_JAC_LOCAL ? 12 : 3) * m->h.n_link) | 1;
  const size_t per_lane = ((size_t)m->h.n_slot * 12 + (size_t)stride) * sizeof(T);
  int nl = block_lanes(per_lane);
  while (nl > 1 && per_lane * nl > 64 * 1024) nl /= 2;  // (float64, local frame, 64 joints and 64 links: 4 lanes)
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  hipLaunchKernelGGL(pose_jacobian_kernel<T>, dim3((unsigned)blocks), dim3(nl * JAC_FANOUT), per_lane * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), (const int32_t*)m->jac_colptr, (const JacEnt*)m->jac_ents,
                     (const uint32_t*)m->jac_emap, m->n_jx, stride, frame, x, fixed, jlin, jang);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "link Jacobian kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// checks shared by the four entry points of dexr_wrench.h: < 0 error, 1 nothing to do, 0 go on
int check_wrench_call(const dexr_pose_model* m, int64_t B, const void* x, const void* fixed, int32_t frame, const void* in_a,
                      const void* in_b, const void* out_a, const void* out_b) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null pose model");
  if (B < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative batch size");
  if (frame != DEXR_JAC_WORLD_ALIGNED && frame != DEXR_JAC_LOCAL) return dexr_set_error(DEXR_ERR_INVALID, "unknown frame %d (0: world aligned, 1: local)", frame);
  if (B == 0) return 1;
  if (!in_a && !in_b) return dexr_set_error(DEXR_ERR_INVALID, "the linear and the angular input are both NULL");
  if (!out_a && !out_b) return dexr_set_error(DEXR_ERR_INVALID, "every output is NULL");
  return check_call(m, B, x, fixed);
}

// gx == NULL: the wrench form (xdot is not read); otherwise the VJP form, gxd may be NULL
template <typename T>
int launch_wrench(const dexr_pose_model* m, int64_t B, const T* x, const T* fixed, const T* xdot, int frame, const T* gl, const T* ga,
                  T* gx, T* gxd, hipStream_t st) {
  const bool vel = gx != nullptr;
  const size_t per_link = vel ? (frame == DEXR_JAC_LOCAL ? 9 : 12) : 6;
  const size_t per_lane = ((size_t)m->h.n_slot * (vel ? 18 : 12) + (size_t)m->h.n_link * per_link) * sizeof(T);
  const int nl = block_lanes(per_lane);
  if (per_lane * nl > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the table needs %zu B of LDS per frame: %d frames do not fit one block", per_lane, nl);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  const JointD<T>* js = tables_of<T>(m).joints;
  const LinkD<T>* ls = tables_of<T>(m).links;
  if (vel)
    hipLaunchKernelGGL((pose_wrench_kernel<T, true>), dim3((unsigned)blocks), dim3(nl), per_lane * nl, st, js, ls, args_of<T>(m, B), x, fixed,
                       xdot, frame, gl, ga, gx, gxd);
  else
    hipLaunchKernelGGL((pose_wrench_kernel<T, false>), dim3((unsigned)blocks), dim3(nl), per_lane * nl, st, js, ls, args_of<T>(m, B), x, fixed,
                       xdot, frame, gl, ga, gx, gxd);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "link wrench kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// checks shared by the two entry points of dexr_ik.h: < 0 error, 1 nothing to do, 0 go on
int check_ik_call(const dexr_pose_model* m, int64_t B, const void* x, const void* fixed, int32_t frame, const void* el, const void* ea,
                  const void* wl, const void* wa, double damping, const void* dx) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null pose model");
  if (B < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative batch size");
  if (frame != DEXR_JAC_WORLD_ALIGNED && frame != DEXR_JAC_LOCAL) return dexr_set_error(DEXR_ERR_INVALID, "unknown frame %d (0: world aligned, 1: local)", frame);
  if (!(damping > 0.0) || damping > 1.7976931348623157e308) return dexr_set_error(DEXR_ERR_INVALID, "damping must be finite and > 0, got %g", damping);
  if (B == 0) return 1;
  if (!el && !ea) return dexr_set_error(DEXR_ERR_INVALID, "the linear and the angular error are both NULL");
  if (wl && !el) return dexr_set_error(DEXR_ERR_INVALID, "w_lin given without err_lin");
  if (wa && !ea) return dexr_set_error(DEXR_ERR_INVALID, "w_ang given without err_ang");
  if (!dx && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "dx_out is NULL");
  return check_call(m, B, x, fixed);
}

template <typename T>
int launch_ik(const dexr_pose_model* m, int64_t B, const T* x, const T* fixed, int frame, const T* el, const T* ea, const T* wl, const T* wa,
              T lambda, T* dx, hipStream_t st) {
  // values of a frame's region: a, o per joint driven by x | IK_LINK per link | packed H | g, y, the factor's diagonal; odd, so
  // that the frames of a wave start in different banks
  const int n_act = m->n_act;
  const int stride = (6 * m->n_jx + IK_LINK * m->h.n_link + n_act * (n_act + 1) / 2 + 3 * n_act) | 1;
  const size_t per_frame = ((size_t)m->h.n_slot * 12 + (size_t)stride) * sizeof(T);
  int nl = IK_FRAMES;
  while (nl > 1 && per_frame * nl > 64 * 1024) nl /= 2;  // (float64, 64 active columns and 64 links: 2 frames)
  if (per_frame * nl > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the table needs %zu B of LDS per frame: one frame does not fit a block", per_frame);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  hipLaunchKernelGGL(pose_ik_kernel<T>, dim3((unsigned)blocks), dim3(nl * IK_FANOUT), per_frame * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), (const JacEnt*)m->jac_ents,
                     (const uint32_t*)m->ik_act_rng, (const int32_t*)m->ik_col_act, (const uint2*)m->ik_tri, m->n_jx, n_act, stride, frame, x,
                     fixed, el, ea, wl, wa, lambda, dx);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "link IK step kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// checks shared by the two entry points of dexr_ik_solve.h: < 0 error, 1 nothing to do, 0 go on
int check_ik_solve_call(const dexr_pose_model* m, int64_t B, const void* x0, const void* fixed, const void* tp, const void* tr, const void* wl,
                        const void* wa, const void* lo, const void* hi, double damping, double max_step, double tol, int32_t max_iters,
                        const void* x_out) {
  const double big = 1.7976931348623157e308;
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null pose model");
  if (B < 0) return dexr_set_error(DEXR_ERR_INVALID, "negative batch size");
  if (!(damping > 0.0) || damping > big) return dexr_set_error(DEXR_ERR_INVALID, "damping must be finite and > 0, got %g", damping);
  if (!(max_step >= 0.0) || max_step > big) return dexr_set_error(DEXR_ERR_INVALID, "max_step must be finite and >= 0 (0: no limit), got %g", max_step);
  if (!(tol >= 0.0) || tol > big) return dexr_set_error(DEXR_ERR_INVALID, "tol must be finite and >= 0, got %g", tol);
  if (max_iters < 1 || max_iters > 256) return dexr_set_error(DEXR_ERR_INVALID, "max_iters must be in 1..256, got %d", max_iters);
  if ((lo == nullptr) != (hi == nullptr)) return dexr_set_error(DEXR_ERR_INVALID, "lo and hi must both be given or both be NULL");
  if (B == 0) return 1;
  if (!tp && !tr) return dexr_set_error(DEXR_ERR_INVALID, "tgt_pos and tgt_rot are both NULL");
  if (wl && !tp) return dexr_set_error(DEXR_ERR_INVALID, "w_lin given without tgt_pos");
  if (wa && !tr) return dexr_set_error(DEXR_ERR_INVALID, "w_ang given without tgt_rot");
  if (!x_out) return dexr_set_error(DEXR_ERR_INVALID, "x_out is NULL");
  if (!x0 && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "x0 is NULL");
  return check_call(m, B, x0, fixed);
}

template <typename T>
int launch_ik_solve(const dexr_pose_model* m, int64_t B, const T* x0, const T* fixed, const T* tp, const T* tr, const T* wl, const T* wa,
                    const T* lo, const T* hi, T lambda, T max_step, T tol, int max_iters, T* x_out, int32_t* iters, T* err, hipStream_t st) {
  // the step kernel's region with the frame's x (n_in values) and E behind it; odd.  Per frame in front of it: sixteen 64-bit
  // partial masks, a stop flag and an iteration count
  const int n_act = m->n_act;
  const int stride = (6 * m->n_jx + IK_LINK * m->h.n_link + n_act * (n_act + 1) / 2 + 3 * n_act + m->h.n_in + 1) | 1;
  const size_t per_frame = ((size_t)m->h.n_slot * 12 + (size_t)stride) * sizeof(T) + IK_FANOUT * sizeof(unsigned long long) + 2 * sizeof(int32_t);
  int nl = IK_FRAMES;
  while (nl > 1 && per_frame * nl > 64 * 1024) nl /= 2;  // (float64, 64 active columns and 64 links: 2 frames)
  if (per_frame * nl > 64 * 1024)
    return dexr_set_error(DEXR_ERR_UNSUPPORTED, "the table needs %zu B of LDS per frame: one frame does not fit a block", per_frame);
  const int64_t blocks = (B + nl - 1) / nl;
  if (blocks > 0x7fffffffLL) return dexr_set_error(DEXR_ERR_INVALID, "batch too large for one launch");
  hipLaunchKernelGGL(pose_ik_solve_kernel<T>, dim3((unsigned)blocks), dim3(nl * IK_FANOUT), per_frame * nl, st, (const JointD<T>*)tables_of<T>(m).joints,
                     (const LinkD<T>*)tables_of<T>(m).links, args_of<T>(m, B), (const JacEnt*)m->jac_ents, (const uint32_t*)m->ik_act_rng,
                     (const int32_t*)m->ik_act_col, (const uint2*)m->ik_tri, m->n_jx, n_act, stride, x0, fixed, tp, tr, wl, wa, lo, hi, lambda,
                     max_step, tol * tol, max_iters, x_out, iters, err);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "link IK solve kernel launch failed: %s", hipGetErrorString(e));
  return DEXR_OK;
}

// device staging of the host-pointer entry points
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t put(const void* src, size_t n) {
    hipError_t e = hipMalloc(&p, n ? n : 8);
    if (e == hipSuccess && src && n) e = hipMemcpy(p, src, n, hipMemcpyHostToDevice);
    return e;
  }
};

#define POSE_HIP(expr)                                                                                         \
  do {                                                                                                         \
    hipError_t e_ = (expr);                                                                                    \
    if (e_ != hipSuccess) return dexr_set_error(DEXR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// the float64 host twin of both entry-point pairs of dexr_wrench.h: copy, run, synchronise
int host_wrench(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, const double* xdot, int32_t frame,
                const double* gl, const double* ga, double* gx_out, double* gxd_out) {
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t nv = (size_t)B * m->h.n_link * 3 * sizeof(double);
  DevBuf dx, dfix, dxd, dl, da, dgx, dgxd;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (gx_out) POSE_HIP(dxd.put(xdot, nx));
  if (gl) POSE_HIP(dl.put(gl, nv));
  if (ga) POSE_HIP(da.put(ga, nv));
  if (gx_out) POSE_HIP(dgx.put(nullptr, nx));
  if (gxd_out) POSE_HIP(dgxd.put(nullptr, nx));
  const int rc = launch_wrench<double>(m, B, (const double*)dx.p, (const double*)dfix.p, (const double*)dxd.p, frame, (const double*)dl.p,
                                       (const double*)da.p, (double*)dgx.p, (double*)dgxd.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (gx_out && nx) POSE_HIP(hipMemcpy(gx_out, dgx.p, nx, hipMemcpyDeviceToHost));
  if (gxd_out && nx) POSE_HIP(hipMemcpy(gxd_out, dgxd.p, nx, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

// a pose blob, validated: what dexr_pose_model_create uploads (the sphere model of dexr_spheres.h checks its own arrays between
// the two steps, so that every argument error comes before the first HIP call)
struct PoseParsed {
  dexr_pose_header h;
  std::vector<dexr_pose_joint> js;
  std::vector<dexr_pose_link> ls;
  int n_base = 0;
  uint64_t used[4] = {0, 0, 0, 0};
};

int parse_pose_blob(const void* blob, size_t nbytes, PoseParsed& parsed) {
  if (nbytes < sizeof(dexr_pose_header)) return dexr_set_error(DEXR_ERR_INVALID, "pose blob truncated: shorter than its header");
  dexr_pose_header& h = parsed.h;
  memcpy(&h, blob, sizeof(h));
  if (h.magic != DEXR_POSE_MAGIC) return dexr_set_error(DEXR_ERR_INVALID, "bad magic 0x%08x in pose blob", h.magic);
  if (h.version != DEXR_POSE_VERSION) return dexr_set_error(DEXR_ERR_INVALID, "pose table version %u, library expects %u", h.version, DEXR_POSE_VERSION);
  if (h.n_joint < 0 || h.n_joint > DEXR_POSE_MAXJ) return dexr_set_error(DEXR_ERR_INVALID, "pose table has %d joints (0..%d)", h.n_joint, DEXR_POSE_MAXJ);
  if (h.n_link < 1 || h.n_link > DEXR_POSE_MAXL) return dexr_set_error(DEXR_ERR_INVALID, "pose table has %d links (1..%d)", h.n_link, DEXR_POSE_MAXL);
  if (h.n_in < 0 || h.n_in > DEXR_POSE_MAXIN || h.n_fixed < 0 || h.n_fixed > DEXR_POSE_MAXIN)
    return dexr_set_error(DEXR_ERR_INVALID, "pose table input widths out of range (n_in %d, n_fixed %d)", h.n_in, h.n_fixed);
  if (h.n_slot < 0 || h.n_slot > DEXR_POSE_MAXSLOT) return dexr_set_error(DEXR_ERR_INVALID, "pose table uses %d slots (0..%d)", h.n_slot, DEXR_POSE_MAXSLOT);
  const size_t want = sizeof(h) + (size_t)h.n_joint * sizeof(dexr_pose_joint) + (size_t)h.n_link * sizeof(dexr_pose_link);
  if (nbytes < want) return dexr_set_error(DEXR_ERR_INVALID, "pose blob truncated: %zu B, its header implies %zu B", nbytes, want);
  if (nbytes != want) return dexr_set_error(DEXR_ERR_INVALID, "pose blob size %zu B, its header implies %zu B", nbytes, want);
  std::vector<dexr_pose_joint>& js = parsed.js;
  std::vector<dexr_pose_link>& ls = parsed.ls;
  js.resize(h.n_joint);
  ls.resize(h.n_link);
  const unsigned char* p = static_cast<const unsigned char*>(blob) + sizeof(h);
  if (h.n_joint) memcpy(js.data(), p, (size_t)h.n_joint * sizeof(dexr_pose_joint));
  memcpy(ls.data(), p + (size_t)h.n_joint * sizeof(dexr_pose_joint), (size_t)h.n_link * sizeof(dexr_pose_link));

  // links: sorted by parent joint (base first), `out` a permutation
  uint64_t out_seen = 0;
  int& n_base = parsed.n_base;
  n_base = 0;
  for (int l = 0; l < h.n_link; ++l) {
    const dexr_pose_link& L = ls[l];
    if (L.parent < -1 || L.parent >= h.n_joint) return dexr_set_error(DEXR_ERR_INVALID, "pose link %d: parent joint %d out of range", l, L.parent);
    if (l > 0 && L.parent < ls[l - 1].parent) return dexr_set_error(DEXR_ERR_INVALID, "pose link %d: links are not sorted by parent joint", l);
    if (L.out < 0 || L.out >= h.n_link || ((out_seen >> L.out) & 1ull)) return dexr_set_error(DEXR_ERR_INVALID, "pose link %d: output row %d out of range or repeated", l, L.out);
    out_seen |= 1ull << L.out;
    if (L.parent == -1) ++n_base;
  }
  // joints: parent before child, contiguous subtrees, slot discipline, link ranges that match the link records
  std::vector<int> slot_owner(DEXR_POSE_MAXSLOT, -1), sub_end(h.n_joint, 0);
  uint64_t* used = parsed.used;
  used[0] = used[1] = used[2] = used[3] = 0;
  int next_link = n_base;
  for (int k = 0; k < h.n_joint; ++k) {
    const dexr_pose_joint& J = js[k];
    if (J.parent < -1 || J.parent >= k) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: parent %d does not come before it", k, J.parent);
    if (J.type != DEXR_POSE_REVOLUTE && J.type != DEXR_POSE_PRISMATIC) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: unknown type %d", k, J.type);
    if (J.src_kind < DEXR_POSE_SRC_X || J.src_kind > DEXR_POSE_SRC_CONST) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: unknown source kind %d", k, J.src_kind);
    const int ncol = J.src_kind == DEXR_POSE_SRC_X ? h.n_in : (J.src_kind == DEXR_POSE_SRC_FIXED ? h.n_fixed : 1);
    if (J.src_col < 0 || J.src_col >= ncol) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: source column %d out of range (%d columns)", k, J.src_col, ncol);
    if (J.src_kind == DEXR_POSE_SRC_X) used[J.src_col >> 6] |= 1ull << (J.src_col & 63);
    // where the running transform comes from
    if (J.parent == -1) {
      if (J.restore != DEXR_POSE_ROOT) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: a root joint must restore the identity", k);
    } else if (J.restore == DEXR_POSE_CONTINUE) {
      if (J.parent != k - 1) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: continues joint %d but its parent is %d", k, k - 1, J.parent);
    } else {
      if (J.restore < 0 || J.restore >= h.n_slot || slot_owner[J.restore] != J.parent)
        return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: restore slot %d does not hold the transform of its parent %d", k, J.restore, J.parent);
    }
    if (J.save != -1) {
      if (J.save < 0 || J.save >= h.n_slot) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: save slot %d out of range", k, J.save);
      slot_owner[J.save] = k;
    }
    if (J.link_begin != next_link || J.link_end < J.link_begin || J.link_end > h.n_link)
      return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: link range [%d, %d) malformed", k, J.link_begin, J.link_end);
    for (int l = J.link_begin; l < J.link_end; ++l)
      if (ls[l].parent != k) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: link %d in its range has parent %d", k, l, ls[l].parent);
    next_link = J.link_end;
  }
  if (next_link != h.n_link) return dexr_set_error(DEXR_ERR_INVALID, "pose table: %d links are in no joint's range", h.n_link - next_link);
  // subtree link ranges: joints below k are the run k+1 .. while parent >= k
  for (int k = 0; k < h.n_joint; ++k) {
    int e = k + 1;
    while (e < h.n_joint && js[e].parent >= k) ++e;
    const int want_end = e < h.n_joint ? js[e].link_begin : h.n_link;
    if (js[k].sub_link_end != want_end) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: subtree link range ends at %d, the tree says %d", k, js[k].sub_link_end, want_end);
    for (int c = k + 1; c < e; ++c) {  // every joint of the run must descend from k (depth-first order)
      int a = js[c].parent;
      while (a > k) a = js[a].parent;
      if (a != k) return dexr_set_error(DEXR_ERR_INVALID, "pose joint %d: joints are not in depth-first order", c);
    }
  }
  return DEXR_OK;
}

int upload_pose_model(const PoseParsed& parsed, dexr_pose_model** out) {
  const dexr_pose_header& h = parsed.h;
  const std::vector<dexr_pose_joint>& js = parsed.js;
  const std::vector<dexr_pose_link>& ls = parsed.ls;
  dexr_pose_model* m = new (std::nothrow) dexr_pose_model();
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "out of host memory");
  m->h = h;
  m->n_base = parsed.n_base;
  for (int w = 0; w < 4; ++w) m->unused[w] = ~parsed.used[w];
  std::vector<JointD<float>> jf;
  std::vector<LinkD<float>> lf;
  std::vector<JointD<double>> jd;
  std::vector<LinkD<double>> ld;
  build_tables<float>(h, js, ls, jf, lf);
  build_tables<double>(h, js, ls, jd, ld);
  hipError_t e = upload(jf, lf, m->f32);
  if (e == hipSuccess) e = upload(jd, ld, m->f64);
  if (e == hipSuccess) e = upload_jacobian_index(h, js, ls, m);
  if (e != hipSuccess) {
    dexr_pose_model_destroy(m);
    return dexr_set_error(DEXR_ERR_HIP, "uploading pose tables failed: %s", hipGetErrorString(e));
  }
  *out = m;
  return DEXR_OK;
}

}  // namespace

extern "C" {

int dexr_pose_model_create(const void* blob, size_t nbytes, dexr_pose_model** out) {
  if (!blob || !out) return dexr_set_error(DEXR_ERR_INVALID, "null argument");
  *out = nullptr;
  PoseParsed parsed;
  const int rc = parse_pose_blob(blob, nbytes, parsed);
  if (rc) return rc;
  return upload_pose_model(parsed, out);
}

void dexr_pose_model_destroy(dexr_pose_model* m) {
  if (!m) return;
  if (m->f32.joints) (void)hipFree(m->f32.joints);
  if (m->f32.links) (void)hipFree(m->f32.links);
  if (m->f64.joints) (void)hipFree(m->f64.joints);
  if (m->f64.links) (void)hipFree(m->f64.links);
  if (m->jac_colptr) (void)hipFree(m->jac_colptr);
  if (m->jac_ents) (void)hipFree(m->jac_ents);
  if (m->jac_emap) (void)hipFree(m->jac_emap);
  if (m->ik_act_rng) (void)hipFree(m->ik_act_rng);
  if (m->ik_col_act) (void)hipFree(m->ik_col_act);
  if (m->ik_tri) (void)hipFree(m->ik_tri);
  if (m->ik_act_col) (void)hipFree(m->ik_act_col);
  delete m;
}

int dexr_pose_model_info(const dexr_pose_model* m, int32_t* n_in, int32_t* n_fixed, int32_t* n_link, int32_t* n_joint) {
  if (!m) return dexr_set_error(DEXR_ERR_INVALID, "null pose model");
  if (n_in) *n_in = m->h.n_in;
  if (n_fixed) *n_fixed = m->h.n_fixed;
  if (n_link) *n_link = m->h.n_link;
  if (n_joint) *n_joint = m->h.n_joint;
  return DEXR_OK;
}

int dexr_link_poses_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, float* pos_out, float* rot_out,
                        void* stream) {
  const int c = check_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!pos_out) return dexr_set_error(DEXR_ERR_INVALID, "pos_out is NULL");
  return launch_forward<float>(m, B, x, fixed, pos_out, rot_out, (hipStream_t)stream);
}

int dexr_link_poses_vjp_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, const float* grad_pos,
                            const float* grad_rot, float* grad_x_out, void* stream) {
  if (m && !grad_pos && !grad_rot) return dexr_set_error(DEXR_ERR_INVALID, "grad_pos and grad_rot are both NULL");
  const int c = check_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_x_out && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  return launch_vjp<float>(m, B, x, fixed, grad_pos, grad_rot, grad_x_out, (hipStream_t)stream);
}

int dexr_link_poses(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, double* pos_out, double* rot_out) {
  const int c = check_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!pos_out) return dexr_set_error(DEXR_ERR_INVALID, "pos_out is NULL");
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t np = (size_t)B * m->h.n_link * 3 * sizeof(double);
  DevBuf dx, dfix, dp, dr;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  POSE_HIP(dp.put(nullptr, np));
  if (rot_out) POSE_HIP(dr.put(nullptr, 3 * np));
  const int rc = launch_forward<double>(m, B, (const double*)dx.p, (const double*)dfix.p, (double*)dp.p, (double*)dr.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  POSE_HIP(hipMemcpy(pos_out, dp.p, np, hipMemcpyDeviceToHost));
  if (rot_out) POSE_HIP(hipMemcpy(rot_out, dr.p, 3 * np, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

int dexr_link_poses_vjp(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, const double* grad_pos,
                        const double* grad_rot, double* grad_x_out) {
  if (m && !grad_pos && !grad_rot) return dexr_set_error(DEXR_ERR_INVALID, "grad_pos and grad_rot are both NULL");
  const int c = check_call(m, B, x, fixed);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!grad_x_out && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "grad_x_out is NULL");
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t np = (size_t)B * m->h.n_link * 3 * sizeof(double);
  DevBuf dx, dfix, dgp, dgr, dgx;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (grad_pos) POSE_HIP(dgp.put(grad_pos, np));
  if (grad_rot) POSE_HIP(dgr.put(grad_rot, 3 * np));
  POSE_HIP(dgx.put(nullptr, nx));
  const int rc = launch_vjp<double>(m, B, (const double*)dx.p, (const double*)dfix.p, (const double*)dgp.p, (const double*)dgr.p,
                                    (double*)dgx.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (nx) POSE_HIP(hipMemcpy(grad_x_out, dgx.p, nx, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

// ---- include/dexr_jacobian.h -----------------------------------------------------------------------------------------------
int dexr_link_jacobians_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, int32_t frame, float* jlin_out,
                            float* jang_out, void* stream) {
  const int c = check_jacobian_call(m, B, x, fixed, frame, jlin_out, jang_out);
  if (c) return c < 0 ? c : DEXR_OK;
  return launch_jacobians<float>(m, B, x, fixed, frame, jlin_out, jang_out, (hipStream_t)stream);
}

int dexr_link_velocities_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, const float* xdot,
                             int32_t frame, float* lin_out, float* ang_out, void* stream) {
  const int c = check_jacobian_call(m, B, x, fixed, frame, lin_out, ang_out);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!xdot && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "xdot is NULL");
  return launch_velocities<float>(m, B, x, fixed, xdot, frame, lin_out, ang_out, (hipStream_t)stream);
}

int dexr_link_jacobians(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, int32_t frame, double* jlin_out,
                        double* jang_out) {
  const int c = check_jacobian_call(m, B, x, fixed, frame, jlin_out, jang_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t nj = (size_t)B * m->h.n_link * 3 * m->h.n_in * sizeof(double);
  DevBuf dx, dfix, dl, da;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (jlin_out) POSE_HIP(dl.put(nullptr, nj));
  if (jang_out) POSE_HIP(da.put(nullptr, nj));
  const int rc = launch_jacobians<double>(m, B, (const double*)dx.p, (const double*)dfix.p, frame, (double*)dl.p, (double*)da.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (jlin_out && nj) POSE_HIP(hipMemcpy(jlin_out, dl.p, nj, hipMemcpyDeviceToHost));
  if (jang_out && nj) POSE_HIP(hipMemcpy(jang_out, da.p, nj, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

int dexr_link_velocities(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, const double* xdot, int32_t frame,
                         double* lin_out, double* ang_out) {
  const int c = check_jacobian_call(m, B, x, fixed, frame, lin_out, ang_out);
  if (c) return c < 0 ? c : DEXR_OK;
  if (!xdot && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "xdot is NULL");
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t nv = (size_t)B * m->h.n_link * 3 * sizeof(double);
  DevBuf dx, dfix, dxd, dl, da;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  POSE_HIP(dxd.put(xdot, nx));
  if (lin_out) POSE_HIP(dl.put(nullptr, nv));
  if (ang_out) POSE_HIP(da.put(nullptr, nv));
  const int rc = launch_velocities<double>(m, B, (const double*)dx.p, (const double*)dfix.p, (const double*)dxd.p, frame, (double*)dl.p,
                                           (double*)da.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (lin_out) POSE_HIP(hipMemcpy(lin_out, dl.p, nv, hipMemcpyDeviceToHost));
  if (ang_out) POSE_HIP(hipMemcpy(ang_out, da.p, nv, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

// ---- include/dexr_wrench.h -------------------------------------------------------------------------------------------------
int dexr_link_wrenches_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, int32_t frame, const float* force,
                           const float* torque, float* tau_out, void* stream) {
  const int c = check_wrench_call(m, B, x, fixed, frame, force, torque, tau_out, nullptr);
  if (c) return c < 0 ? c : DEXR_OK;
  return launch_wrench<float>(m, B, x, fixed, nullptr, frame, force, torque, nullptr, tau_out, (hipStream_t)stream);
}

int dexr_link_velocities_vjp_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, const float* xdot,
                                 int32_t frame, const float* grad_lin, const float* grad_ang, float* grad_x_out, float* grad_xdot_out,
                                 void* stream) {
  const int c = check_wrench_call(m, B, x, fixed, frame, grad_lin, grad_ang, grad_x_out, grad_xdot_out);
  if (c) return c < 0 ? c : DEXR_OK;
  if (grad_x_out && !xdot && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "xdot is NULL");
  return launch_wrench<float>(m, B, x, fixed, xdot, frame, grad_lin, grad_ang, grad_x_out, grad_xdot_out, (hipStream_t)stream);
}

int dexr_link_wrenches(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, int32_t frame, const double* force,
                       const double* torque, double* tau_out) {
  const int c = check_wrench_call(m, B, x, fixed, frame, force, torque, tau_out, nullptr);
  if (c) return c < 0 ? c : DEXR_OK;
  return host_wrench(m, B, x, fixed, nullptr, frame, force, torque, nullptr, tau_out);
}

int dexr_link_velocities_vjp(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, const double* xdot, int32_t frame,
                             const double* grad_lin, const double* grad_ang, double* grad_x_out, double* grad_xdot_out) {
  const int c = check_wrench_call(m, B, x, fixed, frame, grad_lin, grad_ang, grad_x_out, grad_xdot_out);
  if (c) return c < 0 ? c : DEXR_OK;
  if (grad_x_out && !xdot && m->h.n_in > 0) return dexr_set_error(DEXR_ERR_INVALID, "xdot is NULL");
  return host_wrench(m, B, x, fixed, xdot, frame, grad_lin, grad_ang, grad_x_out, grad_xdot_out);
}

// ---- include/dexr_ik.h -------------------------------------------------------------------------------------------------------
int dexr_link_ik_step_dev(const dexr_pose_model* m, int64_t B, const float* x, const float* fixed, int32_t frame, const float* err_lin,
                          const float* err_ang, const float* w_lin, const float* w_ang, float damping, float* dx_out, void* stream) {
  const int c = check_ik_call(m, B, x, fixed, frame, err_lin, err_ang, w_lin, w_ang, (double)damping, dx_out);
  if (c) return c < 0 ? c : DEXR_OK;
  return launch_ik<float>(m, B, x, fixed, frame, err_lin, err_ang, w_lin, w_ang, damping, dx_out, (hipStream_t)stream);
}

int dexr_link_ik_step(const dexr_pose_model* m, int64_t B, const double* x, const double* fixed, int32_t frame, const double* err_lin,
                      const double* err_ang, const double* w_lin, const double* w_ang, double damping, double* dx_out) {
  const int c = check_ik_call(m, B, x, fixed, frame, err_lin, err_ang, w_lin, w_ang, damping, dx_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t nw = (size_t)B * m->h.n_link * sizeof(double);
  DevBuf dx, dfix, dl, da, dwl, dwa, dout;
  POSE_HIP(dx.put(x, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (err_lin) POSE_HIP(dl.put(err_lin, 3 * nw));
  if (err_ang) POSE_HIP(da.put(err_ang, 3 * nw));
  if (w_lin) POSE_HIP(dwl.put(w_lin, nw));
  if (w_ang) POSE_HIP(dwa.put(w_ang, nw));
  POSE_HIP(dout.put(nullptr, nx));
  const int rc = launch_ik<double>(m, B, (const double*)dx.p, (const double*)dfix.p, frame, (const double*)dl.p, (const double*)da.p,
                                   (const double*)dwl.p, (const double*)dwa.p, damping, (double*)dout.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (nx) POSE_HIP(hipMemcpy(dx_out, dout.p, nx, hipMemcpyDeviceToHost));
  return DEXR_OK;
}

// ---- include/dexr_ik_solve.h -----------------------------------------------------------------------------------------------
int dexr_link_ik_solve_dev(const dexr_pose_model* m, int64_t B, const float* x0, const float* fixed, const float* tgt_pos,
                           const float* tgt_rot, const float* w_lin, const float* w_ang, const float* lo, const float* hi, float damping,
                           float max_step, float tol, int32_t max_iters, float* x_out, int32_t* iters_out, float* err_out, void* stream) {
  const int c = check_ik_solve_call(m, B, x0, fixed, tgt_pos, tgt_rot, w_lin, w_ang, lo, hi, (double)damping, (double)max_step, (double)tol,
                                    max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  return launch_ik_solve<float>(m, B, x0, fixed, tgt_pos, tgt_rot, w_lin, w_ang, lo, hi, damping, max_step, tol, max_iters, x_out, iters_out,
                                err_out, (hipStream_t)stream);
}

int dexr_link_ik_solve(const dexr_pose_model* m, int64_t B, const double* x0, const double* fixed, const double* tgt_pos,
                       const double* tgt_rot, const double* w_lin, const double* w_ang, const double* lo, const double* hi, double damping,
                       double max_step, double tol, int32_t max_iters, double* x_out, int32_t* iters_out, double* err_out) {
  const int c = check_ik_solve_call(m, B, x0, fixed, tgt_pos, tgt_rot, w_lin, w_ang, lo, hi, damping, max_step, tol, max_iters, x_out);
  if (c) return c < 0 ? c : DEXR_OK;
  const size_t nx = (size_t)B * m->h.n_in * sizeof(double), nf = (size_t)B * m->h.n_fixed * sizeof(double);
  const size_t nw = (size_t)B * m->h.n_link * sizeof(double), nb = (size_t)m->h.n_in * sizeof(double);
  DevBuf dx, dfix, dp, dr, dwl, dwa, dlo, dhi, dout, dit, derr;
  POSE_HIP(dx.put(x0, nx));
  POSE_HIP(dfix.put(fixed, nf));
  if (tgt_pos) POSE_HIP(dp.put(tgt_pos, 3 * nw));
  if (tgt_rot) POSE_HIP(dr.put(tgt_rot, 9 * nw));
  if (w_lin) POSE_HIP(dwl.put(w_lin, nw));
  if (w_ang) POSE_HIP(dwa.put(w_ang, nw));
  if (lo) POSE_HIP(dlo.put(lo, nb));
  if (hi) POSE_HIP(dhi.put(hi, nb));
  POSE_HIP(dout.put(nullptr, nx));
  POSE_HIP(dit.put(nullptr, (size_t)B * sizeof(int32_t)));
  POSE_HIP(derr.put(nullptr, (size_t)B * sizeof(double)));
  const int rc = launch_ik_solve<double>(m, B, (const double*)dx.p, (const double*)dfix.p, (const double*)dp.p, (const double*)dr.p,
                                         (const double*)dwl.p, (const double*)dwa.p, (const double*)dlo.p, (const double*)dhi.p, damping,
                                         max_step, tol, max_iters, (double*)dout.p, (int32_t*)dit.p, (double*)derr.p, nullptr);
  if (rc) return rc;
  POSE_HIP(hipDeviceSynchronize());
  if (nx) POSE_HIP(hipMemcpy(x_out, dout.p, nx, hipMemcpyDeviceToHost));
  if (iters_out) POSE_HIP(hipMemcpy(iters_out, dit.p, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (err_out) POSE_HIP(hipMemcpy(err_out, derr.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost));
  return DEXR_OK;
}

}  // extern "C"

// ---- include/dexr_spheres.h: sphere-pair self-collision, a fragment of this unit -----------------------------------------------
#include "dexr_spheres.hpp"

// ---- include/dexr_resolve.h: the collision-aware posture solve, the IK solve's resident loop with the sphere phases inside -----
#include "dexr_resolve.hpp"

// ---- include/dexr_obstacles.h: the robot's spheres against posed primitives, the sphere kernel with another phase B ------------
#include "dexr_obstacles.hpp"

// ---- include/dexr_resolve_obstacles.h: the posture solve with the obstacle term, both kernels' phases in one resident loop -----
#include "dexr_resolve_obstacles.hpp"

// ---- include/dexr_sdf_grid.h: the robot's spheres against a sampled signed-distance field, the obstacle kernel with another phase B
#include "dexr_sdf_grid.hpp"

// ---- include/dexr_resolve_grid.h: the posture solve against a signed-distance field, the cell lookup inside the resident loop --
#include "dexr_resolve_grid.hpp"

// ---- include/dexr_resolve_scene.h: the posture solve against several posed bodies at once, sets and grids in one resident loop --
#include "dexr_resolve_scene.hpp"

// ---- include/dexr_cross.h: the spheres of one posed robot against another's, both walks and every pair from both ends in one block --
#include "dexr_cross.hpp"

// ---- include/dexr_resolve_cross.h: the posture solve against a second posed robot, the two-robot term inside the resident loop ------
#include "dexr_resolve_cross.hpp"

// ---- include/dexr_sphere_fit.h: a few inscribed spheres per body from its sampled signed-distance field, a greedy cover in bit masks --
#include "dexr_sphere_fit.hpp"

// ---- include/dexr_distance_transform.h, include/dexr_sdf_grid_dev.h: distance grids from clouds and occupancy, grids that live on the device
#include "dexr_distance_transform.hpp"

// ---- include/dexr_mesh_sdf.h: signed distances of points and grid samples to a triangle mesh, the sampler in front of the grids ----
#include "dexr_mesh_sdf.hpp"

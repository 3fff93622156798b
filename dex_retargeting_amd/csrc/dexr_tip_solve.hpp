// dexr_tip_solve.hpp -- dexr_tip32_kernel: the float32 solve of tip models (dexr_tip.hpp) as a kernel of its own.
//
// dexr_kernel<4, float, MODE_SOLVE, CHAIN, EXT, TIP> runs the tip pass inside the generic persistent-lane loop of the small
// components: every pass of every wave goes through the hand-out of frames to idle lanes, the `fresh` start-point case, the
// free-variable masks of models with fixed / mimic joints, and carries the queue, sequence mode, the float64 hooks and the
// objective-value output as live branches and live scalar registers.  A plain tile launch of a tip model -- the headline: every
// lane gets its one frame before the first pass and never another -- needs none of it.  This kernel is that launch written
// straight:
//   prologue  table pin, the lane's frame (same values, same LDS layout as dexr_kernel -- but the lane's target stays in three
//             registers, its LDS column is not used), clamp to the box, evaluation of the start point (dexr_kernel's pass 0),
//             whose model is adopted.  Its loads go out in batches, one wait per level
//             of their dependency chain, and the frame's own loads are in flight while the constants are pinned -- at every
//             launch size, each issued once (they replace the early touch of the frame's lines that small launches had);
//   loop      the placements of joints 1..3 from LDS into registers, one batch whose latency (a) covers (TipTabRegs),
//             (a) damped 4 x 4 step from the kept model, (b) tip_eval at the trial point unless every live lane takes its
//             blind last step, (c) accept / reject / damping / termination, (d) finished lanes store and drop out;
//             the wave leaves when no lane holds a frame.
//   priority  in launches that fill the chip four waves per SIMD a wave's issue priority falls with the passes it has done and
//             ends higher in the late-placed half of the grid (DEXR_TIP_PRIO below): scheduling only.
// Every floating-point operation the answer depends on is the one dexr_kernel does, on the same operands in the same order
// (steps (2)-(5) of its loop with optmask = all four joints, has && !fresh = has); qpos, status and iters are bitwise
// those of dexr_kernel (tests/test_gpu_tip32_kernel.py).  Calls that need anything else -- queue mode, sequences, fleet
// addressing, fval, float64 -- keep dexr_kernel (dexr_api.hip launch()).
#pragma once
#include "dexr_kernel.hpp"

namespace dexr {

// In-place Cholesky of the damped 4 x 4 model (lower triangle, hidx order) + solve H d = -g: LaneSolver::chol_solve<true>
// (modified Cholesky: a pivot that is not positive is reflected, max(|pivot|, pivot_floor)), operation for operation.
// Returns false where a pivot had to be modified.
static __device__ __forceinline__ bool tip32_chol(float (&H)[10], const float (&g)[4], float (&d)[4], float pivot_floor) {
  using RT = RealTraits<float, true>;
  constexpr auto hidx = [](int r, int c) constexpr { return r * (r + 1) / 2 + c; };
  bool ok = true;
  float inv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float dj = H[hidx(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= H[hidx(j, k)] * H[hidx(j, k)];
    if (!(dj > 1e-6f * pivot_floor)) {
      ok = false;
      dj = fmax(fabs(dj), pivot_floor);
    }
    const float iv = RT::rsqrt(dj);
    inv[j] = iv;
    H[hidx(j, j)] = dj * iv;
#pragma unroll
    for (int i = j + 1; i < 4; ++i) {
      float s = H[hidx(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= H[hidx(i, k)] * H[hidx(j, k)];
      H[hidx(i, j)] = s * iv;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // forward: L y = -g
    float s = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= H[hidx(i, k)] * d[k];
    d[i] = s * inv[i];
  }
#pragma unroll
  for (int i = 3; i >= 0; --i) {  // backward: L^T d = y
    float s = d[i];
#pragma unroll
    for (int k = i + 1; k < 4; ++k) s -= H[hidx(k, i)] * d[k];
    d[i] = s * inv[i];
  }
  return ok;
}

// Issue priority of a wave among the (up to four) waves of its SIMD.  A SIMD issues by priority, then by age, and the workgroup
// dispatcher places a full chip's third and fourth wave per SIMD microseconds after the first two: at equal priority the young
// waves run after the old ones rather than beside them, and a slow frame in a young wave starts its passes late.  The policy is a
// handful of s_setprio behind wave-uniform scalar conditions; no floating-point operation or operand depends on any of it.
// DEXR_TIP_PRIO is a sum of the bits below (-DDEXR_TIP_PRIO=... through DEXR_EXTRA_FLAGS, tools/build_variant.sh);
// -DDEXR_TIP_PRIO=0 is the kernel without any of it, the A/B partner.  What each variant measured: DESIGN.md 4.1,
// profiles/r18_tip32_priority_ab.txt.
//   LADDER    priority 3 from entry through the adopted start-point model and the first pass of the loop, 2 in the second
//             pass, 1 in the third, 0 from the fourth on: it falls with the passes a wave has done.  One counter in a scalar
//             register, one scalar compare per pass once the ladder is through
//   LATE      waves of blocks in the second half of the grid take priority 1 on entry and keep it (leans on dispatch following
//             the block index, which HIP does not promise: where it does not, this costs speed and nothing else)
//   PROLOGUE  priority 3 until the frame has arrived and the start point is evaluated, then 0
//   TAIL      (with LADDER) priority 3 again DEXR_TIP_PRIO_TAIL_AFTER passes after the ladder's end, i.e. from the seventh pass
//             on (the late half: the eighth): the few waves still running then hold the launch's slowest frames.  Alone on the
//             chip they gain nothing; when the next launch of another stream arrives beside them at priority 3, equal priority
//             lets their age win instead of starving them
// LADDER + LATE + TAIL is the default: the ladder, which ends on 1 instead of 0 in the late half, and the tail rung.
// The policy applies to launches of DEXR_TIP_PRIO_MIN_WAVES waves or more -- the launches that fill the chip four waves per
// SIMD, the condition launch() (dexr_api.hip) chooses blocks of eight waves by -- and fewer than DEXR_TIP_PRIO_MAX_WAVES: from
// four generations of waves on, waves replace one another all through the launch, the block index no longer says which waves of
// a SIMD are the late ones, and the policy measured 1-2 us slower (262 144 Allegro frames).  Other launches run at priority 0.
// The upper limit is empirical, from that one shape (four components per frame).  The wave count is that of the grid, blocks x
// waves per block: the launch's waves rounded up to whole blocks, in 32 bits (it wraps only past 2^32 waves, 10^11 frames of a
// four-finger hand, and then costs speed, not answers).
#define DEXR_TIP_PRIO_LADDER 1
#define DEXR_TIP_PRIO_LATE 2
#define DEXR_TIP_PRIO_PROLOGUE 4
#define DEXR_TIP_PRIO_TAIL 8
#ifndef DEXR_TIP_PRIO_TAIL_AFTER
#define DEXR_TIP_PRIO_TAIL_AFTER 3
#endif
#ifndef DEXR_TIP_PRIO
#define DEXR_TIP_PRIO (DEXR_TIP_PRIO_LADDER | DEXR_TIP_PRIO_LATE | DEXR_TIP_PRIO_TAIL)
#endif
#if DEXR_TIP_PRIO & DEXR_TIP_PRIO_TAIL
#define DEXR_TIP_PRIO_DONE (-2 * DEXR_TIP_PRIO_TAIL_AFTER)
#else
#define DEXR_TIP_PRIO_DONE 1
#endif
#ifndef DEXR_TIP_PRIO_MIN_WAVES
#define DEXR_TIP_PRIO_MIN_WAVES 4096
#endif
#ifndef DEXR_TIP_PRIO_MAX_WAVES
#define DEXR_TIP_PRIO_MAX_WAVES 16384
#endif

// -DDEXR_WAVE_TRACE=1 (tools/wave_trace.sh; never in the shipped library): the stamps of dexr_kernel.hpp's WTRACE_*, in the
// same 24 doubles per wave of kp.g64out -- [0] wave start, [1] frame arrived, [2] retired, [3] passes run, [4] HW_ID, [5] XCC_ID,
// [8..23] the end of each of the first 16 passes, 100 MHz wall clock.  Lane 0 stores each stamp when it is taken (the record is
// zeroed before the launch): kept in registers until the wave ends, as dexr_kernel keeps them, they would spill 43 VGPRs of this
// kernel to scratch and the trace would show a different launch.  "Frame arrived" is stamped once the values named there -- the
// last the prologue forms from the frame's loads -- exist, i.e. behind the wait for those loads.
#ifdef DEXR_WAVE_TRACE
#define TIP_WTRACE_PUT(i, v) { if (lane == 0 && wt_o) wt_o[i] = (double)(v); }
#define TIP_WTRACE_START long long wt_t0 = wall_clock64();
#define TIP_WTRACE_DECL double* wt_o = kp.g64out ? kp.g64out + (size_t)wave_global * 24 : nullptr; int wt_n = 0; TIP_WTRACE_PUT(0, wt_t0)
#define TIP_WTRACE_ARRIVED(a, b) { asm volatile("" ::"v"(a), "v"(b)); TIP_WTRACE_PUT(1, wall_clock64()) }
#define TIP_WTRACE_PASS() { if (wt_n < 16) TIP_WTRACE_PUT(8 + wt_n, wall_clock64()) ++wt_n; }
#define TIP_WTRACE_FLUSH() { TIP_WTRACE_PUT(2, wall_clock64()) TIP_WTRACE_PUT(3, wt_n) \
  TIP_WTRACE_PUT(4, __builtin_amdgcn_s_getreg(63492)) TIP_WTRACE_PUT(5, __builtin_amdgcn_s_getreg(63508)) }
#else
#define TIP_WTRACE_START
#define TIP_WTRACE_DECL
#define TIP_WTRACE_ARRIVED(a, b)
#define TIP_WTRACE_PASS()
#define TIP_WTRACE_FLUSH()
#endif

// One wave = 64 frames x one tip component (wave w: component w % n_comp of tile w / n_comp, as dexr_kernel in tile mode).
// blockDim.x = 64 * waves_per_block; dynamic LDS = waves_per_block * 64 * 4 * (3 * lds_frames + 4 * lds_terms + 1) bytes, laid
// out as dexr_kernel's: the lane's target would be at T[(0..2) * 64 + lane] (unused here), the broadcast placements of joints
// 1..3 behind W.
__global__ void __launch_bounds__(DEXR_TIP_BLOCK_MAX, DEXR_CHAIN_MINW) dexr_tip32_kernel(const KernelParams kp, const dexr_comp_table* __restrict__ comps) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  using RT = RealTraits<float, true>;
  constexpr auto hidx = [](int r, int c) constexpr { return r * (r + 1) / 2 + c; };
  TIP_WTRACE_START
#if DEXR_TIP_PRIO
  const unsigned prio_waves = gridDim.x * (blockDim.x >> 6);
  const bool prio_on = prio_waves >= DEXR_TIP_PRIO_MIN_WAVES && prio_waves < DEXR_TIP_PRIO_MAX_WAVES;
  const bool prio_late = (DEXR_TIP_PRIO & DEXR_TIP_PRIO_LATE) && blockIdx.x * 2u >= gridDim.x;
  if (prio_on) {
    if (DEXR_TIP_PRIO & (DEXR_TIP_PRIO_LADDER | DEXR_TIP_PRIO_PROLOGUE)) __builtin_amdgcn_s_setprio(3);
    else if (prio_late) __builtin_amdgcn_s_setprio(1);
  }
#endif
#if DEXR_TIP_PRIO & DEXR_TIP_PRIO_LADDER
  // the ladder's state, stepped down by 2 at the end of each pass until it reaches DEXR_TIP_PRIO_DONE (one scalar compare per pass
  // from then on, and in launches outside the window from the start): 6 -> 4 -> 2 -> 0 sets priority 2, 1, 0 after passes 1, 2, 3;
  // the late half runs 5 -> 3 -> 1, priority 2, 1, and keeps 1; with TAIL the count goes on below zero and sets 3 at DONE
  int prio_c = prio_on ? (prio_late ? 5 : 6) : DEXR_TIP_PRIO_DONE;
#endif
  // The prologue is a few batches of loads, one wait per level of the dependency chain
  //   kernel arguments -> the component's table (+ the lane's LDS constant) -> frame offsets, keypoint indices -> the frame
  // instead of a round trip per value: see TipTabT<float>::fetch / hold (dexr_tip.hpp).
  // Level 0: the options of the solve, all of them kernel arguments, behind one wait -- and with them (as inputs only: the
  // pointers keep what the compiler knows about them) the arguments the index arithmetic and the addresses below need, which
  // would otherwise be fetched one by one where they are first used.
  float a_delta = kp.norm_delta, a_lam0 = kp.lam0, a_tol = kp.tol, a_blind_tol = kp.blind_tol, a_step_cap = kp.step_cap;
  float a_huber = kp.huber_delta, a_inv_norm = kp.inv_norm, a_lam_fastdec = kp.lam_fastdec, a_lam_jump = kp.lam_jump;
  float a_lam_recover = kp.lam_recover, a_stall_ratio = kp.stall_ratio, a_stall_cap = kp.stall_cap;
  float a_scaling = kp.scaling;
  int a_newton = kp.newton, a_stall_from = kp.stall_from, a_max_blind = kp.max_blind, a_max_iter = kp.max_iter;
  asm volatile(""
               : "+s"(a_delta), "+s"(a_lam0), "+s"(a_tol), "+s"(a_blind_tol), "+s"(a_step_cap), "+s"(a_huber), "+s"(a_inv_norm),
                 "+s"(a_lam_fastdec), "+s"(a_lam_jump), "+s"(a_lam_recover), "+s"(a_stall_ratio), "+s"(a_stall_cap), "+s"(a_newton),
                 "+s"(a_stall_from), "+s"(a_max_blind), "+s"(a_max_iter), "+s"(a_scaling)
               : "s"((int)blockDim.x), "s"(kp.last), "s"(kp.kpts), "s"(kp.ref), "s"(kp.B), "s"(kp.n_comp), "s"(kp.n_opt), "s"(kp.n_kp), "s"(kp.n_ref),
                 "s"(kp.lds_frames), "s"(kp.lds_terms));

  const int lane = threadIdx.x & 63;
  const int wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int waves_per_block = blockDim.x >> 6;
  const int64_t wave_global = (int64_t)blockIdx.x * waves_per_block + wave_in_block;
  const int comp = (int)(wave_global % kp.n_comp);
  const int64_t tile = wave_global / kp.n_comp;
  const int64_t nB = kp.B;
  if (tile * 64 >= nB) return;  // (the grid is rounded up to whole blocks)
  TIP_WTRACE_DECL
  const int64_t item = tile * 64 + lane;  // (prologue only: the loop keeps no per-lane address, see retire)
  bool has = item < nB;  // the lane holds a frame that is not finished
  const int ld = kp.n_opt;

  const int per_wave = 64 * (3 * kp.lds_frames + 4 * kp.lds_terms + 1);
  float* P = reinterpret_cast<float*>(lds_raw) + (size_t)wave_in_block * per_wave;
  float* T = P + 64 * 3 * kp.lds_frames;
  float* W = T + 64 * 3 * kp.lds_terms;

  // Level 1: the component's table -- joint 0, the box, the lane's LDS constant, and the four integers the addresses below hang on
  const dexr_comp_table& tb = comps[comp];
  TipTabRegs tt;  // (placements of joints 1..3: prefetched into registers once per pass)
  TipTabT<float>::Stage st;
  int api0 = tb.api[0];  // a tip component's four joints are consecutive columns of last_qpos / qpos_out
  int row = tb.term_ref[0], ft = tb.term_task[0], fo = tb.term_origin[0];
  tt.fetch(tb, lane, st);
  tt.hold(st, api0, row, ft, fo);
  // Level 2: the frame offsets, and which keypoints the term's target is made of
  const int hrow = row < DEXR_MAXT ? row : DEXR_MAXT - 1;  // (keypoint input: row itself; ref_value rows may number more)
  int h_t = kp.h_task[hrow], h_o = kp.h_origin[hrow];
  tt.fetch_off(tb, ft, fo, st);
  tt.hold_off(st, h_t, h_o);

  // Level 3, the lane's frame: start point / regularisation target from last_qpos, the term's target from the keypoints or the
  // ref_value row -- every load issued here, waited for once, behind the pins
  float x[4] = {0.f, 0.f, 0.f, 0.f}, xl[4] = {0.f, 0.f, 0.f, 0.f};
  float fl[4], ra[3], rb[3];  // (set and read by lanes that hold a frame only)
  float tg[3] = {0.f, 0.f, 0.f};  // the lane's target: three registers for the whole solve (T, its LDS column in dexr_kernel, stays unused)
  // the target is keypoint h_t minus keypoint h_o, or keypoint h_t alone, or the ready-made ref_value row: the wave-uniform
  // choice is made on the ADDRESSES (without an origin keypoint rb re-reads ra's line and is not used), so that each load is
  // issued exactly once and no loaded value has to be merged with another or moved between registers before the pins are through
  const bool sub = kp.kpts != nullptr && h_o >= 0;
  if (has) {
    const float* pa = kp.kpts ? kp.kpts + (item * kp.n_kp + h_t) * 3 : kp.ref + (item * kp.n_ref + row) * 3;
    const float* pb = sub ? kp.kpts + (item * kp.n_kp + h_o) * 3 : pa;
#pragma unroll
    for (int k = 0; k < 4; ++k) fl[k] = kp.last[item * ld + api0 + k];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ra[i] = pa[i];
      rb[i] = pb[i];
    }
  }

  // (joint 0, the box and the tip offset stay in the scalar registers hold() / hold_off() returned them in; so does api0)
  tt.place<false>(st, fo, W + 64 * kp.lds_terms, lane);

  // constants of the pass, pinned in SGPRs (the values read by every pass first).  The options are pinned since level 0: the
  // empty asm there made each a scalar register of unknown contents, which the compiler can neither fold back into the
  // kernel-argument load nor load again inside the pass -- a second pin through a VGPR (v_mov, s_nop, v_readfirstlane) adds nothing
  const float k_delta = a_delta, k_lam0 = a_lam0, k_tol = a_tol, k_blind_tol = a_blind_tol;
  const float k_step_cap = a_step_cap;
  const float tip_beta = a_huber, tip_ibeta = tip_pin(1.f / a_huber);
  const float tip_w = a_inv_norm, tip_nw = tip_pin(a_newton != 0 ? 1.f : 0.f);
  const float k_lam_fastdec = a_lam_fastdec, k_lam_jump = a_lam_jump, k_lam_recover = a_lam_recover;
  const float k_stall_ratio = a_stall_ratio;
  const int k_stall_from = a_stall_from, k_max_blind = a_max_blind, k_max_iter = a_max_iter;
  // ... and what the pass derives from them, formed once (the same single multiplications dexr_kernel does) by a vector
  // operation and pinned through tip_pin's readfirstlane (behind a bare "+s" the compiler refuses the copy from the vector
  // register): left to the compiler each becomes a VGPR that is live through the whole loop
  const float k_2delta = tip_pin(2.f * k_delta), k_10tol = tip_pin(10.f * k_tol);
  const float k_stall_max = tip_pin(a_stall_cap * k_tol);
  const float k_lam_ok = tip_pin(fmax(2.f * k_delta, 10.f * k_lam0)), k_lam_ok_half = tip_pin(0.5f * fmax(2.f * k_delta, 10.f * k_lam0));
  // options as thresholds (a comparison with +inf is never true): "lam_fastdec > 0 and rho > 0.9" is rho > k_rho_fast,
  // "lam_recover > 0 and lambda > 10 lam0" is lambda > k_lam_rec_from -- one SGPR each instead of a hoisted lane mask
  const float k_inf = __builtin_inff();
  const float k_rho_fast = tip_pin(a_lam_fastdec > 0 ? 0.9f : k_inf), k_lam_rec_from = tip_pin(a_lam_recover > 0 ? 10.f * a_lam0 : k_inf);

  // ---- the frame has arrived: the term's target into the lane's registers, the start point into the box
  if (has) {
    float rv[3];
    if (sub) {
#pragma unroll
      for (int i = 0; i < 3; ++i) rv[i] = ra[i] - rb[i];
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) rv[i] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) tg[i] = rv[i] * a_scaling;  // f32 multiply: optimizer.py:246
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xl[k] = fl[k];
      x[k] = RT::clamp(fl[k], tt.lo[k], tt.hi[k]);
    }
  }
  TIP_WTRACE_ARRIVED(x[3], tg[2])

  // kept model: data term + regulariser at the accepted point x
  float Hs[10], gs[4], xo[4];
  float F, lam = k_lam0, nu = 2, sprev = 1e30f;
  int my_iters = 0, blind = 0, nrej = 0;

  // value / gradient / Hessian at xe, regulariser included
  auto eval = [&](const float (&xe)[4], float (&g)[4], float (&H)[10]) -> float {
    tt.arrived();
    float Ft = tip_eval<float>(tt, xe, tg[0], tg[1], tg[2], tip_beta, tip_ibeta, tip_w, tip_nw, g, H);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dx = xe[k] - xl[k];
      Ft += k_delta * dx * dx;
      g[k] += k_2delta * dx;
    }
    return Ft;
  };
  // a finished lane hands back its four joints (last_qpos where the solve produced no finite answer) and drops out
  // (the addresses are formed here, from the lane number, behind an opaque copy: hoisted out of the loop they would hold six
  // VGPRs through every pass for three stores per frame)
  auto retire = [&](int status) {
    int l = lane;
    asm volatile("" : "+v"(l));
    const int64_t it = tile * 64 + l;
    bool bad = (status == ST_FALLBACK);
#pragma unroll
    for (int k = 0; k < 4; ++k) bad = bad || !(x[k] == x[k]);
    if (bad) status = ST_FALLBACK;
#pragma unroll
    for (int k = 0; k < 4; ++k) kp.qout[it * ld + api0 + k] = bad ? xl[k] : x[k];
    if (kp.status) atomicMax(&kp.status[it], status);  // (max over the frame's components)
    if (kp.iters) atomicMax(&kp.iters[it], my_iters);
    has = false;
  };

  // ---- start point: adopt its model unconditionally
  tt.prefetch();
  F = eval(x, gs, Hs);
  if (has && !((bool)((int)(F == F) & (int)(fabs(F) < 1e30f)))) retire(ST_FALLBACK);
#if (DEXR_TIP_PRIO & DEXR_TIP_PRIO_PROLOGUE) && !(DEXR_TIP_PRIO & DEXR_TIP_PRIO_LADDER)
  if (prio_on) {
    if (prio_late) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
  }
#endif

  while (__any(has)) {
    // the placements (b) needs, issued here: step (a) uses none of them and covers their way from LDS.  Not gated on (b)'s
    // condition, which (a) produces: a pass that skips (b) -- a wave's last, if any -- has read them for nothing
    tt.prefetch();
    // (a) step from the kept model; joints held at a bound by the gradient sign are taken out of the system
    float g[4], H[10], d[4];
    // (which joints are free: four lane masks as the comparisons deliver them -- the pair conditions are scalar ANDs of them,
    // not bits of an integer in a VGPR that are set and tested again)
    bool fr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gk = gs[k];
      const bool act = (bool)(((int)(x[k] <= tt.lo[k]) & (int)(gk > 0)) | ((int)(x[k] >= tt.hi[k]) & (int)(gk < 0)));
      fr[k] = !act;
      g[k] = !act ? gk : 0.f;
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
      for (int cc = 0; cc < rr; ++cc) H[hidx(rr, cc)] = (fr[rr] && fr[cc]) ? Hs[hidx(rr, cc)] : 0.f;
      H[hidx(rr, rr)] = fr[rr] ? Hs[hidx(rr, rr)] + k_2delta + lam : 1.f;
    }
    float gm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gm[k] = g[k];
    // `ok`: no pivot had to be modified, d is the Newton step of the damped model; a modified step is still tried
    const bool ok = tip32_chol(H, g, d, k_2delta + lam);
    // trust radius: no joint moves more than step_cap; a step from a modified factorisation is stretched (up to 8 x) towards it
    // (sums of two products are written with fmaf: which product a contraction fuses is the compiler's choice per kernel,
    // these are the ones dexr_kernel's code object has -- d.d as d0^2 rounded, then one FMA per further term; pred as the
    // lambda term rounded, then one FMA with g.d)
    float dmax = 0, gd = 0, dd = d[0] * d[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dmax = fmax(dmax, fabs(d[k]));
      gd -= gm[k] * d[k];
      if (k > 0) dd = fmaf(d[k], d[k], dd);
    }
    const bool cut = (bool)((int)(k_step_cap > 0) & ((int)(dmax > k_step_cap) | ((int)!ok & (int)(dmax > 0.f))));
    const float alpha = cut ? fmin(RT::div(k_step_cap, dmax), 8.f) : 1.f;
    // predicted decrease of the damped model along alpha*d:  alpha (1 - alpha/2) (-g.d) + alpha^2/2 lam d.d
    const float pred = fmaf(alpha * (1.f - 0.5f * alpha), gd, 0.5f * alpha * alpha * lam * dd);
    float smax = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xo[k] = x[k];
      const float xt = RT::clamp(x[k] + alpha * d[k], tt.lo[k], tt.hi[k]);
      smax = fmax(smax, fabs(xt - x[k]));
      x[k] = xt;
    }
    // verified, undamped model and a Newton step this short: take it without evaluating the objective there (see dexr_kernel)
    const bool last_step = (bool)((int)has & (int)ok & (int)(smax < k_blind_tol) & (int)(lam <= k_lam0) &
                                  ((int)(smax < k_10tol) | (int)(smax < 0.1f * sprev)));

    // (b) model at the trial point -- unless every lane that still holds a frame retires on the step alone
    float Ft = F;
    if (__any(has && !last_step)) Ft = eval(x, g, H);

    // (c) accept / reject, damping update, termination
    bool accept = false, finished = false;
    int status = ST_MAXITER;
    if (has) {
      const bool finite = (bool)((int)(Ft == Ft) & (int)(smax == smax) & (int)(fabs(Ft) < 1e30f));
      if (last_step && finite) {
        accept = true;
        finished = true;
        status = ST_CONVERGED;
        ++my_iters;
        F = Ft;
      } else {
        // resolution of F in float32 (see dexr_kernel): a predicted decrease below it cannot be verified, only trusted
        const float noise = 16.f * RT::eps() * fmax(fabs(F), 2e-3f);
        const bool below_floor = (bool)((int)ok & (int)finite & (int)(pred <= noise) & (int)(smax < 1e-2f));
        accept = (bool)((int)finite & ((int)(Ft <= F) | (int)below_floor));
        ++my_iters;
        if (accept) {
          const float rho = RT::div(F - Ft, fmax(pred, 1e-30f));
          const float t = 2.f * rho - 1.f;
          float shrink = below_floor ? (float)(1.0 / 3.0) : fmax((float)(1.0 / 3.0), 1.f - t * t * t);
          if (rho > k_rho_fast) shrink = (bool)((int)(nrej <= 2) & (int)(lam > k_lam_rec_from)) ? k_lam_recover : k_lam_fastdec;
          lam = fmax(lam * shrink, 1e-9f);
          nu = 2;
          F = Ft;
          const bool stalled = (bool)((int)below_floor & (int)(blind >= k_stall_from) & (int)(smax > k_stall_ratio * sprev) & (int)(smax < k_stall_max));
          blind = below_floor ? blind + 1 : 0;
          sprev = smax;
          // a step below tol only means convergence when the damping is not what made it small (see dexr_kernel)
          if ((bool)(((int)(smax < k_tol) & (int)(lam <= k_lam_ok)) | (int)stalled | (int)(blind >= k_max_blind))) {
            finished = true;
            status = ST_CONVERGED;
          } else if (smax < k_tol) {
            lam = fmax(0.1f * lam, k_lam_ok_half);
          }
        } else {
          ++nrej;
          lam = fmax(lam, 1e-6f) * nu;
          // go straight to a damping that matters next to the curvature (lam_jump = 0, plain Nielsen: lambda >= 2e-6 here and
          // fmax ignores a NaN, so the fmax with 0 x ds leaves it as it is -- dexr_kernel's `if (lam_jump > 0)` without the branch)
          float ds = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) ds += Hs[hidx(k, k)];
          lam = fmax(lam, k_lam_jump * ds / 4.f);
          nu *= 2;
          if (lam > 1e10f) {  // no descent direction resolvable any more
            finished = true;
            status = finite ? ST_CONVERGED : ST_FALLBACK;
          }
          if ((bool)((int)finite & (int)(smax < k_tol))) {  // rejected step below tol: converged at the rounding floor of F
            finished = true;
            status = ST_CONVERGED;
          }
        }
        finished = (bool)((int)finished | (int)(my_iters >= k_max_iter));  // status stays ST_MAXITER
      }
    }
    // the kept model follows the accepted point; a rejected step goes back to where it started
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = accept ? x[k] : xo[k];
      gs[k] = accept ? g[k] : gs[k];
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) Hs[i] = accept ? H[i] : Hs[i];

    // (d) retire finished frames
    if (finished) retire(status);
    TIP_WTRACE_PASS()
#if DEXR_TIP_PRIO & DEXR_TIP_PRIO_LADDER
    if (prio_c > DEXR_TIP_PRIO_DONE) {
      prio_c -= 2;
      if (prio_c >= 3) __builtin_amdgcn_s_setprio(2);
      else if (prio_c >= 1) __builtin_amdgcn_s_setprio(1);
      else if (prio_c == 0) __builtin_amdgcn_s_setprio(0);
      else if (prio_c <= DEXR_TIP_PRIO_DONE) __builtin_amdgcn_s_setprio(3);  // (TAIL only: without it DONE is the ladder's end)
    }
#endif
  }
  TIP_WTRACE_FLUSH()
}

}  // namespace dexr

#!/usr/bin/env python3
"""GPU box: time of the fused IK solve (dexr_link_ik_solve_dev: the iteration loop inside one kernel) next to the same
iterations driven from torch with the calls the library had before it.  Read-only use of the library.

Workload: Shadow hand vector config, its five tip links, B = 65 536, float32, the optimiser's variables as columns; position and
rotation targets (the poses of q*), both weighted; start q* + U(-0.1, 0.1) clipped to the limits; max_iters = 8, tol = 0.
  (a) one ik_solve_dev call: 8 iterations, bound columns frozen, every iterate on chip
  (b) 8 times from torch: poses_dev (positions and rotations), the position error and the rotation log map in torch,
      ik_step_dev, q = clamp(q + dq) -- no freezing, a plain clamp: what a user of link_ik_step wrote
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so both see the same box;
the MEDIAN over `--rounds` rounds is reported, the rounds beside it.

    python tools/ik_solve_probe.py [--reps 10] [--rounds 7] [--iters 8]
"""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402

REL = "teleop/shadow_hand_right.yml"
TIPS = ["thtip", "fftip", "mftip", "rftip", "lftip"]


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("ik_solve_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    B, L, K = args.batch, len(TIPS), args.iters
    model = opt.pose_model(TIPS)
    n = model.n_in
    assert model.n_fixed == 0
    lim = prob.robot.joint_limits[prob.idx_pin2target].astype(np.float32)
    rng = np.random.default_rng(1)
    q_star = rng.uniform(lim[:, 0], lim[:, 1], (B, n)).astype(np.float32)
    q0 = torch.tensor(np.clip(q_star + rng.uniform(-0.1, 0.1, q_star.shape).astype(np.float32), lim[:, 0], lim[:, 1]), device="cuda")
    q_star = torch.tensor(q_star, device="cuda")
    lo, hi = torch.tensor(lim[:, 0].copy(), device="cuda"), torch.tensor(lim[:, 1].copy(), device="cuda")
    gen = torch.Generator("cuda").manual_seed(2)
    wl = 0.5 + 1.5 * torch.rand((B, L), device="cuda", generator=gen)
    wa = 0.01 * (0.5 + 1.5 * torch.rand((B, L), device="cuda", generator=gen))
    sp = torch.cuda.current_stream().cuda_stream
    tp, tr = torch.empty((B, L, 3), device="cuda"), torch.empty((B, L, 3, 3), device="cuda")
    model.poses_dev(B, q_star.data_ptr(), 0, tp.data_ptr(), tr.data_ptr(), stream=sp)
    # damping: 1e-3 of the largest eigenvalue of J^T W J over the first 1024 frames (the rule of tools/ik_probe.py)
    jlin = torch.empty((1024, L, 3, n), device="cuda")
    jang = torch.empty_like(jlin)
    model.jacobians_dev(1024, q0.data_ptr(), 0, jlin.data_ptr(), jang.data_ptr(), stream=sp)
    H0 = torch.einsum("bl,blri,blrj->bij", wl[:1024], jlin, jlin) + torch.einsum("bl,blri,blrj->bij", wa[:1024], jang, jang)
    lam = float(np.float32(1e-3 * float(torch.linalg.eigvalsh(H0.double().cpu())[:, -1].max())))
    xa, ita, erra = torch.empty((B, n), device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda"), torch.empty((B,), device="cuda")
    p, R, dq = torch.empty_like(tp), torch.empty_like(tr), torch.empty((B, n), device="cuda")
    via = {}

    def errors(q):
        model.poses_dev(B, q.data_ptr(), 0, p.data_ptr(), R.data_ptr(), stream=sp)
        M = tr @ R.transpose(-1, -2)
        v = 0.5 * torch.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1)
        c = 0.5 * (M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2] - 1.0)
        s = v.norm(dim=-1)
        k = torch.where(s > 1e-6, torch.atan2(s, c) / s.clamp_min(1e-30), torch.ones_like(s))
        return (tp - p).contiguous(), (v * k[..., None]).contiguous()

    def a():
        model.ik_solve_dev(B, q0.data_ptr(), 0, tp.data_ptr(), tr.data_ptr(), wl.data_ptr(), wa.data_ptr(), lo.data_ptr(), hi.data_ptr(), lam, K,
                           xa.data_ptr(), ita.data_ptr(), erra.data_ptr(), tol=0.0, max_step=0.0, stream=sp)

    def b():
        q = q0
        for _ in range(K):
            el, ea = errors(q)
            model.ik_step_dev(B, q.data_ptr(), 0, el.data_ptr(), ea.data_ptr(), wl.data_ptr(), wa.data_ptr(), lam, dq.data_ptr(), stream=sp)
            q = torch.maximum(torch.minimum(q + dq, hi), lo)
        via["x"] = q

    KA, KB = f"(a) ik_solve_dev, {K} iterations in one launch", f"(b) {K} x (poses_dev + errors in torch + ik_step_dev + clamp)"
    runs = {KA: a, KB: b}
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, args.reps, args.warmup))
    torch.cuda.synchronize()

    def final_error(q):
        el, ea = errors(q.contiguous())
        return ((wl * (el * el).sum(-1)).sum(-1) + (wa * (ea * ea).sum(-1)).sum(-1)).sqrt()

    ea_, eb_, e0 = final_error(xa), final_error(via["x"]), final_error(q0)
    print(f"# ik_solve_probe: {torch.cuda.get_device_name(0)}, {REL}, links {TIPS}, B = {B}, n_in = {n}, float32, damping {lam:.3e}, "
          f"max_iters = {K}, tol = 0")
    print(f"# HIP events around {args.reps} back-to-back runs after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    print(f"# iterations used by (a): {torch.bincount(ita, minlength=K + 1).tolist()}; max |err_out - recomputed error| = {float((erra - ea_).abs().max()):.3e}")
    print(f"# median error: start {float(e0.median()):.3e}, (a) {float(ea_.median()):.3e}, (b) {float(eb_.median()):.3e}; "
          f"frames where (a) ends lower / (b) ends lower: {int((ea_ < eb_).sum())} / {int((eb_ < ea_).sum())}; max |x of (a) - x of (b)| = "
          f"{float((xa - via['x']).abs().max()):.3e}")
    print(f"{'variant':64s} {'us':>10s}   rounds (us)")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        print(f"{k:64s} {med[k]:10.2f}   {' '.join(f'{v:9.2f}' for v in t[k])}")
    print(f"# (b) / (a) = {med[KB] / med[KA]:.2f}; (a) per iteration = {med[KA] / K:.2f} us")
    if not med[KA] < med[KB]:
        print("# (a) is NOT faster than (b)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""GPU box: time of the link-wrench kernel (dexr_link_wrenches_dev) next to what a user wrote before it, link_jacobians and two
einsums, and of the velocity VJP (dexr_link_velocities_vjp_dev) next to the forward it differentiates.  Read-only use of the
library.

Workload: Shadow hand vector config, its five tip links, B = 65 536, float32, the optimiser's variables as columns.
  (a) one wrenches_dev call, force and torque                         writes 4 B n_in per frame
  (b) jacobians_dev, both blocks, then einsum(jlin, force) + einsum(jang, torque) in torch     writes 4 B 2 L 3 n_in and reads it again
  (c) one velocities_dev call, both outputs (the forward of autograd.link_velocities)
  (d) one velocities_vjp_dev call, both cotangents, grad_x and grad_xdot (its backward)
  (e) one velocities_vjp_dev call, grad_xdot alone (served by the wrench form: what (a) costs)
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box;
the MEDIAN over `--rounds` rounds is reported, the rounds beside it.  Algorithmic bytes of the kernels: inputs read once,
outputs written once; their rate is given as a fraction of the 8.0 TB/s HBM peak of the MI355X (reported, no target).

    python tools/wrench_probe.py [--reps 50] [--rounds 7]
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

PEAK = 8.0e12
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("wrench_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    B, L = args.batch, len(TIPS)
    model = opt.pose_model(TIPS)
    n, n_fixed = model.n_in, model.n_fixed
    assert n_fixed == 0
    lim = prob.robot.joint_limits[prob.idx_pin2target]
    rng = np.random.default_rng(1)
    q = torch.tensor(rng.uniform(lim[:, 0], lim[:, 1], (B, n)).astype(np.float32), device="cuda")
    gen = torch.Generator("cuda").manual_seed(2)
    qd = torch.randn((B, n), device="cuda", generator=gen)
    force, torque = (torch.randn((B, L, 3), device="cuda", generator=gen) for _ in range(2))
    sp = torch.cuda.current_stream().cuda_stream
    tau, tau_e, gx, gxd = (torch.empty((B, n), device="cuda") for _ in range(4))
    jlin = torch.empty((B, L, 3, n), device="cuda")
    jang = torch.empty_like(jlin)
    lin, ang = torch.empty((B, L, 3), device="cuda"), torch.empty((B, L, 3), device="cuda")
    via = {}

    def a():
        model.wrenches_dev(B, q.data_ptr(), 0, force.data_ptr(), torque.data_ptr(), tau.data_ptr(), stream=sp)

    def b():
        model.jacobians_dev(B, q.data_ptr(), 0, jlin.data_ptr(), jang.data_ptr(), stream=sp)
        via["tau"] = torch.einsum("blrc,blr->bc", jlin, force) + torch.einsum("blrc,blr->bc", jang, torque)

    def c():
        model.velocities_dev(B, q.data_ptr(), 0, qd.data_ptr(), lin.data_ptr(), ang.data_ptr(), stream=sp)

    def d():
        model.velocities_vjp_dev(B, q.data_ptr(), 0, qd.data_ptr(), force.data_ptr(), torque.data_ptr(), gx.data_ptr(), gxd.data_ptr(), stream=sp)

    def e():
        model.velocities_vjp_dev(B, q.data_ptr(), 0, qd.data_ptr(), force.data_ptr(), torque.data_ptr(), 0, tau_e.data_ptr(), stream=sp)

    KA, KB, KC, KD, KE = ("(a) wrenches_dev", "(b) jacobians_dev + 2 einsum", "(c) velocities_dev (forward)",
                          "(d) velocities_vjp_dev, both outputs", "(e) velocities_vjp_dev, grad_xdot alone")
    runs = {KA: a, KB: b, KC: c, KD: d, KE: e}
    f = 4 * B
    nbytes = {KA: f * (n + 6 * L + n), KC: f * (2 * n + 6 * L), KD: f * (2 * n + 6 * L + 2 * n), KE: f * (n + 6 * L + n)}
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, args.reps, args.warmup))
    torch.cuda.synchronize()
    diff = float((tau - via["tau"]).abs().max())
    print(f"# wrench_probe: {torch.cuda.get_device_name(0)}, {REL}, links {TIPS}, B = {B}, n_in = {n}, float32")
    print(f"# HIP events around {args.reps} back-to-back runs after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    print(f"# max |tau of (a) - tau of (b)| = {diff:.3e} at max |tau| = {float(tau.abs().max()):.3f}; (e) equals (a) bit for bit: {bool(torch.equal(tau, tau_e))}; "
          f"grad_xdot of (d) equals (a) bit for bit: {bool(torch.equal(tau, gxd))}")
    print(f"{'variant':42s} {'us':>9s} {'rounds (us)':>58s} {'bytes':>12s} {'of 8.0 TB/s':>11s}")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        frac = "" if k not in nbytes else f"{nbytes[k] / (med[k] * 1e-6) / PEAK:11.4f}"
        print(f"{k:42s} {med[k]:9.2f} {' '.join(f'{v:7.2f}' for v in t[k]):>58s} {nbytes.get(k, ''):>12} {frac:>11s}")
    print(f"# (b) / (a) = {med[KB] / med[KA]:.2f}; (d) / (c) = {med[KD] / med[KC]:.2f}; (e) / (a) = {med[KE] / med[KA]:.2f}")
    if not med[KA] < med[KB]:
        print("# (a) is NOT faster than (b)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""GPU box: time of the link-Jacobian kernel (dexr_link_jacobians_dev) next to the only route to the same matrix that
existed before it, 3 L launches of the link-pose VJP kernel with one-hot cotangents.  Read-only use of the library.

Workload: Allegro vector config, its four tip links, B = 65 536, float32, the optimiser's variables as columns.
  (a) one jacobians_dev call, linear block only
  (b) one jacobians_dev call, linear and angular block
  (c) 3 L vjp_dev launches with one-hot grad_pos into a (3 L, B, n) buffer, then one copy into the preallocated (B, L, 3, n)
      tensor (the VJP kernel writes contiguous (B, n) rows, it cannot write the strided slice itself); (c') the launches alone
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same
box; the MINIMUM over `--rounds` rounds is reported.  Algorithmic bytes: 4 B (n_in + n_fixed) read, 4 B L (3 | 6) n_in
written; their rate is given as a fraction of the 8.0 TB/s HBM peak of the MI355X.

    python tools/jacobian_probe.py [--reps 50] [--rounds 5]
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402

PEAK = 8.0e12
REL = "teleop/allegro_hand_right.yml"
TIPS = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_11.0_tip"]


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
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    B, L = args.batch, len(TIPS)
    model = opt.pose_model(TIPS)
    n, n_fixed = model.n_in, model.n_fixed
    assert n_fixed == 0
    lim = prob.robot.joint_limits[prob.idx_pin2target]
    q = torch.tensor(np.random.default_rng(1).uniform(lim[:, 0], lim[:, 1], (B, n)).astype(np.float32), device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    jlin = torch.empty((B, L, 3, n), device="cuda")
    jang = torch.empty_like(jlin)
    via_vjp = torch.empty_like(jlin)
    rows = torch.empty((3 * L, B, n), device="cuda")
    onehot = torch.zeros((3 * L, B, L, 3), device="cuda")
    for l in range(L):
        for r in range(3):
            onehot[3 * l + r, :, l, r] = 1.0

    def a():
        model.jacobians_dev(B, q.data_ptr(), 0, jlin.data_ptr(), 0, stream=sp)

    def b():
        model.jacobians_dev(B, q.data_ptr(), 0, jlin.data_ptr(), jang.data_ptr(), stream=sp)

    def c_launches():
        for i in range(3 * L):
            model.vjp_dev(B, q.data_ptr(), 0, onehot[i].data_ptr(), 0, rows[i].data_ptr(), stream=sp)

    def c():
        c_launches()
        via_vjp.view(B, 3 * L, n).copy_(rows.permute(1, 0, 2))

    KA, KB, KC, KC1 = ("(a) jacobians_dev, linear", "(b) jacobians_dev, linear + angular", "(c) 3L vjp_dev launches + copy",
                       "(c') 3L vjp_dev launches alone")
    runs = {KA: a, KB: b, KC: c, KC1: c_launches}
    blocks = {KA: 3, KB: 6}  # rows of J a variant writes (the yardstick's traffic is not the algorithm's: no fraction)
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, args.reps, args.warmup))
    torch.cuda.synchronize()
    diff = float((jlin - via_vjp).abs().max())
    print(f"# jacobian_probe: {torch.cuda.get_device_name(0)}, {REL}, links {TIPS}, B = {B}, n_in = {n}, float32")
    print(f"# HIP events around {args.reps} back-to-back runs after {args.warmup} warm-up runs; minimum of {args.rounds} alternating rounds")
    print(f"# max |jlin of (a) - jlin assembled by (c)| = {diff:.3e}")
    print(f"{'variant':40s} {'us':>9s} {'rounds (us)':>40s} {'bytes':>12s} {'of 8.0 TB/s':>11s}")
    for k in runs:
        us = min(t[k])
        nbytes = 4 * B * (n + n_fixed) + 4 * B * L * blocks[k] * n if k in blocks else None
        frac = "" if nbytes is None else f"{nbytes / (us * 1e-6) / PEAK:11.4f}"
        print(f"{k:40s} {us:9.2f} {' '.join(f'{v:7.2f}' for v in t[k]):>40s} {'' if nbytes is None else nbytes:>12} {frac:>11s}")
    print(f"# (c) / (a) = {min(t[KC]) / min(t[KA]):.2f}; (c') / (a) = {min(t[KC1]) / min(t[KA]):.2f}")
    if not min(t[KA]) < min(t[KC]):
        print("# (a) is NOT faster than (c)")
        sys.exit(1)


if __name__ == "__main__":
    main()

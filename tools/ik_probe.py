#!/usr/bin/env python3
"""GPU box: time of the fused damped least-squares IK step (dexr_link_ik_step_dev) next to what a user wrote before it --
link_jacobians, einsums for the normal equations and a batched torch.linalg Cholesky solve -- and next to the wrench kernel
alone, the floor of one walk over the table.  Read-only use of the library.

Workload: Shadow hand vector config, its five tip links, B = 65 536, float32, the optimiser's variables as columns; position and
rotation rows, both weighted.
  (a) one ik_step_dev call                                                     writes 4 B n_in per frame
  (b) jacobians_dev, both blocks, then H = einsum(w, J, J) + damping I, g = einsum(w, J, e) for both blocks,
      torch.linalg.cholesky_ex and torch.cholesky_solve                        writes 4 B 2 L 3 n_in per frame and reads it again, twice
  (c) one wrenches_dev call on the same rows (J^T e without H, without a solve)
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box;
the MEDIAN over `--rounds` rounds is reported, the rounds beside it.

    python tools/ik_probe.py [--reps 20] [--rounds 7]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("ik_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    B, L = args.batch, len(TIPS)
    model = opt.pose_model(TIPS)
    n = model.n_in
    assert model.n_fixed == 0
    lim = prob.robot.joint_limits[prob.idx_pin2target]
    rng = np.random.default_rng(1)
    q = torch.tensor(rng.uniform(lim[:, 0], lim[:, 1], (B, n)).astype(np.float32), device="cuda")
    gen = torch.Generator("cuda").manual_seed(2)
    el, ea = 0.01 * torch.randn((B, L, 3), device="cuda", generator=gen), 0.1 * torch.randn((B, L, 3), device="cuda", generator=gen)
    wl, wa = (0.5 + 1.5 * torch.rand((B, L), device="cuda", generator=gen) for _ in range(2))
    fl, fa = wl[..., None] * el, wa[..., None] * ea
    sp = torch.cuda.current_stream().cuda_stream
    dx, tau = torch.empty((B, n), device="cuda"), torch.empty((B, n), device="cuda")
    jlin = torch.empty((B, L, 3, n), device="cuda")
    jang = torch.empty_like(jlin)
    eye = torch.eye(n, device="cuda")
    # damping: 1e-3 of the largest eigenvalue of J^T W J over the first 1024 frames (the rule of tests/test_gpu_ik.py)
    model.jacobians_dev(B, q.data_ptr(), 0, jlin.data_ptr(), jang.data_ptr(), stream=sp)
    H0 = torch.einsum("bl,blri,blrj->bij", wl[:1024], jlin[:1024], jlin[:1024]) + torch.einsum("bl,blri,blrj->bij", wa[:1024], jang[:1024], jang[:1024])
    lam = float(np.float32(1e-3 * float(torch.linalg.eigvalsh(H0.double().cpu())[:, -1].max())))
    via = {}

    def a():
        model.ik_step_dev(B, q.data_ptr(), 0, el.data_ptr(), ea.data_ptr(), wl.data_ptr(), wa.data_ptr(), lam, dx.data_ptr(), stream=sp)

    def b():
        model.jacobians_dev(B, q.data_ptr(), 0, jlin.data_ptr(), jang.data_ptr(), stream=sp)
        H = torch.einsum("bl,blri,blrj->bij", wl, jlin, jlin) + torch.einsum("bl,blri,blrj->bij", wa, jang, jang) + lam * eye
        g = torch.einsum("blri,blr->bi", jlin, fl) + torch.einsum("blri,blr->bi", jang, fa)
        Lc, _ = torch.linalg.cholesky_ex(H)
        via["dx"] = torch.cholesky_solve(g[..., None], Lc)[..., 0]

    def c():
        model.wrenches_dev(B, q.data_ptr(), 0, fl.data_ptr(), fa.data_ptr(), tau.data_ptr(), stream=sp)

    KA, KB, KC = "(a) ik_step_dev", "(b) jacobians_dev + einsum + cholesky_ex + cholesky_solve", "(c) wrenches_dev alone"
    runs = {KA: a, KB: b, KC: c}
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, args.reps, args.warmup))
    torch.cuda.synchronize()
    diff = float((dx - via["dx"]).abs().max())
    print(f"# ik_probe: {torch.cuda.get_device_name(0)}, {REL}, links {TIPS}, B = {B}, n_in = {n}, float32, damping {lam:.3e}")
    print(f"# HIP events around {args.reps} back-to-back runs after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    print(f"# max |dx of (a) - dx of (b)| = {diff:.3e} at max |dx| = {float(dx.abs().max()):.3f}")
    print(f"{'variant':60s} {'us':>10s}   rounds (us)")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        print(f"{k:60s} {med[k]:10.2f}   {' '.join(f'{v:9.2f}' for v in t[k])}")
    print(f"# (b) / (a) = {med[KB] / med[KA]:.2f}; (a) / (c) = {med[KA] / med[KC]:.2f}")
    if not med[KA] < med[KB]:
        print("# (a) is NOT faster than (b)")


if __name__ == "__main__":
    main()

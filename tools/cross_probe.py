#!/usr/bin/env python3
"""GPU box: time of the fused penalty between two posed robots (dexr_cross_penalty_dev: energy, both gradients and both wrenches
from one launch) next to the same loss written in torch, the route a user had before it.  Read-only use of the library.

Workload: the Shadow hand vector configs, right (robot A) against left (robot B), the optimisers' variables as columns, float32,
q uniform inside the limits; the 48-sphere set of tools/collision_probe.py on each (radius 0.012); the right base at the origin
with the identity, the left base with a seeded rotation per frame and placed so that the centroid of its spheres at q = 0 lies
within 4 cm of the centroid of the right hand's; margin 0.010; weights of 1.
  (a) one cross_penalty_dev call: E, dE/dq_a, dE/dq_b, wrench_a, wrench_b
  (b) torch: autograd.link_poses with rotations for both hands, an einsum for the centres, the base pose of B, cdist over
      (B, S_a, S_b), hinge, sum, backward() to q_a, q_b and pos_b (the force half of wrench_b; the torques are not formed)
  (c) the fused obstacle penalty of tools/obstacle_probe.py on its 16 primitives (E and dE/dq, one launch): the scale of what a
      fused collision launch costs
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box; the
MEDIAN over `--rounds` rounds is reported, the rounds beside it.  (a) and (b) compute the same E and gradients (the differences are
printed).

    python tools/cross_probe.py [--reps 10] [--rounds 7] [--batches 2048,65536]
"""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from collision_probe import RADIUS, sphere_set, timed  # noqa: E402
from obstacle_probe import obstacle_set, rotations  # noqa: E402
from dex_retargeting_amd import autograd as ag  # noqa: E402
from dex_retargeting_amd import collision  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402

REL_A, REL_B, N_SPHERE, MARGIN = "teleop/shadow_hand_right.yml", "teleop/shadow_hand_left.yml", 48, 0.010


class Hand:
    def __init__(self, torch, rel, B, seed):
        self.opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
        prob = cases.problem_from_config(rel)
        self.sset = sphere_set(self.opt, N_SPHERE)
        self.model = self.opt.sphere_model(self.sset)
        assert self.model.n_fixed == 0 and self.model.n_sphere == N_SPHERE
        self.n = self.model.n_in
        lim = prob.robot.joint_limits[prob.idx_pin2target].astype(np.float32)
        self.q = torch.tensor(np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (B, self.n)).astype(np.float32), device="cuda")
        self.links = list(self.sset.table_links)
        self.rows = torch.tensor(self.sset.sphere_rows.astype(np.int64), device="cuda")
        self.cen = torch.tensor(self.sset.centers.astype(np.float32), device="cuda")
        self.rad = torch.tensor(self.sset.radii.astype(np.float32), device="cuda")
        self.home = collision.sphere_distances(self.opt, torch.zeros((1, self.n), device="cuda"), self.sset, centers=True)[1][0].mean(0).cpu().numpy()

    def centres(self, torch, q):
        lp, lr = ag.link_poses(self.opt, q, self.links, None, rotations=True)
        return lp[:, self.rows] + torch.einsum("bsij,sj->bsi", lr[:, self.rows], self.cen)


def probe(torch, B, args):
    A, Bh = Hand(torch, REL_A, B, 2), Hand(torch, REL_B, B, 3)
    rng = np.random.default_rng(4)
    rot_np = rotations(rng, B)
    pos_np = A.home + rng.uniform(-0.04, 0.04, (B, 3)) - np.einsum("bij,j->bi", rot_np, Bh.home)
    rot_b = torch.tensor(rot_np.astype(np.float32), device="cuda")
    pos_b = torch.tensor(pos_np.astype(np.float32), device="cuda")
    oset = obstacle_set()
    handle = oset.device_set(torch.cuda.current_device())
    opos = torch.tensor((A.home + rng.uniform(-0.03, 0.03, (B, 3))).astype(np.float32), device="cuda")
    orot = torch.tensor(rotations(rng, B).astype(np.float32), device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    e = torch.empty((B,), device="cuda")
    ga, gb = torch.empty((B, A.n), device="cuda"), torch.empty((B, Bh.n), device="cuda")
    wa, wb = torch.empty((B, 6), device="cuda"), torch.empty((B, 6), device="cuda")
    eo, go = torch.empty((B,), device="cuda"), torch.empty((B, A.n), device="cuda")
    out = {}

    def a():
        A.model.cross_penalty_dev(Bh.model, B, A.q.data_ptr(), 0, Bh.q.data_ptr(), 0, MARGIN, 0, e.data_ptr(), ga.data_ptr(), gb.data_ptr(), wa.data_ptr(),
                                  wb.data_ptr(), pos_b_ptr=pos_b.data_ptr(), rot_b_ptr=rot_b.data_ptr(), stream=sp)

    def b():
        qa, qb, pb = A.q.detach().requires_grad_(True), Bh.q.detach().requires_grad_(True), pos_b.detach().requires_grad_(True)
        ca = A.centres(torch, qa)
        cb = pb[:, None] + torch.einsum("bij,bsj->bsi", rot_b, Bh.centres(torch, qb))
        h = (MARGIN - (torch.cdist(ca, cb) - (A.rad[:, None] + Bh.rad[None]))).clamp_min(0.0)
        E = (h * h).sum((1, 2))
        E.sum().backward()
        out["E"], out["ga"], out["gb"], out["fb"] = E.detach(), qa.grad, qb.grad, pb.grad

    def c():
        A.model.obstacle_penalty_dev(handle, B, A.q.data_ptr(), 0, MARGIN, 0, eo.data_ptr(), go.data_ptr(), 0, opos.data_ptr(), orot.data_ptr(), stream=sp)

    KA, KB = "(a) cross_penalty_dev: E, both gradients, both wrenches, one launch", "(b) torch: link_poses x 2, einsum, cdist, hinge, backward"
    KC = "(c) obstacle_penalty_dev on 16 primitives: E and dE/dq, one launch"
    runs = {KA: a, KB: b, KC: c}
    reps = args.reps if B >= 65536 else 10 * args.reps  # small batches: enough work inside a window
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, reps, args.warmup))
    torch.cuda.synchronize()
    da, db = collision.cross_distances(A.opt, A.q, A.sset, Bh.opt, Bh.q, Bh.sset, None, None, pos_b, rot_b)
    print(f"\n# {REL_A} against {REL_B}: B = {B}, n_in = {A.n} + {Bh.n}, {N_SPHERE} x {N_SPHERE} spheres (radius {RADIUS}), a pose per frame, margin "
          f"{MARGIN}; spheres of A within the margin of B {float((da < MARGIN).float().mean()):.4f}, frames with one {float((da < MARGIN).any(1).float().mean()):.3f}")
    print(f"# max |E| {float(e.abs().max()):.3e}, max |dE/dq_a| {float(ga.abs().max()):.3e}, max |force| {float(wb[:, :3].abs().max()):.3e}; max |E(a) - E(b)| = "
          f"{float((e - out['E']).abs().max()):.3e}, max |grad_a(a) - grad_a(b)| = {float((ga - out['ga']).abs().max()):.3e}, max |grad_b(a) - grad_b(b)| = "
          f"{float((gb - out['gb']).abs().max()):.3e}, max |force_b(a) - force_b(b)| = {float((wb[:, :3] - out['fb']).abs().max()):.3e}")
    print(f"{'variant':72s} {'us':>10s}   rounds (us)")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        print(f"{k:72s} {med[k]:10.2f}   {' '.join(f'{v:9.2f}' for v in t[k])}   range {min(t[k]):.2f} .. {max(t[k]):.2f}")
    print(f"# (b) / (a) = {med[KB] / med[KA]:.2f}; (a) / (c) = {med[KA] / med[KC]:.2f}; (a) = {med[KA] * 1e3 / B:.2f} ns per frame, "
          f"{med[KA] * 1e3 / (B * N_SPHERE * N_SPHERE):.4f} ns per (sphere, sphere) pair")
    if not med[KA] < med[KB]:
        print("# (a) is NOT faster than (b)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2048,65536")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("cross_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    print(f"# cross_probe: {torch.cuda.get_device_name(0)}, float32; HIP events around {args.reps} back-to-back runs (ten times as many below "
          f"B = 65 536) after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    for B in (int(v) for v in args.batches.split(",")):
        probe(torch, B, args)


if __name__ == "__main__":
    main()

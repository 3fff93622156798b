#!/usr/bin/env python3
"""GPU box: time of the fused obstacle penalty (dexr_obstacle_penalty_dev: energy and gradient from one launch) next to the same
loss written in torch, the route a user had before it.  Read-only use of the library.

Workload: the Shadow hand vector config, the optimiser's variables as columns, float32, q uniform inside the limits; the
48-sphere set of tools/collision_probe.py (radius 0.012); 16 primitives, four of each kind, a few centimetres across, seeded; one
obstacle pose per frame: a seeded rotation and the origin within 3 cm of the hand's centroid at q = 0 (a held object); margin
0.010; weights of 1.
  (a) one obstacle_penalty_dev call: E and dE/dq
  (b) torch: autograd.link_poses with rotations, an einsum for the centres, the centres in the obstacle frame, the four signed
      distance functions written with torch operations over (B, S, 4) at a time, hinge, sum, backward() to q
HIP events around `--reps` back-to-back runs after `--warmup`; the two variants alternate inside a round so both see the same
box; the MEDIAN over `--rounds` rounds is reported, the rounds beside it.  Both compute the same E and dE/dq (the differences
are printed).

    python tools/obstacle_probe.py [--reps 10] [--rounds 7] [--batches 2048,65536]
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
from dex_retargeting_amd import autograd as ag  # noqa: E402
from dex_retargeting_amd import collision  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402

REL, N_SPHERE, MARGIN = "teleop/shadow_hand_right.yml", 48, 0.010


def rotations(rng, n):
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(-np.pi, np.pi, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)


def obstacle_set():
    """four spheres, four capsules, four boxes, four half-spaces (the kinds in blocks, which the torch route relies on)."""
    rng = np.random.default_rng(3)
    O = collision.ObstacleSet
    c = lambda: rng.uniform(-0.06, 0.06, (4, 3))  # noqa: E731
    a = c()
    n = rng.standard_normal((4, 3))
    return (O.spheres(c(), rng.uniform(0.005, 0.02, 4)) + O.capsules(a, a + rng.uniform(-0.04, 0.04, (4, 3)), rng.uniform(0.005, 0.015, 4))
            + O.boxes(c(), rng.uniform(0.01, 0.03, (4, 3)), rotations(rng, 4)) + O.half_spaces(n / np.linalg.norm(n, axis=1, keepdims=True), rng.uniform(-0.12, -0.08, 4)))


def torch_sdf(torch, oset, y):
    """y (B, S, 3) -> sdf (B, S, 16): the definitions of include/dexr_obstacles.h with torch operations, four primitives of a kind at a time."""
    t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=y.device)  # noqa: E731
    p = oset.params
    Y = y[:, :, None, :]
    sph = (Y - t(p[0:4, 0:3])).norm(dim=-1) - t(p[0:4, 3])
    a, ab = t(p[4:8, 0:3]), t(p[4:8, 3:6] - p[4:8, 0:3])
    tt = (((Y - a) * ab).sum(-1) / (ab * ab).sum(-1)).clamp(0.0, 1.0)
    cap = (Y - (a + tt[..., None] * ab)).norm(dim=-1) - t(p[4:8, 6])
    R = t(p[8:12, 6:15].reshape(4, 3, 3))
    q = torch.einsum("bsmj,mji->bsmi", Y - t(p[8:12, 0:3]), R).abs() - t(p[8:12, 3:6])
    box = torch.where(q.amax(-1) <= 0, q.amax(-1), q.clamp_min(0.0).norm(dim=-1))
    half = (Y * t(p[12:16, 0:3])).sum(-1) - t(p[12:16, 3])
    return torch.cat([sph, cap, box, half], -1)


def probe(torch, B, args):
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    sset = sphere_set(opt, N_SPHERE)
    oset = obstacle_set()
    assert oset.kinds.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    model = opt.sphere_model(sset)
    assert model.n_fixed == 0 and model.n_sphere == N_SPHERE
    n = model.n_in
    lim = prob.robot.joint_limits[prob.idx_pin2target].astype(np.float32)
    rng = np.random.default_rng(2)
    q = torch.tensor(rng.uniform(lim[:, 0], lim[:, 1], (B, n)).astype(np.float32), device="cuda")
    links = list(sset.table_links)
    rows = torch.tensor(sset.sphere_rows.astype(np.int64), device="cuda")
    cen = torch.tensor(sset.centers.astype(np.float32), device="cuda")
    rad = torch.tensor(sset.radii.astype(np.float32), device="cuda")
    home = collision.sphere_distances(opt, torch.zeros((1, n), device="cuda"), sset, centers=True)[1][0].mean(0).cpu().numpy()
    pos = torch.tensor((home + rng.uniform(-0.03, 0.03, (B, 3))).astype(np.float32), device="cuda")
    rot = torch.tensor(rotations(rng, B).astype(np.float32), device="cuda")
    handle = oset.device_set(torch.cuda.current_device())
    sp = torch.cuda.current_stream().cuda_stream
    ea, ga = torch.empty((B,), device="cuda"), torch.empty((B, n), device="cuda")
    out = {}

    def a():
        model.obstacle_penalty_dev(handle, B, q.data_ptr(), 0, MARGIN, 0, ea.data_ptr(), ga.data_ptr(), 0, pos.data_ptr(), rot.data_ptr(), stream=sp)

    def b():
        qg = q.detach().requires_grad_(True)
        lp, lr = ag.link_poses(opt, qg, links, None, rotations=True)
        ctr = lp[:, rows] + torch.einsum("bsij,sj->bsi", lr[:, rows], cen)
        y = torch.einsum("bji,bsj->bsi", rot, ctr - pos[:, None])
        h = (MARGIN - (torch_sdf(torch, oset, y) - rad[None, :, None])).clamp_min(0.0)
        E = (h * h).sum((1, 2))
        E.sum().backward()
        out["E"], out["g"] = E.detach(), qg.grad

    KA, KB = "(a) obstacle_penalty_dev: E and dE/dq, one launch", "(b) torch: link_poses, einsum, torch SDFs, hinge, backward"
    runs = {KA: a, KB: b}
    reps = args.reps if B >= 65536 else 10 * args.reps  # small batches: enough work inside a window
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, reps, args.warmup))
    torch.cuda.synchronize()
    dist = collision.obstacle_distances(opt, q, sset, oset, pos, rot)
    print(f"\n# {REL}: B = {B}, n_in = {n}, {N_SPHERE} spheres (radius {RADIUS}) x {oset.n_prim} primitives, a pose per frame, margin {MARGIN}; "
          f"spheres within the margin of a primitive {float((dist < MARGIN).float().mean()):.4f}, frames with one {float((dist < MARGIN).any(1).float().mean()):.3f}")
    print(f"# max |E| {float(ea.abs().max()):.3e}, max |dE/dq| {float(ga.abs().max()):.3e}; max |E(a) - E(b)| = {float((ea - out['E']).abs().max()):.3e}, "
          f"max |grad(a) - grad(b)| = {float((ga - out['g']).abs().max()):.3e}")
    print(f"{'variant':64s} {'us':>10s}   rounds (us)")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        print(f"{k:64s} {med[k]:10.2f}   {' '.join(f'{v:9.2f}' for v in t[k])}")
    print(f"# (b) / (a) = {med[KB] / med[KA]:.2f}; (a) = {med[KA] * 1e3 / B:.2f} ns per frame, {med[KA] * 1e3 / (B * N_SPHERE * oset.n_prim):.3f} ns per "
          f"(sphere, primitive) entry")
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
        sys.exit("obstacle_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    print(f"# obstacle_probe: {torch.cuda.get_device_name(0)}, float32; HIP events around {args.reps} back-to-back runs (ten times as many below "
          f"B = 65 536) after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    for B in (int(v) for v in args.batches.split(",")):
        probe(torch, B, args)


if __name__ == "__main__":
    main()

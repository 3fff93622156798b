#!/usr/bin/env python3
"""GPU box: time of the fused self-collision penalty (dexr_sphere_penalty_dev: energy and gradient from one launch) next to the
distance + VJP pair of the same library and to the torch route a user had before it.  Read-only use of the library.

Workload: Shadow hand and Allegro hand vector configs, the optimiser's variables as columns, float32, q uniform inside the
limits.  Spheres of radius 0.012 at every link origin and a second, off-origin one on as many links as make 48 (Shadow) / 32
(Allegro) spheres; collision.default_pairs; margin 0.010; weights of 1.
  (a) one penalty_dev call: E and dE/dq
  (b) distances_dev, the hinge in torch (-2 max(0, margin - d)), distances_vjp_dev: two launches of the library and the
      (B, P) distances and cotangents in HBM
  (c) torch: autograd.link_poses with rotations, an einsum for the centres, a gather of the pair indices, norm, hinge, sum,
      backward()
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box;
the MEDIAN over `--rounds` rounds is reported, the rounds beside it.

    python tools/collision_probe.py [--reps 10] [--rounds 7] [--batches 1,2048,65536]
"""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dex_retargeting_amd import autograd as ag  # noqa: E402
from dex_retargeting_amd import collision  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402

ROBOTS = (("teleop/shadow_hand_right.yml", 48), ("teleop/allegro_hand_right.yml", 32))
RADIUS, MARGIN = 0.012, 0.010


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


def sphere_set(opt, n_sphere):
    links = [f.name for f in opt.robot.kin.frames]
    extra = n_sphere - len(links)
    assert 0 <= extra <= len(links)
    rng = np.random.default_rng(1)
    u = rng.standard_normal((extra, 3))
    off = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.005, 0.015, (extra, 1))
    centers = np.concatenate([np.zeros((len(links), 3)), off]).astype(np.float32).astype(np.float64)
    return collision.SphereSet(links + links[:extra], centers, np.full(n_sphere, RADIUS))


def probe(torch, rel, n_sphere, B, args):
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    sset = sphere_set(opt, n_sphere)
    model = opt.sphere_model(sset)
    assert model.n_fixed == 0
    pairs = collision.default_pairs(opt.robot, sset)
    n, P = model.n_in, model.n_pair
    lim = prob.robot.joint_limits[prob.idx_pin2target].astype(np.float32)
    q = torch.tensor(np.random.default_rng(2).uniform(lim[:, 0], lim[:, 1], (B, n)).astype(np.float32), device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    ea, ga = torch.empty((B,), device="cuda"), torch.empty((B, n), device="cuda")
    dist, gb = torch.empty((B, P), device="cuda"), torch.empty((B, n), device="cuda")
    out = {}
    links = list(sset.table_links)
    rows = torch.tensor(sset.sphere_rows.astype(np.int64), device="cuda")
    cen = torch.tensor(sset.centers.astype(np.float32), device="cuda")
    pi, pj = (torch.tensor(pairs[:, k].astype(np.int64), device="cuda") for k in (0, 1))
    rsum = torch.tensor((sset.radii[pairs[:, 0]] + sset.radii[pairs[:, 1]]).astype(np.float32), device="cuda")

    def a():
        model.penalty_dev(B, q.data_ptr(), 0, MARGIN, 0, ea.data_ptr(), ga.data_ptr(), stream=sp)

    def b():
        model.distances_dev(B, q.data_ptr(), 0, dist.data_ptr(), 0, stream=sp)
        h = (MARGIN - dist).clamp_min(0.0)
        out["Eb"] = (h * h).sum(-1)
        gd = (-2.0 * h).contiguous()
        model.distances_vjp_dev(B, q.data_ptr(), 0, gd.data_ptr(), gb.data_ptr(), stream=sp)

    def c():
        qg = q.detach().requires_grad_(True)
        pos, rot = ag.link_poses(opt, qg, links, None, rotations=True)
        ctr = pos[:, rows] + torch.einsum("bsij,sj->bsi", rot[:, rows], cen)
        D = ctr[:, pi] - ctr[:, pj]
        h = (MARGIN - (D.norm(dim=-1) - rsum)).clamp_min(0.0)
        E = (h * h).sum(-1)
        E.sum().backward()
        out["Ec"], out["gc"] = E.detach(), qg.grad

    KA, KB, KC = "(a) penalty_dev: E and dE/dq, one launch", "(b) distances_dev + hinge in torch + distances_vjp_dev", \
        "(c) torch: link_poses, einsum, gather, norm, hinge, backward"
    runs = {KA: a, KB: b, KC: c}
    reps = args.reps if B >= 65536 else 10 * args.reps  # small batches: enough work inside a window
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, reps, args.warmup))
    torch.cuda.synchronize()
    active = float((dist < MARGIN).float().mean())
    print(f"\n# {rel}: B = {B}, n_in = {n}, {n_sphere} spheres on {len(links)} links, {P} default pairs, radius {RADIUS}, margin {MARGIN}; "
          f"active share {active:.4f}, frames with an active pair {float((dist < MARGIN).any(1).float().mean()):.3f}")
    print(f"# max |E| {float(ea.abs().max()):.3e}, max |dE/dq| {float(ga.abs().max()):.3e}; max |E(a) - E(c)| = {float((ea - out['Ec']).abs().max()):.3e}, "
          f"max |grad(a) - grad(c)| = {float((ga - out['gc']).abs().max()):.3e}, max |grad(a) - grad(b)| = {float((ga - gb).abs().max()):.3e}")
    print(f"{'variant':64s} {'us':>10s}   rounds (us)")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        print(f"{k:64s} {med[k]:10.2f}   {' '.join(f'{v:9.2f}' for v in t[k])}")
    print(f"# (c) / (a) = {med[KC] / med[KA]:.2f}; (b) / (a) = {med[KB] / med[KA]:.2f}; (a) = {med[KA] * 1e3 / B:.2f} ns per frame")
    if not med[KA] < med[KC]:
        print("# (a) is NOT faster than (c)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2048,65536")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("collision_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    print(f"# collision_probe: {torch.cuda.get_device_name(0)}, float32; HIP events around {args.reps} back-to-back runs (ten times as many below "
          f"B = 65 536) after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    for rel, n_sphere in ROBOTS:
        for B in (int(v) for v in args.batches.split(",")):
            probe(torch, rel, n_sphere, B, args)


if __name__ == "__main__":
    main()

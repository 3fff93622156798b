#!/usr/bin/env python3
"""GPU box: time of the fused signed-distance-grid penalty (dexr_grid_penalty_dev: energy and gradient from one launch) next to the
fused primitive penalty on the primitives the grid was sampled from -- unchanged code, the yardstick for what a sphere phase costs
-- and next to the same grid loss written in torch, the route a user had before it.  Read-only use of the library.

Workload: that of tools/obstacle_probe.py -- the Shadow hand vector config, float32, q uniform inside the limits, its 48-sphere
set, its 16 primitives, one obstacle pose per frame (a held object), margin 0.010 -- and the union of those primitives sampled by
SdfGrid.from_obstacles on a box of 32 cm around the obstacle frame's origin, once on 64^3 (1 MB of samples) and once on 256^3
(64 MB: the limit, far beyond the 4 MB L2 of an XCD).
  (a) one grid_penalty_dev call on the 64^3 grid: E and dE/dq
  (b) the same on the 256^3 grid
  (c) one obstacle_penalty_dev call on the 16 primitives (its energy sums over every primitive, the grid's over the union: another
      loss, the same walk and phase C)
  (d) torch on the 64^3 grid: autograd.link_poses with rotations, an einsum for the centres, the centres in the obstacle frame,
      torch.nn.functional.grid_sample (trilinear, align_corners=True, border padding) plus the distance to the box, hinge, sum,
      backward() to q
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box; the
MEDIAN over `--rounds` rounds is reported, the rounds beside it.  (a) and (d) compute the same E and dE/dq (the differences are
printed).

    python tools/grid_probe.py [--reps 10] [--rounds 7] [--batches 65536]
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
from obstacle_probe import MARGIN, N_SPHERE, REL, obstacle_set, rotations  # noqa: E402
from dex_retargeting_amd import autograd as ag  # noqa: E402
from dex_retargeting_amd import collision  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402

BOX = 0.32  # metres: the side of the sampled box, centred on the origin of the obstacle frame


def sampled(oset, n):
    return collision.SdfGrid.from_obstacles(oset, -BOX / 2, BOX / (n - 1), n)


def torch_grid_sdf(torch, V, lo, hi, y):
    """y (B, S, 3) -> sdf (B, S) of include/dexr_sdf_grid.h with torch operations: grid_sample reads the interpolant at the nearest
    point of the box (border padding), the distance to the box is added.  V (1, 1, nx, ny, nz)."""
    yc = torch.minimum(torch.maximum(y, lo), hi)
    u = (2.0 * (yc - lo) / (hi - lo) - 1.0).flip(-1)  # grid_sample's x indexes the last dimension
    v = torch.nn.functional.grid_sample(V, u[None, :, :, None, :], mode="bilinear", padding_mode="border", align_corners=True)[0, 0, :, :, 0]
    e2 = ((y - yc) ** 2).sum(-1)
    return v + torch.where(e2 > 0, e2.clamp_min(1e-30).sqrt(), torch.zeros_like(e2))


def probe(torch, B, args):
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    sset = sphere_set(opt, N_SPHERE)
    oset = obstacle_set()
    g64, g256 = sampled(oset, 64), sampled(oset, 256)
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
    dev = torch.cuda.current_device()
    h64, h256, hprim = g64.device_grid(dev), g256.device_grid(dev), oset.device_set(dev)
    V = torch.tensor(g64.values, device="cuda")[None, None]
    lo = torch.tensor(g64.origin.astype(np.float32), device="cuda")
    hi = torch.tensor((g64.origin + g64.spacing * (np.array(g64.shape) - 1)).astype(np.float32), device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    e = {k: torch.empty((B,), device="cuda") for k in "abc"}
    g = {k: torch.empty((B, n), device="cuda") for k in "abc"}
    out = {}

    def a():
        model.grid_penalty_dev(h64, B, q.data_ptr(), 0, MARGIN, e["a"].data_ptr(), g["a"].data_ptr(), 0, pos.data_ptr(), rot.data_ptr(), stream=sp)

    def b():
        model.grid_penalty_dev(h256, B, q.data_ptr(), 0, MARGIN, e["b"].data_ptr(), g["b"].data_ptr(), 0, pos.data_ptr(), rot.data_ptr(), stream=sp)

    def c():
        model.obstacle_penalty_dev(hprim, B, q.data_ptr(), 0, MARGIN, 0, e["c"].data_ptr(), g["c"].data_ptr(), 0, pos.data_ptr(), rot.data_ptr(), stream=sp)

    def d():
        qg = q.detach().requires_grad_(True)
        lp, lr = ag.link_poses(opt, qg, links, None, rotations=True)
        ctr = lp[:, rows] + torch.einsum("bsij,sj->bsi", lr[:, rows], cen)
        y = torch.einsum("bji,bsj->bsi", rot, ctr - pos[:, None])
        h = (MARGIN - (torch_grid_sdf(torch, V, lo, hi, y) - rad[None, :])).clamp_min(0.0)
        E = (h * h).sum(1)
        E.sum().backward()
        out["E"], out["g"] = E.detach(), qg.grad

    KA, KB = "(a) grid_penalty_dev, 64^3: E and dE/dq, one launch", "(b) grid_penalty_dev, 256^3: E and dE/dq, one launch"
    KC, KD = "(c) obstacle_penalty_dev, the 16 primitives, one launch", "(d) torch: link_poses, einsum, grid_sample, hinge, backward"
    runs = {KA: a, KB: b, KC: c, KD: d}
    reps = args.reps if B >= 65536 else 10 * args.reps  # small batches: enough work inside a window
    t = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            t[k].append(timed(torch, fn, reps, args.warmup))
    torch.cuda.synchronize()
    dist = collision.grid_distances(opt, q, sset, g64, pos, rot)
    lo_n, hi_n = lo.cpu().numpy(), hi.cpu().numpy()
    print(f"\n# {REL}: B = {B}, n_in = {n}, {N_SPHERE} spheres (radius {RADIUS}), a pose per frame, margin {MARGIN}; grids of {BOX} m sampled from "
          f"{oset.n_prim} primitives ({lo_n[0]:.2f} .. {hi_n[0]:.2f} m); spheres within the margin {float((dist < MARGIN).float().mean()):.4f}, frames "
          f"with one {float((dist < MARGIN).any(1).float().mean()):.3f}")
    print(f"# max |E| {float(e['a'].abs().max()):.3e}, max |dE/dq| {float(g['a'].abs().max()):.3e}; max |E(a) - E(d)| = "
          f"{float((e['a'] - out['E']).abs().max()):.3e}, max |grad(a) - grad(d)| = {float((g['a'] - out['g']).abs().max()):.3e}; "
          f"max |E(a) - E(b)| = {float((e['a'] - e['b']).abs().max()):.3e} (another sampling of the same shape)")
    print(f"{'variant':64s} {'us':>10s}   rounds (us)")
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in runs:
        print(f"{k:64s} {med[k]:10.2f}   {' '.join(f'{v:9.2f}' for v in t[k])}")
    print(f"# (b) / (a) = {med[KB] / med[KA]:.2f}; (a) / (c) = {med[KA] / med[KC]:.2f}; (d) / (a) = {med[KD] / med[KA]:.2f}; (a) = "
          f"{med[KA] * 1e3 / B:.2f} ns per frame, {med[KA] * 1e3 / (B * N_SPHERE):.3f} ns per sphere")
    if not med[KA] < med[KD]:
        print("# (a) is NOT faster than (d)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="65536")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("grid_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    print(f"# grid_probe: {torch.cuda.get_device_name(0)}, float32; HIP events around {args.reps} back-to-back runs (ten times as many below "
          f"B = 65 536) after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    for B in (int(v) for v in args.batches.split(",")):
        probe(torch, B, args)


if __name__ == "__main__":
    main()

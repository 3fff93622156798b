#!/usr/bin/env python3
"""GPU box: time of the fused posture solve against a scene of several posed bodies (dexr_sphere_resolve_scene_dev: self-collision,
every body's term, fingertip targets and the accept / reject iteration inside one kernel) next to the single-body solves of the
same build at the same shapes.  Read-only use of the library.

Workload: tools/resolve_grid_probe.py's (Shadow hand vector config, B = 65 536, float32, q uniform inside the limits, the 48-sphere
set with collision.default_pairs (1 007 pairs), margin 0.010, position targets on the five fingertips, posture weight 1e-4, damping
1e-4, max_step 0.2, the joint limits, tol = 0, the 16 primitives and the pose per frame of tools/obstacle_probe.py, their union
sampled on 64^3); the TABLE is one world-fixed half-space (no pose) that fills y < offset, the offset at the 0.3 quantile over the
batch of the lowest sphere, so that about a third of the frames touch it; 8 and 16 trial steps.
  (p1)  resolve_scene_dev, one body: the 16 primitives           against  (a) resolve_obstacles_dev on them: what the generality costs
  (g1)  resolve_scene_dev, one body: the 64^3 grid               against  (g) resolve_grid_dev on it:        the same for a grid
  (tp)  resolve_scene_dev, two bodies: the table + the primitives          (tp) - (p1): what the second body costs
  (tg)  resolve_scene_dev, two bodies: the table + the grid                (tg) - (g1)
  (s)   resolve_dev on the same frames, no obstacle at all
The two-body scenes minimise ANOTHER energy than the one-body ones (the table is there): their frames take other paths and stop at
other trial counts, so (tp) - (p1) is the cost of the second body on this workload, not of its instructions alone.  The same
iteration written in torch is not timed here (tools/resolve_grid_probe.py times it for one body).
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box; the
MEDIAN over `--rounds` rounds is reported, the rounds and their range beside it.

    python tools/resolve_scene_probe.py [--reps 5] [--rounds 5] [--iters 8,16] [--batch 65536]
"""
import argparse
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from dex_retargeting_amd import _lib  # noqa: E402
from dex_retargeting_amd import autograd as ag  # noqa: E402
from dex_retargeting_amd import collision  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402

from collision_probe import MARGIN, sphere_set, timed  # noqa: E402
from grid_probe import sampled  # noqa: E402
from obstacle_probe import obstacle_set, rotations  # noqa: E402
from resolve_probe import DAMPING, MAX_STEP, N_SPHERE, REL, TIPS, U  # noqa: E402

TABLE_Q = 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", default="8,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("resolve_scene_probe: no GPU (a timing needs one)")
    if args.rounds < 3:
        sys.exit("resolve_scene_probe: at least 3 rounds")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    sset = sphere_set(opt, N_SPHERE)
    oset = obstacle_set()
    grid = sampled(oset, 64)
    pairs = collision.default_pairs(opt.robot, sset)
    model = opt.sphere_model(sset, pairs, TIPS)
    assert model.n_fixed == 0 and oset.n_prim == 16
    B, n = args.batch, model.n_in
    lim_np = prob.robot.joint_limits[prob.idx_pin2target].astype(np.float32)
    lim = torch.tensor(lim_np, device="cuda")
    rng = np.random.default_rng(2)
    q = torch.tensor(rng.uniform(lim_np[:, 0], lim_np[:, 1], (B, n)).astype(np.float32), device="cuda")
    tp = ag.link_poses(opt, q, TIPS, None, rotations=False)[0].contiguous()
    home = collision.sphere_distances(opt, torch.zeros((1, n), device="cuda"), sset, centers=True)[1][0].mean(0).cpu().numpy()
    pos = torch.tensor((home + rng.uniform(-0.03, 0.03, (B, 3))).astype(np.float32), device="cuda")
    rot = torch.tensor(rotations(rng, B).astype(np.float32), device="cuda")
    cen = collision.sphere_distances(opt, q, sset, centers=True)[1]
    radii = torch.tensor(sset.radii.astype(np.float32), device="cuda")
    offset = float(torch.quantile((cen[:, :, 1] - radii).min(1).values[:1 << 20], TABLE_Q))
    table = collision.ObstacleSet.half_spaces([[0.0, 1.0, 0.0]], [offset])
    SB = collision.SceneBody
    scenes = {"p1": [SB(oset, pos, rot)], "g1": [SB(grid, pos, rot)], "tp": [SB(table), SB(oset, pos, rot)], "tg": [SB(table), SB(grid, pos, rot)]}
    print(f"# resolve_scene_probe: {torch.cuda.get_device_name(0)}, float32, library {_lib.LIB_PATH}; {REL}: B = {B}, n_in = {n}, {N_SPHERE} spheres, "
          f"{len(pairs)} default pairs, {oset.n_prim} primitives (and their union on 64^3) with a pose per frame, a world-fixed table at y < {offset:.4f}, "
          f"{len(TIPS)} tip targets; HIP events around {args.reps} back-to-back runs after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    for iters in (int(v) for v in args.iters.split(",")):
        out = {}

        def scene(which):
            def run():
                out[which] = collision.resolve_scene_collisions(opt, q, sset, scenes[which], MARGIN, DAMPING, iters, U, link_names=TIPS, target_pos=tp,
                                                                max_step=MAX_STEP, limits=lim, body_energy=True)
            return run

        def a():
            out["a"] = collision.resolve_collisions(opt, q, sset, oset, MARGIN, None, pos, rot, 1.0, None, DAMPING, iters, U, link_names=TIPS,
                                                    target_pos=tp, max_step=MAX_STEP, limits=lim)

        def g():
            out["g"] = collision.resolve_grid_collisions(opt, q, sset, grid, MARGIN, None, pos, rot, 1.0, DAMPING, iters, U, link_names=TIPS, target_pos=tp,
                                                         max_step=MAX_STEP, limits=lim)

        def s():
            out["s"] = collision.resolve_self_collision(opt, q, sset, MARGIN, DAMPING, iters, U, link_names=TIPS, target_pos=tp, max_step=MAX_STEP, limits=lim)

        K = {"p1": f"(p1) resolve_scene_dev, one body, the 16 primitives: {iters} trial steps, one launch",
             "a": f"(a) resolve_obstacles_dev, the 16 primitives: {iters} trial steps, one launch",
             "g1": f"(g1) resolve_scene_dev, one body, the 64^3 grid: {iters} trial steps, one launch",
             "g": f"(g) resolve_grid_dev, the 64^3 grid: {iters} trial steps, one launch",
             "tp": f"(tp) resolve_scene_dev, the table + the 16 primitives: {iters} trial steps, one launch",
             "tg": f"(tg) resolve_scene_dev, the table + the 64^3 grid: {iters} trial steps, one launch",
             "s": f"(s) resolve_dev (no obstacles): {iters} trial steps, one launch"}
        runs = {"p1": scene("p1"), "a": a, "g1": scene("g1"), "g": g, "tp": scene("tp"), "tg": scene("tg"), "s": s}
        t = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t[k].append(timed(torch, fn, args.reps, args.warmup))
        torch.cuda.synchronize()
        for one, sib in (("p1", "a"), ("g1", "g")):
            same = all(torch.equal(u, v) for u, v in zip(out[one][:4], out[sib]))
            print(f"\n# {iters} trial steps: ({one}) against ({sib}): the same bits on every frame: {same}; max |x| difference "
                  f"{float((out[one][0] - out[sib][0]).abs().max()):.3e}; E_obs equals the body energy column: {torch.equal(out[one][2][:, 3], out[one][4][:, 0])}")
        for two, one in (("tp", "p1"), ("tg", "g1")):
            x2, it2, en2, st2, be2 = out[two]
            print(f"# ({two}): frames that touch the table at the answer {float((be2[:, 0] > 0).float().mean()):.3f}, the object {float((be2[:, 1] > 0).float().mean()):.3f}; "
                  f"body energies (median of the touching frames) table {float(be2[:, 0][be2[:, 0] > 0].median()):.3e}, object {float(be2[:, 1][be2[:, 1] > 0].median()):.3e}; "
                  f"iters {torch.bincount(it2).tolist()} against ({one}) {torch.bincount(out[one][1]).tolist()}; status {torch.bincount(st2, minlength=16).tolist()}")
        print(f"{'variant':100s} {'us':>12s} {'range':>10s}   rounds (us)")
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in t:
            print(f"{K[k]:100s} {med[k]:12.1f} {max(t[k]) - min(t[k]):10.1f}   {' '.join(f'{v:11.1f}' for v in t[k])}")
        print(f"# (p1) / (a) = {med['p1'] / med['a']:.3f} ((p1) - (a) = {med['p1'] - med['a']:.1f} us); (g1) / (g) = {med['g1'] / med['g']:.3f} ((g1) - (g) = "
              f"{med['g1'] - med['g']:.1f} us); (tp) / (p1) = {med['tp'] / med['p1']:.3f} ((tp) - (p1) = {med['tp'] - med['p1']:.1f} us); (tg) / (g1) = "
              f"{med['tg'] / med['g1']:.3f} ((tg) - (g1) = {med['tg'] - med['g1']:.1f} us); (tp) = {med['tp'] * 1e3 / B:.1f} ns per frame, "
              f"{med['tp'] * 1e3 / B / iters:.1f} ns per frame and trial step; (s) = {med['s']:.1f} us")


if __name__ == "__main__":
    main()

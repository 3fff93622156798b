#!/usr/bin/env python3
"""GPU box: time of the fused posture solve against a second posed robot (dexr_sphere_resolve_cross_dev: self-collision, the
two-robot term, fingertip targets and the accept / reject iteration inside one kernel) next to what a user had before it.
Read-only use of the library.

Workload: tools/cross_probe.py's two hands (the Shadow hand vector configs, right = robot A, left = robot B, the optimisers'
variables as columns, float32, q uniform inside the limits, the 48-sphere set of tools/collision_probe.py on each; the left hand with
a seeded rotation per frame, the centroid of its spheres within 4 cm of the right hand's) with tools/resolve_probe.py's solve on A
(collision.default_pairs, margin 0.010, position targets on the five fingertips, posture weight 1e-4, damping 1e-4, max_step 0.2,
the joint limits, tol = 0); cross_margin = margin, w_x = 1, weights of 1.
  (x)   resolve_cross_dev: B at its own posture per frame, one launch
  (s)   resolve_dev on the same frames: no other robot at all
  (x1)  resolve_cross_dev with B held at ONE posture on all frames (the first row of q_b)
  (p)   resolve_scene_dev, one body: that posture's 48 centres as sphere primitives of an ObstacleSet, posed by B's pose -- the problem
        of (x1) through the one-body scene solve
  (t)   the loop (x) replaces, in torch: per trial cross_penalty + self_collision_penalty (E and gradients, one launch each),
        link_poses and link_jacobians of the tips, a damped step from torch.linalg.solve on J^T J + u I + lam I (no collision
        curvature), the same accept / reject rule; as many trials as the MEDIAN iters (x) took
(x) and (s), (x1) and (p) minimise different energies or the same through other code: the iters and energies are printed beside the
times.  HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same
box; the MEDIAN over `--rounds` rounds is reported, the rounds and their range beside it.

    python tools/resolve_cross_probe.py [--reps 5] [--rounds 5] [--iters 8,16] [--batch 65536]
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
from dex_retargeting_amd import jacobians as jac  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402

from collision_probe import MARGIN, timed  # noqa: E402
from cross_probe import REL_A, REL_B, Hand  # noqa: E402
from obstacle_probe import rotations  # noqa: E402
from resolve_probe import DAMPING, MAX_STEP, TIPS, U  # noqa: E402


def torch_loop(torch, A, Bh, q0, tp, lim, pos_b, rot_b, iters):
    """the loop the kernel replaces -> (q, E)."""
    n = q0.shape[1]
    eye = torch.eye(n, device="cuda")
    lo, hi = lim[:, 0], lim[:, 1]

    def energy(x):
        Ex, gx, _ = collision.cross_penalty(A.opt, x, A.sset, Bh.opt, Bh.q, Bh.sset, MARGIN, None, None, pos_b, rot_b)
        Ec, gc = collision.self_collision_penalty(A.opt, x, A.sset, MARGIN)
        e = tp - ag.link_poses(A.opt, x, TIPS, None, rotations=False)[0]
        return (e * e).sum((1, 2)) + U * ((x - q0) ** 2).sum(1) + Ec + Ex, e, gc + gx

    x = q0.clone()
    lam = torch.full((x.shape[0],), DAMPING, device="cuda")
    E, e, gc = energy(x)
    for _ in range(iters):
        J = jac.link_jacobians(A.opt, x, TIPS, angular=False)[0].reshape(x.shape[0], -1, n)
        g = torch.einsum("brc,br->bc", J, e.reshape(x.shape[0], -1)) + U * (q0 - x) - 0.5 * gc
        H = J.transpose(1, 2) @ J + U * eye
        dx = torch.linalg.solve(H + lam[:, None, None] * eye, g[..., None])[..., 0]
        m = dx.abs().amax(1, keepdim=True)
        dx = dx * torch.where(m > MAX_STEP, MAX_STEP / m, torch.ones_like(m))
        xt = torch.minimum(torch.maximum(x + dx, lo), hi)
        Et, et, gt = energy(xt)
        acc = Et <= E
        x = torch.where(acc[:, None], xt, x)
        E = torch.where(acc, Et, E)
        e = torch.where(acc[:, None, None], et, e)
        gc = torch.where(acc[:, None], gt, gc)
        lam = torch.where(acc, (lam / _lib.RESOLVE_LAM_DOWN).clamp_min(DAMPING), lam * _lib.RESOLVE_LAM_UP)
    return x, E


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
        sys.exit("resolve_cross_probe: no GPU (a timing needs one)")
    if args.rounds < 3:
        sys.exit("resolve_cross_probe: at least 3 rounds")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    B = args.batch
    A, Bh = Hand(torch, REL_A, B, 2), Hand(torch, REL_B, B, 3)
    n = A.n
    from oracle import cases

    prob = cases.problem_from_config(REL_A)
    lim = torch.tensor(prob.robot.joint_limits[prob.idx_pin2target].astype(np.float32), device="cuda")
    rng = np.random.default_rng(4)
    rot_np = rotations(rng, B)
    pos_np = A.home + rng.uniform(-0.04, 0.04, (B, 3)) - np.einsum("bij,j->bi", rot_np, Bh.home)
    rot_b = torch.tensor(rot_np.astype(np.float32), device="cuda")
    pos_b = torch.tensor(pos_np.astype(np.float32), device="cuda")
    tp = ag.link_poses(A.opt, A.q, TIPS, None, rotations=False)[0].contiguous()
    pairs = collision.default_pairs(A.opt.robot, A.sset)
    one_b = Bh.q[:1].expand(B, -1).contiguous()  # B held at ONE posture on all frames
    cb = collision.sphere_distances(Bh.opt, Bh.q[:1], Bh.sset, centers=True)[1][0].double().cpu().numpy()
    oset = collision.ObstacleSet.spheres(cb, Bh.sset.radii)
    print(f"# resolve_cross_probe: {torch.cuda.get_device_name(0)}, float32, library {_lib.LIB_PATH}; {REL_A} against {REL_B}: B = {B}, n_in = {n}, "
          f"{A.model.n_sphere} x {Bh.model.n_sphere} spheres, {len(pairs)} default pairs of A, {len(TIPS)} tip targets, a pose of B per frame; HIP events around "
          f"{args.reps} back-to-back runs after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    kw = dict(link_names=TIPS, target_pos=tp, max_step=MAX_STEP, limits=lim)
    for iters in (int(v) for v in args.iters.split(",")):
        out = {}

        def x():
            out["x"] = collision.resolve_cross_collisions(A.opt, A.q, A.sset, Bh.opt, Bh.q, Bh.sset, MARGIN, None, pos_b, rot_b, damping=DAMPING,
                                                          max_iters=iters, posture_weight=U, **kw)

        def x1():
            out["x1"] = collision.resolve_cross_collisions(A.opt, A.q, A.sset, Bh.opt, one_b, Bh.sset, MARGIN, None, pos_b, rot_b, damping=DAMPING,
                                                           max_iters=iters, posture_weight=U, **kw)

        def p():
            out["p"] = collision.resolve_scene_collisions(A.opt, A.q, A.sset, [collision.SceneBody(oset, pos_b, rot_b)], MARGIN, DAMPING, iters, U, **kw)

        def s():
            out["s"] = collision.resolve_self_collision(A.opt, A.q, A.sset, MARGIN, DAMPING, iters, U, **kw)

        for fn in (x, x1, p, s):  # once, for the trial counts the torch loop is given
            fn()
        torch.cuda.synchronize()
        med_iters = int(out["x"][1].median())

        def t():
            out["t"] = torch_loop(torch, A, Bh, A.q, tp, lim, pos_b, rot_b, med_iters)

        K = {"x": f"(x) resolve_cross_dev, B at a posture per frame: {iters} trial steps, one launch",
             "s": f"(s) resolve_dev (no other robot): {iters} trial steps, one launch",
             "x1": f"(x1) resolve_cross_dev, B at one posture: {iters} trial steps, one launch",
             "p": f"(p) resolve_scene_dev, one body of 48 sphere primitives: {iters} trial steps, one launch",
             "t": f"(t) torch loop: cross_penalty + self penalty + link_jacobians + solve, {med_iters} trials (the median iters of (x))"}
        runs = {"x": x, "s": s, "x1": x1, "p": p, "t": t}
        tm = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                tm[k].append(timed(torch, fn, args.reps if k != "t" else 1, args.warmup))
        torch.cuda.synchronize()
        ex = out["x"][2]
        print(f"\n# {iters} trial steps: (x) frames with a cross contact at the answer {float((ex[:, 3] > 0).float().mean()):.3f}; iters {torch.bincount(out['x'][1]).tolist()}; "
              f"status {torch.bincount(out['x'][3], minlength=16).tolist()}; median E_x {float(ex[:, 3].median()):.3e}; (s) iters {torch.bincount(out['s'][1]).tolist()}")
        print(f"# (x1) against (p): max |x| difference {float((out['x1'][0] - out['p'][0]).abs().max()):.3e}, median {float((out['x1'][0] - out['p'][0]).abs().amax(1).median()):.3e}; "
              f"iters equal on {float((out['x1'][1] == out['p'][1]).float().mean()):.4f} of the frames; median E {float(out['x1'][2].sum(1).median()):.4e} against "
              f"{float(out['p'][2].sum(1).median()):.4e}")
        print(f"# (t): median E {float(out['t'][1].median()):.4e} after {med_iters} trials against {float(ex.sum(1).median()):.4e} of (x)")
        print(f"{'variant':110s} {'us':>12s} {'range':>10s}   rounds (us)")
        med = {k: statistics.median(v) for k, v in tm.items()}
        for k in tm:
            print(f"{K[k]:110s} {med[k]:12.1f} {max(tm[k]) - min(tm[k]):10.1f}   {' '.join(f'{v:11.1f}' for v in tm[k])}")
        print(f"# (x) / (s) = {med['x'] / med['s']:.3f}; (x1) / (p) = {med['x1'] / med['p']:.3f}; (t) / (x) = {med['t'] / med['x']:.2f}; (x) = "
              f"{med['x'] * 1e3 / B:.1f} ns per frame, {med['x'] * 1e3 / B / iters:.1f} ns per frame and trial step")


if __name__ == "__main__":
    main()

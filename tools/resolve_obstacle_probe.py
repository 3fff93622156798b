#!/usr/bin/env python3
"""GPU box: time of the fused posture solve against obstacles (dexr_sphere_resolve_obstacles_dev: self-collision, obstacle
contacts, fingertip targets and the accept / reject iteration inside one kernel) next to
  (s) dexr_sphere_resolve_dev on the same frames: the difference is what the obstacle term costs, and
  (b) the same iteration written in torch from the calls the library had before it.
Read-only use of the library.

Workload: tools/resolve_probe.py's (Shadow hand vector config, B = 65 536, float32, q uniform inside the limits, the 48-sphere set
of tools/collision_probe.py with collision.default_pairs, margin 0.010, position targets on the five fingertips, posture weight
1e-4, damping 1e-4, max_step 0.2, the joint limits, tol = 0) with the 16 primitives and the pose per frame of
tools/obstacle_probe.py (a held object within 3 cm of the hand's centroid), obstacle margin 0.010, weights of 1; 8 and 16 trial
steps.
  (a) one resolve_obstacles_dev call
  (s) one resolve_dev call
  (b) torch, per trial step: collision.self_collision_penalty and collision.obstacle_penalty (energies and gradients),
      autograd.link_poses + jacobians.link_jacobians of the tips, the pair rows and the contact rows from jacobians.link_jacobians
      of every sphere link (the contact normals by torch.autograd.grad through the signed distances of tools/obstacle_probe.py,
      one primitive at a time), torch.linalg.solve, the step limit, the clamp and the accept / reject rule with torch.where -- in
      chunks of `--chunk` frames; no freeze rule and no caps
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box; the
MEDIAN over `--rounds` rounds is reported, the rounds beside it.

    python tools/resolve_obstacle_probe.py [--reps 5] [--rounds 5] [--iters 8,16] [--batch 65536] [--no-torch]
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
from oracle import cases  # noqa: E402

from collision_probe import MARGIN, sphere_set, timed  # noqa: E402
from obstacle_probe import obstacle_set, rotations, torch_sdf  # noqa: E402
from resolve_probe import DAMPING, MAX_STEP, N_SPHERE, REL, TIPS, U  # noqa: E402


def torch_route(torch, opt, sset, oset, pairs, q0, tp, pos, rot, lim, iters, chunk):
    """the iteration of include/dexr_resolve_obstacles.h from torch, chunk by chunk -> (q, E)."""
    links = list(sset.table_links)
    rows = torch.tensor(sset.sphere_rows.astype(np.int64), device="cuda")
    cen = torch.tensor(sset.centers.astype(np.float32), device="cuda")
    rad = torch.tensor(sset.radii.astype(np.float32), device="cuda")
    pi, pj = (torch.tensor(pairs[:, k].astype(np.int64), device="cuda") for k in (0, 1))
    rsum = torch.tensor((sset.radii[pairs[:, 0]] + sset.radii[pairs[:, 1]]).astype(np.float32), device="cuda")
    n, M = q0.shape[1], oset.n_prim
    eye = torch.eye(n, device="cuda")
    lo, hi = lim[:, 0], lim[:, 1]

    def energy(x, x0, t, p, r):
        Ec, gc = collision.self_collision_penalty(opt, x, sset, MARGIN)
        Eo, go = collision.obstacle_penalty(opt, x, sset, oset, MARGIN, p, r)
        e = t - ag.link_poses(opt, x, TIPS, None, rotations=False)[0]
        return (e * e).sum((1, 2)) + U * ((x - x0) ** 2).sum(1) + Ec + Eo, e, gc + go

    xs, Es = [], []
    for s in range(0, q0.shape[0], chunk):
        x0, t = q0[s:s + chunk].contiguous(), tp[s:s + chunk].contiguous()
        p, r = pos[s:s + chunk].contiguous(), rot[s:s + chunk].contiguous()
        x = x0.clone()
        lam = torch.full((x.shape[0],), DAMPING, device="cuda")
        E, e, gc = energy(x, x0, t, p, r)
        for _ in range(iters):
            jl = jac.link_jacobians(opt, x, TIPS, angular=False)[0]  # (b, 5, 3, n)
            J = jl.reshape(x.shape[0], -1, n)
            g = torch.einsum("brc,br->bc", J, e.reshape(x.shape[0], -1)) + U * (x0 - x) - 0.5 * gc
            H = J.transpose(1, 2) @ J + U * eye
            # point Jacobians of the sphere centres; the rows grad d_p of the active pairs
            sl, sa = jac.link_jacobians(opt, x, links)
            lp, lr = ag.link_poses(opt, x, links, None, rotations=True)
            arm = torch.einsum("bsij,sj->bsi", lr[:, rows], cen)
            ctr = lp[:, rows] + arm
            jpt = sl[:, rows] + torch.cross(sa[:, rows], arm[..., None].expand(-1, -1, -1, n), dim=2)
            D = ctr[:, pi] - ctr[:, pj]
            sp = D.norm(dim=-1)
            act = ((MARGIN - (sp - rsum)) > 0).float()
            dd = torch.einsum("bpr,bprc->bpc", D / sp[..., None], jpt[:, pi] - jpt[:, pj])
            H = H + dd.transpose(1, 2) @ (dd * act[..., None])
            # ... and the rows grad d_sm of the active contacts: world normals through the signed distances, a primitive at a time
            c = ctr.detach().requires_grad_(True)
            sdf = torch_sdf(torch, oset, torch.einsum("bji,bsj->bsi", r, c - p[:, None]))
            for m in range(M):
                nm = torch.autograd.grad(sdf[..., m].sum(), c, retain_graph=m + 1 < M)[0]  # (b, S, 3)
                am = ((MARGIN - (sdf[..., m].detach() - rad)) > 0).float()
                dm = torch.einsum("bsr,bsrc->bsc", nm, jpt)
                H = H + dm.transpose(1, 2) @ (dm * am[..., None])
            dx = torch.linalg.solve(H + lam[:, None, None] * eye, g[..., None])[..., 0]
            mx = dx.abs().amax(1, keepdim=True)
            dx = dx * torch.where(mx > MAX_STEP, MAX_STEP / mx, torch.ones_like(mx))
            xt = torch.minimum(torch.maximum(x + dx, lo), hi)
            Et, et, gt = energy(xt, x0, t, p, r)
            acc = Et <= E
            x = torch.where(acc[:, None], xt, x)
            E = torch.where(acc, Et, E)
            e = torch.where(acc[:, None, None], et, e)
            gc = torch.where(acc[:, None], gt, gc)
            lam = torch.where(acc, (lam / _lib.RESOLVE_LAM_DOWN).clamp_min(DAMPING), lam * _lib.RESOLVE_LAM_UP)
        xs.append(x)
        Es.append(E)
    return torch.cat(xs), torch.cat(Es)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", default="8,16")
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the two fused launches alone")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("resolve_obstacle_probe: no GPU (a timing needs one)")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    sset = sphere_set(opt, N_SPHERE)
    oset = obstacle_set()
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
    print(f"# resolve_obstacle_probe: {torch.cuda.get_device_name(0)}, float32, library {_lib.LIB_PATH}; {REL}: B = {B}, n_in = {n}, {N_SPHERE} "
          f"spheres, {len(pairs)} default pairs, {oset.n_prim} primitives with a pose per frame, {len(TIPS)} tip targets; HIP events around "
          f"{args.reps} back-to-back runs after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    for iters in (int(v) for v in args.iters.split(",")):
        out = {}

        def a():
            out["a"] = collision.resolve_collisions(opt, q, sset, oset, MARGIN, None, pos, rot, 1.0, None, DAMPING, iters, U, link_names=TIPS,
                                                    target_pos=tp, max_step=MAX_STEP, limits=lim)

        def s():
            out["s"] = collision.resolve_self_collision(opt, q, sset, MARGIN, DAMPING, iters, U, link_names=TIPS, target_pos=tp, max_step=MAX_STEP, limits=lim)

        def b():
            out["b"] = torch_route(torch, opt, sset, oset, pairs, q, tp, pos, rot, lim, iters, args.chunk)

        KA, KS = f"(a) resolve_obstacles_dev: {iters} trial steps, one launch", f"(s) resolve_dev (no obstacles): {iters} trial steps, one launch"
        KB = f"(b) torch: {iters} trial steps from the two penalties, link_jacobians, linalg.solve"
        runs = {KA: a, KS: s} if args.no_torch else {KA: a, KS: s, KB: b}
        t = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t[k].append(timed(torch, fn, 1 if k == KB else args.reps, 0 if k == KB else args.warmup))
        torch.cuda.synchronize()
        x, it, en, st = out["a"]
        Eo0 = collision.obstacle_penalty(opt, q, sset, oset, MARGIN, pos, rot)[0]
        Ec0 = collision.self_collision_penalty(opt, q, sset, MARGIN)[0]
        print(f"\n# {iters} trial steps: obstacle energy (median, max) {float(Eo0.median()):.3e}, {float(Eo0.max()):.3e} -> {float(en[:, 3].median()):.3e}, "
              f"{float(en[:, 3].max()):.3e}; frames in contact {float((Eo0 > 0).float().mean()):.3f} -> {float((en[:, 3] > 0).float().mean()):.3f}; collision "
              f"energy median {float(Ec0.median()):.3e} -> {float(en[:, 2].median()):.3e}; pose energy max {float(en[:, 0].max()):.3e}; iters "
              f"{torch.bincount(it).tolist()}; status {torch.bincount(st, minlength=16).tolist()}")
        if not args.no_torch:
            xb, Eb = out["b"]
            print(f"# torch route: max |x(a) - x(b)| = {float((x - xb).abs().max()):.3e}, median {float((x - xb).abs().amax(1).median()):.3e}; total E "
                  f"median (a) {float(en.sum(1).median()):.4e}, (b) {float(Eb.median()):.4e}")
        print(f"{'variant':88s} {'us':>12s}   rounds (us)")
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in runs:
            print(f"{k:88s} {med[k]:12.1f}   {' '.join(f'{v:11.1f}' for v in t[k])}")
        print(f"# (a) = {med[KA] * 1e3 / B:.1f} ns per frame, {med[KA] * 1e3 / B / iters:.1f} ns per frame and trial step; (a) / (s) = {med[KA] / med[KS]:.2f}, "
              f"(a) - (s) = {med[KA] - med[KS]:.1f} us" + ("" if args.no_torch else f"; (b) / (a) = {med[KB] / med[KA]:.1f}"))


if __name__ == "__main__":
    main()

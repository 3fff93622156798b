#!/usr/bin/env python3
"""GPU box: time of the fused posture solve against a signed-distance grid (dexr_sphere_resolve_grid_dev: self-collision, one cell
lookup per sphere, fingertip targets and the accept / reject iteration inside one kernel) next to
  (a) dexr_sphere_resolve_obstacles_dev on the primitives the grid was sampled from -- unchanged code, the cost yardstick: it
      minimises ANOTHER energy, a sum over the 16 primitives where the grid holds their union,
  (s) dexr_sphere_resolve_dev on the same frames: the difference is what the grid term costs, and
  (b) the same iteration written in torch from the calls the library had before it (once, at 8 steps).
Read-only use of the library.

Workload: tools/resolve_obstacle_probe.py's (Shadow hand vector config, B = 65 536, float32, q uniform inside the limits, the
48-sphere set with collision.default_pairs, margin 0.010, position targets on the five fingertips, posture weight 1e-4, damping
1e-4, max_step 0.2, the joint limits, tol = 0, the 16 primitives and the pose per frame of tools/obstacle_probe.py), the union of
the primitives sampled by SdfGrid.from_obstacles as tools/grid_probe.py does: a box of 32 cm on 64^3 (1 MB) and on 256^3 (64 MB);
8 and 16 trial steps.
  (g64), (g256)  one resolve_grid_dev call on either grid
  (a)            one resolve_obstacles_dev call
  (s)            one resolve_dev call
  (b)            torch, per trial step: collision.self_collision_penalty and collision.grid_penalty (energies and gradients),
                 autograd.link_poses + jacobians.link_jacobians of the tips, the pair rows and the contact rows from
                 jacobians.link_jacobians of every sphere link (the contact normals by torch.autograd.grad through grid_sample, the
                 field of tools/grid_probe.py), torch.linalg.solve, the step limit, the clamp and the accept / reject rule with
                 torch.where -- in chunks of `--chunk` frames; no freeze rule
HIP events around `--reps` back-to-back runs after `--warmup`; the variants alternate inside a round so all see the same box; the
MEDIAN over `--rounds` rounds is reported, the rounds and their range beside it.

    python tools/resolve_grid_probe.py [--reps 5] [--rounds 5] [--iters 8,16] [--batch 65536] [--no-torch]
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
from grid_probe import sampled, torch_grid_sdf  # noqa: E402
from obstacle_probe import obstacle_set, rotations  # noqa: E402
from resolve_probe import DAMPING, MAX_STEP, N_SPHERE, REL, TIPS, U  # noqa: E402


def torch_route(torch, opt, sset, grid, pairs, q0, tp, pos, rot, lim, iters, chunk):
    """the iteration of include/dexr_resolve_grid.h from torch, chunk by chunk -> (q, E)."""
    links = list(sset.table_links)
    rows = torch.tensor(sset.sphere_rows.astype(np.int64), device="cuda")
    cen = torch.tensor(sset.centers.astype(np.float32), device="cuda")
    rad = torch.tensor(sset.radii.astype(np.float32), device="cuda")
    pi, pj = (torch.tensor(pairs[:, k].astype(np.int64), device="cuda") for k in (0, 1))
    rsum = torch.tensor((sset.radii[pairs[:, 0]] + sset.radii[pairs[:, 1]]).astype(np.float32), device="cuda")
    V = torch.tensor(grid.values, device="cuda")[None, None]
    glo = torch.tensor(grid.origin.astype(np.float32), device="cuda")
    ghi = torch.tensor((grid.origin + grid.spacing * (np.array(grid.shape) - 1)).astype(np.float32), device="cuda")
    n = q0.shape[1]
    eye = torch.eye(n, device="cuda")
    lo, hi = lim[:, 0], lim[:, 1]

    def energy(x, x0, t, p, r):
        Ec, gc = collision.self_collision_penalty(opt, x, sset, MARGIN)
        Eo, go = collision.grid_penalty(opt, x, sset, grid, MARGIN, p, r)
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
            # ... and the rows grad d_s of the active spheres: world normals by one backward pass through grid_sample
            c = ctr.detach().requires_grad_(True)
            sdf = torch_grid_sdf(torch, V, glo, ghi, torch.einsum("bji,bsj->bsi", r, c - p[:, None]))
            nm = torch.autograd.grad(sdf.sum(), c)[0]  # (b, S, 3)
            am = ((MARGIN - (sdf.detach() - rad)) > 0).float()
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
    ap.add_argument("--no-torch", action="store_true", help="time the fused launches alone")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("resolve_grid_probe: no GPU (a timing needs one)")
    if args.rounds < 3:
        sys.exit("resolve_grid_probe: at least 3 rounds")
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, REL)).build().optimizer
    prob = cases.problem_from_config(REL)
    sset = sphere_set(opt, N_SPHERE)
    oset = obstacle_set()
    grids = {"g64": sampled(oset, 64), "g256": sampled(oset, 256)}
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
    print(f"# resolve_grid_probe: {torch.cuda.get_device_name(0)}, float32, library {_lib.LIB_PATH}; {REL}: B = {B}, n_in = {n}, {N_SPHERE} "
          f"spheres, {len(pairs)} default pairs, {oset.n_prim} primitives sampled on 64^3 and 256^3 with a pose per frame, {len(TIPS)} tip targets; HIP "
          f"events around {args.reps} back-to-back runs after {args.warmup} warm-up runs; median of {args.rounds} alternating rounds")
    for iters in (int(v) for v in args.iters.split(",")):
        out = {}

        def g(which):
            def run():
                out[which] = collision.resolve_grid_collisions(opt, q, sset, grids[which], MARGIN, None, pos, rot, 1.0, DAMPING, iters, U, link_names=TIPS,
                                                               target_pos=tp, max_step=MAX_STEP, limits=lim)
            return run

        def a():
            out["a"] = collision.resolve_collisions(opt, q, sset, oset, MARGIN, None, pos, rot, 1.0, None, DAMPING, iters, U, link_names=TIPS,
                                                    target_pos=tp, max_step=MAX_STEP, limits=lim)

        def s():
            out["s"] = collision.resolve_self_collision(opt, q, sset, MARGIN, DAMPING, iters, U, link_names=TIPS, target_pos=tp, max_step=MAX_STEP, limits=lim)

        def b():
            out["b"] = torch_route(torch, opt, sset, grids["g64"], pairs, q, tp, pos, rot, lim, iters, args.chunk)

        KG, KH = f"(g64) resolve_grid_dev, 64^3: {iters} trial steps, one launch", f"(g256) resolve_grid_dev, 256^3: {iters} trial steps, one launch"
        KA, KS = f"(a) resolve_obstacles_dev, the 16 primitives: {iters} trial steps, one launch", f"(s) resolve_dev (no obstacles): {iters} trial steps, one launch"
        KB = f"(b) torch: {iters} trial steps from the two penalties, link_jacobians, grid_sample, linalg.solve (once)"
        runs = {KG: g("g64"), KH: g("g256"), KA: a, KS: s}
        t = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                t[k].append(timed(torch, fn, args.reps, args.warmup))
        if not args.no_torch and iters == 8:
            t[KB] = [timed(torch, b, 1, 0)]
        torch.cuda.synchronize()
        x, it, en, st = out["g64"]
        Eo0 = collision.grid_penalty(opt, q, sset, grids["g64"], MARGIN, pos, rot)[0]
        Ec0 = collision.self_collision_penalty(opt, q, sset, MARGIN)[0]
        d0 = collision.grid_distances(opt, q, sset, grids["g64"], pos, rot)
        d1 = collision.grid_distances(opt, x, sset, grids["g64"], pos, rot)
        c0, c1 = (d0 < MARGIN).sum(1).float(), (d1 < MARGIN).sum(1).float()
        print(f"\n# {iters} trial steps, 64^3: grid energy (median, max) {float(Eo0.median()):.3e}, {float(Eo0.max()):.3e} -> {float(en[:, 3].median()):.3e}, "
              f"{float(en[:, 3].max()):.3e}; frames in contact {float((Eo0 > 0).float().mean()):.3f} -> {float((en[:, 3] > 0).float().mean()):.3f}; contacts per "
              f"frame (mean, max) {float(c0.mean()):.2f}, {int(c0.max())} -> {float(c1.mean()):.2f}, {int(c1.max())}; collision energy median "
              f"{float(Ec0.median()):.3e} -> {float(en[:, 2].median()):.3e}; pose energy max {float(en[:, 0].max()):.3e}; iters {torch.bincount(it).tolist()}; "
              f"status {torch.bincount(st, minlength=16).tolist()}")
        xh, _, eh, _ = out["g256"]
        xa, ita, ea, _ = out["a"]
        print(f"# 256^3 against 64^3: max |x| difference {float((x - xh).abs().max()):.3e}, median {float((x - xh).abs().amax(1).median()):.3e} (another sampling "
              f"of the same shape); (a) ends with obstacle energy median {float(ea[:, 3].median()):.3e}, iters {torch.bincount(ita).tolist()}")
        if KB in t:
            xb, Eb = out["b"]
            print(f"# torch route: max |x(g64) - x(b)| = {float((x - xb).abs().max()):.3e}, median {float((x - xb).abs().amax(1).median()):.3e}; total E "
                  f"median (g64) {float(en.sum(1).median()):.4e}, (b) {float(Eb.median()):.4e}")
        print(f"{'variant':100s} {'us':>12s} {'range':>10s}   rounds (us)")
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in t:
            print(f"{k:100s} {med[k]:12.1f} {max(t[k]) - min(t[k]):10.1f}   {' '.join(f'{v:11.1f}' for v in t[k])}")
        spread = max(max(t[KG]) - min(t[KG]), max(t[KA]) - min(t[KA]))
        print(f"# (g64) = {med[KG] * 1e3 / B:.1f} ns per frame, {med[KG] * 1e3 / B / iters:.1f} ns per frame and trial step; (g64) / (s) = "
              f"{med[KG] / med[KS]:.2f}, (g64) - (s) = {med[KG] - med[KS]:.1f} us; (g64) / (a) = {med[KG] / med[KA]:.2f}; (g256) / (g64) = "
              f"{med[KH] / med[KG]:.2f}" + (f"; (b) / (g64) = {med[KB] / med[KG]:.1f}" if KB in t else ""))
        if med[KG] > med[KA] + spread:
            print(f"# (g64) EXCEEDS (a) by {med[KG] - med[KA]:.1f} us, more than the round-to-round range of the two ({spread:.1f} us)")
        elif not med[KS] <= med[KG]:
            print("# (g64) is below (s)")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""GPU box: times of the link-pose kernels (dexr_link_poses_dev / dexr_link_poses_vjp_dev) next to the solve of the same
config, one process, one session.  HIP events around `--reps` back-to-back launches after `--warmup`, `--rounds` rounds in
which the solve and the pose launches alternate so both see the same box; the median round is reported.

    python tools/link_poses_probe.py [--reps 200] [--rounds 5] > profiles/r09_link_poses.txt

Columns: us per launch, ms per 65 536 frames (the launch time scaled by 65 536 / B), algorithmic bytes per frame
(forward: 4 n_in in, 12 L (+ 36 L) out; VJP: 4 n_in + 12 L (+ 36 L) in, 4 n_in out) and the fraction of 8 TB/s they amount to."""
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

PEAK = 8e12


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    print(f"# link_poses_probe: {torch.cuda.get_device_name(0)}, reps {args.reps}, warm-up {args.warmup}, median of {args.rounds} "
          "alternating rounds; HIP events")
    print(f"{'config':34s} {'links':>14s} {'B':>6s} {'kernel':>12s} {'us/launch':>10s} {'ms/65536':>9s} {'B/frame':>8s} {'of 8 TB/s':>9s}")
    for rel, tips in (("teleop/shadow_hand_right_dexpilot.yml", ["thtip", "fftip", "mftip", "rftip", "lftip"]),
                      ("teleop/allegro_hand_right.yml", ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_11.0_tip"])):
        seq = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build()
        opt = seq.optimizer
        prob = cases.problem_from_config(rel)
        sets = [("tips", tips)]
        if "shadow" in rel:
            sets.append(("all links", [f.name for f in opt.robot.kin.frames][:64]))
        for B in (1, 2048, 65536):
            d = cases.human_set(prob, B)
            ref = torch.tensor(d["ref"], device="cuda")
            last = torch.tensor(d["last"], device="cuda")
            q = torch.empty_like(last)
            st = torch.zeros(B, dtype=torch.int32, device="cuda") if prob.kind == "dexpilot" else None
            stat = torch.zeros(B, dtype=torch.int32, device="cuda")
            sp = torch.cuda.current_stream().cuda_stream
            dm = opt.device_model()
            dm.reserve(B)

            def solve():
                if st is not None:
                    st.zero_()
                dm.retarget_dev(B, ref.data_ptr(), 0, last.data_ptr(), 0 if st is None else st.data_ptr(), q.data_ptr(),
                                stat.data_ptr(), opts=opt._options(), stream=sp)

            solve()
            torch.cuda.synchronize()
            n_in = opt.opt_dof
            for label, links in sets:
                L = len(links)
                model = opt.pose_model(links)
                pos = torch.empty((B, L, 3), device="cuda")
                rot = torch.empty((B, L, 3, 3), device="cuda")
                gp, gr, gx = torch.randn_like(pos), torch.randn_like(rot), torch.empty_like(q)
                runs = {
                    "solve": (solve, None),
                    "fwd pos": (lambda: model.poses_dev(B, q.data_ptr(), 0, pos.data_ptr(), 0, stream=sp), 4 * n_in + 12 * L),
                    "fwd pos+rot": (lambda: model.poses_dev(B, q.data_ptr(), 0, pos.data_ptr(), rot.data_ptr(), stream=sp), 4 * n_in + 48 * L),
                    "vjp pos": (lambda: model.vjp_dev(B, q.data_ptr(), 0, gp.data_ptr(), 0, gx.data_ptr(), stream=sp), 8 * n_in + 12 * L),
                    "vjp pos+rot": (lambda: model.vjp_dev(B, q.data_ptr(), 0, gp.data_ptr(), gr.data_ptr(), gx.data_ptr(), stream=sp),
                                    8 * n_in + 48 * L),
                }
                t = {k: [] for k in runs}
                for _ in range(args.rounds):
                    for k, (fn, _) in runs.items():  # alternate: every kernel once per round
                        t[k].append(timed(torch, fn, args.reps, args.warmup))
                for k, (_, nbytes) in runs.items():
                    us = statistics.median(t[k])
                    frac = "" if nbytes is None else f"{nbytes * B / (us * 1e-6) / PEAK:9.4f}"
                    print(f"{rel:34s} {label + ' L=' + str(L):>14s} {B:6d} {k:>12s} {us:10.2f} {us * 65536 / B / 1e3:9.3f} "
                          f"{'' if nbytes is None else nbytes:>8} {frac:>9s}", flush=True)
                us_pair = statistics.median(t["fwd pos"]) + statistics.median(t["vjp pos"])
                print(f"#   {rel} {label} B={B}: forward + VJP (positions) = {us_pair:.2f} us = "
                      f"{us_pair / statistics.median(t['solve']):.3f} x the solve of the same frames", flush=True)


if __name__ == "__main__":
    main()

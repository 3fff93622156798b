#!/usr/bin/env python3
"""GPU: float64 solves on the sixteen-lane kernel (dexr_tuning.kernel_f64 = WIDE) against the two paths beside it, per config.

For every shipped config whose handle fits the sixteen-lane kernel (or the ones named with --config): B tracking frames
(tests/test_gpu_all_configs protocol: frame b starts from the float32 answer for frame b - 1, DexPilot bits carried), then
three launches through dexr_retarget_kp_dev, each timed with HIP events after warm-up (median of --reps):
  f32       -- the float32 default;
  reg64     -- precision = 1 on an untouched handle (the register kernel, today's default for float64);
  wide64    -- precision = 1 with kernel_f64 = WIDE.
Reports per-frame iteration means / maxima and max |q_wide64 - q_f32| (both float32 rows).  Writes the table to --out
(default build/reports/f64_wide_probe.txt; profiles/r07_f64_wide.txt is its committed copy).

    python tools/f64_wide_probe.py [--batch 65536] [--reps 5] [--config teleop/shadow_hand_right_dexpilot.yml ...]
"""
import argparse
import ctypes
import glob
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dex_retargeting_amd import _lib  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402


def model_of(rel):
    return RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer.device_model()


def run(model, kp, last, st0, opts, reps, warmup):
    B, n = last.shape
    q = torch.empty_like(last)
    st = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    iters = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    times = []
    for r in range(warmup + reps):
        if st0 is not None:
            st.copy_(st0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model.retarget_dev(B, kp.data_ptr(), 0, last.data_ptr(), st.data_ptr() if st0 is not None else 0, q.data_ptr(),
                           status.data_ptr(), iters.data_ptr(), 0, opts, torch.cuda.current_stream().cuda_stream, keypoints=True)
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            times.append(e0.elapsed_time(e1))
    it = iters.cpu().numpy()
    return float(np.median(times)), q.cpu().numpy(), it, int((status == 2).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", action="append")
    ap.add_argument("--out", default=os.path.join(REPO, "build", "reports", "f64_wide_probe.txt"))
    a = ap.parse_args()
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    rels = a.config or sorted(os.path.relpath(p, cases.CONFIG_DIR) for p in glob.glob(os.path.join(cases.CONFIG_DIR, "*", "*.yml")))
    B = a.batch
    lines = [f"# float64 solves on the sixteen-lane kernel: {B} tracking frames per config, HIP events, median of {a.reps} after "
             f"{a.warmup} warm-up launches (tools/f64_wide_probe.py)",
             "# f32 = float32 default; reg64 = precision 1, untouched handle (register kernel); wide64 = precision 1, kernel_f64 = WIDE",
             "# iters: mean / max passes per frame; dq = max |q_wide64 - q_f32| (float32 rows); st2 = frames with status 2 (wide64)",
             f"{'config':44s} {'f32 ms':>8s} {'reg64 ms':>9s} {'wide64 ms':>9s} {'reg/wide':>8s} {'it f32':>11s} {'it reg64':>11s} "
             f"{'it wide64':>11s} {'dq':>9s} {'st2':>4s}"]
    print("\n".join(lines), flush=True)
    f64 = _lib.default_options(precision=1)
    for rel in rels:
        base = model_of(rel)
        n = ctypes.c_int32()
        if _lib.load().dexr_model_lane_plan(base._h, 0, ctypes.byref(n), None, None, None) != 0:
            continue
        wide = model_of(rel)
        t = wide.get_tuning()
        t.kernel_f64 = _lib.KERNEL_WIDE
        if _lib.load().dexr_model_set_tuning(wide._h, ctypes.byref(t)) != 0:
            line = f"{rel:44s} (kernel_f64 = WIDE refused: {_lib.load().dexr_last_error().decode()})"
            print(line, flush=True)
            lines.append(line)
            continue
        prob = cases.problem_from_config(rel)
        kpn = cases.human_keypoints(B + 1, seed=cases.SEED)
        mid = np.repeat(prob.joint_limits.mean(1)[None], B, 0).astype(np.float32)
        st = np.zeros(B, np.uint32) if prob.kind == "dexpilot" else None
        lastn = base.retarget(np.ascontiguousarray(kpn[:-1]), None, mid, state=st, keypoints=True)
        kp = torch.from_numpy(np.ascontiguousarray(kpn[1:], dtype=np.float32)).cuda()
        last = torch.from_numpy(lastn).cuda()
        st0 = None if st is None else torch.from_numpy(st.view(np.int32)).cuda()
        t32, q32, i32, _ = run(base, kp, last, st0, None, a.reps, a.warmup)
        tr, _, ir, _ = run(base, kp, last, st0, f64, a.reps, a.warmup)
        tw, qw, iw, s2 = run(wide, kp, last, st0, f64, a.reps, a.warmup)
        dq = float(np.abs(qw.astype(np.float64) - q32).max())
        line = (f"{rel:44s} {t32:8.3f} {tr:9.3f} {tw:9.3f} {tr / tw:8.1f} {i32.mean():6.2f}/{i32.max():4d} {ir.mean():6.2f}/{ir.max():4d} "
                f"{iw.mean():6.2f}/{iw.max():4d} {dq:9.1e} {s2:4d}")
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""GPU: milliseconds per 65 536 frames of the implicit-gradient VJP (dexr_retarget_vjp_dev, MODE_VJP of the general kernel)
next to the forward solve (dexr_retarget_dev, the product path) for Allegro vector, Shadow DexPilot, LEAP position and the
arm + Shadow hand model (37 variables, general kernel for both).  Median of `--reps` timed calls after `--warmup`, torch
events on the current stream.

    python tools/vjp_probe.py [--frames 65536] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402
from oracle import cases  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def probe(name, seq, prob, B, reps, warmup):
    opt = seq.optimizer
    d = cases.human_set(prob, B)
    dev = "cuda"
    ref = torch.tensor(d["ref"], device=dev)
    last = torch.tensor(d["last"], device=dev)
    fixed = torch.tensor(d["fixed"], device=dev) if d["fixed"].shape[1] else None
    st = torch.zeros(B, dtype=torch.int32, device=dev) if prob.kind == "dexpilot" else None
    st0 = None if st is None else st.clone()
    q = torch.empty_like(last)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    gq = torch.randn(last.shape, device=dev, generator=torch.Generator(dev).manual_seed(0))
    gref, glast = torch.zeros_like(ref), torch.zeros_like(last)
    vst = torch.zeros(B, dtype=torch.int32, device=dev)
    fm, vm = opt.device_model(), opt.vjp_model()
    stream = torch.cuda.current_stream().cuda_stream
    fp = 0 if fixed is None else fixed.data_ptr()

    def fwd():
        if st is not None:
            st.copy_(st0)
        fm.retarget_dev(B, ref.data_ptr(), fp, last.data_ptr(), 0 if st is None else st.data_ptr(), q.data_ptr(), status.data_ptr(),
                        opts=opt._options(), stream=stream)

    def vjp():
        vm.vjp_dev(B, ref.data_ptr(), fp, last.data_ptr(), 0 if st0 is None else st0.data_ptr(), q.data_ptr(), gq.data_ptr(),
                   gref.data_ptr(), glast.data_ptr(), vst.data_ptr(), stream=stream)

    t_fwd = timed(fwd, reps, warmup)
    t_vjp = timed(vjp, reps, warmup)
    torch.cuda.synchronize()
    ok = int((vst == 0).sum())
    return dict(model=name, frames=B, fwd_ms=round(t_fwd, 4), vjp_ms=round(t_vjp, 4), n_opt=opt.opt_dof,
                vjp_kernel=vm.kernel()[0], fwd_kernel=fm.kernel()[0], vjp_status0=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
    rows = []
    for rel in ["teleop/allegro_hand_right.yml", "teleop/shadow_hand_right_dexpilot.yml", "offline/leap_hand_right.yml"]:
        seq = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build()
        rows.append(probe(rel, seq, cases.problem_from_config(rel), a.frames, a.reps, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
    from test_gpu_generic import arm_hand

    seq, prob = arm_hand("position")
    rows.append(probe("arm_shadow_hand position (37 variables)", seq, prob, a.frames, a.reps, a.warmup))
    print(json.dumps(rows[-1]), flush=True)


if __name__ == "__main__":
    main()

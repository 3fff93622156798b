#!/usr/bin/env python3
"""GPU: answers of the float32 tip solve as the commit BEFORE the prologue rework gives them -> tip_prologue_parent.npz.

Run once, on a build of that parent commit:

    python tests/golden/gen_tip_prologue_golden.py

tests/test_gpu_tip_prologue.py compares later builds with the file bit for bit.  The two tip kernels (dexr_tip32_kernel and
dexr_kernel<4, float, SOLVE, CHAIN, EXT, TIP>) share TipTabT<float>::load, so comparing them with each other
(tests/test_gpu_tip32_kernel.py) cannot see a mistake in it; the parent's answers can.

The inputs are not stored: they are regenerated from the bench_data seeds (this module's `inputs`, which the test imports).
Stored per (robot, regime, B): qpos float32, status int8, iters int16 of retarget_dev.  On the parent the dedicated kernel
and the register-chain kernel agree bit for bit, and so do keypoint input and the ref_value rows formed from the same
keypoints on the host (one float32 subtraction either way); the generator asserts both, so one record serves the four
(kernel, input form) combinations.  It also checks the full-chip identity the test relies on -- rows of one 65 536-frame launch
= the same rows solved as sixteen 4 096-frame launches -- and records whether it held ("fullchip_identity")."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench_data  # noqa: E402
from dex_retargeting_amd import _lib  # noqa: E402
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR  # noqa: E402
from dex_retargeting_amd.retargeting_config import RetargetingConfig  # noqa: E402

OUT = os.path.join(HERE, "tip_prologue_parent.npz")
ROBOTS = {"allegro": "teleop/allegro_hand_right.yml", "leap": "teleop/leap_hand_right.yml"}
BATCHES = [1, 63, 65, 193]
REGIMES = ["tracking", "cold"]
FULL_B, FULL_PART = 65536, 4096
TILE = 64

_seq = {}


def build(robot):
    if robot not in _seq:
        RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
        _seq[robot] = RetargetingConfig.load_from_file(os.path.join(bench_data.CONFIG_DIR, ROBOTS[robot])).build()
    return _seq[robot]


def tracking(seq, B):
    """bench.py's frames, as tests/test_gpu_tip32_kernel.py stages them: keypoints of frame b + 1, warm start = the answer for frame b."""
    model = seq.optimizer.device_model()
    kp = bench_data.human_keypoints(B + 1)
    mid = np.repeat(seq.joint_limits.mean(1)[None], B, 0).astype(np.float32)
    last = model.retarget(np.ascontiguousarray(kp[:-1]), None, mid, keypoints=True)
    return np.ascontiguousarray(kp[1:]), last


def ref_rows(seq, kp):
    """ref_value rows of raw keypoints: kp[task] - kp[origin] in float32, the subtraction the kernel does on keypoint input."""
    origin, task = np.asarray(seq.optimizer.target_link_human_indices)
    return np.ascontiguousarray(kp[:, task] - kp[:, origin], dtype=np.float32)


def inputs(robot, regime, B):
    """{"kp": (input, last) or absent, "ref": (input, last)}: the case's inputs in each form it exists in."""
    seq = build(robot)
    if regime == "tracking":
        kp, last = tracking(seq, B)
        return {"kp": (kp, last), "ref": (ref_rows(seq, kp), last)}
    ref, start = bench_data.reachable_batch(seq, B, 0.5)  # cold starts: bound-active joints, where lo / hi matter
    return {"ref": (ref, start)}


def solve(model, inp, last, keypoints, kernel, pad=TILE):
    """retarget_dev on device copies; qpos is allocated `pad` rows longer than the batch and pre-filled with NaN.
    Returns qpos (B + pad, n), status (B,), iters (B,)."""
    import torch

    dev = torch.device("cuda:0")
    B = last.shape[0]
    t_in, t_last = torch.from_numpy(np.ascontiguousarray(inp)).to(dev), torch.from_numpy(np.ascontiguousarray(last)).to(dev)
    t_q = torch.full((B + pad, last.shape[1]), float("nan"), dtype=torch.float32, device=dev)
    t_status = torch.zeros(B, dtype=torch.int32, device=dev)
    t_iters = torch.zeros(B, dtype=torch.int32, device=dev)
    model.tune(kernel=kernel)
    try:
        model.retarget_dev(B, t_in.data_ptr(), 0, t_last.data_ptr(), 0, t_q.data_ptr(), status_ptr=t_status.data_ptr(),
                           iters_ptr=t_iters.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, keypoints=keypoints)
        torch.cuda.synchronize()
    finally:
        model.tune(kernel=_lib.KERNEL_AUTO)
    return t_q.cpu().numpy(), t_status.cpu().numpy(), t_iters.cpu().numpy()


def full_chip(robot="allegro"):
    """(whole, parts): qpos / status / iters of one FULL_B-frame tracking launch and of the same rows as FULL_B / FULL_PART launches."""
    import torch

    seq = build(robot)
    model = seq.optimizer.device_model()
    kp, last = tracking(seq, FULL_B)
    whole = solve(model, kp, last, True, _lib.KERNEL_AUTO, pad=0)
    dev = torch.device("cuda:0")
    t_kp, t_last = torch.from_numpy(kp).to(dev), torch.from_numpy(last).to(dev)
    t_q = torch.full(last.shape, float("nan"), dtype=torch.float32, device=dev)
    t_status = torch.zeros(FULL_B, dtype=torch.int32, device=dev)
    t_iters = torch.zeros(FULL_B, dtype=torch.int32, device=dev)
    for b0 in range(0, FULL_B, FULL_PART):
        model.retarget_dev(FULL_PART, t_kp[b0:].data_ptr(), 0, t_last[b0:].data_ptr(), 0, t_q[b0:].data_ptr(),
                           status_ptr=t_status[b0:].data_ptr(), iters_ptr=t_iters[b0:].data_ptr(),
                           stream=torch.cuda.current_stream().cuda_stream, keypoints=True)
    torch.cuda.synchronize()
    return whole, (t_q.cpu().numpy(), t_status.cpu().numpy(), t_iters.cpu().numpy())


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def main():
    out = {}
    for robot in ROBOTS:
        model = build(robot).optimizer.device_model()
        for regime in REGIMES:
            for B in BATCHES:
                got = []
                for form, (inp, last) in inputs(robot, regime, B).items():
                    for kernel in (_lib.KERNEL_AUTO, _lib.KERNEL_REGISTER_CHAIN):
                        got.append(solve(model, inp, last, form == "kp", kernel))
                assert all(same(got[0], g) for g in got[1:]), f"{robot} {regime} B={B}: kernels / input forms disagree on the parent"
                q, status, iters = got[0]
                assert np.isfinite(q[:B]).all() and np.isnan(q[B:]).all()
                key = f"{robot}/{regime}/{B}"
                out[key + "/qpos"] = q[:B]
                out[key + "/status"] = status.astype(np.int8)
                out[key + "/iters"] = iters.astype(np.int16)
                print(f"{key}: iters mean {iters.mean():.2f} max {iters.max()}  status max {status.max()}  checksum {float(q[:B].astype(np.float64).sum()):.6f}")
    whole, parts = full_chip()
    out["fullchip_identity"] = np.array(same(whole, parts))
    print("full-chip identity (one 65 536-frame launch = sixteen 4 096-frame launches) on this build:", bool(out["fullchip_identity"]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

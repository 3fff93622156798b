"""GPU: the dedicated float32 tip solve kernel (csrc/dexr_tip_solve.hpp, dexr_tip32_kernel) against the kernel it stands in for.

Plain tile launches of a tip model -- float32, no queue, no sequence, no fleet addressing, no objective values -- run
dexr_tip32_kernel; dexr_tuning.kernel = DEXR_KERNEL_REGISTER_CHAIN sends the same call through dexr_kernel<4, float, SOLVE, CHAIN, EXT, TIP>, the
code every other call of such a model keeps.  The new kernel does the arithmetic of the old one operation for operation, so
qpos, status and iters are compared with np.array_equal, on the headline inputs (tracking frames, warm start) and on the
reference's cold regime, where rejected steps, the damping jump, modified pivots and bound-active joints occur.

The calls go through the device-pointer entry point without an fval pointer: the host-array entry points always ask for the
objective values, which keeps them on dexr_kernel."""
import os

import numpy as np
import pytest

import bench_data
from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig

pytestmark = pytest.mark.gpu
RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))

CONFIGS = ["teleop/allegro_hand_right.yml", "teleop/leap_hand_right.yml"]
BATCHES = [1, 63, 64, 65, 4096, 65536]
ST_CONVERGED, ST_MAXITER = 0, 1

_cache = {}


def build(rel):
    if rel not in _cache:
        _cache[rel] = RetargetingConfig.load_from_file(os.path.join(bench_data.CONFIG_DIR, rel)).build()
    return _cache[rel]


def solve_dev(model, inp, last, keypoints, tip_kernel, opts=None, fval=False):
    """One retarget_dev call on device copies of (inp, last) with (tip_kernel = 1) or without (0) the dedicated kernel; (qpos, status, iters[, fval])."""
    import torch

    dev = torch.device("cuda:0")
    B = last.shape[0]
    t_in, t_last = torch.from_numpy(np.ascontiguousarray(inp)).to(dev), torch.from_numpy(np.ascontiguousarray(last)).to(dev)
    t_q = torch.full(last.shape, float("nan"), dtype=torch.float32, device=dev)
    t_status = torch.zeros(B, dtype=torch.int32, device=dev)
    t_iters = torch.zeros(B, dtype=torch.int32, device=dev)
    t_fval = torch.zeros(B, dtype=torch.float32, device=dev) if fval else None
    model.tune(kernel=_lib.KERNEL_AUTO if tip_kernel else _lib.KERNEL_REGISTER_CHAIN)
    try:
        model.retarget_dev(B, t_in.data_ptr(), 0, t_last.data_ptr(), 0, t_q.data_ptr(), status_ptr=t_status.data_ptr(),
                           iters_ptr=t_iters.data_ptr(), fval_ptr=t_fval.data_ptr() if fval else 0, opts=opts,
                           stream=torch.cuda.current_stream().cuda_stream, keypoints=keypoints)
        torch.cuda.synchronize()
    finally:
        model.tune(kernel=_lib.KERNEL_AUTO)
    out = (t_q.cpu().numpy(), t_status.cpu().numpy(), t_iters.cpu().numpy())
    return out + (t_fval.cpu().numpy(),) if fval else out


def tracking(seq, model, B, seed=bench_data.SEED):
    """The headline inputs as bench.py stages them: frame b + 1 of the fixture walk, warm start = the solver's answer for frame b."""
    kp = bench_data.human_keypoints(B + 1, seed=seed)
    mid = np.repeat(seq.joint_limits.mean(1)[None], B, 0).astype(np.float32)
    last = model.retarget(np.ascontiguousarray(kp[:-1]), None, mid, keypoints=True)
    return np.ascontiguousarray(kp[1:]), last


def on_bound(q, limits):
    """(B, n) bool: the joint sits on a face of the solver's box.  The box is the joint limits up to the clipping margin the
    tables carry, so its faces are read off the answers themselves: a clamped joint holds the face's value exactly, i.e. the
    column's extreme value, shared bit for bit by several frames (interior answers are continuous and do not tie) and within
    2e-3 rad of the configured limit."""
    out = np.zeros(q.shape, bool)
    for ext, lim in ((q.min(0), limits[:, 0]), (q.max(0), limits[:, 1])):
        hit = q == ext
        out |= hit & (hit.sum(0) >= 2) & (np.abs(ext - lim) < 2e-3)
    return out


def assert_same(new, old):
    for a, b, what in zip(new, old, ("qpos", "status", "iters")):
        assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} entries differ"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("rel", CONFIGS)
def test_tracking_frames_bitwise_equal(rel, B):
    seq = build(rel)
    model = seq.optimizer.device_model()
    assert model.kernel() == (_lib.KERNEL_REGISTER, 4, 2)
    kp, last = tracking(seq, model, B)
    new = solve_dev(model, kp, last, True, 1)
    old = solve_dev(model, kp, last, True, 0)
    assert np.isfinite(new[0]).all() and (new[1] == ST_CONVERGED).all() and new[2].min() >= 1
    assert_same(new, old)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("rel", CONFIGS)
def test_cold_starts_bitwise_equal(rel, B):
    """Reachable targets, start sigma = 0.5 rad away: the batches of 4 096 frames and more must contain long solves (more than
    8 passes: rejected steps, raised damping, modified pivots) and answers with a joint on its bound, or the comparison would
    never have reached those branches (a batch of 1 or 64 frames cannot be required to)."""
    seq = build(rel)
    model = seq.optimizer.device_model()
    ref, start = bench_data.reachable_batch(seq, B, 0.5)
    new = solve_dev(model, ref, start, False, 1)
    old = solve_dev(model, ref, start, False, 0)
    n_long = int((new[2] > 8).sum())
    n_bound = int(on_bound(new[0], seq.joint_limits).any(1).sum())
    print(f"{rel} B={B}: iters > 8: {n_long} frames, a joint on its bound: {n_bound} frames, iters max {new[2].max()}")
    if B >= 4096:
        assert n_long > 0 and n_bound > 0
    assert np.isfinite(new[0]).all()
    assert_same(new, old)


@pytest.mark.parametrize("case", ["tol", "max_iter", "newton", "lam_jump"])
@pytest.mark.parametrize("rel", CONFIGS)
def test_non_default_options_bitwise_equal(rel, case):
    seq = build(rel)
    model = seq.optimizer.device_model()
    B = 4096
    ref, start = bench_data.reachable_batch(seq, B, 0.5, seed=bench_data.SEED + 3)
    opts = {"tol": _lib.default_options(tol=1e-4), "max_iter": _lib.default_options(max_iter=3),
            "newton": _lib.default_options(newton=0), "lam_jump": None}[case]
    if case == "lam_jump":
        model.tune(lam_jump=0.0)
    try:
        new = solve_dev(model, ref, start, False, 1, opts=opts)
        old = solve_dev(model, ref, start, False, 0, opts=opts)
    finally:
        model.tune(lam_jump=None)
    assert_same(new, old)
    default = solve_dev(model, ref, start, False, 1)
    assert not np.array_equal(default[2], new[2]), "the option did not change the iteration: nothing was tested"
    if case == "max_iter":
        assert new[2].max() == 3
        hit = new[1] == ST_MAXITER
        assert hit.any() and np.array_equal(hit, old[1] == ST_MAXITER) and np.array_equal(new[0][hit], old[0][hit])


@pytest.mark.parametrize("rel", CONFIGS)
def test_calls_outside_the_dispatch_condition_keep_the_serial_chain_kernel(rel):
    """float64, objective values asked for, sequence mode and queue mode do not take the dedicated kernel: with
    dexr_tuning.kernel = AUTO and REGISTER_CHAIN they run the same code and give the same answers."""
    import torch

    seq = build(rel)
    model = seq.optimizer.device_model()
    B = 4096
    kp, last = tracking(seq, model, B, seed=bench_data.SEED + 7)
    plain = solve_dev(model, kp, last, True, 1)
    # objective values requested
    a, b = solve_dev(model, kp, last, True, 1, fval=True), solve_dev(model, kp, last, True, 0, fval=True)
    assert_same(a, b)
    # (a frame's objective value is the float32 atomic sum of its four components' terms, in the order the waves arrive: equal
    # up to the rounding of three additions, 3 x 2^-24 relative, not bit for bit -- in either kernel choice)
    assert np.allclose(a[3], b[3], rtol=4e-7, atol=0) and (a[3] > 0).all() and np.isfinite(plain[0]).all()
    # float64 launches
    ref, start = bench_data.reachable_batch(seq, 512, 0.5, seed=bench_data.SEED + 9)
    q64 = []
    for tip_kernel in (1, 0):
        model.tune(kernel=_lib.KERNEL_AUTO if tip_kernel else _lib.KERNEL_REGISTER_CHAIN)
        try:
            q64.append(model.retarget_f64(ref, None, start))
        finally:
            model.tune(kernel=_lib.KERNEL_AUTO)
    assert np.isfinite(q64[0]).all() and np.array_equal(q64[0], q64[1])
    # queue mode (persist_from = 0: every batch is drained from the per-component queues): a frame's answer does not
    # depend on which lane solved it
    model.tune(persist_from=0)
    try:
        qa, qb = solve_dev(model, kp, last, True, 1), solve_dev(model, kp, last, True, 0)
    finally:
        model.tune(persist_from=8)
    assert_same(qa, qb)
    # sequence mode: T frames of B sequences in one launch
    T, Bs = 3, 256
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(bench_data.human_keypoints(Bs * T, seed=11).reshape(T, Bs, 21, 3)).to(dev).contiguous()
    raws = []
    for tip_kernel in (1, 0):
        model.tune(kernel=_lib.KERNEL_AUTO if tip_kernel else _lib.KERNEL_REGISTER_CHAIN)
        try:
            t_last = torch.from_numpy(last[:Bs].copy()).to(dev)
            raw = torch.empty((T, Bs, last.shape[1]), dtype=torch.float32, device=dev)
            model.retarget_seq_dev(Bs, T, frames.data_ptr(), 0, t_last.data_ptr(), 0, raw.data_ptr(),
                                   stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            model.tune(kernel=_lib.KERNEL_AUTO)
        raws.append(raw.cpu().numpy())
    assert np.isfinite(raws[0]).all() and np.array_equal(raws[0], raws[1])


def test_register_chain_is_a_tuning_value_of_the_register_family():
    model = build(CONFIGS[0]).optimizer.device_model()
    try:
        model.tune(kernel=_lib.KERNEL_REGISTER_CHAIN)
        assert model.get_tuning().kernel == _lib.KERNEL_REGISTER_CHAIN
        model.tune(max_blind=8)  # (a round trip of the struct keeps the value)
        assert model.get_tuning().kernel == _lib.KERNEL_REGISTER_CHAIN and model.kernel() == (_lib.KERNEL_REGISTER, 4, 2)
    finally:
        model.tune(kernel=_lib.KERNEL_AUTO)
    assert model.kernel() == (_lib.KERNEL_REGISTER, 4, 2)

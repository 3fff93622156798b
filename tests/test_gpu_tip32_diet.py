"""GPU: dexr_tip32_kernel after its instruction diet against the kernel it stands in for, bit for bit, on the solve options no
other test passes to it.

The dedicated float32 tip solve (csrc/dexr_tip_solve.hpp) takes its solve options, the box, joint 0 and the tip offset as the
scalar registers they arrive in (no second pin through a VGPR), forms its derived constants -- 1 / huber_delta, the +inf
thresholds of lam_fastdec / lam_recover, the Newton select -- once before the loop, and keeps the free-variable masks as lane
masks.  Each of these is an option's or a bound's way into the pass.  dexr_tuning.kernel = KERNEL_REGISTER_CHAIN sends the same
call through dexr_kernel<4, float, SOLVE, CHAIN, EXT, TIP>, whose code this left untouched and which is the reference here: qpos,
status and iters are compared with np.array_equal, through the entry point tests/golden/gen_tip_prologue_golden.py uses
(retarget_dev on device copies, the output one tile longer than the batch and pre-filled with NaN).  The same cases held a build
that decided acceptance before it formed the derivatives and updated the kept model in place (tried, dropped).

  * robots: the Allegro and LEAP teleop vector configs; B = 1, 63, 65, 193 (a lone lane, a partial tile, a tile plus one, three
    tiles plus one), reachable_batch(seq, B, 0.5) cold starts: rejected steps, bound-active joints, modified pivots;
  * options: a non-default huber_delta; lam_fastdec = 0 with lam_recover > 0 (both thresholds of the damping ladder +inf or
    live); lam_jump = 0; newton = 0; step_cap = 0; max_iter = 3, where lanes leave with ST_MAXITER on a step they accepted --
    the case an in-place update of the kept model can get wrong;
  * one cold-start case at the default options whose precondition is stated on the REFERENCE kernel's output: within one tile its
    iters take at least four distinct values, i.e. accepting, rejecting, finishing and blind-step lanes share a wave.

Not covered: the kernel's term-without-origin branch (h_origin < 0).  Tip models are per-finger VECTOR models, whose every term
has an origin keypoint, so no shipped tip model reaches it."""
import importlib.util
import os

import numpy as np
import pytest

import bench_data
from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_tip_prologue_golden", os.path.join(HERE, "golden", "gen_tip_prologue_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

ST_MAXITER = 1
HUBER = 5e-3  # (the configs ship 2e-2)
# name -> (huber_delta of the model or None, dexr_tuning overrides, SolveOptions overrides)
CASES = {
    "huber_delta": (HUBER, {}, {}),
    "lam_fastdec_0_lam_recover": (None, {"lam_fastdec": 0.0, "lam_recover": 0.25}, {}),
    "lam_jump_0": (None, {"lam_jump": 0.0}, {}),
    "newton_0": (None, {}, {"newton": 0}),
    "step_cap_0": (None, {"step_cap": 0.0}, {}),
    "max_iter_3": (None, {}, {"max_iter": 3}),
}
_seq, _inputs = {}, {}


def build(robot, huber=None):
    """The robot's retargeting, as shipped (gen's own, shared with the other tests) or with another huber_delta."""
    if huber is None:
        return gen.build(robot)
    if (robot, huber) not in _seq:
        RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
        cfg = RetargetingConfig.load_from_file(os.path.join(bench_data.CONFIG_DIR, gen.ROBOTS[robot]))
        cfg.huber_delta = huber
        _seq[(robot, huber)] = cfg.build()
    return _seq[(robot, huber)]


def cold(robot, B):
    if (robot, B) not in _inputs:
        _inputs[(robot, B)] = bench_data.reachable_batch(gen.build(robot), B, 0.5)
    return _inputs[(robot, B)]


def solve(model, ref, start, kernel, tune, opts):
    """gen.solve with options: retarget_dev on device copies, qpos one tile longer than the batch and pre-filled with NaN."""
    import torch

    dev = torch.device("cuda:0")
    B = start.shape[0]
    t_in, t_last = torch.from_numpy(np.ascontiguousarray(ref)).to(dev), torch.from_numpy(np.ascontiguousarray(start)).to(dev)
    t_q = torch.full((B + gen.TILE, start.shape[1]), float("nan"), dtype=torch.float32, device=dev)
    t_status = torch.zeros(B, dtype=torch.int32, device=dev)
    t_iters = torch.zeros(B, dtype=torch.int32, device=dev)
    before = model.get_tuning()
    restore = {k: (None if k in ("lam_jump", "lam_fastdec") else getattr(before, k)) for k in tune}
    model.tune(kernel=kernel, **tune)
    try:
        model.retarget_dev(B, t_in.data_ptr(), 0, t_last.data_ptr(), 0, t_q.data_ptr(), status_ptr=t_status.data_ptr(),
                           iters_ptr=t_iters.data_ptr(), opts=_lib.default_options(**opts) if opts else None,
                           stream=torch.cuda.current_stream().cuda_stream, keypoints=False)
        torch.cuda.synchronize()
    finally:
        model.tune(kernel=_lib.KERNEL_AUTO, **restore)
    return t_q.cpu().numpy(), t_status.cpu().numpy(), t_iters.cpu().numpy()


def assert_same(new, old, B):
    assert new[0].shape[0] == B + gen.TILE and np.isnan(new[0][B:]).all(), "rows beyond the batch were written"
    assert np.isfinite(new[0][:B]).all()
    for a, b, what in zip(new, old, ("qpos", "status", "iters")):
        assert np.array_equal(a, b, equal_nan=True), f"{what}: {int((a != b).sum())} entries differ"


@pytest.mark.parametrize("B", gen.BATCHES)
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("robot", list(gen.ROBOTS))
def test_options_bitwise_equal(robot, case, B):
    huber, tune, opts = CASES[case]
    model = build(robot, huber).optimizer.device_model()
    assert model.kernel() == (_lib.KERNEL_REGISTER, 4, 2)
    ref, start = cold(robot, B)
    new = solve(model, ref, start, _lib.KERNEL_AUTO, tune, opts)
    old = solve(model, ref, start, _lib.KERNEL_REGISTER_CHAIN, tune, opts)
    print(f"{robot} {case} B={B}: iters mean {old[2].mean():.2f} max {old[2].max()}  status max {old[1].max()}")
    assert_same(new, old, B)
    if case == "max_iter_3":
        assert old[2].max() == 3
        if B >= 63:  # frames that ran out of passes (a frame's status is the maximum over its four components' lanes)
            assert (old[1] == ST_MAXITER).any()
    if B == 193:  # the option reached the kernel: the iteration is not the default one
        default = solve(gen.build(robot).optimizer.device_model(), ref, start, _lib.KERNEL_REGISTER_CHAIN, {}, {})
        assert not (np.array_equal(default[2], old[2]) and np.array_equal(default[0], old[0], equal_nan=True)), \
            "the option did not change the iteration: nothing was tested"


@pytest.mark.parametrize("robot", list(gen.ROBOTS))
def test_cold_starts_with_every_kind_of_lane_in_one_wave(robot):
    B = 193
    model = build(robot).optimizer.device_model()
    ref, start = cold(robot, B)
    old = solve(model, ref, start, _lib.KERNEL_REGISTER_CHAIN, {}, {})
    # stated on the reference kernel: lanes of one tile leave after different numbers of passes
    assert max(len(np.unique(old[2][t:t + gen.TILE])) for t in range(0, B, gen.TILE)) >= 4
    new = solve(model, ref, start, _lib.KERNEL_AUTO, {}, {})
    assert_same(new, old, B)

"""GPU: dexr_tip32_kernel with its pass loop off the LDS round trips, against the kernel it stands in for, bit for bit.

The dedicated float32 tip solve (csrc/dexr_tip_solve.hpp) keeps the lane's target in three registers instead of the lane's LDS
column, and reads the broadcast placements of joints 1..3 in ONE batch at the head of every pass (TipTabRegs, csrc/dexr_tip.hpp)
instead of joint by joint inside the kinematic chain.  Neither changes an operation or an operand, so qpos, status and iters are
compared with np.array_equal against dexr_tuning.kernel = KERNEL_REGISTER_CHAIN -- dexr_kernel<4, float, SOLVE, CHAIN, EXT, TIP>,
whose code is untouched (it reads target and placements from LDS at the point of use) -- through the entry point
tests/golden/gen_tip_prologue_golden.py uses: retarget_dev on device copies, the output one tile longer than the batch and
pre-filled with NaN.

  * the target: both ways it is formed -- keypoint input (task keypoint minus origin keypoint, in the kernel) and ready-made
    ref_value rows (keypoints=False) -- and the lanes of a partial tile, which hold no frame and must write nothing;
  * the placements: both robots' tables, Allegro and LEAP teleop vector;
  * B = 1, 63, 65, 193 (a lone lane, a partial tile, a tile plus one, three tiles plus one); tracking warm starts, and
    reachable_batch(seq, B, 0.5) cold starts: rejected steps, bound-active joints, modified pivots;
  * a pass that skips the evaluation although the placements were read for it: a wave whose every live lane takes its blind
    last step.  At B = 1 a wave has one live lane; the precondition is stated on the REFERENCE kernel's iters: with the blind
    step switched off (blind_tol_scale = 0) the frame needs more passes, so with it at least one of its four waves ended on a
    pass without evaluation.  The frame is the first of a tracking walk of 16 for which that holds (a blind step shorter than
    tol ends the solve in the pass a verified step would have ended it in, and cannot be told from one);
  * one launch of 65 536 frames (blocks of 8 waves begin at 4 096 waves), the headline's frames: checksums and array_equal."""
import importlib.util
import os

import numpy as np
import pytest

from dex_retargeting_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_tip_prologue_golden", os.path.join(HERE, "golden", "gen_tip_prologue_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

_inputs = {}


def inputs(robot, regime, B):
    if (robot, regime, B) not in _inputs:
        _inputs[(robot, regime, B)] = gen.inputs(robot, regime, B)
    return _inputs[(robot, regime, B)]


def assert_same(new, old, B, pad=gen.TILE):
    assert new[0].shape[0] == B + pad and np.isnan(new[0][B:]).all(), "rows beyond the batch were written"
    assert np.isfinite(new[0][:B]).all()
    for a, b, what in zip(new, old, ("qpos", "status", "iters")):
        assert np.array_equal(a, b, equal_nan=True), f"{what}: {int((a != b).sum())} entries differ"


@pytest.mark.parametrize("B", gen.BATCHES)
@pytest.mark.parametrize("regime", gen.REGIMES)
@pytest.mark.parametrize("robot", list(gen.ROBOTS))
def test_bitwise_equal_to_the_register_chain_kernel(robot, regime, B):
    model = gen.build(robot).optimizer.device_model()
    assert model.kernel() == (_lib.KERNEL_REGISTER, 4, 2)
    forms = inputs(robot, regime, B)
    assert ("kp" in forms) == (regime == "tracking")
    inp, last = forms["ref"]
    old = gen.solve(model, inp, last, False, _lib.KERNEL_REGISTER_CHAIN)
    print(f"{robot} {regime} B={B}: iters mean {old[2].mean():.2f} max {old[2].max()}  status max {old[1].max()}")
    for form, (inp, last) in forms.items():  # (the two forms hold the same float32 targets: one reference serves both)
        assert_same(gen.solve(model, inp, last, form == "kp", _lib.KERNEL_AUTO), old, B)


def solve_without_blind_steps(model, inp, last):
    scale = model.get_tuning().blind_tol_scale
    model.tune(blind_tol_scale=0.0)
    try:
        return gen.solve(model, inp, last, True, _lib.KERNEL_REGISTER_CHAIN)
    finally:
        model.tune(blind_tol_scale=scale)


@pytest.mark.parametrize("robot", list(gen.ROBOTS))
def test_pass_without_evaluation(robot):
    B, WALK = 1, 16
    seq = gen.build(robot)
    model = seq.optimizer.device_model()
    # which frames of a short tracking walk end on a blind step, by the reference kernel (a blind step shorter than tol ends the
    # solve in the same pass as a verified one and does not show: those frames are not counted)
    kp, last = gen.tracking(seq, WALK)
    it_blind = gen.solve(model, kp, last, True, _lib.KERNEL_REGISTER_CHAIN)[2]
    it_verified = solve_without_blind_steps(model, kp, last)[2]
    frames = np.flatnonzero(it_blind < it_verified)
    print(f"{robot}: iters {it_blind} with the blind last step, {it_verified} without")
    assert len(frames) > 0
    j = frames[0]
    kp, last = kp[j:j + 1], last[j:j + 1]
    old = gen.solve(model, kp, last, True, _lib.KERNEL_REGISTER_CHAIN)
    # stated on the reference kernel, for the launch of this one frame: a blind last step was taken (every pass in front of it is
    # the same pass in both solves)
    assert old[2][0] < solve_without_blind_steps(model, kp, last)[2][0]
    assert_same(gen.solve(model, kp, last, True, _lib.KERNEL_AUTO), old, B)


def test_full_chip_launch():
    B = gen.FULL_B
    seq = gen.build("allegro")
    model = seq.optimizer.device_model()
    kp, last = gen.tracking(seq, B)  # bench_data.human_keypoints(B + 1), the warm starts bench.py stages
    new = gen.solve(model, kp, last, True, _lib.KERNEL_AUTO)
    old = gen.solve(model, kp, last, True, _lib.KERNEL_REGISTER_CHAIN)
    sums = [(float(q[:B].astype(np.float64).sum()), int(it.sum())) for q, _, it in (new, old)]
    print(f"B={B}: checksum {sums[0][0]:.6f}  iters mean {old[2].mean():.4f} max {old[2].max()}")
    assert sums[0] == sums[1]
    assert_same(new, old, B)

"""GPU: dexr_tip32_kernel keeps the answers of dexr_kernel<4, float, SOLVE, CHAIN, EXT, TIP> bit for bit around the control flow
that steering a wave's issue priority adds (dexr_tip_solve.hpp, DEXR_TIP_PRIO): the ladder inside the pass loop, and the exits
before and inside it.

Priority itself cannot change a result; a branch placed around it can.  So every case solves the same frames twice --
dexr_tuning.kernel = KERNEL_AUTO (dexr_tip32_kernel) and KERNEL_REGISTER_CHAIN (dexr_kernel) -- and compares qpos, status and iters
with np.array_equal:

  * robots: the Allegro and LEAP teleop vector configs;
  * regimes: tracking frames (keypoint input, warm start) and reachable_batch(seq, B, 0.5) cold starts (ref_value rows);
  * B = 1, 63, 65, 193: a lone lane, a partial tile, a tile plus one, three tiles plus one.  These launches are below the size
    the kernel steers priority from (DEXR_TIP_PRIO_MIN_WAVES = 4 096 waves): they cover the policy-OFF path, i.e. that the
    conditions around the policy leave small launches alone.  And 65 537, 4 100 waves: inside the window, the policy ON, blocks
    of eight waves, both halves of the grid (the late half ends its ladder on another rung), a partial last tile;
  * max_iter = 1, 2 and 3 through the call's options, at B = 65 537: every wave of the launch leaves the loop on that rung of the
    ladder -- the exits inside it -- and every frame is finished by the cap at the latest, status MAXITER where it was the cap;
    some frame must run into the cap, or no wave was made to leave there.  The same at B = 65, policy off;
  * qpos is allocated one tile longer than B and pre-filled with NaN: rows beyond B must stay NaN.

max_iter = 0 is not a case: the entry point reads a max_iter that is not positive as "the default" (64), so no option makes a
wave skip the loop; the last test pins that reading, so that a change of it brings the case up again.

The inputs are tests/golden/gen_tip_prologue_golden.py's (imported, as tests/test_gpu_tip_prologue.py does)."""
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

BATCHES = [1, 63, 65, 193, 65537]
FORM = {"tracking": "kp", "cold": "ref"}
STATUS_MAXITER = 1  # DEXR_STATUS_MAXITER (include/dexr.h)
_inputs = {}


def inputs(robot, regime, B):
    key = (robot, regime, B)
    if key not in _inputs:
        _inputs[key] = gen.inputs(robot, regime, B)[FORM[regime]]
    return _inputs[key]


def solve(model, inp, last, keypoints, kernel, max_iter=None):
    """gen.solve with the call's options: qpos (B + TILE, n) pre-filled with NaN, status (B,), iters (B,)."""
    import torch

    dev = torch.device("cuda:0")
    B = last.shape[0]
    opts = None if max_iter is None else _lib.default_options(max_iter=max_iter)
    t_in, t_last = torch.from_numpy(np.ascontiguousarray(inp)).to(dev), torch.from_numpy(np.ascontiguousarray(last)).to(dev)
    t_q = torch.full((B + gen.TILE, last.shape[1]), float("nan"), dtype=torch.float32, device=dev)
    t_status = torch.zeros(B, dtype=torch.int32, device=dev)
    t_iters = torch.zeros(B, dtype=torch.int32, device=dev)
    model.tune(kernel=kernel)
    try:
        model.retarget_dev(B, t_in.data_ptr(), 0, t_last.data_ptr(), 0, t_q.data_ptr(), status_ptr=t_status.data_ptr(),
                           iters_ptr=t_iters.data_ptr(), opts=opts, stream=torch.cuda.current_stream().cuda_stream, keypoints=keypoints)
        torch.cuda.synchronize()
    finally:
        model.tune(kernel=_lib.KERNEL_AUTO)
    return t_q.cpu().numpy(), t_status.cpu().numpy(), t_iters.cpu().numpy()


def both(robot, regime, B, max_iter=None):
    inp, last = inputs(robot, regime, B)
    model = gen.build(robot).optimizer.device_model()
    assert model.kernel()[2] == 2, "not a tip model: neither launch would run a tip kernel"
    got = solve(model, inp, last, FORM[regime] == "kp", _lib.KERNEL_AUTO, max_iter)
    want = solve(model, inp, last, FORM[regime] == "kp", _lib.KERNEL_REGISTER_CHAIN, max_iter)
    q = got[0]
    assert q.shape[0] == B + gen.TILE and np.isnan(q[B:]).all(), "rows beyond the batch were written"
    assert np.isfinite(q[:B]).all()
    for a, b, what in zip(got, want, ("qpos", "status", "iters")):
        assert np.array_equal(a, b, equal_nan=True), f"{what}: {int((a != b).sum())} entries differ from dexr_kernel's"
    return got


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("regime", list(FORM))
@pytest.mark.parametrize("robot", list(gen.ROBOTS))
def test_answers_are_dexr_kernels(robot, regime, B):
    both(robot, regime, B)


@pytest.mark.parametrize("max_iter", [1, 2, 3])
@pytest.mark.parametrize("B", [65, 65537])  # (policy off / policy on: see the module docstring)
@pytest.mark.parametrize("regime", list(FORM))
@pytest.mark.parametrize("robot", list(gen.ROBOTS))
def test_waves_that_leave_on_a_rung_of_the_ladder(robot, regime, B, max_iter):
    _, status, iters = both(robot, regime, B, max_iter)
    assert (iters >= 1).all() and iters.max() <= max_iter
    assert ((status == STATUS_MAXITER) <= (iters == max_iter)).all()
    # (a start 0.5 rad off per joint is not solved in three passes, and of 65 537 tracking frames some need more -- the bench's
    # frames run up to 12; 65 tracking frames may all be through)
    if regime == "cold" or B == 65537:
        assert (status == STATUS_MAXITER).any(), "no frame ran into the cap: no wave was made to leave on this rung"
    if B == 65537:  # every WAVE leaves on the rung: each tile of 64 frames (x its finger components) holds a capped frame
        capped = np.pad(iters == max_iter, (0, -B % gen.TILE)).reshape(-1, gen.TILE).any(1)
        assert capped[:-1].mean() > 0.5, "most waves were through before the cap: the exits on this rung were hardly taken"


def test_max_iter_zero_means_the_default():
    inp, last = inputs("allegro", "cold", 65)
    model = gen.build("allegro").optimizer.device_model()
    zero = solve(model, inp, last, False, _lib.KERNEL_AUTO, 0)
    default = solve(model, inp, last, False, _lib.KERNEL_AUTO, None)
    assert zero[2].max() > 3, "max_iter = 0 capped the solve: it is a case of the ladder tests now"
    for a, b in zip(zero, default):
        assert np.array_equal(a, b, equal_nan=True)

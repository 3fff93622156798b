"""GPU: the float32 tip solve against the answers of the commit before its prologue was reworked (tests/golden/tip_prologue_parent.npz,
written by tests/golden/gen_tip_prologue_golden.py on a build of that commit).

The prologue -- TipTabT<float>::load and what dexr_tip32_kernel does before its pass loop -- reads the component's constants, the
box, the frame offsets and the lane's frame.  Both tip kernels share load(), so tests/test_gpu_tip32_kernel.py, which compares
them with each other, passes whatever load() does wrong; here both are held to recorded answers, bit for bit (np.array_equal on
qpos, status and iters):

  * robots: the Allegro and LEAP teleop vector configs;
  * kernels: KERNEL_AUTO (dexr_tip32_kernel) and KERNEL_REGISTER_CHAIN (dexr_kernel<4, float, SOLVE, CHAIN, EXT, TIP>);
  * B = 1, 63, 65, 193: a lone lane, a partial tile, a tile plus one, three tiles plus one -- the smallest shapes at which the
    lane / tile addressing of the frame loads can go wrong;
  * keypoint input and ready-made ref_value rows (the kernel's kpts == nullptr branch);
  * tracking frames (warm start) and reachable_batch(seq, B, 0.5) cold starts, which reach bound-active joints (lo / hi);
  * qpos is allocated one tile longer than B and pre-filled with NaN: rows beyond B must stay NaN;
  * one 65 536-frame launch (4 096 waves: blocks of eight, no early touch of the frame's lines) against the same rows solved as
    sixteen 4 096-frame launches.  The generator checked that this identity holds on the parent commit (a lane's arithmetic sees
    no other lane) and recorded it under "fullchip_identity".

The kernel's `o < 0` branch (a term without an origin keypoint: h_origin < 0) is not covered: tip models are per-finger VECTOR
models, whose every term has an origin keypoint, so no shipped tip model takes it."""
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

KERNELS = {"auto": _lib.KERNEL_AUTO, "register_chain": _lib.KERNEL_REGISTER_CHAIN}
_inputs = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(gen.OUT)


def inputs(robot, regime, B):
    key = (robot, regime, B)
    if key not in _inputs:
        _inputs[key] = gen.inputs(robot, regime, B)
    return _inputs[key]


@pytest.mark.parametrize("B", gen.BATCHES)
@pytest.mark.parametrize("regime,form", [("tracking", "kp"), ("tracking", "ref"), ("cold", "ref")])  # (cold starts have no keypoints)
@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("robot", list(gen.ROBOTS))
def test_answers_are_the_parent_commits(golden, robot, kernel, regime, form, B):
    inp, last = inputs(robot, regime, B)[form]
    model = gen.build(robot).optimizer.device_model()
    q, status, iters = gen.solve(model, inp, last, form == "kp", KERNELS[kernel])
    key = f"{robot}/{regime}/{B}"
    assert q.shape[0] == B + gen.TILE and np.isnan(q[B:]).all(), "rows beyond the batch were written"
    for got, what in ((q[:B], "qpos"), (status, "status"), (iters, "iters")):
        want = golden[f"{key}/{what}"]
        assert np.array_equal(got, want.astype(got.dtype)), f"{what}: {int((got != want).sum())} entries differ from the parent commit's"


def test_full_chip_launch_equals_its_rows_solved_in_sixteen_launches(golden):
    assert bool(golden["fullchip_identity"]), "the generator found the identity broken on the parent commit: this case has no basis"
    whole, parts = gen.full_chip()
    assert np.isfinite(whole[0]).all()
    for a, b, what in zip(whole, parts, ("qpos", "status", "iters")):
        assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} entries differ"

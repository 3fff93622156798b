"""CPU tests of the differentiable solve: the C-ABI symbols, the float64 reference VJP (tests/vjp_reference.py) against
central differences of the oracle's tight solve, and the autograd module's argument checks."""
import ctypes
import os

import numpy as np
import pytest

from vjp_reference import Targets, held_mask, vjp_reference

from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases, solvers

RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))

CONFIGS = ["teleop/allegro_hand_right.yml", "offline/leap_hand_right.yml", "teleop/shadow_hand_right_dexpilot.yml",
           "teleop/schunk_svh_hand_right.yml"]
VJP_SYMBOLS = ["dexr_retarget_vjp_dev", "dexr_retarget_vjp"]


def test_library_exports_the_vjp_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)  # (symbol lookup only: no device call)
    for name in VJP_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS


def _tight(prob, tg, ref64, fixed, last, x0):
    return solvers.solve_lm_batched(prob, ref64, fixed, last, x0=x0, tol=1e-12, newton=True, max_iter=200, **tg.kw_at(ref64))


@pytest.mark.parametrize("rel", CONFIGS)
def test_reference_vjp_is_the_derivative_of_the_argmin(rel):
    """Directional derivatives of L = gq . q*(ref, last) along random (ref, last) directions: the reference VJP against
    central differences of the oracle's tight solve (tol 1e-12, warm-started at x*), two solves per direction."""
    prob = cases.problem_from_config(rel)
    assert (prob.kind == "vector" and len(prob.mimic) > 0) == ("schunk" in rel)
    B = 16
    d = cases.human_set(prob, B)
    ref, fixed = d["ref"], d["fixed"]
    h = 2.0 ** -13
    # the oracle solve rounds last_qpos to float32 (as the reference does): on the grid of h, last +- h dl (dl a sign vector)
    # stays exact in float32
    last = (np.round(d["last"] / h) * h).astype(np.float32)
    state = np.zeros(B, np.uint32) if prob.kind == "dexpilot" else None
    tg = Targets(prob, ref, state)
    last64 = last.astype(np.float64)
    x = solvers.solve_lm_batched(prob, ref, fixed, last, tol=1e-12, newton=True, max_iter=200, **tg.kw)
    rng = np.random.default_rng(7)
    gq = rng.standard_normal(x.shape)
    gref, glast = vjp_reference(prob, ref, fixed, last, x, gq, state=state)
    dr = rng.standard_normal(ref.shape)
    dr /= np.linalg.norm(dr.reshape(B, -1), axis=1)[:, None, None]
    dl = rng.choice([-1.0, 1.0], size=last.shape)
    assert np.array_equal((last64 + h * dl).astype(np.float32), last64 + h * dl)
    ref64 = ref.astype(np.float64)
    xp = _tight(prob, tg, ref64 + h * dr, fixed, last64 + h * dl, x)
    xm = _tight(prob, tg, ref64 - h * dr, fixed, last64 - h * dl, x)
    fd = np.einsum("bn,bn->b", gq, (xp - xm) / (2 * h))
    an = np.einsum("bij,bij->b", gref, dr) + np.einsum("bn,bn->b", glast, dl)
    scale = np.linalg.norm(gref.reshape(B, -1), axis=1) + np.linalg.norm(glast, axis=1)
    err = np.abs(fd - an) / scale
    assert err.max() <= 1e-4, (rel, err)


def test_reference_vjp_with_a_joint_held_at_its_bound():
    """Frames whose start sits on a joint limit the objective pushes against: the held variable gets no gradient and the
    free ones still match the tight-solve differences."""
    rel = "teleop/allegro_hand_right.yml"
    prob = cases.problem_from_config(rel)
    B = 16
    d = cases.human_set(prob, B)
    ref, fixed = d["ref"], d["fixed"]
    lo, hi = prob.bounds
    tg = Targets(prob, ref)
    x = solvers.solve_lm_batched(prob, ref, fixed, d["last"], tol=1e-12, newton=True, max_iter=200)
    # pull `last` hard beyond a bound on the variable of each frame that is closest to one: its minimiser then sits on it
    j = np.argmin(np.minimum(x - lo, hi - x), axis=1)
    last = x.copy()
    rows = np.arange(B)
    to_lo = (x - lo)[rows, j] < (hi - x)[rows, j]
    last[rows, j] = np.where(to_lo, lo[j] - 2.0, hi[j] + 2.0)
    last = last.astype(np.float32)
    last64 = last.astype(np.float64)
    x = solvers.solve_lm_batched(prob, ref, fixed, last, x0=x, tol=1e-12, newton=True, max_iter=200)
    held = held_mask(prob, x)
    assert held[rows, j].sum() >= B // 2, held[rows, j]
    rng = np.random.default_rng(11)
    gq = rng.standard_normal(x.shape)
    gref, glast = vjp_reference(prob, ref, fixed, last, x, gq)
    assert np.all(glast[held] == 0)
    dr = rng.standard_normal(ref.shape)
    dr /= np.linalg.norm(dr.reshape(B, -1), axis=1)[:, None, None]
    h = 1e-4
    ref64 = ref.astype(np.float64)
    xp = _tight(prob, tg, ref64 + h * dr, fixed, last64, x)
    xm = _tight(prob, tg, ref64 - h * dr, fixed, last64, x)
    assert np.all(xp[held] == x[held]) and np.all(xm[held] == x[held])
    fd = np.einsum("bn,bn->b", gq, (xp - xm) / (2 * h))
    an = np.einsum("bij,bij->b", gref, dr)
    err = np.abs(fd - an) / np.linalg.norm(gref.reshape(B, -1), axis=1)
    assert err.max() <= 1e-4, err


def _optimizer(rel="teleop/allegro_hand_right.yml"):
    return RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer


def test_autograd_rejects_cpu_tensors_and_bad_shapes():
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    opt = _optimizer()
    n = opt.opt_dof
    n_ref = opt.compiled_model().n_ref
    ref = torch.zeros((4, n_ref, 3))
    last = torch.zeros((4, n))
    with pytest.raises(ValueError, match="CUDA"):
        ag.retarget(opt, ref, last)  # CPU tensors of the right shapes
    with pytest.raises(ValueError, match="torch tensors"):
        ag.retarget(opt, ref.numpy(), last)
    with pytest.raises(ValueError, match="ref_value must have shape"):
        ag.retarget(opt, ref[:, :-1], last)
    with pytest.raises(ValueError, match="last_qpos must have shape"):
        ag.retarget(opt, ref, last[:, :-1])
    with pytest.raises(ValueError, match="float32"):
        ag.retarget(opt, ref, last.double())
    with pytest.raises(ValueError, match="state"):
        ag.retarget(opt, ref, last, state=torch.zeros(3, dtype=torch.int32))
    kp = torch.zeros((4, 21, 3), requires_grad=True)
    rv = ag.ref_value_from_keypoints(opt, kp)
    assert tuple(rv.shape) == (4, n_ref, 3)
    rv.sum().backward()
    assert kp.grad is not None
    with pytest.raises(ValueError):
        ag.ref_value_from_keypoints(opt, torch.zeros((4, 21)))

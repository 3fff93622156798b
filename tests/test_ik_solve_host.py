"""CPU tests of the IK solve's interface (include/dexr_ik_solve.h, jacobians.link_ik_solve): the export list against the header,
the argument rules of the torch front (every one a ValueError before any device call), and the behaviour of the yardstick
tests/ik_solve_reference.py on the inputs of tests/test_gpu_ik_solve.py, so that the inputs are proven before a GPU sees them.

INPUTS (solve_inputs; both sets share robot, links, q*, damping and B = 33 with test_ik_host.tracking_inputs).  Targets are the
poses of q* in float64 (a float32 run rounds them; rounded targets are not reachable exactly and would put a floor of 1e-6 of the
initial error under test (i)), weights w_lin ~ U(0.5, 2), w_ang ~ 0.01 U(0.5, 2) from default_rng(SEED); starts, weights, limits
and damping are float32-representable.
  "near"   start = the tracking start (q* + U(-0.1, 0.1), clipped), limits = the robot's, no step limit.
  "tight"  limits pulled in by a quarter of their range on each side, start = clip(q* + U(-0.3, 0.3)) into them (same generator),
           max_step = 0.2: about half of the variables end on a bound.
SEED = 5 is the first seed tried: the freeze decisions of the float32 and the float64 reference runs agree on every frame of
the six hands with it (test (iii) below)."""
import functools
import os
import re

import numpy as np
import pytest

import ik_solve_reference as isr
import test_gpu_link_poses as glp
from testutil import REPO
from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_ik_host import TRACK_B, tracking_inputs
from test_jacobian_host import SUBSET_CFG

RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
HEADER = os.path.join(REPO, "include", "dexr_ik_solve.h")
SEED, STEPS = 5, 8
ARM, GRIPPER = "arm_shadow_hand_right", "panda_gripper_glb"
KINDS = ("near", "tight")


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def solve_inputs(name, kind):
    """dict: orc, links, x0 (33, dof), tgt_pos, tgt_rot, w_lin, w_ang, lo, hi, damping, max_step; arrays read-only."""
    assert kind in KINDS
    orc, links, q_star, q0, damping = tracking_inputs(name)
    tgt_pos, tgt_rot = isr.link_poses(orc, q_star, links)  # float64: a float32 run rounds them, as it must
    rng = np.random.default_rng(SEED)
    w_lin = _r32(rng.uniform(0.5, 2, (TRACK_B, len(links))))
    w_ang = _r32(0.01 * rng.uniform(0.5, 2, (TRACK_B, len(links))))
    lim = orc.joint_limits
    lo, hi, x0, max_step = _r32(lim[:, 0]), _r32(lim[:, 1]), q0, 0.0
    if kind == "tight":
        quarter = 0.25 * (lim[:, 1] - lim[:, 0])
        lo, hi = _r32(lim[:, 0] + quarter), _r32(lim[:, 1] - quarter)
        x0 = _r32(q_star + rng.uniform(-0.3, 0.3, q_star.shape))
        max_step = 0.2
    x0 = np.clip(x0, lo, hi)
    assert (lo < hi).all() and np.array_equal(x0, _r32(x0))
    d = dict(orc=orc, links=links, x0=x0, tgt_pos=tgt_pos, tgt_rot=tgt_rot, w_lin=w_lin, w_ang=w_ang, lo=lo, hi=hi,
             damping=float(np.float32(damping)), max_step=max_step)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, kind, dtype=np.float64, max_iters=STEPS, tol=0.0):
    """the yardstick's run on solve_inputs(name, kind), computed once and shared: (xs, frozen, iters, errs), read-only."""
    d = solve_inputs(name, kind)
    out = isr.ik_solve(d["orc"], d["x0"], d["links"], d["tgt_pos"], d["tgt_rot"], d["w_lin"], d["w_ang"], d["lo"], d["hi"], d["damping"],
                       max_iters, tol, d["max_step"], dtype)
    for a in out:
        a.setflags(write=False)
    return out


def test_exports_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    assert declared == set(_lib.IK_SOLVE_EXPORTS) and len(_lib.IK_SOLVE_EXPORTS) == 2 and len(set(_lib.IK_SOLVE_EXPORTS)) == 2
    assert len(_lib.IK_EXPORTS) == 2
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS, _lib.WRENCH_EXPORTS, _lib.IK_EXPORTS):
        assert not set(_lib.IK_SOLVE_EXPORTS) & set(other)
    lib = _lib.load()
    for name in _lib.IK_SOLVE_EXPORTS:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in ("dexr_ik.h", "dexr_wrench.h", "dexr_jacobian.h", "dexr_pose.h"):
        assert not _declared(os.path.join(REPO, "include", h)) & declared
    from dex_retargeting_amd import jacobians as jac

    assert "link_ik_solve" in jac.__all__ and "robot_link_ik_solve" in jac.__all__


def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import jacobians as jac

    touched = []
    monkeypatch.setattr(_lib.PoseModel, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("ik_solve_dev", "ik_step_dev", "poses_dev", "wrenches_dev", "velocities_dev", "jacobians_dev"):
        monkeypatch.setattr(_lib.PoseModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip"]
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    p = torch.zeros((4, 2, 3), dtype=torch.float32)
    r = torch.eye(3, dtype=torch.float32).expand(4, 2, 3, 3).contiguous()
    w = torch.ones((4, 2), dtype=torch.float32)
    lim = torch.tensor([[-1.0, 1.0]] * 16, dtype=torch.float32)

    def raises(q=good, names=tips, match=None, **kw):
        kw.setdefault("target_pos", p)
        kw.setdefault("damping", 1e-3)
        kw.setdefault("max_iters", 8)
        with pytest.raises(ValueError, match=match):
            jac.link_ik_solve(opt, q, names, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises(match="CUDA")
    raises(match="CUDA", target_pos=None, target_rot=r)
    raises(match="CUDA", target_rot=r, pos_weight=w, rot_weight=w, limits=lim, tol=1e-4, max_step=0.2)
    raises(match="CUDA", damping=1, max_iters=1, tol=0, max_step=0)  # Python ints are numbers too
    raises(match="CUDA", max_iters=256)
    with pytest.raises(ValueError, match="CUDA"):
        jac.robot_link_ik_solve(opt.robot, good, tips, p, r, w, w, 1e-3, 8, 0.0, 0.0, lim)
    with pytest.raises(ValueError, match="CUDA"):
        jac.link_ik_solve(opt, good, tips, p, r, w, w, 1e-3, 8, 0.0, 0.0, lim, None)
    # the wrong dtype
    raises(q=good.double(), match="float32")
    raises(target_pos=p.double(), match="float32")
    raises(target_rot=r.half(), match="float32")
    raises(pos_weight=w.double(), match="float32")
    raises(target_rot=r, rot_weight=w.long(), match="float32")
    raises(limits=lim.double(), match="float32")
    # the wrong shape of a target, a weight, the limits (and of q); tensors that are none
    for bad in (p[:3], p[:, :1], p[:, :, :2], p.reshape(4, 6), torch.zeros((4, 3, 3))):
        raises(target_pos=bad, match="shape")
    for bad in (r[:3], r[:, :1], r[:, :, :2], r[..., :2], r.reshape(4, 2, 9), p):
        raises(target_rot=bad, match="shape")
    for bad in (w[:3], w[:, :1], w.reshape(-1), w[:, :, None], torch.ones((4, 2, 3))):
        raises(pos_weight=bad, match="shape")
        raises(target_rot=r, rot_weight=bad, match="shape")
    for bad in (lim[:15], lim.t(), lim[:, :1], lim.reshape(-1), torch.zeros((16, 3))):
        raises(limits=bad, match="shape")
    raises(target_pos=p.numpy(), match="torch tensor")
    raises(target_rot=r.numpy(), match="torch tensor")
    raises(pos_weight=w.numpy(), match="torch tensor")
    raises(limits=lim.numpy(), match="torch tensor")
    raises(limits=[[-1.0, 1.0]] * 16, match="torch tensor")
    for bad in (good[:3], good[:, :15], good.reshape(-1)):
        raises(q=bad)
    raises(q=good.numpy(), match="torch tensor")
    # both targets None; a weight without its target
    with pytest.raises(ValueError, match="both None"):
        jac.link_ik_solve(opt, good, tips, damping=1e-3, max_iters=8)
    with pytest.raises(ValueError, match="both None"):
        jac.robot_link_ik_solve(opt.robot, good, tips, None, None, damping=1e-3, max_iters=8)
    raises(target_pos=None, target_rot=r, pos_weight=w, match="pos_weight given without target_pos")
    raises(rot_weight=w, match="rot_weight given without target_rot")
    # damping and max_iters: required; damping a positive finite Python float, max_iters a Python int in 1..256
    with pytest.raises(ValueError, match="damping is required"):
        jac.link_ik_solve(opt, good, tips, p, max_iters=8)
    with pytest.raises(ValueError, match="max_iters is required"):
        jac.link_ik_solve(opt, good, tips, p, damping=1e-3)
    with pytest.raises(ValueError, match="max_iters is required"):
        jac.robot_link_ik_solve(opt.robot, good, tips, p, damping=1e-3)
    for bad in (0, 0.0, -1, -1.0, float("nan"), float("inf"), -float("inf"), torch.tensor(1e-3), None, "1e-3", True):
        raises(damping=bad, match="damping")
    for bad in (0, -1, 257, 8.0, float("nan"), torch.tensor(8), None, "8", True):
        raises(max_iters=bad, match="max_iters")
    # tol and max_step: finite Python floats >= 0
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.0), None, "0", True):
        raises(tol=bad, match="tol")
        raises(max_step=bad, match="max_step")
    # an unknown link, names that are no list, more than 64 links
    raises(names=["link_15.0_tip", "no_such_link"], match="is not a link name")
    raises(names="link_15.0_tip")
    raises(names=[])
    many = (tips * 33)[:65]
    raises(names=many, target_pos=torch.zeros((4, 65, 3), dtype=torch.float32), match="at most 64 links")
    with pytest.raises(ValueError, match="at most 64 links"):
        jac.robot_link_ik_solve(opt.robot, good, many, torch.zeros((4, 65, 3), dtype=torch.float32), damping=1e-3, max_iters=8)
    with pytest.raises(ValueError, match="CUDA"):  # 64 links are one table
        jac.link_ik_solve(opt, good, many[:64], torch.zeros((4, 64, 3), dtype=torch.float32), damping=1e-3, max_iters=8)
    # there is no frame argument
    with pytest.raises(TypeError):
        jac.link_ik_solve(opt, good, tips, p, damping=1e-3, max_iters=8, frame="local")
    # fixed_qpos: one too many, one missing, one of the wrong width
    raises(fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    assert len(sub.idx_pin2fixed) == 6
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    with pytest.raises(ValueError, match="fixed_qpos"):
        jac.link_ik_solve(sub, q10, tips, p, damping=1e-3, max_iters=8)
    with pytest.raises(ValueError, match="fixed_qpos"):
        jac.link_ik_solve(sub, q10, tips, p, damping=1e-3, max_iters=8, fixed_qpos=torch.zeros((4, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="shape"):
        jac.link_ik_solve(sub, q10, tips, p, damping=1e-3, max_iters=8, limits=lim, fixed_qpos=torch.zeros((4, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match="CUDA"):
        jac.link_ik_solve(sub, q10, tips, target_rot=r, damping=1e-3, max_iters=8, limits=lim[:10],
                          fixed_qpos=torch.zeros((4, 6), dtype=torch.float32))
    assert touched == []


# ---- the yardstick's own behaviour on the inputs of the GPU tests ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(glp.ROBOTS))
def test_near_start_inputs_converge_in_the_reference(name):
    """(i) every hand's error falls below 1e-6 of its initial value within 8 steps; the arm's only falls."""
    assert len(glp.ROBOTS) == 8 and ARM in glp.ROBOTS and GRIPPER in glp.ROBOTS
    d = solve_inputs(name, "near")
    xs, frozen, iters, errs = reference(name, "near")
    assert xs.shape == (STEPS + 1, TRACK_B, d["orc"].dof) and frozen.shape == (STEPS, TRACK_B, d["orc"].dof) and errs.shape == (STEPS + 1, TRACK_B)
    assert np.isfinite(xs).all() and np.isfinite(errs).all() and (errs[0] > 0).all()
    ratio = float((errs[-1] / errs[0]).max())
    print(f"{name}: error after {STEPS} steps / initial error, worst frame {ratio:.3e}; largest initial error {errs[0].max():.3e}; "
          f"iters {np.bincount(iters, minlength=STEPS + 1).tolist()}; frozen decisions {int(frozen.sum())}")
    assert ratio < (1.0 if name == ARM else 1e-6), name
    assert ((xs >= d["lo"]) & (xs <= d["hi"])).all()


@pytest.mark.parametrize("name", sorted(glp.ROBOTS))
def test_tight_bound_inputs_end_on_their_bounds_in_the_reference(name):
    """(ii) at least a quarter of the active entries of the result sit exactly on a bound, every entry is within the bounds."""
    d = solve_inputs(name, "tight")
    xs, frozen, iters, errs = reference(name, "tight")
    act = isr.active_columns(d["orc"], d["x0"], d["links"])
    x = xs[-1][:, act]
    on = (x == d["lo"][act]) | (x == d["hi"][act])
    print(f"{name}: {int(act.sum())} active columns of {len(act)}; {on.mean():.3f} of the active entries end on a bound; "
          f"{int(frozen.sum())} frozen decisions; error after / before, worst frame {float((errs[-1] / errs[0]).max()):.3e}")
    assert act.any() and on.mean() >= 0.25, name
    assert ((xs >= d["lo"]) & (xs <= d["hi"])).all() and np.isfinite(errs).all()
    assert frozen.any() and (np.abs(np.diff(xs, axis=0)).max((1, 2)) <= 0.2 * (1 + 1e-12)).all()
    assert np.array_equal(xs[:, :, ~act], np.broadcast_to(d["x0"][:, ~act], xs[:, :, ~act].shape))  # unread columns never move


@pytest.mark.parametrize("name", sorted(set(glp.ROBOTS) - {ARM, GRIPPER}))
def test_float32_and_float64_reference_runs_freeze_alike(name):
    """(iii) the two runs take the same freeze decisions on every frame of the six hands, on both input sets (the gripper's
    error reaches exact zero, after which the sign of g is rounding noise; the arm's float32 iterates drift enough to flip
    one: both exempt)."""
    for kind in KINDS:
        f64, f32 = reference(name, kind)[1], reference(name, kind, np.float32)[1]
        differing = int((f64 != f32).any((0, 2)).sum())
        dist = float(np.abs(reference(name, kind, np.float32)[0][-1].astype(np.float64) - reference(name, kind)[0][-1]).max())
        print(f"{name} {kind}: {f64.size} decisions, {int(f64.sum())} frozen, frames with a differing decision: {differing}; "
              f"float32 run is {dist:.3e} from the float64 run")
        assert reference(name, kind, np.float32)[0].dtype == np.float32
        assert differing == 0, (name, kind)

"""CPU tests of the link-wrench / velocity-VJP interface (include/dexr_wrench.h, jacobians.link_wrenches,
autograd.link_velocities): the export list against the header, the argument rules of the torch front (every one a ValueError
before any device call), and the yardstick itself: tests/velocity_vjp_reference.py against central differences of the
oracle's own Jacobians contracted with the rate."""
import os
import re

import numpy as np
import pytest

import pose_zoo
import velocity_vjp_reference as ref
from testutil import REPO
from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from oracle.kin import OracleRobot
from test_gpu_link_jacobians import oracle_jacobians, to_local
from test_jacobian_host import SUBSET_CFG

RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
HEADER = os.path.join(REPO, "include", "dexr_wrench.h")


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


def test_wrench_exports_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    assert declared == set(_lib.WRENCH_EXPORTS) and len(_lib.WRENCH_EXPORTS) == 4 and len(set(_lib.WRENCH_EXPORTS)) == 4
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS):
        assert not set(_lib.WRENCH_EXPORTS) & set(other)
    lib = _lib.load()
    for name in _lib.WRENCH_EXPORTS:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    # the two older headers keep their functions: the new ones live in the new header alone
    for h in ("dexr_jacobian.h", "dexr_pose.h"):
        assert not _declared(os.path.join(REPO, "include", h)) & declared
    assert (_lib.JAC_WORLD_ALIGNED, _lib.JAC_LOCAL) == (ref.WORLD, ref.LOCAL)


def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag
    from dex_retargeting_amd import jacobians as jac

    touched = []
    monkeypatch.setattr(_lib.PoseModel, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("wrenches_dev", "velocities_vjp_dev", "velocities_dev", "jacobians_dev"):
        monkeypatch.setattr(_lib.PoseModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip"]
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    w = torch.zeros((4, 2, 3), dtype=torch.float32)

    def wrench_raises(q=good, names=tips, match=None, **kw):
        kw.setdefault("force", w)
        with pytest.raises(ValueError, match=match):
            jac.link_wrenches(opt, q, names, **kw)

    def vel_raises(q=good, qdot=good, names=tips, match=None, **kw):
        with pytest.raises(ValueError, match=match):
            ag.link_velocities(opt, q, qdot, names, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    wrench_raises(match="CUDA")
    wrench_raises(match="CUDA", force=None, torque=w)
    wrench_raises(match="CUDA", torque=w, frame="local")
    vel_raises(match="CUDA")
    vel_raises(match="CUDA", frame="local", angular=False)
    with pytest.raises(ValueError, match="CUDA"):
        jac.robot_link_wrenches(opt.robot, good, tips, force=w)
    with pytest.raises(ValueError, match="CUDA"):
        ag.robot_link_velocities(opt.robot, good, good, tips)
    # the wrong dtype
    wrench_raises(q=good.double(), match="float32")
    wrench_raises(force=w.double(), match="float32")
    wrench_raises(torque=w.half(), match="float32")
    vel_raises(q=good.double(), qdot=good.double(), match="float32")
    vel_raises(qdot=good.double(), match="float32")
    # the wrong shape of force, torque or qdot (and of q); tensors that are none
    for bad in (w[:3], w[:, :1], w[:, :, :2], w.reshape(4, 6), torch.zeros((4, 3, 3))):
        wrench_raises(force=bad, match="shape")
        wrench_raises(torque=bad, match="shape")
    wrench_raises(force=w.numpy(), match="torch tensor")
    wrench_raises(torque=[[0.0] * 3] * 2)
    for bad in (good[:3], good[:, :15], good.reshape(-1)):
        vel_raises(qdot=bad, match="shape")
        wrench_raises(q=bad)
        vel_raises(q=bad, qdot=bad)
    vel_raises(qdot=good.numpy())
    # both of force and torque None
    with pytest.raises(ValueError, match="both None"):
        jac.link_wrenches(opt, good, tips)
    with pytest.raises(ValueError, match="both None"):
        jac.robot_link_wrenches(opt.robot, good, tips, None, None)
    # an unknown link, names that are no list
    wrench_raises(names=["link_15.0_tip", "no_such_link"], match="is not a link name")
    vel_raises(names=tips + ["no_such_link"], match="is not a link name")
    wrench_raises(names="link_15.0_tip")
    vel_raises(names="link_15.0_tip")
    vel_raises(names=[])
    # an unknown frame
    for frame in ("LOCAL", "body", 1, None):
        wrench_raises(frame=frame, match="frame")
        vel_raises(frame=frame, match="frame")
    # fixed_qpos: one too many, one missing, one of the wrong width
    wrench_raises(fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    vel_raises(fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    assert len(sub.idx_pin2fixed) == 6
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    with pytest.raises(ValueError, match="fixed_qpos"):
        jac.link_wrenches(sub, q10, tips, force=w)
    with pytest.raises(ValueError, match="fixed_qpos"):
        ag.link_velocities(sub, q10, q10, tips)
    with pytest.raises(ValueError, match="fixed_qpos"):
        ag.link_velocities(sub, q10, q10, tips, fixed_qpos=torch.zeros((4, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="CUDA"):
        jac.link_wrenches(sub, q10, tips, torque=w, fixed_qpos=torch.zeros((4, 6), dtype=torch.float32))
    assert touched == []


# ---- the yardstick against an independent one: central differences of einsum(oracle_jacobians(q), qd), float64 ----------------
H = 1e-5


def _fd_check(orc, links, q, tag):
    """max |reference - central differences| in q and in qd against 1e-6 max(1, max |want|), both frames.  Truncation is
    h^2 O(10) = 1e-9 and round-off 1e-16 / h = 1e-11 times the loss: both sit orders below the gate."""
    rng = np.random.default_rng(43)
    B, L = q.shape[0], len(links)
    qd = rng.standard_normal(q.shape)
    gv, gw = rng.standard_normal((B, L, 3)), rng.standard_normal((B, L, 3))

    def loss(q_, qd_, frame):
        jl, ja, R = oracle_jacobians(orc, q_, links)
        v, w = np.einsum("blrc,bc->blr", jl, qd_), np.einsum("blrc,bc->blr", ja, qd_)
        if frame == ref.LOCAL:
            v, w = to_local(R, v), to_local(R, w)
        return (v * gv).sum((1, 2)) + (w * gw).sum((1, 2))

    for frame in (ref.WORLD, ref.LOCAL):
        gq, gqd = ref.velocity_vjp(orc, q, qd, links, gv, gw, frame)
        fq, fqd = np.zeros_like(q), np.zeros_like(q)
        for c in range(q.shape[1]):
            e = np.zeros(q.shape[1])
            e[c] = H
            fq[:, c] = (loss(q + e, qd, frame) - loss(q - e, qd, frame)) / (2 * H)
            fqd[:, c] = (loss(q, qd + e, frame) - loss(q, qd - e, frame)) / (2 * H)
        e_q, e_qd = np.abs(gq - fq).max(), np.abs(gqd - fqd).max()
        print(f"{tag} frame={frame}: max |grad_q - central differences| = {e_q:.3e} at max |grad_q| = {np.abs(fq).max():.3f}, "
              f"max |grad_qd - central differences| = {e_qd:.3e} at max |grad_qd| = {np.abs(fqd).max():.3f}")
        assert e_q <= 1e-6 * max(1.0, np.abs(fq).max()), (tag, frame)
        assert e_qd <= 1e-6 * max(1.0, np.abs(fqd).max()), (tag, frame)
        # the pieces: one cotangent alone, the wrench product, the forward the gradient is of
        a, b = ref.velocity_vjp(orc, q, qd, links, gv, None, frame), ref.velocity_vjp(orc, q, qd, links, None, gw, frame)
        assert np.abs(a[0] + b[0] - gq).max() <= 1e-12 * max(1.0, np.abs(gq).max()) and np.abs(a[1] + b[1] - gqd).max() <= 1e-12 * max(1.0, np.abs(gqd).max())
        assert np.array_equal(ref.wrenches(orc, q, links, gv, gw, frame), gqd)
        jl, ja, R = oracle_jacobians(orc, q, links)
        v, w = np.einsum("blrc,bc->blr", jl, qd), np.einsum("blrc,bc->blr", ja, qd)
        if frame == ref.LOCAL:
            v, w = to_local(R, v), to_local(R, w)
        lin, ang = ref.link_velocities(orc, q, qd, links, frame)
        assert np.abs(lin - v).max() <= 1e-12 * max(1.0, np.abs(v).max()) and np.abs(ang - w).max() <= 1e-12 * max(1.0, np.abs(w).max())
    return np.abs(fq).max()


@pytest.mark.parametrize("urdf,free", [("shadow_hand/shadow_hand_right.urdf", True), ("panda_gripper/panda_gripper_glb.urdf", False)])
def test_reference_equals_central_differences_of_the_oracle_jacobians(urdf, free):
    orc = OracleRobot(os.path.join(cases.URDF_DIR, urdf), free)
    links = orc.links[::3] + [orc.links[-1]]
    lim = orc.joint_limits
    q = np.random.default_rng(42).uniform(lim[:, 0], lim[:, 1], (3, orc.dof))
    _fd_check(orc, links, q, f"{urdf} free={free}")


def test_reference_equals_central_differences_below_revolute_and_prismatic_forks(tmp_path):
    """prismatic joints with revolute ancestors (the (W x a) . F term, which neither robot above reaches) and forks: a
    heap-shaped tree of the pose zoo, every sixth joint prismatic."""
    m = pose_zoo.build("two_trees100_a", tmp_path)
    links = m.links[::7] + [m.links[-1], m.links[5], m.links[11]]
    lim = m.orc.joint_limits
    q = np.random.default_rng(44).uniform(lim[:, 0], lim[:, 1], (3, m.orc.dof))
    assert _fd_check(m.orc, links, q, "two_trees100_a") > 1e-3
    # the dtype argument: a float32 run of the reference stays float32 and stays near its float64 run
    qd = np.random.default_rng(45).standard_normal(q.shape)
    g = np.random.default_rng(46).standard_normal((3, len(links), 3))
    g64 = ref.velocity_vjp(m.orc, q, qd, links, g, g)
    g32 = ref.velocity_vjp(m.orc, q.astype(np.float32), qd.astype(np.float32), links, g.astype(np.float32), g.astype(np.float32),
                           dtype=np.float32)
    assert g32[0].dtype == g32[1].dtype == np.float32
    assert 0 < np.abs(g32[0] - g64[0]).max() <= 1e-3 * max(1.0, np.abs(g64[0]).max())

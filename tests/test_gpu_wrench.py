"""GPU tests of the link-wrench / velocity-VJP kernels (csrc/dexr_pose.hip, include/dexr_wrench.h): the float64 host entry
points against tests/velocity_vjp_reference.py (robot order, optimizer order with the mimic fold and fixed joints), against
the Jacobian matrix and the link-pose VJP, the float32 device entry points against the float64 host twin, the table limits on
the synthetic robots of tests/pose_zoo.py, batch shapes, the raw ABI's argument errors and the torch front.

GATES OF THE FLOAT32 TESTS.  tau / grad_xdot is the contraction of the Jacobian with the cotangents, so its gate is the sum
over its terms of |cotangent| times the gate of the Jacobian entry it multiplies (pose_zoo.gates, derived in the docstring of
tests/test_gpu_pose_zoo.py; the `_local` variants in the local frame), entry by entry:
    gate(tau[b, c]) = sum_l |force[b, l]|_1 g_jlin[l, c] + |torque[b, l]|_1 g_jang[l, c].
No existing gate covers grad_x (a second derivative), so it is measured, never against the kernel: the reference helper runs
once in float64 and once with every operation in float32 on the same inputs, and the device may be 4 x as far from the float64
host twin as the reference's float32 run is from its own float64 run (max norm, per robot, frame and table).  The factor covers
another summation order (per-joint range sums against per-link chains) and fma contraction.  Both figures are printed; those
of the MI355X are in docs/experiments/link_wrenches.md."""
import os

import numpy as np
import pytest

import pose_zoo as zoo
import test_gpu_link_poses as glp
import velocity_vjp_reference as ref
from dex_retargeting_amd import _lib
from dex_retargeting_amd import pose_tables as pt
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from oracle import cases
from oracle.kin import OracleRobot
from test_gpu_link_jacobians import OPT_ORDER, _gate, _opt_inputs, _optimizer_and_problem
from test_jacobian_host import SUBSET_CFG

pytestmark = pytest.mark.gpu
ROBOTS = glp.ROBOTS
WORLD, LOCAL = _lib.JAC_WORLD_ALIGNED, _lib.JAC_LOCAL
FRAMES = (WORLD, LOCAL)


def _r32(a):
    return a.astype(np.float32).astype(np.float64)


def _configs(robot, B, seed):
    lim = robot.joint_limits
    return np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (B, robot.dof))


def _cotangents(B, L, seed):
    rng = np.random.default_rng(seed)
    return _r32(rng.standard_normal((B, L, 3))), _r32(rng.standard_normal((B, L, 3)))


# ---- the float32 device entry points on numpy arrays, every output pre-filled with NaN -----------------------------------------
def _dev(torch, a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def dev_vjp(model, torch, x, xd, gl, ga, fixed=None, frame=WORLD, want_x=True, want_xd=True):
    """dexr_link_velocities_vjp_dev -> numpy (grad_x or None, grad_xdot or None)."""
    B = x.shape[0]
    tx, txd, tf, tgl, tga = (_dev(torch, a) for a in (x, xd, fixed, gl, ga))
    gx = _nan(torch, (B, model.n_in)) if want_x else None
    gxd = _nan(torch, (B, model.n_in)) if want_xd else None
    model.velocities_vjp_dev(B, _ptr(tx), _ptr(tf), _ptr(txd), _ptr(tgl), _ptr(tga), _ptr(gx), _ptr(gxd), frame=frame,
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (None if gx is None else gx.cpu().numpy()), (None if gxd is None else gxd.cpu().numpy())


def dev_wrenches(model, torch, x, force, torque, fixed=None, frame=WORLD):
    B = x.shape[0]
    tx, tf, tfo, tto = (_dev(torch, a) for a in (x, fixed, force, torque))
    tau = _nan(torch, (B, model.n_in))
    model.wrenches_dev(B, _ptr(tx), _ptr(tf), _ptr(tfo), _ptr(tto), _ptr(tau), frame=frame, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return tau.cpu().numpy()


# ---- 1. float64 host twin against the reference helper, robot order ---------------------------------------------------------------
@pytest.mark.parametrize("name,free", [("shadow_hand_right", True), ("panda_gripper_glb", False), ("arm_shadow_hand_right", False)])
def test_host_float64_against_the_reference_robot_order(name, free, require_gpu):
    robot = RobotWrapper(ROBOTS[name], add_dummy_free_joints=free)
    orc = OracleRobot(ROBOTS[name], free)
    links = [f.name for f in robot.kin.frames][:64]
    B = 33
    q = _configs(robot, B, 21)
    qd = np.random.default_rng(22).standard_normal(q.shape)
    gl, ga = _cotangents(B, len(links), 23)
    model = robot.pose_model(links)
    for frame in FRAMES:
        want_q, want_qd = ref.velocity_vjp(orc, q, qd, links, gl, ga, frame)
        gx, gxd = model.velocities_vjp(q, qd, grad_lin=gl, grad_ang=ga, frame=frame)
        e_x, e_xd = np.abs(gx - want_q).max(), np.abs(gxd - want_qd).max()
        print(f"{name} free={free} frame={frame}: max |grad_x - reference| = {e_x:.3e} at max {np.abs(want_q).max():.3f}, "
              f"max |grad_xdot - reference| = {e_xd:.3e} at max {np.abs(want_qd).max():.3f}")
        _gate(e_x, want_q, (name, frame, "grad_x"))
        _gate(e_xd, want_qd, (name, frame, "grad_xdot"))
        for a, b in ((gl, None), (None, ga)):  # one cotangent alone
            w_q, w_qd = ref.velocity_vjp(orc, q, qd, links, a, b, frame)
            g_x, g_xd = model.velocities_vjp(q, qd, grad_lin=a, grad_ang=b, frame=frame)
            _gate(np.abs(g_x - w_q).max(), w_q, (name, frame, "grad_x, one cotangent"))
            _gate(np.abs(g_xd - w_qd).max(), w_qd, (name, frame, "grad_xdot, one cotangent"))
        # the wrench product is the Jacobian, transposed, times the wrench
        jlin, jang = model.jacobians(q, frame=frame)
        tau = model.wrenches(q, force=gl, torque=ga, frame=frame)
        err = np.abs(tau - (np.einsum("blrc,blr->bc", jlin, gl) + np.einsum("blrc,blr->bc", jang, ga))).max()
        print(f"{name} frame={frame}: max |wrenches - einsum(jacobians)| = {err:.3e}")
        assert err <= 1e-10, (name, frame)
        assert np.abs(model.wrenches(q, torque=ga, frame=frame) - np.einsum("blrc,blr->bc", jang, ga)).max() <= 1e-10
    err = np.abs(model.wrenches(q, force=gl) - model.vjp(q, grad_pos=gl)).max()
    print(f"{name}: max |wrenches(force) - link-pose vjp(grad_pos)| = {err:.3e}")
    assert err <= 1e-10, name


# ---- 2. optimizer order: mimic fold and fixed joints ------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", OPT_ORDER + ["subset"])
def test_host_float64_optimizer_order_folds_mimic_and_fixed_joints(rel, require_gpu):
    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames][:64]
    B = 33
    x, fixed = _opt_inputs(prob, B, 24)
    xd = np.random.default_rng(25).standard_normal(x.shape)
    gl, ga = _cotangents(B, len(links), 26)
    model = opt.pose_model(links)
    assert (model.n_in, model.n_fixed) == (opt.opt_dof, len(opt.idx_pin2fixed))
    # the full joint vector and its rate: target joints from x / xdot, mimic joints follow their source, fixed joints stand still
    q = prob.full_qpos(x, fixed)
    qd = np.zeros_like(q)
    qd[:, prob.idx_pin2target] = xd
    for m, s, mult in zip(prob.idx_pin2mimic, prob.idx_pin2source, prob.multipliers):
        qd[:, m] = mult * qd[:, s]
    fx = fixed if fixed.shape[1] else None
    for frame in FRAMES:
        full_q, full_qd = ref.velocity_vjp(prob.robot, q, qd, links, gl, ga, frame)
        want_x, want_xd = glp._fold(prob, full_q), glp._fold(prob, full_qd)
        gx, gxd = model.velocities_vjp(x, xd, fx, grad_lin=gl, grad_ang=ga, frame=frame)
        e_x, e_xd = np.abs(gx - want_x).max(), np.abs(gxd - want_xd).max()
        print(f"{rel} frame={frame}: max |grad_x - folded reference| = {e_x:.3e}, |grad_xdot - folded reference| = {e_xd:.3e} "
              f"({len(prob.idx_pin2mimic)} mimic joints)")
        _gate(e_x, want_x, (rel, frame, "grad_x"))
        _gate(e_xd, want_xd, (rel, frame, "grad_xdot"))
        tau = model.wrenches(x, fx, force=gl, torque=ga, frame=frame)
        _gate(np.abs(tau - want_xd).max(), want_xd, (rel, frame, "tau"))
        if len(prob.idx_pin2mimic):  # a column fed by its own joint and by mimic joints received the sum, not one share
            cols = sorted({list(prob.idx_pin2target).index(s) for s in prob.idx_pin2source})
            own = full_qd[:, prob.idx_pin2target]
            assert np.abs(want_xd[:, cols] - own[:, cols]).max() > 1e-3 and np.abs(gxd[:, cols] - own[:, cols]).max() > 1e-3, rel
    if rel == "subset":
        assert model.n_fixed == 6


# ---- 3. float32 device against the float64 host twin ------------------------------------------------------------------------------
def _member(name, kin, orc, links):
    """what pose_zoo.gates reads of a robot and a chunk of its links."""
    smap = pt.SourceMap.robot_order(kin)
    depth = max(len(kin.ancestors(kin.frames[kin.body_frame_index(n)].parent)) if kin.frames[kin.body_frame_index(n)].parent >= 0 else 0
                for n in links)
    return zoo.Member(name, kin, orc, list(links), smap, pt.compile_poses(kin, list(links), smap), depth)


def _tau_gate(g, force, torque, frame):
    s = "_local" if frame == LOCAL else ""
    return np.abs(force).sum(2) @ g["jlin" + s] + np.abs(torque).sum(2) @ g["jang" + s]


def _full_rate(smap, xdot):
    """rate of the full joint vector: joints that read x move at mult xdot[col], the others stand still."""
    qd = np.zeros((xdot.shape[0], len(smap.entries)))
    for k, (kind, col, mult, _) in enumerate(smap.entries):
        if kind == pt.SRC_X:
            qd[:, k] = mult * xdot[:, col]
    return qd


def _reference_float32_error(orc, q, qd, links, gl, ga, frame):
    """max |float32 run - float64 run| of the reference's grad_q on float32-representable inputs, and the float64 run."""
    g64, _ = ref.velocity_vjp(orc, q, qd, links, gl, ga, frame)
    f32 = lambda a: a.astype(np.float32)  # noqa: E731
    g32, _ = ref.velocity_vjp(orc, f32(q), f32(qd), links, f32(gl), f32(ga), frame, dtype=np.float32)
    assert g32.dtype == np.float32
    return float(np.abs(g32.astype(np.float64) - g64).max()), g64


def _check_device_against_host(torch, tag, model, member, x, xd, fixed, gl, ga, reach=None):
    """both entry points, both frames: finite everywhere (NaN pre-fill), tau / grad_xdot under the derived gate, grad_x under
    4 x the reference's own float32 error.  -> the printed figures."""
    if reach is None:
        reach = float(np.abs(model.poses(x, fixed, rotations=False)[0]).max())
    g = zoo.gates(member, reach)
    q_full, qd_full = zoo.full_q(member.smap, x, fixed), _full_rate(member.smap, xd)
    rows = []
    for frame in FRAMES:
        hx, hxd = model.velocities_vjp(x, xd, fixed, grad_lin=gl, grad_ang=ga, frame=frame)
        dx, dxd = dev_vjp(model, torch, x, xd, gl, ga, fixed, frame)
        tau = dev_wrenches(model, torch, x, gl, ga, fixed, frame)
        for what, a in (("grad_x", dx), ("grad_xdot", dxd), ("tau", tau)):
            assert a.shape == hx.shape and a.dtype == np.float32 and np.isfinite(a).all(), (tag, frame, what, "an entry was not written or is not finite")
        gate = _tau_gate(g, gl, ga, frame)
        e_xd, e_tau = np.abs(dxd - hxd), np.abs(tau - hxd)
        ref_err, _ = _reference_float32_error(member.orc, q_full, qd_full, member.links, gl, ga, frame)
        e_x = float(np.abs(dx - hx).max())
        ratio = float(np.max(np.where(gate > 0, e_xd / np.maximum(gate, 1e-300), 0.0)))
        print(f"{tag} frame={frame}: float32 max |grad_xdot - host| = {e_xd.max():.3e} (largest gate {gate.max():.3e}, largest error / gate "
              f"{ratio:.3f}); max |grad_x - host| = {e_x:.3e}, the reference's float32 run is {ref_err:.3e} from its float64 run "
              f"(gate {4 * ref_err:.3e}), max |grad_x| = {np.abs(hx).max():.3f}")
        rows.append((tag, frame, float(e_xd.max()), float(gate.max()), e_x, ref_err))
        assert (e_xd <= gate).all() and (e_tau <= gate).all(), (tag, frame, "grad_xdot / tau", float(e_xd.max()), float(e_tau.max()))
        assert e_x <= 4 * ref_err, (tag, frame, "grad_x", e_x, ref_err)  # (the panda gripper: two prismatic joints, 0 <= 0)
    return rows


@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_host_twin(name, require_gpu):
    torch = pytest.importorskip("torch")
    assert len(ROBOTS) == 8
    robot = RobotWrapper(ROBOTS[name])
    orc = OracleRobot(ROBOTS[name])
    B = 130
    q = _r32(_configs(robot, B, 27))
    qd = _r32(np.random.default_rng(28).standard_normal(q.shape))
    for ci, names in enumerate(glp._chunks([f.name for f in robot.kin.frames])):
        gl, ga = _cotangents(B, len(names), 29 + ci)
        _check_device_against_host(torch, f"{name}[{ci}]", robot.pose_model(names), _member(name, robot.kin, orc, names), q, qd, None, gl, ga)


# ---- 4. table limits: the synthetic robots of tests/pose_zoo.py --------------------------------------------------------------------
ZOO = ["chain64", "binary64", "binary64_slots8", "two_trees100_a", "wide_map"]
ZB = 33  # the float32 VJP form runs 16 frames per block on the 64-link members, the float64 one 8: ragged tails of 1


class ZooCase:
    def __init__(self, name, directory):
        self.m = m = zoo.build(name, directory)
        self.model = _lib.PoseModel(m.blob)
        self.x, self.fixed, self.xdot = zoo.inputs(m, ZB, 2026)
        self.gl, self.ga = _cotangents(ZB, len(m.links), 2027)
        self._f64 = self._f32 = None

    def f64(self):
        if self._f64 is None:
            o = {}
            for frame in FRAMES:
                o[f"gx {frame}"], o[f"gxd {frame}"] = self.model.velocities_vjp(self.x, self.xdot, self.fixed, self.gl, self.ga, frame)
                o[f"tau {frame}"] = self.model.wrenches(self.x, self.fixed, self.gl, self.ga, frame)
            self._f64 = o
        return self._f64

    def f32(self, torch):
        if self._f32 is None:
            o = {}
            for frame in FRAMES:
                o[f"gx {frame}"], o[f"gxd {frame}"] = dev_vjp(self.model, torch, self.x, self.xdot, self.gl, self.ga, self.fixed, frame)
                o[f"tau {frame}"] = dev_wrenches(self.model, torch, self.x, self.gl, self.ga, self.fixed, frame)
            self._f32 = o
        return self._f32


@pytest.fixture(scope="module")
def zoo_cases(tmp_path_factory):
    d, made = tmp_path_factory.mktemp("wrench_zoo"), {}

    def get(name):
        if name not in made:
            made[name] = ZooCase(name, d)
        return made[name]

    return get


@pytest.mark.parametrize("name", ZOO)
def test_table_limits_float64_and_float32(name, zoo_cases, require_gpu):
    torch = pytest.importorskip("torch")
    c = zoo_cases(name)
    m, tab = c.m, c.m.tab
    assert {k: int(tab["h"][k]) for k in ("n_joint", "n_slot", "n_in", "n_link")} == {k: zoo.FACTS[name][k] for k in ("n_joint", "n_slot", "n_in", "n_link")}
    q, qd = zoo.full_q(m.smap, c.x, c.fixed), _full_rate(m.smap, c.xdot)
    got = c.f64()
    for frame in FRAMES:
        full_q, full_qd = ref.velocity_vjp(m.orc, q, qd, m.links, c.gl, c.ga, frame)
        want_x, want_xd = zoo.fold(m.smap, full_q), zoo.fold(m.smap, full_qd)
        e_x, e_xd, e_tau = (float(np.abs(got[f"{k} {frame}"] - w).max()) for k, w in (("gx", want_x), ("gxd", want_xd), ("tau", want_xd)))
        print(f"{name} frame={frame}: float64 max |grad_x - reference| = {e_x:.3e}, |grad_xdot - reference| = {e_xd:.3e}, |tau - reference| = {e_tau:.3e}")
        _gate(e_x, want_x, (name, frame, "grad_x"))
        _gate(e_xd, want_xd, (name, frame, "grad_xdot"))
        _gate(e_tau, want_xd, (name, frame, "tau"))
        assert np.array_equal(got[f"tau {frame}"], got[f"gxd {frame}"]), (name, frame)
        if name == "wide_map":  # the column eight joints feed holds all eight shares
            shares = [mult * full_qd[:, k] for k, (kind, col, mult, _) in enumerate(m.smap.entries) if kind == pt.SRC_X and col == zoo.SHARED_COL]
            assert len(shares) == 8 and all(np.abs(s).max() > 1e-6 for s in shares)
            _gate(float(np.abs(got[f"gxd {frame}"][:, zoo.SHARED_COL] - np.sum(shares, 0)).max()), want_xd, (name, frame, "shared column"))
            for drop in range(8):  # ... and no seven of them
                less = np.sum(shares, 0) - shares[drop]
                assert np.abs(got[f"gxd {frame}"][:, zoo.SHARED_COL] - less).max() > 1e-8
    # float32: finite everywhere, the gates of test 3 (the reach of the member from its float64 poses)
    _check_device_against_host(torch, name, c.model, m, c.x, c.xdot, c.fixed, c.gl, c.ga)
    got32 = c.f32(torch)
    unread = np.flatnonzero(zoo.abs_mult(m).sum(0) == 0)
    if name == "wide_map":
        assert len(unread) == 233 and {int(u) // 64 for u in unread} == {0, 1, 2, 3}
    if name == "two_trees100_a":
        assert set(unread.tolist()) == set(range(50))
    for outs in (got, got32):
        for k, a in outs.items():
            assert np.isfinite(a).all(), (name, k)
            assert np.array_equal(a[:, unread], np.zeros_like(a[:, unread])), (name, k, "an unread column is not an exact zero")
            if not k.startswith("gx "):  # every read column takes a torque (grad_x of a root joint's column may be 0)
                read = np.setdiff1d(np.arange(a.shape[1]), unread)
                assert (np.abs(a[:, read]).max(0) > 0).all(), (name, k)


def test_slots_three_to_seven_give_the_bits_of_slots_zero_to_four(zoo_cases, require_gpu):
    torch = pytest.importorskip("torch")
    a, b = zoo_cases("binary64"), zoo_cases("binary64_slots8")
    assert int(b.m.tab["h"]["n_slot"]) == 8 and {int(s) for s in b.m.tab["joints"]["save"] if s >= 0} == {3, 4, 5, 6, 7}
    assert np.array_equal(a.x, b.x) and np.array_equal(a.gl, b.gl) and np.array_equal(a.xdot, b.xdot)
    for outs_a, outs_b, what in ((a.f64(), b.f64(), "float64"), (a.f32(torch), b.f32(torch), "float32")):
        for k in outs_a:
            assert np.array_equal(outs_a[k], outs_b[k]), (what, k)


# ---- 5. batch shapes ------------------------------------------------------------------------------------------------------------
def test_batch_shapes_null_arguments_and_the_two_entry_points_agree_bitwise(require_gpu):
    torch = pytest.importorskip("torch")
    robot = RobotWrapper(ROBOTS["shadow_hand_right"])
    links = ["thtip", "fftip", "mftip", "rftip", "lftip", "palm"]
    model = robot.pose_model(links)
    B = 130
    x = _configs(robot, B, 31).astype(np.float32)
    xd = np.random.default_rng(32).standard_normal(x.shape).astype(np.float32)
    gl, ga = (a.astype(np.float32) for a in _cotangents(B, len(links), 33))
    zero = np.zeros_like(gl)
    lib = _lib.load()
    for frame in FRAMES:
        GX, GXD = dev_vjp(model, torch, x, xd, gl, ga, frame=frame)  # B = 130: two full blocks and a ragged one
        TAU = dev_wrenches(model, torch, x, gl, ga, frame=frame)
        assert all(np.isfinite(a).all() for a in (GX, GXD, TAU))
        assert np.array_equal(GXD, TAU), (frame, "grad_xdot of the VJP entry is not the wrench product bit for bit")
        for lo, hi in ((0, 1), (0, 64), (64, 130), (129, 130)):
            gx, gxd = dev_vjp(model, torch, x[lo:hi], xd[lo:hi], gl[lo:hi], ga[lo:hi], frame=frame)
            tau = dev_wrenches(model, torch, x[lo:hi], gl[lo:hi], ga[lo:hi], frame=frame)
            assert np.array_equal(gx, GX[lo:hi]) and np.array_equal(gxd, GXD[lo:hi]) and np.array_equal(tau, TAU[lo:hi]), (frame, lo, hi)
        # one output NULL: the other keeps its bits
        only_x, none = dev_vjp(model, torch, x, xd, gl, ga, frame=frame, want_xd=False)
        assert none is None and np.array_equal(only_x, GX), frame
        none, only_xd = dev_vjp(model, torch, x, xd, gl, ga, frame=frame, want_x=False)
        assert none is None and np.array_equal(only_xd, GXD), frame
        # one input NULL: what a cotangent of zeros gives
        for a, b, za, zb in ((gl, None, gl, zero), (None, ga, zero, ga)):
            gx0, gxd0 = dev_vjp(model, torch, x, xd, za, zb, frame=frame)
            gx1, gxd1 = dev_vjp(model, torch, x, xd, a, b, frame=frame)
            assert np.array_equal(gx0, gx1) and np.array_equal(gxd0, gxd1), frame
            assert np.array_equal(dev_wrenches(model, torch, x, a, b, frame=frame), gxd1), frame
            assert not np.array_equal(gx1, GX) and not np.array_equal(gxd1, GXD)
        # B = 0: a no-op, NULL pointers and all
        assert lib.dexr_link_wrenches_dev(model.handle, 0, None, None, frame, None, None, None, None) == 0
        assert lib.dexr_link_velocities_vjp_dev(model.handle, 0, None, None, None, frame, None, None, None, None, None) == 0
        assert lib.dexr_link_wrenches(model.handle, 0, None, None, frame, None, None, None) == 0
        assert lib.dexr_link_velocities_vjp(model.handle, 0, None, None, None, frame, None, None, None, None) == 0
    z = np.zeros((0, robot.dof))
    assert model.wrenches(z, force=np.zeros((0, 6, 3))).shape == (0, robot.dof)
    g0, gd0 = model.velocities_vjp(z, z, grad_ang=np.zeros((0, 6, 3)))
    assert g0.shape == gd0.shape == (0, robot.dof)


# ---- 6. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    robot = RobotWrapper(ROBOTS["allegro_hand_right"])
    model = robot.pose_model(["link_15.0_tip", "link_3.0_tip"])
    B = 4
    x = torch.zeros((B, robot.dof), dtype=torch.float32, device="cuda")
    g = torch.zeros((B, 2, 3), dtype=torch.float32, device="cuda")
    out, out2 = _nan(torch, (B, robot.dof)), _nan(torch, (B, robot.dof))
    h, xp, gp, op, op2 = model.handle, x.data_ptr(), g.data_ptr(), out.data_ptr(), out2.data_ptr()
    INVALID = -1

    def invalid(rc, word=None):
        assert rc == INVALID
        msg = lib.dexr_last_error()
        assert len(msg) > 0 and (word is None or word in msg), msg

    wr, vj = lib.dexr_link_wrenches_dev, lib.dexr_link_velocities_vjp_dev
    invalid(wr(None, B, xp, None, WORLD, gp, gp, op, None), b"null pose model")
    invalid(vj(None, B, xp, None, xp, WORLD, gp, gp, op, op2, None), b"null pose model")
    invalid(wr(h, -1, xp, None, WORLD, gp, gp, op, None), b"negative")
    invalid(vj(h, -1, xp, None, xp, WORLD, gp, gp, op, op2, None), b"negative")
    invalid(wr(h, B, xp, None, 2, gp, gp, op, None), b"frame")
    invalid(vj(h, B, xp, None, xp, -1, gp, gp, op, op2, None), b"frame")
    invalid(wr(h, B, xp, None, WORLD, None, None, op, None), b"input are both NULL")
    invalid(vj(h, B, xp, None, xp, WORLD, None, None, op, op2, None), b"input are both NULL")
    invalid(wr(h, B, xp, None, WORLD, gp, gp, None, None), b"output is NULL")
    invalid(vj(h, B, xp, None, xp, WORLD, gp, gp, None, None, None), b"output is NULL")
    invalid(wr(h, B, None, None, WORLD, gp, gp, op, None), b"x is NULL")
    invalid(vj(h, B, None, None, xp, WORLD, gp, gp, op, op2, None), b"x is NULL")
    invalid(vj(h, B, xp, None, None, WORLD, gp, gp, op, op2, None), b"xdot")
    invalid(vj(h, B, xp, None, None, LOCAL, gp, None, op, None, None), b"xdot")
    # a table that reads fixed columns
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.pose_model(("link_15.0_tip", "link_3.0_tip"))
    assert ms.n_fixed == 6 and ms.n_in == 10
    invalid(wr(ms.handle, B, xp, None, WORLD, gp, gp, op, None), b"fixed")
    invalid(vj(ms.handle, B, xp, None, xp, WORLD, gp, gp, op, op2, None), b"fixed")
    # the host twins keep the same rules
    z = np.zeros((B, robot.dof))
    zg = np.zeros((B, 2, 3))
    zp, zgp = (a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)) for a in (z, zg))
    invalid(lib.dexr_link_wrenches(h, B, zp, None, WORLD, None, None, zp), b"input are both NULL")
    invalid(lib.dexr_link_wrenches(h, B, zp, None, 7, zgp, None, zp), b"frame")
    invalid(lib.dexr_link_wrenches(h, B, zp, None, WORLD, zgp, None, None), b"output is NULL")
    invalid(lib.dexr_link_velocities_vjp(h, B, zp, None, zp, WORLD, zgp, None, None, None), b"output is NULL")
    invalid(lib.dexr_link_velocities_vjp(h, B, zp, None, None, WORLD, zgp, None, zp, None), b"xdot")
    invalid(lib.dexr_link_velocities_vjp(None, B, zp, None, zp, WORLD, zgp, None, zp, None), b"null pose model")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(out2).all())  # nothing was launched
    with pytest.raises(ValueError, match="shape"):
        model.wrenches(z, force=np.zeros((B, 3, 3)))
    with pytest.raises(ValueError, match="shape"):
        model.velocities_vjp(z, z[:, :3], grad_lin=zg)


# ---- 7. torch front ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_torch_front_equals_the_entry_points_bitwise(rel, require_gpu, monkeypatch):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag
    from dex_retargeting_amd import jacobians as jac

    opt, prob = _optimizer_and_problem(rel)
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_11.0_tip"]
    B = 130
    x, fixed = _opt_inputs(prob, B, 34)
    gen = torch.Generator("cuda").manual_seed(6)
    f = torch.tensor(fixed.astype(np.float32), device="cuda") if fixed.shape[1] else None
    fp = _ptr(f)
    gl, ga = (torch.randn((B, 4, 3), device="cuda", generator=gen) for _ in range(2))
    qd0 = torch.randn((B, opt.opt_dof), device="cuda", generator=gen)
    model = opt.pose_model(tips)
    sp = torch.cuda.current_stream().cuda_stream
    asked = []  # (grad_x pointer, grad_xdot pointer) of every VJP launch
    real = _lib.PoseModel.velocities_vjp_dev

    def spy(self, B_, x_ptr, fixed_ptr, xdot_ptr, gl_ptr, ga_ptr, gx_ptr, gxd_ptr, **kw):
        asked.append((gl_ptr, ga_ptr, gx_ptr, gxd_ptr))
        return real(self, B_, x_ptr, fixed_ptr, xdot_ptr, gl_ptr, ga_ptr, gx_ptr, gxd_ptr, **kw)

    monkeypatch.setattr(_lib.PoseModel, "velocities_vjp_dev", spy)
    for frame, fid in (("world", WORLD), ("local", LOCAL)):
        q = torch.tensor(x.astype(np.float32), device="cuda", requires_grad=True)
        qd = qd0.clone().requires_grad_(True)
        lin, ang = ag.link_velocities(opt, q, qd, tips, f, frame=frame)
        wl, wa = jac.link_velocities(opt, q, qd, tips, f, frame=frame)
        assert torch.equal(lin, wl) and torch.equal(ang, wa) and lin.requires_grad and ang.requires_grad and not wl.requires_grad
        ((lin * gl).sum() + (ang * ga).sum()).backward()
        wx, wxd = _nan(torch, q.shape), _nan(torch, q.shape)
        real(model, B, q.detach().data_ptr(), fp, qd.detach().data_ptr(), gl.data_ptr(), ga.data_ptr(), wx.data_ptr(), wxd.data_ptr(),
             frame=fid, stream=sp)
        assert torch.equal(q.grad, wx) and torch.equal(qd.grad, wxd) and bool(torch.isfinite(q.grad).all())
        assert asked and all(p != 0 for p in asked[-1])
        # a loss that uses `ang` alone: grad_lin arrives as NULL; angular=False: one output
        q2, qd2 = q.detach().clone().requires_grad_(True), qd.detach().clone().requires_grad_(True)
        (ag.link_velocities(opt, q2, qd2, tips, f, frame=frame)[1] * ga).sum().backward()
        assert asked[-1][0] == 0 and asked[-1][1] != 0
        real(model, B, q.detach().data_ptr(), fp, qd.detach().data_ptr(), 0, ga.data_ptr(), wx.data_ptr(), wxd.data_ptr(), frame=fid, stream=sp)
        assert torch.equal(q2.grad, wx) and torch.equal(qd2.grad, wxd)
        q3, qd3 = q.detach().clone().requires_grad_(True), qd.detach().clone().requires_grad_(True)
        lin3, none = ag.link_velocities(opt, q3, qd3, tips, f, frame=frame, angular=False)
        assert none is None and torch.equal(lin3, wl)
        (lin3 * gl).sum().backward()
        assert asked[-1][0] != 0 and asked[-1][1] == 0
        real(model, B, q.detach().data_ptr(), fp, qd.detach().data_ptr(), gl.data_ptr(), 0, wx.data_ptr(), wxd.data_ptr(), frame=fid, stream=sp)
        assert torch.equal(q3.grad, wx) and torch.equal(qd3.grad, wxd)
        # qdot without a gradient: no grad_xdot buffer is asked for (and the other way round)
        q4 = q.detach().clone().requires_grad_(True)
        (ag.link_velocities(opt, q4, qd.detach(), tips, f, frame=frame)[0] * gl).sum().backward()
        assert asked[-1][2] != 0 and asked[-1][3] == 0 and torch.equal(q4.grad, q3.grad)
        qd5 = qd.detach().clone().requires_grad_(True)
        (ag.link_velocities(opt, q.detach(), qd5, tips, f, frame=frame)[0] * gl).sum().backward()
        assert asked[-1][2] == 0 and asked[-1][3] != 0 and torch.equal(qd5.grad, qd3.grad)
        # the wrench product of the torch front
        tau = jac.link_wrenches(opt, q, tips, gl, ga, f, frame=frame)
        wt = _nan(torch, q.shape)
        model.wrenches_dev(B, q.detach().data_ptr(), fp, gl.data_ptr(), ga.data_ptr(), wt.data_ptr(), frame=fid, stream=sp)
        assert torch.equal(tau, wt) and torch.equal(tau, qd.grad) and not tau.requires_grad
        model.wrenches_dev(B, q.detach().data_ptr(), fp, 0, ga.data_ptr(), wt.data_ptr(), frame=fid, stream=sp)
        assert torch.equal(jac.link_wrenches(opt, q, tips, torque=ga, fixed_qpos=f, frame=frame), wt)
    e = torch.zeros((0, opt.opt_dof), device="cuda")
    assert jac.link_wrenches(opt, e, tips, force=gl[:0], fixed_qpos=None if f is None else f[:0]).shape == (0, opt.opt_dof)


def test_torch_front_chunks_more_than_sixty_four_links(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag
    from dex_retargeting_amd import jacobians as jac

    robot = RobotWrapper(ROBOTS["shadow_hand_right"])
    names = [f.name for f in robot.kin.frames]
    many = (names * 4)[:70]
    B = 5
    q = torch.tensor(_configs(robot, B, 35).astype(np.float32), device="cuda", requires_grad=True)
    gen = torch.Generator("cuda").manual_seed(7)
    qd = torch.randn(q.shape, device="cuda", generator=gen).requires_grad_(True)
    gl, ga = (torch.randn((B, 70, 3), device="cuda", generator=gen) for _ in range(2))
    lin, ang = ag.robot_link_velocities(robot, q, qd, many, frame="local")
    wl, wa = jac.robot_link_velocities(robot, q, qd, many, frame="local")
    assert lin.shape == ang.shape == (B, 70, 3) and torch.equal(lin, wl) and torch.equal(ang, wa)
    ((lin * gl).sum() + (ang * ga).sum()).backward()
    sp = torch.cuda.current_stream().cuda_stream
    parts = []
    for lo, hi in ((0, 64), (64, 70)):
        m = robot.pose_model(many[lo:hi])
        a, b, t = _nan(torch, q.shape), _nan(torch, q.shape), _nan(torch, q.shape)
        cl, ca = gl[:, lo:hi].contiguous(), ga[:, lo:hi].contiguous()
        m.velocities_vjp_dev(B, q.detach().data_ptr(), 0, qd.detach().data_ptr(), cl.data_ptr(), ca.data_ptr(), a.data_ptr(), b.data_ptr(),
                             frame=LOCAL, stream=sp)
        m.wrenches_dev(B, q.detach().data_ptr(), 0, cl.data_ptr(), ca.data_ptr(), t.data_ptr(), frame=LOCAL, stream=sp)
        parts.append((a, b, t))
    assert torch.equal(q.grad, parts[0][0] + parts[1][0]) and torch.equal(qd.grad, parts[0][1] + parts[1][1])
    tau = jac.robot_link_wrenches(robot, q, many, gl, ga, frame="local")
    assert tau.shape == q.shape and torch.equal(tau, parts[0][2] + parts[1][2]) and not tau.requires_grad


def test_keypoints_to_link_velocity_loss_end_to_end(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    rel = "teleop/allegro_hand_right.yml"
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    B = 8
    d = cases.human_set(prob, B)
    kp = glp._t(d["kp"], torch, dtype=torch.float32, requires_grad=True)
    last = glp._t(d["last"], torch)
    q = ag.retarget(opt, ag.ref_value_from_keypoints(opt, kp), last)
    qdot = (q - last) * 30.0  # the rate between two frames of a 30 Hz track
    lin, ang = ag.link_velocities(opt, q, qdot, list(prob.computed_links))
    ((lin ** 2).sum() + 1e-2 * (ang ** 2).sum()).backward()
    assert bool(torch.isfinite(kp.grad).all()) and float(kp.grad.abs().max()) > 0

"""GPU tests of the link-Jacobian and link-velocity kernels (csrc/dexr_pose.hip, include/dexr_jacobian.h): the float64 host
entry points against the oracle's closed forms (robot order and optimizer order with the mimic fold and fixed joints),
consistency with the link-pose VJP, the float32 device entry points against the oracle at the float32-rounded inputs, zero
columns and base links, batch shapes, the raw ABI's argument errors and the torch front.

Gates of the float32 tests (none is a measured figure).  The pose tests cap position and rotation-entry error at 1e-5; an
entry of a x (p - o) then errs by at most |da| |p - o| + |dp| + |do| <= 1.7e-5 * 1.2 m + 2e-5 = 4e-5 and an entry of a by
1.7e-5 (2e-5 is asked); a velocity is a sum of n_in such entries times xdot.  Measured on the MI355X: see
docs/experiments/link_jacobians.md."""
import os

import numpy as np
import pytest

import test_gpu_link_poses as glp
from dex_retargeting_amd import _lib
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from oracle import cases
from oracle.kin import OracleRobot
from oracle.objectives import OracleProblem
from test_jacobian_host import SUBSET, SUBSET_CFG

pytestmark = pytest.mark.gpu
ROBOTS = glp.ROBOTS
WORLD, LOCAL = _lib.JAC_WORLD_ALIGNED, _lib.JAC_LOCAL
OPT_ORDER = ["offline/schunk_svh_hand_right.yml", "teleop/schunk_svh_hand_right.yml", "teleop/ability_hand_right.yml",
             "offline/inspire_hand_right.yml", "teleop/inspire_hand_right_dexpilot.yml", "offline/shadow_hand_right.yml",
             "teleop/allegro_hand_right.yml"]  # the configs of test_host_float64_vjp_optimizer_order_folds_mimic_joints


def oracle_jacobians(orc, q, links):
    """World-aligned (jlin, jang) (B, L, 3, dof) and the link rotations (B, L, 3, 3) from OracleRobot._walk, float64:
    jlin is OracleRobot.point_jacobians, jang the world axes of the revolute joints on the chain."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    jlin = orc.point_jacobians(q, links)
    jang = np.zeros_like(jlin)
    Rs = []
    for li, name in enumerate(links):
        R, _, info = orc._walk(q, name)
        Rs.append(R)
        for qi, typ, a_w, _ in info:
            if typ == "revolute":
                jang[:, li, :, qi] = a_w
    return jlin, jang, np.stack(Rs, 1)


def to_local(R, J):
    """R_l^T applied to the row axis of (B, L, 3, n) or to (B, L, 3)."""
    return np.einsum("blji,blj...->bli...", R, J)


def _configs(robot, B, seed):
    lim = robot.joint_limits
    return np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (B, robot.dof))


def _gate(err, want, what):
    scale = max(1.0, float(np.abs(want).max()))
    assert err <= 1e-10 * scale, (what, err, scale)


# ---- 1. float64 host twin, robot order -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_host_float64_jacobians_robot_order(name, require_gpu):
    for free in (False, True):
        robot = RobotWrapper(ROBOTS[name], add_dummy_free_joints=free)
        orc = OracleRobot(ROBOTS[name], free)
        links = [f.name for f in robot.kin.frames][:64]
        q = _configs(robot, 33, 7)
        model = robot.pose_model(links)
        jlin, jang = model.jacobians(q)
        wl, wa, R = oracle_jacobians(orc, q, links)
        e_lin, e_ang = np.abs(jlin - wl).max(), np.abs(jang - wa).max()
        print(f"{name} free={free}: world max |jlin - oracle| = {e_lin:.3e}, |jang - oracle| = {e_ang:.3e}, max |J| = {np.abs(wl).max():.3f}")
        _gate(e_lin, wl, (name, free, "jlin"))
        _gate(e_ang, wa, (name, free, "jang"))
        only_lin, none = model.jacobians(q, angular=False)
        assert none is None and np.array_equal(only_lin, jlin)
        # local frame, row by row against frame_jacobian_local, 3 configurations
        ll, la = model.jacobians(q[:3], frame=LOCAL)
        ids = [robot.get_link_index(n) for n in links]
        batched = robot.link_jacobians(q[:3], ids, local=True)
        assert batched.shape == (3, len(links), 6, robot.dof)
        assert np.array_equal(batched[:, :, :3], ll) and np.array_equal(batched[:, :, 3:], la)
        worst = single = 0.0
        for b in range(3):
            for li, ln in enumerate(links):
                want = orc.frame_jacobian_local(q[b], ln)
                for r in range(3):
                    worst = max(worst, np.abs(ll[b, li, r] - want[r]).max(), np.abs(la[b, li, r] - want[3 + r]).max())
                single = max(single, np.abs(batched[b, li] - robot.compute_single_link_local_jacobian(q[b], ids[li])).max())
        print(f"{name} free={free}: local max |J - frame_jacobian_local| = {worst:.3e}, |batched - single link| = {single:.3e}")
        _gate(worst, wl, (name, free, "local"))
        assert single <= 1e-10, (name, free)
        world6 = robot.link_jacobians(q[:3], ids, local=False)
        assert np.array_equal(world6[:, :, :3], jlin[:3]) and np.array_equal(world6[:, :, 3:], jang[:3])


# ---- 2. optimizer order: mimic fold and fixed joints ---------------------------------------------------------------------------
def _optimizer_and_problem(rel):
    if rel == "subset":  # target_joint_names = a subset of the joints: the rest arrive through `fixed`
        opt = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
        robot = OracleRobot(os.path.join(cases.URDF_DIR, SUBSET_CFG["urdf_path"]))
        prob = OracleProblem(robot, "vector", SUBSET, target_origin_link_names=SUBSET_CFG["target_origin_link_names"],
                             target_task_link_names=SUBSET_CFG["target_task_link_names"], scaling=1.6)
        return opt, prob
    return RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer, cases.problem_from_config(rel)


def _fold4(prob, J):
    """(B, L, 3, dof) in the full qpos -> (B, L, 3, n_opt): glp._fold, the chain rule of full_qpos, column by column."""
    return glp._fold(prob, J.reshape(-1, J.shape[-1])).reshape(J.shape[:-1] + (len(prob.idx_pin2target),))


def _opt_inputs(prob, B, seed):
    rng = np.random.default_rng(seed)
    lim = prob.robot.joint_limits
    x = rng.uniform(lim[prob.idx_pin2target, 0], lim[prob.idx_pin2target, 1], (B, len(prob.idx_pin2target)))
    fixed = rng.uniform(lim[prob.idx_pin2fixed, 0], lim[prob.idx_pin2fixed, 1], (B, len(prob.idx_pin2fixed)))
    return x, fixed


@pytest.mark.parametrize("rel", OPT_ORDER + ["subset"])
def test_host_float64_jacobians_optimizer_order_fold_mimic_and_fixed_joints(rel, require_gpu):
    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames][:64]
    x, fixed = _opt_inputs(prob, 33, 8)
    model = opt.pose_model(links)
    assert (model.n_in, model.n_fixed) == (opt.opt_dof, len(opt.idx_pin2fixed))
    if rel == "subset":
        assert model.n_fixed == 6
    wl, wa, _ = oracle_jacobians(prob.robot, prob.full_qpos(x, fixed), links)
    wl, wa = _fold4(prob, wl), _fold4(prob, wa)
    jlin, jang = model.jacobians(x, fixed)
    e_lin, e_ang = np.abs(jlin - wl).max(), np.abs(jang - wa).max()
    print(f"{rel}: max |jlin - folded oracle| = {e_lin:.3e}, |jang - folded oracle| = {e_ang:.3e} ({len(prob.idx_pin2mimic)} mimic joints)")
    assert e_lin <= 1e-10 and e_ang <= 1e-10, rel


# ---- 3. consistency with the link-pose VJP -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/shadow_hand_right_dexpilot.yml", "offline/schunk_svh_hand_right.yml"])
def test_host_float64_jacobian_contracted_equals_the_vjp(rel, require_gpu):
    opt, prob = _optimizer_and_problem(rel)
    links = list(prob.computed_links)
    x, fixed = _opt_inputs(prob, 33, 9)
    model = opt.pose_model(links)
    g = np.random.default_rng(10).standard_normal((33, len(links), 3))
    jlin, _ = model.jacobians(x, fixed, angular=False)
    got = np.einsum("blrc,blr->bc", jlin, g)
    want = model.vjp(x, fixed, grad_pos=g)
    err = np.abs(got - want).max()
    print(f"{rel}: max |einsum(jlin, g) - vjp| = {err:.3e}")
    assert err <= 1e-10, rel


# ---- 4. velocities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,free", [("shadow_hand_right", True), ("panda_gripper_glb", False), ("arm_shadow_hand_right", False)])
def test_host_float64_velocities_equal_jacobian_times_rate(name, free, require_gpu):
    robot = RobotWrapper(ROBOTS[name], add_dummy_free_joints=free)
    orc = OracleRobot(ROBOTS[name], free)
    links = [f.name for f in robot.kin.frames][:64]
    q = _configs(robot, 33, 11)
    qd = np.random.default_rng(12).standard_normal(q.shape)
    wl, wa, R = oracle_jacobians(orc, q, links)
    vl, va = np.einsum("blrc,bc->blr", wl, qd), np.einsum("blrc,bc->blr", wa, qd)
    model = robot.pose_model(links)
    for frame, want_l, want_a in ((WORLD, vl, va), (LOCAL, to_local(R, vl), to_local(R, va))):
        lin, ang = model.velocities(q, qd, frame=frame)
        e_l, e_a = np.abs(lin - want_l).max(), np.abs(ang - want_a).max()
        print(f"{name} free={free} frame={frame}: max |lin - J qd| = {e_l:.3e}, |ang - J qd| = {e_a:.3e}, max |v| = {np.abs(want_l).max():.3f}")
        _gate(e_l, want_l, (name, frame, "lin"))
        _gate(e_a, want_a, (name, frame, "ang"))
        only, none = model.velocities(q, qd, frame=frame, angular=False)
        assert none is None and np.array_equal(only, lin)


# ---- 5. float32 device entry points ------------------------------------------------------------------------------------------
def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def dev_jacobians(model, torch, x32, fixed32=None, frame=WORLD, lin=True, ang=True, stream=None):
    """dexr_link_jacobians_dev on torch tensors, outputs pre-filled with NaN -> numpy (jlin or None, jang or None)."""
    B = x32.shape[0]
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        x = torch.tensor(x32, device="cuda")
        f = None if fixed32 is None else torch.tensor(fixed32, device="cuda")
        shape = (B, model.n_link, 3, model.n_in)
        jl = _nan(torch, shape) if lin else None
        ja = _nan(torch, shape) if ang else None
        model.jacobians_dev(B, x.data_ptr(), 0 if f is None else f.data_ptr(), 0 if jl is None else jl.data_ptr(),
                            0 if ja is None else ja.data_ptr(), frame=frame, stream=st.cuda_stream)
    st.synchronize()
    return (None if jl is None else jl.cpu().numpy()), (None if ja is None else ja.cpu().numpy())


def dev_velocities(model, torch, x32, xd32, fixed32=None, frame=WORLD, lin=True, ang=True, stream=None):
    B = x32.shape[0]
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        x, xd = torch.tensor(x32, device="cuda"), torch.tensor(xd32, device="cuda")
        f = None if fixed32 is None else torch.tensor(fixed32, device="cuda")
        vl = _nan(torch, (B, model.n_link, 3)) if lin else None
        va = _nan(torch, (B, model.n_link, 3)) if ang else None
        model.velocities_dev(B, x.data_ptr(), 0 if f is None else f.data_ptr(), xd.data_ptr(), 0 if vl is None else vl.data_ptr(),
                             0 if va is None else va.data_ptr(), frame=frame, stream=st.cuda_stream)
    st.synchronize()
    return (None if vl is None else vl.cpu().numpy()), (None if va is None else va.cpu().numpy())


@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_oracle(name, require_gpu):
    torch = pytest.importorskip("torch")
    assert len(ROBOTS) == 8
    robot = RobotWrapper(ROBOTS[name])
    orc = OracleRobot(ROBOTS[name])
    links = [f.name for f in robot.kin.frames]
    B = 512
    q32 = _configs(robot, B, 2024).astype(np.float32)
    qd32 = np.random.default_rng(2025).standard_normal(q32.shape).astype(np.float32)
    q64, qd64 = q32.astype(np.float64), qd32.astype(np.float64)  # the oracle sees exactly what the kernel sees
    stream = torch.cuda.Stream()
    e = dict(jlin=0.0, jang=0.0, lin=0.0, ang=0.0)
    for names in glp._chunks(links):
        model = robot.pose_model(names)
        wl, wa, R = oracle_jacobians(orc, q64, names)
        vl, va = np.einsum("blrc,bc->blr", wl, qd64), np.einsum("blrc,bc->blr", wa, qd64)
        for frame in (WORLD, LOCAL):
            want = (wl, wa, vl, va) if frame == WORLD else tuple(to_local(R, a) for a in (wl, wa, vl, va))
            jl, ja = dev_jacobians(model, torch, q32, frame=frame, stream=stream)
            lin, ang = dev_velocities(model, torch, q32, qd32, frame=frame, stream=stream)
            for k, got, w in zip(("jlin", "jang", "lin", "ang"), (jl, ja, lin, ang), want):
                assert got.shape == w.shape and np.isfinite(got).all(), (name, k, frame, "an entry was not written or is not finite")
                e[k] = max(e[k], float(np.abs(got - w).max()))
    vscale = max(1.0, float(np.abs(qd32).max()) * robot.dof)
    print(f"{name}: float32 device max |jlin err| = {e['jlin']:.3e}, |jang err| = {e['jang']:.3e}, |lin err| = {e['lin']:.3e}, "
          f"|ang err| = {e['ang']:.3e} (velocity gate {4e-5 * vscale:.3e})")
    assert e["jlin"] <= 4e-5 and e["jang"] <= 2e-5, (name, e)
    assert e["lin"] <= 4e-5 * vscale and e["ang"] <= 4e-5 * vscale, (name, e, vscale)


# ---- 6. zero columns and base links --------------------------------------------------------------------------------------------
def test_columns_of_other_fingers_are_exact_zeros(require_gpu):
    torch = pytest.importorskip("torch")
    opt, prob = _optimizer_and_problem("teleop/shadow_hand_right_dexpilot.yml")
    x, fixed = _opt_inputs(prob, 130, 14)
    model = opt.pose_model(["thtip"])
    wl, wa, _ = oracle_jacobians(prob.robot, prob.full_qpos(x, fixed), ["thtip"])
    wl, wa = _fold4(prob, wl), _fold4(prob, wa)
    other = [c for c, n in enumerate(opt.target_joint_names) if n[:2] in ("FF", "MF", "RF", "LF")]
    assert len(other) >= 13 and not np.abs(wl[..., other]).any() and not np.abs(wa[..., other]).any()
    moving = [c for c in range(opt.opt_dof) if c not in other]
    assert np.abs(wl[..., moving]).max() > 1e-3
    j64l, j64a = model.jacobians(x, fixed)
    fx = fixed.astype(np.float32) if fixed.shape[1] else None
    j32l, j32a = dev_jacobians(model, torch, x.astype(np.float32), fx)
    for J in (j64l, j64a, j32l, j32a):
        assert np.array_equal(J[..., other], np.zeros_like(J[..., other]))  # exact 0.0, written by the kernel (NaN pre-fill)
        assert np.isfinite(J).all()
    assert np.abs(j64l - wl).max() <= 1e-10 and np.abs(j32l - wl).max() <= 4e-5 and np.abs(j32a - wa).max() <= 2e-5


def test_base_link_one_link_and_sixty_four_links_of_the_arm_and_hand_model(require_gpu):
    torch = pytest.importorskip("torch")
    name = "arm_shadow_hand_right"
    robot = RobotWrapper(ROBOTS[name])
    orc = OracleRobot(ROBOTS[name])
    names = [f.name for f in robot.kin.frames]
    base = names[0]
    assert robot.kin.frames[0].parent == -1 and len(names) >= 30
    B = 130
    q = _configs(robot, B, 15)
    q32 = q.astype(np.float32)
    qd = np.random.default_rng(16).standard_normal(q.shape)
    for links in ([base], [names[-1]], (names * 3)[:64], [names[-1], base, names[5]]):
        model = robot.pose_model(links)
        wl, wa, R = oracle_jacobians(orc, q, links)
        for frame in (WORLD, LOCAL):  # (float64, 64 links: the block shrinks below 64 lanes, more so in the local frame)
            tl, ta = (wl, wa) if frame == WORLD else (to_local(R, wl), to_local(R, wa))
            jl, ja = model.jacobians(q, frame=frame)
            _gate(np.abs(jl - tl).max(), tl, (len(links), frame, "f64 jlin"))
            _gate(np.abs(ja - ta).max(), ta, (len(links), frame, "f64 jang"))
            lin, ang = model.velocities(q, qd, frame=frame)
            _gate(np.abs(lin - np.einsum("blrc,bc->blr", tl, qd)).max(), tl, (len(links), frame, "f64 lin"))
            _gate(np.abs(ang - np.einsum("blrc,bc->blr", ta, qd)).max(), ta, (len(links), frame, "f64 ang"))
            w32l, w32a, R32 = oracle_jacobians(orc, q32.astype(np.float64), links)
            if frame == LOCAL:
                w32l, w32a = to_local(R32, w32l), to_local(R32, w32a)
            dl, da = dev_jacobians(model, torch, q32, frame=frame)
            assert np.abs(dl - w32l).max() <= 4e-5 and np.abs(da - w32a).max() <= 2e-5, (len(links), frame)
            vl32, va32 = dev_velocities(model, torch, q32, qd.astype(np.float32), frame=frame)
            for li, ln in enumerate(links):
                if ln == base:  # a link on the fixed base: an all-zero Jacobian row and no velocity, exactly
                    for a in (jl, ja, dl, da, lin, ang, vl32, va32):
                        assert np.array_equal(a[:, li], np.zeros_like(a[:, li])), (len(links), frame)
    # more than 64 links through the wrapper: chunked
    ids = [robot.get_link_index(n) for n in (names * 4)[:70]]
    J = robot.link_jacobians(q[:3], ids, local=False)
    wl, wa, _ = oracle_jacobians(orc, q[:3], (names * 4)[:70])
    assert J.shape == (3, 70, 6, robot.dof) and np.abs(J[:, :, :3] - wl).max() <= 1e-10 and np.abs(J[:, :, 3:] - wa).max() <= 1e-10


# ---- 7. batch shapes -----------------------------------------------------------------------------------------------------------
def test_batch_shapes_are_row_independent(require_gpu):
    torch = pytest.importorskip("torch")
    robot = RobotWrapper(ROBOTS["shadow_hand_right"])
    links = ["thtip", "fftip", "mftip", "rftip", "lftip", "palm"]
    model = robot.pose_model(links)
    x = _configs(robot, 130, 17).astype(np.float32)
    xd = np.random.default_rng(18).standard_normal(x.shape).astype(np.float32)
    lib = _lib.load()
    for frame in (WORLD, LOCAL):
        JL, JA = dev_jacobians(model, torch, x, frame=frame)  # B = 130: two full blocks and a ragged one
        VL, VA = dev_velocities(model, torch, x, xd, frame=frame)
        assert all(np.isfinite(a).all() for a in (JL, JA, VL, VA))
        for lo, hi in ((0, 1), (0, 64), (64, 130), (129, 130)):  # B = 1; 64 + 66: the same rows at another place of another batch
            jl, ja = dev_jacobians(model, torch, x[lo:hi], frame=frame)
            vl, va = dev_velocities(model, torch, x[lo:hi], xd[lo:hi], frame=frame)
            assert np.array_equal(jl, JL[lo:hi]) and np.array_equal(ja, JA[lo:hi]), (frame, lo, hi)
            assert np.array_equal(vl, VL[lo:hi]) and np.array_equal(va, VA[lo:hi]), (frame, lo, hi)
        # one output NULL: the other keeps its bits
        assert np.array_equal(dev_jacobians(model, torch, x, frame=frame, ang=False)[0], JL)
        assert np.array_equal(dev_jacobians(model, torch, x, frame=frame, lin=False)[1], JA)
        assert np.array_equal(dev_velocities(model, torch, x, xd, frame=frame, ang=False)[0], VL)
        assert np.array_equal(dev_velocities(model, torch, x, xd, frame=frame, lin=False)[1], VA)
        # B = 0: a no-op, NULL pointers and all
        assert lib.dexr_link_jacobians_dev(model.handle, 0, None, None, frame, None, None, None) == 0
        assert lib.dexr_link_velocities_dev(model.handle, 0, None, None, None, frame, None, None, None) == 0
        assert lib.dexr_link_jacobians(model.handle, 0, None, None, frame, None, None) == 0
        assert lib.dexr_link_velocities(model.handle, 0, None, None, None, frame, None, None) == 0
    j0, a0 = model.jacobians(np.zeros((0, robot.dof)))
    assert j0.shape == a0.shape == (0, 6, 3, robot.dof)
    v0, w0 = model.velocities(np.zeros((0, robot.dof)), np.zeros((0, robot.dof)))
    assert v0.shape == w0.shape == (0, 6, 3)


# ---- 8. argument errors through the raw ABI ------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    robot = RobotWrapper(ROBOTS["allegro_hand_right"])
    model = robot.pose_model(["link_15.0_tip", "link_3.0_tip"])
    B = 4
    x = torch.zeros((B, robot.dof), dtype=torch.float32, device="cuda")
    out = _nan(torch, (B, 2, 3, robot.dof))
    v = _nan(torch, (B, 2, 3))
    h, xp, op, vp = model.handle, x.data_ptr(), out.data_ptr(), v.data_ptr()
    INVALID = -1
    assert lib.dexr_link_jacobians_dev(h, B, xp, None, WORLD, None, None, None) == INVALID
    assert b"both NULL" in lib.dexr_last_error()
    assert lib.dexr_link_velocities_dev(h, B, xp, None, xp, WORLD, None, None, None) == INVALID
    assert lib.dexr_link_jacobians_dev(h, B, xp, None, 2, op, None, None) == INVALID
    assert b"frame" in lib.dexr_last_error()
    assert lib.dexr_link_velocities_dev(h, B, xp, None, xp, -1, vp, None, None) == INVALID
    assert lib.dexr_link_jacobians_dev(None, B, xp, None, WORLD, op, None, None) == INVALID
    assert lib.dexr_link_velocities_dev(None, B, xp, None, xp, WORLD, vp, None, None) == INVALID
    assert lib.dexr_link_velocities_dev(h, B, xp, None, None, WORLD, vp, None, None) == INVALID
    assert b"xdot" in lib.dexr_last_error()
    assert lib.dexr_link_jacobians_dev(h, B, None, None, WORLD, op, None, None) == INVALID
    assert lib.dexr_link_jacobians_dev(h, -1, xp, None, WORLD, op, None, None) == INVALID
    # a table that reads fixed columns
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.pose_model(("link_15.0_tip",))
    assert ms.n_fixed == 6 and ms.n_in == 10
    assert lib.dexr_link_jacobians_dev(ms.handle, B, xp, None, WORLD, op, None, None) == INVALID
    assert b"fixed" in lib.dexr_last_error()
    assert lib.dexr_link_velocities_dev(ms.handle, B, xp, None, xp, WORLD, vp, None, None) == INVALID
    # the host twins keep the same rules
    z = np.zeros((B, robot.dof))
    zp = z.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    assert lib.dexr_link_jacobians(h, B, zp, None, WORLD, None, None) == INVALID
    assert lib.dexr_link_jacobians(h, B, zp, None, 7, zp, None) == INVALID
    assert lib.dexr_link_velocities(h, B, zp, None, None, WORLD, zp, None) == INVALID
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(v).all())  # nothing was launched


# ---- 9. torch front ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_torch_front_equals_the_entry_points_bitwise(rel, require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import jacobians as jac

    opt, prob = _optimizer_and_problem(rel)
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_11.0_tip"]
    B = 300
    x, fixed = _opt_inputs(prob, B, 19)
    q = torch.tensor(x.astype(np.float32), device="cuda", requires_grad=True)
    qd = torch.randn(q.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    f = torch.tensor(fixed.astype(np.float32), device="cuda") if fixed.shape[1] else None
    fp = 0 if f is None else f.data_ptr()
    model = opt.pose_model(tips)
    sp = torch.cuda.current_stream().cuda_stream
    for frame, fid in (("world", WORLD), ("local", LOCAL)):
        wl, wa = _nan(torch, (B, 4, 3, opt.opt_dof)), _nan(torch, (B, 4, 3, opt.opt_dof))
        model.jacobians_dev(B, q.detach().data_ptr(), fp, wl.data_ptr(), wa.data_ptr(), frame=fid, stream=sp)
        jl, ja = jac.link_jacobians(opt, q, tips, f, frame=frame)
        assert torch.equal(jl, wl) and torch.equal(ja, wa) and not jl.requires_grad and not ja.requires_grad
        jl2, none = jac.link_jacobians(opt, q, tips, f, frame=frame, angular=False)
        assert none is None and torch.equal(jl2, wl)
        vl, va = _nan(torch, (B, 4, 3)), _nan(torch, (B, 4, 3))
        model.velocities_dev(B, q.detach().data_ptr(), fp, qd.data_ptr(), vl.data_ptr(), va.data_ptr(), frame=fid, stream=sp)
        lin, ang = jac.link_velocities(opt, q, qd, tips, f, frame=frame)
        assert torch.equal(lin, vl) and torch.equal(ang, va) and not lin.requires_grad and not ang.requires_grad
        # the contraction and the matrix agree (float32: n_opt products of entries below 1.2 m x |qd|)
        assert float((torch.einsum("blrc,bc->blr", jl, qd) - lin).abs().max()) <= 4e-5 * max(1.0, float(qd.abs().max()) * opt.opt_dof)
    j0, a0 = jac.link_jacobians(opt, q[:0], tips, None if f is None else f[:0])  # B = 0: shapes, no launch
    assert j0.shape == a0.shape == (0, 4, 3, opt.opt_dof)


def test_torch_front_chunks_more_than_sixty_four_links(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import jacobians as jac

    robot = RobotWrapper(ROBOTS["shadow_hand_right"])
    names = [f.name for f in robot.kin.frames]
    many = (names * 4)[:70]
    q = torch.tensor(_configs(robot, 5, 20).astype(np.float32), device="cuda")
    qd = torch.ones_like(q)
    jl, ja = jac.robot_link_jacobians(robot, q, many)
    lin, ang = jac.robot_link_velocities(robot, q, qd, many, frame="local")
    assert jl.shape == ja.shape == (5, 70, 3, robot.dof) and lin.shape == ang.shape == (5, 70, 3)
    sp = torch.cuda.current_stream().cuda_stream
    parts_l, parts_a, parts_v, parts_w = [], [], [], []
    for chunk in (many[:64], many[64:]):
        m = robot.pose_model(chunk)
        a, b = _nan(torch, (5, len(chunk), 3, robot.dof)), _nan(torch, (5, len(chunk), 3, robot.dof))
        m.jacobians_dev(5, q.data_ptr(), 0, a.data_ptr(), b.data_ptr(), frame=WORLD, stream=sp)
        v, w = _nan(torch, (5, len(chunk), 3)), _nan(torch, (5, len(chunk), 3))
        m.velocities_dev(5, q.data_ptr(), 0, qd.data_ptr(), v.data_ptr(), w.data_ptr(), frame=LOCAL, stream=sp)
        parts_l.append(a), parts_a.append(b), parts_v.append(v), parts_w.append(w)
    assert torch.equal(jl, torch.cat(parts_l, 1)) and torch.equal(ja, torch.cat(parts_a, 1))
    assert torch.equal(lin, torch.cat(parts_v, 1)) and torch.equal(ang, torch.cat(parts_w, 1))
    assert not any(t.requires_grad for t in (jl, ja, lin, ang))

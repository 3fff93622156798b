"""GPU tests of the link-pose kernels (csrc/dexr_pose.hip, include/dexr_pose.h): the float64 host entry points against the
reference's own forward kinematics and against the closed-form VJP evaluated from the oracle, the float32 device entry
points against the oracle at the float32-rounded inputs under measured ceilings (tests/golden/link_poses_ceilings.json),
consistency with the dexr_fk path on every shipped config, the torch autograd functions, and batch shapes.

Measured on the MI355X at the commit named in link_poses_ceilings.json (max over 4 096 configurations and every link):
see that file; the bound of test_device_float32_against_the_oracle is 4 x those figures."""
import glob
import json
import os

import numpy as np
import pytest

from testutil import REPO
from dex_retargeting_amd import _lib, pose_tables as pt
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from oracle import cases
from oracle.kin import OracleRobot

pytestmark = pytest.mark.gpu
RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
FK = np.load(os.path.join(REPO, "tests", "golden", "fk_golden.npz"))
FK_KEYS = sorted(k[: -len("__links")] for k in FK.files if k.endswith("__links"))
ALL = sorted(os.path.relpath(p, cases.CONFIG_DIR) for p in glob.glob(os.path.join(cases.CONFIG_DIR, "*", "*.yml")))
CEILINGS = os.path.join(REPO, "tests", "golden", "link_poses_ceilings.json")


def _hand_urdfs():
    """every fixture robot (the right hand where both exist) + the arm-and-hand model of tests/urdf."""
    out = {}
    for p in sorted(glob.glob(os.path.join(cases.URDF_DIR, "*", "*.urdf"))):
        name = os.path.basename(p)[: -len(".urdf")]
        if name.endswith("_left") and os.path.exists(p.replace("_left.urdf", "_right.urdf")):
            continue
        out[name] = p
    out["arm_shadow_hand_right"] = os.path.join(REPO, "tests", "urdf", "arm_shadow_hand_right.urdf")
    return out


ROBOTS = _hand_urdfs()


def _urdf_of(key):
    free = key.endswith("__free")
    base = key[: -len("__free")] if free else key
    if base.startswith("testurdf__"):
        return os.path.join(REPO, "tests", "urdf", base[len("testurdf__"):] + ".urdf"), free
    return os.path.join(cases.URDF_DIR, base.replace("__", "/") + ".urdf"), free


def _q_by_name(dof_names, key, c):
    val = dict(zip(FK[key + "__joints"].tolist(), FK[key + "__cfg"][c].tolist()))
    mims = FK[key + "__mimic"].tolist()
    if mims != [""]:
        for n, s, a, b in zip(mims, FK[key + "__mimic_src"].tolist(), FK[key + "__mimic_mult"], FK[key + "__mimic_off"]):
            val[n] = val[s] * float(a) + float(b)
    return np.array([val[n] for n in dof_names])


def _chunks(names, n=64):
    return [names[c:c + n] for c in range(0, len(names), n)]


def oracle_vjp(orc, q, links, gp, gr):
    """The closed form in float64 from oracle.kin: per link the wrench about the world origin, per ancestor joint
    a . (T0 - o x F) (revolute) or a . F (prismatic).  q (B, dof) -> (B, dof)."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    g = np.zeros_like(q)
    for li, name in enumerate(links):
        R, p, info = orc._walk(q, name)
        f = np.zeros_like(p) if gp is None else gp[:, li]
        t0 = np.cross(p, f)
        if gr is not None:
            for c in range(3):
                t0 = t0 + np.cross(R[:, :, c], gr[:, li, :, c])
        for qi, typ, a_w, o_w in info:
            if typ == "revolute":
                g[:, qi] += np.einsum("bi,bi->b", a_w, t0 - np.cross(o_w, f))
            else:
                g[:, qi] += np.einsum("bi,bi->b", a_w, f)
    return g


def _fold(prob, g_full):
    """gradient in the full robot qpos -> gradient in the optimiser's variables (chain rule of full_qpos)."""
    out = g_full[:, prob.idx_pin2target].copy()
    for m, s, mult in zip(prob.idx_pin2mimic, prob.idx_pin2source, prob.multipliers):
        out[:, list(prob.idx_pin2target).index(s)] += mult * g_full[:, m]
    return out


CASES3 = ("position-only", "rotation-only", "both")


def _grads(rng, B, L, case, dtype=np.float64):
    gp = rng.standard_normal((B, L, 3)).astype(dtype) if case != "rotation-only" else None
    gr = rng.standard_normal((B, L, 3, 3)).astype(dtype) if case != "position-only" else None
    return gp, gr


# ---- 6. host float64 entry points against the reference's FK ------------------------------------------------------------
@pytest.mark.parametrize("key", FK_KEYS)
def test_host_float64_poses_equal_reference_fk(key, require_gpu):
    path, free = _urdf_of(key)
    robot = RobotWrapper(path, add_dummy_free_joints=free)
    links = FK[key + "__links"].tolist()
    q = np.stack([_q_by_name(robot.dof_joint_names, key, c) for c in range(FK[key + "__cfg"].shape[0])])
    T = FK[key + "__T"]
    worst = 0.0
    for c0, names in zip(range(0, len(links), 64), _chunks(links)):
        pos, rot = _lib.PoseModel(pt.compile_poses(robot.kin, names)).poses(q)
        want = T[:, c0:c0 + len(names)]
        worst = max(worst, np.abs(pos - want[:, :, :3, 3]).max(), np.abs(rot - want[:, :, :3, :3]).max())
    print(f"{key}: host float64 max |pose - reference| = {worst:.3e}")
    assert worst <= 1e-12, key
    got = robot.link_poses(q, [robot.get_link_index(n) for n in links])
    assert got.shape == (q.shape[0], len(links), 4, 4)
    assert np.abs(got - T).max() <= 1e-12, key
    # the paths that exist keep their results: positions through dexr_fk, get_link_pose on top of them
    assert np.abs(robot.link_positions(q, [robot.get_link_index(n) for n in links]) - T[:, :, :3, 3]).max() < 2e-6


# ---- 7. host float64 VJP against the closed form evaluated from the oracle ------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_host_float64_vjp_robot_order(name, require_gpu):
    for free in (False, True):
        robot = RobotWrapper(ROBOTS[name], add_dummy_free_joints=free)
        orc = OracleRobot(ROBOTS[name], free)
        links = [f.name for f in robot.kin.frames][:64]
        rng = np.random.default_rng(7)
        lim = robot.joint_limits
        q = rng.uniform(lim[:, 0], lim[:, 1], (33, robot.dof))
        model = robot.pose_model(links)
        for case in CASES3:
            gp, gr = _grads(rng, 33, len(links), case)
            g = model.vjp(q, None, gp, gr)
            want = oracle_vjp(orc, q, links, gp, gr)
            err, scale = np.abs(g - want).max(), max(1.0, np.abs(want).max())
            print(f"{name} free={free} {case}: max |g - closed form| = {err:.3e} at max |g| = {np.abs(want).max():.3f}")
            assert err <= 1e-10 * scale, (name, free, case)


@pytest.mark.parametrize("rel", ["offline/schunk_svh_hand_right.yml", "teleop/schunk_svh_hand_right.yml", "teleop/ability_hand_right.yml",
                                 "offline/inspire_hand_right.yml", "teleop/inspire_hand_right_dexpilot.yml",
                                 "offline/shadow_hand_right.yml", "teleop/allegro_hand_right.yml"])
def test_host_float64_vjp_optimizer_order_folds_mimic_joints(rel, require_gpu):
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    links = [f.name for f in opt.robot.kin.frames][:64]
    rng = np.random.default_rng(8)
    lim = prob.robot.joint_limits
    x = rng.uniform(lim[prob.idx_pin2target, 0], lim[prob.idx_pin2target, 1], (33, len(prob.idx_pin2target)))
    fixed = rng.uniform(lim[prob.idx_pin2fixed, 0], lim[prob.idx_pin2fixed, 1], (33, len(prob.idx_pin2fixed)))
    q_full = prob.full_qpos(x, fixed)
    model = opt.pose_model(links)
    assert (model.n_in, model.n_fixed, model.n_link) == (opt.opt_dof, len(opt.idx_pin2fixed), len(links))
    pos, rot = model.poses(x, fixed)
    R, p = prob.robot.link_poses(q_full, links)
    assert np.abs(pos - p).max() <= 1e-12 and np.abs(rot - R).max() <= 1e-12
    for case in CASES3:
        gp, gr = _grads(rng, 33, len(links), case)
        g = model.vjp(x, fixed, gp, gr)
        want = _fold(prob, oracle_vjp(prob.robot, q_full, links, gp, gr))
        assert np.abs(g - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), (rel, case)


# ---- 8. device float32 entry points against the oracle at the float32-rounded inputs ----------------------------------------
def measure_device_errors(name, B=4096):
    """max |pos error| (m), max |rot entry error|, max |grad error| / max(1, max |g|) of the float32 device entry points on
    `B` seeded configurations inside the joint limits, every link, torch tensors on a non-default stream."""
    import torch

    robot = RobotWrapper(ROBOTS[name])
    orc = OracleRobot(ROBOTS[name])
    links = [f.name for f in robot.kin.frames]
    rng = np.random.default_rng(2024)
    lim = robot.joint_limits
    q32 = rng.uniform(lim[:, 0], lim[:, 1], (B, robot.dof)).astype(np.float32)
    q64 = q32.astype(np.float64)  # the oracle sees exactly what the kernel sees
    e_pos = e_rot = e_grad = 0.0
    stream = torch.cuda.Stream()
    for names in _chunks(links):
        model = robot.pose_model(names)
        L = len(names)
        gp32, gr32 = _grads(rng, B, L, "both", np.float32)
        with torch.cuda.stream(stream):
            x = torch.tensor(q32, device="cuda")
            pos = torch.empty((B, L, 3), dtype=torch.float32, device="cuda")
            rot = torch.empty((B, L, 3, 3), dtype=torch.float32, device="cuda")
            gp, gr = torch.tensor(gp32, device="cuda"), torch.tensor(gr32, device="cuda")
            gx = torch.full((B, robot.dof), float("nan"), dtype=torch.float32, device="cuda")
            model.poses_dev(B, x.data_ptr(), 0, pos.data_ptr(), rot.data_ptr(), stream=stream.cuda_stream)
            model.vjp_dev(B, x.data_ptr(), 0, gp.data_ptr(), gr.data_ptr(), gx.data_ptr(), stream=stream.cuda_stream)
        stream.synchronize()
        R, p = orc.link_poses(q64, names)
        want = oracle_vjp(orc, q64, names, gp32.astype(np.float64), gr32.astype(np.float64))
        e_pos = max(e_pos, float(np.abs(pos.cpu().numpy() - p).max()))
        e_rot = max(e_rot, float(np.abs(rot.cpu().numpy() - R).max()))
        e_grad = max(e_grad, float(np.abs(gx.cpu().numpy() - want).max() / max(1.0, np.abs(want).max())))
    return dict(pos=e_pos, rot=e_rot, grad=e_grad)


@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_oracle(name, require_gpu):
    pytest.importorskip("torch")
    with open(CEILINGS) as f:
        ceil = json.load(f)
    got = measure_device_errors(name)
    print(f"{name}: measured now {got}; recorded {ceil['robots'][name]} at {ceil['commit']}")
    for k in ("pos", "rot", "grad"):
        bound = 4.0 * ceil["robots"][name][k]
        if k != "grad":
            assert bound <= 1e-5, (name, k, bound)  # ~30 joints x 4 roundings x 6e-8: beyond this it is a defect, not noise
        assert np.isfinite(got[k]) and got[k] <= bound, (name, k, got[k], bound)


def test_ceilings_cover_exactly_the_fixture_robots():
    with open(CEILINGS) as f:
        ceil = json.load(f)
    assert sorted(ceil["robots"]) == sorted(ROBOTS) and len(ROBOTS) == 8 and ceil["configurations"] == 4096


# ---- 9. consistency with the kernels that already exist ------------------------------------------------------------------
@pytest.mark.parametrize("rel", ALL)
def test_positions_agree_with_the_fk_path_at_a_solve(rel, require_gpu):
    """At the answer of a 256-frame solve, the optimiser's computed links through the optimizer-order pose table equal
    RobotWrapper.link_positions (dexr_fk, untouched) within that path's own bound 2e-6: float64 arithmetic on both sides,
    so the difference is the float32 table entries of dexr_fk.  (The float32 device arithmetic is pinned against the oracle
    by test_device_float32_against_the_oracle.)"""
    assert len(ALL) == 39
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    d = cases.human_set(prob, 256)
    st = np.zeros(256, np.uint32) if prob.kind == "dexpilot" else None
    q = opt.retarget_batch(d["ref"], d["fixed"], d["last"], state=st)
    links = list(prob.computed_links)
    pos, _ = opt.pose_model(links).poses(q, d["fixed"], rotations=False)
    full = prob.full_qpos(q.astype(np.float64), d["fixed"])
    want = opt.robot.link_positions(full, [opt.robot.get_link_index(n) for n in links])
    err = np.abs(pos - want).max()
    print(f"{rel}: max |link_poses - link_positions| = {err:.3e}")
    assert err < 2e-6, rel


# ---- 10. autograd ---------------------------------------------------------------------------------------------------------
def _t(a, torch, **kw):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", **kw)


@pytest.mark.parametrize("rel", ["teleop/shadow_hand_right_dexpilot.yml", "offline/schunk_svh_hand_right.yml"])
def test_autograd_link_poses_equals_the_entry_points_bitwise(rel, require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    links = list(prob.computed_links)
    B, L = 300, len(links)
    d = cases.human_set(prob, B)
    q = _t(d["last"], torch, requires_grad=True)
    fixed = _t(d["fixed"], torch) if d["fixed"].shape[1] else None
    model = opt.pose_model(links)
    pos_d = torch.empty((B, L, 3), dtype=torch.float32, device="cuda")
    rot_d = torch.full((B, L, 3, 3), 7.0, dtype=torch.float32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    fp = 0 if fixed is None else fixed.data_ptr()
    model.poses_dev(B, q.detach().data_ptr(), fp, pos_d.data_ptr(), rot_d.data_ptr(), stream=sp)
    pos, rot = ag.link_poses(opt, q, links, fixed)
    assert torch.equal(pos, pos_d) and torch.equal(rot, rot_d)
    gen = torch.Generator("cuda").manual_seed(3)
    gp = torch.randn(pos.shape, device="cuda", generator=gen)
    gr = torch.randn(rot.shape, device="cuda", generator=gen)
    for case in CASES3:
        outs, gs = [], []
        if case != "rotation-only":
            outs.append(pos), gs.append(gp)
        if case != "position-only":
            outs.append(rot), gs.append(gr)
        (g,) = torch.autograd.grad(outs, q, gs, retain_graph=True)
        want = torch.full_like(q, float("nan"))
        model.vjp_dev(B, q.detach().data_ptr(), fp, gp.data_ptr() if case != "rotation-only" else 0,
                      gr.data_ptr() if case != "position-only" else 0, want.data_ptr(), stream=sp)
        assert torch.equal(g, want) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, case
    # rotations=False: no rot is produced, the positions are the same bits, and the kernel is not handed a rot buffer
    pos2, none = ag.link_poses(opt, q, links, fixed, rotations=False)
    assert none is None and torch.equal(pos2, pos_d)
    rot_d.fill_(7.0)
    model.poses_dev(B, q.detach().data_ptr(), fp, pos_d.data_ptr(), 0, stream=sp)
    torch.cuda.synchronize()
    assert bool((rot_d == 7.0).all()) and torch.equal(pos2, pos_d)
    (g2,) = torch.autograd.grad(pos2, q, gp)
    (g1,) = torch.autograd.grad(pos, q, gp)
    assert torch.equal(g1, g2)
    # robot order: full qpos, float64 converted once
    full = prob.full_qpos(d["last"].astype(np.float64), d["fixed"])
    p64, r64 = ag.robot_link_poses(opt.robot, _t(full, torch, dtype=torch.float64), links)
    p32, r32 = ag.robot_link_poses(opt.robot, _t(full.astype(np.float32), torch), links)
    assert torch.equal(p64, p32) and torch.equal(r64, r32) and p32.dtype == torch.float32
    assert float((p32 - pos_d).abs().max()) < 1e-5


def test_autograd_link_poses_argument_checks(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    rel = "teleop/allegro_hand_right.yml"
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip"]
    good = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    launches = []
    orig = _lib.PoseModel.poses_dev
    _lib.PoseModel.poses_dev = lambda self, *a, **k: launches.append(1) or orig(self, *a, **k)
    try:
        for bad in (good.double(), good[:, :15], good.reshape(-1), good.cpu(), good.cpu().numpy()):
            with pytest.raises(ValueError):
                ag.link_poses(opt, bad, tips)
        with pytest.raises(ValueError):
            ag.link_poses(opt, good, tips, fixed_qpos=torch.zeros((4, 1), dtype=torch.float32, device="cuda"))
        with pytest.raises(ValueError):
            ag.link_poses(opt, good, [])
        with pytest.raises(ValueError, match="is not a link name"):
            ag.link_poses(opt, good, ["no_such_link"])
        with pytest.raises(ValueError):
            ag.robot_link_poses(opt.robot, good[:, :3], tips)
        assert launches == []
        pos, rot = ag.link_poses(opt, good, tips)
        assert launches == [1] and pos.shape == (4, 2, 3) and rot.shape == (4, 2, 3, 3)
        p0, r0 = ag.link_poses(opt, good[:0], tips)  # B = 0: shapes, no launch
        assert p0.shape == (0, 2, 3) and r0.shape == (0, 2, 3, 3) and launches == [1]
    finally:
        _lib.PoseModel.poses_dev = orig
    # the C entry points' own contract
    m = opt.pose_model(tuple(tips))
    lib = _lib.load()
    assert lib.dexr_link_poses_dev(m.handle, 0, None, None, None, None, None) == 0
    assert lib.dexr_link_poses_vjp_dev(m.handle, 4, good.data_ptr(), None, None, None, good.data_ptr(), None) == -1
    assert b"both NULL" in lib.dexr_last_error()
    assert lib.dexr_link_poses_dev(None, 4, None, None, None, None, None) == -1


@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "teleop/shadow_hand_right_dexpilot.yml", "offline/schunk_svh_hand_right.yml"])
def test_keypoints_to_task_space_loss_end_to_end(rel, require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    B = 256
    d = cases.human_set(prob, B)
    links = list(prob.computed_links)
    kp = _t(d["kp"], torch, dtype=torch.float32, requires_grad=True)
    last = _t(d["last"], torch, requires_grad=True)
    fixed = _t(d["fixed"], torch) if d["fixed"].shape[1] else None
    st = np.zeros(B, np.int32) if prob.kind == "dexpilot" else None
    contact = torch.randn((B, len(links), 3), device="cuda", generator=torch.Generator("cuda").manual_seed(1)) * 0.05
    ref = ag.ref_value_from_keypoints(opt, kp)
    q = ag.retarget(opt, ref, last, fixed, None if st is None else _t(st, torch))
    tips, _ = ag.link_poses(opt, q, links, fixed, rotations=False)
    loss = ((tips - contact) ** 2).sum()
    loss.backward()
    assert bool(torch.isfinite(kp.grad).all()) and float(kp.grad.abs().max()) > 0
    assert bool(torch.isfinite(last.grad).all()) and float(last.grad.abs().max()) > 0
    # the two pieces by hand: grad_q from the pose VJP entry point, then the solve's VJP entry point fed with it
    sp = torch.cuda.current_stream().cuda_stream
    fp = 0 if fixed is None else fixed.data_ptr()
    g_tips = (2 * (tips - contact)).detach().contiguous()
    grad_q = torch.full_like(q, float("nan"))
    opt.pose_model(links).vjp_dev(B, q.detach().data_ptr(), fp, g_tips.data_ptr(), 0, grad_q.data_ptr(), stream=sp)
    gref, glast = torch.zeros_like(ref), torch.zeros_like(last)
    stat = torch.zeros(B, dtype=torch.int32, device="cuda")
    st_in = None if st is None else _t(st, torch)
    opt.vjp_model().vjp_dev(B, ref.detach().data_ptr(), fp, last.detach().data_ptr(), 0 if st_in is None else st_in.data_ptr(),
                            q.detach().data_ptr(), grad_q.data_ptr(), gref.data_ptr(), glast.data_ptr(), stat.data_ptr(), stream=sp)
    (want_kp,) = torch.autograd.grad(ag.ref_value_from_keypoints(opt, kp), kp, gref)
    assert torch.equal(kp.grad, want_kp) and torch.equal(last.grad, glast)


# ---- 11. shapes --------------------------------------------------------------------------------------------------------
def _dev_run(model, torch, x32, gp32, gr32, rotations=True):
    B, L = x32.shape[0], model.n_link
    x = torch.tensor(x32, device="cuda")
    pos = torch.full((B, L, 3), float("nan"), dtype=torch.float32, device="cuda")
    rot = torch.full((B, L, 3, 3), float("nan"), dtype=torch.float32, device="cuda")
    gx = torch.full((B, model.n_in), float("nan"), dtype=torch.float32, device="cuda")
    gp, gr = torch.tensor(gp32, device="cuda"), torch.tensor(gr32, device="cuda")
    sp = torch.cuda.current_stream().cuda_stream
    model.poses_dev(B, x.data_ptr(), 0, pos.data_ptr(), rot.data_ptr() if rotations else 0, stream=sp)
    model.vjp_dev(B, x.data_ptr(), 0, gp.data_ptr(), gr.data_ptr(), gx.data_ptr(), stream=sp)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), rot.cpu().numpy(), gx.cpu().numpy()


def test_batch_shapes_are_row_independent(require_gpu):
    torch = pytest.importorskip("torch")
    robot = RobotWrapper(ROBOTS["shadow_hand_right"])
    links = ["thtip", "fftip", "mftip", "rftip", "lftip", "palm"]
    model = robot.pose_model(links)
    rng = np.random.default_rng(12)
    lim = robot.joint_limits
    N = 65600
    x = rng.uniform(lim[:, 0], lim[:, 1], (N, robot.dof)).astype(np.float32)
    gp = rng.standard_normal((N, len(links), 3)).astype(np.float32)
    gr = rng.standard_normal((N, len(links), 3, 3)).astype(np.float32)
    P, R, G = _dev_run(model, torch, x, gp, gr)
    assert np.isfinite(P).all() and np.isfinite(R).all() and np.isfinite(G).all()
    for B in (1, 63, 64, 65, 4097, 65536):
        for off in (0, 17):  # the same rows at another position of another batch
            if off + B > N:
                continue
            p, r, g = _dev_run(model, torch, x[off:off + B], gp[off:off + B], gr[off:off + B])
            assert np.array_equal(p, P[off:off + B]) and np.array_equal(r, R[off:off + B]) and np.array_equal(g, G[off:off + B]), (B, off)
    # B = 0: a no-op on both kinds of entry point
    assert _lib.load().dexr_link_poses_dev(model.handle, 0, None, None, None, None, None) == 0
    assert _lib.load().dexr_link_poses_vjp_dev(model.handle, 0, None, None, None, None, None, None) == -1  # both gradients NULL
    p0, r0 = model.poses(np.zeros((0, robot.dof)))
    assert p0.shape == (0, 6, 3) and r0.shape == (0, 6, 3, 3)
    assert model.vjp(np.zeros((0, robot.dof)), None, np.zeros((0, 6, 3)), None).shape == (0, robot.dof)
    # a row of NaN: that frame is non-finite, every other row keeps its bits
    xn = x[:200].copy()
    xn[77] = np.nan
    p, r, g = _dev_run(model, torch, xn, gp[:200], gr[:200])
    keep = np.arange(200) != 77
    assert np.array_equal(p[keep], P[:200][keep]) and np.array_equal(r[keep], R[:200][keep]) and np.array_equal(g[keep], G[:200][keep])
    assert not np.isfinite(p[77]).any() and not np.isfinite(g[77]).all()


def test_one_link_sixty_four_links_and_a_base_link(require_gpu):
    torch = pytest.importorskip("torch")
    robot = RobotWrapper(ROBOTS["shadow_hand_right"])
    orc = OracleRobot(ROBOTS["shadow_hand_right"])
    rng = np.random.default_rng(13)
    lim = robot.joint_limits
    B = 130
    x = rng.uniform(lim[:, 0], lim[:, 1], (B, robot.dof)).astype(np.float32)
    names = [f.name for f in robot.kin.frames]
    base = robot.kin.frames[0].name
    assert robot.kin.frames[0].parent == -1
    with open(CEILINGS) as f:
        ceil = json.load(f)["robots"]["shadow_hand_right"]
    for links in (["fftip"], (names * 3)[:64], [base], ["thtip", base, "lftip"]):
        L = len(links)
        model = robot.pose_model(links)
        assert model.n_link == L
        gp = rng.standard_normal((B, L, 3)).astype(np.float32)
        gr = rng.standard_normal((B, L, 3, 3)).astype(np.float32)
        p, r, g = _dev_run(model, torch, x, gp, gr)
        Rw, pw = orc.link_poses(x.astype(np.float64), links)
        want = oracle_vjp(orc, x.astype(np.float64), links, gp.astype(np.float64), gr.astype(np.float64))
        # float32: the robot's own ceilings (same arithmetic, same relative measure as test_device_float32_against_the_oracle)
        assert np.abs(p - pw).max() <= 4 * ceil["pos"] and np.abs(r - Rw).max() <= 4 * ceil["rot"]
        assert np.abs(g - want).max() <= 4 * ceil["grad"] * max(1.0, np.abs(want).max())
        # the float64 twins
        p64, r64 = model.poses(x.astype(np.float64))
        g64 = model.vjp(x.astype(np.float64), None, gp.astype(np.float64), gr.astype(np.float64))
        assert np.abs(p64 - pw).max() <= 1e-12 and np.abs(r64 - Rw).max() <= 1e-12
        assert np.abs(g64 - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
        if links == [base]:
            assert np.array_equal(p, np.zeros((B, 1, 3), np.float32)) and np.array_equal(r[:, 0], np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3)))
            assert np.array_equal(g, np.zeros_like(g)) and np.array_equal(g64, np.zeros_like(g64))
    # more than 64 links through the wrapper: chunked
    ids = [robot.get_link_index(n) for n in (names * 4)[:70]]
    T = robot.link_poses(x[:3].astype(np.float64), ids)
    Rw, pw = orc.link_poses(x[:3].astype(np.float64), (names * 4)[:70])
    assert T.shape == (3, 70, 4, 4) and np.abs(T[:, :, :3, :3] - Rw).max() <= 1e-12 and np.abs(T[:, :, :3, 3] - pw).max() <= 1e-12
    import torch as _torch
    from dex_retargeting_amd import autograd as ag

    p70, r70 = ag.robot_link_poses(robot, _torch.tensor(x[:3], device="cuda"), (names * 4)[:70])
    assert p70.shape == (3, 70, 3) and r70.shape == (3, 70, 3, 3) and np.abs(p70.cpu().numpy() - pw).max() < 1e-5

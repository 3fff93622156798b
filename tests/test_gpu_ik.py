"""GPU tests of the damped least-squares IK step (csrc/dexr_pose.hip, include/dexr_ik.h): the float64 host entry point against
tests/ik_reference.py (robot order, optimizer order with the mimic fold and fixed joints), its residual through the wrench and
velocity kernels, the float32 device entry point against the float64 host twin, the table limits on the synthetic robots of
tests/pose_zoo.py, row independence and isolation, the raw ABI's argument errors, the torch front and a tracking loop.

INPUTS.  Errors 0.01 N(0, 1) m and 0.1 N(0, 1) rad, weights uniform in [0.5, 2] with about one in eight exactly 0, everything
float32-representable.  The damping of a table is 1e-3 times the largest eigenvalue of J^T W J over the batch, computed in
float64 from the oracle's Jacobians for both blocks of rows, with unit weights and with the weights of the test, the larger of
the two, rounded UP to float32.  Every system a test solves is J^T W J + damping I of a subset of those rows (a subset's
matrix is smaller in the positive semi-definite order), so its condition number is at most (lmax + damping) / damping <= 1001:
asserted on both full forms, a condition on the inputs and not a measurement.

GATES.  float64: 1e-9 max |want| per table (n u kappa = 64 * 1.1e-16 * 1e3 = 7e-12, two orders of margin).  float32: the
device may be 8 x as far from the float64 host twin as the reference's own float32 run (dtype=np.float32 throughout) is from
its float64 run, max norm per table and frame; tests/test_gpu_wrench.py uses 4 x for a sum, the factor is doubled because
LAPACK's pivoted LU in the reference and the kernel's Cholesky share the bound kappa n u but not the error.  Both figures are
printed; those of the MI355X are in docs/experiments/link_ik.md."""
import numpy as np
import pytest

import ik_reference as ikr
import pose_zoo as zoo
import test_gpu_link_poses as glp
from dex_retargeting_amd import _lib
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from oracle.kin import OracleRobot
from test_gpu_link_jacobians import OPT_ORDER, _fold4, _opt_inputs, _optimizer_and_problem, oracle_jacobians
from test_ik_host import TRACK_STEPS, assert_descends, tracking_inputs
from test_jacobian_host import SUBSET_CFG

pytestmark = pytest.mark.gpu
ROBOTS = glp.ROBOTS
WORLD, LOCAL = _lib.JAC_WORLD_ALIGNED, _lib.JAC_LOCAL
FRAMES = (WORLD, LOCAL)
KAPPA = 1001.0


def _r32(a):
    return a.astype(np.float32).astype(np.float64)


def _configs(robot, B, seed):
    lim = robot.joint_limits
    return _r32(np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], (B, robot.dof)))


def _errors_and_weights(B, L, seed):
    rng = np.random.default_rng(seed)
    el, ea = _r32(0.01 * rng.standard_normal((B, L, 3))), _r32(0.1 * rng.standard_normal((B, L, 3)))
    wl, wa = _r32(rng.uniform(0.5, 2, (B, L))), _r32(rng.uniform(0.5, 2, (B, L)))
    wl[rng.random((B, L)) < 0.125] = 0.0
    wa[rng.random((B, L)) < 0.125] = 0.0
    return el, ea, wl, wa


def _damping(jl, ja, wl, wa):
    """float32(1e-3 max_b lambda_max(J^T W J)), rounded up, over unit weights and the given ones; and the condition numbers of
    the two damped matrices, asserted <= 1001."""
    one = np.ones_like(wl)
    B, L, _, n = jl.shape
    A = np.concatenate([jl, ja], 1).reshape(B, 6 * L, n)
    Hs = [np.matmul(A.transpose(0, 2, 1), A * np.repeat(np.concatenate([a, b], 1), 3, axis=1)[:, :, None]) for a, b in ((one, one), (wl, wa))]
    lmax = max(float(np.linalg.eigvalsh(H)[:, -1].max()) for H in Hs)
    lam = np.float32(1e-3 * lmax)
    if float(lam) < 1e-3 * lmax:
        lam = np.nextafter(lam, np.float32(np.inf))
    lam = float(lam)
    assert lam > 0 and np.isfinite(lam)
    for H in Hs:
        ev = np.linalg.eigvalsh(H + lam * np.eye(H.shape[-1]))
        kappa = float((ev[:, -1] / ev[:, 0]).max())
        assert kappa <= KAPPA * (1 + 1e-9), kappa  # (1e-9: the eigenvalue solver's own rounding)
    return lam


class Table:
    """One pose table with its inputs and yardstick: x, fixed the table's inputs, q_full the oracle's joint vector, fold the
    chain rule of the source map on the last axis of a Jacobian (None: robot order)."""

    def __init__(self, tag, model, orc, links, x, fixed, q_full, fold, seed):
        self.tag, self.model, self.orc, self.links, self.x, self.fixed, self.q_full, self.fold = tag, model, orc, list(links), x, fixed, q_full, fold
        B, L = x.shape[0], len(self.links)
        self.el, self.ea, self.wl, self.wa = _errors_and_weights(B, L, seed)
        jl, ja, _ = oracle_jacobians(orc, q_full, self.links)
        if fold is not None:
            jl, ja = fold(jl), fold(ja)
        self.lam = _damping(jl, ja, self.wl, self.wa)
        self._want, self._jac = {}, {}

    def form(self, rows, weighted):
        el = self.el if rows != "rotation-only" else None
        ea = self.ea if rows != "position-only" else None
        return el, ea, (self.wl if weighted and el is not None else None), (self.wa if weighted and ea is not None else None)

    def want(self, rows, weighted, frame, dtype=np.float64):
        """the reference, computed once per form and shared."""
        key = (rows, weighted, frame, dtype)
        if key not in self._want:
            el, ea, wl, wa = self.form(rows, weighted)
            c = (lambda a: None if a is None else a.astype(dtype))
            if (frame, dtype) not in self._jac:  # the reference's Jacobians depend on the frame and the type alone
                self._jac[frame, dtype] = ikr.jacobians(self.orc, self.q_full.astype(dtype), self.links, frame, dtype)
            self._want[key] = ikr.ik_step(self.orc, self.q_full.astype(dtype), self.links, c(el), c(ea), c(wl), c(wa), self.lam, frame, dtype, self.fold,
                                          jac=self._jac[frame, dtype])
            self._want[key].setflags(write=False)
        return self._want[key]

    def host(self, rows, weighted, frame):
        el, ea, wl, wa = self.form(rows, weighted)
        return self.model.ik_step(self.x, self.fixed, el, ea, wl, wa, self.lam, frame)

    def dev(self, torch, rows, weighted, frame):
        el, ea, wl, wa = self.form(rows, weighted)
        return dev_ik(self.model, torch, self.x, el, ea, wl, wa, self.lam, self.fixed, frame)


# ---- the float32 device entry point on numpy arrays, the output pre-filled with NaN ---------------------------------------------
def _dev(torch, a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def dev_ik(model, torch, x, el, ea, wl, wa, damping, fixed=None, frame=WORLD):
    B = x.shape[0]
    tx, tf, tel, tea, twl, twa = (_dev(torch, a) for a in (x, fixed, el, ea, wl, wa))
    dx = _nan(torch, (B, model.n_in))
    model.ik_step_dev(B, _ptr(tx), _ptr(tf), _ptr(tel), _ptr(tea), _ptr(twl), _ptr(twa), damping, _ptr(dx), frame=frame,
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dx.cpu().numpy()


ROWS = ("position-only", "rotation-only", "both")


def _check_float64(t):
    """every input form, both frames, weights NULL and given: <= 1e-9 max |want| per table."""
    worst = 0.0
    for frame in FRAMES:
        for rows in ROWS:
            for weighted in (False, True):
                want = t.want(rows, weighted, frame)
                got = t.host(rows, weighted, frame)
                scale = float(np.abs(want).max())
                err = float(np.abs(got - want).max())
                worst = max(worst, err / scale if scale > 0 else float(err > 0))  # (rotation rows of a gripper without a revolute joint: 0 = 0)
                assert got.shape == want.shape and np.isfinite(got).all()
                assert err <= 1e-9 * scale, (t.tag, frame, rows, weighted, err, scale)
    print(f"{t.tag}: float64 largest max |dx - reference| / max |reference| over 12 forms = {worst:.3e} (gate 1e-9), damping {t.lam:.3e}")
    return worst


def _check_float32(torch, t, forms=(("both", True), ("position-only", False))):
    """the device against the host twin under 8 x the reference's own float32 distance, per table and frame."""
    rows_out = []
    for frame in FRAMES:
        for rows, weighted in forms:
            w64 = t.want(rows, weighted, frame)
            ref_err = float(np.abs(t.want(rows, weighted, frame, np.float32).astype(np.float64) - w64).max())
            host = t.host(rows, weighted, frame)
            dev = dev_ik(t.model, torch, t.x, *t.form(rows, weighted), t.lam, t.fixed, frame)
            assert dev.dtype == np.float32 and dev.shape == host.shape and np.isfinite(dev).all(), (t.tag, frame, rows, "an entry was not written or is not finite")
            err = float(np.abs(dev - host).max())
            ratio = err / ref_err if ref_err > 0 else (0.0 if err == 0 else float("inf"))
            print(f"{t.tag} frame={frame} {rows}{' weighted' if weighted else ''}: float32 max |dx - host| = {err:.3e}, the reference's float32 run is "
                  f"{ref_err:.3e} from its float64 run (gate {8 * ref_err:.3e}, error / reference distance {ratio:.2f}), max |dx| = {np.abs(w64).max():.3e}")
            rows_out.append((t.tag, frame, rows, err, ref_err))
            if ref_err > 0:
                assert err <= 8 * ref_err, (t.tag, frame, rows, err, ref_err)
            else:  # a table the reference solves alike in both types: nothing to scale by, the float64 gate
                assert err <= 1e-9 * float(np.abs(w64).max()), (t.tag, frame, rows, err)
    return rows_out


# ---- 1. float64 host entry point against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_host_float64_against_the_reference_robot_order(name, require_gpu):
    for free in (False, True):
        robot = RobotWrapper(ROBOTS[name], add_dummy_free_joints=free)
        orc = OracleRobot(ROBOTS[name], free)
        links = [f.name for f in robot.kin.frames][:64]
        q = _configs(robot, 130, 81)
        _check_float64(Table(f"{name} free={free}", robot.pose_model(links), orc, links, q, None, q, None, 82))


@pytest.mark.parametrize("rel", OPT_ORDER + ["subset"])
def test_host_float64_optimizer_order_folds_mimic_and_fixed_joints(rel, require_gpu):
    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames][:64]
    x, fixed = (_r32(a) for a in _opt_inputs(prob, 130, 83))
    model = opt.pose_model(links)
    assert (model.n_in, model.n_fixed) == (opt.opt_dof, len(opt.idx_pin2fixed))
    if rel == "subset":
        assert model.n_fixed == 6
    t = Table(rel, model, prob.robot, links, x, fixed if fixed.shape[1] else None, prob.full_qpos(x, fixed), lambda J: _fold4(prob, J), 84)
    _check_float64(t)
    if len(prob.idx_pin2mimic):  # folding dx of the full joint vector instead of J gives another step
        full = ikr.ik_step(prob.robot, t.q_full, links, t.el, t.ea, t.wl, t.wa, t.lam)
        assert np.abs(glp._fold(prob, full) - t.want("both", True, WORLD)).max() > 1e-6 * np.abs(full).max()


# ---- 2. the residual through the kernels the step fuses -----------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["robot:shadow_hand_right", "offline/schunk_svh_hand_right.yml"])
def test_residual_through_the_wrench_and_velocity_kernels(rel, require_gpu):
    """the normal equations J^T W (e - J dx) = damping dx, with J^T and J applied by dexr_link_wrenches / dexr_link_velocities."""
    if rel.startswith("robot:"):
        robot = RobotWrapper(ROBOTS[rel[6:]], add_dummy_free_joints=True)
        links = [f.name for f in robot.kin.frames][:64]
        model, x, fixed = robot.pose_model(links), _configs(robot, 130, 85), None
        orc, q_full, fold = OracleRobot(ROBOTS[rel[6:]], True), x, None
    else:
        opt, prob = _optimizer_and_problem(rel)
        links = [f.name for f in opt.robot.kin.frames][:64]
        x, fixed = (_r32(a) for a in _opt_inputs(prob, 130, 85))
        fixed = fixed if fixed.shape[1] else None
        model, orc, q_full, fold = opt.pose_model(links), prob.robot, prob.full_qpos(x, fixed), (lambda J: _fold4(prob, J))
    t = Table(rel, model, orc, links, x, fixed, q_full, fold, 86)
    for frame in FRAMES:
        for rows in ROWS:
            el, ea, wl, wa = t.form(rows, True)
            dx = t.host(rows, True, frame)
            lin, ang = model.velocities(x, dx, fixed, frame=frame)
            f = None if el is None else wl[..., None] * (el - lin)
            m = None if ea is None else wa[..., None] * (ea - ang)
            rhs = model.wrenches(x, fixed, None if el is None else wl[..., None] * el, None if ea is None else wa[..., None] * ea, frame)
            err = float(np.abs(model.wrenches(x, fixed, f, m, frame) - t.lam * dx).max())
            print(f"{rel} frame={frame} {rows}: max |J^T W (e - J dx) - damping dx| = {err:.3e} at max |J^T W e| = {np.abs(rhs).max():.3e}")
            assert err <= 1e-9 * float(np.abs(rhs).max()), (rel, frame, rows)


# ---- 3. float32 device entry point against the float64 host twin ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_host_twin(name, require_gpu):
    torch = pytest.importorskip("torch")
    assert len(ROBOTS) == 8
    robot = RobotWrapper(ROBOTS[name])
    orc = OracleRobot(ROBOTS[name])
    q = _configs(robot, 130, 87)
    for ci, names in enumerate(glp._chunks([f.name for f in robot.kin.frames])):
        _check_float32(torch, Table(f"{name}[{ci}]", robot.pose_model(names), orc, names, q, None, q, None, 88 + ci))


# ---- 4. table limits: the synthetic robots of tests/pose_zoo.py ----------------------------------------------------------------------
ZOO = ["chain64", "binary64", "binary64_slots8", "star40", "two_trees100_b", "wide_map"]
ZB = 33  # float32: 4 frames per block on the 64-link members, float64 2: ragged tails of 1


@pytest.fixture(scope="module")
def zoo_tables(tmp_path_factory):
    d, made = tmp_path_factory.mktemp("ik_zoo"), {}

    def get(name):
        if name not in made:
            m = zoo.build(name, d)
            x, fixed, _ = zoo.inputs(m, ZB, 2031)
            t = Table(name, _lib.PoseModel(m.blob), m.orc, m.links, x, fixed, zoo.full_q(m.smap, x, fixed), (lambda J, m=m: zoo.fold(m.smap, J)), 2032)
            t.member = m
            made[name] = t
        return made[name]

    return get


@pytest.mark.parametrize("name", ZOO)
def test_table_limits_float64_and_float32(name, zoo_tables, require_gpu):
    torch = pytest.importorskip("torch")
    t = zoo_tables(name)
    m, tab = t.member, t.member.tab
    assert {k: int(tab["h"][k]) for k in ("n_joint", "n_slot", "n_in", "n_link")} == {k: zoo.FACTS[name][k] for k in ("n_joint", "n_slot", "n_in", "n_link")}
    read = np.flatnonzero(zoo.abs_mult(m).sum(0) > 0)
    unread = np.setdiff1d(np.arange(t.model.n_in), read)
    if name == "chain64":
        assert len(read) == 64 and t.model.n_link == 64  # the largest H and the smallest block
    if name == "star40":
        assert int((tab["links"]["parent"] == -1).sum()) == 3 and len(set(m.links)) < len(m.links)
    if name == "two_trees100_b":
        assert t.model.n_in == 100 and (read < 64).any() and (read >= 64).any()
        H, _ = ikr.normal_equations(m.orc, t.q_full, m.links, t.el, t.ea, t.wl, t.wa, fold=t.fold)
        lo, hi = read[read < 50], read[read >= 50]
        assert np.abs(H[:, lo][:, :, hi]).max() == 0 and np.abs(H[:, lo][:, :, lo]).max() > 0 and np.abs(H[:, hi][:, :, hi]).max() > 0  # block diagonal
    if name == "wide_map":
        assert t.model.n_in == 256 and len(unread) == 233 and zoo.SHARED_COL in read
        kinds = {int(k) for k in tab["joints"]["src_kind"]}
        assert kinds == {0, 1, 2} and int((tab["joints"]["src_col"][tab["joints"]["src_kind"] == 0] == zoo.SHARED_COL).sum()) == 8
    _check_float64(t)
    _check_float32(torch, t)
    for frame in FRAMES:
        for got in (t.host("both", True, frame), t.dev(torch, "both", True, frame)):  # (the device output was pre-filled with NaN)
            assert np.isfinite(got).all()
            assert np.array_equal(got[:, unread], np.zeros_like(got[:, unread])), (name, frame, "an unread column is not an exact zero")
            assert (np.abs(got[:, read]).max(0) > 0).all(), (name, frame)


def test_slots_three_to_seven_give_the_bits_of_slots_zero_to_four(zoo_tables, require_gpu):
    torch = pytest.importorskip("torch")
    a, b = zoo_tables("binary64"), zoo_tables("binary64_slots8")
    assert int(b.member.tab["h"]["n_slot"]) == 8 and {int(s) for s in b.member.tab["joints"]["save"] if s >= 0} == {3, 4, 5, 6, 7}
    assert np.array_equal(a.x, b.x) and np.array_equal(a.el, b.el) and np.array_equal(a.wa, b.wa) and a.lam == b.lam
    for frame in FRAMES:
        for rows in ROWS:
            assert np.array_equal(a.host(rows, True, frame), b.host(rows, True, frame)), ("float64", frame, rows)
            assert np.array_equal(a.dev(torch, rows, True, frame), b.dev(torch, rows, True, frame)), ("float32", frame, rows)


# ---- 5. row independence and isolation ---------------------------------------------------------------------------------------------
def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    robot = RobotWrapper(ROBOTS["shadow_hand_right"])
    orc = OracleRobot(ROBOTS["shadow_hand_right"])
    tips = ["thtip", "fftip", "mftip", "rftip", "lftip"]
    B = 130
    q = _configs(robot, B, 91)
    t = Table("shadow tips", robot.pose_model(tips), orc, tips, q, None, q, None, 92)
    model, lam = t.model, t.lam
    lib = _lib.load()
    for frame in FRAMES:
        for rows in ROWS:
            el, ea, wl, wa = t.form(rows, True)
            cut = lambda a, lo, hi: None if a is None else a[lo:hi]  # noqa: E731
            DX = dev_ik(model, torch, q, el, ea, wl, wa, lam, frame=frame)  # B = 130: eight full blocks of 16 frames and a ragged one
            assert np.isfinite(DX).all() and np.abs(DX).max() > 0
            for lo, hi in ((0, 1), (0, 63), (0, 64), (65, 130), (129, 130)):  # B = 1, 63, 64, 65, 1
                dx = dev_ik(model, torch, q[lo:hi], cut(el, lo, hi), cut(ea, lo, hi), cut(wl, lo, hi), cut(wa, lo, hi), lam, frame=frame)
                assert np.array_equal(dx, DX[lo:hi]), (frame, rows, lo, hi)
            # all-zero weights: the step is exactly 0
            zl, za = (None if a is None else np.zeros_like(a) for a in (wl, wa))
            assert np.array_equal(dev_ik(model, torch, q, el, ea, zl, za, lam, frame=frame), np.zeros_like(DX)), (frame, rows)
        # a NaN in err_lin of frame 7: row 7 is not finite, every other row keeps its bits
        el, ea, wl, wa = t.form("both", True)
        DX = dev_ik(model, torch, q, el, ea, wl, wa, lam, frame=frame)
        bad = el.copy()
        bad[7, 2, 1] = np.nan
        dx = dev_ik(model, torch, q, bad, ea, wl, wa, lam, frame=frame)
        assert not np.isfinite(dx[7]).all(), frame
        keep = np.arange(B) != 7
        assert np.array_equal(dx[keep], DX[keep]), frame
        # B = 0: a no-op, NULL pointers and all
        assert lib.dexr_link_ik_step_dev(model.handle, 0, None, None, frame, None, None, None, None, lam, None, None) == 0
        assert lib.dexr_link_ik_step(model.handle, 0, None, None, frame, None, None, None, None, lam, None) == 0
    z = np.zeros((0, robot.dof))
    assert model.ik_step(z, err_lin=np.zeros((0, 5, 3)), damping=lam).shape == (0, robot.dof)


# ---- 6. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    robot = RobotWrapper(ROBOTS["allegro_hand_right"])
    model = robot.pose_model(["link_15.0_tip", "link_3.0_tip"])
    B = 4
    x = torch.zeros((B, robot.dof), dtype=torch.float32, device="cuda")
    e = torch.zeros((B, 2, 3), dtype=torch.float32, device="cuda")
    w = torch.ones((B, 2), dtype=torch.float32, device="cuda")
    out = _nan(torch, (B, robot.dof))
    h, xp, ep, wp, op = model.handle, x.data_ptr(), e.data_ptr(), w.data_ptr(), out.data_ptr()
    INVALID = -1

    def invalid(rc, word=None):
        assert rc == INVALID
        msg = lib.dexr_last_error()
        assert len(msg) > 0 and (word is None or word in msg), msg

    ik = lib.dexr_link_ik_step_dev
    invalid(ik(None, B, xp, None, WORLD, ep, ep, wp, wp, 1e-3, op, None), b"null pose model")
    invalid(ik(h, -1, xp, None, WORLD, ep, ep, wp, wp, 1e-3, op, None), b"negative")
    invalid(ik(h, B, xp, None, 2, ep, ep, wp, wp, 1e-3, op, None), b"frame")
    invalid(ik(h, B, xp, None, -1, ep, ep, wp, wp, 1e-3, op, None), b"frame")
    invalid(ik(h, B, xp, None, WORLD, None, None, None, None, 1e-3, op, None), b"error are both NULL")
    invalid(ik(h, B, xp, None, WORLD, ep, ep, wp, wp, 1e-3, None, None), b"dx_out is NULL")
    invalid(ik(h, B, None, None, WORLD, ep, ep, wp, wp, 1e-3, op, None), b"x is NULL")
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        invalid(ik(h, B, xp, None, LOCAL, ep, ep, wp, wp, bad, op, None), b"damping")
    invalid(ik(h, B, xp, None, WORLD, None, ep, wp, None, 1e-3, op, None), b"w_lin given without err_lin")
    invalid(ik(h, B, xp, None, WORLD, ep, None, None, wp, 1e-3, op, None), b"w_ang given without err_ang")
    # a table that reads fixed columns
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.pose_model(("link_15.0_tip", "link_3.0_tip"))
    assert ms.n_fixed == 6 and ms.n_in == 10
    invalid(ik(ms.handle, B, xp, None, WORLD, ep, ep, wp, wp, 1e-3, op, None), b"fixed")
    # the host twin keeps the same rules
    z, ze, zw = np.zeros((B, robot.dof)), np.zeros((B, 2, 3)), np.ones((B, 2))
    zp, zep, zwp = (a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)) for a in (z, ze, zw))
    hk = lib.dexr_link_ik_step
    invalid(hk(None, B, zp, None, WORLD, zep, None, None, None, 1e-3, zp), b"null pose model")
    invalid(hk(h, -2, zp, None, WORLD, zep, None, None, None, 1e-3, zp), b"negative")
    invalid(hk(h, B, zp, None, 7, zep, None, None, None, 1e-3, zp), b"frame")
    invalid(hk(h, B, zp, None, WORLD, None, None, None, None, 1e-3, zp), b"error are both NULL")
    invalid(hk(h, B, zp, None, WORLD, zep, None, None, None, 1e-3, None), b"dx_out is NULL")
    invalid(hk(h, B, None, None, WORLD, zep, None, None, None, 1e-3, zp), b"x is NULL")
    invalid(hk(h, B, zp, None, WORLD, zep, None, None, zwp, 1e-3, zp), b"w_ang given without err_ang")
    invalid(hk(h, B, zp, None, WORLD, None, zep, zwp, None, 1e-3, zp), b"w_lin given without err_lin")
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        invalid(hk(h, B, zp, None, WORLD, zep, None, None, None, bad, zp), b"damping")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # nothing was launched
    with pytest.raises(ValueError, match="shape"):
        model.ik_step(z, err_lin=np.zeros((B, 3, 3)), damping=1e-3)
    with pytest.raises(ValueError, match="shape"):
        model.ik_step(z, err_lin=ze, w_lin=np.ones((B, 3)), damping=1e-3)
    with pytest.raises(ValueError, match="damping"):
        model.ik_step(z, err_lin=ze)


# ---- 7. torch front ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_torch_front_equals_the_entry_points_bitwise(rel, require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import jacobians as jac

    opt, prob = _optimizer_and_problem(rel)
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_11.0_tip"]
    B, lam = 130, 2e-3
    x, fixed = _opt_inputs(prob, B, 93)
    gen = torch.Generator("cuda").manual_seed(8)
    f = torch.tensor(fixed.astype(np.float32), device="cuda") if fixed.shape[1] else None
    q = torch.tensor(x.astype(np.float32), device="cuda")
    pe, re = 0.01 * torch.randn((B, 4, 3), device="cuda", generator=gen), 0.1 * torch.randn((B, 4, 3), device="cuda", generator=gen)
    pw, rw = (0.5 + 1.5 * torch.rand((B, 4), device="cuda", generator=gen) for _ in range(2))
    model = opt.pose_model(tips)
    robot = opt.robot
    qr = torch.tensor(_configs(robot, B, 94).astype(np.float32), device="cuda")
    rmodel = robot.pose_model(tips)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = side.cuda_stream
        for frame, fid in (("world", WORLD), ("local", LOCAL)):
            for a, b, c, d in ((pe, re, pw, rw), (pe, None, None, None), (None, re, None, rw)):
                dq = jac.link_ik_step(opt, q, tips, a, b, c, d, lam, f, frame)
                want = _nan(torch, q.shape)
                model.ik_step_dev(B, q.data_ptr(), _ptr(f), _ptr(a), _ptr(b), _ptr(c), _ptr(d), lam, want.data_ptr(), frame=fid, stream=sp)
                assert dq.shape == (B, opt.opt_dof) and dq.dtype == torch.float32 and not dq.requires_grad
                assert torch.equal(dq, want) and bool(torch.isfinite(dq).all())
                dr = jac.robot_link_ik_step(robot, qr, tips, a, b, c, d, damping=lam, frame=frame)
                want = _nan(torch, qr.shape)
                rmodel.ik_step_dev(B, qr.data_ptr(), 0, _ptr(a), _ptr(b), _ptr(c), _ptr(d), lam, want.data_ptr(), frame=fid, stream=sp)
                assert dr.shape == (B, robot.dof) and torch.equal(dr, want)
            # non-contiguous inputs: views with the same values
            qn = torch.stack([q, q], 2)[:, :, 0]
            pen = torch.stack([pe, pe], 3)[..., 0]
            pwn = pw.t().contiguous().t()
            fn = None if f is None else torch.stack([f, f], 2)[:, :, 1]
            assert not qn.is_contiguous() and not pen.is_contiguous() and not pwn.is_contiguous()
            assert torch.equal(jac.link_ik_step(opt, qn, tips, pen, None, pwn, damping=lam, fixed_qpos=fn, frame=frame),
                               jac.link_ik_step(opt, q, tips, pe, None, pw, damping=lam, fixed_qpos=f, frame=frame))
            # a q that requires grad: the step carries no graph
            assert not jac.link_ik_step(opt, q.clone().requires_grad_(True), tips, pe, damping=lam, fixed_qpos=f, frame=frame).requires_grad
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e = torch.zeros((0, opt.opt_dof), device="cuda")
    assert jac.link_ik_step(opt, e, tips, pe[:0], damping=lam, fixed_qpos=None if f is None else f[:0]).shape == (0, opt.opt_dof)


# ---- 8. tracking loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_tracking_loop_follows_the_numpy_loop_and_descends(name, require_gpu):
    orc, links, q_star, q0, damping = tracking_inputs(name)
    xs, _ = ikr.tracking_loop(orc, q0, q_star, links, damping, TRACK_STEPS)
    model = RobotWrapper(ROBOTS[name]).pose_model(links)
    target = model.poses(q_star, rotations=False)[0]
    x, errs, worst = q0.copy(), [], 0.0
    for k in range(TRACK_STEPS):
        e = target - model.poses(x, rotations=False)[0]
        errs.append(np.linalg.norm(e.reshape(len(x), -1), axis=1))
        x = x + model.ik_step(x, err_lin=e, damping=damping)
        worst = max(worst, float(np.abs(x - xs[k + 1]).max()))
        assert np.abs(x - xs[k + 1]).max() <= 1e-9, (name, k)
    errs.append(np.linalg.norm((target - model.poses(x, rotations=False)[0]).reshape(len(x), -1), axis=1))
    errs = np.stack(errs)
    print(f"{name}: largest |iterate - numpy loop's| over {TRACK_STEPS} steps = {worst:.3e}; error after / before, worst frame "
          f"{float((errs[-1] / np.maximum(errs[0], 1e-300)).max()):.3e}")
    assert_descends(errs, target, name)

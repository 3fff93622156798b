"""GPU tests of the IK solve to link pose targets (csrc/dexr_pose.hip, include/dexr_ik_solve.h): the float64 host entry point
against tests/ik_solve_reference.py (final answers, intermediate iterates, the per-frame stop), the float32 device entry point
against the float64 host twin, the table limits on the synthetic robots of tests/pose_zoo.py, row independence and isolation,
the raw ABI's argument errors and the torch front.

INPUTS.  The eight fixture robots run the two input sets of tests/test_ik_solve_host.py (solve_inputs: "near" and "tight", B = 33,
the last five links), whose reference runs are proven there on the CPU and shared from there.  Tables with a source map
(optimizer order, the zoo) get table_inputs below: x* as the existing tests draw it, targets = the poses of x*, start = x* +
U(-pert, pert), bounds 0.01 inside the smallest and the largest start of each column (so every column has frames on both
bounds, about half of which the gradient pushes outward), max_step = 0.2.

GATES.  float64: 1e-9 absolute (radians and metres) on x and err, iters equal: the gate of the tracking test of
tests/test_gpu_ik.py.  float32: max |x32 - x64| may be 8 x the distance between the reference's own float32 and float64 runs
(the step test's factor; both runs round the float64 targets, which is most of that distance).  The ratios are printed; those
of the MI355X are in docs/experiments/link_ik_solve.md."""
import functools

import numpy as np
import pytest

import ik_solve_reference as isr
import pose_zoo as zoo
import test_gpu_link_poses as glp
from dex_retargeting_amd import _lib
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from oracle.kin import OracleRobot
from test_gpu_link_jacobians import OPT_ORDER, _fold4, _opt_inputs, _optimizer_and_problem, oracle_jacobians
from test_ik_solve_host import KINDS, STEPS, reference, solve_inputs
from test_jacobian_host import SUBSET_CFG

pytestmark = pytest.mark.gpu
ROBOTS = glp.ROBOTS
GATE64 = 1e-9


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def table_inputs(orc, links, x_star, full, fold, pert, seed):
    """the input dict of solve_inputs for a table with a source map (see the module docstring)."""
    rng = np.random.default_rng(seed)
    B, L = x_star.shape[0], len(links)
    x0 = _r32(x_star + rng.uniform(-pert, pert, x_star.shape))
    lo, hi = _r32(x0.min(0) + 0.01), _r32(x0.max(0) - 0.01)
    flat = hi <= lo  # (a column whose starts lie within 0.02: bounds it never meets)
    lo[flat], hi[flat] = x0.min(0)[flat] - 1.0, x0.max(0)[flat] + 1.0
    x0 = np.clip(x0, lo, hi)
    tgt_pos, tgt_rot = isr.link_poses(orc, full(x_star), links)
    jl = fold(oracle_jacobians(orc, full(x0), links)[0])
    damping = float(np.float32(1e-3 * float(np.linalg.eigvalsh(np.einsum("blri,blrj->bij", jl, jl))[:, -1].max())))
    assert damping > 0
    return dict(orc=orc, links=list(links), x0=x0, tgt_pos=tgt_pos, tgt_rot=tgt_rot, w_lin=_r32(rng.uniform(0.5, 2, (B, L))),
                w_ang=_r32(0.01 * rng.uniform(0.5, 2, (B, L))), lo=lo, hi=hi, damping=damping, max_step=0.2, full=full, fold=fold)


def ref_run(d, max_iters, tol=0.0, dtype=np.float64):
    return isr.ik_solve(d["orc"], d["x0"], d["links"], d["tgt_pos"], d["tgt_rot"], d["w_lin"], d["w_ang"], d["lo"], d["hi"], d["damping"],
                        max_iters, tol, d["max_step"], dtype, d.get("full"), d.get("fold"))


def host_run(model, d, max_iters, tol=0.0, fixed=None):
    return model.ik_solve(d["x0"], fixed, d["tgt_pos"], d["tgt_rot"], d["w_lin"], d["w_ang"], d["lo"], d["hi"], d["damping"], max_iters,
                          tol, d["max_step"])


# ---- the float32 device entry point on numpy arrays, the outputs pre-filled with NaN / -7 -------------------------------------------
def _dev(torch, a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def dev_run(model, torch, d, max_iters, tol=0.0, fixed=None, rows=slice(None), alias=False, **over):
    """-> (x, iters, err) of dexr_link_ik_solve_dev on the frames `rows` of d; alias: x_out is x0's buffer."""
    a = dict(d, **over)
    cut = lambda v: None if v is None else v[rows]  # noqa: E731
    x0, tf, tp, tr, wl, wa = (_dev(torch, cut(a[k]) if k != "fixed" else cut(fixed)) for k in ("x0", "fixed", "tgt_pos", "tgt_rot", "w_lin", "w_ang"))
    lo, hi = _dev(torch, a["lo"]), _dev(torch, a["hi"])
    B = x0.shape[0]
    x = x0 if alias else _nan(torch, (B, model.n_in))
    iters = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    err = _nan(torch, (B,))
    model.ik_solve_dev(B, _ptr(x0), _ptr(tf), _ptr(tp), _ptr(tr), _ptr(wl), _ptr(wa), _ptr(lo), _ptr(hi), a["damping"], max_iters, _ptr(x),
                       _ptr(iters), _ptr(err), tol=tol, max_step=a["max_step"], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return x.cpu().numpy(), iters.cpu().numpy(), err.cpu().numpy()


@functools.lru_cache(maxsize=None)
def robot_model(name):
    return RobotWrapper(ROBOTS[name]).pose_model(solve_inputs(name, "near")["links"])


ZERO = 1e-12  # an error below this is a rounding of zero (64 eps max |target| = 3e-15 for a hand; the gate is 1e-9)


def _compare64(tag, got, want_x, want_iters, want_err, errs=None):
    """x and err within GATE64, iters equal.  `errs` (iterations + 1, B), the reference's errors, is given by the runs with
    tol = 0, where a frame stops early only when its E is an EXACT zero: whether the last rounding lands on 0 or on 1e-17 is
    noise (on the MI355X the ability hand's frames went on to max_iters where numpy met 0.0 at iteration 7).  There iters must
    equal the reference's on every frame whose reference error stays above ZERO, and be no smaller than the first iteration
    at which it is below ZERO on the others."""
    x, iters, err = got
    if errs is not None:
        first_zero = np.where((errs <= ZERO).any(0), (errs <= ZERO).argmax(0), len(errs))
        noise = first_zero <= want_iters
        assert (iters[noise] >= first_zero[noise]).all() and (iters[noise] <= len(errs) - 1).all(), tag
        want_iters = np.where(noise, iters, want_iters).astype(np.int32)
    ex, ee = float(np.abs(x - want_x).max()), float(np.abs(err - want_err).max())
    print(f"{tag}: float64 max |x - reference| = {ex:.3e}, max |err - reference| = {ee:.3e} (gate {GATE64:.0e}), iters {np.bincount(iters).tolist()}")
    assert x.shape == want_x.shape and np.isfinite(x).all() and np.isfinite(err).all()
    assert iters.dtype == np.int32 and np.array_equal(iters, want_iters), tag
    assert ex <= GATE64 and ee <= GATE64, (tag, ex, ee)


# ---- 1. float64 host twin against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_host_float64_against_the_reference(name, require_gpu):
    assert len(ROBOTS) == 8
    for kind in KINDS:
        d = solve_inputs(name, kind)
        xs, _, iters, errs = reference(name, kind)
        _compare64(f"{name} {kind}", host_run(robot_model(name), d, STEPS), xs[-1], iters, errs[-1], errs)


@pytest.mark.parametrize("rel", OPT_ORDER + ["subset"])
def test_host_float64_optimizer_order_folds_mimic_and_fixed_joints(rel, require_gpu):
    opt, prob = _optimizer_and_problem(rel)
    # (the last five frames; the ten-variable subset drives those through `fixed` alone, it takes four finger tips instead)
    links = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_11.0_tip"] if rel == "subset" else [f.name for f in opt.robot.kin.frames][-5:]
    x_star, fixed = (_r32(a) for a in _opt_inputs(prob, 33, 183))
    model = opt.pose_model(links)
    assert (model.n_in, model.n_fixed) == (opt.opt_dof, len(opt.idx_pin2fixed))
    if rel == "subset":
        assert model.n_fixed == 6
    fixed = fixed if fixed.shape[1] else None
    d = table_inputs(prob.robot, links, x_star, lambda x: prob.full_qpos(x, fixed), lambda J: _fold4(prob, J), 0.1, 184)
    xs, frozen, iters, errs = ref_run(d, STEPS)
    assert frozen.any() and (errs[-1] < errs[0]).all() and isr.active_columns(prob.robot, d["full"](d["x0"]), links, d["fold"]).any()
    _compare64(rel, host_run(model, d, STEPS, fixed=fixed), xs[-1], iters, errs[-1], errs)


# ---- 2. intermediate iterates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_one_two_and_three_iterations_reproduce_the_reference_iterates(name, require_gpu):
    for kind in KINDS:
        d = solve_inputs(name, kind)
        xs, _, iters, errs = reference(name, kind)
        for n in (1, 2, 3):
            assert (iters >= n).all()  # no frame has stopped by then: iterate n of the long run is the answer of the short one
            _compare64(f"{name} {kind} max_iters={n}", host_run(robot_model(name), d, n), xs[n], np.full(len(iters), n, np.int32), errs[n])
        # the iterates are still ten gates apart (the gripper, the fastest: 5e-8): a loop that runs one short or one long fails
        assert np.abs(xs[3] - xs[2]).max() > 10 * GATE64, (name, kind)


# ---- 3. stopping ----------------------------------------------------------------------------------------------------------------------
def stop_tolerance(errs):
    """the geometric mean of the two middle values of the sorted step-3 errors: about half of the frames stop there."""
    e = np.sort(errs[3])
    return float(np.sqrt(e[len(e) // 2 - 1] * e[len(e) // 2]))


def _stopping_reference(d, tol_from):
    tol = stop_tolerance(tol_from)
    xs, _, iters, errs = ref_run(d, STEPS, tol)
    assert tol > 0 and not ((errs > tol / 1.01) & (errs < tol * 1.01)).any()  # no decision hangs on rounding
    assert len(np.unique(iters)) >= 2, np.bincount(iters)
    return tol, xs, iters, errs


NO_TOL = {"ability_hand_right", "inspire_hand_right"}  # an error of the reference run lies within 1 % of the recipe's tol on these two


@pytest.mark.parametrize("name", sorted(set(ROBOTS) - NO_TOL))
def test_frames_stop_where_the_reference_stops_them(name, require_gpu):
    """six robots: on the other two the step-3 errors crowd around their median (neighbours 1 % apart), so the recipe's tol
    would sit where rounding decides a stop; _stopping_reference asserts that it does not, on the inputs alone."""
    d = solve_inputs(name, "near")
    tol, xs, iters, errs = _stopping_reference(d, reference(name, "near")[3])
    x, it, err = host_run(robot_model(name), d, STEPS, tol)
    print(f"{name}: tol {tol:.3e}, frames per iteration count {np.bincount(iters, minlength=STEPS + 1).tolist()}")
    _compare64(f"{name} tol", (x, it, err), xs[-1], iters, errs[-1])
    assert (err[it < STEPS] <= tol).all() and (it >= 1).all()


# ---- 4. float32 device entry point against the float64 host twin -------------------------------------------------------------------
GATE32 = 8.0


@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_host_twin(name, require_gpu):
    torch = pytest.importorskip("torch")
    for kind in KINDS:
        d = solve_inputs(name, kind)
        x64 = host_run(robot_model(name), d, STEPS)[0]
        dist = float(np.abs(reference(name, kind, np.float32)[0][-1].astype(np.float64) - reference(name, kind)[0][-1]).max())
        x, iters, err = dev_run(robot_model(name), torch, d, STEPS)
        assert x.dtype == np.float32 and np.isfinite(x).all() and np.isfinite(err).all() and (iters >= 0).all() and (iters <= STEPS).all()
        e = float(np.abs(x - x64).max())
        ratio = e / dist if dist > 0 else (0.0 if e == 0 else float("inf"))
        print(f"{name} {kind}: float32 max |x - host| = {e:.3e}, the reference's float32 run is {dist:.3e} from its float64 run "
              f"(error / reference distance {ratio:.2f}, gate {GATE32:g})")
        act = isr.active_columns(d["orc"], d["x0"], d["links"])
        lo, hi = d["lo"].astype(np.float32), d["hi"].astype(np.float32)
        assert ((x[:, act] >= lo[act]) & (x[:, act] <= hi[act])).all(), (name, kind, "an active entry is outside its bounds")
        assert np.array_equal(x[:, ~act], d["x0"][:, ~act].astype(np.float32))
        assert ratio <= GATE32, (name, kind, e, dist)


# ---- 5. table limits: the synthetic robots of tests/pose_zoo.py ----------------------------------------------------------------------
ZOO = ["chain64", "binary64", "binary64_slots8", "star40", "two_trees100_b", "wide_map"]
ZB, ZITERS = 33, 3  # float32: 4 frames per block on the 64-link members, float64 2: ragged tails of 1


@pytest.fixture(scope="module")
def zoo_tables(tmp_path_factory):
    d, made = tmp_path_factory.mktemp("ik_solve_zoo"), {}

    def get(name):
        if name not in made:
            m = zoo.build(name, d)
            x, fixed, _ = zoo.inputs(m, ZB, 2031)
            inp = table_inputs(m.orc, m.links, x, (lambda v, m=m, fixed=fixed: zoo.full_q(m.smap, v, fixed)), (lambda J, m=m: zoo.fold(m.smap, J)),
                               0.02, 2033)
            made[name] = (m, _lib.PoseModel(m.blob), fixed, inp)
        return made[name]

    return get


@pytest.mark.parametrize("name", ZOO)
def test_table_limits_float64(name, zoo_tables, require_gpu):
    m, model, fixed, d = zoo_tables(name)
    assert (model.n_in, model.n_link) == (zoo.FACTS[name]["n_in"], zoo.FACTS[name]["n_link"])
    xs, frozen, iters, errs = ref_run(d, ZITERS)
    assert frozen.any() and (iters == ZITERS).all()
    got = host_run(model, d, ZITERS, fixed=fixed)
    _compare64(name, got, xs[-1], iters, errs[-1])
    unread = zoo.abs_mult(m).sum(0) == 0
    assert np.array_equal(got[0][:, unread], d["x0"][:, unread])
    if name == "wide_map":
        assert model.n_in == 256 and int(unread.sum()) == 233
    if name == "star40":  # three links on the fixed base: they never move, their error counts
        assert int((m.tab["links"]["parent"] == -1).sum()) == 3


def test_slots_three_to_seven_give_the_bits_of_slots_zero_to_four(zoo_tables, require_gpu):
    torch = pytest.importorskip("torch")
    (_, ma, fa, da), (mb, mbm, fb, db) = zoo_tables("binary64"), zoo_tables("binary64_slots8")
    assert int(mb.tab["h"]["n_slot"]) == 8
    assert all(np.array_equal(da[k], db[k]) for k in ("x0", "tgt_pos", "tgt_rot", "w_lin", "w_ang", "lo", "hi")) and da["damping"] == db["damping"]
    for a, b in zip(host_run(ma, da, ZITERS, fixed=fa), host_run(mbm, db, ZITERS, fixed=fb)):
        assert np.array_equal(a, b), "float64"
    for a, b in zip(dev_run(ma, torch, da, ZITERS, fixed=fa), dev_run(mbm, torch, db, ZITERS, fixed=fb)):
        assert np.array_equal(a, b) and np.isfinite(a).all(), "float32"


# ---- 6. row independence and isolation ---------------------------------------------------------------------------------------------
def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    name, tips, B = "shadow_hand_right", ["thtip", "fftip", "mftip", "rftip", "lftip"], 130
    orc = OracleRobot(ROBOTS[name])
    lim = orc.joint_limits
    rng = np.random.default_rng(191)
    q_star = _r32(rng.uniform(lim[:, 0], lim[:, 1], (B, orc.dof)))
    lo, hi = _r32(lim[:, 0]), _r32(lim[:, 1])
    x0 = np.clip(_r32(q_star + rng.uniform(-0.1, 0.1, q_star.shape)), lo, hi)
    tgt_pos, tgt_rot = isr.link_poses(orc, q_star, tips)
    jl = oracle_jacobians(orc, x0, tips)[0]
    d = dict(orc=orc, links=tips, x0=x0, tgt_pos=tgt_pos, tgt_rot=tgt_rot, w_lin=_r32(rng.uniform(0.5, 2, (B, 5))),
             w_ang=_r32(0.01 * rng.uniform(0.5, 2, (B, 5))), lo=lo, hi=hi, max_step=0.0,
             damping=float(np.float32(1e-3 * float(np.linalg.eigvalsh(np.einsum("blri,blrj->bij", jl, jl))[:, -1].max()))))
    # tol by the recipe of the stopping test.  (130 frames of this slowly converging set leave some twenty errors within 1 % of
    # it, whatever the seed: no matter here, every comparison below is between two runs of the device, bit for bit)
    tol = stop_tolerance(ref_run(d, STEPS)[3])
    model = RobotWrapper(ROBOTS[name]).pose_model(tips)
    X, IT, ERR = dev_run(model, torch, d, STEPS, tol)  # B = 130: eight full blocks of 16 frames and a ragged one
    print(f"shadow tips: tol {tol:.3e}, float32 frames per iteration count {np.bincount(IT, minlength=STEPS + 1).tolist()}")
    assert np.isfinite(X).all() and np.isfinite(ERR).all() and len(np.unique(IT)) >= 2
    assert any(len(np.unique(IT[b:b + 16])) >= 2 for b in range(0, B, 16))  # block neighbours stop at different iterations
    for a, b in ((0, 1), (0, 63), (0, 64), (65, 130), (129, 130)):  # B = 1, 63, 64, 65, 1
        x, it, err = dev_run(model, torch, d, STEPS, tol, rows=slice(a, b))
        assert np.array_equal(x, X[a:b]) and np.array_equal(it, IT[a:b]) and np.array_equal(err, ERR[a:b]), (a, b)
    # x_out aliasing x0
    x, it, err = dev_run(model, torch, d, STEPS, tol, alias=True)
    assert np.array_equal(x, X) and np.array_equal(it, IT) and np.array_equal(err, ERR)
    # a NaN in the target of frame 7: that frame runs to max_iters and is not finite, every other row keeps its bits
    bad = tgt_pos.copy()
    bad[7, 2, 1] = np.nan
    x, it, err = dev_run(model, torch, d, STEPS, tol, tgt_pos=bad)
    keep = np.arange(B) != 7
    assert it[7] == STEPS and not (np.isfinite(x[7]).all() and np.isfinite(err[7]))
    assert np.array_equal(x[keep], X[keep]) and np.array_equal(it[keep], IT[keep]) and np.array_equal(err[keep], ERR[keep])
    # all-zero weights: the start comes back, after no iteration, with no error
    x, it, err = dev_run(model, torch, d, STEPS, tol, w_lin=np.zeros((B, 5)), w_ang=np.zeros((B, 5)))
    assert np.array_equal(x, x0.astype(np.float32)) and not it.any() and not err.any()
    # B = 0: a no-op, NULL pointers and all
    lib = _lib.load()
    assert lib.dexr_link_ik_solve_dev(model.handle, 0, None, None, None, None, None, None, None, None, 1e-3, 0.0, 0.0, 8, None, None, None, None) == 0
    assert lib.dexr_link_ik_solve(model.handle, 0, None, None, None, None, None, None, None, None, 1e-3, 0.0, 0.0, 8, None, None, None) == 0
    x, it, err = model.ik_solve(np.zeros((0, orc.dof)), tgt_pos=np.zeros((0, 5, 3)), damping=1e-3, max_iters=8)
    assert x.shape == (0, orc.dof) and it.shape == (0,) and err.shape == (0,)


# ---- 7. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    robot = RobotWrapper(ROBOTS["allegro_hand_right"])
    model = robot.pose_model(["link_15.0_tip", "link_3.0_tip"])
    B = 4
    x = torch.zeros((B, robot.dof), dtype=torch.float32, device="cuda")
    p = torch.zeros((B, 2, 3), dtype=torch.float32, device="cuda")
    r = torch.eye(3, dtype=torch.float32, device="cuda").expand(B, 2, 3, 3).contiguous()
    w = torch.ones((B, 2), dtype=torch.float32, device="cuda")
    b = torch.ones((robot.dof,), dtype=torch.float32, device="cuda")
    out, eo = _nan(torch, (B, robot.dof)), _nan(torch, (B,))
    it = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    h, xp, pp, rp, wp, lp, hp, op, ip, ep = (model.handle, x.data_ptr(), p.data_ptr(), r.data_ptr(), w.data_ptr(), (-b).data_ptr(), b.data_ptr(),
                                             out.data_ptr(), it.data_ptr(), eo.data_ptr())
    INVALID = -1

    def invalid(rc, word=None):
        assert rc == INVALID
        msg = lib.dexr_last_error()
        assert len(msg) > 0 and (word is None or word in msg), msg

    def dev(m=h, n=B, x0=xp, fixed=None, tp=pp, tr=rp, wl=wp, wa=wp, lo=lp, hi=hp, damping=1e-3, max_step=0.0, tol=0.0, max_iters=8, xo=op):
        return lib.dexr_link_ik_solve_dev(m, n, x0, fixed, tp, tr, wl, wa, lo, hi, damping, max_step, tol, max_iters, xo, ip, ep, None)

    invalid(dev(m=None), b"null pose model")
    invalid(dev(n=-1), b"negative")
    invalid(dev(tp=None, tr=None, wl=None, wa=None), b"both NULL")
    invalid(dev(tp=None, wa=None), b"w_lin given without tgt_pos")
    invalid(dev(tr=None, wl=None), b"w_ang given without tgt_rot")
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        invalid(dev(damping=bad), b"damping")
    invalid(dev(x0=None), b"x0 is NULL")
    invalid(dev(xo=None), b"x_out is NULL")
    invalid(dev(lo=None), b"lo and hi")
    invalid(dev(hi=None), b"lo and hi")
    for bad in (0, -1, 257, 1 << 20):
        invalid(dev(max_iters=bad), b"max_iters")
    for bad in (-1e-6, float("nan"), float("inf"), -float("inf")):
        invalid(dev(tol=bad), b"tol")
        invalid(dev(max_step=bad), b"max_step")
    # a table that reads fixed columns
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.pose_model(("link_15.0_tip", "link_3.0_tip"))
    assert ms.n_fixed == 6 and ms.n_in == 10
    invalid(dev(m=ms.handle), b"fixed")
    # the host twin keeps the same rules
    z, zp, zr, zw, zb = np.zeros((B, robot.dof)), np.zeros((B, 2, 3)), np.tile(np.eye(3), (B, 2, 1, 1)), np.ones((B, 2)), np.ones(robot.dof)
    zo, zi, ze = np.full((B, robot.dof), np.nan), np.full(B, -7, np.int32), np.full(B, np.nan)
    dp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    zip_ = zi.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))

    def host(m=h, n=B, x0=dp(z), tp=dp(zp), tr=dp(zr), wl=dp(zw), wa=dp(zw), lo=dp(-zb), hi=dp(zb), damping=1e-3, max_step=0.0, tol=0.0, max_iters=8,
             xo=dp(zo)):
        return lib.dexr_link_ik_solve(m, n, x0, None, tp, tr, wl, wa, lo, hi, damping, max_step, tol, max_iters, xo, zip_, dp(ze))

    invalid(host(m=None), b"null pose model")
    invalid(host(n=-2), b"negative")
    invalid(host(tp=None, tr=None, wl=None, wa=None), b"both NULL")
    invalid(host(tp=None, wa=None), b"w_lin given without tgt_pos")
    invalid(host(tr=None, wl=None), b"w_ang given without tgt_rot")
    invalid(host(x0=None), b"x0 is NULL")
    invalid(host(xo=None), b"x_out is NULL")
    invalid(host(lo=None), b"lo and hi")
    invalid(host(hi=None), b"lo and hi")
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        invalid(host(damping=bad), b"damping")
    for bad in (0, 257, -3):
        invalid(host(max_iters=bad), b"max_iters")
    for bad in (-1.0, float("nan"), float("inf")):
        invalid(host(tol=bad), b"tol")
        invalid(host(max_step=bad), b"max_step")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(eo).all()) and bool((it == -7).all())  # nothing was launched
    assert np.isnan(zo).all() and np.isnan(ze).all() and (zi == -7).all()
    with pytest.raises(ValueError, match="shape"):
        model.ik_solve(z, tgt_pos=np.zeros((B, 3, 3)), damping=1e-3, max_iters=8)
    with pytest.raises(ValueError, match="shape"):
        model.ik_solve(z, tgt_rot=zp, damping=1e-3, max_iters=8)
    with pytest.raises(ValueError, match="shape"):
        model.ik_solve(z, tgt_pos=zp, lo=-zb[:3], hi=zb[:3], damping=1e-3, max_iters=8)
    with pytest.raises(ValueError, match="lo and hi"):
        model.ik_solve(z, tgt_pos=zp, lo=-zb, damping=1e-3, max_iters=8)
    with pytest.raises(ValueError, match="damping"):
        model.ik_solve(z, tgt_pos=zp, max_iters=8)
    with pytest.raises(ValueError, match="max_iters"):
        model.ik_solve(z, tgt_pos=zp, damping=1e-3)


# ---- 8. torch front ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_torch_front_equals_the_entry_points_bitwise(rel, require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import jacobians as jac

    opt, prob = _optimizer_and_problem(rel)
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_11.0_tip"]
    B, lam, n, tol, step = 130, 2e-3, 6, 1e-3, 0.2
    x, fixed = _opt_inputs(prob, B, 193)
    gen = torch.Generator("cuda").manual_seed(9)
    f = torch.tensor(fixed.astype(np.float32), device="cuda") if fixed.shape[1] else None
    q = torch.tensor(x.astype(np.float32), device="cuda")
    model, robot = opt.pose_model(tips), opt.robot
    rmodel = robot.pose_model(tips)
    rl = robot.joint_limits
    qr = torch.tensor(np.random.default_rng(194).uniform(rl[:, 0], rl[:, 1], (B, robot.dof)).astype(np.float32), device="cuda")
    rlim = torch.tensor(rl.astype(np.float32), device="cuda")
    lim = torch.tensor(prob.robot.joint_limits[prob.idx_pin2target].astype(np.float32), device="cuda")
    # targets: the poses of a perturbed configuration, by the library's own forward kernel
    tp, tr = (torch.empty((B, 4, 3), device="cuda"), torch.empty((B, 4, 3, 3), device="cuda"))
    qt = (q + 0.1 * (torch.rand(q.shape, device="cuda", generator=gen) - 0.5)).contiguous()
    model.poses_dev(B, qt.data_ptr(), _ptr(f), tp.data_ptr(), tr.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    pw, rw = (0.5 + 1.5 * torch.rand((B, 4), device="cuda", generator=gen) for _ in range(2))
    rw = 0.01 * rw
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def raw(m, x0, fx, a, b, c, d, lm, sp):
        want, wi, we = _nan(torch, x0.shape), torch.full((B,), -7, dtype=torch.int32, device="cuda"), _nan(torch, (B,))
        lo, hi = (None, None) if lm is None else (lm[:, 0].contiguous(), lm[:, 1].contiguous())
        m.ik_solve_dev(B, x0.data_ptr(), _ptr(fx), _ptr(a), _ptr(b), _ptr(c), _ptr(d), _ptr(lo), _ptr(hi), lam, n, want.data_ptr(), wi.data_ptr(),
                       we.data_ptr(), tol=tol, max_step=step, stream=sp)
        return want, wi, we

    with torch.cuda.stream(side):
        sp = side.cuda_stream
        for a, b, c, d, lm in ((tp, tr, pw, rw, lim), (tp, None, None, None, None), (None, tr, None, rw, lim)):
            got = jac.link_ik_solve(opt, q, tips, a, b, c, d, lam, n, tol, step, lm, f)
            want = raw(model, q, f, a, b, c, d, lm, sp)
            assert got[0].shape == (B, opt.opt_dof) and got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].shape == (B,)
            assert all(torch.equal(u, v) and not u.requires_grad for u, v in zip(got, want)) and bool(torch.isfinite(got[0]).all())
            gr = jac.robot_link_ik_solve(robot, qr, tips, a, b, c, d, damping=lam, max_iters=n, tol=tol, max_step=step,
                                         limits=None if lm is None else rlim)
            wr = raw(rmodel, qr, None, a, b, c, d, None if lm is None else rlim, sp)
            assert gr[0].shape == (B, robot.dof) and all(torch.equal(u, v) for u, v in zip(gr, wr))
        # non-contiguous inputs: views with the same values
        qn = torch.stack([q, q], 2)[:, :, 0]
        tpn = torch.stack([tp, tp], 3)[..., 0]
        trn = tr.transpose(2, 3).contiguous().transpose(2, 3)
        pwn = pw.t().contiguous().t()
        limn = torch.stack([lim, lim], 2)[:, :, 1]
        fn = None if f is None else torch.stack([f, f], 2)[:, :, 1]
        assert not any(t.is_contiguous() for t in (qn, tpn, trn, pwn, limn))
        a = jac.link_ik_solve(opt, qn, tips, tpn, trn, pwn, rw, damping=lam, max_iters=n, limits=limn, fixed_qpos=fn)
        b = jac.link_ik_solve(opt, q, tips, tp, tr, pw, rw, damping=lam, max_iters=n, limits=lim, fixed_qpos=f)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        # a q0 that requires grad: the outputs carry no graph
        assert not any(t.requires_grad for t in jac.link_ik_solve(opt, q.clone().requires_grad_(True), tips, tp, damping=lam, max_iters=n, fixed_qpos=f))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e = torch.zeros((0, opt.opt_dof), device="cuda")
    out = jac.link_ik_solve(opt, e, tips, tp[:0], damping=lam, max_iters=n, fixed_qpos=None if f is None else f[:0])
    assert out[0].shape == (0, opt.opt_dof) and out[1].shape == (0,) and out[2].shape == (0,)

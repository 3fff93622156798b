"""GPU tests of the sphere-pair self-collision (csrc/dexr_spheres.hpp, include/dexr_spheres.h): the float64 host entry points and
the float32 device entry points against tests/collision_reference.py, optimizer order, row independence, the table limits on the
synthetic robots of tests/pose_zoo.py, the penalty against the VJP, the raw ABI's argument errors and the torch front.

INPUTS.  The eight fixture robots run the two sphere sets of tests/test_collision_host.py (collision_inputs: "origins" and
"offset", B = 33, margin 0.010), whose reference runs are proven there on the CPU and shared from there.

GATES.  float64: 1e-9 absolute (metres, metres per radian, square metres) on every output, the GATE64 of the IK tests.  float32:
max |out32 - reference64| of an output may be 8 x the distance between the reference's OWN float32 and float64 runs on that
output (the factor of the IK step and solve tests); where that distance is zero (the gripper's energy and gradient) the output
must be exact zeros.  The ratios are printed; those of the MI355X are in docs/experiments/sphere_collision.md."""
import numpy as np
import pytest

import collision_reference as cref
import ik_solve_reference as isr
import pose_zoo as zoo
import test_gpu_link_poses as glp
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, GRIPPER, MARGIN, ROBOTS, SETS, collision_inputs, reference, robot_of
from test_gpu_link_jacobians import OPT_ORDER, _fold4, _opt_inputs, _optimizer_and_problem
from test_jacobian_host import SUBSET_CFG

pytestmark = pytest.mark.gpu
GATE64, GATE32 = 1e-9, 8.0
OUTPUTS = ("dist", "centers", "vjp", "E", "grad")


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- the float32 device entry points on numpy arrays, the outputs pre-filled with NaN ------------------------------------------------
def _dev(torch, a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def dev_distances(model, torch, x, fixed=None, centers=True):
    xd, fd = _dev(torch, x), _dev(torch, fixed)
    n = xd.shape[0]
    dist, cen = _nan(torch, (n, model.n_pair)), (_nan(torch, (n, model.n_sphere, 3)) if centers else None)
    model.distances_dev(n, _ptr(xd), _ptr(fd), _ptr(dist), _ptr(cen), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), (None if cen is None else cen.cpu().numpy())


def dev_vjp(model, torch, x, gd, fixed=None):
    xd, fd, g = _dev(torch, x), _dev(torch, fixed), _dev(torch, gd)
    gx = _nan(torch, (xd.shape[0], model.n_in))
    model.distances_vjp_dev(xd.shape[0], _ptr(xd), _ptr(fd), _ptr(g), _ptr(gx), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return gx.cpu().numpy()


def dev_penalty(model, torch, x, margin, w=None, fixed=None, energy=True, grad=True):
    xd, fd, wd = _dev(torch, x), _dev(torch, fixed), _dev(torch, w)
    n = xd.shape[0]
    e, gx = (_nan(torch, (n,)) if energy else None), (_nan(torch, (n, model.n_in)) if grad else None)
    model.penalty_dev(n, _ptr(xd), _ptr(fd), margin, _ptr(wd), _ptr(e), _ptr(gx), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (None if e is None else e.cpu().numpy()), (None if gx is None else gx.cpu().numpy())


def host_all(model, x, gd, margin, w=None, fixed=None):
    dist, cen = model.distances(x, fixed, centers=True)
    E, grad = model.penalty(x, margin, w, fixed)
    return dict(dist=dist, centers=cen, vjp=model.distances_vjp(x, gd, fixed), E=E, grad=grad)


def dev_all(model, torch, x, gd, margin, w=None, fixed=None):
    dist, cen = dev_distances(model, torch, x, fixed)
    E, grad = dev_penalty(model, torch, x, margin, w, fixed)
    return dict(dist=dist, centers=cen, vjp=dev_vjp(model, torch, x, gd, fixed), E=E, grad=grad)


def ref_all(orc, q_full, links, rows, centers, radii, pairs, gd, margin, w=None, dtype=np.float64, fold=None):
    q_full = np.asarray(q_full, dtype)
    dist, c, _ = cref.distances(orc, q_full, links, rows, centers, radii, pairs, dtype)
    dd = cref.distance_jacobian(orc, q_full, links, rows, centers, radii, pairs, dtype, fold)
    ww = np.ones(len(pairs), dtype) if w is None else np.asarray(w, dtype)
    h = np.maximum(dtype(0), dtype(margin) - dist)
    return dict(dist=dist, centers=c, vjp=np.einsum("bp,bpc->bc", np.asarray(gd, dtype), dd), E=(ww * h * h).sum(-1),
                grad=np.einsum("bp,bpc->bc", dtype(-2) * ww * h, dd))


def compare64(tag, got, want):
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, (tag, k)
        e = float(np.abs(got[k] - want[k]).max())
        print(f"{tag}: float64 max |{k} - reference| = {e:.3e} (gate {GATE64:.0e})")
        assert np.isfinite(got[k]).all() and e <= GATE64, (tag, k, e)


def compare32(tag, got, want64, want32):
    """the gate of each output comes from the reference's own two runs, never from the code under test"""
    for k in OUTPUTS:
        assert got[k].shape == want64[k].shape and got[k].dtype == np.float32, (tag, k)
        dist = float(np.abs(want32[k].astype(np.float64) - want64[k]).max())
        e = float(np.abs(got[k].astype(np.float64) - want64[k]).max())
        ratio = e / dist if dist > 0 else (0.0 if e == 0 else float("inf"))
        print(f"{tag}: float32 max |{k} - reference64| = {e:.3e}, the reference's float32 run is {dist:.3e} from its float64 run "
              f"(error / reference distance {ratio:.2f}, gate {GATE32:g})")
        assert np.isfinite(got[k]).all(), (tag, k)
        if dist == 0:
            assert not got[k].any(), (tag, k, "exact zeros expected")
        assert ratio <= GATE32, (tag, k, e, dist)


def robot_model(name, kind):
    return robot_of(name)[0].sphere_model(collision_inputs(name, kind)["sset"])


# ---- 1. float64 host entry points against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_host_float64_against_the_reference(name, require_gpu):
    assert len(ROBOTS) == 8
    for kind in SETS:
        d, r = collision_inputs(name, kind), reference(name, kind)
        model = robot_model(name, kind)
        assert (model.n_in, model.n_fixed, model.n_sphere, model.n_pair) == (d["orc"].dof, 0, d["sset"].n_sphere, len(d["pairs"]))
        compare64(f"{name} {kind}", host_all(model, d["q"], r["gd"], d["margin"]), r)
        # either output of the penalty alone is the same bits
        E, g = model.penalty(d["q"], d["margin"])
        assert np.array_equal(model.penalty(d["q"], d["margin"], want_grad=False)[0], E) and np.array_equal(model.penalty(d["q"], d["margin"], want_energy=False)[1], g)


# ---- 2. float32 device entry points against the float64 reference --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_reference(name, require_gpu):
    torch = pytest.importorskip("torch")
    for kind in SETS:
        d, r64, r32 = collision_inputs(name, kind), reference(name, kind), reference(name, kind, np.float32)
        got = dev_all(robot_model(name, kind), torch, d["q"], r64["gd"], d["margin"])
        compare32(f"{name} {kind}", got, r64, r32)
        if name == GRIPPER and kind == "origins":
            assert not got["E"].any() and not got["grad"].any()


# ---- 3. optimizer order: mimic joints fold, fixed joints move the geometry and take no gradient ----------------------------------------
@pytest.mark.parametrize("rel", OPT_ORDER + ["subset"])
def test_optimizer_order_folds_mimic_and_fixed_joints(rel, require_gpu):
    torch = pytest.importorskip("torch")
    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames]
    # default pairs skip neighbouring links: spheres of 3 cm, so that links two joints apart come inside the margin
    sset = collision.SphereSet(links, np.zeros((len(links), 3)), np.full(len(links), 0.030))
    pairs = collision.default_pairs(opt.robot, sset)
    x, fixed = (_r32(a) for a in _opt_inputs(prob, B, 211))
    model = opt.sphere_model(sset)
    assert (model.n_in, model.n_fixed, model.n_pair) == (opt.opt_dof, len(opt.idx_pin2fixed), len(pairs)) and opt.sphere_model(sset) is model
    if rel == "subset":
        assert model.n_fixed == 6
    fx = fixed if fixed.shape[1] else None
    fold = lambda J: _fold4(prob, J)  # noqa: E731
    rows, cen, rad = np.arange(len(links)), np.zeros((len(links), 3)), np.full(len(links), 0.030)
    gd = _r32(np.random.default_rng(212).standard_normal((B, len(pairs))))
    w = _r32(np.random.default_rng(213).uniform(0.5, 2.0, len(pairs)))
    q_full = prob.full_qpos(x, fixed)
    r64 = ref_all(prob.robot, q_full, links, rows, cen, rad, pairs, gd, MARGIN, w, np.float64, fold)
    r32 = ref_all(prob.robot, q_full, links, rows, cen, rad, pairs, gd, MARGIN, w, np.float32, fold)
    assert (r64["E"] > 0).any() and np.abs(r64["grad"]).max() > 0
    h64 = host_all(model, x, gd, MARGIN, w, fx)
    compare64(rel, h64, r64)
    d32 = dev_all(model, torch, x, gd, MARGIN, w, fx)
    compare32(rel, d32, r64, r32)
    act = isr.active_columns(prob.robot, q_full, links, fold)
    print(f"{rel}: {int(act.sum())} of {len(act)} columns are read, {len(prob.idx_pin2mimic)} mimic joints, {model.n_fixed} fixed joints, {len(pairs)} default pairs")
    for out in (h64, d32):  # columns no joint reads: exact zeros
        assert not out["grad"][:, ~act].any() and not out["vjp"][:, ~act].any()
    if fx is not None:  # fixed joints move the geometry
        moved = model.distances(x, fx + 0.05)[0]
        assert np.abs(moved - h64["dist"]).max() > 1e-4
    # the torch front is the same launch
    from dex_retargeting_amd import collision as col

    qt, ft, wt = _dev(torch, x), _dev(torch, fx), _dev(torch, w)
    E, g = col.self_collision_penalty(opt, qt, sset, MARGIN, wt, ft)
    assert np.array_equal(E.cpu().numpy(), d32["E"]) and np.array_equal(g.cpu().numpy(), d32["grad"])
    assert np.array_equal(col.sphere_distances(opt, qt, sset, ft).cpu().numpy(), d32["dist"])


# ---- 4. row independence and isolation ---------------------------------------------------------------------------------------------
def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    name, kind = "shadow_hand_right", "offset"
    d, r = collision_inputs(name, kind), reference(name, kind)
    model = robot_model(name, kind)
    w = _r32(np.random.default_rng(5).uniform(0.5, 2.0, model.n_pair))
    full = dev_all(model, torch, d["q"], r["gd"], d["margin"], w)
    assert all(np.isfinite(full[k]).all() for k in OUTPUTS) and (full["E"] > 0).any()
    for b in range(B):  # every row alone: B = 1
        one = dev_all(model, torch, d["q"][b:b + 1], r["gd"][b:b + 1], d["margin"], w)
        for k in OUTPUTS:
            assert np.array_equal(one[k][0], full[k][b]), (b, k)
    perm = np.random.default_rng(6).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    mixed = dev_all(model, torch, d["q"][perm], r["gd"][perm], d["margin"], w)
    for k in OUTPUTS:
        assert np.array_equal(mixed[k], full[k][perm]), k
    # the float64 twin: one row alone and the whole batch
    h = host_all(model, d["q"], r["gd"], d["margin"], w)
    h1 = host_all(model, d["q"][20:21], r["gd"][20:21], d["margin"], w)
    assert all(np.array_equal(h1[k][0], h[k][20]) for k in OUTPUTS)
    # a NaN in row 7 spoils row 7 alone
    bad = d["q"].copy()
    bad[7, 3] = np.nan
    got = dev_all(model, torch, bad, r["gd"], d["margin"], w)
    keep = np.arange(B) != 7
    assert np.isnan(got["E"][7]) and np.isnan(got["grad"][7]).any() and np.isnan(got["dist"][7]).any() and np.isnan(got["vjp"][7]).any()
    for k in OUTPUTS:
        assert np.array_equal(got[k][keep], full[k][keep]), k
    # B = 0: a no-op, NULL pointers and all
    lib = _lib.load()
    assert lib.dexr_sphere_distances_dev(model.handle, 0, None, None, None, None, None) == 0
    assert lib.dexr_sphere_distances_vjp_dev(model.handle, 0, None, None, None, None, None) == 0
    assert lib.dexr_sphere_penalty_dev(model.handle, 0, None, None, 0.01, None, None, None, None) == 0
    assert lib.dexr_sphere_penalty(model.handle, 0, None, None, 0.01, None, None, None) == 0
    e, g = model.penalty(np.zeros((0, model.n_in)), 0.01)
    assert e.shape == (0,) and g.shape == (0, model.n_in) and model.distances(np.zeros((0, model.n_in)))[0].shape == (0, model.n_pair)


# ---- 5. table limits: the synthetic robots of tests/pose_zoo.py ----------------------------------------------------------------------
ZB, ZMARGIN, ZR = 9, 0.020, 0.010  # float32: 8 frames per block on the 128-sphere member, float64 4: ragged tails of 1


def _zoo_case(name, tmp):
    """-> (member, rows, centers, radii, pairs) of the sphere model a zoo member is tested with."""
    m = zoo.build(name, tmp)
    L = len(m.links)
    rng = np.random.default_rng(301)
    if name == "binary64_slots8":  # 64 joints, 64 links, 8 slots: 128 spheres and every pair
        u = rng.standard_normal((L, 3))
        off = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.005, 0.015, (L, 1))
        rows = np.repeat(np.arange(L), 2)
        centers = _r32(np.stack([np.zeros((L, 3)), off], 1).reshape(2 * L, 3))
        pairs = [(i, j) for i in range(2 * L) for j in range(i + 1, 2 * L)]
        assert len(rows) == 128 and len(pairs) == 8128
    elif name == "chain64":  # one pair only: the two spheres of one link, far down the chain
        rows, centers, pairs = np.array([40, 40]), _r32([[0.0, 0.0, 0.0], [0.004, -0.007, 0.009]]), [(1, 0)]
    else:  # wide_map: 50 spheres (no multiple of 16), n_in = 256; star40: 44, three on the fixed base, a link listed twice
        rows, centers = np.arange(L), _r32(rng.uniform(-0.01, 0.01, (L, 3)))
        pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    return m, rows, centers, np.full(len(rows), ZR), np.array(pairs, np.int32)


@pytest.mark.parametrize("name", ["binary64_slots8", "wide_map", "star40", "chain64"])
def test_table_limits(name, tmp_path, require_gpu):
    torch = pytest.importorskip("torch")
    m, rows, centers, radii, pairs = _zoo_case(name, tmp_path)
    model = _lib.SphereModel(m.blob, rows, centers, radii, pairs)
    assert (model.n_in, model.n_sphere, model.n_pair) == (zoo.FACTS[name]["n_in"], len(rows), len(pairs))
    x, fixed, _ = zoo.inputs(m, ZB, 2041)
    q_full = zoo.full_q(m.smap, x, fixed)
    fold = lambda J: zoo.fold(m.smap, J)  # noqa: E731
    gd = _r32(np.random.default_rng(302).standard_normal((ZB, len(pairs))))
    w = _r32(np.random.default_rng(303).uniform(0.5, 2.0, len(pairs)))
    r64 = ref_all(m.orc, q_full, m.links, rows, centers, radii, pairs, gd, ZMARGIN, w, np.float64, fold)
    r32 = ref_all(m.orc, q_full, m.links, rows, centers, radii, pairs, gd, ZMARGIN, w, np.float32, fold)
    assert (r64["E"] > 0).all()
    h64 = host_all(model, x, gd, ZMARGIN, w, fixed)
    compare64(name, h64, r64)
    d32 = dev_all(model, torch, x, gd, ZMARGIN, w, fixed)
    compare32(name, d32, r64, r32)
    unread = zoo.abs_mult(m).sum(0) == 0
    for out in (h64, d32):
        assert not out["grad"][:, unread].any() and not out["vjp"][:, unread].any()
    same = rows[pairs[:, 0]] == rows[pairs[:, 1]]
    if name == "binary64_slots8":  # the two spheres of one link: a constant distance
        assert same.sum() == 64 and np.abs(h64["dist"][:, same] - h64["dist"][:1, same]).max() <= GATE64
    if name == "wide_map":
        assert model.n_in == 256 and model.n_fixed == 256 and int(unread.sum()) == 233 and model.n_sphere % 16 != 0
    if name == "chain64":  # one pair, on one link: constant distance, no gradient beyond rounding (compare32 gates it), no NaN
        assert model.n_pair == 1 and same.all()
        want = np.linalg.norm(centers[1] - centers[0]) - 2 * ZR
        assert np.abs(h64["dist"] - want).max() <= GATE64 and np.abs(h64["grad"]).max() <= GATE64 and np.abs(h64["vjp"]).max() <= GATE64
        assert np.abs(d32["dist"] - want).max() <= 1e-6
    if name == "star40":
        assert int((m.tab["links"]["parent"] == -1).sum()) == 3  # three spheres on the fixed base: they move with nothing
        base = np.isin(rows, [l["out"] for l in m.tab["links"] if l["parent"] == -1])
        both = base[pairs[:, 0]] & base[pairs[:, 1]]
        assert both.sum() == 3 and np.abs(h64["dist"][:, both] - h64["dist"][:1, both]).max() == 0
        assert (h64["dist"][:, base[pairs[:, 0]] ^ base[pairs[:, 1]]].std(0) > 1e-6).any()  # a base sphere against a moving one counts


def test_coincident_spheres_and_a_duplicated_pair(tmp_path, require_gpu):
    torch = pytest.importorskip("torch")
    m = zoo.build("star40", tmp_path)
    assert m.links[20] == m.links[2]  # the link listed twice: spheres at equal centres on rows 2 and 20 coincide
    c = _r32([[0.003, -0.002, 0.005]] * 2 + [[0.0, 0.0, 0.0]])
    rows, radii = np.array([2, 20, 7]), np.array([0.010, 0.004, 0.010])
    x, fixed, _ = zoo.inputs(m, ZB, 2042)
    q_full = zoo.full_q(m.smap, x, fixed)
    fold = lambda J: zoo.fold(m.smap, J)  # noqa: E731
    # coincident: d = -(r_i + r_j), zero gradient, no NaN
    one = _lib.SphereModel(m.blob, rows, c, radii, [(0, 1)])
    dist, _ = one.distances(x, fixed)
    E, g = one.penalty(x, ZMARGIN, None, fixed)
    assert np.array_equal(dist, np.full((ZB, 1), -(0.010 + 0.004))) and not g.any() and not one.distances_vjp(x, np.ones((ZB, 1)), fixed).any()
    assert np.abs(E - (ZMARGIN + 0.014) ** 2).max() <= 1e-15
    d32, _ = dev_distances(one, torch, x, fixed, centers=False)
    e32, g32 = dev_penalty(one, torch, x, ZMARGIN, None, fixed)
    assert np.array_equal(d32, np.full((ZB, 1), -(np.float32(0.010 + 0.004)), np.float32)) and not g32.any() and np.isfinite(e32).all()
    assert not dev_vjp(one, torch, x, np.ones((ZB, 1)), fixed).any()
    # a duplicated pair counts twice
    single = _lib.SphereModel(m.blob, rows, c, radii, [(0, 2)])
    twice = _lib.SphereModel(m.blob, rows, c, radii, [(0, 2), (1, 0), (0, 2)])
    w3 = np.array([1.5, 0.75, 1.5])
    gd = _r32(np.random.default_rng(8).standard_normal((ZB, 3)))
    r64 = ref_all(m.orc, q_full, m.links, rows, c, radii, np.array([(0, 2), (1, 0), (0, 2)]), gd, 0.2, w3, np.float64, fold)
    r32 = ref_all(m.orc, q_full, m.links, rows, c, radii, np.array([(0, 2), (1, 0), (0, 2)]), gd, 0.2, w3, np.float32, fold)
    h64 = host_all(twice, x, gd, 0.2, w3, fixed)
    compare64("duplicated pair", h64, r64)
    compare32("duplicated pair", dev_all(twice, torch, x, gd, 0.2, w3, fixed), r64, r32)
    assert np.array_equal(h64["dist"][:, 0], h64["dist"][:, 2]) and (r64["E"] > 0).all()
    # a margin above every distance: the pair is active in every frame, and two listings of it are exactly twice one
    e1, g1 = single.penalty(x, 0.5, None, fixed)
    e2, g2 = _lib.SphereModel(m.blob, rows, c, radii, [(0, 2), (0, 2)]).penalty(x, 0.5, None, fixed)
    assert (e1 > 0).all() and np.array_equal(e2, 2 * e1) and np.abs(g2 - 2 * g1).max() <= GATE64


# ---- 6. the penalty's gradient against the VJP fed with -2 w h -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shadow_hand_right", "arm_shadow_hand_right"])
def test_penalty_gradient_equals_the_vjp_of_its_forces(name, require_gpu):
    torch = pytest.importorskip("torch")
    kind = "offset"
    d, r64, r32 = collision_inputs(name, kind), reference(name, kind), reference(name, kind, np.float32)
    model = robot_model(name, kind)
    dist, _ = dev_distances(model, torch, d["q"], centers=False)
    h = np.maximum(np.float32(0), np.float32(d["margin"]) - dist)
    via = dev_vjp(model, torch, d["q"], np.float32(-2) * h)
    _, g = dev_penalty(model, torch, d["q"], d["margin"])
    gate = GATE32 * float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
    e = float(np.abs(via.astype(np.float64) - g).max())
    print(f"{name}: max |penalty gradient - VJP of -2 h| = {e:.3e} (gate {gate:.3e} = {GATE32:g} x the reference's float32 distance), max |gradient| {np.abs(g).max():.3e}")
    assert (h > 0).any() and gate > 0 and e <= gate
    # float64: the same two routes within GATE64
    dist64 = model.distances(d["q"])[0]
    via64 = model.distances_vjp(d["q"], -2 * np.maximum(0.0, d["margin"] - dist64))
    assert np.abs(via64 - model.penalty(d["q"], d["margin"])[1]).max() <= GATE64


# ---- 7. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    d = collision_inputs("allegro_hand_right", "origins")
    model = robot_model("allegro_hand_right", "origins")
    n, P, S = 4, model.n_pair, model.n_sphere
    x = torch.zeros((n, model.n_in), dtype=torch.float32, device="cuda")
    gd = torch.ones((n, P), dtype=torch.float32, device="cuda")
    w = torch.ones((P,), dtype=torch.float32, device="cuda")
    dist, cen, e, gx = _nan(torch, (n, P)), _nan(torch, (n, S, 3)), _nan(torch, (n,)), _nan(torch, (n, model.n_in))
    h, xp = model.handle, x.data_ptr()
    INVALID = -1

    def invalid(rc, word=None):
        assert rc == INVALID
        msg = lib.dexr_last_error()
        assert len(msg) > 0 and (word is None or word in msg), msg

    invalid(lib.dexr_sphere_distances_dev(None, n, xp, None, dist.data_ptr(), None, None), b"null sphere model")
    invalid(lib.dexr_sphere_distances_dev(h, -1, xp, None, dist.data_ptr(), None, None), b"negative")
    invalid(lib.dexr_sphere_distances_dev(h, n, None, None, dist.data_ptr(), cen.data_ptr(), None), b"x is NULL")
    invalid(lib.dexr_sphere_distances_dev(h, n, xp, None, None, cen.data_ptr(), None), b"dist_out is NULL")
    invalid(lib.dexr_sphere_distances_vjp_dev(None, n, xp, None, gd.data_ptr(), gx.data_ptr(), None), b"null sphere model")
    invalid(lib.dexr_sphere_distances_vjp_dev(h, n, xp, None, None, gx.data_ptr(), None), b"grad_dist is NULL")
    invalid(lib.dexr_sphere_distances_vjp_dev(h, n, xp, None, gd.data_ptr(), None, None), b"grad_x_out is NULL")
    invalid(lib.dexr_sphere_distances_vjp_dev(h, n, None, None, gd.data_ptr(), gx.data_ptr(), None), b"x is NULL")
    invalid(lib.dexr_sphere_penalty_dev(None, n, xp, None, 0.01, None, e.data_ptr(), gx.data_ptr(), None), b"null sphere model")
    invalid(lib.dexr_sphere_penalty_dev(h, -3, xp, None, 0.01, None, e.data_ptr(), gx.data_ptr(), None), b"negative")
    invalid(lib.dexr_sphere_penalty_dev(h, n, xp, None, 0.01, w.data_ptr(), None, None, None), b"both NULL")
    invalid(lib.dexr_sphere_penalty_dev(h, n, None, None, 0.01, None, e.data_ptr(), gx.data_ptr(), None), b"x is NULL")
    for bad in (-1e-6, -1.0, float("nan"), float("inf"), -float("inf")):
        invalid(lib.dexr_sphere_penalty_dev(h, n, xp, None, bad, None, e.data_ptr(), gx.data_ptr(), None), b"margin")
    # a model that reads fixed columns
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.sphere_model(collision.SphereSet(["link_15.0_tip", "link_3.0_tip"], np.zeros((2, 3)), [0.01, 0.01], [(0, 1)]))
    assert ms.n_fixed == 6 and ms.n_in == 10
    invalid(lib.dexr_sphere_penalty_dev(ms.handle, n, xp, None, 0.01, None, e.data_ptr(), None, None), b"fixed")
    invalid(lib.dexr_sphere_distances_dev(ms.handle, n, xp, None, dist.data_ptr(), None, None), b"fixed")
    # the host twins keep the same rules
    z, zg, zw = np.zeros((n, model.n_in)), np.ones((n, P)), np.ones(P)
    zd, zc, ze, zx = np.full((n, P), np.nan), np.full((n, S, 3), np.nan), np.full(n, np.nan), np.full((n, model.n_in), np.nan)
    dp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    invalid(lib.dexr_sphere_distances(None, n, dp(z), None, dp(zd), dp(zc)), b"null sphere model")
    invalid(lib.dexr_sphere_distances(h, -2, dp(z), None, dp(zd), dp(zc)), b"negative")
    invalid(lib.dexr_sphere_distances(h, n, None, None, dp(zd), dp(zc)), b"x is NULL")
    invalid(lib.dexr_sphere_distances(h, n, dp(z), None, None, dp(zc)), b"dist_out is NULL")
    invalid(lib.dexr_sphere_distances_vjp(h, n, dp(z), None, None, dp(zx)), b"grad_dist is NULL")
    invalid(lib.dexr_sphere_distances_vjp(h, n, dp(z), None, dp(zg), None), b"grad_x_out is NULL")
    invalid(lib.dexr_sphere_penalty(h, n, dp(z), None, 0.01, dp(zw), None, None), b"both NULL")
    for bad in (-1.0, float("nan"), float("inf")):
        invalid(lib.dexr_sphere_penalty(h, n, dp(z), None, bad, None, dp(ze), dp(zx)), b"margin")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dist, cen, e, gx))  # nothing was launched
    assert all(np.isnan(a).all() for a in (zd, zc, ze, zx))
    with pytest.raises(ValueError, match="shape"):
        model.distances_vjp(z, zg[:, :-1])
    with pytest.raises(ValueError, match="shape"):
        model.penalty(z, 0.01, zw[:-1])
    with pytest.raises(ValueError, match="shape"):
        model.distances(z[:, :-1])
    assert d["sset"].n_sphere == S


# ---- 8. torch front ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_torch_front_equals_the_entry_points_bitwise(rel, require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames]
    names = links + links[:4]
    cen = np.concatenate([np.zeros((len(links), 3)), _r32(np.random.default_rng(9).uniform(-0.01, 0.01, (4, 3)))])
    sset = collision.SphereSet(names, cen, np.full(len(names), 0.030))  # (default pairs: 3 cm reaches links two joints apart)
    n, margin = 130, 0.008
    x, fixed = _opt_inputs(prob, n, 221)
    q = _dev(torch, x)
    f = _dev(torch, fixed) if fixed.shape[1] else None
    model = opt.sphere_model(sset)
    w = _dev(torch, np.random.default_rng(222).uniform(0.5, 2.0, model.n_pair))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = side.cuda_stream
        for wt in (None, w):
            E, g = collision.self_collision_penalty(opt, q, sset, margin, wt, f)
            we, wg = _nan(torch, (n,)), _nan(torch, (n, model.n_in))
            model.penalty_dev(n, q.data_ptr(), _ptr(f), margin, _ptr(wt), we.data_ptr(), wg.data_ptr(), stream=sp)
            assert torch.equal(E, we) and torch.equal(g, wg) and not E.requires_grad and not g.requires_grad and bool((E > 0).any())
            qg = q.clone().requires_grad_(True)
            Eg = ag.self_collision_penalty(opt, qg, sset, margin, wt, f)
            assert Eg.requires_grad and torch.equal(Eg.detach(), E)
            Eg.sum().backward()
            assert torch.equal(qg.grad, g)
            # a weighted sum of the energies scales the rows
            qh = q.clone().requires_grad_(True)
            scale = torch.linspace(0.5, 2.0, n, device="cuda")
            (ag.self_collision_penalty(opt, qh, sset, margin, wt, f) * scale).sum().backward()
            assert torch.equal(qh.grad, scale[:, None] * g)
            # no gradient asked: the same energy, no graph
            En = ag.self_collision_penalty(opt, q, sset, margin, wt, f)
            assert torch.equal(En, E) and not En.requires_grad
        dist, c = collision.sphere_distances(opt, q, sset, f, centers=True)
        wd, wc = _nan(torch, (n, model.n_pair)), _nan(torch, (n, model.n_sphere, 3))
        model.distances_dev(n, q.data_ptr(), _ptr(f), wd.data_ptr(), wc.data_ptr(), stream=sp)
        assert torch.equal(dist, wd) and torch.equal(c, wc) and torch.equal(collision.sphere_distances(opt, q, sset, f), wd)
        qg = q.clone().requires_grad_(True)
        dg = ag.sphere_distances(opt, qg, sset, f)
        cot = torch.randn(dist.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        assert torch.equal(dg.detach(), wd)
        dg.backward(cot)
        want = _nan(torch, (n, model.n_in))
        model.distances_vjp_dev(n, q.data_ptr(), _ptr(f), cot.data_ptr(), want.data_ptr(), stream=sp)
        assert torch.equal(qg.grad, want) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        # non-contiguous inputs: views with the same values
        qn = torch.stack([q, q], 2)[:, :, 0]
        fn = None if f is None else torch.stack([f, f], 2)[:, :, 1]
        wn = torch.stack([w, w], 1)[:, 0]
        assert not qn.is_contiguous() and not wn.is_contiguous()
        a = collision.self_collision_penalty(opt, qn, sset, margin, wn, fn)
        b = collision.self_collision_penalty(opt, q, sset, margin, w, f)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        # the robot_* twins over the full qpos
        robot = opt.robot
        rl = robot.joint_limits
        qr = _dev(torch, np.random.default_rng(223).uniform(rl[:, 0], rl[:, 1], (n, robot.dof)))
        rm = robot.sphere_model(sset)
        Er, gr = collision.robot_self_collision_penalty(robot, qr, sset, margin)
        we, wg = _nan(torch, (n,)), _nan(torch, (n, robot.dof))
        rm.penalty_dev(n, qr.data_ptr(), 0, margin, 0, we.data_ptr(), wg.data_ptr(), stream=sp)
        assert torch.equal(Er, we) and torch.equal(gr, wg)
        qrg = qr.clone().requires_grad_(True)
        ag.robot_self_collision_penalty(robot, qrg, sset, margin).sum().backward()
        assert torch.equal(qrg.grad, wg)
        assert torch.equal(ag.robot_sphere_distances(robot, qr, sset), collision.robot_sphere_distances(robot, qr, sset))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e = torch.zeros((0, opt.opt_dof), device="cuda")
    E0, g0 = collision.self_collision_penalty(opt, e, sset, margin, None, None if f is None else f[:0])
    assert E0.shape == (0,) and g0.shape == (0, opt.opt_dof)
    assert collision.sphere_distances(opt, e, sset, None if f is None else f[:0]).shape == (0, model.n_pair)


def test_keypoints_to_self_collision_loss_end_to_end(require_gpu):
    torch = pytest.importorskip("torch")
    import os

    from dex_retargeting_amd import autograd as ag

    rel = "teleop/allegro_hand_right.yml"
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    n = 256
    d = cases.human_set(prob, n)
    links = [f.name for f in opt.robot.kin.frames]
    # spheres of 5 cm on every link origin and every pair: links two joints apart are always inside the margin, and their
    # distance depends on the joint between them
    S = len(links)
    sset = collision.SphereSet(links, np.zeros((S, 3)), np.full(S, 0.05), [(i, j) for i in range(S) for j in range(i + 1, S)])
    kp = glp._t(d["kp"], torch, dtype=torch.float32, requires_grad=True)
    last = glp._t(d["last"], torch, requires_grad=True)
    fixed = glp._t(d["fixed"], torch) if d["fixed"].shape[1] else None
    ref = ag.ref_value_from_keypoints(opt, kp)
    q = ag.retarget(opt, ref, last, fixed, None)
    E = ag.self_collision_penalty(opt, q, sset, 0.01, None, fixed)
    assert E.shape == (n,) and bool((E > 0).all())
    E.sum().backward()
    assert bool(torch.isfinite(kp.grad).all()) and float(kp.grad.abs().max()) > 0
    assert bool(torch.isfinite(last.grad).all())
    # grad_q of the loss is the no-graph call's
    _, g = collision.self_collision_penalty(opt, q.detach(), sset, 0.01, None, fixed)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0

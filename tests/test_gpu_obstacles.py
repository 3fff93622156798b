"""GPU tests of the obstacle collision (csrc/dexr_obstacles.hpp, include/dexr_obstacles.h): the float64 host entry points and the
float32 device entry points against tests/obstacle_reference.py, the limits of the tables, optimizer order, row independence, the
penalty against the VJP, the raw ABI's argument errors, the torch front and autograd.

INPUTS.  The eight fixture robots run obstacle_inputs of tests/test_obstacle_host.py (the "offset" sphere set, B = 33: two blocks
and a ragged tail; nine primitives of all four kinds with a seeded pose per frame), whose reference runs and conditions are proven
there on the CPU and shared from there.  Every other case is built by make_case, which asserts the same conditions on its own
reference before a GPU sees it: no active box-interior entry within TIE_GAP of a tie of its two largest q_i, no active entry
within a millimetre of a sphere's centre or a capsule's axis.

GATES.  float64: 1e-9 absolute on every output (GATE64 of the sphere family).  float32: max |out32 - reference64| of an output may
be 8 x the distance between the reference's OWN float32 and float64 runs on that output (GATE32); where that distance is zero the
output must be exact zeros.  `nearest` is compared where the two smallest d_sm of the float64 reference differ by more than
NEAR_GAP = 1e-5 m (a hundred times the float32 error of a distance), and the cotangent of every VJP is zero elsewhere.  The ratios
are printed; those of the MI355X are in docs/experiments/obstacle_collision.md."""
import functools
import os

import numpy as np
import pytest

import collision_reference as cref
import ik_solve_reference as isr
import obstacle_reference as oref
import pose_zoo as zoo
import test_gpu_link_poses as glp
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, MARGIN, ROBOTS, robot_of
from test_gpu_link_jacobians import OPT_ORDER, _fold4, _opt_inputs, _optimizer_and_problem
from test_jacobian_host import SUBSET_CFG
from test_obstacle_host import TIE_GAP, _kink_distance, _rotations, clear_nearest, masked_cotangent, obstacle_inputs, obstacles, reference

pytestmark = pytest.mark.gpu
GATE64, GATE32 = 1e-9, 8.0
FLOATS = ("dist", "vjp", "E", "grad", "wrench")
OUTPUTS = FLOATS + ("nearest",)


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- the float32 device entry points on numpy arrays, the outputs pre-filled with NaN (nearest: -1) ---------------------------------
def _dev(torch, a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _np(t):
    return None if t is None else t.cpu().numpy()


def _handle(torch, oset):
    return oset.device_set(torch.cuda.current_device())


def dev_distances(model, oset, torch, x, fixed=None, pos=None, rot=None, dist=True, nearest=True):
    xd, fd, pd, rd = (_dev(torch, a) for a in (x, fixed, pos, rot))
    n = xd.shape[0]
    d = _nan(torch, (n, model.n_sphere)) if dist else None
    k = torch.full((n, model.n_sphere), -1, dtype=torch.int32, device="cuda") if nearest else None
    model.obstacle_distances_dev(_handle(torch, oset), n, _ptr(xd), _ptr(fd), _ptr(d), _ptr(k), _ptr(pd), _ptr(rd),
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _np(d), _np(k)


def dev_vjp(model, oset, torch, x, gd, fixed=None, pos=None, rot=None):
    xd, fd, pd, rd, g = (_dev(torch, a) for a in (x, fixed, pos, rot, gd))
    gx = _nan(torch, (xd.shape[0], model.n_in))
    model.obstacle_distances_vjp_dev(_handle(torch, oset), xd.shape[0], _ptr(xd), _ptr(fd), _ptr(g), _ptr(gx), _ptr(pd), _ptr(rd),
                                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _np(gx)


def dev_penalty(model, oset, torch, x, margin, w=None, fixed=None, pos=None, rot=None, energy=True, grad=True, wrench=True):
    xd, fd, pd, rd, wd = (_dev(torch, a) for a in (x, fixed, pos, rot, w))
    n = xd.shape[0]
    e, gx, wr = (_nan(torch, (n,)) if energy else None), (_nan(torch, (n, model.n_in)) if grad else None), (_nan(torch, (n, 6)) if wrench else None)
    model.obstacle_penalty_dev(_handle(torch, oset), n, _ptr(xd), _ptr(fd), margin, _ptr(wd), _ptr(e), _ptr(gx), _ptr(wr), _ptr(pd), _ptr(rd),
                               stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _np(e), _np(gx), _np(wr)


def dev_all(model, oset, torch, x, gd, margin, w=None, fixed=None, pos=None, rot=None):
    dist, near = dev_distances(model, oset, torch, x, fixed, pos, rot)
    E, grad, wrench = dev_penalty(model, oset, torch, x, margin, w, fixed, pos, rot)
    return dict(dist=dist, nearest=near, vjp=dev_vjp(model, oset, torch, x, gd, fixed, pos, rot), E=E, grad=grad, wrench=wrench)


def host_all(model, oset, x, gd, margin, w=None, fixed=None, pos=None, rot=None):
    h = oset.device_set(0)
    dist, near = model.obstacle_distances(h, x, fixed, pos, rot)
    E, grad, wrench = model.obstacle_penalty(h, x, margin, w, fixed, pos, rot)
    return dict(dist=dist, nearest=near, vjp=model.obstacle_distances_vjp(h, x, gd, fixed, pos, rot), E=E, grad=grad, wrench=wrench)


def _compare_nearest(tag, got, want, clear, n_prim):
    assert got["nearest"].dtype == np.int32 and got["nearest"].shape == want["nearest"].shape, tag
    assert (got["nearest"] >= 0).all() and (got["nearest"] < n_prim).all(), tag
    assert np.array_equal(got["nearest"][clear], want["nearest"][clear]), (tag, "nearest")


def compare64(tag, got, want, clear, n_prim):
    for k in FLOATS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, (tag, k)
        e = float(np.abs(got[k] - want[k]).max())
        print(f"{tag}: float64 max |{k} - reference| = {e:.3e} (gate {GATE64:.0e})")
        assert np.isfinite(got[k]).all() and e <= GATE64, (tag, k, e)
    _compare_nearest(tag, got, want, clear, n_prim)


def compare32(tag, got, want64, want32, clear, n_prim):
    """the gate of each output comes from the reference's own two runs, never from the code under test"""
    for k in FLOATS:
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
    _compare_nearest(tag, got, want64, clear, n_prim)


def make_case(orc, q_full, links, rows, centers, radii, oset, pos, rot, w, gd, margin, fold=None):
    """the references of one case, float64 and float32, with the conditions the gates rest on asserted on the float64 run: dict
    r64, r32, gd (the cotangent, zero where the nearest primitive is not clear), clear (B, S)."""
    args = (orc, q_full, links, rows, centers, radii, oset.kinds, oset.params, pos, rot)
    F = oref.fields(*args, np.float64, fold)
    clear = clear_nearest(F["d"])
    gdm = np.where(clear, gd, 0.0)

    def outs(F_):
        dist, near = oref.distances(F_)
        E, grad, wrench, h = oref.penalty(F_, margin, w)
        return dict(dist=dist, nearest=near, vjp=oref.distances_vjp(F_, gdm), E=E, grad=grad, wrench=wrench, h=h)

    r64, r32 = outs(F), outs(oref.fields(*args, np.float32, fold))
    R = np.broadcast_to(np.eye(3), (len(F["c"]), 3, 3)) if rot is None else rot
    point, tie = _kink_distance(oset.kinds, oset.params, np.einsum("bji,bsj->bsi", R, F["arm"]))
    active = r64["h"] > 0
    assert (tie[active] >= TIE_GAP).all(), ("an active box-interior entry near a tie", float(tie[active].min()))
    assert (point[active] >= 1e-3).all(), ("an active entry near a centre or an axis", float(point[active].min()))
    return dict(r64=r64, r32=r32, gd=gdm, clear=clear)


def robot_model(name):
    return robot_of(name)[0].sphere_model(obstacle_inputs(name)["sset"])


def _robot_args(d):
    return dict(w=d["w"], pos=d["pos"], rot=d["rot"])


# ---- 1. float64 host entry points against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_host_float64_against_the_reference(name, require_gpu):
    assert len(ROBOTS) == 8
    d, r = obstacle_inputs(name), reference(name)
    model, oset = robot_model(name), d["oset"]
    assert (model.n_in, model.n_fixed, model.n_sphere) == (d["orc"].dof, 0, d["sset"].n_sphere) and oset.device_set(0).n_prim == 9
    got = host_all(model, oset, d["q"], masked_cotangent(name), d["margin"], **_robot_args(d))
    compare64(name, got, r, clear_nearest(r["d"]), oset.n_prim)
    assert (got["E"][d["far"]] == 0).all() and not got["grad"][d["far"]].any() and not got["wrench"][d["far"]].any()
    # each output of a call alone is the same bits
    h = oset.device_set(0)
    for k, want in (("want_energy", "E"), ("want_grad", "grad"), ("want_wrench", "wrench")):
        flags = {f: f == k for f in ("want_energy", "want_grad", "want_wrench")}
        one = model.obstacle_penalty(h, d["q"], d["margin"], d["w"], None, d["pos"], d["rot"], **flags)
        assert [o is not None for o in one] == [flags[f] for f in ("want_energy", "want_grad", "want_wrench")]
        assert np.array_equal(next(o for o in one if o is not None), got[want]), k
    assert model.obstacle_distances(h, d["q"], None, d["pos"], d["rot"], nearest=False)[1] is None


# ---- 2. float32 device entry points against the float64 reference --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_reference(name, require_gpu):
    torch = pytest.importorskip("torch")
    d, r64, r32 = obstacle_inputs(name), reference(name), reference(name, np.float32)
    got = dev_all(robot_model(name), d["oset"], torch, d["q"], masked_cotangent(name), d["margin"], **_robot_args(d))
    compare32(name, got, r64, r32, clear_nearest(r64["d"]), d["oset"].n_prim)
    assert (got["E"][d["far"]] == 0).all() and not got["grad"][d["far"]].any() and not got["wrench"][d["far"]].any() and (got["E"] > 0).any()


# ---- 3. the limits -------------------------------------------------------------------------------------------------------------------
LIMIT_ROBOT = "allegro_hand_right"
M64_SEED, ZOO_SEED, ORDER_SEED = 5, 303, 293  # each the first seed (from 3, 302, 232 on) with which make_case's conditions hold


def random_set(M, seed):
    """M seeded primitives of mixed kinds a few centimetres across around the origin of the obstacle frame (one box in twenty: every
    box adds interior ties that an active entry must stay clear of)."""
    rng = np.random.default_rng(seed)
    O, parts = collision.ObstacleSet, []
    for kind in rng.choice(4, M, p=[0.4, 0.4, 0.05, 0.15]):
        c = rng.uniform(-0.06, 0.06, (1, 3))
        if kind == oref.SPHERE:
            parts.append(O.spheres(c, rng.uniform(0.005, 0.02, 1)))
        elif kind == oref.CAPSULE:
            parts.append(O.capsules(c, c + rng.uniform(-0.04, 0.04, (1, 3)), rng.uniform(0.005, 0.015, 1)))
        elif kind == oref.BOX:
            parts.append(O.boxes(c, rng.uniform(0.01, 0.03, (1, 3)), _rotations(rng, 1)))
        else:
            n = rng.standard_normal((1, 3))
            parts.append(O.half_spaces(n / np.linalg.norm(n), rng.uniform(-0.12, -0.08, 1)))
    return O.concat(*parts)


ONE_KIND = {k: n for n, k in (("spheres", oref.SPHERE), ("capsules", oref.CAPSULE), ("boxes", oref.BOX), ("half_spaces", oref.HALFSPACE))}


@functools.lru_cache(maxsize=None)
def limit_case(which):
    """-> (inputs, oset, case) on LIMIT_ROBOT: "M1" one capsule, "M64" a full set of mixed kinds, or one kind of obstacles() alone."""
    d = obstacle_inputs(LIMIT_ROBOT)
    if which == "M1":
        oset = collision.ObstacleSet.capsules([[-0.03, 0.0, 0.0]], [[0.04, 0.01, 0.02]], [0.02])
    elif which == "M64":
        oset = random_set(64, M64_SEED)
    else:
        full = obstacles()
        keep = full.kinds == which
        oset = collision.ObstacleSet(full.kinds[keep], full.params[keep])
        assert set(oset.kinds.tolist()) == {which} and oset.n_prim >= 2
    w = _r32(np.random.default_rng(71).uniform(0.5, 2.0, oset.n_prim))
    case = make_case(d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"], oset, d["pos"], d["rot"], w, d["gd"], d["margin"])
    assert (case["r64"]["E"] > 0).any()
    return d, oset, w, case


@pytest.mark.parametrize("which", ["M1", "M64"] + sorted(ONE_KIND))
def test_limits_of_the_obstacle_set(which, require_gpu):
    torch = pytest.importorskip("torch")
    d, oset, w, case = limit_case(which)
    tag = which if isinstance(which, str) else f"only {ONE_KIND[which]}"
    assert oset.n_prim == {"M1": 1, "M64": _lib.OBSTACLE_MAX}.get(which, oset.n_prim)
    if which == "M64":
        assert len(set(oset.kinds.tolist())) == 4 and len(set(case["r64"]["nearest"].reshape(-1).tolist())) > 8
    model = robot_model(LIMIT_ROBOT)
    kw = dict(w=w, pos=d["pos"], rot=d["rot"])
    compare64(tag, host_all(model, oset, d["q"], case["gd"], d["margin"], **kw), case["r64"], case["clear"], oset.n_prim)
    compare32(tag, dev_all(model, oset, torch, d["q"], case["gd"], d["margin"], **kw), case["r64"], case["r32"], case["clear"], oset.n_prim)


ZB, ZR, ZMARGIN = 9, 0.010, 0.020  # float32: 8 frames per block on the 128-sphere member, float64 4: ragged tails of 1


def zoo_case(tmp):
    """the 64-joint, 64-link, 8-slot member of tests/pose_zoo.py with two spheres per link: S = 128."""
    m = zoo.build("binary64_slots8", tmp)
    L = len(m.links)
    rng = np.random.default_rng(301)
    u = rng.standard_normal((L, 3))
    off = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.005, 0.015, (L, 1))
    rows = np.repeat(np.arange(L), 2)
    centers = _r32(np.stack([np.zeros((L, 3)), off], 1).reshape(2 * L, 3))
    radii = np.full(len(rows), ZR)
    x, fixed, _ = zoo.inputs(m, ZB, 2051)
    q_full = zoo.full_q(m.smap, x, fixed)
    c = cref.centres(m.orc, q_full, m.links, rows, centers)[0]
    rng = np.random.default_rng(ZOO_SEED)
    rot = _r32(_rotations(rng, ZB))
    pos = _r32(c.mean(1) + rng.uniform(-0.02, 0.02, (ZB, 3)))
    oset = obstacles()
    w = _r32(rng.uniform(0.5, 2.0, oset.n_prim))
    gd = _r32(rng.standard_normal((ZB, len(rows))))
    case = make_case(m.orc, q_full, m.links, rows, centers, radii, oset, pos, rot, w, gd, ZMARGIN, lambda J: zoo.fold(m.smap, J))
    return m, rows, centers, radii, x, fixed, pos, rot, oset, w, case


def test_limit_of_the_sphere_table(tmp_path, require_gpu):
    torch = pytest.importorskip("torch")
    m, rows, centers, radii, x, fixed, pos, rot, oset, w, case = zoo_case(tmp_path)
    model = _lib.SphereModel(m.blob, rows, centers, radii, [(0, 1)])  # (the pair list plays no part)
    assert (model.n_in, model.n_sphere) == (zoo.FACTS["binary64_slots8"]["n_in"], _lib.SPHERE_MAX) and (case["r64"]["E"] > 0).any()
    kw = dict(w=w, fixed=fixed, pos=pos, rot=rot)
    h64 = host_all(model, oset, x, case["gd"], ZMARGIN, **kw)
    compare64("128 spheres", h64, case["r64"], case["clear"], oset.n_prim)
    d32 = dev_all(model, oset, torch, x, case["gd"], ZMARGIN, **kw)
    compare32("128 spheres", d32, case["r64"], case["r32"], case["clear"], oset.n_prim)
    unread = zoo.abs_mult(m).sum(0) == 0
    for out in (h64, d32):
        assert not out["grad"][:, unread].any() and not out["vjp"][:, unread].any()


def test_a_pose_left_out_is_zeros_and_the_identity_and_a_far_set_gives_exact_zeros(require_gpu):
    torch = pytest.importorskip("torch")
    d = obstacle_inputs("shadow_hand_right")
    model, oset, gd = robot_model("shadow_hand_right"), d["oset"], masked_cotangent("shadow_hand_right")
    zeros, eye = np.zeros((B, 3)), np.broadcast_to(np.eye(3), (B, 3, 3))
    for pos, rot in ((None, d["rot"]), (d["pos"], None), (None, None)):
        a = dev_all(model, oset, torch, d["q"], gd, d["margin"], d["w"], None, pos, rot)
        b = dev_all(model, oset, torch, d["q"], gd, d["margin"], d["w"], None, zeros if pos is None else pos, eye if rot is None else rot)
        assert all(np.array_equal(a[k], b[k]) for k in OUTPUTS) and np.isfinite(a["E"]).all() and (a["E"] > 0).any()
        a = host_all(model, oset, d["q"], gd, d["margin"], d["w"], None, pos, rot)
        b = host_all(model, oset, d["q"], gd, d["margin"], d["w"], None, zeros if pos is None else pos, eye if rot is None else rot)
        assert all(np.array_equal(a[k], b[k]) for k in OUTPUTS)
    # a set far from the hand: exact zeros
    far = _r32(d["pos"] + np.array([10.0, -10.0, 10.0]))
    spheres = collision.ObstacleSet.spheres(d["params"][:2, :3], d["params"][:2, 3]) + collision.ObstacleSet.boxes(d["params"][5:6, :3], d["params"][5:6, 3:6])
    for out in (dev_all(model, spheres, torch, d["q"], gd, d["margin"], None, None, far, d["rot"]),
                host_all(model, spheres, d["q"], gd, d["margin"], None, None, far, d["rot"])):
        assert not out["E"].any() and not out["grad"].any() and not out["wrench"].any() and (out["dist"] > 5).all()


# ---- 4. optimizer order: mimic joints fold, fixed joints move the geometry and take no gradient ----------------------------------------
@functools.lru_cache(maxsize=None)
def order_case(rel):
    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames]
    rows, cen, rad = np.arange(len(links)), np.zeros((len(links), 3)), np.full(len(links), 0.030)
    sset = collision.SphereSet(links, cen, rad)  # (default pairs: 3 cm reaches links two joints apart)
    x, fixed = (_r32(a) for a in _opt_inputs(prob, B, 231))
    q_full = prob.full_qpos(x, fixed)
    c = cref.centres(prob.robot, q_full, links, rows, cen)[0]
    rng = np.random.default_rng(ORDER_SEED)
    rot = _r32(_rotations(rng, B))
    pos = _r32(c.mean(1) + rng.uniform(-0.02, 0.02, (B, 3)))
    oset = obstacles()
    w = _r32(rng.uniform(0.5, 2.0, oset.n_prim))
    gd = _r32(rng.standard_normal((B, len(links))))
    fold = lambda J: _fold4(prob, J)  # noqa: E731
    case = make_case(prob.robot, q_full, links, rows, cen, rad, oset, pos, rot, w, gd, MARGIN, fold)
    return opt, prob, links, sset, x, fixed, q_full, pos, rot, oset, w, fold, case


@pytest.mark.parametrize("rel", OPT_ORDER + ["subset"])
def test_optimizer_order_folds_mimic_and_fixed_joints(rel, require_gpu):
    torch = pytest.importorskip("torch")
    opt, prob, links, sset, x, fixed, q_full, pos, rot, oset, w, fold, case = order_case(rel)
    model = opt.sphere_model(sset)
    assert (model.n_in, model.n_fixed, model.n_sphere) == (opt.opt_dof, len(opt.idx_pin2fixed), len(links))
    if rel == "subset":
        assert model.n_fixed == 6
    fx = fixed if fixed.shape[1] else None
    r64, r32 = case["r64"], case["r32"]
    assert (r64["E"] > 0).any() and np.abs(r64["grad"]).max() > 0
    kw = dict(w=w, fixed=fx, pos=pos, rot=rot)
    h64 = host_all(model, oset, x, case["gd"], MARGIN, **kw)
    compare64(rel, h64, r64, case["clear"], oset.n_prim)
    d32 = dev_all(model, oset, torch, x, case["gd"], MARGIN, **kw)
    compare32(rel, d32, r64, r32, case["clear"], oset.n_prim)
    act = isr.active_columns(prob.robot, q_full, links, fold)
    print(f"{rel}: {int(act.sum())} of {len(act)} columns are read, {len(prob.idx_pin2mimic)} mimic joints, {model.n_fixed} fixed joints")
    for out in (h64, d32):  # columns no joint reads: exact zeros
        assert not out["grad"][:, ~act].any() and not out["vjp"][:, ~act].any()
    if fx is not None:  # fixed joints move the geometry
        moved = model.obstacle_distances(oset.device_set(0), x, fx + 0.05, pos, rot)[0]
        assert np.abs(moved - h64["dist"]).max() > 1e-4
    # the torch front is the same launch
    qt, ft, wt, pt, rt = (_dev(torch, a) for a in (x, fx, w, pos, rot))
    E, g, wr = collision.obstacle_penalty(opt, qt, sset, oset, MARGIN, pt, rt, wt, ft, wrench=True)
    assert np.array_equal(_np(E), d32["E"]) and np.array_equal(_np(g), d32["grad"]) and np.array_equal(_np(wr), d32["wrench"])
    E2, g2 = collision.obstacle_penalty(opt, qt, sset, oset, MARGIN, pt, rt, wt, ft)
    assert torch.equal(E2, E) and torch.equal(g2, g)
    dist, near = collision.obstacle_distances(opt, qt, sset, oset, pt, rt, ft, nearest=True)
    assert np.array_equal(_np(dist), d32["dist"]) and np.array_equal(_np(near), d32["nearest"]) and near.dtype == torch.int32
    assert torch.equal(collision.obstacle_distances(opt, qt, sset, oset, pt, rt, ft), dist)


# ---- 5. row independence and isolation ---------------------------------------------------------------------------------------------
def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    name = "shadow_hand_right"
    d, gd = obstacle_inputs(name), masked_cotangent(name)
    model, oset = robot_model(name), d["oset"]
    q, w, pos, rot, margin = d["q"], d["w"], d["pos"], d["rot"], d["margin"]
    full = dev_all(model, oset, torch, q, gd, margin, w, None, pos, rot)
    assert all(np.isfinite(full[k]).all() for k in FLOATS) and (full["E"] > 0).any()
    for b in range(B):  # every row alone: B = 1
        one = dev_all(model, oset, torch, q[b:b + 1], gd[b:b + 1], margin, w, None, pos[b:b + 1], rot[b:b + 1])
        for k in OUTPUTS:
            assert np.array_equal(one[k][0], full[k][b]), (b, k)
    perm = np.random.default_rng(6).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    mixed = dev_all(model, oset, torch, q[perm], gd[perm], margin, w, None, pos[perm], rot[perm])
    for k in OUTPUTS:
        assert np.array_equal(mixed[k], full[k][perm]), k
    # the float64 twin: one row alone and the whole batch
    h = host_all(model, oset, q, gd, margin, w, None, pos, rot)
    h1 = host_all(model, oset, q[20:21], gd[20:21], margin, w, None, pos[20:21], rot[20:21])
    assert all(np.array_equal(h1[k][0], h[k][20]) for k in OUTPUTS)
    # a NaN in row 7 of q, of obstacle_pos or of obstacle_rot spoils row 7 alone
    keep = np.arange(B) != 7
    for which in ("q", "pos", "rot"):
        bq, bp, br = q.copy(), pos.copy(), rot.copy()
        {"q": bq, "pos": bp, "rot": br}[which].reshape(B, -1)[7, 1] = np.nan
        got = dev_all(model, oset, torch, bq, gd, margin, w, None, bp, br)
        assert np.isnan(got["E"][7]) and all(np.isnan(got[k][7]).any() for k in ("grad", "dist", "vjp", "wrench")), which
        for k in OUTPUTS:
            assert np.array_equal(got[k][keep], full[k][keep]), (which, k)
    # each optional output alone gives the same bits as all together
    for flags, k in ((dict(grad=False, wrench=False), 0), (dict(energy=False, wrench=False), 1), (dict(energy=False, grad=False), 2)):
        one = dev_penalty(model, oset, torch, q, margin, w, None, pos, rot, **flags)
        assert [o is not None for o in one] == [i == k for i in range(3)] and np.array_equal(one[k], full[("E", "grad", "wrench")[k]])
    assert np.array_equal(dev_distances(model, oset, torch, q, None, pos, rot, nearest=False)[0], full["dist"])
    assert np.array_equal(dev_distances(model, oset, torch, q, None, pos, rot, dist=False)[1], full["nearest"])
    # B = 0: a no-op, NULL pointers and all
    lib, hs, ho = _lib.load(), model.handle, oset.device_set(0).handle
    assert lib.dexr_obstacle_distances_dev(hs, ho, 0, None, None, None, None, None, None, None) == 0
    assert lib.dexr_obstacle_distances_vjp_dev(hs, ho, 0, None, None, None, None, None, None, None) == 0
    assert lib.dexr_obstacle_penalty_dev(hs, ho, 0, None, None, None, None, 0.01, None, None, None, None, None) == 0
    assert lib.dexr_obstacle_penalty(hs, ho, 0, None, None, None, None, 0.01, None, None, None, None) == 0
    e, g, wr = model.obstacle_penalty(oset.device_set(0), np.zeros((0, model.n_in)), 0.01)
    assert e.shape == (0,) and g.shape == (0, model.n_in) and wr.shape == (0, 6)


# ---- 6. the penalty's gradient against the VJP fed with the nearest-only force, on a one-primitive set ----------------------------------
@functools.lru_cache(maxsize=None)
def one_box_case():
    d = obstacle_inputs("shadow_hand_right")
    full = obstacles()
    oset = collision.ObstacleSet(full.kinds[4:5], full.params[4:5])
    assert oset.kinds.tolist() == [oref.BOX]
    return d, oset, make_case(d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"], oset, d["pos"], d["rot"], None, d["gd"], d["margin"])


def test_penalty_gradient_equals_the_vjp_of_its_forces(require_gpu):
    torch = pytest.importorskip("torch")
    d, oset, case = one_box_case()
    model = robot_model("shadow_hand_right")
    w = np.array([1.5])
    dist, near = dev_distances(model, oset, torch, d["q"], None, d["pos"], d["rot"])
    h = np.maximum(np.float32(0), np.float32(d["margin"]) - dist)
    via = dev_vjp(model, oset, torch, d["q"], np.float32(-2) * np.float32(1.5) * h, None, d["pos"], d["rot"])
    _, g, _ = dev_penalty(model, oset, torch, d["q"], d["margin"], w, None, d["pos"], d["rot"])
    r64, r32 = case["r64"], case["r32"]
    gate = GATE32 * 1.5 * float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
    e = float(np.abs(via.astype(np.float64) - g).max())
    print(f"one box: max |penalty gradient - VJP of -2 w h| = {e:.3e} (gate {gate:.3e} = {GATE32:g} x the reference's float32 distance), "
          f"max |gradient| {np.abs(g).max():.3e}")
    assert (h > 0).any() and not near.any() and gate > 0 and e <= gate
    # float64: the same two routes within GATE64
    ho = oset.device_set(0)
    dist64 = model.obstacle_distances(ho, d["q"], None, d["pos"], d["rot"])[0]
    via64 = model.obstacle_distances_vjp(ho, d["q"], -2 * 1.5 * np.maximum(0.0, d["margin"] - dist64), None, d["pos"], d["rot"])
    assert np.abs(via64 - model.obstacle_penalty(ho, d["q"], d["margin"], w, None, d["pos"], d["rot"])[1]).max() <= GATE64


# ---- 7. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    model, oset = robot_model("allegro_hand_right"), obstacles()
    n, S, M = 4, model.n_sphere, oset.n_prim
    x = torch.zeros((n, model.n_in), dtype=torch.float32, device="cuda")
    gd = torch.ones((n, S), dtype=torch.float32, device="cuda")
    w = torch.ones((M,), dtype=torch.float32, device="cuda")
    dist, e, gx, wr = _nan(torch, (n, S)), _nan(torch, (n,)), _nan(torch, (n, model.n_in)), _nan(torch, (n, 6))
    near = torch.full((n, S), -1, dtype=torch.int32, device="cuda")
    h, o, xp = model.handle, oset.device_set(torch.cuda.current_device()).handle, x.data_ptr()
    INVALID = -1

    def invalid(rc, word=None):
        assert rc == INVALID
        msg = lib.dexr_last_error()
        assert len(msg) > 0 and (word is None or word in msg), msg

    D, V, P = lib.dexr_obstacle_distances_dev, lib.dexr_obstacle_distances_vjp_dev, lib.dexr_obstacle_penalty_dev
    invalid(D(None, o, n, xp, None, None, None, dist.data_ptr(), None, None), b"null sphere model")
    invalid(D(h, None, n, xp, None, None, None, dist.data_ptr(), None, None), b"null obstacle set")
    invalid(D(h, o, -1, xp, None, None, None, dist.data_ptr(), None, None), b"negative")
    invalid(D(h, o, n, None, None, None, None, dist.data_ptr(), near.data_ptr(), None), b"x is NULL")
    invalid(D(h, o, n, xp, None, None, None, None, None, None), b"both NULL")
    invalid(V(None, o, n, xp, None, None, None, gd.data_ptr(), gx.data_ptr(), None), b"null sphere model")
    invalid(V(h, None, n, xp, None, None, None, gd.data_ptr(), gx.data_ptr(), None), b"null obstacle set")
    invalid(V(h, o, n, xp, None, None, None, None, gx.data_ptr(), None), b"grad_dist is NULL")
    invalid(V(h, o, n, xp, None, None, None, gd.data_ptr(), None, None), b"grad_x_out is NULL")
    invalid(V(h, o, n, None, None, None, None, gd.data_ptr(), gx.data_ptr(), None), b"x is NULL")
    invalid(P(None, o, n, xp, None, None, None, 0.01, None, e.data_ptr(), gx.data_ptr(), wr.data_ptr(), None), b"null sphere model")
    invalid(P(h, None, n, xp, None, None, None, 0.01, None, e.data_ptr(), gx.data_ptr(), wr.data_ptr(), None), b"null obstacle set")
    invalid(P(h, o, -3, xp, None, None, None, 0.01, None, e.data_ptr(), gx.data_ptr(), wr.data_ptr(), None), b"negative")
    invalid(P(h, o, n, xp, None, None, None, 0.01, w.data_ptr(), None, None, None, None), b"all NULL")
    invalid(P(h, o, n, None, None, None, None, 0.01, None, e.data_ptr(), gx.data_ptr(), None, None), b"x is NULL")
    for bad in (-1e-6, -1.0, float("nan"), float("inf"), -float("inf")):
        invalid(P(h, o, n, xp, None, None, None, bad, None, e.data_ptr(), gx.data_ptr(), wr.data_ptr(), None), b"margin")
    # a model that reads fixed columns
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.sphere_model(collision.SphereSet(["link_15.0_tip", "link_3.0_tip"], np.zeros((2, 3)), [0.01, 0.01], [(0, 1)]))
    assert ms.n_fixed == 6 and ms.n_in == 10
    invalid(P(ms.handle, o, n, xp, None, None, None, 0.01, None, e.data_ptr(), None, None, None), b"fixed")
    invalid(D(ms.handle, o, n, xp, None, None, None, dist.data_ptr(), None, None), b"fixed")
    # the host twins keep the same rules
    z, zg, zw = np.zeros((n, model.n_in)), np.ones((n, S)), np.ones(M)
    zd, ze, zx, zr = np.full((n, S), np.nan), np.full(n, np.nan), np.full((n, model.n_in), np.nan), np.full((n, 6), np.nan)
    zn = np.full((n, S), -1, np.int32)
    dp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    ip = zn.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))
    invalid(lib.dexr_obstacle_distances(None, o, n, dp(z), None, None, None, dp(zd), ip), b"null sphere model")
    invalid(lib.dexr_obstacle_distances(h, None, n, dp(z), None, None, None, dp(zd), ip), b"null obstacle set")
    invalid(lib.dexr_obstacle_distances(h, o, -2, dp(z), None, None, None, dp(zd), ip), b"negative")
    invalid(lib.dexr_obstacle_distances(h, o, n, None, None, None, None, dp(zd), ip), b"x is NULL")
    invalid(lib.dexr_obstacle_distances(h, o, n, dp(z), None, None, None, None, None), b"both NULL")
    invalid(lib.dexr_obstacle_distances_vjp(h, o, n, dp(z), None, None, None, None, dp(zx)), b"grad_dist is NULL")
    invalid(lib.dexr_obstacle_distances_vjp(h, o, n, dp(z), None, None, None, dp(zg), None), b"grad_x_out is NULL")
    invalid(lib.dexr_obstacle_penalty(h, o, n, dp(z), None, None, None, 0.01, dp(zw), None, None, None), b"all NULL")
    for bad in (-1.0, float("nan"), float("inf")):
        invalid(lib.dexr_obstacle_penalty(h, o, n, dp(z), None, None, None, bad, None, dp(ze), dp(zx), dp(zr)), b"margin")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dist, e, gx, wr)) and bool((near == -1).all())  # nothing was launched
    assert all(np.isnan(a).all() for a in (zd, ze, zx, zr)) and (zn == -1).all()
    ho = oset.device_set(0)
    with pytest.raises(ValueError, match="shape"):
        model.obstacle_distances_vjp(ho, z, zg[:, :-1])
    with pytest.raises(ValueError, match="shape"):
        model.obstacle_penalty(ho, z, 0.01, zw[:-1])
    with pytest.raises(ValueError, match="shape"):
        model.obstacle_distances(ho, z, None, np.zeros((n, 2)))
    with pytest.raises(ValueError, match="shape"):
        model.obstacle_distances(ho, z, None, None, np.zeros((n, 9)))
    with pytest.raises(ValueError, match="shape"):
        model.obstacle_distances(ho, z[:, :-1])


# ---- 8. autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_autograd_reaches_q_and_the_obstacle_position(rel, require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    opt, prob, links, sset, x, fixed, q_full, pos, rot, oset, w, fold, case = order_case(rel)
    q, f, wt, pt, rt = (_dev(torch, a) for a in (x, fixed if fixed.shape[1] else None, w, pos, rot))
    model = opt.sphere_model(sset)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        E, g, wr = collision.obstacle_penalty(opt, q, sset, oset, MARGIN, pt, rt, wt, f, wrench=True)
        assert not E.requires_grad and bool((E > 0).any())
        qg, pg = q.clone().requires_grad_(True), pt.clone().requires_grad_(True)
        Eg = ag.obstacle_penalty(opt, qg, sset, oset, MARGIN, pg, rt, wt, f)
        assert Eg.requires_grad and torch.equal(Eg.detach(), E)
        Eg.sum().backward()
        assert torch.equal(qg.grad, g) and torch.equal(pg.grad, wr[:, :3]) and float(pg.grad.abs().max()) > 0
        # a weighted sum of the energies scales the rows; q alone, the position alone
        scale = torch.linspace(0.5, 2.0, B, device="cuda")
        qh = q.clone().requires_grad_(True)
        (ag.obstacle_penalty(opt, qh, sset, oset, MARGIN, pt, rt, wt, f) * scale).sum().backward()
        assert torch.equal(qh.grad, scale[:, None] * g)
        ph = pt.clone().requires_grad_(True)
        (ag.obstacle_penalty(opt, q, sset, oset, MARGIN, ph, rt, wt, f) * scale).sum().backward()
        assert torch.equal(ph.grad, scale[:, None] * wr[:, :3])
        # no gradient asked: the same energy, no graph
        En = ag.obstacle_penalty(opt, q, sset, oset, MARGIN, pt, rt, wt, f)
        assert torch.equal(En, E) and not En.requires_grad
        with pytest.raises(ValueError, match="wrench=True"):
            ag.obstacle_penalty(opt, q, sset, oset, MARGIN, pt, rt.clone().requires_grad_(True), wt, f)
        # the distances: backward is the VJP launch
        dist = collision.obstacle_distances(opt, q, sset, oset, pt, rt, f)
        qd = q.clone().requires_grad_(True)
        dg = ag.obstacle_distances(opt, qd, sset, oset, pt, rt, f)
        assert torch.equal(dg.detach(), dist)
        cot = _dev(torch, case["gd"])
        dg.backward(cot)
        want = _nan(torch, (B, model.n_in))
        model.obstacle_distances_vjp_dev(_handle(torch, oset), B, q.data_ptr(), _ptr(f), cot.data_ptr(), want.data_ptr(), pt.data_ptr(), rt.data_ptr(),
                                         stream=side.cuda_stream)
        assert torch.equal(qd.grad, want) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
        # non-contiguous inputs: views with the same values
        qn, pn, rn = torch.stack([q, q], 2)[:, :, 0], torch.stack([pt, pt], 2)[:, :, 1], torch.stack([rt, rt], 3)[:, :, :, 0]
        assert not qn.is_contiguous() and not pn.is_contiguous() and not rn.is_contiguous()
        a = collision.obstacle_penalty(opt, qn, sset, oset, MARGIN, pn, rn, wt, f, wrench=True)
        assert all(torch.equal(u, v) for u, v in zip(a, (E, g, wr)))
        # the robot_* twins over the full qpos
        robot = opt.robot
        rl = robot.joint_limits
        qr = _dev(torch, np.random.default_rng(233).uniform(rl[:, 0], rl[:, 1], (B, robot.dof)))
        rm = robot.sphere_model(sset)
        Er, gr, wrr = collision.robot_obstacle_penalty(robot, qr, sset, oset, MARGIN, pt, rt, wrench=True)
        we, wg, ww = _nan(torch, (B,)), _nan(torch, (B, robot.dof)), _nan(torch, (B, 6))
        rm.obstacle_penalty_dev(_handle(torch, oset), B, qr.data_ptr(), 0, MARGIN, 0, we.data_ptr(), wg.data_ptr(), ww.data_ptr(), pt.data_ptr(),
                                rt.data_ptr(), stream=side.cuda_stream)
        assert torch.equal(Er, we) and torch.equal(gr, wg) and torch.equal(wrr, ww)
        qrg = qr.clone().requires_grad_(True)
        ag.robot_obstacle_penalty(robot, qrg, sset, oset, MARGIN, pt, rt).sum().backward()
        assert torch.equal(qrg.grad, wg)
        assert torch.equal(ag.robot_obstacle_distances(robot, qr, sset, oset, pt, rt), collision.robot_obstacle_distances(robot, qr, sset, oset, pt, rt))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e0 = torch.zeros((0, opt.opt_dof), device="cuda")
    E0, g0, w0 = collision.obstacle_penalty(opt, e0, sset, oset, MARGIN, pt[:0], rt[:0], None, None if f is None else f[:0], wrench=True)
    assert E0.shape == (0,) and g0.shape == (0, opt.opt_dof) and w0.shape == (0, 6)
    assert collision.obstacle_distances(opt, e0, sset, oset, fixed_qpos=None if f is None else f[:0]).shape == (0, model.n_sphere)


def test_keypoints_to_obstacle_loss_end_to_end(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    rel = "teleop/allegro_hand_right.yml"
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    n = 256
    d = cases.human_set(prob, n)
    links = [f.name for f in opt.robot.kin.frames]
    S = len(links)
    sset = collision.SphereSet(links, np.zeros((S, 3)), np.full(S, 0.02), [(i, j) for i in range(S) for j in range(i + 1, S)])
    # a ball of 8 cm radius centred 5 cm from the hand's centroid, above a table: every frame has spheres inside it
    oset = collision.ObstacleSet.spheres([[0.0, 0.0, 0.0]], [0.08]) + collision.ObstacleSet.half_spaces([[0.0, 0.0, 1.0]], [-0.2])
    kp = glp._t(d["kp"], torch, dtype=torch.float32, requires_grad=True)
    last = glp._t(d["last"], torch, requires_grad=True)
    fixed = glp._t(d["fixed"], torch) if d["fixed"].shape[1] else None
    q = ag.retarget(opt, ag.ref_value_from_keypoints(opt, kp), last, fixed, None)
    centre = collision.sphere_distances(opt, q.detach(), sset, fixed, centers=True)[1].mean(1)  # (n, 3): the hand's centroid
    pos = (centre + torch.tensor([0.0, 0.0, 0.05], device="cuda")).requires_grad_(True)
    E = ag.obstacle_penalty(opt, q, sset, oset, 0.01, pos, None, None, fixed)
    assert E.shape == (n,) and bool((E > 0).all())
    E.sum().backward()
    assert bool(torch.isfinite(kp.grad).all()) and float(kp.grad.abs().max()) > 0
    assert bool(torch.isfinite(last.grad).all()) and bool(torch.isfinite(pos.grad).all()) and float(pos.grad.abs().max()) > 0
    # grad_q of the loss is the no-graph call's
    _, g = collision.obstacle_penalty(opt, q.detach(), sset, oset, 0.01, pos.detach(), None, None, fixed)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0

"""CPU tests of the collision-aware posture solve's interface (include/dexr_resolve.h, dex_retargeting_amd/collision.py): the export
list and the constants against the header, the argument rules of the torch front (every one a ValueError before any device call),
the cache keys of the sphere models with and without target links, and the yardstick tests/resolve_reference.py on the inputs of
tests/test_gpu_resolve.py, so that they are proven before a GPU sees them.

INPUTS (resolve_inputs; shared with the GPU tests).  The eight robots, the "origins" geometry of test_collision_host.collision_inputs
(a sphere of radius 0.010 at every link origin, B = 33 postures uniform inside the limits) with default_pairs(robot, set, 2) -- on
the gripper, whose three links are never more than two joints apart, default_pairs(robot, set, 0).  margin 0.010, collision weight 1,
posture weight 1e-4 on every column, damping 1e-4, max_step 0.2, tol 0, the robot's joint limits; every scalar rounded to float32
so that the float32 and the float64 runs start from the same numbers.

DECISION GUARDS.  The accept / reject rule compares two energies and the curvature takes a pair in or out at the margin: float32
rounding can flip either, after which two runs are different, equally valid, descents.  A frame is CLEAR at guards (gd, ge) when no
pair came within gd metres of the margin at any evaluated point and no accept test had |Et - E| / E within ge.  float64
comparisons use (1e-10, 1e-9); float32 comparisons (1e-5, 1e-3): 1e-5 m is about 100 times the 1e-7 m that float32 FK rounds a
0.3 m hand to, 1e-3 is 50 times the 2e-5 relative error of a float32 h^2 at h = 1 cm.  Frames that are not clear are never dropped:
the GPU tests put them through the functional checks (finite, inside the limits, E does not rise)."""
import functools
import os
import re

import numpy as np
import pytest

import resolve_reference as rr
from testutil import REPO
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import ARM, B, GRIPPER, MARGIN, ROBOTS, collision_inputs, robot_of
from test_jacobian_host import SUBSET_CFG

HEADER = os.path.join(REPO, "include", "dexr_resolve.h")
GUARD64, GUARD32 = (1e-10, 1e-9), (1e-5, 1e-3)
STEPS64, STEPS32 = 6, 3


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _f32(v):
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def resolve_inputs(name):
    """dict: the geometry of collision_inputs(name, "origins") with the pairs of this file, the limits and the scalars; read-only."""
    d = dict(collision_inputs(name, "origins"))
    robot, orc = robot_of(name)
    pairs = collision.default_pairs(robot, d["sset"], 0 if name == GRIPPER else 2)
    assert 1 <= len(pairs) <= _lib.SPHERE_MAXPAIR
    lim = _r32(orc.joint_limits)
    d.update(pairs=pairs, sset=collision.SphereSet(d["sset"].links, d["centers"], d["radii"], pairs), lo=lim[:, 0].copy(), hi=lim[:, 1].copy(),
             margin=_f32(MARGIN), u=np.full(orc.dof, _f32(1e-4)), damping=_f32(1e-4), max_step=_f32(0.2), tol=0.0, wcol=1.0)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def problem(d, dtype=np.float64, **over):
    kw = dict(posture_weight=d["u"], collision_weight=d["wcol"], dtype=dtype)
    kw.update(over)
    return rr.Problem(d["orc"], d["links"], kw.pop("n_target", 0), d["rows"], d["centers"], d["radii"], d["pairs"], d["margin"], **kw)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64, steps=STEPS64):
    """the yardstick's run on resolve_inputs(name), trial by trial, computed once and shared, read-only."""
    d = resolve_inputs(name)
    res = rr.resolve(problem(d, dtype), d["q"], d["damping"], steps, d["lo"], d["hi"], d["tol"], d["max_step"])
    for v in res.values():
        v.setflags(write=False)
    return res


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_constants_are_the_header():
    declared = _declared(HEADER)
    assert declared == set(_lib.RESOLVE_EXPORTS) and len(_lib.RESOLVE_EXPORTS) == 2 and len(set(_lib.RESOLVE_EXPORTS)) == 2
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS, _lib.WRENCH_EXPORTS, _lib.IK_EXPORTS, _lib.IK_SOLVE_EXPORTS, _lib.SPHERE_EXPORTS):
        assert not set(_lib.RESOLVE_EXPORTS) & set(other)
    lib = _lib.load()
    for name in _lib.RESOLVE_EXPORTS:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in ("dexr_spheres.h", "dexr_ik_solve.h", "dexr_ik.h", "dexr_wrench.h", "dexr_jacobian.h", "dexr_pose.h", "dexr.h"):
        assert not _declared(os.path.join(REPO, "include", h)) & declared
    text = open(HEADER).read()
    define = lambda n: int(re.search(rf"#define DEXR_RESOLVE_{n} (\d+)", text).group(1))  # noqa: E731
    assert define("MAXACTIVE") == _lib.RESOLVE_MAXACTIVE == rr.MAXACTIVE == 256
    assert define("LAM_UP") == _lib.RESOLVE_LAM_UP == rr.LAM_UP == 8 and define("LAM_DOWN") == _lib.RESOLVE_LAM_DOWN == rr.LAM_DOWN == 4
    assert define("MAXREJECT") == _lib.RESOLVE_MAXREJECT == rr.MAXREJECT == 12
    assert (define("CONVERGED"), define("STALLED"), define("TRUNCATED")) == (1, 2, 4)
    assert (_lib.RESOLVE_CONVERGED, _lib.RESOLVE_STALLED, _lib.RESOLVE_TRUNCATED) == (rr.CONVERGED, rr.STALLED, rr.TRUNCATED) == (1, 2, 4)
    assert "resolve_self_collision" in collision.__all__ and "robot_resolve_self_collision" in collision.__all__
    src = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_resolve.hpp")).read()
    assert "getenv" not in src and "atomic" not in src.replace("no atomics", "") and "asm" not in src.replace("__restrict__", "")
    for n in ("DEXR_RESOLVE_LAM_UP", "DEXR_RESOLVE_LAM_DOWN", "DEXR_RESOLVE_MAXREJECT", "DEXR_RESOLVE_MAXACTIVE"):
        assert n in src  # the kernel reads the named constants, not numbers of its own


# ---- 2. the argument rules of the torch front -----------------------------------------------------------------------------------------
def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    touched = []
    for cls in (_lib.SphereModel, _lib.PoseModel):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("resolve_dev", "penalty_dev", "distances_dev"):
        monkeypatch.setattr(_lib.SphereModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "base_link"]
    sset = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    n_pair = len(collision.default_pairs(opt.robot, sset))
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    names = ["link_11.0_tip", "link_3.0_tip"]
    p = torch.zeros((4, 2, 3), dtype=torch.float32)
    r = torch.eye(3, dtype=torch.float32).expand(4, 2, 3, 3).contiguous()
    w = torch.ones((4, 2), dtype=torch.float32)
    pw = torch.ones((n_pair,), dtype=torch.float32)
    u = torch.ones((16,), dtype=torch.float32)
    lim = torch.tensor([[-1.0, 1.0]] * 16, dtype=torch.float32)
    fronts = [lambda q, s, *a, **k: collision.resolve_self_collision(opt, q, s, *a, **k),
              lambda q, s, *a, **k: collision.robot_resolve_self_collision(opt.robot, q, s, *a, **k)]

    def raises(match=None, q=good, s=sset, **kw):
        kw.setdefault("margin", 0.01)
        kw.setdefault("damping", 1e-4)
        kw.setdefault("max_iters", 8)
        for f in fronts:
            with pytest.raises(ValueError, match=match):
                f(q, s, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises("CUDA")
    raises("CUDA", posture_weight=1e-4, q_ref=good, collision_weight=2.0, pair_weight=pw, tol=1e-6, max_step=0.2, limits=lim)
    raises("CUDA", posture_weight=u, link_names=names, target_pos=p, target_rot=r, pos_weight=w, rot_weight=w)
    raises("CUDA", margin=0, damping=1, max_iters=1, collision_weight=0, posture_weight=0, tol=0, max_step=0)  # Python ints are numbers too
    raises("CUDA", max_iters=256, link_names=names, target_rot=r)
    with pytest.raises(ValueError, match="CUDA"):  # the positional order of the issue
        collision.resolve_self_collision(opt, good, sset, 0.01, 1e-4, 8, 1e-4, good, 1.0, pw, names, p, r, w, w, 0.0, 0.2, lim, None)
    # dtypes, shapes, types
    raises("float32", q=good.double())
    for name, t in (("q_ref", good), ("posture_weight", u), ("limits", lim), ("pair_weight", pw)):
        raises("float32", **{name: t.double()})
        raises("torch tensor" if name != "posture_weight" else "posture_weight", **{name: t.numpy()})
    for name, t in (("target_pos", p), ("target_rot", r)):
        raises("float32", link_names=names, **{name: t.double()})
        raises("torch tensor", link_names=names, **{name: t.numpy()})
    raises("float32", link_names=names, target_pos=p, pos_weight=w.double())
    raises("float32", link_names=names, target_rot=r, rot_weight=w.long())
    for bad in (good[:3], good[:, :15], torch.zeros((4, 16, 1))):
        raises("shape", q_ref=bad)
    for bad in (u[:15], u[None], torch.ones((17,))):
        raises("shape", posture_weight=bad)
    for bad in (lim[:15], lim.t(), lim.reshape(-1)):
        raises("shape", limits=bad)
    for bad in (pw[:-1], pw[None]):
        raises("shape", pair_weight=bad)
    for bad in (p[:3], p[:, :1], p[:, :, :2], torch.zeros((4, 3, 3))):
        raises("shape", link_names=names, target_pos=bad)
    for bad in (r[:3], r[:, :1], r[..., :2], p):
        raises("shape", link_names=names, target_rot=bad)
    for bad in (w[:3], w[:, :1], w.reshape(-1)):
        raises("shape", link_names=names, target_pos=p, pos_weight=bad)
        raises("shape", link_names=names, target_rot=r, rot_weight=bad)
    for bad in (good[:, :15], good.reshape(-1)):
        raises("shape", q=bad)
    raises("torch tensor", q=good.numpy())
    # the sphere set and the links
    raises("SphereSet", s=tips)
    raises("is not a link name", s=collision.SphereSet(["link_15.0_tip", "no_such_link"], np.zeros((2, 3)), [0.01, 0.01]))
    raises("0 pairs", s=collision.SphereSet(["link_15.0_tip", "link_15.0"], np.zeros((2, 3)), [0.01, 0.01]))
    raises("is not a link name", link_names=["link_3.0_tip", "no_such_link"], target_pos=p)
    raises("link_names", link_names="link_3.0_tip", target_pos=p)
    raises("link_names", link_names=[], target_pos=p)
    raises("need link_names", target_pos=p)
    raises("need link_names", rot_weight=w)
    raises("both None", link_names=names)
    raises("pos_weight given without target_pos", link_names=names, target_rot=r, pos_weight=w)
    raises("rot_weight given without target_rot", link_names=names, target_pos=p, rot_weight=w)
    many = [f.name for f in opt.robot.kin.frames]
    assert len(many) < 62
    raises("at most 64", link_names=(many * 4)[:65], target_pos=torch.zeros((4, 65, 3), dtype=torch.float32))
    # the scalars
    for f in fronts:
        with pytest.raises(TypeError):
            f(good, sset)  # margin is positional
        with pytest.raises(ValueError, match="damping is required"):
            f(good, sset, 0.01, max_iters=8)
        with pytest.raises(ValueError, match="max_iters is required"):
            f(good, sset, 0.01, 1e-4)
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.01), None, "0.01", True):
        raises("margin", margin=bad)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), torch.tensor(1e-3), None, "1e-3", True):
        raises("damping", damping=bad)
    for bad in (0, -1, 257, 8.0, float("nan"), torch.tensor(8), None, "8", True):
        raises("max_iters", max_iters=bad)
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.0), None, "0", True):
        raises("tol", tol=bad)
        raises("max_step", max_step=bad)
        raises("collision_weight", collision_weight=bad)
    for bad in (-1e-9, float("nan"), float("inf"), "0", True, [1e-4] * 16):
        raises("posture_weight", posture_weight=bad)
    # fixed_qpos: one too many, one missing, one of the wrong width
    with pytest.raises(ValueError, match="fixed_qpos"):
        collision.resolve_self_collision(opt, good, sset, 0.01, 1e-4, 8, fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    assert len(sub.idx_pin2fixed) == 6
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    for fq, word in ((None, "fixed_qpos"), (torch.zeros((4, 5), dtype=torch.float32), "fixed_qpos"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                     (torch.zeros((4, 6), dtype=torch.float32), "CUDA")):
        with pytest.raises(ValueError, match=word):
            collision.resolve_self_collision(sub, q10, sset, 0.01, 1e-4, 8, fixed_qpos=fq)
    with pytest.raises(ValueError, match="shape"):
        collision.resolve_self_collision(sub, q10, sset, 0.01, 1e-4, 8, limits=lim, fixed_qpos=torch.zeros((4, 6), dtype=torch.float32))
    assert touched == []


# ---- 3. the cache of the sphere models --------------------------------------------------------------------------------------------------
def test_sphere_models_are_cached_with_and_without_target_links(monkeypatch):
    made = []
    monkeypatch.setattr(_lib.SphereModel, "__init__", lambda self, blob, rows, cen, rad, pairs: made.append((list(rows), len(pairs))))
    tables = []
    from dex_retargeting_amd import pose_tables

    real = pose_tables.compile_poses
    monkeypatch.setattr(pose_tables, "compile_poses", lambda kin, links, smap=None: tables.append(list(links)) or real(kin, links, smap))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "link_3.0_tip"]  # the second link carries two spheres
    a = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    pairs = collision.default_pairs(opt.robot, a)
    for owner in (opt, opt.robot):
        made.clear(), tables.clear()
        m = owner.sphere_model(a)
        assert owner.sphere_model(a, pairs) is m and owner.sphere_model(a, None, ()) is m and owner.sphere_model(a, pairs, []) is m  # today's key: the set
        assert a in owner._sphere_models and made == [([0, 1, 2, 1], len(pairs))] and tables == [tips[:3]]
        # target links: a key of its own; the table is the targets in the caller's order, then the sphere links not among them
        tl = ["link_11.0_tip", "link_7.0_tip", "base_link"]
        t = owner.sphere_model(a, pairs, tl)
        assert t is not m and owner.sphere_model(a, pairs, tuple(tl)) is t and owner.sphere_model(a) is m
        assert tables[-1] == tl + ["link_15.0_tip", "link_3.0_tip"] and made[-1] == ([3, 4, 1, 4], len(pairs)) and len(made) == 2
        assert owner.sphere_model(a, pairs, tl[::-1]) is not t and tables[-1] == tl[::-1] + ["link_15.0_tip", "link_3.0_tip"]
        assert owner.sphere_model(a, pairs[:1], tl) is not t and made[-1][1] == 1 and len(made) == 4
        assert collision.sphere_model_key(a, pairs, tl) in owner._sphere_models and collision.sphere_model_key(a, pairs, ()) is a
    n = len(opt._sphere_models)
    opt.set_kinematic_adaptor(opt.adaptor)
    assert n == 4 and len(opt._sphere_models) == 0


# ---- 4. the yardstick: g is -1/2 the gradient of its E ------------------------------------------------------------------------------
H, GATE_E = 1e-6, 1e-6  # the step and the gate of test_collision_host's energy check (see its docstring: E is C1 only)


@pytest.mark.parametrize("name", ["allegro_hand_right", "shadow_hand_right"])
def test_reference_g_is_minus_half_the_central_difference_of_its_energy(name):
    """Every term of E at once: position and rotation targets on the first three links of the table, a posture term towards a
    reference away from x, weighted pairs.  The central difference errs by H^2 |E'''| / 6 + eps |E| / H: E <= 1 (rotation errors
    of a radian), so 1e-10 at most, plus the C1 caveat of the collision term (5e-7 at the very worst); gate 1e-6 on g, which is
    HALF the gradient the collision check gates with 1e-6."""
    d = resolve_inputs(name)
    rng = np.random.default_rng(41)
    x = d["q"][:4].copy()
    n, nt, L = x.shape[1], 3, len(d["links"])
    links = d["links"][-nt:] + d["links"][:-nt]  # the last three links of the robot are the target rows, in front of the table
    p, R = rr.isr.link_poses(d["orc"], _r32(x + rng.uniform(-0.2, 0.2, x.shape)), links[:nt])
    d = dict(d, links=links, rows=(d["rows"] + nt) % L)
    P = problem(d, n_target=nt, tgt_pos=p, tgt_rot=R, w_pos=rng.uniform(0.5, 2, (4, nt)), w_rot=rng.uniform(0.01, 0.1, (4, nt)),
                x_ref=x + rng.uniform(-0.3, 0.3, x.shape), posture_weight=rng.uniform(0, 1e-2, n), pair_weight=rng.uniform(0.5, 2, len(d["pairs"])),
                collision_weight=1.5)
    E3, h, _ = P.energies(x)
    g, Hm = P.system(x, h)
    assert (E3[:, :2] > 0).all() and (h > 0).any() and np.allclose(Hm, Hm.transpose(0, 2, 1), rtol=0, atol=1e-12) and np.linalg.eigvalsh(Hm).min() > -1e-9
    worst = 0.0
    for c in range(n):
        xp, xm = x.copy(), x.copy()
        xp[:, c] += H
        xm[:, c] -= H
        cd = (P.energies(xp)[0].sum(1) - P.energies(xm)[0].sum(1)) / (2 * H)
        worst = max(worst, float(np.abs(g[:, c] + 0.5 * cd).max()))
    print(f"{name}: max |g + 1/2 central difference of E| = {worst:.3e} (gate {GATE_E:.0e}), max |g| = {np.abs(g).max():.3e}")
    assert worst <= GATE_E


# ---- 5. the yardstick on the inputs of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_reference_descends_monotonically_and_most_frames_are_clear(name):
    assert len(ROBOTS) == 8 and ARM in ROBOTS and GRIPPER in ROBOTS
    d, res = resolve_inputs(name), reference(name)
    E = res["energy"].sum(-1)
    dec = res["decisions"]
    assert res["xs"].shape == (STEPS64 + 1, B, d["orc"].dof) and np.isfinite(res["xs"]).all()
    assert (np.diff(E, axis=0) <= 0).all(), "an accepted trial raised E"
    assert ((res["xs"] >= d["lo"]) & (res["xs"] <= d["hi"])).all()
    moved = np.abs(np.diff(res["xs"], axis=0)).max(-1) > 0
    assert not (moved & (dec != 1)).any()  # only an accepted trial moves the point
    clear32, clear64 = rr.clear(res, STEPS32, *GUARD32), rr.clear(res, STEPS64, *GUARD64)
    print(f"{name}: {len(d['pairs'])} pairs; over {STEPS64} trials {int((dec == 1).sum())} accepted, {int((dec == 0).sum())} rejected; median E "
          f"{np.median(E[0]):.2e} -> {np.median(E[STEPS32]):.2e} -> {np.median(E[-1]):.2e}; clear frames: {int(clear32.sum())} of {B} at the float32 "
          f"guards over {STEPS32} trials, {int(clear64.sum())} at the float64 guards over {STEPS64}; status counts {np.bincount(res['status'][-1], minlength=8)}")
    assert 2 * clear32.sum() >= B and 2 * clear64.sum() >= B, name
    assert not (res["status"] & rr.TRUNCATED).any()
    if name != GRIPPER:
        assert (dec == 1).any() and (dec == 0).any(), "the runs must hold accepted and rejected trials"

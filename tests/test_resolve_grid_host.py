"""CPU tests of the posture solve against a signed-distance grid's interface (include/dexr_resolve_grid.h,
dex_retargeting_amd/collision.py): the export list against the header, the place and the contents of the fragment, the argument rules
of the torch fronts (every one a ValueError before any device call), and the yardstick tests/resolve_grid_reference.py on the inputs
of tests/test_gpu_resolve_grid.py, so that they are proven before a GPU sees them.

INPUTS (shared with the GPU tests).  resolve_obstacle_inputs(name) of tests/test_resolve_obstacle_host.py as it stands: the
"origins" geometry, B = 33, margin 0.010, one seeded obstacle pose per frame (seed 64, 65 for the gripper), every fourth frame 2 m
away, obstacle_margin = margin, obstacle weight 1.  In the place of its primitives stands GRID_A = grid_a() of
tests/test_grid_host.py, those primitives sampled on 17^3; on Allegro and Shadow also GRID_P = grid_p(), the polynomial grid, whose
interpolant has no kink at a cell face.

DECISION GUARDS: GUARD64, GUARD32, STEPS64, STEPS32 of tests/test_resolve_host.py, unchanged, with a `gap` that also covers the
contacts and the faces of the cells of active spheres (resolve_grid_reference).  At least NEED = 17 of the 33 frames must be clear at
both guards on every robot, the sibling's condition.

CENTRAL DIFFERENCES: step H = 1e-6 and gate GATE_E of tests/test_resolve_host.py; on the frames whose every sphere is further than
FD_GAP = 1e-5 m from a face or clamp plane: a step moves a sphere by less than H x 0.5 m/rad = 5e-7 m, so that every sphere stays in
its cell, where the field is a polynomial."""
import functools
import os

import numpy as np
import pytest

import resolve_grid_reference as rgr
import resolve_reference as rr
from testutil import REPO
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, GRIPPER, ROBOTS
from test_grid_host import FD_GAP, grid_a, grid_p
from test_jacobian_host import SUBSET_CFG
from test_resolve_host import GATE_E, GUARD32, GUARD64, H, STEPS32, STEPS64, _declared, _r32, problem
from test_resolve_obstacle_host import NEED, OKEYS, pose_seed, resolve_obstacle_inputs

HEADER = os.path.join(REPO, "include", "dexr_resolve_grid.h")
FRAGMENT = os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_resolve_grid.hpp")
GRIDS = {"A": grid_a, "P": grid_p}


@functools.lru_cache(maxsize=None)
def resolve_grid_inputs(name, which="A"):
    """dict: resolve_obstacle_inputs(name) and `grid` (GRID_A or GRID_P); read-only."""
    d = dict(resolve_obstacle_inputs(name), grid=GRIDS[which]())
    return d


def grid_problem(d, dtype=np.float64, **over):
    """the yardstick's Problem of a dict of resolve_grid_inputs (keys a run does not have are absent: None)."""
    kw = dict(posture_weight=d.get("u"), collision_weight=d["wcol"], dtype=dtype, obstacle_margin=d["omargin"], opos=d.get("pos"), orot=d.get("rot"),
              obstacle_weight=d["wobs"])
    kw.update({k: d[k] for k in OKEYS if d.get(k) is not None})
    kw.update(over)
    g = d["grid"]
    return rgr.Problem(d["orc"], d["links"], kw.pop("n_target", 0), d["rows"], d["centers"], d["radii"], d["pairs"], d["margin"], g.values, g.origin,
                       g.spacing, **kw)


def reference_run(d, steps, dtype=np.float64, **over):
    return rgr.resolve(grid_problem(d, dtype, **over), d["q"], d["damping"], steps, d.get("lo"), d.get("hi"), d["tol"], d["max_step"])


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64, steps=STEPS64, which="A"):
    """the yardstick's run on resolve_grid_inputs(name, which), trial by trial, computed once and shared, read-only."""
    res = reference_run(resolve_grid_inputs(name, which), steps, dtype)
    for v in res.values():
        v.setflags(write=False)
    return res


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_the_header_and_the_fragment_is_in_its_place():
    declared = _declared(HEADER)
    exports = _lib.RESOLVE_GRID_EXPORTS
    assert declared == set(exports) == {"dexr_sphere_resolve_grid_dev", "dexr_sphere_resolve_grid"} and len(exports) == 2
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS, _lib.WRENCH_EXPORTS, _lib.IK_EXPORTS, _lib.IK_SOLVE_EXPORTS, _lib.SPHERE_EXPORTS,
                  _lib.RESOLVE_EXPORTS, _lib.OBSTACLE_EXPORTS, _lib.RESOLVE_OBSTACLE_EXPORTS, _lib.SDF_GRID_EXPORTS):
        assert not set(exports) & set(other)
    lib = _lib.load()
    for name in exports:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h != "dexr_resolve_grid.h":
            assert not _declared(os.path.join(REPO, "include", h)) & declared, h
    text = open(HEADER).read()
    assert '#include "dexr_sdf_grid.h"' in text and '#include "dexr_resolve.h"' in text and "#define" not in text.split("#define DEXR_RESOLVE_GRID_H")[1]
    assert "DEXR_RESOLVE_CONTACTS_TRUNCATED of dexr_resolve_obstacles.h is never set" in text and "DEXR_SPHERE_MAX = 128" in text
    assert _lib.SPHERE_MAX == 128
    assert (rgr.MAXACTIVE, rgr.LAM_UP, rgr.LAM_DOWN, rgr.MAXREJECT) == (_lib.RESOLVE_MAXACTIVE, _lib.RESOLVE_LAM_UP, _lib.RESOLVE_LAM_DOWN, _lib.RESOLVE_MAXREJECT)
    assert (rgr.CONVERGED, rgr.STALLED, rgr.TRUNCATED, rgr.CONTACTS_TRUNCATED) == (_lib.RESOLVE_CONVERGED, _lib.RESOLVE_STALLED, _lib.RESOLVE_TRUNCATED,
                                                                                 _lib.RESOLVE_CONTACTS_TRUNCATED)
    assert "resolve_grid_collisions" in collision.__all__ and "robot_resolve_grid_collisions" in collision.__all__
    assert hasattr(_lib.SphereModel, "resolve_grid_dev") and hasattr(_lib.SphereModel, "resolve_grid")
    src = open(FRAGMENT).read()
    assert "getenv" not in src and "atomic" not in src.replace("no atomics", "") and "asm" not in src.replace("__restrict__", "")
    for n in ("DEXR_RESOLVE_LAM_UP", "DEXR_RESOLVE_LAM_DOWN", "DEXR_RESOLVE_MAXREJECT", "DEXR_RESOLVE_MAXACTIVE"):
        assert n in src  # the kernel reads the named constants, not numbers of its own
    assert "DEXR_RESOLVE_MAXCONTACT" not in src and "DEXR_RESOLVE_CONTACTS_TRUNCATED" not in src  # no cap, no bit
    assert src.count('#include "') == 1 and '#include "dexr_resolve_grid.h"' in src  # (a fragment: no unit of its own)
    assert "grid_sdf<T, true>" in src and "V[" not in src  # every lookup goes through grid_sdf and its clamps
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_resolve_grid.hpp"') == 1 and pose.count("dexr_resolve_grid.hpp") == 1
    assert pose.index('"dexr_resolve_grid.hpp"') > pose.index('"dexr_sdf_grid.hpp"')


# ---- 2. the argument rules of the torch fronts ----------------------------------------------------------------------------------------
def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    touched = []
    for cls in (_lib.SphereModel, _lib.PoseModel, _lib.ObstacleSet, _lib.SdfGrid):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("resolve_grid_dev", "resolve_obstacles_dev", "resolve_dev", "grid_penalty_dev", "penalty_dev"):
        monkeypatch.setattr(_lib.SphereModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "base_link"]
    sset = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    grid = grid_a()
    n_pair = len(collision.default_pairs(opt.robot, sset))
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    names = ["link_11.0_tip", "link_3.0_tip"]
    p = torch.zeros((4, 2, 3), dtype=torch.float32)
    r = torch.eye(3, dtype=torch.float32).expand(4, 2, 3, 3).contiguous()
    w = torch.ones((4, 2), dtype=torch.float32)
    pw = torch.ones((n_pair,), dtype=torch.float32)
    u = torch.ones((16,), dtype=torch.float32)
    lim = torch.tensor([[-1.0, 1.0]] * 16, dtype=torch.float32)
    pos, rot = torch.zeros((4, 3), dtype=torch.float32), torch.eye(3, dtype=torch.float32).repeat(4, 1, 1)
    fronts = [lambda q, s, o, *a, **k: collision.resolve_grid_collisions(opt, q, s, o, *a, **k),
              lambda q, s, o, *a, **k: collision.robot_resolve_grid_collisions(opt.robot, q, s, o, *a, **k)]

    def raises(match=None, q=good, s=sset, o=grid, **kw):
        kw.setdefault("margin", 0.01)
        kw.setdefault("damping", 1e-4)
        kw.setdefault("max_iters", 8)
        for f in fronts:
            with pytest.raises(ValueError, match=match):
                f(q, s, o, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises("CUDA")
    raises("CUDA", obstacle_margin=0.02, obstacle_pos=pos, obstacle_rot=rot, obstacle_weight=2.0)
    raises("CUDA", posture_weight=1e-4, q_ref=good, collision_weight=2.0, pair_weight=pw, tol=1e-6, max_step=0.2, limits=lim)
    raises("CUDA", posture_weight=u, link_names=names, target_pos=p, target_rot=r, pos_weight=w, rot_weight=w, obstacle_pos=pos)
    raises("CUDA", margin=0, obstacle_margin=0, obstacle_weight=0, damping=1, max_iters=1)  # Python ints are numbers too
    with pytest.raises(ValueError, match="CUDA"):  # the positional order of the signature: resolve_collisions' without prim_weight
        collision.resolve_grid_collisions(opt, good, sset, grid, 0.01, 0.02, pos, rot, 1.0, 1e-4, 8, 1e-4, good, 1.0, pw, names, p, r, w, w, 0.0, 0.2, lim,
                                          None)
    with pytest.raises(ValueError, match="CUDA"):
        collision.robot_resolve_grid_collisions(opt.robot, good, sset, grid, 0.01, 0.02, pos, rot, 1.0, 1e-4, 8, 1e-4, good, 1.0, pw, names, p, r, w, w, 0.0,
                                                0.2, lim)
    for f in fronts:
        with pytest.raises(TypeError):
            f(good, sset, grid, 0.01, damping=1e-4, max_iters=8, prim_weight=None)  # a grid has no primitives to weigh
    # the grid side
    raises("SdfGrid", o=(grid.values, grid.origin, grid.spacing))
    raises("SdfGrid", o=None)
    raises("SdfGrid", o=collision.ObstacleSet.spheres([[0.0, 0.0, 0.0]], [0.03]))
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.01), "0.01", True):
        raises("obstacle_margin", obstacle_margin=bad)
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(1.0), None, "1", True):
        raises("obstacle_weight", obstacle_weight=bad)
    raises("float32", obstacle_pos=pos.double())
    raises("float32", obstacle_rot=rot.double())
    raises("torch tensor", obstacle_pos=pos.numpy())
    raises("torch tensor", obstacle_rot=rot.numpy())
    for bad in (pos[:3], pos[:, :2], pos[0]):
        raises("obstacle_pos must have shape", obstacle_pos=bad)
    for bad in (rot[:3], rot.reshape(4, 9), pos):
        raises("obstacle_rot must have shape", obstacle_rot=bad)
    # the rules of resolve_self_collision hold as they are
    raises("float32", q=good.double())
    raises("torch tensor", q=good.numpy())
    for bad in (good[:, :15], good.reshape(-1)):
        raises("shape", q=bad)
    for name, t in (("q_ref", good), ("posture_weight", u), ("limits", lim), ("pair_weight", pw)):
        raises("float32", **{name: t.double()})
        raises("torch tensor" if name != "posture_weight" else "posture_weight", **{name: t.numpy()})
    for bad in (pw[:-1], pw[None]):
        raises("shape", pair_weight=bad)
    raises("shape", q_ref=good[:3])
    raises("shape", limits=lim.t())
    raises("shape", link_names=names, target_pos=p[:, :1])
    raises("SphereSet", s=tips)
    raises("is not a link name", s=collision.SphereSet(["link_15.0_tip", "no_such_link"], np.zeros((2, 3)), [0.01, 0.01]))
    raises("0 pairs", s=collision.SphereSet(["link_15.0_tip", "link_15.0"], np.zeros((2, 3)), [0.01, 0.01]))
    raises("is not a link name", link_names=["link_3.0_tip", "no_such_link"], target_pos=p)
    raises("need link_names", target_pos=p)
    raises("both None", link_names=names)
    for f in fronts:
        with pytest.raises(TypeError):
            f(good, sset, grid)  # margin is positional
        with pytest.raises(ValueError, match="damping is required"):
            f(good, sset, grid, 0.01, max_iters=8)
        with pytest.raises(ValueError, match="max_iters is required"):
            f(good, sset, grid, 0.01, damping=1e-4)
    for bad in (-1e-9, float("nan"), float("inf"), None, "0.01", True):
        raises("margin", margin=bad)
    for bad in (0, -1.0, float("nan"), None, True):
        raises("damping", damping=bad)
    for bad in (0, 257, 8.0, None, True):
        raises("max_iters", max_iters=bad)
    for bad in (-1e-9, float("nan"), None, True):
        raises("tol", tol=bad)
        raises("max_step", max_step=bad)
        raises("collision_weight", collision_weight=bad)
    # fixed_qpos: one too many, one missing, one of the wrong width
    with pytest.raises(ValueError, match="fixed_qpos"):
        collision.resolve_grid_collisions(opt, good, sset, grid, 0.01, damping=1e-4, max_iters=8, fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    for fq, word in ((None, "fixed_qpos"), (torch.zeros((4, 5), dtype=torch.float32), "fixed_qpos"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                     (torch.zeros((4, 6), dtype=torch.float32), "CUDA")):
        with pytest.raises(ValueError, match=word):
            collision.resolve_grid_collisions(sub, q10, sset, grid, 0.01, damping=1e-4, max_iters=8, fixed_qpos=fq)
    assert touched == []


# ---- 3. the yardstick: g is -1/2 the gradient of its E ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A", "P"])
@pytest.mark.parametrize("name", ["allegro_hand_right", "shadow_hand_right"])
def test_reference_g_is_minus_half_the_central_difference_of_its_energy(name, which):
    """Every term of E at once, as in the sibling (its step and gate), with an obstacle weight and an obstacle margin of its own, on the
    first four near frames whose spheres all keep FD_GAP from the faces (an inactive sphere that a step activates counts too)."""
    d = resolve_grid_inputs(name, which)
    rng = np.random.default_rng(41)
    omargin = 0.02
    away = grid_problem(d, obstacle_margin=omargin).fields(d["q"], False)["gap"].min(1) > FD_GAP
    sel = np.flatnonzero(~d["far"] & away)[:4]
    assert len(sel) == 4, "fewer than four near frames keep FD_GAP from every face"
    x = d["q"][sel].copy()
    n, nt, L = x.shape[1], 3, len(d["links"])
    links = d["links"][-nt:] + d["links"][:-nt]  # the last three links of the robot are the target rows, in front of the table
    p, R = rr.isr.link_poses(d["orc"], _r32(x + rng.uniform(-0.2, 0.2, x.shape)), links[:nt])
    d = dict(d, links=links, rows=(d["rows"] + nt) % L, q=x, pos=d["pos"][sel], rot=d["rot"][sel], omargin=omargin, wobs=0.75)
    P = grid_problem(d, n_target=nt, tgt_pos=p, tgt_rot=R, w_pos=rng.uniform(0.5, 2, (4, nt)), w_rot=rng.uniform(0.01, 0.1, (4, nt)),
                     x_ref=x + rng.uniform(-0.3, 0.3, x.shape), posture_weight=rng.uniform(0, 1e-2, n), pair_weight=rng.uniform(0.5, 2, len(d["pairs"])),
                     collision_weight=1.5)
    E4, hs, _ = P.energies(x)
    g, Hm = P.system(x, hs)
    assert (E4[:, :2] > 0).all() and (E4[:, 3] > 0).all() and (hs[0] > 0).any() and np.allclose(Hm, Hm.transpose(0, 2, 1), rtol=0, atol=1e-12)
    assert np.linalg.eigvalsh(Hm).min() > -1e-9
    worst = 0.0
    for c in range(n):
        xp, xm = x.copy(), x.copy()
        xp[:, c] += H
        xm[:, c] -= H
        cd = (P.energies(xp)[0].sum(1) - P.energies(xm)[0].sum(1)) / (2 * H)
        worst = max(worst, float(np.abs(g[:, c] + 0.5 * cd).max()))
    print(f"{name} GRID_{which}: max |g + 1/2 central difference of E| = {worst:.3e} (gate {GATE_E:.0e}), max |g| = {np.abs(g).max():.3e}, E_obs {E4[:, 3]}")
    assert worst <= GATE_E


# ---- 4. the yardstick on the inputs of the GPU tests ---------------------------------------------------------------------------------
CASES = [(n, "A") for n in sorted(ROBOTS)] + [("allegro_hand_right", "P"), ("shadow_hand_right", "P")]


@pytest.mark.parametrize("name,which", CASES)
def test_reference_descends_monotonically_and_enough_frames_are_clear(name, which):
    assert len(ROBOTS) == 8 and B == 33
    d, res = resolve_grid_inputs(name, which), reference(name, which=which)
    E = res["energy"].sum(-1)
    dec = res["decisions"]
    assert res["xs"].shape == (STEPS64 + 1, B, d["orc"].dof) and res["energy"].shape == (STEPS64 + 1, B, 4) and np.isfinite(res["xs"]).all()
    assert (np.diff(E, axis=0) <= 0).all(), "an accepted trial raised E"
    assert ((res["xs"] >= d["lo"]) & (res["xs"] <= d["hi"])).all()
    moved = np.abs(np.diff(res["xs"], axis=0)).max(-1) > 0
    assert not (moved & (dec != 1)).any()  # only an accepted trial moves the point
    clear32, clear64 = rgr.clear(res, STEPS32, *GUARD32), rgr.clear(res, STEPS64, *GUARD64)
    print(f"{name} GRID_{which} (pose seed {pose_seed(name)}): over {STEPS64} trials {int((dec == 1).sum())} accepted, {int((dec == 0).sum())} rejected; "
          f"median E {np.median(E[0]):.2e} -> {np.median(E[-1]):.2e}; frames with E_obs > 0 at x0: {int((res['energy'][0, :, 3] > 0).sum())}; clear frames: "
          f"{int(clear32.sum())} of {B} at the float32 guards over {STEPS32} trials, {int(clear64.sum())} at the float64 guards over {STEPS64}; "
          f"status counts {np.bincount(res['status'][-1], minlength=16)}")
    assert clear32.sum() >= NEED and clear64.sum() >= NEED, name
    assert (dec == 1).any() and (dec == 0).any(), "the runs must hold accepted and rejected trials"
    assert (res["energy"][0, :, 3] > 0).any() and not res["energy"][:, d["far"], 3].any()  # contact on some frames, none on the far ones
    assert not (res["status"] & (rgr.TRUNCATED | rgr.CONTACTS_TRUNCATED)).any()


# ---- 5. without the grid term the yardstick is resolve_reference -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["allegro_hand_right", GRIPPER])
def test_reference_with_obstacle_weight_zero_is_the_self_collision_reference(name):
    d = resolve_grid_inputs(name)
    a = reference_run(dict(d, wobs=0.0), STEPS32)
    b = rr.resolve(problem(d), d["q"], d["damping"], STEPS32, d["lo"], d["hi"], d["tol"], d["max_step"])
    assert np.array_equal(a["xs"], b["xs"]) and np.array_equal(a["iters"], b["iters"]) and np.array_equal(a["status"], b["status"])
    assert np.array_equal(a["energy"][..., :3], b["energy"]) and not a["energy"][..., 3].any() and np.array_equal(a["decisions"], b["decisions"])

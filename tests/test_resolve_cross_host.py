"""CPU tests of the posture solve against a second posed robot's interface (include/dexr_resolve_cross.h,
dex_retargeting_amd/collision.py): the export list and the constants against the header, the place and the contents of the
fragment, the argument rules of the three torch fronts (every one a ValueError before any device call), the yardstick
tests/resolve_cross_reference.py against central differences of its own float64 energy, and the conditions the GPU gates rest on,
asserted on the inputs of tests/test_gpu_resolve_cross.py before a GPU sees them.

INPUTS (cross_resolve_inputs; shared with the GPU tests).  Five pairs of robots (PAIRS, of tests/test_cross_host.py), B = 33.  Robot
A is resolve_inputs(name_a) of tests/test_resolve_host.py as it stands (the "origins" set with its self pairs, the limits, margin
0.010, posture weight 1e-4, damping 1e-4, max_step 0.2).  Robot B is side_inputs(name_b) of tests/test_cross_host.py (the "offset"
set, two spheres of radius 0.010 per link) at q_b = its q in reversed frame order, so that a robot against its own handle is not in
the same posture.  B is placed by the `place` recipe of tests/test_cross_host.py with A's base at the identity (place_other: the
same draws in the same order, A's pose left out): per frame a seeded rotation, and a seeded sphere of B lies LO .. HI = 5 .. 35 mm,
centre to centre, from a seeded sphere of A in a seeded direction (two radii and the margin are 30 mm).  The frames b % 8 == 5 are
moved (10, -10, 10) m away: the far frames.  cross_margin = margin, w_x = W_X = 1.5, cross_weight seeded in 0.5 .. 2.

CONDITIONS, asserted on the float64 reference alone, on every pair: at least half of the frames have an active cross contact at x0;
the run holds accepted and rejected trials; no active contact has centres nearer than 1 mm at any evaluated point; at least half
of the frames are clear at GUARD32 over STEPS32 trials and at least half at GUARD64 over STEPS64 (tests/test_resolve_host.py).

POSE_SEED = 5 is the first of the seeds 0, 1, 2, ... with which the conditions hold on all five pairs, with the placement range as
it stands.  Why the earlier ones fail (test_the_pose_seed_is_the_first_that_meets_the_conditions prints it): fewer than 17 frames
clear at the float32 guards over STEPS32 trials -- seeds 0, 1, 3 and 4 on gripper_arm (16, 14, 10 and 10 frames; the gripper's two
finger columns meet their bounds and its few pairs sit near the margin), seed 2 on allegro_right_left (16 frames).  With seed 5
the clear frames of 33 are (float32 guards / float64 guards, recorded from test_reference_descends_and_the_conditions_hold):
allegro_right_left 19 / 29, gripper_arm 17 / 25, leap_same 26 / 33, shadow_allegro 25 / 33, shadow_right_left 28 / 33.

CENTRAL DIFFERENCES: step H = 1e-6 and gate GATE_E = 1e-6 of tests/test_collision_host.py."""
import functools
import os
import re

import numpy as np
import pytest

import collision_reference as cref
import resolve_cross_reference as rxr
import resolve_reference as rr
from testutil import REPO
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, GATE_E, H
from test_cross_host import FAR, PAIRS as CROSS_PAIRS, side_inputs
from test_jacobian_host import SUBSET_CFG
from test_obstacle_host import _rotations
from test_resolve_host import GUARD32, GUARD64, STEPS32, STEPS64, _declared, _r32, resolve_inputs
from test_resolve_obstacle_host import OKEYS

HEADER = os.path.join(REPO, "include", "dexr_resolve_cross.h")
FRAGMENT = os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_resolve_cross.hpp")
PAIRS = {k: CROSS_PAIRS[k] for k in ("allegro_right_left", "shadow_right_left", "shadow_allegro", "gripper_arm", "leap_same")}
POSE_SEED, XW_SEED, W_X = 5, 46, 1.5
LO, HI = 0.005, 0.035
XKEYS = OKEYS + ("max_contact",)


def place_other(ca, cb, seed, n, lo=LO, hi=HI):
    """test_cross_host.place with A's base at the identity: the same draws in the same order (A's rotation and position are drawn
    and left out) -> pos_b, rot_b, float32-representable: the pose of B's root in A's root frame."""
    rng = np.random.default_rng(seed)
    _, rot_b = _rotations(rng, n), _r32(_rotations(rng, n))
    rng.uniform(-0.1, 0.1, (n, 3))
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ia, ib = rng.integers(0, ca.shape[1], n), rng.integers(0, cb.shape[1], n)
    pos_b = ca[np.arange(n), ia] + u * rng.uniform(lo, hi, (n, 1)) - np.einsum("bij,bj->bi", rot_b, cb[np.arange(n), ib])
    return _r32(pos_b), rot_b


@functools.lru_cache(maxsize=None)
def cross_resolve_inputs(case, seed=POSE_SEED, lo=LO, hi=HI):
    """dict: resolve_inputs(name_a) and b (side_inputs(name_b)), q_b, opos, orot, xmargin, wx, xw (S_a, S_b), far; read-only."""
    na, nb = PAIRS[case]
    d = dict(resolve_inputs(na))
    b = side_inputs(nb)
    q_b = np.ascontiguousarray(b["q"][::-1])
    ca = cref.centres(d["orc"], d["q"], d["links"], d["rows"], d["centers"])[0]
    cb = cref.centres(b["orc"], q_b, b["links"], b["rows"], b["centers"])[0]
    opos, orot = place_other(ca, cb, seed, B, lo, hi)
    opos = opos.copy()
    opos[FAR] += np.array([10.0, -10.0, 10.0])
    xw = _r32(np.random.default_rng(XW_SEED).uniform(0.5, 2.0, (len(d["radii"]), len(b["radii"]))))
    d.update(case=case, b=b, q_b=q_b, opos=_r32(opos), orot=orot, xmargin=d["margin"], wx=W_X, xw=xw, far=FAR.copy())
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def other_of(d):
    b = d["b"]
    return rxr.Other(b["orc"], d["q_b"], b["links"], b["rows"], b["centers"], b["radii"], d.get("opos"), d.get("orot"))


def cross_problem(d, dtype=np.float64, **over):
    """the yardstick's Problem of a dict of cross_resolve_inputs (keys a run does not have are absent: None)."""
    kw = dict(posture_weight=d.get("u"), collision_weight=d["wcol"], dtype=dtype, cross_margin=d["xmargin"], w_x=d["wx"], cross_weight=d.get("xw"))
    kw.update({k: d[k] for k in XKEYS if d.get(k) is not None})
    kw.update(over)
    return rxr.Problem(d["orc"], d["links"], kw.pop("n_target", 0), d["rows"], d["centers"], d["radii"], d["pairs"], d["margin"], other_of(d), **kw)


def reference_run(d, steps, dtype=np.float64, **over):
    """the yardstick's run, trial by trial; `closest` (0-d): the smallest centre distance of an active contact at any evaluated point."""
    P = cross_problem(d, dtype, **over)
    res = rxr.resolve(P, d["q"], d["damping"], steps, d.get("lo"), d.get("hi"), d["tol"], d["max_step"])
    res["closest"] = np.array(P.closest)
    return res


@functools.lru_cache(maxsize=None)
def reference(case, dtype=np.float64, steps=STEPS64, seed=POSE_SEED):
    """the yardstick's run on cross_resolve_inputs(case), computed once and shared, read-only."""
    res = reference_run(cross_resolve_inputs(case, seed), steps, dtype)
    for v in res.values():
        v.setflags(write=False)
    return res


def conditions(res):
    """-> None where the conditions the GPU gates rest on hold on a float64 run over STEPS64 trials, else what fails."""
    active0 = res["energy"][0, :, 3] > 0
    if 2 * active0.sum() < B:
        return f"only {int(active0.sum())} of {B} frames have an active cross contact at x0"
    dec = res["decisions"]
    if not ((dec == 1).any() and (dec == 0).any()):
        return "the run does not hold both accepted and rejected trials"
    if float(res["closest"]) < 1e-3:
        return f"an active contact has centres {float(res['closest']) * 1e3:.2f} mm apart"
    c32, c64 = rxr.clear(res, STEPS32, *GUARD32), rxr.clear(res, STEPS64, *GUARD64)
    if 2 * c32.sum() < B or 2 * c64.sum() < B:
        return f"clear frames {int(c32.sum())} (float32 guards, {STEPS32} trials), {int(c64.sum())} (float64 guards, {STEPS64} trials) of {B}"
    return None


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_the_header_and_the_fragment_is_in_its_place():
    declared = _declared(HEADER)
    exports = _lib.RESOLVE_CROSS_SYMBOLS
    assert declared == set(exports) == {"dexr_sphere_resolve_cross_dev", "dexr_sphere_resolve_cross"} and len(exports) == 2
    for n in dir(_lib):
        if n.endswith("EXPORTS"):
            assert not set(exports) & set(getattr(_lib, n)), n
    lib = _lib.load()
    for name in exports:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h != "dexr_resolve_cross.h":
            assert not _declared(os.path.join(REPO, "include", h)) & declared, h
    text = open(HEADER).read()
    assert '#include "dexr_cross.h"' in text and '#include "dexr_resolve_obstacles.h"' in text
    assert not re.search(r"#define\s+DEXR_RESOLVE_(MAXCONTACT|CONTACTS_TRUNCATED)", text)  # reused, not redefined
    assert (rxr.MAXACTIVE, rxr.MAXCONTACT, rxr.LAM_UP, rxr.LAM_DOWN, rxr.MAXREJECT) == (_lib.RESOLVE_MAXACTIVE, _lib.RESOLVE_MAXCONTACT, _lib.RESOLVE_LAM_UP,
                                                                                       _lib.RESOLVE_LAM_DOWN, _lib.RESOLVE_MAXREJECT)
    assert (rxr.CONVERGED, rxr.STALLED, rxr.TRUNCATED, rxr.CONTACTS_TRUNCATED) == (_lib.RESOLVE_CONVERGED, _lib.RESOLVE_STALLED, _lib.RESOLVE_TRUNCATED,
                                                                                 _lib.RESOLVE_CONTACTS_TRUNCATED)
    for n in ("resolve_cross_collisions", "robot_resolve_cross_collisions", "resolve_bimanual_collisions", "relative_pose"):
        assert n in collision.__all__
    assert hasattr(_lib.SphereModel, "resolve_cross_dev") and hasattr(_lib.SphereModel, "resolve_cross")
    src = open(FRAGMENT).read()
    assert "getenv" not in src and "atomic" not in src.replace("no atomics", "") and "asm" not in src.replace("__restrict__", "")
    for n in ("DEXR_RESOLVE_LAM_UP", "DEXR_RESOLVE_LAM_DOWN", "DEXR_RESOLVE_MAXREJECT", "DEXR_RESOLVE_MAXACTIVE", "DEXR_RESOLVE_MAXCONTACT",
              "DEXR_RESOLVE_CONTACTS_TRUNCATED"):
        assert n in src  # the kernel reads the named constants, not numbers of its own
    assert src.count('#include "') == 1 and '#include "dexr_resolve_cross.h"' in src  # (a fragment: no unit of its own)
    assert "cross_gap(" in src and "cross_inv(" in src and "cross_walk<T, false>" in src  # the pair arithmetic is dexr_cross.hpp's
    assert "resolve_scene_loop<" not in src and "resolve_contact_loop<" not in src  # the loop has a home of its own
    for phase in ("resolve_start", "resolve_walk", "resolve_pair_forces", "resolve_count_pairs", "resolve_decide<true>", "resolve_pair_total",
                  "resolve_all_stopped", "resolve_list_pairs", "resolve_gradient<true>", "resolve_frozen", "resolve_base_h", "resolve_pair_contact",
                  "resolve_stage_row", "resolve_rank16", "resolve_damp", "ik_factor_solve", "resolve_step", "resolve_output"):
        assert phase in src, phase  # the loop is made of the shared phases
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_resolve_cross.hpp"') == 1 and pose.count("dexr_resolve_cross.hpp") == 1
    assert pose.index('"dexr_cross.hpp"') < pose.index('"dexr_resolve_cross.hpp"') < pose.index('"dexr_mesh_sdf.hpp"')


def header_bytes(v, n_jx, n_link_targets, S_a, n_act, n_in, n_pair, S_b, slots_a, slots_b):
    """the LDS formula of the header, restated."""
    n_tri = n_act * (n_act + 1) // 2
    values = (6 * n_jx + 11 * n_link_targets + 6 * S_a + 16 + max(n_tri, 16 * n_act + 16) + n_tri + 4 * n_act + 2 * n_in + 8 + 3 * S_b + 12 + 16) | 1
    return (128 + 16 * S_a + v * (12 * (slots_a + slots_b) + values) + 4 * (_lib.RESOLVE_MAXACTIVE + 22) + 4 * 17 + 2 * _lib.RESOLVE_MAXCONTACT
            + ((n_pair + 3) & ~3))


def test_the_header_states_the_formula_the_test_restates():
    text = " ".join(open(HEADER).read().replace(" * ", " ").split())
    assert "values = (6 n_jx + L + 6 S_a + 16 + max(n_tri, 16 n_act + 16) + n_tri + 4 n_act + 2 n_in + 8 + 3 S_b + 12 + 16) | 1" in text
    assert "bytes = 128 + 16 S_a + v (12 (n_slot_a + n_slot_b) + values) + 4 (DEXR_RESOLVE_MAXACTIVE + 22) + 4 17 + 2 DEXR_RESOLVE_MAXCONTACT" in text
    # two Shadow-sized hands, 24 columns each, 48 spheres against 48, 900 self pairs, no targets: 9 668 B in float32, four frames a block
    b32 = header_bytes(4, 24, 0, 48, 24, 24, 900, 48, 3, 3)
    assert b32 * 16 > 64 * 1024 >= b32 * 4


def test_a_null_model_is_invalid_before_a_device_is_looked_for():
    lib = _lib.load()
    z4, z3 = (None,) * 4, (None,) * 3
    dev = lambda a, b, B=4: lib.dexr_sphere_resolve_cross_dev(a, B, *z4, 0, *z4, 0.01, 1.0, *z3, 1e-4, 0.0, 0.0, 8, b, *z4, 0.01, 1.0, None,  # noqa: E731
                                                             *z4, None)
    host = lambda a, b, B=4: lib.dexr_sphere_resolve_cross(a, B, *z4, 0, *z4, 0.01, 1.0, *z3, 1e-4, 0.0, 0.0, 8, b, *z4, 0.01, 1.0, None, *z4)  # noqa: E731
    for f in (dev, host):
        for B_ in (4, 0):
            assert f(None, None, B_) == -1 and b"null sphere model" in lib.dexr_last_error()
    # (every other DEXR_ERR_INVALID case needs a model, which needs a device: tests/test_gpu_resolve_cross.py)


# ---- 2. the argument rules of the torch fronts ----------------------------------------------------------------------------------------
def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    touched = []
    for cls in (_lib.SphereModel, _lib.PoseModel):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("resolve_cross_dev", "resolve_dev", "cross_penalty_dev", "penalty_dev"):
        monkeypatch.setattr(_lib.SphereModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "base_link"]
    sa = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    sb = collision.SphereSet(tips[:3], np.zeros((3, 3)), np.full(3, 0.01))
    n_pair = len(collision.default_pairs(opt.robot, sa))
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    xw = torch.ones((4, 3), dtype=torch.float32)
    pw = torch.ones((n_pair,), dtype=torch.float32)
    lim = torch.tensor([[-1.0, 1.0]] * 16, dtype=torch.float32)
    pos, rot = torch.zeros((4, 3), dtype=torch.float32), torch.eye(3, dtype=torch.float32).repeat(4, 1, 1)
    fronts = [lambda qa, s, qb, t, *a, **k: collision.resolve_cross_collisions(opt, qa, s, opt, qb, t, *a, **k),
              lambda qa, s, qb, t, *a, **k: collision.robot_resolve_cross_collisions(opt.robot, qa, s, opt.robot, qb, t, *a, **k)]

    def raises(match=None, qa=good, s=sa, qb=good, t=sb, **kw):
        kw.setdefault("margin", 0.01)
        kw.setdefault("damping", 1e-4)
        kw.setdefault("max_iters", 8)
        for f in fronts:
            with pytest.raises(ValueError, match=match):
                f(qa, s, qb, t, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises("CUDA")
    raises("CUDA", cross_margin=0.02, other_pos=pos, other_rot=rot, cross_weight=xw, pair_weight=pw, w_x=2.0)
    raises("CUDA", cross_margin=0, w_x=0, posture_weight=1e-4, q_ref=good, collision_weight=2.0, tol=1e-6, max_step=0.2, limits=lim)
    with pytest.raises(ValueError, match="CUDA"):  # the positional order of the signature
        collision.resolve_cross_collisions(opt, good, sa, opt, good, sb, 0.01, 0.02, pos, rot, xw, pw, 1.0, 1e-4, 8)
    # the other robot's arguments
    raises("spheres_b must be a collision.SphereSet", t=tips)
    raises("is not a link name", t=collision.SphereSet(["link_15.0_tip", "no_such_link"], np.zeros((2, 3)), [0.01, 0.01]))
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.01), "0.01", True):
        raises("cross_margin", cross_margin=bad)
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(1.0), None, "1", True):
        raises("w_x", w_x=bad)
    raises("float32", cross_weight=xw.double())
    raises("torch tensor", cross_weight=xw.numpy())
    for bad in (xw.T.contiguous(), xw[:3], xw[None], xw.reshape(-1), torch.ones((4, 4))):
        raises("cross_weight must have shape", cross_weight=bad)
    raises("float32", other_pos=pos.double())
    raises("float32", other_rot=rot.double())
    raises("torch tensor", other_pos=pos.numpy())
    raises("torch tensor", other_rot=rot.numpy())
    for bad in (pos[:3], pos[:, :2], pos[0]):
        raises("other_pos must have shape", other_pos=bad)
    for bad in (rot[:3], rot.reshape(4, 9), pos):
        raises("other_rot must have shape", other_rot=bad)
    raises("float32", qb=good.double())
    raises("torch tensor", qb=good.numpy())
    for bad in (good[:, :15], good.reshape(-1)):
        raises("shape", qb=bad)
    raises("one row per frame", qb=good[:3])
    # the rules of resolve_self_collision hold as they are, for A
    raises("float32", qa=good.double())
    raises("torch tensor", qa=good.numpy())
    for bad in (good[:, :15], good.reshape(-1)):
        raises("shape", qa=bad)
    raises("SphereSet", s=tips)
    raises("float32", pair_weight=pw.double())
    raises("shape", pair_weight=pw[:-1])
    raises("shape", limits=lim.t())
    raises("need link_names", target_pos=torch.zeros((4, 2, 3)))
    for f in fronts:
        with pytest.raises(TypeError):
            f(good, sa, good, sb)  # margin is positional
        with pytest.raises(ValueError, match="damping is required"):
            f(good, sa, good, sb, 0.01, max_iters=8)
        with pytest.raises(ValueError, match="max_iters is required"):
            f(good, sa, good, sb, 0.01, damping=1e-4)
    for bad in (-1e-9, float("nan"), float("inf"), None, "0.01", True):
        raises("margin", margin=bad)
    for bad in (0, -1.0, float("nan"), None, True):
        raises("damping", damping=bad)
    for bad in (0, 257, 8.0, None, True):
        raises("max_iters", max_iters=bad)
    # fixed_qpos on either side: one too many, one missing, one of the wrong width
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    kw = dict(damping=1e-4, max_iters=8)
    with pytest.raises(ValueError, match="fixed_qpos"):
        collision.resolve_cross_collisions(opt, good, sa, opt, good, sb, 0.01, fixed_qpos_b=torch.zeros((4, 1), dtype=torch.float32), **kw)
    for fq, word in ((None, "fixed_qpos"), (torch.zeros((4, 5), dtype=torch.float32), "fixed_qpos"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                     (torch.zeros((4, 6), dtype=torch.float32), "CUDA")):
        with pytest.raises(ValueError, match=word):
            collision.resolve_cross_collisions(sub, q10, sa, opt, good, sb, 0.01, fixed_qpos_a=fq, **kw)
        with pytest.raises(ValueError, match=word):
            collision.resolve_cross_collisions(opt, good, sa, sub, q10, sb, 0.01, fixed_qpos_b=fq, **kw)
    # the alternating front: its own rules, then those of the fronts it calls
    bi = lambda **k: collision.resolve_bimanual_collisions(opt, good, sa, opt, good, sb, 0.01, **{**dict(pos_a=pos, rot_a=rot, pos_b=pos, rot_b=rot,  # noqa: E731
                                                                                                       damping=1e-4, max_iters=8), **k})
    for k_, bad, word in (("sweeps", 0, "sweeps"), ("sweeps", 1.0, "sweeps"), ("sweeps", True, "sweeps"), ("pos_a", pos.numpy(), "torch tensor"),
                          ("rot_b", rot.double(), "float32"), ("pos_b", pos[:3], "pos_b must have shape"), ("rot_a", rot.reshape(4, 9), "rot_a must have shape"),
                          ("args_a", dict(damping=1.0), "args_a holds"), ("args_b", dict(fixed_qpos=None), "args_b holds"),
                          ("cross_weight", xw.reshape(-1), "cross_weight must have shape"), ("cross_weight", xw.T.contiguous(), "cross_weight must have shape"),
                          ("w_x", -1.0, "w_x"), ("cross_margin", -1.0, "cross_margin")):
        with pytest.raises(ValueError, match=word):
            bi(**{k_: bad})
    with pytest.raises(ValueError, match="CUDA"):
        bi(sweeps=2, cross_weight=xw, cross_margin=0.02, w_x=2.0, args_a=dict(pair_weight=pw, limits=lim), args_b=dict(posture_weight=1e-4))
    assert touched == []
    # the host-pointer method keeps the shape rules (no device: the handle is never read)
    m = _lib.SphereModel.__new__(_lib.SphereModel)
    m.n_in, m.n_fixed, m.n_sphere, m.n_pair = 16, 0, 4, 3
    z = np.zeros((4, 16))
    for call in (lambda: m.resolve_cross(m, z, z[:3], 0.01, 1e-4, 8), lambda: m.resolve_cross(m, z, z, 0.01, 1e-4, 8, other_pos=np.zeros((4, 2))),
                 lambda: m.resolve_cross(m, z, z, 0.01, 1e-4, 8, other_rot=np.zeros((4, 9))),
                 lambda: m.resolve_cross(m, z, z, 0.01, 1e-4, 8, cross_pair_weight=np.ones((4, 3))), lambda: m.resolve_cross(m, z, z[:, :15], 0.01, 1e-4, 8),
                 lambda: m.resolve_cross(m, z, z, 0.01, None, 8), lambda: m.resolve_cross(m, z, z)):
        with pytest.raises(ValueError):
            call()


# ---- 3. the yardstick: g is -1/2 the gradient of its E ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["allegro_right_left", "shadow_right_left"])
def test_reference_g_is_minus_half_the_central_difference_of_its_energy(case):
    """Every term of E at once (targets, posture, weighted self pairs, the weighted cross term with a pose), on the first four frames
    with an active cross contact."""
    d = cross_resolve_inputs(case)
    rng = np.random.default_rng(41)
    sel = np.flatnonzero(reference(case)["energy"][0, :, 3] > 0)[:4]
    assert len(sel) == 4
    x = d["q"][sel].copy()
    n, nt, L = x.shape[1], 3, len(d["links"])
    links = d["links"][-nt:] + d["links"][:-nt]  # the last three links of the robot are the target rows, in front of the table
    p, R = rr.isr.link_poses(d["orc"], _r32(x + rng.uniform(-0.2, 0.2, x.shape)), links[:nt])
    d = dict(d, links=links, rows=(d["rows"] + nt) % L, q=x, q_b=d["q_b"][sel], opos=d["opos"][sel], orot=d["orot"][sel])
    P = cross_problem(d, n_target=nt, tgt_pos=p, tgt_rot=R, w_pos=rng.uniform(0.5, 2, (4, nt)), w_rot=rng.uniform(0.01, 0.1, (4, nt)),
                      x_ref=x + rng.uniform(-0.3, 0.3, x.shape), posture_weight=rng.uniform(0, 1e-2, n), pair_weight=rng.uniform(0.5, 2, len(d["pairs"])),
                      collision_weight=1.5)
    E, hs, _ = P.energies(x)
    g, Hm = P.system(x, hs)
    assert E.shape == (4, 4) and (E[:, :2] > 0).all() and (E[:, 3] > 0).all() and (hs[1] > 0).any((1, 2)).all()
    assert np.allclose(Hm, Hm.transpose(0, 2, 1), rtol=0, atol=1e-12) and np.linalg.eigvalsh(Hm).min() > -1e-9
    worst = 0.0
    for c in range(n):
        xp, xm = x.copy(), x.copy()
        xp[:, c] += H
        xm[:, c] -= H
        cd = (P.energies(xp)[0].sum(1) - P.energies(xm)[0].sum(1)) / (2 * H)
        worst = max(worst, float(np.abs(g[:, c] + 0.5 * cd).max()))
    print(f"{case}: max |g + 1/2 central difference of E| = {worst:.3e} (gate {GATE_E:.0e}), max |g| = {np.abs(g).max():.3e}, E_x {E[:, 3]}")
    assert worst <= GATE_E


# ---- 4. the yardstick on the inputs of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PAIRS))
def test_reference_descends_and_the_conditions_hold(case):
    assert len(PAIRS) == 5 and B == 33
    d, res = cross_resolve_inputs(case), reference(case)
    for k in ("q", "q_b", "opos", "orot", "xw"):
        assert np.array_equal(d[k], _r32(d[k])), k
    E = res["energy"].sum(-1)
    dec = res["decisions"]
    assert res["xs"].shape == (STEPS64 + 1, B, d["orc"].dof) and res["energy"].shape == (STEPS64 + 1, B, 4) and np.isfinite(res["xs"]).all()
    assert (np.diff(E, axis=0) <= 0).all(), "an accepted trial raised E"
    assert ((res["xs"] >= d["lo"]) & (res["xs"] <= d["hi"])).all()
    moved = np.abs(np.diff(res["xs"], axis=0)).max(-1) > 0
    assert not (moved & (dec != 1)).any()  # only an accepted trial moves the point
    c32, c64 = rxr.clear(res, STEPS32, *GUARD32), rxr.clear(res, STEPS64, *GUARD64)
    print(f"{case}: {len(d['radii'])} spheres against {len(d['b']['radii'])}; over {STEPS64} trials {int((dec == 1).sum())} accepted, "
          f"{int((dec == 0).sum())} rejected; median E {np.median(E[0]):.2e} -> {np.median(E[-1]):.2e}; frames with an active cross contact at x0: "
          f"{int((res['energy'][0, :, 3] > 0).sum())}; closest active centres {float(res['closest']) * 1e3:.2f} mm; clear frames: {int(c32.sum())} of {B} at the "
          f"float32 guards over {STEPS32} trials, {int(c64.sum())} at the float64 guards over {STEPS64}; status counts "
          f"{np.bincount(res['status'][-1], minlength=16)}")
    assert conditions(res) is None
    assert d["far"].mean() >= 0.1 and not res["energy"][:, d["far"], 3].any()  # the far frames are kept, and B is out of reach there
    assert (res["energy"][-1, :, 3] < res["energy"][0, :, 3]).any()  # the solve pushes A out of B
    assert not (res["status"] & (rxr.TRUNCATED | rxr.CONTACTS_TRUNCATED)).any()


def test_the_pose_seed_is_the_first_that_meets_the_conditions():
    for seed in range(POSE_SEED + 1):
        failed = None
        for case in sorted(PAIRS):
            failed = conditions(reference(case, seed=seed))
            if failed:
                print(f"seed {seed}: {case}: {failed}")
                break
        assert (failed is None) == (seed == POSE_SEED), (seed, failed)


def test_reference_with_w_x_zero_is_the_self_collision_reference():
    """x, iters, status, decisions and the first three energies of the two yardsticks are equal where the cross term has no weight."""
    d = cross_resolve_inputs("allegro_right_left")
    a = reference_run(d, STEPS32, w_x=0.0)
    P = rr.Problem(d["orc"], d["links"], 0, d["rows"], d["centers"], d["radii"], d["pairs"], d["margin"], posture_weight=d["u"],
                   collision_weight=d["wcol"])
    b = rr.resolve(P, d["q"], d["damping"], STEPS32, d["lo"], d["hi"], d["tol"], d["max_step"])
    for key in ("xs", "iters", "decisions", "lam", "frozen"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["energy"][..., :3], b["energy"]) and not a["energy"][..., 3].any()

"""CPU tests of the collision between two posed robots (include/dexr_cross.h, dex_retargeting_amd/collision.py): the export list
against the header, the limits, the NULL-model errors of the raw ABI (no device is looked for), the argument rules of the torch
front (every one a ValueError before any device call), the yardstick tests/cross_reference.py against central differences of its
own float64 energy and distances, and the conditions the GPU gates rest on, asserted on the inputs of tests/test_gpu_cross.py
before a GPU sees them.

INPUTS (cross_inputs; shared with the GPU tests).  Six pairs of robots (PAIRS), each side with the "offset" sphere set of
test_collision_host.collision_inputs (two spheres of radius 0.010 per link, the same recipe restated for the left hands, which are
not among that module's robots), B = 33, margin = 0.010.  q_a is the side's q, q_b the other side's in reversed frame order (so that
a robot against its own handle is not in the same posture).  Per frame robot A has a seeded rotation and a base within 10 cm of the
origin; robot B has a seeded rotation and is placed so that a seeded sphere of it lies 5 .. 35 mm, centre to centre, from a seeded
sphere of A in a seeded direction (two radii and the margin are 30 mm); the frames b % 8 == 5 are moved (10, -10, 10) m away: the far
frames.

CONDITIONS asserted on the float64 reference alone, per pair: at least half of the frames have an active pair (d < margin); at
least a tenth are far, with E, both gradients and both wrenches exact zeros; no active pair has centres nearer than 1 mm (the
normal's singular point); at least 90 % of the (frame, sphere) entries of either side are clear: the two smallest d of the sphere
differ by more than NEAR_GAP = 1e-5 m, a hundred times the float32 error of a distance, so that float32 rounding cannot change
which sphere is the nearest.  `nearest` is compared on clear entries and the cotangents of every VJP are zero elsewhere.

POSE_SEED = 1 is the first of the seeds 0, 1, 2, ... with which the conditions hold on all six pairs (with 0 an active pair of
shadow_right_left has centres 0.81 mm apart).

CENTRAL DIFFERENCES (float64, H = 1e-6 rad or m; the step and the gates of test_collision_host.py, for the reasons written there:
1e-8 for distances, 1e-6 for the energy).  The distances are checked through L = sum ga dist_a + sum gb dist_b with seeded
cotangents that are zero on entries that are not clear and scaled to sum |g| = 1, so that the error of dL is at most the largest
error of a single distance's derivative: the same gate holds for L.  Differentiated in q_a, q_b, the translation of each base
(against the force half of that base's wrench) and a small world rotation of each base about its origin, rot <- exp([theta e_k]x) rot
(against the torque half), which pins the definition of the wrench and its signs."""
import functools
import os
import re

import numpy as np
import pytest

import collision_reference as cref
import cross_reference as xref
from testutil import REPO
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from oracle.kin import OracleRobot
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from test_collision_host import ARM, B, GRIPPER, MARGIN, OFFSET_SEED, Q_SEED, RADIUS, ROBOTS, collision_inputs, robot_of
from test_jacobian_host import SUBSET_CFG
from test_obstacle_host import NEAR_GAP, _rotations

HEADER = os.path.join(REPO, "include", "dexr_cross.h")
POSE_SEED, W_SEED, GD_SEED = 1, 44, 45
INVALID = -1
PAIRS = {"allegro_right_left": ("allegro_hand_right", "allegro_hand_left"), "shadow_right_left": ("shadow_hand_right", "shadow_hand_left"),
         "shadow_allegro": ("shadow_hand_right", "allegro_hand_right"), "inspire_ability": ("inspire_hand_right", "ability_hand_right"),
         "gripper_arm": (GRIPPER, ARM), "leap_same": ("leap_hand_right", "leap_hand_right")}
FAR = np.arange(B) % 8 == 5
FLOATS = ("dist_a", "dist_b", "vjp_a", "vjp_b", "vjp_wa", "vjp_wb", "E", "grad_a", "grad_b", "wrench_a", "wrench_b")


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def left_robot(name):
    path = ROBOTS[name.replace("_left", "_right")].replace("_right.urdf", "_left.urdf")
    assert os.path.exists(path), path
    return RobotWrapper(path), OracleRobot(path)


@functools.lru_cache(maxsize=None)
def side_inputs(name):
    """collision_inputs(name, "offset") for the robots of test_collision_host; the same recipe for a left hand (q from Q_SEED + 1)."""
    if name in ROBOTS:
        return collision_inputs(name, "offset")
    robot, orc = left_robot(name)
    links = [f.name for f in robot.kin.frames]
    L = len(links)
    rng = np.random.default_rng(OFFSET_SEED)
    u = rng.standard_normal((L, 3))
    off = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.005, 0.015, (L, 1))
    names = [n for n in links for _ in range(2)]
    centers = _r32(np.stack([np.zeros((L, 3)), off], 1).reshape(2 * L, 3))
    radii = np.full(len(names), RADIUS)
    rows = np.array([links.index(n) for n in names])
    lim = orc.joint_limits
    q = np.clip(_r32(np.random.default_rng(Q_SEED + 1).uniform(lim[:, 0], lim[:, 1], (B, orc.dof))), _r32(lim[:, 0]), _r32(lim[:, 1]))
    sset = collision.SphereSet(names, centers, radii, [(0, 1)])  # (the pair list plays no part)
    d = dict(orc=orc, links=links, sset=sset, rows=rows, centers=centers, radii=radii, q=q, margin=MARGIN)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def wrapper_of(name):
    return robot_of(name)[0] if name in ROBOTS else left_robot(name)[0]


def place(ca, cb, seed, n, lo=0.005, hi=0.035):
    """seeded base poses for root-frame centres ca (n, S_a, 3), cb (n, S_b, 3): -> pos_a, rot_a, pos_b, rot_b, float32-representable;
    per frame a seeded sphere of B lies lo .. hi metres (centre to centre) from a seeded sphere of A, in a seeded direction."""
    rng = np.random.default_rng(seed)
    rot_a, rot_b = _r32(_rotations(rng, n)), _r32(_rotations(rng, n))
    pos_a = _r32(rng.uniform(-0.1, 0.1, (n, 3)))
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    ia, ib = rng.integers(0, ca.shape[1], n), rng.integers(0, cb.shape[1], n)
    at_a = pos_a + np.einsum("bij,bj->bi", rot_a, ca[np.arange(n), ia])
    pos_b = at_a + u * rng.uniform(lo, hi, (n, 1)) - np.einsum("bij,bj->bi", rot_b, cb[np.arange(n), ib])
    return pos_a, rot_a, _r32(pos_b), rot_b


@functools.lru_cache(maxsize=None)
def cross_inputs(case, seed=POSE_SEED):
    """dict: a, b (side_inputs), q_a, q_b, pos_a, rot_a, pos_b, rot_b, w (S_a, S_b), ga (B, S_a), gb (B, S_b), margin; read-only."""
    na, nb = PAIRS[case]
    a, b = side_inputs(na), side_inputs(nb)
    q_a, q_b = a["q"], np.ascontiguousarray(b["q"][::-1])
    ca = cref.centres(a["orc"], q_a, a["links"], a["rows"], a["centers"])[0]
    cb = cref.centres(b["orc"], q_b, b["links"], b["rows"], b["centers"])[0]
    pos_a, rot_a, pos_b, rot_b = place(ca, cb, seed, B)
    pos_b = pos_b.copy()
    pos_b[FAR] += np.array([10.0, -10.0, 10.0])
    Sa, Sb = len(a["radii"]), len(b["radii"])
    d = dict(a=a, b=b, q_a=q_a, q_b=q_b, pos_a=pos_a, rot_a=rot_a, pos_b=_r32(pos_b), rot_b=rot_b, margin=MARGIN,
             w=_r32(np.random.default_rng(W_SEED).uniform(0.5, 2.0, (Sa, Sb))),
             ga=_r32(np.random.default_rng(GD_SEED).standard_normal((B, Sa))), gb=_r32(np.random.default_rng(GD_SEED + 1).standard_normal((B, Sb))))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def sides(d, dtype=np.float64, jacobian=True, fold_a=None, fold_b=None, **over):
    """the two reference sides of an inputs dict (keys of `over` replace q_a, q_b, pos_*, rot_*)."""
    g = lambda k: over.get(k, d[k])  # noqa: E731
    a, b = d["a"], d["b"]
    A = xref.side(a["orc"], g("q_a"), a["links"], a["rows"], a["centers"], a["radii"], g("pos_a"), g("rot_a"), dtype, fold_a, jacobian)
    Bs = xref.side(b["orc"], g("q_b"), b["links"], b["rows"], b["centers"], b["radii"], g("pos_b"), g("rot_b"), dtype, fold_b, jacobian)
    return A, Bs


def clear_entries(d64):
    """(clear_a (B, S_a), clear_b (B, S_b)) from the float64 d (B, S_a, S_b): the two smallest d of a sphere differ by more than
    NEAR_GAP (every entry where the other side has one sphere)."""
    out = []
    for axis in (2, 1):
        if d64.shape[axis] == 1:
            out.append(np.ones(np.delete(d64.shape, axis), bool))
        else:
            two = np.sort(d64, axis).take([0, 1], axis)
            out.append(two.take(1, axis) - two.take(0, axis) > NEAR_GAP)
    return out


def outputs(A, Bs, margin, w, ga, gb):
    """every output of the three forms from two reference sides, and d, s, h."""
    F = xref.fields(A, Bs)
    da, na, db, nb = xref.distances(F)
    va, vb, vwa, vwb = xref.distances_vjp(F, A, Bs, ga, gb)
    E, gxa, gxb, wa, wb, h = xref.penalty(F, A, Bs, margin, w)
    return dict(dist_a=da, nearest_a=na, dist_b=db, nearest_b=nb, vjp_a=va, vjp_b=vb, vjp_wa=vwa, vjp_wb=vwb, E=E, grad_a=gxa, grad_b=gxb,
                wrench_a=wa, wrench_b=wb, d=F["d"], s=F["s"], h=h)


def make_case(d, fold_a=None, fold_b=None):
    """the float64 and float32 references of an inputs dict with the cotangents masked to the clear entries: dict r64, r32, ga, gb,
    clear_a, clear_b; the condition on the centres asserted."""
    A, Bs = sides(d, np.float64, True, fold_a, fold_b)
    clear_a, clear_b = clear_entries(xref.fields(A, Bs)["d"])
    ga, gb = np.where(clear_a, d["ga"], 0.0), np.where(clear_b, d["gb"], 0.0)
    r64 = outputs(A, Bs, d["margin"], d["w"], ga, gb)
    r32 = outputs(*sides(d, np.float32, True, fold_a, fold_b), d["margin"], d["w"], ga, gb)
    active = r64["h"] > 0
    assert not active.any() or r64["s"][active].min() >= 1e-3, ("an active pair with centres nearer than 1 mm", float(r64["s"][active].min()))
    out = dict(r64=r64, r32=r32, ga=ga, gb=gb, clear_a=clear_a, clear_b=clear_b)
    for r in (r64, r32):
        for v in r.values():
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    return make_case(cross_inputs(case))


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    assert declared == set(_lib.CROSS_EXPORTS) and len(_lib.CROSS_EXPORTS) == 6 and len(set(_lib.CROSS_EXPORTS)) == 6
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("EXPORTS") and n != "CROSS_EXPORTS"]
    assert len(others) == 14
    for other in others:
        assert not set(_lib.CROSS_EXPORTS) & set(other)
    lib = _lib.load()
    for name in _lib.CROSS_EXPORTS:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in os.listdir(os.path.join(REPO, "include")):
        if h != "dexr_cross.h":
            assert not _declared(os.path.join(REPO, "include", h)) & declared, h
    text = open(HEADER).read()
    assert int(re.search(r"#define DEXR_CROSS_FRAMES (\d+)", text).group(1)) == _lib.CROSS_FRAMES == 16
    assert int(re.search(r"#define DEXR_CROSS_LDS (\d+)", text).group(1)) == _lib.CROSS_LDS == 64 * 1024
    from dex_retargeting_amd import autograd as ag

    for n in ("cross_distances", "cross_penalty", "robot_cross_distances", "robot_cross_penalty"):
        assert n in collision.__all__ and n in ag.__all__
    src = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_cross.hpp")).read()
    assert "getenv" not in src and "atomic" not in src and "asm" not in src.replace("__restrict__", "")
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_cross.hpp"') == 1 and pose.index('"dexr_resolve_scene.hpp"') < pose.index('"dexr_cross.hpp"') < pose.index('"dexr_mesh_sdf.hpp"')


def test_the_header_states_the_working_set_of_the_largest_pair():
    """the LDS formula of the header, restated: 128 spheres against 128, 64 joints and 8 fork slots each."""
    slots, S, jx = 8, _lib.SPHERE_MAX, 64
    dist = (12 * 2 * slots + 3 * 2 * S + 24) | 1
    pen = (12 * 2 * slots + 9 * 2 * S + 24 + 16 + 192 + 6 * 2 * jx) | 1
    vjp = (12 * 2 * slots + 9 * 2 * S + 24 + 16 + 192 + 6 * 2 * jx + 2 * S) | 1
    assert (pen, vjp) == (3497, 3753)
    text = " ".join(open(HEADER).read().replace(" * ", " ").split())
    for word in ("3 497 values", "27 976 B", "13 988 B", "3 753", "30 024 B"):
        assert word in text, word

    def frames(values, size):
        nl = _lib.CROSS_FRAMES
        while nl > 1 and values * size * nl > _lib.CROSS_LDS:
            nl //= 2
        assert values * size * nl <= _lib.CROSS_LDS
        return nl

    assert (frames(pen, 8), frames(pen, 4), frames(vjp, 8), frames(dist, 8), frames(dist, 4)) == (2, 4, 2, 8, 16)


def test_a_null_model_is_invalid_before_a_device_is_looked_for():
    lib = _lib.load()
    z = (None,) * 8
    calls = [lambda a, b: lib.dexr_cross_distances_dev(a, b, 4, *z, None, None, None, None, None),
             lambda a, b: lib.dexr_cross_distances_vjp_dev(a, b, 4, *z, None, None, None, None, None, None, None),
             lambda a, b: lib.dexr_cross_penalty_dev(a, b, 4, *z, 0.01, None, None, None, None, None, None, None),
             lambda a, b: lib.dexr_cross_distances(a, b, 4, *z, None, None, None, None),
             lambda a, b: lib.dexr_cross_distances_vjp(a, b, 4, *z, None, None, None, None, None, None),
             lambda a, b: lib.dexr_cross_penalty(a, b, 4, *z, 0.01, None, None, None, None, None, None)]
    for f in calls:
        assert f(None, None) == INVALID and b"null sphere model" in lib.dexr_last_error()
    # (every other DEXR_ERR_INVALID case needs a model, which needs a device: tests/test_gpu_cross.py)


# ---- 2. the argument rules of the torch front ---------------------------------------------------------------------------------------
def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    touched = []
    for cls in (_lib.SphereModel, _lib.PoseModel):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("cross_distances_dev", "cross_distances_vjp_dev", "cross_penalty_dev"):
        monkeypatch.setattr(_lib.SphereModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    assert len(sub.idx_pin2fixed) == 6 and sub.opt_dof == 10
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "base_link"]
    sa = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    sb = collision.SphereSet(tips[:3], np.zeros((3, 3)), np.full(3, 0.01))
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    w = torch.ones((4, 3), dtype=torch.float32)
    pos, rot = torch.zeros((4, 3), dtype=torch.float32), torch.eye(3, dtype=torch.float32).repeat(4, 1, 1)
    fronts = [lambda qa, s, qb, t, margin=0.01, **k: collision.cross_penalty(opt, qa, s, opt, qb, t, margin, **k),
              lambda qa, s, qb, t, margin=0.01, **k: ag.cross_penalty(opt, qa, s, opt, qb, t, margin, **k),
              lambda qa, s, qb, t, margin=0.01, **k: collision.robot_cross_penalty(opt.robot, qa, s, opt.robot, qb, t, margin, **k),
              lambda qa, s, qb, t, margin=0.01, **k: ag.robot_cross_penalty(opt.robot, qa, s, opt.robot, qb, t, margin, **k)]
    dists = [lambda qa, s, qb, t, **k: collision.cross_distances(opt, qa, s, opt, qb, t, **k),
             lambda qa, s, qb, t, **k: ag.cross_distances(opt, qa, s, opt, qb, t, **k),
             lambda qa, s, qb, t, **k: collision.robot_cross_distances(opt.robot, qa, s, opt.robot, qb, t, **k),
             lambda qa, s, qb, t, **k: ag.robot_cross_distances(opt.robot, qa, s, opt.robot, qb, t, **k)]

    def raises(fns, match=None, qa=good, s=sa, qb=good, t=sb, **kw):
        for f in fns:
            with pytest.raises(ValueError, match=match):
                f(qa, s, qb, t, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises(fronts + dists, "CUDA")
    raises(fronts + dists, "CUDA", pos_a=pos, rot_a=rot, pos_b=pos, rot_b=rot)
    raises(fronts, "CUDA", pair_weight=w, margin=0)
    raises(fronts, "CUDA", margin=1)  # Python ints are numbers too
    raises(fronts[::2], "CUDA", wrench=True)
    raises(dists[::2], "CUDA", nearest=True)
    # dtype, shape, type of either q; both sides' B equal
    for side in ("qa", "qb"):
        raises(fronts + dists, "float32", **{side: good.double()})
        for bad in (good[:, :15], good.reshape(-1), good[:, :, None]):
            raises(fronts + dists, "shape", **{side: bad})
        raises(fronts + dists, "torch tensor", **{side: good.numpy()})
    raises(fronts + dists, "one row per frame", qb=good[:3])
    raises(fronts + dists, "one row per frame", qa=good[:1])
    # the sphere sets
    for side in ("s", "t"):
        raises(fronts + dists, "SphereSet", **{side: tips})
        raises(fronts + dists, "is not a link name", **{side: collision.SphereSet(["link_15.0_tip", "no_such_link"], np.zeros((2, 3)), [0.01, 0.01])})
    # margin: a finite Python float >= 0
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.01), None, "0.01", True):
        raises(fronts, "margin", margin=bad)
    # pair_weight: a float32 tensor (S_a, S_b)
    raises(fronts, "float32", pair_weight=w.double())
    raises(fronts, "torch tensor", pair_weight=w.numpy())
    for bad in (w.T.contiguous(), w[:3], w[None], w.reshape(-1), torch.ones((4, 4))):
        raises(fronts, "pair_weight must have shape", pair_weight=bad)
    # the four base poses: float32 tensors of one pose per frame
    for k in ("pos_a", "pos_b"):
        raises(fronts + dists, "float32", **{k: pos.double()})
        raises(fronts + dists, "torch tensor", **{k: pos.numpy()})
        for bad in (pos[:3], pos[:, :2], pos[0], torch.zeros((1, 3))):
            raises(fronts + dists, f"{k} must have shape", **{k: bad})
    for k in ("rot_a", "rot_b"):
        raises(fronts + dists, "float32", **{k: rot.double()})
        raises(fronts + dists, "torch tensor", **{k: rot.numpy()})
        for bad in (rot[:3], rot.reshape(4, 9), rot[0], pos):
            raises(fronts + dists, f"{k} must have shape", **{k: bad})
        # no gradient flows to a rotation matrix: the message names the way to the torque
        raises(fronts[1::2] + dists[1::2], "wrench=True", **{k: rot.clone().requires_grad_(True)})
    # fixed_qpos on either side: one too many, one missing, one of the wrong width
    raises(fronts[:2] + dists[:2], "fixed_qpos", fixed_qpos_a=torch.zeros((4, 1), dtype=torch.float32))
    raises(fronts[:2] + dists[:2], "fixed_qpos", fixed_qpos_b=torch.zeros((4, 1), dtype=torch.float32))
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    for fq, word in ((None, "fixed_qpos"), (torch.zeros((4, 5), dtype=torch.float32), "fixed_qpos"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                     (torch.zeros((4, 6), dtype=torch.float32), "CUDA")):
        for f in (collision.cross_distances, ag.cross_distances):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sa, opt, good, sb, fixed_qpos_a=fq)
            with pytest.raises(ValueError, match=word):
                f(opt, good, sa, sub, q10, sb, fixed_qpos_b=fq)
        for f in (collision.cross_penalty, ag.cross_penalty):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sa, opt, good, sb, 0.01, fixed_qpos_a=fq)
            with pytest.raises(ValueError, match=word):
                f(opt, good, sa, sub, q10, sb, 0.01, fixed_qpos_b=fq)
    assert touched == []
    # the host-pointer methods keep the shape rules (no device: the handle is never read)
    m = _lib.SphereModel.__new__(_lib.SphereModel)
    m.n_in, m.n_fixed, m.n_sphere = 16, 0, 4
    z = np.zeros((4, 16))
    for call in (lambda: m.cross_distances(m, z, z[:3]), lambda: m.cross_distances(m, z, z, pos_b=np.zeros((4, 2))),
                 lambda: m.cross_distances(m, z, z, rot_a=np.zeros((4, 9))), lambda: m.cross_distances_vjp(m, z, z, grad_dist_a=np.zeros((4, 5))),
                 lambda: m.cross_distances_vjp(m, z, z, grad_dist_b=np.zeros((3, 4))), lambda: m.cross_penalty(m, z, z, 0.01, np.ones((4, 3))),
                 lambda: m.cross_penalty(m, z[:, :15], z, 0.01)):
        with pytest.raises(ValueError):
            call()


# ---- 3. the yardstick against central differences of its own energy and distances ---------------------------------------------------
H, GATE_D, GATE_E = 1e-6, 1e-8, 1e-6


def _small_rotation(k, theta):
    K = np.zeros((3, 3))
    i, j = (k + 1) % 3, (k + 2) % 3
    K[j, i], K[i, j] = 1.0, -1.0
    return np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * (K @ K)


def test_reference_gradients_equal_central_differences():
    d = cross_inputs("shadow_right_left")
    near = np.flatnonzero(~FAR)[:4]  # four frames with the hands in reach
    d4 = {k: (v[near] if isinstance(v, np.ndarray) and k not in ("w",) else v) for k, v in d.items()}
    A, Bs = sides(d4)
    F = xref.fields(A, Bs)
    clear_a, clear_b = clear_entries(F["d"])
    ga, gb = np.where(clear_a, d4["ga"], 0.0), np.where(clear_b, d4["gb"], 0.0)
    scale = np.abs(ga).sum(1, keepdims=True) + np.abs(gb).sum(1, keepdims=True)
    ga, gb = ga / scale, gb / scale  # per frame sum |g| = 1
    va, vb, vwa, vwb = xref.distances_vjp(F, A, Bs, ga, gb)
    E, gxa, gxb, wa, wb, h = xref.penalty(F, A, Bs, d["margin"], d["w"])
    assert (h > 0).any(1).any(1).all() and clear_a.mean() > 0.9 and clear_b.mean() > 0.9

    def values(**over):
        A_, B_ = sides(d4, jacobian=False, **over)
        F_ = xref.fields(A_, B_)
        da, _, db, _ = xref.distances(F_)
        return (ga * da).sum(1) + (gb * db).sum(1), xref.penalty(F_, A_, B_, d["margin"], d["w"])[0]

    worst = dict(L=0.0, E=0.0)

    def check(plus, minus, want_l, want_e, what):
        (lp, ep), (lm, em) = values(**plus), values(**minus)
        el, ee = float(np.abs((lp - lm) / (2 * H) - want_l).max()), float(np.abs((ep - em) / (2 * H) - want_e).max())
        worst["L"], worst["E"] = max(worst["L"], el), max(worst["E"], ee)
        assert el <= GATE_D and ee <= GATE_E, (what, el, ee)

    for key, vjp, grad in (("q_a", va, gxa), ("q_b", vb, gxb)):
        for c in range(d4[key].shape[1]):
            qp, qm = d4[key].copy(), d4[key].copy()
            qp[:, c] += H
            qm[:, c] -= H
            check({key: qp}, {key: qm}, vjp[:, c], grad[:, c], (key, c))
    for tag, vw, w in (("a", vwa, wa), ("b", vwb, wb)):
        for k in range(3):
            pp, pm = d4[f"pos_{tag}"].copy(), d4[f"pos_{tag}"].copy()
            pp[:, k] += H
            pm[:, k] -= H
            check({f"pos_{tag}": pp}, {f"pos_{tag}": pm}, vw[:, k], w[:, k], (f"pos_{tag}", k))
            rp, rm = _small_rotation(k, H) @ d4[f"rot_{tag}"], _small_rotation(k, -H) @ d4[f"rot_{tag}"]
            check({f"rot_{tag}": rp}, {f"rot_{tag}": rm}, vw[:, 3 + k], w[:, 3 + k], (f"rot_{tag}", k))
    print(f"shadow_right_left, 4 frames: max |dL - central difference| = {worst['L']:.3e} (gate {GATE_D:.0e}), max |dE - central difference| = "
          f"{worst['E']:.3e} (gate {GATE_E:.0e}); max |dE/dq_a| {np.abs(gxa).max():.3e}, max |force| {np.abs(wa[:, :3]).max():.3e}, "
          f"max |torque| {np.abs(wa[:, 3:]).max():.3e}")
    assert np.abs(gxa).max() > 1e-3 and np.abs(gxb).max() > 1e-3 and np.abs(wa[:, 3:]).max() > 1e-4 and np.abs(vwb[:, 3:]).max() > 1e-4
    # action and reaction: the forces cancel, the torques cancel about the world origin
    assert np.abs(wa[:, :3] + wb[:, :3]).max() < 1e-12
    ta = wa[:, 3:] + np.cross(d4["pos_a"], wa[:, :3])
    tb = wb[:, 3:] + np.cross(d4["pos_b"], wb[:, :3])
    assert np.abs(ta + tb).max() < 1e-12


# ---- 4. the inputs of the GPU tests -------------------------------------------------------------------------------------------------
def conditions(d, r64, clear_a, clear_b):
    """-> None where the conditions the GPU gates rest on hold, else what fails."""
    active = r64["h"] > 0
    if active.any((1, 2)).mean() < 0.5:
        return f"only {active.any((1, 2)).mean():.2f} of the frames have an active pair"
    if active.any() and r64["s"][active].min() < 1e-3:
        return f"an active pair has centres {r64['s'][active].min() * 1e3:.2f} mm apart"
    if min(clear_a.mean(), clear_b.mean()) < 0.9:
        return f"clear shares {clear_a.mean():.3f}, {clear_b.mean():.3f}"
    return None


@pytest.mark.parametrize("case", sorted(PAIRS))
def test_gpu_inputs_meet_the_conditions_the_gpu_gates_rest_on(case):
    assert len(PAIRS) == 6
    d, ref = cross_inputs(case), reference(case)
    r64 = ref["r64"]
    for k in ("q_a", "q_b", "pos_a", "rot_a", "pos_b", "rot_b", "w", "ga", "gb"):
        assert np.array_equal(d[k], _r32(d[k])), k
    active = r64["h"] > 0
    print(f"{case}: {r64['d'].shape[1]} spheres against {r64['d'].shape[2]}; frames with an active pair {active.any((1, 2)).mean():.3f}, active "
          f"share of the pairs {active.mean():.4f}, penetrating share {(r64['d'] < 0).mean():.4f}, smallest centre distance of an active pair "
          f"{r64['s'][active].min() * 1e3:.2f} mm, clear share {ref['clear_a'].mean():.4f} (A) {ref['clear_b'].mean():.4f} (B), max E "
          f"{r64['E'].max():.3e}, max |grad| {max(np.abs(r64['grad_a']).max(), np.abs(r64['grad_b']).max()):.3e}")
    assert conditions(d, r64, ref["clear_a"], ref["clear_b"]) is None
    assert FAR.mean() >= 0.1
    for k in ("E", "grad_a", "grad_b", "wrench_a", "wrench_b"):
        assert np.isfinite(r64[k]).all() and not r64[k][FAR].any() and not ref["r32"][k][FAR].any(), k
    assert (r64["dist_a"][FAR] > 5).all() and (r64["E"][~FAR] > 0).any() and np.abs(r64["vjp_a"]).max() > 0 and np.abs(r64["vjp_b"]).max() > 0


def test_the_pose_seed_is_the_first_that_meets_the_conditions():
    for seed in range(POSE_SEED + 1):
        failed = None
        for case in sorted(PAIRS):
            d = cross_inputs(case, seed)
            A, Bs = sides(d, jacobian=False)
            F = xref.fields(A, Bs)
            h = np.maximum(0.0, d["margin"] - F["d"])
            failed = conditions(d, dict(h=h, s=F["s"]), *clear_entries(F["d"]))
            if failed:
                print(f"seed {seed}: {case}: {failed}")
                break
        assert (failed is None) == (seed == POSE_SEED), (seed, failed)

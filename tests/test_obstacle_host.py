"""CPU tests of the obstacle collision's interface (include/dexr_obstacles.h, dex_retargeting_amd/collision.py): the export list
against the header, dexr_obstacle_set_create's validation (every malformed input DEXR_ERR_INVALID before a device is looked for),
collision.ObstacleSet and the argument rules of the torch front (every one a ValueError before any device call), the yardstick
tests/obstacle_reference.py against central differences of its own float64 values, and the behaviour of the yardstick on the
inputs of tests/test_gpu_obstacles.py, so that the inputs are proven before a GPU sees them.

INPUTS (obstacle_inputs; shared with the GPU tests).  collision_inputs(name, "offset") of tests/test_collision_host.py: the eight
fixture robots, two spheres of radius 0.010 per link, B = 33, q seeded.  OBSTACLES is one set of all four kinds, nine primitives
a few centimetres across around the origin of the obstacle frame (a degenerate capsule a == b and a rotated box among them).  The
obstacle frame has a pose per frame from default_rng(POSE_SEED): a random rotation, and the origin at the centroid of the frame's
sphere centres plus an offset of up to 2 cm -- a held object inside the hand's workspace; in every fourth frame the origin is moved
2 m against the half-space's normal, which takes every sphere out of reach of every primitive (E == 0 there).  Poses, margin
0.010 and the primitive weights (default_rng(W_SEED), 0.5 .. 2) are float32-representable.  POSE_SEED = 64 is the first of the
seeds 0, 1, 2, ... with which the conditions of section 4 hold on all eight robots and no active entry is within a millimetre of a
sphere's centre or a capsule's axis (with each of 0 .. 63 some robot has an active box-interior entry nearer than 1e-4 m to a tie,
or such an entry).

CENTRAL DIFFERENCES (float64, step H = 1e-7).  A smooth f errs by H^2 |f'''| / 6 + eps |f| / H.  A signed distance has |sdf| < 1
(rounding: 1e-9) and, at distance rho from a sphere's centre or a capsule's axis, |f'''| <= 3 / rho^2: with rho >= POINT_SDF =
1e-3 m the first term is 5e-9; gate 1e-8.  E: up to a few hundred active entries of w h^2 <= 2 * 0.06^2 with lever arms below
0.5 m/rad: rounding 1e-9; the curvature term of an entry is H^2 2 w h 3 / (6 rho^2) <= 2.4e-7 at rho = POINT_E = 1e-4 m; and E is
only C1: an entry within H |d'| of the margin, of a box face's edge or of a capsule's end cap adds H times the jump of its second
derivative (2 w d'^2 <= 1, or 2 w h kappa d'^2 with h <= 0.06, kappa = 1 / distance), 1e-7 per such entry at the very worst; gate
2e-6 (the gradients themselves reach 1e-1).
KINKS.  The distance itself is not differentiable where a box-interior point has its two largest q_i tied (the normal jumps), on
a sphere's centre and on a capsule's axis (the curvature diverges).  An entry is near a kink when it is within TIE = 1e-5 m of
such a tie (a hundred steps) or within POINT_* of such a point or axis.  A frame with an ACTIVE entry (h > 0) near a kink is left
out of the comparison of E; at most 2 % of the frames may be (asserted: POSE_SEED is committed)."""
import functools
import os
import re

import numpy as np
import pytest

import collision_reference as cref
import obstacle_reference as oref
from testutil import REPO
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, MARGIN, ROBOTS, collision_inputs, robot_of
from test_jacobian_host import SUBSET_CFG

HEADER = os.path.join(REPO, "include", "dexr_obstacles.h")
POSE_SEED, W_SEED, GD_SEED = 64, 42, 43
INVALID, HIP = -1, -2
H, TIE, POINT_SDF, POINT_E, GATE_SDF, GATE_E = 1e-7, 1e-5, 1e-3, 1e-4, 1e-8, 2e-6
TIE_GAP, NEAR_GAP = 1e-4, 1e-5  # what the GPU gates rest on


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _rotations(rng, n):
    """n rotation matrices from seeded axis-angles (Rodrigues)."""
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(-np.pi, np.pi, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    return np.eye(3) + np.sin(ang)[:, None, None] * K + (1 - np.cos(ang))[:, None, None] * (K @ K)


def _box_rotation():
    return _rotations(np.random.default_rng(7), 1)[0]


@functools.lru_cache(maxsize=None)
def obstacles():
    """the set of the GPU tests: all four kinds, nine primitives (metres, obstacle frame)."""
    s = collision.ObstacleSet.spheres([[0.02, 0.0, 0.01], [-0.04, 0.03, -0.02]], [0.03, 0.02])
    c = collision.ObstacleSet.capsules([[-0.05, -0.02, 0.03], [0.0, 0.05, -0.03]], [[0.05, 0.01, 0.04], [0.0, 0.05, -0.03]], [0.012, 0.015])
    b = collision.ObstacleSet.boxes([[0.0, -0.04, 0.0], [0.05, 0.04, -0.03]], [[0.03, 0.015, 0.04], [0.02, 0.02, 0.01]],
                                    [_box_rotation(), np.eye(3)])
    h = collision.ObstacleSet.half_spaces([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]], [-0.06, -0.09])
    sset = s + c + b + h + collision.ObstacleSet.spheres([[0.0, -0.07, 0.05]], [0.0])
    assert sset.n_prim == 9 and sorted(set(sset.kinds.tolist())) == [0, 1, 2, 3]
    return sset


@functools.lru_cache(maxsize=None)
def obstacle_inputs(name):
    """dict: the collision_inputs(name, "offset") entries and oset, kinds, params, pos (B, 3), rot (B, 3, 3), w (M,), gd (B, S);
    arrays read-only."""
    d = dict(collision_inputs(name, "offset"))
    oset = obstacles()
    c = cref.centres(d["orc"], d["q"], d["links"], d["rows"], d["centers"])[0]
    rng = np.random.default_rng(POSE_SEED)
    rot = _r32(_rotations(rng, B))
    pos = c.mean(1) + rng.uniform(-0.02, 0.02, (B, 3))
    far = np.arange(B) % 4 == 3
    pos[far] -= 2.0 * (rot[far] @ np.array([0.0, 0.0, 1.0]))
    d.update(oset=oset, kinds=oset.kinds, params=oset.params, pos=_r32(pos), rot=rot, far=far,
             w=_r32(np.random.default_rng(W_SEED).uniform(0.5, 2.0, oset.n_prim)),
             gd=_r32(np.random.default_rng(GD_SEED).standard_normal((B, len(d["radii"])))))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _geo(d):
    return d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"], d["kinds"], d["params"]


def clear_nearest(d64):
    """(B, S) bool from the float64 d (B, S, M): the two smallest differ by more than NEAR_GAP, so that float32 rounding cannot
    change which primitive is the nearest (every entry of a one-primitive set)."""
    if d64.shape[-1] == 1:
        return np.ones(d64.shape[:2], bool)
    two = np.sort(d64, -1)[..., :2]
    return two[..., 1] - two[..., 0] > NEAR_GAP


@functools.lru_cache(maxsize=None)
def masked_cotangent(name):
    """`gd` with zeros where the nearest primitive is not clear: the cotangent of every VJP of the GPU tests, read-only."""
    d = obstacle_inputs(name)
    F = oref.fields(*_geo(d), d["pos"], d["rot"], jacobian=False)
    g = np.where(clear_nearest(F["d"]), d["gd"], 0.0)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(name, dtype=np.float64):
    """the yardstick on obstacle_inputs(name), computed once and shared, read-only: dict dist, nearest, vjp (of the cotangent
    masked_cotangent(name)), E, grad, wrench (with the weights `w`), and d (B, S, M), h (B, S, M)."""
    d = obstacle_inputs(name)
    F = oref.fields(*_geo(d), d["pos"], d["rot"], dtype)
    dist, near = oref.distances(F)
    E, grad, wrench, h = oref.penalty(F, d["margin"], d["w"])
    out = dict(dist=dist, nearest=near, vjp=oref.distances_vjp(F, masked_cotangent(name)), E=E, grad=grad, wrench=wrench, d=F["d"], h=h)
    for k, v in out.items():
        assert v.dtype == (np.int32 if k == "nearest" else dtype), k
        v.setflags(write=False)
    return out


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    assert declared == set(_lib.OBSTACLE_EXPORTS) and len(_lib.OBSTACLE_EXPORTS) == 9 and len(set(_lib.OBSTACLE_EXPORTS)) == 9
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS, _lib.WRENCH_EXPORTS, _lib.IK_EXPORTS, _lib.IK_SOLVE_EXPORTS,
                  _lib.SPHERE_EXPORTS, _lib.RESOLVE_EXPORTS):
        assert not set(_lib.OBSTACLE_EXPORTS) & set(other)
    lib = _lib.load()
    for name in _lib.OBSTACLE_EXPORTS:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in ("dexr_resolve.h", "dexr_spheres.h", "dexr_ik_solve.h", "dexr_ik.h", "dexr_wrench.h", "dexr_jacobian.h", "dexr_pose.h", "dexr.h"):
        assert not _declared(os.path.join(REPO, "include", h)) & declared
    text = open(HEADER).read()
    assert int(re.search(r"#define DEXR_OBSTACLE_MAX (\d+)", text).group(1)) == _lib.OBSTACLE_MAX == 64
    assert int(re.search(r"#define DEXR_OBSTACLE_PARAMS (\d+)", text).group(1)) == _lib.OBSTACLE_PARAMS == 16
    for i, k in enumerate(("SPHERE", "CAPSULE", "BOX", "HALFSPACE")):
        assert int(re.search(rf"#define DEXR_OBSTACLE_{k} (\d+)", text).group(1)) == getattr(_lib, f"OBSTACLE_{k}") == i
    assert (oref.SPHERE, oref.CAPSULE, oref.BOX, oref.HALFSPACE) == (0, 1, 2, 3)
    from dex_retargeting_amd import autograd as ag

    for n in ("obstacle_distances", "obstacle_penalty", "robot_obstacle_distances", "robot_obstacle_penalty"):
        assert n in collision.__all__ and n in ag.__all__
    assert "ObstacleSet" in collision.__all__
    for f in ("dexr_obstacles.hpp", "dexr_spheres.hpp"):
        src = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", f)).read()
        assert "getenv" not in src and "atomic" not in src and "asm" not in src.replace("__restrict__", ""), f
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_obstacles.hpp"') == 1 and pose.index('"dexr_obstacles.hpp"') > pose.index('"dexr_resolve.hpp"')


def _create(kind, param, n_prim=None):
    lib = _lib.load()
    kind = None if kind is None else np.ascontiguousarray(kind, np.int32)
    param = None if param is None else np.ascontiguousarray(param, np.float64)
    h = _lib.C.c_void_p()
    p = lambda a, t: None if a is None else a.ctypes.data_as(_lib.C.POINTER(t))  # noqa: E731
    rc = lib.dexr_obstacle_set_create(len(kind) if n_prim is None else n_prim, p(kind, _lib.C.c_int32), p(param, _lib.C.c_double), _lib.C.byref(h))
    if rc == 0:
        lib.dexr_obstacle_set_destroy(h)
    else:
        assert not h.value
    return rc, lib.dexr_last_error().decode()


def _malformed():
    """(word of the C message, word of the Python message, kinds, params) of every malformed set."""
    ok = obstacles()
    K, P = ok.kinds, ok.params
    cases_ = []

    def one(cword, pyword, m, col, value):
        p = P.copy()
        p[m, col] = value
        cases_.append((cword, pyword, K, p))

    for bad in (np.nan, np.inf, -np.inf):
        one("finite", "finite", 0, 1, bad)
        one("finite", "finite", 6, 15, bad)  # an unused parameter too
    one("radius", "radius", 0, 3, -1e-9)
    one("radius", "radius", 2, 6, -1.0)
    one("half extent", "half extents", 4, 4, 0.0)
    one("half extent", "half extents", 5, 3, -0.01)
    one("orthonormal", "orthonormal", 4, 6, P[4, 6] + 1e-5)
    p = P.copy()
    p[5, 6:15] = (2 * np.eye(3)).reshape(-1)
    cases_.append(("orthonormal", "orthonormal", K, p))
    one("unit", "unit", 6, 2, 1.0 + 1e-5)
    one("unit", "unit", 7, 0, 0.0)
    for bad in (-1, 4, 99):
        k = K.copy()
        k[3] = bad
        cases_.append(("kind", "kinds", k, P))
    cases_.append(("primitives", "1..64", np.zeros(65, np.int32), np.tile(P[:1], (65, 1))))
    return cases_


def test_obstacle_set_create_validates_before_it_looks_for_a_device():
    ok = obstacles()
    for cword, _, k, p in _malformed():
        rc, msg = _create(k, p)
        assert rc == INVALID and cword in msg, (rc, msg, cword)
    rc, msg = _create(ok.kinds, ok.params, n_prim=0)
    assert rc == INVALID and "primitives" in msg
    for a in (dict(kind=None, param=ok.params), dict(kind=ok.kinds, param=None)):
        rc, msg = _create(n_prim=9, **a)
        assert rc == INVALID and "null" in msg
    assert _lib.load().dexr_obstacle_set_create(9, None, None, None) == INVALID
    # the limits themselves are fine: 64 primitives, radii of zero, a rotation and a normal off by less than 1e-6
    want = 0 if _lib.load().dexr_device_count() > 0 else HIP  # a well-formed input needs a device
    p = ok.params.copy()
    p[4, 6] += 5e-7
    p[6, 2] += 5e-7
    p[0, 3] = p[2, 6] = 0.0
    for k, pp in ((ok.kinds, ok.params), (ok.kinds, p), (np.tile(ok.kinds[:8], 8), np.tile(ok.params[:8], (8, 1)))):
        rc, msg = _create(k, pp)
        assert rc == want, (rc, msg)
    if want == HIP:
        with pytest.raises(_lib.DexrError, match="libdexr error -2"):
            _lib.ObstacleSet(ok.kinds, ok.params)
    with pytest.raises(ValueError, match="one row per primitive"):
        _lib.ObstacleSet(ok.kinds, ok.params[:, :15])
    lib = _lib.load()
    assert lib.dexr_obstacle_set_info(None, None) == INVALID and b"null obstacle set" in lib.dexr_last_error()
    lib.dexr_obstacle_set_destroy(None)


# ---- 2. ObstacleSet and the argument rules of the torch front -------------------------------------------------------------------------
def test_obstacle_set_is_plain_hashable_data_with_the_rules_of_the_c_side(monkeypatch):
    a, O = obstacles(), collision.ObstacleSet
    b = O(a.kinds.tolist(), a.params.copy())
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1 and a.n_prim == 9 and a.params.shape == (9, 16) and a.kinds.dtype == np.int32
    assert a != O.spheres([[0, 0, 0]], [0.01]) and a != O(a.kinds, np.where(a.params == 0.03, 0.031, a.params))
    with pytest.raises(ValueError):
        a.params[0, 0] = 1.0
    s = O.spheres([[1, 2, 3]], [0.5])
    c = O.capsules([[1, 2, 3]], [[4, 5, 6]], [0.25])
    x = O.boxes([[1, 2, 3]], [[0.1, 0.2, 0.3]])
    h = O.half_spaces([[0, 1, 0]], [0.75])
    assert s.params[0].tolist() == [1, 2, 3, 0.5] + [0] * 12 and c.params[0].tolist() == [1, 2, 3, 4, 5, 6, 0.25] + [0] * 9
    assert x.params[0].tolist() == [1, 2, 3, 0.1, 0.2, 0.3, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0] and h.params[0].tolist() == [0, 1, 0, 0.75] + [0] * 12
    both = s + h + x
    assert both.kinds.tolist() == [0, 3, 2] and both == O.concat(s, h, x) and np.array_equal(both.params[1], h.params[0]) and "box" in repr(both)
    for _, pyword, k, p in _malformed():
        with pytest.raises(ValueError, match=pyword):
            O(k, p)
    for bad, word in ((lambda: O([], np.zeros((0, 16))), "1..64"), (lambda: O([0], np.zeros((1, 15))), "shape"),
                      (lambda: O.spheres(np.zeros((2, 3)), [0.01]), "shape"), (lambda: O.spheres(np.zeros((2, 2)), [0.01, 0.01]), "shape"),
                      (lambda: O.spheres(np.zeros((0, 3)), []), "shape"), (lambda: O.capsules(np.zeros((1, 3)), np.zeros((2, 3)), [0.01]), "shape"),
                      (lambda: O.boxes(np.zeros((1, 3)), [[0.1, 0.1]]), "shape"), (lambda: O.boxes(np.zeros((1, 3)), [[0.1, 0.1, 0.1]], np.eye(3)), "shape"),
                      (lambda: O.half_spaces([[0, 0, 1]], [[0.0]]), "shape"), (lambda: O.concat(), "ObstacleSet"), (lambda: O.concat(s, "x"), "ObstacleSet"),
                      (lambda: O.concat(*[a] * 8), "1..64")):
        with pytest.raises(ValueError, match=word):
            bad()
    with pytest.raises(TypeError):
        s + 1
    assert O.concat(*[O.spheres(np.zeros((8, 3)), np.zeros(8))] * 8).n_prim == 64
    # the device tables: made once per set (and device), kept with it
    made = []
    monkeypatch.setattr(_lib.ObstacleSet, "__init__", lambda self, kind, param: made.append((len(kind), np.asarray(param).shape)))
    t = O.spheres([[0, 0, 0]], [0.01])
    assert t.device_set(0) is t.device_set(0) and t.device_set(1) is not t.device_set(0) and made == [(1, (1, 16))] * 2


def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    touched = []
    for cls in (_lib.SphereModel, _lib.PoseModel, _lib.ObstacleSet):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("obstacle_distances_dev", "obstacle_distances_vjp_dev", "obstacle_penalty_dev"):
        monkeypatch.setattr(_lib.SphereModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "base_link"]
    sset = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    obs = obstacles()
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    w = torch.ones((obs.n_prim,), dtype=torch.float32)
    pos, rot = torch.zeros((4, 3), dtype=torch.float32), torch.eye(3, dtype=torch.float32).repeat(4, 1, 1)
    fronts = [lambda q, s, o, margin=0.01, **k: collision.obstacle_penalty(opt, q, s, o, margin, **k),
              lambda q, s, o, margin=0.01, **k: ag.obstacle_penalty(opt, q, s, o, margin, **k),
              lambda q, s, o, margin=0.01, **k: collision.robot_obstacle_penalty(opt.robot, q, s, o, margin, **k),
              lambda q, s, o, margin=0.01, **k: ag.robot_obstacle_penalty(opt.robot, q, s, o, margin, **k)]
    dists = [lambda q, s, o, **k: collision.obstacle_distances(opt, q, s, o, **k), lambda q, s, o, **k: ag.obstacle_distances(opt, q, s, o, **k),
             lambda q, s, o, **k: collision.robot_obstacle_distances(opt.robot, q, s, o, **k),
             lambda q, s, o, **k: ag.robot_obstacle_distances(opt.robot, q, s, o, **k)]

    def raises(fns, match=None, q=good, s=sset, o=obs, **kw):
        for f in fns:
            with pytest.raises(ValueError, match=match):
                f(q, s, o, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises(fronts + dists, "CUDA")
    raises(fronts + dists, "CUDA", obstacle_pos=pos, obstacle_rot=rot)
    raises(fronts, "CUDA", prim_weight=w, margin=0)
    raises(fronts, "CUDA", margin=1)  # Python ints are numbers too
    raises(fronts[::2], "CUDA", wrench=True)
    raises(dists[::2], "CUDA", nearest=True)
    # dtype, shape, type of q
    raises(fronts + dists, "float32", q=good.double())
    for bad in (good[:, :15], good.reshape(-1), good[:, :, None]):
        raises(fronts + dists, "shape", q=bad)
    raises(fronts + dists, "torch tensor", q=good.numpy())
    # the sphere set and the obstacle set
    raises(fronts + dists, "SphereSet", s=tips)
    raises(fronts + dists, "is not a link name", s=collision.SphereSet(["link_15.0_tip", "no_such_link"], np.zeros((2, 3)), [0.01, 0.01]))
    raises(fronts + dists, "0 pairs", s=collision.SphereSet(["link_15.0_tip", "link_15.0"], np.zeros((2, 3)), [0.01, 0.01]))
    raises(fronts + dists, "ObstacleSet", o=(obs.kinds, obs.params))
    raises(fronts + dists, "ObstacleSet", o=None)
    # margin: a finite Python float >= 0
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.01), None, "0.01", True):
        raises(fronts, "margin", margin=bad)
    # prim_weight: a float32 tensor of one weight per primitive
    raises(fronts, "float32", prim_weight=w.double())
    raises(fronts, "torch tensor", prim_weight=w.numpy())
    for bad in (w[:5], w[None], torch.ones((obs.n_prim, 1)), torch.ones(obs.n_prim + 1)):
        raises(fronts, "shape", prim_weight=bad)
    # the obstacle pose: float32 tensors of one pose per frame
    raises(fronts + dists, "float32", obstacle_pos=pos.double())
    raises(fronts + dists, "float32", obstacle_rot=rot.double())
    raises(fronts + dists, "torch tensor", obstacle_pos=pos.numpy())
    raises(fronts + dists, "torch tensor", obstacle_rot=rot.numpy())
    for bad in (pos[:3], pos[:, :2], pos[0], torch.zeros((1, 3))):
        raises(fronts + dists, "obstacle_pos must have shape", obstacle_pos=bad)
    for bad in (rot[:3], rot.reshape(4, 9), rot[0], pos):
        raises(fronts + dists, "obstacle_rot must have shape", obstacle_rot=bad)
    # no gradient flows to a rotation matrix: the message names the way to the torque
    raises(fronts[1::2] + dists[1::2], "wrench=True", obstacle_rot=rot.clone().requires_grad_(True))
    # fixed_qpos: one too many, one missing, one of the wrong width
    raises(fronts[:2] + dists[:2], "fixed_qpos", fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    assert len(sub.idx_pin2fixed) == 6
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    for fq, word in ((None, "fixed_qpos"), (torch.zeros((4, 5), dtype=torch.float32), "fixed_qpos"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                     (torch.zeros((4, 6), dtype=torch.float32), "CUDA")):
        for f in (collision.obstacle_distances, ag.obstacle_distances):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sset, obs, fixed_qpos=fq)
        for f in (collision.obstacle_penalty, ag.obstacle_penalty):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sset, obs, 0.01, fixed_qpos=fq)
    assert touched == []


# ---- 3. the yardstick against central differences -----------------------------------------------------------------------------------
def test_reference_sdf_gradients_equal_central_differences():
    ok = obstacles()
    rng = np.random.default_rng(51)
    y = rng.uniform(-0.12, 0.12, (4000, 3))
    d, g = oref.sdf(ok.kinds, ok.params, y)
    assert d.shape == (4000, 9) and g.shape == (4000, 9, 3)
    fd = np.zeros_like(g)
    for i in range(3):
        e = np.zeros(3)
        e[i] = H
        fd[..., i] = (oref.sdf(ok.kinds, ok.params, y + e)[0] - oref.sdf(ok.kinds, ok.params, y - e)[0]) / (2 * H)
    kink = _near_kink(ok.kinds, ok.params, y, POINT_SDF)
    err = np.where(kink, 0.0, np.abs(fd - g).max(-1))
    inside_box = (d[:, 4] < 0).mean(), (d[:, 5] < 0).mean()
    print(f"max |grad sdf - central difference| = {err.max():.3e} (gate {GATE_SDF:.0e}); {int(kink.sum())} of {kink.size} entries near "
          f"a kink; box-interior share {inside_box[0]:.3f}, {inside_box[1]:.3f}")
    assert err.max() <= GATE_SDF and kink.mean() < 0.01 and min(inside_box) > 0.001
    # unit normals off the kinks; on a sphere's centre and a capsule's axis: no direction, no NaN
    assert np.abs(np.linalg.norm(g[~kink], axis=-1) - 1).max() < 1e-12
    on = np.array([ok.params[0, :3], ok.params[3, :3], ok.params[2, :3]])  # a sphere's centre, a degenerate capsule's, an end of an axis
    d0, g0 = oref.sdf(ok.kinds, ok.params, on)
    assert not g0[0, 0].any() and not g0[1, 3].any() and not g0[2, 2].any() and np.isfinite(d0).all() and np.isfinite(g0).all()
    assert d0[0, 0] == -ok.params[0, 3] and d0[1, 3] == -ok.params[3, 6] and d0[2, 2] == -ok.params[2, 6]
    # float32 runs in float32
    d32, g32 = oref.sdf(ok.kinds, ok.params, y.astype(np.float32), np.float32)
    assert d32.dtype == g32.dtype == np.float32 and np.abs(d32 - d).max() < 1e-6


def _kink_distance(kinds, params, y):
    """-> (point (..., M): the distance of y from a sphere's centre or a capsule's axis, tie (..., M): inside a box the gap between
    the two largest q_i); inf where the kind has no such kink."""
    d, _ = oref.sdf(kinds, params, y)
    point, tie = np.full(d.shape, np.inf), np.full(d.shape, np.inf)
    for m, (kind, v) in enumerate(zip(kinds, params)):
        if kind in (oref.SPHERE, oref.CAPSULE):
            point[..., m] = d[..., m] + (v[3] if kind == oref.SPHERE else v[6])  # |D|
        elif kind == oref.BOX:
            qq = np.sort(np.abs((y - v[:3]) @ v[6:15].reshape(3, 3)) - v[3:6], -1)
            tie[..., m] = np.where(qq[..., 2] <= 0, qq[..., 2] - qq[..., 1], np.inf)
    return point, tie


def _near_kink(kinds, params, y, point_gap):
    point, tie = _kink_distance(kinds, params, y)
    return (point < point_gap) | (tie < TIE)


@pytest.mark.parametrize("name", ["shadow_hand_right", "allegro_hand_right"])
def test_reference_energy_gradients_equal_central_differences(name):
    d = obstacle_inputs(name)
    orc, q, links, rows, centers, radii, kinds, params = _geo(d)
    pos, rot, w, margin = d["pos"], d["rot"], d["w"], d["margin"]

    def energy(q_, pos_=pos, rot_=rot):
        return oref.penalty(oref.fields(orc, q_, links, rows, centers, radii, kinds, params, pos_, rot_, jacobian=False), margin, w)[0]

    F = oref.fields(orc, q, links, rows, centers, radii, kinds, params, pos, rot)
    E, grad, wrench, h = oref.penalty(F, margin, w)
    y = np.einsum("bji,bsj->bsi", rot, F["arm"])
    near_kink = (_near_kink(kinds, params, y, POINT_E) & (h > 0)).any((1, 2))
    keep = ~near_kink
    assert near_kink.mean() <= 0.02, f"{int(near_kink.sum())} of {B} frames have an active entry near a kink"
    worst = {}
    fd = np.zeros_like(grad)
    for c in range(orc.dof):
        e = np.zeros(orc.dof)
        e[c] = H
        fd[:, c] = (energy(q + e) - energy(q - e)) / (2 * H)
    worst["q"] = float(np.abs(fd - grad)[keep].max())
    fd = np.zeros((B, 6))
    for i in range(3):
        e = np.zeros(3)
        e[i] = H
        fd[:, i] = (energy(q, pos + e) - energy(q, pos - e)) / (2 * H)
        # a world-aligned small rotation of the obstacle about its origin: R_o -> exp([e]) R_o, to first order (I + [e]) R_o
        K = np.zeros((3, 3))
        K[(i + 2) % 3, (i + 1) % 3], K[(i + 1) % 3, (i + 2) % 3] = H, -H
        fd[:, 3 + i] = (energy(q, pos, (np.eye(3) + K) @ rot) - energy(q, pos, (np.eye(3) - K) @ rot)) / (2 * H)
    worst["force"] = float(np.abs(fd - wrench)[keep, :3].max())
    worst["torque"] = float(np.abs(fd - wrench)[keep, 3:].max())
    print(f"{name}: max |dE/dq - cd| = {worst['q']:.3e}, |wrench force - cd| = {worst['force']:.3e}, |wrench torque - cd| = {worst['torque']:.3e} "
          f"(gate {GATE_E:.0e}); max |dE/dq| {np.abs(grad).max():.3e}, max |force| {np.abs(wrench[:, :3]).max():.3e}, max |torque| "
          f"{np.abs(wrench[:, 3:]).max():.3e}; {int(near_kink.sum())} frames left out")
    assert (E[keep] > 0).any() and np.abs(grad).max() > 1e-3 and np.abs(wrench[:, 3:]).max() > 1e-4
    assert max(worst.values()) <= GATE_E
    # the VJP is the contraction of the nearest normals with the same Jacobian: against central differences of the distances
    dist, near = oref.distances(F)
    gd = d["gd"]
    c = int(np.abs(grad).sum(0).argmax())
    e = np.zeros(orc.dof)
    e[c] = H
    dp, dm = (oref.distances(oref.fields(orc, x, links, rows, centers, radii, kinds, params, pos, rot, jacobian=False))[0] for x in (q + e, q - e))
    gap = np.sort(F["d"], -1)
    smooth = (gap[..., 1] - gap[..., 0] > NEAR_GAP) & ~np.take_along_axis(_near_kink(kinds, params, y, POINT_E), near[..., None].astype(np.int64), 2)[..., 0]
    want = (np.where(smooth, gd * (dp - dm) / (2 * H), 0.0)).sum(1)
    got = oref.distances_vjp(F, np.where(smooth, gd, 0.0))[:, c]
    assert np.abs(want - got).max() <= 1e-7 and smooth.mean() > 0.95


# ---- 4. the inputs of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_gpu_inputs_meet_the_conditions_the_gpu_gates_rest_on(name):
    d, r = obstacle_inputs(name), reference(name)
    kinds, params = d["kinds"], d["params"]
    assert d["pos"].shape == (B, 3) and d["rot"].shape == (B, 3, 3) and d["margin"] == MARGIN
    for k in ("pos", "rot", "w", "gd", "q", "centers"):
        assert np.array_equal(d[k], _r32(d[k])), k
    assert np.abs(np.einsum("bji,bjk->bik", d["rot"], d["rot"]) - np.eye(3)).max() < 1e-6
    F = oref.fields(*_geo(d), d["pos"], d["rot"], jacobian=False)
    y = np.einsum("bji,bsj->bsi", d["rot"], F["arm"])
    active = r["h"] > 0
    # every active box-interior entry is at least TIE_GAP from a tie of its two largest q_i
    tie = _kink_distance(kinds, params, y)[1]
    box = np.isin(kinds, [oref.BOX])
    interior = active[..., box] & np.isfinite(tie[..., box])
    assert interior.any() or name == "panda_gripper_glb"
    assert (tie[..., box][interior] >= TIE_GAP).all(), float(tie[..., box][interior].min())
    # ... and no active entry is within a millimetre of a sphere's centre or a capsule's axis, where the normal turns fastest
    point = _kink_distance(kinds, params, y)[0]
    assert (point[active] >= 1e-3).all(), float(point[active].min())
    # nearest is compared only where the two smallest d differ by more than NEAR_GAP: at most 1 % of the entries are left out
    close = ~clear_nearest(r["d"])
    assert close.mean() <= 0.01 and np.array_equal(masked_cotangent(name) == 0, close | (d["gd"] == 0))
    # E > 0 on some frames and E == 0 on some (the far frames exactly)
    E = r["E"]
    assert (E > 0).any() and (E[d["far"]] == 0).all() and d["far"].sum() == 8 and not r["grad"][d["far"]].any() and not r["wrench"][d["far"]].any()
    assert np.isfinite(r["grad"]).all() and np.abs(r["grad"]).max() > 0 and np.abs(r["wrench"]).max() > 0
    used = sorted(set(r["nearest"].reshape(-1).tolist()))
    print(f"{name}: {r['dist'].shape[1]} spheres x {len(kinds)} primitives; active share {active.mean():.4f}, frames with E > 0 {(E > 0).mean():.3f}, "
          f"box-interior active entries {int(interior.sum())} (smallest tie gap {tie[..., box][interior].min() if interior.any() else float('nan'):.2e} m), "
          f"entries with the two nearest within {NEAR_GAP:g} m {close.mean():.4f}, nearest primitives used {used}, max E {E.max():.3e}, "
          f"max |grad| {np.abs(r['grad']).max():.3e}, max |wrench| {np.abs(r['wrench']).max():.3e}")
    assert len(used) >= 3

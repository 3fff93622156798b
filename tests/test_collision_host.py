"""CPU tests of the sphere-pair self-collision's interface (include/dexr_spheres.h, dex_retargeting_amd/collision.py): the export
list against the header, dexr_sphere_model_create's validation (every malformed input DEXR_ERR_INVALID before a device is looked
for), the argument rules of the torch front (every one a ValueError before any device call), default_pairs against a brute-force
path count, the yardstick tests/collision_reference.py against central differences of its own float64 distances and energy, and
the behaviour of the yardstick on the inputs of tests/test_gpu_collision.py, so that the inputs are proven before a GPU sees them.

INPUTS (collision_inputs; shared with the GPU tests).  The eight robots of test_gpu_link_poses.ROBOTS, every link of each (at most
39), B = 33 (two full sixteen-frame blocks and a ragged one), q uniform inside the limits from default_rng(Q_SEED = 11),
float32-representable.  margin = 0.010.
  "origins"  one sphere of radius 0.010 at every link origin.
  "offset"   two spheres of radius 0.010 per link: one at the origin, one at an offset of 5 .. 15 mm in a random direction from
             default_rng(OFFSET_SEED), so that R_l center counts.  OFFSET_SEED = 26 is the first of the seeds 0, 1, 2, ... with which
             the conditions below hold on all seven robots (with each of 0 .. 25 some robot has a frame with two centres
             nearer than 3 mm).
Pairs: every i < j whose centres are more than 4 mm apart at the home configuration (q = 0).  In the "offset" set that includes the
two spheres of one link (5 .. 15 mm apart, always penetrating, constant distance), on the gripper too: the gripper's exact zeros
are asserted on "origins", no condition is set on its "offset" set.

CONDITIONS asserted on the reference alone (float64), per set: on the six hands and the arm-and-hand robot at least 0.5 % of the
(frame, pair) entries are active (d < margin), at least 90 % of the frames have an active pair, and the smallest centre distance is
at least 3 mm (no pair sits near the singular point of the normal); the gripper's "origins" energy and gradient are exact zeros.

CENTRAL DIFFERENCES (float64, step H = 1e-6 rad or m).  For a smooth f the central difference errs by H^2 |f'''| / 6 + eps |f| / H.
Distances: |d| <= 0.5 m, |d'''| of order |d'| <= 0.5 m/rad: 1e-13 + 1e-10; gate 1e-8.  Energy: per pair w h^2 <= 1e-3 and
2 h |d'| <= 0.03, a few dozen active pairs: 1e-10 again -- but E is only C1: a pair within H |d'| of the margin adds H times the jump
2 w d'^2 <= 0.5 of its second derivative, 5e-7 at the very worst; gate 1e-6 (the gradients themselves reach 1e-2 .. 1e-1)."""
import functools
import os
import re

import numpy as np
import pytest

import collision_reference as cref
import test_gpu_link_poses as glp
from testutil import REPO
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd import pose_tables as pt
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from oracle import cases
from oracle.kin import OracleRobot
from test_jacobian_host import SUBSET_CFG

RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
HEADER = os.path.join(REPO, "include", "dexr_spheres.h")
ROBOTS = glp.ROBOTS
ARM, GRIPPER = "arm_shadow_hand_right", "panda_gripper_glb"
SETS = ("origins", "offset")
B, Q_SEED, OFFSET_SEED, MARGIN, RADIUS = 33, 11, 26, 0.010, 0.010
INVALID, HIP = -1, -2


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def robot_of(name):
    return RobotWrapper(ROBOTS[name]), OracleRobot(ROBOTS[name])


@functools.lru_cache(maxsize=None)
def collision_inputs(name, kind):
    """dict: orc, links (table links), sset (a SphereSet with explicit pairs), rows, centers, radii, pairs, q (33, dof), margin;
    arrays read-only."""
    assert kind in SETS
    robot, orc = robot_of(name)
    links = [f.name for f in robot.kin.frames]
    assert len(links) == len(set(links)) <= 64 and robot.kin.dof_joint_names == orc.dof_joint_names
    L = len(links)
    if kind == "origins":
        names, centers = list(links), np.zeros((L, 3))
    else:
        rng = np.random.default_rng(OFFSET_SEED)
        u = rng.standard_normal((L, 3))
        off = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.005, 0.015, (L, 1))
        names = [n for n in links for _ in range(2)]
        centers = _r32(np.stack([np.zeros((L, 3)), off], 1).reshape(2 * L, 3))
    radii = np.full(len(names), RADIUS)
    rows = np.array([links.index(n) for n in names])
    home = cref.centres(orc, np.zeros((1, orc.dof)), links, rows, centers)[0][0]
    S = len(names)
    pairs = np.array([(i, j) for i in range(S) for j in range(i + 1, S) if np.linalg.norm(home[i] - home[j]) > 0.004], np.int32)
    lim = orc.joint_limits
    q = _r32(np.random.default_rng(Q_SEED).uniform(lim[:, 0], lim[:, 1], (B, orc.dof)))
    q = np.clip(q, _r32(lim[:, 0]), _r32(lim[:, 1]))
    sset = collision.SphereSet(names, centers, radii, pairs)
    assert sset.table_links == tuple(links) and np.array_equal(sset.sphere_rows, rows)
    d = dict(orc=orc, links=links, sset=sset, rows=rows, centers=centers, radii=radii, pairs=pairs, q=q, margin=MARGIN)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _geo(d):
    return d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"], d["pairs"]


@functools.lru_cache(maxsize=None)
def reference(name, kind, dtype=np.float64):
    """the yardstick on collision_inputs(name, kind), computed once and shared, read-only: dict dist, centers, E, grad, h, and
    for the seeded cotangent `gd` (B, P) the VJP `vjp`."""
    d = collision_inputs(name, kind)
    orc, q, links, rows, centers, radii, pairs = _geo(d)
    q = q.astype(dtype)
    dist, c, _ = cref.distances(orc, q, links, rows, centers, radii, pairs, dtype)
    dd = cref.distance_jacobian(orc, q, links, rows, centers, radii, pairs, dtype)
    gd = _r32(np.random.default_rng(17).standard_normal(dist.shape))
    h = np.maximum(dtype(0), dtype(d["margin"]) - dist)
    out = dict(dist=dist, centers=c, gd=gd, vjp=np.einsum("bp,bpc->bc", gd.astype(dtype), dd), h=h, E=(h * h).sum(-1),
               grad=np.einsum("bp,bpc->bc", dtype(-2) * h, dd))
    for v in out.values():
        assert v.dtype == dtype or v is gd
        v.setflags(write=False)
    return out


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    assert declared == set(_lib.SPHERE_EXPORTS) and len(_lib.SPHERE_EXPORTS) == 9 and len(set(_lib.SPHERE_EXPORTS)) == 9
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS, _lib.WRENCH_EXPORTS, _lib.IK_EXPORTS, _lib.IK_SOLVE_EXPORTS):
        assert not set(_lib.SPHERE_EXPORTS) & set(other)
    lib = _lib.load()
    for name in _lib.SPHERE_EXPORTS:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in ("dexr_ik_solve.h", "dexr_ik.h", "dexr_wrench.h", "dexr_jacobian.h", "dexr_pose.h", "dexr.h"):
        assert not _declared(os.path.join(REPO, "include", h)) & declared
    text = open(HEADER).read()
    assert int(re.search(r"#define DEXR_SPHERE_MAX (\d+)", text).group(1)) == _lib.SPHERE_MAX == 128
    assert int(re.search(r"#define DEXR_SPHERE_MAXPAIR (\d+)", text).group(1)) == _lib.SPHERE_MAXPAIR == 8192
    from dex_retargeting_amd import autograd as ag

    for n in ("sphere_distances", "self_collision_penalty", "robot_sphere_distances", "robot_self_collision_penalty"):
        assert n in collision.__all__ and n in ag.__all__
    assert "SphereSet" in collision.__all__ and "default_pairs" in collision.__all__
    src = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_spheres.hpp")).read()
    assert "getenv" not in src and "atomic" not in src and "asm" not in src.replace("__restrict__", "")


def _create(blob, link, center, radius, pair, n_sphere=None, n_pair=None):
    lib = _lib.load()
    link, center, radius, pair = (None if a is None else np.ascontiguousarray(a, t) for a, t in
                                  ((link, np.int32), (center, np.float64), (radius, np.float64), (pair, np.int32)))
    h = _lib.C.c_void_p()
    p = lambda a, t: None if a is None else a.ctypes.data_as(_lib.C.POINTER(t))  # noqa: E731
    buf = _lib.C.create_string_buffer(blob, len(blob))
    rc = lib.dexr_sphere_model_create(buf, len(blob), len(link) if n_sphere is None else n_sphere, p(link, _lib.C.c_int32),
                                      p(center, _lib.C.c_double), p(radius, _lib.C.c_double), len(pair) if n_pair is None else n_pair,
                                      p(pair, _lib.C.c_int32), _lib.C.byref(h))
    if rc == 0:
        lib.dexr_sphere_model_destroy(h)
    else:
        assert not h.value
    return rc, lib.dexr_last_error().decode()


def test_sphere_model_create_validates_before_it_looks_for_a_device():
    robot, _ = robot_of("allegro_hand_right")
    links = [f.name for f in robot.kin.frames][:5]
    blob = pt.compile_poses(robot.kin, links)
    link, cen, rad, pair = [0, 1, 2, 4, 4], np.zeros((5, 3)), np.full(5, 0.01), [[0, 1], [1, 2], [3, 4], [0, 1]]

    def invalid(word, **kw):
        a = dict(blob=blob, link=link, center=cen, radius=rad, pair=pair)
        a.update(kw)
        rc, msg = _create(**a)
        assert rc == INVALID and word in msg, (rc, msg, word)

    invalid("magic", blob=bytes([blob[0] ^ 0xFF]) + blob[1:])
    invalid("truncated", blob=blob[:-8])
    invalid("truncated", blob=blob[:10])
    invalid("size", blob=blob + b"\0" * 8)
    invalid("spheres", n_sphere=0)
    invalid("spheres", n_sphere=129, link=[0] * 129, center=np.zeros((129, 3)), radius=np.zeros(129))
    invalid("pairs", n_pair=0)
    invalid("pairs", pair=[[0, 1]] * 8193)
    invalid("link row", link=[0, 1, 2, 4, 5])
    invalid("link row", link=[-1, 1, 2, 4, 4])
    invalid("sphere index", pair=[[0, 5]])
    invalid("sphere index", pair=[[-1, 2]])
    invalid("with itself", pair=[[0, 1], [2, 2]])
    for bad in (np.nan, np.inf, -np.inf):
        c = cen.copy()
        c[3, 1] = bad
        invalid("centre", center=c)
    for bad in (np.nan, np.inf, -1e-9, -1.0):
        r = rad.copy()
        r[2] = bad
        invalid("radius", radius=r)
    for k in ("link", "center", "radius", "pair"):
        invalid("null", **{k: None}, n_sphere=5, n_pair=4)
    # the blob comes first: a bad blob AND bad spheres reports the blob
    invalid("magic", blob=bytes([blob[0] ^ 0xFF]) + blob[1:], n_sphere=0)
    # the limits themselves are fine: 128 spheres and every pair (8128), a radius of zero, a duplicated pair
    full = [[i, j] for i in range(128) for j in range(i + 1, 128)]
    assert len(full) == 8128
    want = 0 if _lib.load().dexr_device_count() > 0 else HIP  # a well-formed input needs a device
    for a in (dict(blob=blob, link=link, center=cen, radius=rad * 0, pair=pair),
              dict(blob=blob, link=[i % 5 for i in range(128)], center=np.zeros((128, 3)), radius=np.zeros(128), pair=full)):
        rc, msg = _create(**a)
        assert rc == want, (rc, msg)
    if want == HIP:
        with pytest.raises(_lib.DexrError, match="libdexr error -2"):
            _lib.SphereModel(blob, link, cen, rad, pair)
    with pytest.raises(ValueError, match="one row per sphere"):
        _lib.SphereModel(blob, link, cen[:4], rad, pair)


# ---- 2. SphereSet and the argument rules of the torch front -------------------------------------------------------------------------
def test_sphere_set_is_plain_hashable_data():
    a = collision.SphereSet(["a", "b", "a"], np.zeros((3, 3)), [0.01, 0.02, 0.0], [[0, 1], [2, 1]])
    b = collision.SphereSet(("a", "b", "a"), [[0, 0, 0]] * 3, np.array([0.01, 0.02, 0.0]), np.array([[0, 1], [2, 1]]))
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a.links == ("a", "b", "a") and a.table_links == ("a", "b") and a.sphere_rows.tolist() == [0, 1, 0] and a.n_sphere == 3
    assert a != collision.SphereSet(["a", "b", "a"], np.zeros((3, 3)), [0.01, 0.02, 0.0]) and a != collision.SphereSet(["a", "b", "a"], np.zeros((3, 3)), [0.01, 0.02, 0.001], [[0, 1], [2, 1]])
    with pytest.raises(ValueError):
        a.centers[0, 0] = 1.0
    ok = dict(links=["a", "b"], centers=np.zeros((2, 3)), radii=[0.01, 0.01])
    for bad, word in ((dict(links="ab"), "links"), (dict(links=[]), "links"), (dict(links=[1, 2]), "links"), (dict(centers=np.zeros((3, 3))), "shape"),
                      (dict(centers=np.zeros((2, 2))), "shape"), (dict(radii=[0.01]), "shape"), (dict(radii=[0.01, -1e-9]), "radii"),
                      (dict(radii=[0.01, np.nan]), "radii"), (dict(centers=[[0, 0, np.inf], [0, 0, 0]]), "finite"),
                      (dict(pairs=[[0, 0]]), "different"), (dict(pairs=[[0, 2]]), "index"), (dict(pairs=[[-1, 1]]), "index"),
                      (dict(pairs=[0, 1]), "shape"), (dict(pairs=np.zeros((0, 2), int)), "pairs"), (dict(pairs=[[0, 1]] * 8193), "pairs")):
        with pytest.raises(ValueError, match=word):
            collision.SphereSet(**dict(ok, **bad))
    with pytest.raises(ValueError, match="128"):
        collision.SphereSet(["a"] * 129, np.zeros((129, 3)), np.zeros(129))
    with pytest.raises(ValueError, match="64 distinct"):
        collision.SphereSet([f"l{i}" for i in range(65)], np.zeros((65, 3)), np.zeros(65))
    assert collision.SphereSet([f"l{i % 64}" for i in range(128)], np.zeros((128, 3)), np.zeros(128)).n_sphere == 128


def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    touched = []
    for cls in (_lib.SphereModel, _lib.PoseModel):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("distances_dev", "distances_vjp_dev", "penalty_dev"):
        monkeypatch.setattr(_lib.SphereModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "base_link"]
    sset = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    n_pair = len(collision.default_pairs(opt.robot, sset))
    assert n_pair == 6
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    w = torch.ones((n_pair,), dtype=torch.float32)
    fronts = [lambda q, s, margin=0.01, pair_weight=None, **k: collision.self_collision_penalty(opt, q, s, margin, pair_weight, **k),
              lambda q, s, margin=0.01, pair_weight=None, **k: ag.self_collision_penalty(opt, q, s, margin, pair_weight, **k),
              lambda q, s, margin=0.01, pair_weight=None, **k: collision.robot_self_collision_penalty(opt.robot, q, s, margin, pair_weight, **k),
              lambda q, s, margin=0.01, pair_weight=None, **k: ag.robot_self_collision_penalty(opt.robot, q, s, margin, pair_weight, **k)]
    dists = [lambda q, s, **k: collision.sphere_distances(opt, q, s, **k), lambda q, s, **k: ag.sphere_distances(opt, q, s, **k),
             lambda q, s, **k: collision.robot_sphere_distances(opt.robot, q, s, **k), lambda q, s, **k: ag.robot_sphere_distances(opt.robot, q, s, **k)]

    def raises(fns, match=None, q=good, s=sset, **kw):
        for f in fns:
            with pytest.raises(ValueError, match=match):
                f(q, s, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises(fronts + dists, "CUDA")
    raises(fronts, "CUDA", pair_weight=w, margin=0)
    raises(fronts, "CUDA", margin=1)  # Python ints are numbers too
    raises(dists[::2], "CUDA", centers=True)
    # dtype, shape, type of q
    raises(fronts + dists, "float32", q=good.double())
    for bad in (good[:, :15], good.reshape(-1), good[:, :, None]):
        raises(fronts + dists, "shape", q=bad)
    raises(fronts + dists, "torch tensor", q=good.numpy())
    # the sphere set: not one, an unknown link, no pair left by default_pairs
    raises(fronts + dists, "SphereSet", s=tips)
    raises(fronts + dists, "is not a link name", s=collision.SphereSet(["link_15.0_tip", "no_such_link"], np.zeros((2, 3)), [0.01, 0.01]))
    raises(fronts + dists, "0 pairs", s=collision.SphereSet(["link_15.0_tip", "link_15.0"], np.zeros((2, 3)), [0.01, 0.01]))
    # margin: a finite Python float >= 0
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.01), None, "0.01", True):
        raises(fronts, "margin", margin=bad)
    # pair_weight: a float32 tensor of one weight per pair
    raises(fronts, "float32", pair_weight=w.double())
    raises(fronts, "torch tensor", pair_weight=w.numpy())
    for bad in (w[:5], w[None], torch.ones((n_pair, 1)), torch.ones(n_pair + 1)):
        raises(fronts, "shape", pair_weight=bad)
    # fixed_qpos: one too many, one missing, one of the wrong width
    raises(fronts[:2] + dists[:2], "fixed_qpos", fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    assert len(sub.idx_pin2fixed) == 6
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    for fq, word in ((None, "fixed_qpos"), (torch.zeros((4, 5), dtype=torch.float32), "fixed_qpos"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                     (torch.zeros((4, 6), dtype=torch.float32), "CUDA")):
        for f in (collision.sphere_distances, ag.sphere_distances):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sset, fixed_qpos=fq)
        for f in (collision.self_collision_penalty, ag.self_collision_penalty):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sset, 0.01, fixed_qpos=fq)
    with pytest.raises(ValueError, match="skip_joint_distance"):
        collision.default_pairs(opt.robot, sset, -1)
    assert touched == []


def test_sphere_models_are_cached_per_set_and_dropped_with_the_adaptor(monkeypatch):
    made = []
    monkeypatch.setattr(_lib.SphereModel, "__init__", lambda self, blob, rows, cen, rad, pairs: made.append((len(rows), len(pairs))))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip"]
    a = collision.SphereSet(tips, np.zeros((3, 3)), np.full(3, 0.01))
    same = collision.SphereSet(list(tips), np.zeros((3, 3)), [0.01, 0.01, 0.01])
    other = collision.SphereSet(tips, np.zeros((3, 3)), np.full(3, 0.02), [(0, 1)])
    m = opt.sphere_model(a)
    assert opt.sphere_model(same) is m and opt.sphere_model(other) is not m and made == [(3, 3), (3, 1)]
    assert opt.robot.sphere_model(a) is opt.robot.sphere_model(same) and opt.robot.sphere_model(a) is not m and len(made) == 3
    opt.set_kinematic_adaptor(opt.adaptor)
    assert opt.sphere_model(a) is not m and len(made) == 4


# ---- 3. default_pairs against a brute-force path count ------------------------------------------------------------------------------
def _path_joint_count(urdf, a, b):
    """movable joints on the tree path between links a and b: breadth-first search over the URDF's joints as an undirected graph."""
    nbr = {}
    for j in urdf.joints:
        w = 0 if j.type == "fixed" else 1
        nbr.setdefault(j.parent, []).append((j.child, w))
        nbr.setdefault(j.child, []).append((j.parent, w))
    seen, todo = {a: 0}, [a]
    while todo:
        u = todo.pop(0)
        for v, w in nbr.get(u, []):
            if v not in seen:
                seen[v] = seen[u] + w
                todo.append(v)
    return seen[b]


@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_default_pairs_equal_a_brute_force_path_count(name):
    assert len(ROBOTS) == 8
    robot, _ = robot_of(name)
    links = [f.name for f in robot.kin.frames]
    names = links + links[:3]  # three links carry two spheres
    sset = collision.SphereSet(names, np.zeros((len(names), 3)), np.zeros(len(names)))
    count = {(a, b): _path_joint_count(robot.kin.urdf, a, b) for a in links for b in links}
    for skip in (0, 1, 2):
        want = [(i, j) for i in range(len(names)) for j in range(i + 1, len(names)) if names[i] != names[j] and count[names[i], names[j]] > skip]
        got = collision.default_pairs(robot, sset, skip)
        assert got.dtype == np.int32 and got.shape == (len(want), 2) and [tuple(p) for p in got.tolist()] == want, (name, skip)
    print(f"{name}: {len(names)} spheres, default pairs {len(collision.default_pairs(robot, sset))} of {len(names) * (len(names) - 1) // 2}")


# ---- 4. the yardstick against central differences of its own distances and energy ---------------------------------------------------
H, GATE_D, GATE_E = 1e-6, 1e-8, 1e-6


@pytest.mark.parametrize("name,kind", [("allegro_hand_right", "origins"), ("shadow_hand_right", "offset")])
def test_reference_gradients_equal_central_differences(name, kind):
    d = collision_inputs(name, kind)
    orc, q, links, rows, centers, radii, pairs = _geo(d)
    q = q[:4]
    w = _r32(np.random.default_rng(3).uniform(0.5, 2.0, len(pairs)))
    dd = cref.distance_jacobian(orc, q, links, rows, centers, radii, pairs)
    E, g, h = cref.penalty(orc, q, links, rows, centers, radii, pairs, d["margin"], w)
    assert (h > 0).any() and dd.shape == (4, len(pairs), orc.dof)
    worst_d = worst_e = 0.0
    for c in range(orc.dof):
        qp, qm = q.copy(), q.copy()
        qp[:, c] += H
        qm[:, c] -= H
        dp, dm = (cref.distances(orc, x, links, rows, centers, radii, pairs)[0] for x in (qp, qm))
        ep, em = (cref.penalty(orc, x, links, rows, centers, radii, pairs, d["margin"], w)[0] for x in (qp, qm))
        worst_d = max(worst_d, float(np.abs((dp - dm) / (2 * H) - dd[:, :, c]).max()))
        worst_e = max(worst_e, float(np.abs((ep - em) / (2 * H) - g[:, c]).max()))
    print(f"{name} {kind}: max |dd/dq - central difference| = {worst_d:.3e} (gate {GATE_D:.0e}), max |dE/dq - central difference| = "
          f"{worst_e:.3e} (gate {GATE_E:.0e}), max |dE/dq| = {np.abs(g).max():.3e}")
    assert worst_d <= GATE_D and worst_e <= GATE_E
    # the VJP is the contraction of the same matrix
    gd = np.random.default_rng(4).standard_normal(dd.shape[:2])
    assert np.allclose(cref.distances_vjp(orc, q, links, rows, centers, radii, pairs, gd), np.einsum("bp,bpc->bc", gd, dd), rtol=0, atol=1e-14)


# ---- 5. the inputs of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_gpu_inputs_have_active_pairs_and_stay_away_from_coincidence(name, kind):
    d = collision_inputs(name, kind)
    r = reference(name, kind)
    dist, E, grad = r["dist"], r["E"], r["grad"]
    assert d["q"].shape == (B, d["orc"].dof) and np.array_equal(d["q"], _r32(d["q"])) and np.array_equal(d["centers"], _r32(d["centers"]))
    assert 1 <= len(d["pairs"]) <= _lib.SPHERE_MAXPAIR and d["sset"].n_sphere == (1 if kind == "origins" else 2) * len(d["links"])
    active = dist < d["margin"]
    centre = dist + 2 * RADIUS
    print(f"{name} {kind}: {d['sset'].n_sphere} spheres, {len(d['pairs'])} pairs; active share {active.mean():.4f}, penetrating share "
          f"{(dist < 0).mean():.4f}, frames with an active pair {active.any(1).mean():.3f}, smallest centre distance {centre.min() * 1e3:.2f} mm, "
          f"max E {E.max():.3e}, max |grad| {np.abs(grad).max():.3e}")
    assert np.isfinite(dist).all() and np.isfinite(grad).all()
    if name == GRIPPER:
        if kind == "origins":
            assert not active.any() and not E.any() and not grad.any()
        return  # (its "offset" set has active pairs, the off-origin spheres of the fingers among them: no condition is set on it)
    assert active.mean() >= 0.005 and active.any(1).mean() >= 0.9 and centre.min() >= 0.003, (name, kind)
    assert (E > 0).any() and np.abs(grad).max() > 0
    if kind == "offset":  # the second sphere of a link is off its origin: R_l center counts
        assert np.abs(r["centers"][:, 1::2] - r["centers"][:, 0::2]).max() > 0.004

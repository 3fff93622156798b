"""CPU tests of the pose tables (include/dexr_pose.h, dex_retargeting_amd/pose_tables.py) through the numpy interpreter
tests/pose_interp.py: full link poses against the reference's own forward kinematics (tests/golden/fk_golden.npz), the
optimizer-order source map against the oracle, the closed-form VJP against central differences of the oracle, blob
validation of dexr_pose_model_create, the export list, and the source hash that keys the headline PMC summary."""
import glob
import json
import os
import re
import tempfile

import numpy as np
import pytest

import pose_interp as pi
from testutil import REPO
from dex_retargeting_amd import _build, _lib, pose_tables as pt
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from dex_retargeting_amd.urdf import KinematicModel, parse_urdf
from oracle import cases
from oracle.kin import OracleRobot

RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
FK = np.load(os.path.join(REPO, "tests", "golden", "fk_golden.npz"))
FK_KEYS = sorted(k[: -len("__links")] for k in FK.files if k.endswith("__links"))
ALL_CONFIGS = sorted(os.path.relpath(p, cases.CONFIG_DIR) for p in glob.glob(os.path.join(cases.CONFIG_DIR, "*", "*.yml")))


def _urdf_of(key):
    free = key.endswith("__free")
    base = key[: -len("__free")] if free else key
    if base.startswith("testurdf__"):
        return os.path.join(REPO, "tests", "urdf", base[len("testurdf__"):] + ".urdf"), free
    return os.path.join(cases.URDF_DIR, base.replace("__", "/") + ".urdf"), free


def _q_by_name(dof_names, key, c):
    """golden configuration c -> full q in `dof_names` order, mimic joints filled the way the reference's FK fills them
    (as tests/test_reference_pins.py::_q_by_name)."""
    val = dict(zip(FK[key + "__joints"].tolist(), FK[key + "__cfg"][c].tolist()))
    mims = FK[key + "__mimic"].tolist()
    if mims != [""]:
        for n, s, a, b in zip(mims, FK[key + "__mimic_src"].tolist(), FK[key + "__mimic_mult"], FK[key + "__mimic_off"]):
            val[n] = val[s] * float(a) + float(b)
    return np.array([val[n] for n in dof_names])


def _chunks(names, n=64):
    return [names[c:c + n] for c in range(0, len(names), n)]


# ---- 1. full poses of every link of every fixture against the reference's FK ---------------------------------------------
def test_fk_golden_has_every_fixture():
    urdfs = glob.glob(os.path.join(cases.URDF_DIR, "*", "*.urdf"))
    assert len(urdfs) >= 13 and len(FK_KEYS) >= 2 * len(urdfs) + 1


@pytest.mark.parametrize("key", FK_KEYS)
def test_interpreted_tables_equal_reference_poses(key):
    path, free = _urdf_of(key)
    km = KinematicModel(parse_urdf(path, add_dummy_free_joints=free))
    links = FK[key + "__links"].tolist()
    n_cfg = FK[key + "__cfg"].shape[0]
    assert n_cfg == 4
    q = np.stack([_q_by_name(km.dof_joint_names, key, c) for c in range(n_cfg)])
    T = FK[key + "__T"]  # (cfg, link, 4, 4)
    worst = 0.0
    for c0, names in zip(range(0, len(links), 64), _chunks(links)):
        blob = pt.compile_poses(km, names)
        tab = pi.parse(blob)
        assert int(tab["h"]["n_joint"]) <= 64 and int(tab["h"]["n_slot"]) <= 6
        pos, rot = pi.poses(tab, q)
        want = T[:, c0:c0 + len(names)]
        worst = max(worst, np.abs(rot - want[:, :, :3, :3]).max(), np.abs(pos - want[:, :, :3, 3]).max())
        # the one-running-transform walk with numbered fork slots (what the kernel does) visits the same joint frames
        Rs, ps, _ = pi._joint_frames(tab, pi.joint_values(tab, q))
        for k, (R, p) in enumerate(pi.walk_with_slots(tab, q)):
            assert np.array_equal(R, Rs[k]) and np.array_equal(p, ps[k]), (key, k)
    print(f"{key}: max |pose - reference| = {worst:.3e}")
    assert worst <= 1e-12, key


def test_table_layout_matches_header():
    h = open(os.path.join(REPO, "include", "dexr_pose.h")).read()
    assert int(re.search(r"#define DEXR_POSE_MAGIC (0x[0-9a-fA-F]+)u", h).group(1), 16) == pt.MAGIC == 0x53505844
    for name, val in (("VERSION", pt.VERSION), ("MAXJ", pt.MAXJ), ("MAXL", pt.MAXL), ("MAXSLOT", pt.MAXSLOT), ("MAXIN", pt.MAXIN)):
        assert int(re.search(rf"#define DEXR_POSE_{name} (\d+)", h).group(1)) == val
    assert (pt.HEADER_DTYPE.itemsize, pt.JOINT_DTYPE.itemsize, pt.LINK_DTYPE.itemsize) == (32, 176, 104)
    assert (pi.HEADER, pi.JOINT, pi.LINK) == (pt.HEADER_DTYPE, pt.JOINT_DTYPE, pt.LINK_DTYPE)


def test_nested_forks_reuse_slots_and_more_than_64_links_are_refused():
    xml = ['<robot name="tree"><link name="l0"/>']
    joints = [("a0", "l0", "l1"), ("b0", "l1", "l2"), ("c0", "l2", "l3"), ("c1", "l2", "l4"), ("b1", "l1", "l5"),
              ("d0", "l5", "l6"), ("e0", "l0", "l7"), ("d1", "l5", "l8")]
    for i in range(1, 9):
        xml.append(f'<link name="l{i}"/>')
    for n, (name, p, c) in enumerate(joints):
        typ = "prismatic" if name == "d0" else "revolute"
        xml.append(f'<joint name="{name}" type="{typ}"><parent link="{p}"/><child link="{c}"/>'
                   f'<origin xyz="0.0{n+1} 0.02 0.1" rpy="0.{n} 0.2 -0.{n}"/><axis xyz="{(n%3==0)*1} {(n%3==1)*1} {(n%3==2)*1}"/>'
                   f'<limit lower="-1" upper="1"/></joint>')
    xml.append("</robot>")
    with tempfile.NamedTemporaryFile("w", suffix=".urdf", delete=False) as f:
        f.write("".join(xml))
    try:
        km = KinematicModel(parse_urdf(f.name))
        orc = OracleRobot(f.name)
    finally:
        os.unlink(f.name)
    links = [f"l{i}" for i in (6, 0, 3, 7, 4, 1, 5, 2, 3, 8)]  # any order, a repeat, the base link
    tab = pi.parse(pt.compile_poses(km, links))
    # a0 forks into two forks of equal size: the first runs while a0's transform is still needed, the last reuses its slot
    assert int(tab["h"]["n_slot"]) == 2 and (tab["joints"]["restore"] == pt.ROOT).sum() == 2
    q = np.random.default_rng(0).uniform(-1, 1, (5, km.dof))
    pos, rot = pi.poses(tab, q)
    R, p = orc.link_poses(q, links)
    assert np.abs(pos - p).max() < 1e-13 and np.abs(rot - R).max() < 1e-13
    Rs, ps, _ = pi._joint_frames(tab, pi.joint_values(tab, q))
    for k, (Rk, pk) in enumerate(pi.walk_with_slots(tab, q)):
        assert np.array_equal(Rk, Rs[k]) and np.array_equal(pk, ps[k])
    # only the joints the links depend on are in the table
    assert int(pi.parse(pt.compile_poses(km, ["l7"]))["h"]["n_joint"]) == 1
    assert int(pi.parse(pt.compile_poses(km, ["l0"]))["h"]["n_joint"]) == 0
    with pytest.raises(ValueError, match="1..64 links"):
        pt.compile_poses(km, ["l1"] * 65)
    with pytest.raises(ValueError, match="1..64 links"):
        pt.compile_poses(km, [])
    with pytest.raises(ValueError, match="is not a link name"):
        pt.compile_poses(km, ["nope"])


# ---- 2. optimizer-order source map on every shipped config ---------------------------------------------------------------
def _optimizer(rel):
    cfg = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel))
    return cfg._build_optimizer()


def _seeded_x(prob, B, seed):
    rng = np.random.default_rng(seed)
    lim = prob.robot.joint_limits
    x = rng.uniform(lim[prob.idx_pin2target, 0], lim[prob.idx_pin2target, 1], (B, len(prob.idx_pin2target)))
    fixed = rng.uniform(lim[prob.idx_pin2fixed, 0], lim[prob.idx_pin2fixed, 1], (B, len(prob.idx_pin2fixed)))
    return x, fixed


def test_shipped_configs_include_mimic_fixed_and_free_joint_cases():
    seen = {"mimic": set(), "fixed": 0, "free": 0}
    for rel in ALL_CONFIGS:
        prob = cases.problem_from_config(rel)
        if len(prob.idx_pin2mimic):
            seen["mimic"].add(os.path.basename(rel).split("_hand")[0])
        seen["fixed"] += len(prob.idx_pin2fixed) > 0
        seen["free"] += bool(prob.cfg.get("add_dummy_free_joint", False))
    assert {"ability", "inspire", "schunk_svh"} <= seen["mimic"] and seen["free"] >= 13 and len(ALL_CONFIGS) == 39


@pytest.mark.parametrize("rel", ALL_CONFIGS)
def test_optimizer_order_map_equals_oracle(rel):
    opt = _optimizer(rel)
    prob = cases.problem_from_config(rel)
    assert list(opt.idx_pin2target) == list(prob.idx_pin2target) and list(opt.idx_pin2fixed) == list(prob.idx_pin2fixed)
    links = [f.name for f in opt.robot.kin.frames]
    x, fixed = _seeded_x(prob, 4, 11)
    q_full = prob.full_qpos(x, fixed)
    if len(prob.idx_pin2mimic):
        assert np.array_equal(q_full, prob.robot.mimic_forward(q_full))
    sm = opt.pose_source_map()
    assert (sm.n_in, sm.n_fixed) == (opt.opt_dof, len(opt.idx_pin2fixed))
    worst = 0.0
    for names in _chunks(links):
        tab = pi.parse(pt.compile_poses(opt.robot.kin, names, sm))
        pos, rot = pi.poses(tab, x, fixed)
        R, p = prob.robot.link_poses(q_full, names)
        worst = max(worst, np.abs(pos - p).max(), np.abs(rot - R).max())
    print(f"{rel}: max |pose - oracle| = {worst:.3e}")
    assert worst <= 1e-12, rel


# ---- 3. the closed-form VJP against central differences of the oracle -----------------------------------------------------
def _fd_grad(f, x, h=1e-6):
    g = np.zeros_like(x)
    for c in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, c] += h
        xm[:, c] -= h
        g[:, c] = (f(xp) - f(xm)) / (2 * h)
    return g


VJP_ROBOTS = ["shadow_hand/shadow_hand_right.urdf", "schunk_hand/schunk_svh_hand_right.urdf", "panda_gripper/panda_gripper_glb.urdf"]


@pytest.mark.parametrize("free", [False, True])
@pytest.mark.parametrize("urdf", VJP_ROBOTS)
def test_interpreted_vjp_equals_central_differences_of_the_oracle(urdf, free):
    path = os.path.join(cases.URDF_DIR, urdf)
    km = KinematicModel(parse_urdf(path, add_dummy_free_joints=free))
    orc = OracleRobot(path, free)
    links = [f.name for f in km.frames][:64]
    tab = pi.parse(pt.compile_poses(km, links))
    rng = np.random.default_rng(3)
    lim = km.joint_limits
    q = rng.uniform(lim[:, 0], lim[:, 1], (3, km.dof))
    gp = rng.standard_normal((3, len(links), 3))
    gr = rng.standard_normal((3, len(links), 3, 3))
    for name, a, b in (("position-only", gp, None), ("rotation-only", None, gr), ("both", gp, gr)):
        def loss(qq):
            R, p = orc.link_poses(qq, links)
            return (0 if a is None else (p * a).sum((1, 2))) + (0 if b is None else (R * b).sum((1, 2, 3)))

        g = pi.vjp(tab, q, None, a, b)
        fd = _fd_grad(loss, q)
        err, scale = np.abs(g - fd).max(), max(1.0, np.abs(g).max())
        print(f"{urdf} free={free} {name}: max |g - fd| = {err:.3e} at max |g| = {np.abs(g).max():.3f}")
        assert err <= 1e-7 * scale, (urdf, free, name)


@pytest.mark.parametrize("rel", ["offline/schunk_svh_hand_right.yml", "teleop/ability_hand_right.yml",
                                 "teleop/inspire_hand_right_dexpilot.yml", "offline/shadow_hand_right.yml"])
def test_interpreted_vjp_folds_mimic_joints_like_the_chain_rule(rel):
    opt = _optimizer(rel)
    prob = cases.problem_from_config(rel)
    links = [f.name for f in opt.robot.kin.frames][:64]
    x, fixed = _seeded_x(prob, 3, 5)
    tab = pi.parse(pt.compile_poses(opt.robot.kin, links, opt.pose_source_map()))
    rng = np.random.default_rng(4)
    gp = rng.standard_normal((3, len(links), 3))
    gr = rng.standard_normal((3, len(links), 3, 3))

    def loss(xx):
        R, p = prob.robot.link_poses(prob.robot.mimic_forward(prob.full_qpos(xx, fixed)) if len(prob.idx_pin2mimic)
                                     else prob.full_qpos(xx, fixed), links)
        return (p * gp).sum((1, 2)) + (R * gr).sum((1, 2, 3))

    g = pi.vjp(tab, x, fixed, gp, gr)
    fd = _fd_grad(loss, x)
    assert np.abs(g - fd).max() <= 1e-7 * max(1.0, np.abs(g).max()), rel
    # the same through the robot-order table and the chain rule of q_full(x): target columns + mult x mimic columns
    g_full = pi.vjp(pi.parse(pt.compile_poses(opt.robot.kin, links)), prob.full_qpos(x, fixed), None, gp, gr)
    want = g_full[:, prob.idx_pin2target].copy()
    for m, s, mult in zip(prob.idx_pin2mimic, prob.idx_pin2source, prob.multipliers):
        want[:, list(prob.idx_pin2target).index(s)] += mult * g_full[:, m]
    assert np.abs(g - want).max() <= 1e-12 * max(1.0, np.abs(g).max()), rel


# ---- 4. blob validation, exports --------------------------------------------------------------------------------------
def _shadow_blob():
    km = KinematicModel(parse_urdf(os.path.join(cases.URDF_DIR, "shadow_hand/shadow_hand_right.urdf")))
    return km, pt.compile_poses(km, ["thtip", "fftip", "mftip", "rftip", "lftip", "palm"])


def _patched(blob, section, index, field, value):
    h = np.frombuffer(blob[:32], pt.HEADER_DTYPE)[0]
    nj = int(h["n_joint"])
    b = bytearray(blob)
    if section == "header":
        rec = np.frombuffer(bytes(b[:32]), pt.HEADER_DTYPE).copy()
        rec[0][field] = value
        b[:32] = rec.tobytes()
    elif section == "joint":
        o = 32 + index * pt.JOINT_DTYPE.itemsize
        rec = np.frombuffer(bytes(b[o:o + pt.JOINT_DTYPE.itemsize]), pt.JOINT_DTYPE).copy()
        rec[0][field] = value
        b[o:o + pt.JOINT_DTYPE.itemsize] = rec.tobytes()
    else:
        o = 32 + nj * pt.JOINT_DTYPE.itemsize + index * pt.LINK_DTYPE.itemsize
        rec = np.frombuffer(bytes(b[o:o + pt.LINK_DTYPE.itemsize]), pt.LINK_DTYPE).copy()
        rec[0][field] = value
        b[o:o + pt.LINK_DTYPE.itemsize] = rec.tobytes()
    return bytes(b)


def test_pose_model_create_rejects_malformed_blobs():
    km, blob = _shadow_blob()
    nj = int(np.frombuffer(blob[:32], pt.HEADER_DTYPE)[0]["n_joint"])
    bad = [
        ("magic", bytes([blob[0] ^ 0xFF]) + blob[1:]),
        ("version", _patched(blob, "header", 0, "version", 9)),
        ("truncated", blob[:10]),
        ("truncated", blob[:-8]),
        ("truncated", blob[:32]),
        ("size", blob + b"\0" * 8),
        ("joints", _patched(blob, "header", 0, "n_joint", 65)),
        ("links", _patched(blob, "header", 0, "n_link", 65)),
        ("links", _patched(blob, "header", 0, "n_link", 0)),
        ("slots", _patched(blob, "header", 0, "n_slot", 9)),
        ("does not come before", _patched(blob, "joint", 2, "parent", 2)),
        ("does not come before", _patched(blob, "joint", 2, "parent", nj)),
        ("does not come before", _patched(blob, "joint", 0, "parent", -2)),
        ("column", _patched(blob, "joint", 1, "src_col", km.dof)),
        ("column", _patched(blob, "joint", 1, "src_col", -1)),
        ("column", _patched(blob, "joint", 1, "src_kind", pt.SRC_FIXED)),  # n_fixed == 0: no column is in range
        ("source kind", _patched(blob, "joint", 1, "src_kind", 3)),
        ("type", _patched(blob, "joint", 1, "type", 2)),
        ("slot", _patched(blob, "joint", nj - 1, "restore", 5)),
        ("slot", _patched(blob, "joint", 1, "save", 8)),
        ("link range", _patched(blob, "joint", nj - 1, "link_end", 99)),
        ("subtree", _patched(blob, "joint", 0, "sub_link_end", 1)),
        ("parent joint", _patched(blob, "link", 0, "parent", nj)),
        ("output row", _patched(blob, "link", 1, "out", 6)),
        ("output row", _patched(blob, "link", 1, "out", 0)),
    ]
    for what, b in bad:
        with pytest.raises(_lib.DexrError, match=what):
            _lib.PoseModel(b)
        assert "libdexr error -1" in str(pytest.raises(_lib.DexrError, _lib.PoseModel, b).value), what  # DEXR_ERR_INVALID


@pytest.mark.skipif(_lib.load().dexr_device_count() > 0, reason="only meaningful on a box without a GPU")
def test_pose_model_has_no_cpu_fallback():
    with pytest.raises(_lib.DexrError, match="libdexr error -2"):  # DEXR_ERR_HIP: a well-formed table needs a device
        _lib.PoseModel(_shadow_blob()[1])


def test_pose_exports_are_the_header_and_the_library_exports_them():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "dexr_pose.h")).read()
    declared = set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.POSE_EXPORTS) and len(_lib.POSE_EXPORTS) == 7
    for name in declared:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    assert not set(_lib.POSE_EXPORTS) & set(_lib.EXPORTS)
    src = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert "getenv" not in src and "atomic" not in src and "asm" not in src.replace("__restrict__", "")


# ---- 5. the headline workload's source hash still keys its committed PMC summary ---------------------------------------------
def test_headline_source_hash_is_unchanged():
    with open(os.path.join(REPO, "profiles", "pmc_allegro_vector.json")) as f:
        assert _build.source_hash("allegro_vector") == json.load(f)["source_sha16"]
    assert "dexr_pose.hip" not in _build._COMMON_SOURCES and not any("dexr_pose" in s for v in _build.KERNEL_SOURCES.values() for s in v)

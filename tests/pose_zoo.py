"""Synthetic robots at the limits of the pose-table format (include/dexr_pose.h), for tests/test_pose_zoo_host.py and
tests/test_gpu_pose_zoo.py: seeded URDF text written to a directory of the caller, the compiled table, the oracle of the same
file, seeded inputs, the chain-rule fold of a source map and the derived float32 gates.  Joints are revolute or prismatic
with limits, or fixed; every axis is a random unit vector, every origin has a rotation of 0.2 .. 1 rad about each axis and an
offset of 1 .. 3 cm along each; prismatic joints travel +-2 cm, revolute joints [-1.2, 0.9] rad unless a member says otherwise.

    chain64          64 joints in series, every fifth prismatic, a fixed-joint child link every eighth joint; 64 links
    chain64_turns    chain64 with revolute limits of +-20 rad
    binary64         a prismatic root joint, a complete binary tree of 62 joints below it, one more joint under a leaf
    binary64_slots8  the blob of binary64 with slot s renumbered 7 - s and n_slot = 8
    star40           40 joints on the base link, two links fixed to the base; shuffled links with a repeat and the base
    two_trees100_a   two heap-shaped trees of 50 joints off the base, robot order (n_in = 100): 50 links of the second tree
    two_trees100_b   32 links of each tree, closed under parents: 64 joints, columns on both sides of 64
    two_trees100_c   64 links that need more than 64 joints: the compiler refuses
    wide_map         two_trees100_a behind a hand-built source map with n_in = n_fixed = 256"""
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import pose_interp as pi
from dex_retargeting_amd import pose_tables as pt
from dex_retargeting_amd.urdf import KinematicModel, parse_urdf
from oracle.kin import OracleRobot

REV_LIMITS, PRI_LIMITS = (-1.2, 0.9), (-0.02, 0.02)
MEMBERS = ["chain64", "chain64_turns", "binary64", "binary64_slots8", "star40", "two_trees100_a", "two_trees100_b", "wide_map"]
REFUSED = "two_trees100_c"
SHARED_COL = 130  # the column of wide_map that feeds eight joints
WIDE_X_COLS = (0, 63, 64, 127, 128, 191, 192, 255)
# what the table of a member must look like: joints, fork slots, input columns, ROOT restores, links on the fixed base.
# Slots by hand, S(fork) = max(1 + S(smaller child), S(larger child)): the five fork levels of binary64 give 5; in a heap of
# 50 joints 15..23 fork into leaves (1), 7..10 give 2, 3 and 4 give 3, 1 gives 4, 2 gives 3 and runs first, so the root gives 4;
# a heap cut after joint 31 is a complete tree of four fork levels
FACTS = {
    "chain64": dict(n_joint=64, n_slot=0, n_in=64, n_root=1, n_base=0, n_link=64),
    "chain64_turns": dict(n_joint=64, n_slot=0, n_in=64, n_root=1, n_base=0, n_link=64),
    "binary64": dict(n_joint=64, n_slot=5, n_in=64, n_root=1, n_base=0, n_link=64),
    "binary64_slots8": dict(n_joint=64, n_slot=8, n_in=64, n_root=1, n_base=0, n_link=64),
    "star40": dict(n_joint=40, n_slot=0, n_in=40, n_root=40, n_base=3, n_link=44),
    "two_trees100_a": dict(n_joint=50, n_slot=4, n_in=100, n_root=1, n_base=0, n_link=50),
    "two_trees100_b": dict(n_joint=64, n_slot=4, n_in=100, n_root=2, n_base=0, n_link=64),
    "wide_map": dict(n_joint=50, n_slot=4, n_in=256, n_root=1, n_base=0, n_link=50),
}


class _Urdf:
    def __init__(self, name, seed, rev_limits=REV_LIMITS):
        self.name, self.rng, self.rev_limits = name, np.random.default_rng(seed), rev_limits
        self.links, self.joints = [], []

    def link(self, name):
        self.links.append(f'<link name="{name}"/>')
        return name

    def joint(self, name, typ, parent, child):
        """a joint from `parent` to the new link `child`: random origin and axis, the member's limits."""
        rng = self.rng
        sign = lambda: rng.choice([-1.0, 1.0], 3)  # noqa: E731
        xyz, rpy = sign() * rng.uniform(0.01, 0.03, 3), sign() * rng.uniform(0.2, 1.0, 3)
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        f = lambda v: " ".join(f"{c:.17g}" for c in v)  # noqa: E731
        body = f'<parent link="{parent}"/><child link="{self.link(child)}"/><origin xyz="{f(xyz)}" rpy="{f(rpy)}"/>'
        if typ != "fixed":
            lo, hi = self.rev_limits if typ == "revolute" else PRI_LIMITS
            body += f'<axis xyz="{f(axis)}"/><limit lower="{lo}" upper="{hi}"/>'
        self.joints.append(f'<joint name="{name}" type="{typ}">{body}</joint>')
        return child

    def write(self, directory):
        path = os.path.join(str(directory), f"{self.name}.urdf")
        with open(path, "w") as fh:
            fh.write(f'<robot name="{self.name}">' + "".join(self.links + self.joints) + "</robot>")
        return KinematicModel(parse_urdf(path)), OracleRobot(path)


def _chain64(u):
    prev = u.link("base")
    links, fixed = [], []
    for k in range(64):
        prev = u.joint(f"j{k:02d}", "prismatic" if k % 5 == 4 else "revolute", prev, f"l{k:02d}")
        links.append(prev)
        if k % 8 == 7:
            fixed.append(u.joint(f"f{k:02d}", "fixed", prev, f"t{k:02d}"))
    # 64 links: the eight behind fixed joints and 56 of the chain, its last one among them
    return [l for k, l in enumerate(links) if k % 8 != 3] + fixed


def _binary64(u):
    u.link("base")
    level = [u.joint("r", "prismatic", "base", "lr")]
    links, n = list(level), 0
    for depth in range(5):
        nxt = []
        for parent in level:
            for side in "ab":
                n += 1
                nxt.append(u.joint(f"j{parent[1:]}{side}", "prismatic" if n % 4 == 0 else "revolute", parent, f"l{parent[1:]}{side}"))
        links += nxt
        level = nxt
    assert len(links) == 63
    links.append(u.joint("jextra", "revolute", level[11], "lextra"))
    return links


def _star40(u):
    u.link("base")
    links = [u.joint(f"j{k:02d}", "prismatic" if k % 3 == 1 else "revolute", "base", f"l{k:02d}") for k in range(40)]
    links += [u.joint("fa", "fixed", "base", "ta"), u.joint("fb", "fixed", "ta", "tb")]
    links = [links[i] for i in u.rng.permutation(len(links))]
    links.insert(5, "base")
    links.insert(20, links[2])  # a repeat
    return links


def _two_trees(u):
    """-> link names [tree][heap index]: joint i of a tree hangs off joint (i - 1) // 2, joint 0 off the base."""
    u.link("base")
    out = []
    for t in "ab":
        names = []
        for i in range(50):
            parent = "base" if i == 0 else names[(i - 1) // 2]
            names.append(u.joint(f"{t}j{i:02d}", "prismatic" if i % 6 == 5 else "revolute", parent, f"{t}l{i:02d}"))
        out.append(names)
    return out


def _renumber_slots(blob, n_slot=8):
    """every slot s of the blob becomes n_slot - 1 - s: the same arithmetic at other LDS addresses."""
    nj = int(np.frombuffer(blob[:32], pt.HEADER_DTYPE)[0]["n_joint"])
    head = np.frombuffer(blob[:32], pt.HEADER_DTYPE).copy()
    joints = np.frombuffer(blob[32:32 + nj * pt.JOINT_DTYPE.itemsize], pt.JOINT_DTYPE).copy()
    head["n_slot"] = n_slot
    for field in ("save", "restore"):
        s = joints[field]
        joints[field] = np.where(s >= 0, n_slot - 1 - s, s)
    return head.tobytes() + joints.tobytes() + blob[32 + nj * pt.JOINT_DTYPE.itemsize:]


def _wide_map(kin, rng):
    """SourceMap(256, 256) over the second tree (dofs 50..99; the first tree is not in the table): 16 joints from `fixed`,
    4 constants, 8 revolute joints on one column with multipliers of both signs, 22 joints on columns of their own."""
    dofs = list(range(50, 100))
    rev = [k for k in dofs if kin.joints[k].type == "revolute"]
    shared = [rev[i] for i in (1, 5, 9, 14, 20, 27, 33, 40)]
    rest = [k for k in dofs if k not in shared]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    fixed, const, own = rest[:16], rest[16:20], rest[20:]
    entries = [(pt.SRC_CONST, 0, 0.0, 0.0)] * 50 + [None] * 50
    for i, k in enumerate(shared):
        entries[k] = (pt.SRC_X, SHARED_COL, (-1.0) ** i * rng.uniform(0.4, 1.2), (-1.0) ** (i // 2) * rng.uniform(0.05, 0.2))
    free = [c for c in range(256) if c not in WIDE_X_COLS and c != SHARED_COL]
    xcols = list(WIDE_X_COLS) + [free[i] for i in rng.permutation(len(free))[:len(own) - len(WIDE_X_COLS)]]
    fcols = [0, 255] + [int(c) for c in 1 + rng.permutation(254)[:len(fixed) - 2]]
    for kind, joints, cols in ((pt.SRC_X, own, xcols), (pt.SRC_FIXED, fixed, fcols)):
        for k, c in zip(joints, cols):
            entries[k] = (kind, int(c), float(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1.5)), float(rng.uniform(-0.3, 0.3)))
    for k in const:
        j = kin.joints[k]
        entries[k] = (pt.SRC_CONST, 0, float(rng.uniform(-2, 2)), float(rng.uniform(0.3, 0.9) * (j.upper if rng.random() < 0.5 else j.lower)))
    return pt.SourceMap(256, 256, entries)


@dataclass
class Member:
    name: str
    kin: KinematicModel
    orc: OracleRobot
    links: List[str]
    smap: pt.SourceMap
    blob: Optional[bytes]  # None: compile_poses refuses the member
    depth: int             # the longest joint chain of a requested link

    @property
    def tab(self):
        return pi.parse(self.blob)


def build(name, directory) -> Member:
    base = {"chain64_turns": "chain64", "binary64_slots8": "binary64", "wide_map": "two_trees100_a"}.get(name, name)
    base, which = (base[:-2], base[-1]) if base.startswith("two_trees100_") else (base, "")
    seed = {"chain64": 64, "binary64": 65, "star40": 40, "two_trees100": 100}[base]
    u = _Urdf(name, seed, (-20.0, 20.0) if name == "chain64_turns" else REV_LIMITS)
    made = {"chain64": _chain64, "binary64": _binary64, "star40": _star40, "two_trees100": _two_trees}[base](u)
    kin, orc = u.write(directory)
    assert kin.dof_joint_names == orc.dof_joint_names
    if base == "two_trees100":
        a, b = made
        links = {"a": b, "b": a[:32] + b[:32], "c": a + b[36:]}[which]
    else:
        links = made
    smap = _wide_map(kin, u.rng) if name == "wide_map" else pt.SourceMap.robot_order(kin)
    depth = max(len(kin.ancestors(kin.frames[kin.body_frame_index(n)].parent)) if kin.frames[kin.body_frame_index(n)].parent >= 0 else 0
                for n in links)
    if name == REFUSED:
        return Member(name, kin, orc, links, smap, None, depth)
    blob = pt.compile_poses(kin, links, smap)
    if name == "binary64_slots8":
        blob = _renumber_slots(blob)
    return Member(name, kin, orc, links, smap, blob, depth)


# ---- the source map as the chain rule sees it -------------------------------------------------------------------------------
def full_q(smap, x, fixed=None):
    """q_k = mult_k in[col_k] + off_k for every dof joint of the model: what the oracle is asked."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    q = np.zeros((x.shape[0], len(smap.entries)))
    for k, (kind, col, mult, off) in enumerate(smap.entries):
        src = x[:, col] if kind == pt.SRC_X else (np.asarray(fixed, np.float64)[:, col] if kind == pt.SRC_FIXED else 0.0)
        q[:, k] = mult * src + off
    return q


def fold(smap, d_full):
    """derivative in the full joint vector (..., dof) -> derivative in x (..., n_in): column col_k collects mult_k times
    column k of every joint that reads x."""
    d_full = np.asarray(d_full)
    out = np.zeros(d_full.shape[:-1] + (smap.n_in,))
    for k, (kind, col, mult, _) in enumerate(smap.entries):
        if kind == pt.SRC_X:
            out[..., col] += mult * d_full[..., k]
    return out


def inputs(m: Member, B, seed):
    """seeded float32-representable (x, fixed, xdot) as float64: a column read by one joint puts that joint inside its
    limits, a column read by several (or by none) is uniform in +-0.5."""
    rng = np.random.default_rng(seed)
    sm = m.smap
    x, fixed = rng.uniform(-0.5, 0.5, (B, sm.n_in)), rng.uniform(-0.5, 0.5, (B, sm.n_fixed))
    readers = {}
    for k, (kind, col, mult, off) in enumerate(sm.entries):
        readers.setdefault((kind, col), []).append(k)
    for (kind, col), ks in readers.items():
        if kind == pt.SRC_CONST or len(ks) != 1:
            continue
        j, (_, _, mult, off) = m.kin.joints[ks[0]], sm.entries[ks[0]]
        (x if kind == pt.SRC_X else fixed)[:, col] = (rng.uniform(j.lower, j.upper, B) - off) / mult
    xdot = rng.standard_normal((B, sm.n_in))
    r32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    return r32(x), (r32(fixed) if sm.n_fixed else None), r32(xdot)


# ---- float32 gates (derived in the docstring of tests/test_gpu_pose_zoo.py) ---------------------------------------------------
def abs_mult(m: Member):
    """(n_link, n_in): per requested link (the caller's order) and column, sum |mult| over the joints of the link's chain
    that read the column; 0 where no joint above the link reads it."""
    tab = m.tab
    out = np.zeros((len(tab["links"]), int(tab["h"]["n_in"])))
    for l in tab["links"]:
        k = int(l["parent"])
        while k >= 0:
            j = tab["joints"][k]
            if int(j["src_kind"]) == pt.SRC_X:
                out[int(l["out"]), int(j["src_col"])] += abs(float(j["mult"]))
            k = int(j["parent"])
    return out


def gates(m: Member, reach):
    """g_rot per rotation / axis entry, g_pos per position entry, and per (link, column) the gates of an entry of the linear
    Jacobian, of the angular Jacobian (world aligned, and in the link's own axes) and of d rot / d x."""
    g_rot = max(4 * m.depth, 12) * 2.0 ** -24
    g_pos = g_rot * max(1.0, reach)
    am = abs_mult(m)
    jlin, jang = am * (2 * reach * g_rot + 2 * g_pos), am * g_rot
    turn = np.sqrt(3.0) * g_rot * am  # R^T v against the exact R^T: g_rot |v|_1 <= sqrt(3) g_rot |v|
    return dict(rot=g_rot, pos=g_pos, jlin=jlin, jang=jang, jlin_local=jlin + turn * 2 * reach, jang_local=jang + turn,
                drot=am * 2 * g_rot)


def contraction_gates(g, xdot=None, grad_pos=None, grad_rot=None, local=False):
    """velocity gates (B, L, 1) for |xdot| (lin, ang), or the VJP gate (B, n_in) for |grad_pos| and / or |grad_rot|."""
    if xdot is not None:
        a, s = np.abs(xdot), "_local" if local else ""
        return (a @ g["jlin" + s].T)[:, :, None], (a @ g["jang" + s].T)[:, :, None]
    out = 0.0
    if grad_pos is not None:
        out = out + np.abs(grad_pos).sum(2) @ g["jlin"]
    if grad_rot is not None:
        out = out + np.abs(grad_rot).sum((2, 3)) @ g["drot"]
    return out


# ---- what the oracle says -------------------------------------------------------------------------------------------------
def expect(m: Member, x, fixed=None):
    """float64 from OracleRobot at the full joint vector, derivatives folded by the chain rule: pos (B, L, 3), rot
    (B, L, 3, 3), world-aligned jlin, jang (B, L, 3, n_in), and q_full."""
    from test_gpu_link_jacobians import oracle_jacobians

    q = full_q(m.smap, x, fixed)
    jl, ja, R = oracle_jacobians(m.orc, q, m.links)
    _, p = m.orc.link_poses(q, m.links)
    return dict(q=q, pos=p, rot=R, jlin=fold(m.smap, jl), jang=fold(m.smap, ja))


def expect_vjp(m: Member, q_full, grad_pos, grad_rot):
    from test_gpu_link_poses import oracle_vjp

    return fold(m.smap, oracle_vjp(m.orc, q_full, m.links, grad_pos, grad_rot))

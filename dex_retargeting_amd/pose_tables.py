"""Compiler of the pose tables (include/dexr_pose.h): the kinematic tree above a list of links, float64 throughout, with
the joints in depth-first order, the fork save / restore slots of the one-lane-per-frame walk, the links sorted by parent
joint, and a source map that says where every joint value comes from.  Host plumbing, cold path; the per-frame arithmetic
is csrc/dexr_pose.hip."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .urdf import KinematicModel

MAGIC = 0x53505844
VERSION = 1
MAXJ, MAXL, MAXSLOT, MAXIN = 64, 64, 8, 256
REVOLUTE, PRISMATIC = 0, 1
SRC_X, SRC_FIXED, SRC_CONST = 0, 1, 2
CONTINUE, ROOT = -1, -2

HEADER_DTYPE = np.dtype([("magic", "<u4"), ("version", "<u4"), ("n_joint", "<i4"), ("n_link", "<i4"), ("n_in", "<i4"),
                         ("n_fixed", "<i4"), ("n_slot", "<i4"), ("reserved", "<i4")])
JOINT_DTYPE = np.dtype([("parent", "<i4"), ("type", "<i4"), ("src_kind", "<i4"), ("src_col", "<i4"), ("restore", "<i4"),
                        ("save", "<i4"), ("link_begin", "<i4"), ("link_end", "<i4"), ("sub_link_end", "<i4"),
                        ("reserved", "<i4"), ("mult", "<f8"), ("off", "<f8"), ("X", "<f8", (12,)), ("axis", "<f8", (3,))])
LINK_DTYPE = np.dtype([("parent", "<i4"), ("out", "<i4"), ("X", "<f8", (12,))])


@dataclass
class SourceMap:
    """q_k = mult * in[col] + off per dof joint of the kinematic model (pinocchio dof order): `entries[k]` is
    (kind, col, mult, off) with kind SRC_X (row of x, gets a gradient), SRC_FIXED (row of fixed) or SRC_CONST (q_k = off)."""
    n_in: int
    n_fixed: int
    entries: List[Tuple[int, int, float, float]]

    @staticmethod
    def robot_order(kin: KinematicModel) -> "SourceMap":
        """x = the full qpos in pinocchio dof order."""
        return SourceMap(kin.dof, 0, [(SRC_X, k, 1.0, 0.0) for k in range(kin.dof)])

    @staticmethod
    def optimizer_order(kin: KinematicModel, idx_pin2target, idx_pin2fixed, mimic=()) -> "SourceMap":
        """x = the (B, n_opt) rows of the optimiser (target-joint order), fixed = its fixed_qpos rows, mimic joints
        `(mimic dof, source dof, multiplier, offset)` folded onto the column of their source."""
        entries: List[Optional[Tuple[int, int, float, float]]] = [None] * kin.dof
        for c, k in enumerate(idx_pin2target):
            entries[int(k)] = (SRC_X, c, 1.0, 0.0)
        for c, k in enumerate(idx_pin2fixed):
            entries[int(k)] = (SRC_FIXED, c, 1.0, 0.0)
        for m, s, mult, off in mimic:
            src = entries[int(s)]
            if src is None or src[0] == SRC_CONST:
                raise ValueError(f"mimic joint {kin.joints[int(m)].name}: its source joint is neither a target nor a fixed joint")
            entries[int(m)] = (src[0], src[1], float(mult) * src[2], float(mult) * src[3] + float(off))
        for k, e in enumerate(entries):
            if e is None:
                raise ValueError(f"joint {kin.joints[k].name} is neither a target, a fixed nor a mimic joint")
        return SourceMap(len(idx_pin2target), len(idx_pin2fixed), entries)  # type: ignore[arg-type]


def compile_poses(kin: KinematicModel, link_names: Sequence[str], source_map: Optional[SourceMap] = None) -> bytes:
    """Pose table blob for `link_names` (any links of the model, at most 64 per table, repeats allowed)."""
    sm = source_map or SourceMap.robot_order(kin)
    if len(sm.entries) != kin.dof:
        raise ValueError(f"the source map has {len(sm.entries)} entries, the model {kin.dof} joints")
    if not 1 <= len(link_names) <= MAXL:
        raise ValueError(f"a pose table holds 1..{MAXL} links, got {len(link_names)}")
    if sm.n_in > MAXIN or sm.n_fixed > MAXIN:
        raise ValueError(f"a pose table reads at most {MAXIN} columns per input row")
    bodies = [kin.frames[kin.body_frame_index(n)] for n in link_names]
    needed = set()
    for f in bodies:
        if f.parent >= 0:
            needed.update(kin.ancestors(f.parent))
    children = {k: [] for k in needed}
    roots = []
    for k in sorted(needed):
        p = kin.joints[k].parent
        (children[p] if p >= 0 else roots).append(k)
    size = {}
    for k in sorted(needed, reverse=True):  # (a child has a larger dof index than its parent: depth-first numbering)
        size[k] = 1 + sum(size[c] for c in children[k])
    # depth-first order, smallest subtree first: the transform of a fork is dropped when its LAST child starts, so the
    # largest subtree runs with the slot already free and at most log2(n_joint) slots are alive at once
    order: List[int] = []
    restore, save = {}, {}
    free = list(range(MAXJ))
    n_slot = 0

    def emit(k: int, how: int):
        nonlocal n_slot
        order.append(k)
        restore[k] = how
        kids = sorted(children[k], key=lambda c: (size[c], c))
        save[k] = -1
        if len(kids) >= 2:
            save[k] = free.pop(0)
            n_slot = max(n_slot, save[k] + 1)
        for i, c in enumerate(kids):
            if i == len(kids) - 1 and save[k] >= 0:
                free.insert(0, save[k])
                free.sort()
            emit(c, CONTINUE if i == 0 else save[k])

    for r in sorted(roots, key=lambda c: (size[c], c)):
        emit(r, ROOT)
    if len(order) > MAXJ:
        raise ValueError(f"the links depend on {len(order)} joints, a pose table holds {MAXJ}")
    if n_slot > MAXSLOT:
        raise ValueError(f"the tree needs {n_slot} fork slots, a pose table holds {MAXSLOT}")
    new = {k: i for i, k in enumerate(order)}

    lorder = sorted(range(len(bodies)), key=lambda i: (new[bodies[i].parent] if bodies[i].parent >= 0 else -1, i))
    links = np.zeros(len(bodies), LINK_DTYPE)
    for pos, i in enumerate(lorder):
        f = bodies[i]
        links[pos]["parent"] = new[f.parent] if f.parent >= 0 else -1
        links[pos]["out"] = i
        links[pos]["X"] = np.asarray(f.placement, np.float64)[:3, :4].reshape(12)
    lparent = links["parent"]

    joints = np.zeros(len(order), JOINT_DTYPE)
    for i, k in enumerate(order):
        j = kin.joints[k]
        kind, col, mult, off = sm.entries[k]
        ncol = {SRC_X: sm.n_in, SRC_FIXED: sm.n_fixed, SRC_CONST: 1}[kind]
        if not 0 <= col < ncol:
            raise ValueError(f"joint {j.name}: source column {col} out of range")
        rec = joints[i]
        rec["parent"] = new[j.parent] if j.parent >= 0 else -1
        rec["type"] = REVOLUTE if j.type == "revolute" else PRISMATIC
        rec["src_kind"], rec["src_col"], rec["mult"], rec["off"] = kind, col, mult, off
        rec["restore"], rec["save"] = restore[k], save[k]
        rec["link_begin"] = int(np.searchsorted(lparent, i, "left"))
        rec["link_end"] = int(np.searchsorted(lparent, i, "right"))
        rec["sub_link_end"] = int(np.searchsorted(lparent, i + size[k] - 1, "right"))
        rec["X"] = np.asarray(j.placement, np.float64)[:3, :4].reshape(12)
        rec["axis"] = np.asarray(j.axis, np.float64)
    header = np.zeros(1, HEADER_DTYPE)
    header["magic"], header["version"] = MAGIC, VERSION
    header["n_joint"], header["n_link"] = len(order), len(bodies)
    header["n_in"], header["n_fixed"], header["n_slot"] = sm.n_in, sm.n_fixed, n_slot
    return header.tobytes() + joints.tobytes() + links.tobytes()


__all__ = ["SourceMap", "compile_poses", "HEADER_DTYPE", "JOINT_DTYPE", "LINK_DTYPE"]

"""Self-collision of a sphere approximation of the robot on the GPU (include/dexr_spheres.h, csrc/dexr_spheres.hpp), for torch
tensors: signed distances of sphere pairs and a fused penalty that returns the energy and its gradient from one launch.

A ``SphereSet`` puts spheres on links (a centre in the link's own frame and a radius each) and lists the pairs to test; with
``pairs=None`` the pairs are ``default_pairs``: every two spheres whose links differ and have more than one movable joint on
the tree path between them (neighbouring links always touch and are skipped).  Per frame

    c_s = p_l + R_l center_s          d_p = |c_i - c_j| - r_i - r_j          h_p = max(0, margin - d_p)
    E = sum_p w_p h_p^2               dE/dq = sum_p -2 w_p h_p dd_p/dq

``sphere_distances(optimizer, q, sphere_set)`` gives d (B, P) -- negative where two spheres interpenetrate -- and
``self_collision_penalty(optimizer, q, sphere_set, margin)`` gives (E (B,), dE/dq (B, n_opt)) from ONE kernel launch, in which
neither distances nor forces nor normals reach memory.  Mimic joints fold onto their source's column, fixed joints move the
geometry and take no gradient, variables no joint reads get exact zeros.  The squared hinge makes E continuously
differentiable.

The outputs of this module carry NO autograd graph; ``autograd.sphere_distances`` and ``autograd.self_collision_penalty`` are
the same kernels with one, so that a penetration loss composes with ``autograd.retarget`` and reaches the keypoints.
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np

from . import _lib
from .autograd import _check_poses


class SphereSet:
    """Spheres on links and the pairs to test: plain data, immutable, hashable by content.

    links    (S,) the name of the link that carries each sphere (a link may carry many), at most 64 distinct names
    centers  (S, 3) sphere centres, each in the frame of its own link
    radii    (S,) >= 0
    pairs    (P, 2) sphere indices, i != j, or None: `default_pairs` of the robot the set is used with.

    `table_links` are the distinct names in order of first appearance (the link list of the pose table), `sphere_rows` the row of
    each sphere in it."""

    def __init__(self, links: Sequence[str], centers, radii, pairs=None):
        if isinstance(links, str) or len(links) == 0 or not all(isinstance(n, str) for n in links):
            raise ValueError("links must be a non-empty sequence of link names, one per sphere")
        names = tuple(links)
        cen = np.array(centers, dtype=np.float64)
        rad = np.array(radii, dtype=np.float64).reshape(-1)
        S = len(names)
        if cen.shape != (S, 3) or rad.shape != (S,):
            raise ValueError(f"{S} links name {S} spheres: centers must have shape ({S}, 3) and radii ({S},), got {cen.shape} and {rad.shape}")
        if not 1 <= S <= _lib.SPHERE_MAX:
            raise ValueError(f"a sphere set holds 1..{_lib.SPHERE_MAX} spheres, got {S}")
        row_of = {}
        for n in names:
            row_of.setdefault(n, len(row_of))
        if len(row_of) > 64:
            raise ValueError(f"a sphere set takes at most 64 distinct links (one pose table), got {len(row_of)}")
        if not np.isfinite(cen).all():
            raise ValueError("centers must be finite")
        if not (np.isfinite(rad).all() and (rad >= 0).all()):
            raise ValueError("radii must be finite and >= 0")
        rows = np.array([row_of[n] for n in names], dtype=np.int32)
        table = tuple(row_of)
        if pairs is not None:
            pr = np.array(pairs, dtype=np.int64)
            if pr.ndim != 2 or pr.shape[1] != 2:
                raise ValueError(f"pairs must have shape (P, 2), got {pr.shape}")
            if not 1 <= pr.shape[0] <= _lib.SPHERE_MAXPAIR:
                raise ValueError(f"a sphere set holds 1..{_lib.SPHERE_MAXPAIR} pairs, got {pr.shape[0]}")
            if (pr < 0).any() or (pr >= S).any():
                raise ValueError(f"pairs index spheres 0..{S - 1}")
            if (pr[:, 0] == pr[:, 1]).any():
                raise ValueError("a pair must name two different spheres (i != j)")
            pr = pr.astype(np.int32)
            pr.setflags(write=False)
        else:
            pr = None
        for a in (cen, rad, rows):
            a.setflags(write=False)
        self.links, self.table_links, self.centers, self.radii, self.sphere_rows, self.pairs = names, table, cen, rad, rows, pr
        self._key = (names, cen.tobytes(), rad.tobytes(), None if pr is None else pr.tobytes())

    @property
    def n_sphere(self) -> int:
        return len(self.radii)

    def __hash__(self):
        return hash(self._key)

    def __eq__(self, other):
        return isinstance(other, SphereSet) and self._key == other._key

    def __repr__(self):
        return f"SphereSet({self.n_sphere} spheres on {len(self.table_links)} links, {'default pairs' if self.pairs is None else f'{len(self.pairs)} pairs'})"


def _kin_of(robot):
    return robot.kin if hasattr(robot, "kin") else robot.robot.kin


def default_pairs(robot, sphere_set: SphereSet, skip_joint_distance: int = 1) -> np.ndarray:
    """(P, 2) int32: every i < j whose links differ and have MORE than `skip_joint_distance` movable joints on the tree path
    between them (links welded by fixed joints have distance 0, a link and its child across one joint 1).  `robot`: a
    RobotWrapper (or an optimizer: its robot)."""
    if isinstance(skip_joint_distance, bool) or not isinstance(skip_joint_distance, int) or skip_joint_distance < 0:
        raise ValueError(f"skip_joint_distance must be a Python int >= 0, got {skip_joint_distance!r}")
    kin = _kin_of(robot)
    chains = []
    for n in sphere_set.table_links:
        f = kin.frames[kin.body_frame_index(n)]
        chains.append(frozenset(kin.ancestors(f.parent)) if f.parent >= 0 else frozenset())
    rows = sphere_set.sphere_rows
    out = [(i, j) for i in range(len(rows)) for j in range(i + 1, len(rows))
           if rows[i] != rows[j] and len(chains[rows[i]] ^ chains[rows[j]]) > skip_joint_distance]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def _resolved_pairs(robot, sphere_set):
    pairs = sphere_set.pairs if sphere_set.pairs is not None else default_pairs(robot, sphere_set)
    if not 1 <= len(pairs) <= _lib.SPHERE_MAXPAIR:
        raise ValueError(f"the sphere set gives {len(pairs)} pairs with this robot, a sphere model holds 1..{_lib.SPHERE_MAXPAIR}")
    return pairs


def build_sphere_model(kin, sphere_set: SphereSet, pairs, source_map=None) -> _lib.SphereModel:
    """the device model of a sphere set on a kinematic model (what Optimizer.sphere_model / RobotWrapper.sphere_model cache)."""
    from .pose_tables import compile_poses

    return _lib.SphereModel(compile_poses(kin, list(sphere_set.table_links), source_map), sphere_set.sphere_rows, sphere_set.centers,
                            sphere_set.radii, pairs)


def _check(n_in, n_fixed, kin, robot, q, fixed_qpos, sphere_set, what, margin=None, pair_weight=None, penalty=False):
    """Every argument rule -- the sphere set, the links, the scalars, types, dtypes, shapes and last the device -- before anything
    touches the GPU.  Returns the pairs of the set on this robot."""
    import torch

    if not isinstance(sphere_set, SphereSet):
        raise ValueError("sphere_set must be a collision.SphereSet")
    for n in sphere_set.table_links:
        kin.body_frame_index(n)  # ValueError on an unknown link
    pairs = _resolved_pairs(robot, sphere_set)
    if penalty:
        if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not math.isfinite(margin) or margin < 0:
            raise ValueError(f"margin must be a finite Python float >= 0, got {margin!r}")
        if pair_weight is not None:
            if not isinstance(pair_weight, torch.Tensor):
                raise ValueError("pair_weight must be a torch tensor")
            if pair_weight.dtype != torch.float32:
                raise ValueError(f"pair_weight must be float32, got {pair_weight.dtype}")
            if tuple(pair_weight.shape) != (len(pairs),):
                raise ValueError(f"pair_weight must have shape ({len(pairs)},), one weight per pair, got {tuple(pair_weight.shape)}")
    _check_poses(n_in, n_fixed, q, fixed_qpos, sphere_set.table_links, what=what)  # (ends with the device)
    if penalty and pair_weight is not None and pair_weight.device != q.device:
        raise ValueError(f"pair_weight is on {pair_weight.device}, {what} on {q.device}: all tensors must be on one CUDA device")
    return pairs


def _inputs(x, fixed_qpos):
    xc = x.detach().contiguous()
    fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
    return xc, fixed


def _distances(model, x, fixed_qpos, centers):
    import torch

    B = x.shape[0]
    xc, fixed = _inputs(x, fixed_qpos)
    with torch.cuda.device(x.device):
        dist = torch.empty((B, model.n_pair), dtype=torch.float32, device=x.device)
        cen = torch.empty((B, model.n_sphere, 3), dtype=torch.float32, device=x.device) if centers else None
        if B > 0:
            model.distances_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), dist.data_ptr(),
                                0 if cen is None else cen.data_ptr(), stream=torch.cuda.current_stream(x.device).cuda_stream)
    return (dist, cen) if centers else dist


def _penalty(model, x, fixed_qpos, margin, pair_weight, want_grad=True):
    """one launch -> (E (B,), grad (B, n_in) or None)."""
    import torch

    B = x.shape[0]
    xc, fixed = _inputs(x, fixed_qpos)
    w = None if pair_weight is None else pair_weight.detach().contiguous()
    with torch.cuda.device(x.device):
        e = torch.empty((B,), dtype=torch.float32, device=x.device)
        g = torch.empty((B, model.n_in), dtype=torch.float32, device=x.device) if want_grad else None
        if B > 0:
            model.penalty_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), float(margin), 0 if w is None else w.data_ptr(),
                              e.data_ptr(), 0 if g is None else g.data_ptr(), stream=torch.cuda.current_stream(x.device).cuda_stream)
    return e, g


def sphere_distances(optimizer, q, sphere_set: SphereSet, fixed_qpos=None, centers: bool = False):
    """Signed distances of the set's sphere pairs at the optimiser's variables: q (B, n_opt) float32 CUDA -- what `retarget`
    returns --, fixed_qpos (B, n_fixed) or None -> dist (B, P) float32, negative where two spheres interpenetrate; with
    `centers=True` -> (dist, centers (B, S, 3)), the world centres of the spheres.  No autograd graph."""
    pairs = _check(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos, sphere_set, "q")
    return _distances(optimizer.sphere_model(sphere_set, pairs), q, fixed_qpos, centers)


def self_collision_penalty(optimizer, q, sphere_set: SphereSet, margin, pair_weight=None, fixed_qpos=None):
    """(E (B,), grad_q (B, n_opt)) float32 from ONE launch: E = sum_p w_p max(0, margin - d_p)^2 and its gradient in q.  margin:
    a finite Python float >= 0 (metres; pairs nearer than it are pushed apart); pair_weight (P,) float32 >= 0 or None (1), shared
    by the batch.  No autograd graph: `autograd.self_collision_penalty` is the same launch with one."""
    pairs = _check(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos, sphere_set, "q",
                   margin, pair_weight, penalty=True)
    return _penalty(optimizer.sphere_model(sphere_set, pairs), q, fixed_qpos, margin, pair_weight)


def robot_sphere_distances(robot, qpos, sphere_set: SphereSet, centers: bool = False):
    """The same for a full robot qpos (B, robot.dof) in dof order; every joint is a column of its own."""
    pairs = _check(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, "qpos")
    return _distances(robot.sphere_model(sphere_set, pairs), qpos, None, centers)


def robot_self_collision_penalty(robot, qpos, sphere_set: SphereSet, margin, pair_weight=None):
    """(E (B,), grad_qpos (B, robot.dof)) for a full robot qpos in dof order."""
    pairs = _check(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, "qpos", margin, pair_weight, penalty=True)
    return _penalty(robot.sphere_model(sphere_set, pairs), qpos, None, margin, pair_weight)


__all__ = ["SphereSet", "default_pairs", "sphere_distances", "self_collision_penalty", "robot_sphere_distances",
           "robot_self_collision_penalty"]

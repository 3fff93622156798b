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

An ``ObstacleSet`` is the other side of a collision with something that is not the robot (include/dexr_obstacles.h,
csrc/dexr_obstacles.hpp): spheres, capsules, boxes and half-spaces in an obstacle frame that has a world pose per frame
(``obstacle_pos``, ``obstacle_rot``: a held object) or none (a shared scene).  ``obstacle_distances`` gives the signed distance of
every sphere of a ``SphereSet`` to the nearest primitive, ``obstacle_penalty`` the squared-hinge energy over every (sphere,
primitive) entry, its gradient in q and, asked for, the wrench on the obstacle, again from ONE launch.  ``resolve_collisions``
is ``resolve_self_collision`` with that energy added (include/dexr_resolve_obstacles.h): one launch takes retargeted postures out of
the robot's own links and out of the object.

An ``SdfGrid`` is an obstacle that no handful of primitives describes -- a mesh, a scan, a depth fusion -- as float32 samples of
its signed-distance field on a regular grid of the obstacle frame (include/dexr_sdf_grid.h, csrc/dexr_sdf_grid.hpp), posed like
an ``ObstacleSet``.  ``grid_distances`` and ``grid_penalty`` are ``obstacle_distances`` and ``obstacle_penalty`` against it: one
trilinear lookup per sphere however complex the shape is, the distance continued outside the grid's box by the distance to the
box.  ``SdfGrid.from_obstacles`` samples an ``ObstacleSet``.  ``resolve_grid_collisions`` is ``resolve_collisions`` against a grid
(include/dexr_resolve_grid.h): a sphere has one contact at most, so nothing is capped.

A grid need not come from a shape known in advance (include/dexr_distance_transform.h, csrc/dexr_distance_transform.hpp):
``SdfGrid.from_points`` and ``SdfGrid.from_occupancy`` make one from a depth camera's point cloud or a voxel occupancy map by the
exact Euclidean distance transform on the device, whose cost does not grow with the number of points.  A ``DeviceSdfGrid`` is a
grid whose samples live on the device and are rewritten in place (``update_from_points``, ``update_from_occupancy``) on the
current stream: a scene that changes per frame feeds ``grid_penalty`` and ``resolve_grid_collisions`` without a host copy.

The other robot is the one obstacle that has its own q per frame (include/dexr_cross.h, csrc/dexr_cross.hpp): the other hand of a
two-handed recording, a second gripper, the arm beside the hand.  ``cross_distances`` and ``cross_penalty`` take two optimisers,
two q, two ``SphereSet`` and a base pose per robot and frame (``pos_a``, ``rot_a``, ``pos_b``, ``rot_b``), and give the distance of
every sphere of either robot to the nearest sphere of the other, and the squared-hinge energy over every (sphere of A, sphere of
B) pair with its gradient in both q and, asked for, the wrench on either base -- ONE launch that walks both robots.

A ``SphereSet`` need not be written by hand (include/dexr_sphere_fit.h, csrc/dexr_sphere_fit.hpp): ``link_grid`` samples a link's
mesh into a grid with one spacing, ``fit_spheres`` takes a few inscribed spheres from the grids of all links in one call -- a
greedy cover, every round the sphere that covers the most interior samples no earlier one covers -- and ``SphereSet.from_meshes``
and ``SphereSet.from_urdf`` chain the two for the meshes, or the ``<collision>`` elements of the URDF, of a robot.

The outputs of this module carry NO autograd graph; ``autograd.sphere_distances``, ``autograd.self_collision_penalty``,
``autograd.obstacle_distances``, ``autograd.obstacle_penalty``, ``autograd.grid_distances``, ``autograd.grid_penalty``,
``autograd.cross_distances`` and ``autograd.cross_penalty`` are the same kernels with one, so that a penetration loss composes
with ``autograd.retarget`` and reaches the keypoints.
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

    @classmethod
    def from_meshes(cls, robot, meshes, spheres_per_link=4, max_dim=48, min_radius=0.0, inflate=0.0, coverage=1.0, pairs=None):
        """A sphere set fitted to the links' meshes: `meshes` is {link name: TriangleMesh in the link's own frame}, `spheres_per_link`
        an int or {link name: int}.  Every mesh is sampled by `link_grid(mesh, max_dim)` and all links are fitted in ONE `fit_spheres`
        call; the spheres of a link follow each other in the order the rounds took them, the links in the dict's order.  A link
        whose fit is empty (no sample inside the mesh deeper than min_radius: raise max_dim) is a ValueError naming it, and so are more
        than 128 spheres in total or a name the robot does not have."""
        if not isinstance(meshes, dict) or not meshes or not all(isinstance(n, str) and isinstance(m, TriangleMesh) for n, m in meshes.items()):
            raise ValueError("meshes must be a non-empty dict {link name: collision.TriangleMesh}")
        known = set(_kin_of(robot).link_names)
        for n in meshes:
            if n not in known:
                raise ValueError(f"the robot has no link {n!r}")
        if isinstance(spheres_per_link, dict):
            missing = [n for n in meshes if n not in spheres_per_link]
            if missing:
                raise ValueError(f"spheres_per_link names no count for {missing}")
            k = [spheres_per_link[n] for n in meshes]
        else:
            k = [spheres_per_link] * len(meshes)
        if not all(isinstance(v, (int, np.integer)) and v >= 1 for v in k):
            raise ValueError(f"spheres_per_link must be integers >= 1, got {k}")
        if sum(k) > _lib.SPHERE_MAX:
            raise ValueError(f"a sphere set holds at most {_lib.SPHERE_MAX} spheres, {len(meshes)} links ask for {sum(k)}")
        if len(meshes) > _lib.SPHERE_FIT_MAX_BODIES:
            raise ValueError(f"a sphere set takes at most {_lib.SPHERE_FIT_MAX_BODIES} links, got {len(meshes)}")
        _fit_scalars(min_radius, inflate, coverage)  # before any sampling
        grids = [link_grid(m, max_dim) for m in meshes.values()]
        fits = fit_spheres(grids, np.array(k), min_radius, inflate, coverage)
        links, centers, radii = [], [], []
        for name, fit in zip(meshes, fits):
            if len(fit) == 0:
                raise ValueError(f"link {name!r}: no sphere fits ({fit.n_interior} interior samples at max_dim = {max_dim}, min_radius = {min_radius})")
            links += [name] * len(fit)
            centers.append(fit.centers)
            radii.append(fit.radii)
        return cls(links, np.concatenate(centers), np.concatenate(radii), pairs)

    @classmethod
    def from_urdf(cls, robot, urdf_path, spheres_per_link=4, max_dim=48, min_radius=0.0, inflate=0.0, coverage=1.0, pairs=None):
        """`SphereSet.from_meshes` of the <collision> geometry of a URDF file (`urdf.parse_collision_geometry`, tessellated and loaded
        by `meshio.link_mesh`): every link of the robot that has geometry, in file order."""
        from . import meshio
        from .urdf import parse_collision_geometry

        geometry = parse_collision_geometry(urdf_path)
        known = set(_kin_of(robot).link_names)
        names = [n for n, items in geometry.items() if items and n in known]
        if not names:
            raise ValueError(f"{urdf_path}: no link of the robot has <collision> geometry")
        meshes = {n: TriangleMesh(*meshio.link_mesh(geometry[n]), drop_degenerate=True) for n in names}
        return cls.from_meshes(robot, meshes, spheres_per_link, max_dim, min_radius, inflate, coverage, pairs)

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


def sphere_model_key(sphere_set: SphereSet, pairs, target_links=()):
    """the cache key of a sphere model: the set alone without target links, else (set, pairs, target links)."""
    if not target_links:
        return sphere_set
    return sphere_set, None if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32).tobytes(), tuple(target_links)


def resolve_table(sphere_set: SphereSet, target_links=()):
    """(table links, sphere rows) of a sphere model: the set's own table without target links; with them the target links in the
    caller's order followed by the sphere links not among them, the sphere rows remapped."""
    if not target_links:
        return list(sphere_set.table_links), sphere_set.sphere_rows
    targets = list(target_links)
    row_of = {}
    for i, n in enumerate(targets):
        row_of.setdefault(n, i)
    rest = [n for n in sphere_set.table_links if n not in row_of]
    for k, n in enumerate(rest):
        row_of[n] = len(targets) + k
    return targets + rest, np.array([row_of[n] for n in sphere_set.links], dtype=np.int32)


def build_sphere_model(kin, sphere_set: SphereSet, pairs, source_map=None, target_links=()) -> _lib.SphereModel:
    """the device model of a sphere set on a kinematic model (what Optimizer.sphere_model / RobotWrapper.sphere_model cache)."""
    from .pose_tables import compile_poses

    table, rows = resolve_table(sphere_set, target_links)
    return _lib.SphereModel(compile_poses(kin, table, source_map), rows, sphere_set.centers, sphere_set.radii, pairs)


def _check(n_in, n_fixed, kin, robot, q, fixed_qpos, sphere_set, what, margin=None, pair_weight=None, penalty=False, poses=True):
    """Every argument rule -- the sphere set, the links, the scalars, types, dtypes, shapes and last the device -- before anything
    touches the GPU.  Returns the pairs of the set on this robot.  `poses=False` leaves the rules of q and fixed_qpos and the
    device to a caller that checks more first."""
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
    if not poses:
        return pairs
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


_REQUIRED = object()


def _resolve_rules(n_in, x0, sphere_set, damping, max_iters, posture_weight, q_ref, collision_weight, link_names, target_pos, target_rot,
                   pos_weight, rot_weight, tol, max_step, limits):
    """The argument rules of the resolve that `_check` does not know, none of which looks at a device: the scalars, then the types,
    dtypes and shapes of the optional tensors.  Returns the optional tensors by name, for the device rule that comes last."""
    import torch

    if not isinstance(sphere_set, SphereSet):
        raise ValueError("sphere_set must be a collision.SphereSet")
    if damping is _REQUIRED:
        raise ValueError("damping is required: a positive finite Python float (there is no default)")
    if isinstance(damping, bool) or not isinstance(damping, (int, float)) or not math.isfinite(damping) or damping <= 0:
        raise ValueError(f"damping must be a positive finite Python float, got {damping!r}")
    if max_iters is _REQUIRED:
        raise ValueError("max_iters is required: a Python int in 1..256 (there is no default)")
    if isinstance(max_iters, bool) or not isinstance(max_iters, int) or not 1 <= max_iters <= 256:
        raise ValueError(f"max_iters must be a Python int in 1..256, got {max_iters!r}")
    for name, v in (("collision_weight", collision_weight), ("tol", tol), ("max_step", max_step)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite Python float >= 0, got {v!r}")
    if posture_weight is not None and not isinstance(posture_weight, torch.Tensor):
        if isinstance(posture_weight, bool) or not isinstance(posture_weight, (int, float)) or not math.isfinite(posture_weight) or posture_weight < 0:
            raise ValueError(f"posture_weight must be a finite Python float >= 0 or a ({n_in},) float32 tensor, got {posture_weight!r}")
    if link_names is None:
        if any(a is not None for a in (target_pos, target_rot, pos_weight, rot_weight)):
            raise ValueError("target_pos, target_rot, pos_weight and rot_weight need link_names: the links they are targets of")
        L = 0
    else:
        if isinstance(link_names, str) or len(link_names) == 0 or not all(isinstance(n, str) for n in link_names):
            raise ValueError("link_names must be a non-empty sequence of link names")
        if target_pos is None and target_rot is None:
            raise ValueError("link_names given but target_pos and target_rot are both None: at least one of them is required")
        if pos_weight is not None and target_pos is None:
            raise ValueError("pos_weight given without target_pos")
        if rot_weight is not None and target_rot is None:
            raise ValueError("rot_weight given without target_rot")
        L = len(link_names)
        n_table = len(resolve_table(sphere_set, link_names)[0])
        if n_table > 64:
            raise ValueError(f"the target links and the sphere links make {n_table} links, a resolve takes at most 64 (one pose table)")
    B = x0.shape[0] if isinstance(x0, torch.Tensor) and x0.ndim == 2 else None
    named = [(n, t, s) for n, t, s in (("q_ref", q_ref, (B, n_in)), ("target_pos", target_pos, (B, L, 3)), ("target_rot", target_rot, (B, L, 3, 3)),
                                       ("pos_weight", pos_weight, (B, L)), ("rot_weight", rot_weight, (B, L)), ("limits", limits, (n_in, 2)))
             if t is not None]
    if isinstance(posture_weight, torch.Tensor):
        named.append(("posture_weight", posture_weight, (n_in,)))
    for name, t, _ in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    for name, t, _ in named:
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    for name, t, shape in named:
        if (B is not None or shape[0] is not None) and tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    return [(n, t) for n, t, _ in named]


def _resolve(model_of, n_in, n_fixed, kin, robot, x0, what, fixed_qpos, sphere_set, margin, damping, max_iters, posture_weight, q_ref,
             collision_weight, pair_weight, link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits):
    """every rule, then one model and one launch."""
    import torch

    named = _resolve_rules(n_in, x0, sphere_set, damping, max_iters, posture_weight, q_ref, collision_weight, link_names, target_pos,
                           target_rot, pos_weight, rot_weight, tol, max_step, limits)
    for n in link_names or ():
        kin.body_frame_index(n)  # ValueError on an unknown link
    pairs = _check(n_in, n_fixed, kin, robot, x0, fixed_qpos, sphere_set, what, margin, pair_weight, penalty=True)  # (ends with the device)
    for name, t in named:
        if t.device != x0.device:
            raise ValueError(f"{name} is on {t.device}, {what} on {x0.device}: all tensors must be on one CUDA device")
    B = x0.shape[0]
    xc, fixed = _inputs(x0, fixed_qpos)
    c = lambda a: None if a is None else a.detach().contiguous()  # noqa: E731
    xr, tp, tr, wl, wa, pw = (c(a) for a in (q_ref, target_pos, target_rot, pos_weight, rot_weight, pair_weight))
    lo, hi = (None, None) if limits is None else (limits.detach()[:, 0].contiguous(), limits.detach()[:, 1].contiguous())
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x0.device):
        if isinstance(posture_weight, torch.Tensor):
            u = c(posture_weight)
        else:
            u = None if not posture_weight else torch.full((n_in,), float(posture_weight), dtype=torch.float32, device=x0.device)
        model = model_of(sphere_set, pairs, tuple(link_names or ()))
        q = torch.empty((B, model.n_in), dtype=torch.float32, device=x0.device)
        iters = torch.empty((B,), dtype=torch.int32, device=x0.device)
        energy = torch.empty((B, 3), dtype=torch.float32, device=x0.device)
        status = torch.empty((B,), dtype=torch.int32, device=x0.device)
        if B > 0:
            model.resolve_dev(B, xc.data_ptr(), ptr(fixed), float(margin), float(damping), int(max_iters), q.data_ptr(), iters.data_ptr(),
                              energy.data_ptr(), status.data_ptr(), x_ref_ptr=ptr(xr), posture_weight_ptr=ptr(u),
                              n_target=len(link_names or ()), target_pos_ptr=ptr(tp), target_rot_ptr=ptr(tr), pos_weight_ptr=ptr(wl),
                              rot_weight_ptr=ptr(wa), collision_weight=float(collision_weight), pair_weight_ptr=ptr(pw), lo_ptr=ptr(lo),
                              hi_ptr=ptr(hi), tol=float(tol), max_step=float(max_step), stream=torch.cuda.current_stream(x0.device).cuda_stream)
    return q, iters, energy, status


def resolve_self_collision(optimizer, q0, sphere_set: SphereSet, margin, damping=_REQUIRED, max_iters=_REQUIRED, posture_weight=None,
                           q_ref=None, collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None, target_rot=None,
                           pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None, fixed_qpos=None):
    """Project postures out of self-penetration inside ONE launch: from q0 (B, n_opt) float32 CUDA, up to `max_iters` (1..256)
    damped Gauss-Newton trial steps on

        E = sum_l w_pos |target_pos_l - p_l|^2 + w_rot |log(target_rot_l R_l^T)|^2  +  sum_c u_c (q_c - q_ref_c)^2
            + collision_weight * sum_p w_p max(0, margin - d_p)^2

    with an accept / reject rule and a damping of its own per frame (a trial that raises E is dropped and the damping grows
    eightfold; an accepted one divides it by four, never below `damping`), so that E never rises: the answer is the last
    accepted point.  -> (q (B, n_opt) float32, iters (B) int32 the trial steps taken, energy (B, 3) float32 the three terms of
    E at q, status (B) int32: bits _lib.RESOLVE_CONVERGED (an accepted step moved nothing by more than `tol`), RESOLVE_STALLED
    (twelve rejections in a row), RESOLVE_TRUNCATED (a point had more than 256 active pairs; the curvature used the first 256)).
    posture_weight u: a Python float or an (n_opt,) float32 tensor >= 0, None: 0; q_ref (B, n_opt) or None: q0.  link_names with
    target_pos (B, L, 3) and / or target_rot (B, L, 3, 3), pos_weight, rot_weight (B, L) or None (1) are world targets as in
    `jacobians.link_ik_solve`; the links need carry no sphere.  pair_weight (P,) as in `self_collision_penalty`.  limits
    (n_opt, 2) float32 or None: a variable on a bound that the step would push outward is frozen, every trial is clamped.
    max_step > 0 scales a step so that its largest entry is max_step at most.  `margin`, `damping` and `max_iters` are required.
    Mimic joints fold onto their source's column, fixed joints do not move, variables no joint reads come back unchanged.  The
    target links and the sphere links together are at most 64.  No autograd graph."""
    return _resolve(optimizer.sphere_model, optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q0, "q",
                    fixed_qpos, sphere_set, margin, damping, max_iters, posture_weight, q_ref, collision_weight, pair_weight, link_names,
                    target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits)


def robot_resolve_self_collision(robot, qpos0, sphere_set: SphereSet, margin, damping=_REQUIRED, max_iters=_REQUIRED, posture_weight=None,
                                 q_ref=None, collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None, target_rot=None,
                                 pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None):
    """The same for a full robot qpos (B, robot.dof) in dof order; every joint is a column of its own, limits (robot.dof, 2)."""
    return _resolve(robot.sphere_model, robot.dof, 0, robot.kin, robot, qpos0, "qpos", None, sphere_set, margin, damping, max_iters,
                    posture_weight, q_ref, collision_weight, pair_weight, link_names, target_pos, target_rot, pos_weight, rot_weight, tol,
                    max_step, limits)


# ---- obstacles: the robot's spheres against posed primitives outside the robot (include/dexr_obstacles.h) -------------------------
class ObstacleSet:
    """1 .. 64 primitives in an obstacle frame: plain data, immutable, hashable by content.

    kinds   (M,) of _lib.OBSTACLE_SPHERE / OBSTACLE_CAPSULE / OBSTACLE_BOX / OBSTACLE_HALFSPACE
    params  (M, 16) float64, per kind (the rest zeros):
              sphere      centre (3), radius >= 0
              capsule     end a (3), end b (3), radius >= 0
              box         centre (3), half extents (3) > 0, rotation (9, row-major, box axes -> obstacle frame, orthonormal to 1e-6)
              half-space  normal (3, unit to 1e-6), offset: the solid is n . y <= offset

    Built with `ObstacleSet.spheres / capsules / boxes / half_spaces`; `a + b` (or `ObstacleSet.concat`) puts sets together, the
    primitives of `a` first.  The rules are those of dexr_obstacle_set_create; a broken one is a ValueError.  The device tables of
    a set are made at its first use and kept with it (`device_set`)."""

    def __init__(self, kinds, params):
        k = np.array(kinds, dtype=np.int64).reshape(-1)
        p = np.array(params, dtype=np.float64)
        M = len(k)
        if not 1 <= M <= _lib.OBSTACLE_MAX:
            raise ValueError(f"an obstacle set holds 1..{_lib.OBSTACLE_MAX} primitives, got {M}")
        if p.shape != (M, _lib.OBSTACLE_PARAMS):
            raise ValueError(f"{M} kinds name {M} primitives: params must have shape ({M}, {_lib.OBSTACLE_PARAMS}), got {p.shape}")
        if ((k < _lib.OBSTACLE_SPHERE) | (k > _lib.OBSTACLE_HALFSPACE)).any():
            raise ValueError(f"kinds must be one of {_lib.OBSTACLE_SPHERE} (sphere), {_lib.OBSTACLE_CAPSULE} (capsule), "
                             f"{_lib.OBSTACLE_BOX} (box), {_lib.OBSTACLE_HALFSPACE} (half-space)")
        if not np.isfinite(p).all():
            raise ValueError("obstacle parameters must be finite")
        tol = 1e-6
        for m in range(M):
            v = p[m]
            if k[m] in (_lib.OBSTACLE_SPHERE, _lib.OBSTACLE_CAPSULE):
                r = v[3] if k[m] == _lib.OBSTACLE_SPHERE else v[6]
                if r < 0:
                    raise ValueError(f"primitive {m}: the radius must be >= 0, got {r}")
            elif k[m] == _lib.OBSTACLE_BOX:
                if not (v[3:6] > 0).all():
                    raise ValueError(f"primitive {m}: the half extents must be > 0, got {v[3:6].tolist()}")
                R = v[6:15].reshape(3, 3)
                if np.abs(R.T @ R - np.eye(3)).max() > tol:
                    raise ValueError(f"primitive {m}: the box rotation is not orthonormal to {tol}")
            elif abs(np.linalg.norm(v[:3]) - 1.0) > tol:
                raise ValueError(f"primitive {m}: the half-space normal is not unit to {tol}")
        k = k.astype(np.int32)
        for a in (k, p):
            a.setflags(write=False)
        self.kinds, self.params = k, p
        self._key = (k.tobytes(), p.tobytes())
        self._device_sets = {}

    @staticmethod
    def _rows(kind, blocks, n_name):
        """(M, 16) from per-primitive blocks [(name, array, width)], M read from the first."""
        first = np.array(blocks[0][1], dtype=np.float64)
        M = first.shape[0] if first.ndim >= 1 else 0
        p = np.zeros((M, _lib.OBSTACLE_PARAMS))
        o = 0
        for name, a, width in blocks:
            a = np.array(a, dtype=np.float64)
            want = (M,) if width == 1 else ((M, 3, 3) if width == 9 else (M, width))
            if a.shape != want or M == 0:
                raise ValueError(f"{name} must have shape {('M',) + want[1:]} with one row per {n_name}, got {a.shape}")
            p[:, o:o + width] = a.reshape(M, width)
            o += width
        return ObstacleSet(np.full(M, kind), p)

    @classmethod
    def spheres(cls, centers, radii):
        """centers (M, 3), radii (M,)."""
        return cls._rows(_lib.OBSTACLE_SPHERE, [("centers", centers, 3), ("radii", radii, 1)], "sphere")

    @classmethod
    def capsules(cls, a, b, radii):
        """the two ends a, b (M, 3) of each axis, radii (M,); a == b is a sphere."""
        return cls._rows(_lib.OBSTACLE_CAPSULE, [("a", a, 3), ("b", b, 3), ("radii", radii, 1)], "capsule")

    @classmethod
    def boxes(cls, centers, half_extents, rotations=None):
        """centers (M, 3), half_extents (M, 3) > 0, rotations (M, 3, 3) box axes -> obstacle frame, or None: axis-aligned."""
        if rotations is None:
            n = np.array(centers, dtype=np.float64)
            rotations = np.broadcast_to(np.eye(3), (n.shape[0] if n.ndim >= 1 else 0, 3, 3))
        return cls._rows(_lib.OBSTACLE_BOX, [("centers", centers, 3), ("half_extents", half_extents, 3), ("rotations", rotations, 9)], "box")

    @classmethod
    def half_spaces(cls, normals, offsets):
        """unit normals (M, 3) pointing out of the solid, offsets (M,): the free side is n . y > offset."""
        return cls._rows(_lib.OBSTACLE_HALFSPACE, [("normals", normals, 3), ("offsets", offsets, 1)], "half-space")

    @classmethod
    def concat(cls, *sets):
        if not sets or not all(isinstance(s, ObstacleSet) for s in sets):
            raise ValueError("concat takes one or more ObstacleSet")
        return cls(np.concatenate([s.kinds for s in sets]), np.concatenate([s.params for s in sets]))

    def __add__(self, other):
        if not isinstance(other, ObstacleSet):
            return NotImplemented
        return ObstacleSet.concat(self, other)

    @property
    def n_prim(self) -> int:
        return len(self.kinds)

    def device_set(self, device_index: int = 0) -> _lib.ObstacleSet:
        """the set's tables on a device (made with that device current), cached with the set."""
        if device_index not in self._device_sets:
            self._device_sets[device_index] = _lib.ObstacleSet(self.kinds, self.params)
        return self._device_sets[device_index]

    def __hash__(self):
        return hash(self._key)

    def __eq__(self, other):
        return isinstance(other, ObstacleSet) and self._key == other._key

    def __repr__(self):
        names = ("spheres", "capsules", "boxes", "half-spaces")
        return "ObstacleSet(" + ", ".join(f"{int((self.kinds == i).sum())} {n}" for i, n in enumerate(names) if (self.kinds == i).any()) + ")"


def _check_obstacles(n_in, n_fixed, kin, robot, q, fixed_qpos, sphere_set, obstacles, obstacle_pos, obstacle_rot, what, margin=None,
                     prim_weight=None, penalty=False, grid=False):
    """Every argument rule in the order of `_check` -- the sphere set, the links, the pairs, the obstacle set (with `grid` an
    SdfGrid), the scalars, then types, dtypes and shapes, and last the device -- before anything touches the GPU."""
    import torch

    if not isinstance(sphere_set, SphereSet):
        raise ValueError("sphere_set must be a collision.SphereSet")
    for n in sphere_set.table_links:
        kin.body_frame_index(n)  # ValueError on an unknown link
    pairs = _resolved_pairs(robot, sphere_set)
    if grid and not isinstance(obstacles, SdfGrid):
        raise ValueError("grid must be a collision.SdfGrid")
    if not grid and not isinstance(obstacles, ObstacleSet):
        raise ValueError("obstacles must be a collision.ObstacleSet")
    if penalty and (isinstance(margin, bool) or not isinstance(margin, (int, float)) or not math.isfinite(margin) or margin < 0):
        raise ValueError(f"margin must be a finite Python float >= 0, got {margin!r}")
    B = q.shape[0] if isinstance(q, torch.Tensor) and q.ndim == 2 else None
    named = [(n, t, s) for n, t, s in (("obstacle_pos", obstacle_pos, (B, 3)), ("obstacle_rot", obstacle_rot, (B, 3, 3))) if t is not None]
    if penalty and prim_weight is not None:
        named.append(("prim_weight", prim_weight, (obstacles.n_prim,)))
    for name, t, _ in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    for name, t, _ in named:
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    for name, t, shape in named:
        if (B is not None or shape[0] is not None) and tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    _check_poses(n_in, n_fixed, q, fixed_qpos, sphere_set.table_links, what=what)  # (ends with the device)
    for name, t, _ in named:
        if t.device != q.device:
            raise ValueError(f"{name} is on {t.device}, {what} on {q.device}: all tensors must be on one CUDA device")
    return pairs


def _obstacle_pose(obstacle_pos, obstacle_rot):
    c = lambda a: None if a is None else a.detach().contiguous()  # noqa: E731
    return c(obstacle_pos), c(obstacle_rot)


def _obstacle_distances(model, obstacles, x, fixed_qpos, obstacle_pos, obstacle_rot, nearest):
    import torch

    B = x.shape[0]
    xc, fixed = _inputs(x, fixed_qpos)
    pos, rot = _obstacle_pose(obstacle_pos, obstacle_rot)
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x.device):
        dist = torch.empty((B, model.n_sphere), dtype=torch.float32, device=x.device)
        near = torch.empty((B, model.n_sphere), dtype=torch.int32, device=x.device) if nearest else None
        if B > 0:
            model.obstacle_distances_dev(obstacles.device_set(torch.cuda.current_device()), B, xc.data_ptr(), ptr(fixed), dist.data_ptr(),
                                         ptr(near), ptr(pos), ptr(rot), stream=torch.cuda.current_stream(x.device).cuda_stream)
    return (dist, near) if nearest else dist


def _obstacle_penalty(model, obstacles, x, fixed_qpos, margin, prim_weight, obstacle_pos, obstacle_rot, want_grad=True, want_wrench=False):
    """one launch -> (E (B,), grad (B, n_in) or None, wrench (B, 6) or None)."""
    import torch

    B = x.shape[0]
    xc, fixed = _inputs(x, fixed_qpos)
    pos, rot = _obstacle_pose(obstacle_pos, obstacle_rot)
    w = None if prim_weight is None else prim_weight.detach().contiguous()
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x.device):
        e = torch.empty((B,), dtype=torch.float32, device=x.device)
        g = torch.empty((B, model.n_in), dtype=torch.float32, device=x.device) if want_grad else None
        wr = torch.empty((B, 6), dtype=torch.float32, device=x.device) if want_wrench else None
        if B > 0:
            model.obstacle_penalty_dev(obstacles.device_set(torch.cuda.current_device()), B, xc.data_ptr(), ptr(fixed), float(margin), ptr(w),
                                       e.data_ptr(), ptr(g), ptr(wr), ptr(pos), ptr(rot), stream=torch.cuda.current_stream(x.device).cuda_stream)
    return e, g, wr


def obstacle_distances(optimizer, q, sphere_set: SphereSet, obstacles: ObstacleSet, obstacle_pos=None, obstacle_rot=None, fixed_qpos=None,
                       nearest: bool = False):
    """Signed distance of every sphere of the set to the nearest primitive of `obstacles` at the optimiser's variables: q
    (B, n_opt) float32 CUDA, obstacle_pos (B, 3) and obstacle_rot (B, 3, 3) float32 the world pose of the obstacle frame per
    frame, or None (zero translation / identity: a shared scene) -> dist (B, S) float32 in the set's sphere order, negative
    where a sphere penetrates; with `nearest=True` -> (dist, nearest (B, S) int32), the first primitive that attains the
    minimum.  No autograd graph."""
    pairs = _check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos, sphere_set,
                             obstacles, obstacle_pos, obstacle_rot, "q")
    return _obstacle_distances(optimizer.sphere_model(sphere_set, pairs), obstacles, q, fixed_qpos, obstacle_pos, obstacle_rot, nearest)


def obstacle_penalty(optimizer, q, sphere_set: SphereSet, obstacles: ObstacleSet, margin, obstacle_pos=None, obstacle_rot=None,
                     prim_weight=None, fixed_qpos=None, wrench: bool = False):
    """(E (B,), grad_q (B, n_opt)) float32 from ONE launch: E = sum_s sum_m w_m max(0, margin - d_sm)^2 over every sphere s of
    the set and every primitive m, d_sm the signed distance of the sphere's surface to the primitive, and its gradient in q.
    margin: a finite Python float >= 0 (metres); prim_weight (M,) float32 >= 0 or None (1), shared by the batch; obstacle_pos,
    obstacle_rot as in `obstacle_distances`.  With `wrench=True` -> (E, grad_q, wrench (B, 6)): dE/d(obstacle translation) and
    dE/d(a world-aligned small rotation of the obstacle about its origin).  No autograd graph: `autograd.obstacle_penalty` is
    the same launch with one."""
    pairs = _check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos, sphere_set,
                             obstacles, obstacle_pos, obstacle_rot, "q", margin, prim_weight, penalty=True)
    e, g, wr = _obstacle_penalty(optimizer.sphere_model(sphere_set, pairs), obstacles, q, fixed_qpos, margin, prim_weight, obstacle_pos,
                                 obstacle_rot, want_wrench=wrench)
    return (e, g, wr) if wrench else (e, g)


def robot_obstacle_distances(robot, qpos, sphere_set: SphereSet, obstacles: ObstacleSet, obstacle_pos=None, obstacle_rot=None,
                             nearest: bool = False):
    """The same for a full robot qpos (B, robot.dof) in dof order; every joint is a column of its own."""
    pairs = _check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, obstacles, obstacle_pos, obstacle_rot, "qpos")
    return _obstacle_distances(robot.sphere_model(sphere_set, pairs), obstacles, qpos, None, obstacle_pos, obstacle_rot, nearest)


def robot_obstacle_penalty(robot, qpos, sphere_set: SphereSet, obstacles: ObstacleSet, margin, obstacle_pos=None, obstacle_rot=None,
                           prim_weight=None, wrench: bool = False):
    """(E (B,), grad_qpos (B, robot.dof)[, wrench (B, 6)]) for a full robot qpos in dof order."""
    pairs = _check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, obstacles, obstacle_pos, obstacle_rot, "qpos", margin,
                             prim_weight, penalty=True)
    e, g, wr = _obstacle_penalty(robot.sphere_model(sphere_set, pairs), obstacles, qpos, None, margin, prim_weight, obstacle_pos, obstacle_rot,
                                 want_wrench=wrench)
    return (e, g, wr) if wrench else (e, g)


# ---- a sampled signed-distance field: the robot's spheres against a mesh, a scan, a depth fusion (include/dexr_sdf_grid.h) -------------
def _primitive_sdf(kind, v, y):
    """the signed distance of the points y (..., 3) to one primitive of an ObstacleSet, the formulas of include/dexr_obstacles.h"""
    if kind == _lib.OBSTACLE_HALFSPACE:
        return y @ v[:3] - v[3]
    if kind == _lib.OBSTACLE_BOX:
        q = np.abs((y - v[:3]) @ v[6:15].reshape(3, 3)) - v[3:6]
        mx = q.max(-1)
        return np.where(mx <= 0, mx, np.linalg.norm(np.maximum(q, 0.0), axis=-1))
    if kind == _lib.OBSTACLE_CAPSULE:
        a, ab, r = v[:3], v[3:6] - v[:3], v[6]
        l2 = ab @ ab
        t = np.clip((y - a) @ ab / l2, 0.0, 1.0) if l2 > 0 else np.zeros(y.shape[:-1])
        return np.linalg.norm(y - (a + t[..., None] * ab), axis=-1) - r
    return np.linalg.norm(y - v[:3], axis=-1) - v[3]


class TriangleMesh:
    """A triangle mesh of an obstacle frame: plain data, immutable, hashable by content.

    vertices  (V, 3) float64, finite, 1 .. 2^20 of them
    faces     (T, 3) int32 vertex indices, 1 .. 2^20 of them; a triangle whose cross product (b - a) x (c - a) is exactly zero in
              float64 is refused, or with `drop_degenerate=True` removed first

    The rules are those of dexr_mesh_create (include/dexr_mesh_sdf.h); a broken one is a ValueError.  The sign of a distance comes
    from the generalised winding number: it is right for a closed mesh whose normals (b - a) x (c - a) point outwards
    (`is_closed` and `volume > 0`), and a majority vote on an open one.  `SdfGrid.from_mesh` samples the mesh into a grid,
    `mesh_distances` gives the distances of arbitrary points.  The device tables of a mesh are made at its first use and kept with
    it (`device_mesh`)."""

    def __init__(self, vertices, faces, drop_degenerate: bool = False):
        v = np.array(vertices, dtype=np.float64)
        f = np.array(faces)
        if v.ndim != 2 or v.shape[1] != 3:
            raise ValueError(f"vertices must have shape (V, 3), got {v.shape}")
        if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
            raise ValueError(f"faces must be integers of shape (T, 3), got {f.dtype} {f.shape}")
        f = f.astype(np.int64)
        if not 1 <= len(v) <= _lib.MESH_MAX_VERTICES:
            raise ValueError(f"a mesh holds 1..{_lib.MESH_MAX_VERTICES} vertices, got {len(v)}")
        if len(f) and (f.min() < 0 or f.max() >= len(v)):
            raise ValueError(f"a face index is outside 0..{len(v) - 1}")
        if not np.isfinite(v).all():
            raise ValueError("the vertices must be finite")
        if len(f):
            a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
            with np.errstate(over="ignore", invalid="ignore"):
                flat = (np.cross(b - a, c - a) == 0.0).all(1)
            if flat.any():
                if not drop_degenerate:
                    raise ValueError(f"triangle {int(np.flatnonzero(flat)[0])} has no area ({int(flat.sum())} such): drop_degenerate=True removes them")
                f = f[~flat]
        if not 1 <= len(f) <= _lib.MESH_MAX_TRIANGLES:
            raise ValueError(f"a mesh holds 1..{_lib.MESH_MAX_TRIANGLES} triangles, got {len(f)}")
        f = np.ascontiguousarray(f.astype(np.int32))
        for a in (v, f):
            a.setflags(write=False)
        self.vertices, self.faces = v, f
        self._key = (v.shape, f.shape, v.tobytes(), f.tobytes())
        self._hash = hash(self._key)
        self._device_meshes = {}

    @property
    def n_vertex(self) -> int:
        return len(self.vertices)

    @property
    def n_triangle(self) -> int:
        return len(self.faces)

    @property
    def bounds(self) -> np.ndarray:
        """(2, 3): the smallest and the largest coordinate of all vertices per axis."""
        return np.stack([self.vertices.min(0), self.vertices.max(0)])

    @property
    def is_closed(self) -> bool:
        """every undirected edge belongs to exactly two triangles, which traverse it in opposite directions."""
        f = self.faces.astype(np.int64)
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        V = self.n_vertex
        directed = e[:, 0] * V + e[:, 1]
        if len(np.unique(directed)) != len(directed):  # a directed edge twice: two triangles run along it the same way
            return False
        lo, hi = e.min(1), e.max(1)
        _, counts = np.unique(lo * V + hi, return_counts=True)
        return bool((counts == 2).all())

    @property
    def volume(self) -> float:
        """the signed sum of a . (b x c) / 6: the enclosed volume of a closed mesh with outward normals, negative inside out."""
        a, b, c = (self.vertices[self.faces[:, k]] for k in range(3))
        return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)

    def device_mesh(self, device_index: int = 0) -> _lib.TriangleMesh:
        """the mesh's records on a device (made with that device current), cached with the mesh."""
        if device_index not in self._device_meshes:
            self._device_meshes[device_index] = _lib.TriangleMesh(self.vertices, self.faces)
        return self._device_meshes[device_index]

    def __hash__(self):
        return self._hash

    def __eq__(self, other):
        return isinstance(other, TriangleMesh) and self._key == other._key

    def __repr__(self):
        return f"TriangleMesh({self.n_vertex} vertices, {self.n_triangle} triangles)"


def mesh_distances(mesh: TriangleMesh, points, winding: bool = False):
    """Signed distances of points to a mesh: points (..., 3) float32 CUDA -> dist of shape points.shape[:-1], float32, negative
    inside; with `winding=True` -> (dist, w), w the generalised winding number behind the sign (include/dexr_mesh_sdf.h).  Brute
    force on the current stream, points x triangles pairs.  No autograd graph."""
    import torch

    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a collision.TriangleMesh")
    if not isinstance(points, torch.Tensor):
        raise ValueError("points must be a torch tensor")
    if points.dtype != torch.float32:
        raise ValueError(f"points must be float32, got {points.dtype}")
    if points.ndim < 1 or points.shape[-1] != 3:
        raise ValueError(f"points must have shape (..., 3), got {tuple(points.shape)}")
    if not points.is_cuda:
        raise ValueError("points must be a CUDA tensor")
    pc = points.detach().contiguous()
    P = pc.numel() // 3
    with torch.cuda.device(points.device):
        dist = torch.empty(points.shape[:-1], dtype=torch.float32, device=points.device)
        w = torch.empty(points.shape[:-1], dtype=torch.float32, device=points.device) if winding else None
        if P > 0:
            mesh.device_mesh(torch.cuda.current_device()).distances_dev(P, pc.data_ptr(), dist.data_ptr(), 0 if w is None else w.data_ptr(),
                                                                        stream=torch.cuda.current_stream(points.device).cuda_stream)
    return (dist, w) if winding else dist


class SdfGrid:
    """A signed-distance field sampled on a regular grid of an obstacle frame: plain data, immutable, hashable by content.

    values   (nx, ny, nz) float32 samples in C order (kept as float32: what the device holds), each dimension 2 .. 1024, at most
             2^24 samples, all finite
    origin   (3,) or a scalar: the position of sample (0, 0, 0) in the obstacle frame, finite
    spacing  (3,) or a scalar: the distance between samples along each axis, finite and > 0 (it may differ per axis)

    Sample (ix, iy, iz) sits at origin + (ix, iy, iz) * spacing.  Between samples the field is the trilinear interpolant, outside
    the grid's box it is the interpolant at the nearest point of the box plus the distance to the box (include/dexr_sdf_grid.h).
    The rules are those of dexr_sdf_grid_create; a broken one is a ValueError.  `SdfGrid.from_obstacles` samples an ObstacleSet.
    The device copy of a grid is made at its first use and kept with it (`device_grid`)."""

    def __init__(self, values, origin, spacing):
        with np.errstate(over="ignore"):  # (a value beyond float32 becomes an infinity, which is refused below)
            v = np.array(values, dtype=np.float32)
        if v.ndim != 3:
            raise ValueError(f"values must have shape (nx, ny, nz), got {v.shape}")
        try:
            o = np.array(np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,)))
            h = np.array(np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,)))
        except ValueError:
            raise ValueError("origin and spacing must each be a scalar or have shape (3,)") from None
        lo, hi = _lib.SDF_GRID_MIN_DIM, _lib.SDF_GRID_MAX_DIM
        if min(v.shape) < lo or max(v.shape) > hi:
            raise ValueError(f"every dimension of a grid is {lo}..{hi} samples, got {v.shape}")
        if v.size > _lib.SDF_GRID_MAX_SAMPLES:
            raise ValueError(f"a grid holds at most {_lib.SDF_GRID_MAX_SAMPLES} samples, got {v.size}")
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            inv_ok = np.isfinite(1.0 / h).all()
        if not (np.isfinite(h).all() and (h > 0).all() and inv_ok):
            raise ValueError(f"spacing must be finite and > 0, got {h.tolist()}")
        if not np.isfinite(o).all():
            raise ValueError(f"origin must be finite, got {o.tolist()}")
        if not np.isfinite(v).all():
            raise ValueError("the samples must be finite")
        v = np.ascontiguousarray(v)
        for a in (v, o, h):
            a.setflags(write=False)
        self.values, self.origin, self.spacing = v, o, h
        self._key = (v.shape, v.tobytes(), o.tobytes(), h.tobytes())
        self._hash = hash(self._key)
        self._device_grids = {}

    @classmethod
    def from_obstacles(cls, obstacle_set: ObstacleSet, origin, spacing, shape):
        """the union of an ObstacleSet sampled in float64 -- the minimum over its primitives of the signed distances of
        include/dexr_obstacles.h -- on `shape` = (nx, ny, nz) (or one int for all three) samples from `origin` at `spacing`, rounded
        to float32: a grid of a known shape without a mesh library."""
        if not isinstance(obstacle_set, ObstacleSet):
            raise ValueError("obstacle_set must be a collision.ObstacleSet")
        try:
            n = tuple(int(k) for k in np.broadcast_to(np.asarray(shape), (3,)))
            o = np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,))
            h = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
        except (ValueError, TypeError):
            raise ValueError("shape, origin and spacing must each be a scalar or have shape (3,)") from None
        if min(n) < _lib.SDF_GRID_MIN_DIM or max(n) > _lib.SDF_GRID_MAX_DIM or n[0] * n[1] * n[2] > _lib.SDF_GRID_MAX_SAMPLES:
            raise ValueError(f"every dimension of a grid is {_lib.SDF_GRID_MIN_DIM}..{_lib.SDF_GRID_MAX_DIM} samples and there are at most "
                             f"{_lib.SDF_GRID_MAX_SAMPLES}, got {n}")
        ax = [o[a] + np.arange(n[a]) * h[a] for a in range(3)]
        values = np.empty(n, dtype=np.float32)
        for ix in range(n[0]):  # a slab at a time: the memory of one slab per primitive, whatever the grid
            y = np.stack(np.broadcast_arrays(ax[0][ix], ax[1][:, None], ax[2][None, :]), -1)
            d = np.full(n[1:], np.inf)
            for kind, v in zip(obstacle_set.kinds, obstacle_set.params):
                d = np.minimum(d, _primitive_sdf(kind, v, y))
            values[ix] = d
        return cls(values, o, h)

    @classmethod
    def from_mesh(cls, mesh: TriangleMesh, origin=None, spacing=_REQUIRED, shape=None, padding=0.0, precision="float64",
                  allow_open: bool = False):
        """the signed distance to a TriangleMesh (include/dexr_mesh_sdf.h) sampled on the device, brute force: every sample against
        every triangle.  `spacing` is required (a scalar or (3,)).  With `origin` and `shape` both None the box is fitted to the mesh:
        origin = lo - padding and shape = ceil((hi - lo + 2 padding) / spacing) + 1 per axis, lo and hi the mesh's bounds; otherwise
        both are given, as in `from_obstacles`.  precision "float64": float64 arithmetic rounded to float32 at the store, the contract
        of `from_obstacles`; "float32": float32 arithmetic through a torch buffer on the current CUDA device.  The sign is right
        only for a closed mesh with outward normals: a mesh with `is_closed == False` or `volume <= 0` is a ValueError unless
        `allow_open=True` (an inside-out mesh would give a field that is positive everywhere)."""
        if not isinstance(mesh, TriangleMesh):
            raise ValueError("mesh must be a collision.TriangleMesh")
        if spacing is _REQUIRED:
            raise ValueError("spacing is required")
        if precision not in ("float64", "float32"):
            raise ValueError(f"precision must be 'float64' or 'float32', got {precision!r}")
        if (origin is None) != (shape is None):
            raise ValueError("origin and shape must both be given or both be None (None: the box is fitted to the mesh)")
        try:
            h = np.array(np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,)))
            pad = float(padding)
        except (ValueError, TypeError):
            raise ValueError("spacing must be a scalar or have shape (3,), padding a number") from None
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            inv_ok = np.isfinite(1.0 / h).all()
        if not (np.isfinite(h).all() and (h > 0).all() and inv_ok):
            raise ValueError(f"spacing must be finite and > 0, got {h.tolist()}")
        if not (math.isfinite(pad) and pad >= 0):
            raise ValueError(f"padding must be finite and >= 0, got {padding}")
        if origin is None:
            lo, hi = mesh.bounds
            o = lo - pad
            cells = np.ceil((hi - lo + 2 * pad) / h)
            if not (np.isfinite(cells).all() and (cells < 2 ** 31).all()):
                raise ValueError(f"the fitted box needs {cells.tolist()} cells per axis")
            n = tuple(int(k) + 1 for k in cells)
        else:
            try:
                n = tuple(int(k) for k in np.broadcast_to(np.asarray(shape), (3,)))
                o = np.array(np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,)))
            except (ValueError, TypeError):
                raise ValueError("shape and origin must each be a scalar or have shape (3,)") from None
        if min(n) < _lib.SDF_GRID_MIN_DIM or max(n) > _lib.SDF_GRID_MAX_DIM or n[0] * n[1] * n[2] > _lib.SDF_GRID_MAX_SAMPLES:
            raise ValueError(f"every dimension of a grid is {_lib.SDF_GRID_MIN_DIM}..{_lib.SDF_GRID_MAX_DIM} samples and there are at most "
                             f"{_lib.SDF_GRID_MAX_SAMPLES}, got {n}")
        if not np.isfinite(o).all():
            raise ValueError(f"origin must be finite, got {o.tolist()}")
        if not allow_open:
            if not mesh.is_closed:
                raise ValueError("the mesh is not closed (an edge that does not belong to exactly two triangles of opposite direction): its "
                                 "winding number is fractional and the sign only a majority vote; allow_open=True accepts that")
            if not mesh.volume > 0:
                raise ValueError(f"the mesh has volume {mesh.volume:g} <= 0: its triangles are oriented inside out and every sample would be "
                                 "positive; flip the faces, or allow_open=True accepts that")
        if precision == "float64":
            values = mesh.device_mesh().sample_grid(n, o, h)
        else:
            import torch

            with torch.cuda.device(torch.cuda.current_device()):
                buf = torch.empty(n, dtype=torch.float32, device="cuda")
                mesh.device_mesh(torch.cuda.current_device()).sample_grid_dev(n, o, h, buf.data_ptr(),
                                                                              stream=torch.cuda.current_stream().cuda_stream)
                values = buf.cpu().numpy()
        return cls(values, o, h)

    @classmethod
    def from_points(cls, points, origin, spacing, shape, min_points=1, radius=None, max_distance=None, signed=False):
        """the unsigned distance to a point cloud (include/dexr_distance_transform.h): `DeviceSdfGrid.from_points` computed on the
        device of `points` and returned as a host-owned, immutable grid, as `from_mesh(precision="float32")` does."""
        return DeviceSdfGrid.from_points(points, origin, spacing, shape, min_points, radius, max_distance, signed).to_host()

    @classmethod
    def from_occupancy(cls, occ, origin, spacing, signed=True, radius=None, max_distance=None):
        """the distance to the occupied voxels of a uint8 occupancy map, signed by default: `DeviceSdfGrid.from_occupancy`
        computed on the device of `occ` and returned as a host-owned, immutable grid."""
        return DeviceSdfGrid.from_occupancy(occ, origin, spacing, signed, radius, max_distance).to_host()

    @property
    def shape(self):
        return self.values.shape

    def device_grid(self, device_index: int = 0) -> _lib.SdfGrid:
        """the grid's samples on a device (made with that device current), cached with the grid."""
        if device_index not in self._device_grids:
            self._device_grids[device_index] = _lib.SdfGrid(self.values, self.origin, self.spacing)
        return self._device_grids[device_index]

    def __hash__(self):
        return self._hash

    def __eq__(self, other):
        return isinstance(other, SdfGrid) and self._key == other._key

    def __repr__(self):
        return f"SdfGrid({'x'.join(str(k) for k in self.shape)} samples, origin {self.origin.tolist()}, spacing {self.spacing.tolist()})"


def _edt_grid_rules(shape, origin, spacing):
    """the grid rules of include/dexr_distance_transform.h -> (n (3 ints), origin (3,) float64, h float): ONE spacing"""
    try:
        ns = np.broadcast_to(np.asarray(shape), (3,))
        o = np.array(np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,)))
        hs = np.array(np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,)))
    except (ValueError, TypeError):
        raise ValueError("shape, origin and spacing must each be a scalar or have shape (3,)") from None
    if ns.dtype.kind not in "iu":
        raise ValueError(f"shape must be integers, got {np.asarray(shape).tolist()}")
    n = tuple(int(k) for k in ns)
    if min(n) < _lib.SDF_GRID_MIN_DIM or max(n) > _lib.SDF_GRID_MAX_DIM or n[0] * n[1] * n[2] > _lib.SDF_GRID_MAX_SAMPLES:
        raise ValueError(f"every dimension of a grid is {_lib.SDF_GRID_MIN_DIM}..{_lib.SDF_GRID_MAX_DIM} samples and there are at most "
                         f"{_lib.SDF_GRID_MAX_SAMPLES}, got {n}")
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        inv_ok = np.isfinite(1.0 / hs).all()
    if not (np.isfinite(hs).all() and (hs > 0).all() and inv_ok):
        raise ValueError(f"spacing must be finite and > 0, got {hs.tolist()}")
    if not (hs[0] == hs[1] == hs[2]):
        raise ValueError(f"a distance transform needs ONE spacing for the three axes, got {hs.tolist()}")
    if not np.isfinite(o).all():
        raise ValueError(f"origin must be finite, got {o.tolist()}")
    return n, o, float(hs[0])


def _edt_scalars(n, h, min_points, radius, max_distance, signed, cloud):
    """the scalar rules -> (min_points, radius, max_distance) with the defaults filled in"""
    if cloud and signed:
        raise ValueError("signed=True needs an occupancy map: a point cloud has no inside")
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or min_points < 1:
        raise ValueError(f"min_points must be an integer >= 1, got {min_points!r}")
    if signed:
        if radius is not None:
            raise ValueError("the signed form has no radius: its surface sits h / 2 from the voxel centres")
        radius = 0.0
    elif radius is None:
        radius = h * math.sqrt(3.0) / 2.0
    if max_distance is None:
        max_distance = h * math.sqrt(sum((k - 1) ** 2 for k in n))  # the diagonal of the grid's box
    try:
        radius, max_distance = float(radius), float(max_distance)
    except (TypeError, ValueError):
        raise ValueError("radius and max_distance must be numbers") from None
    if not (math.isfinite(radius) and radius >= 0):
        raise ValueError(f"radius must be finite and >= 0, got {radius}")
    if not (math.isfinite(max_distance) and max_distance > 0):
        raise ValueError(f"max_distance must be finite and > 0, got {max_distance}")
    return int(min_points), radius, max_distance


def _edt_tensor_rules(t, name, dtype, shape_text, shape_ok):
    """type, dtype, shape, layout, and last the device"""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not shape_ok(tuple(t.shape)):
        raise ValueError(f"{name} must have shape {shape_text}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA tensor, got one on {t.device}")


def _edt_points_rules(points):
    import torch

    _edt_tensor_rules(points, "points", torch.float32, "(N, 3)", lambda s: len(s) == 2 and s[1] == 3 and s[0] <= _lib.EDT_MAX_POINTS)


class DeviceSdfGrid(SdfGrid):
    """An `SdfGrid` whose samples live on ONE CUDA device and may be rewritten in place: the grid of a scene that changes per frame
    (include/dexr_sdf_grid_dev.h, include/dexr_distance_transform.h).  `grid_distances`, `grid_penalty`, `autograd.grid_penalty`,
    `resolve_grid_collisions` and a `SceneBody` of `resolve_scene_collisions` take it like any SdfGrid, through `device_grid`, with
    their kernels unchanged; `fit_spheres` refuses it, because it reads the samples on the host.

    It has `shape`, `origin` (3,) and `spacing` (3,; one value three times), is hashed and compared by IDENTITY (its content
    changes), and is bound to the device it was made on: `device_grid(i)` for another device is a ValueError.  `.values` raises;
    `to_host()` returns an ordinary immutable SdfGrid of the samples as they are after the work enqueued so far on the current
    stream, and is the only method that synchronises.

    `empty` makes a grid of zeros on the current CUDA device, `from_points` and `from_occupancy` one on the device of their
    tensor; all of them and the in-place `update_from_points` / `update_from_occupancy` run on the current stream of that device,
    allocate the workspace of the transform once, and make no host copy.  Updates and consumers are ordered by the stream they
    are enqueued on: on one stream an update followed by `grid_penalty` needs no synchronise; across streams the ordering is the
    caller's.  A consumer reads the samples when its kernel RUNS: in particular the backward of `autograd.grid_penalty` reads
    whatever the grid holds when backward runs, not what it held at the forward.

    The fields are those of include/dexr_distance_transform.h.  A cloud (points (N, 3) float32 CUDA, contiguous) gives the unsigned
    distance to the voxels that hold at least `min_points` points, minus `radius` (default h sqrt(3) / 2: never larger than the
    true distance to the nearest kept point; 0: the raw distance between voxel centres), clamped at `max_distance` (default the
    diagonal of the grid's box).  An occupancy map (nx, ny, nz) uint8 CUDA gives, with signed=True, a field that is negative
    inside the occupied voxels with its surface halfway between a free and an occupied voxel, and with signed=False the
    unsigned form.  Every sample is finite whatever the input."""

    def __init__(self, shape, origin, spacing, device=None):
        n, o, h = _edt_grid_rules(shape, origin, spacing)
        import torch

        self._shape, self._h = n, h
        self.origin, self.spacing = o, np.full(3, h)
        for a in (self.origin, self.spacing):
            a.setflags(write=False)
        self._device = torch.cuda.current_device() if device is None else torch.device(device).index
        self._workspace = None
        with torch.cuda.device(self._device):
            self._grid = _lib.DeviceSdfGrid(n, o, self.spacing, 0, torch.cuda.current_stream().cuda_stream)

    @classmethod
    def empty(cls, shape, origin, spacing):
        """a grid of zeros on the current CUDA device"""
        return cls(shape, origin, spacing)

    @classmethod
    def from_points(cls, points, origin, spacing, shape, min_points=1, radius=None, max_distance=None, signed=False):
        n, _, h = _edt_grid_rules(shape, origin, spacing)
        _edt_scalars(n, h, min_points, radius, max_distance, signed, cloud=True)
        _edt_points_rules(points)
        g = cls(shape, origin, spacing, device=points.device)
        g.update_from_points(points, min_points, radius, max_distance)
        return g

    @classmethod
    def from_occupancy(cls, occ, origin, spacing, signed=True, radius=None, max_distance=None):
        import torch

        shape = tuple(occ.shape) if isinstance(occ, torch.Tensor) and occ.ndim == 3 else (2, 2, 2)  # (not a map: refused below)
        n, _, h = _edt_grid_rules(shape, origin, spacing)
        _edt_scalars(n, h, 1, radius, max_distance, signed, cloud=False)
        _edt_tensor_rules(occ, "occ", torch.uint8, "(nx, ny, nz)", lambda s: len(s) == 3)
        g = cls(shape, origin, spacing, device=occ.device)
        g.update_from_occupancy(occ, signed, radius, max_distance)
        return g

    def _launch(self, t, what, run):
        import torch

        if t.device.index != self._device:
            raise ValueError(f"{what} is on cuda:{t.device.index}, this DeviceSdfGrid lives on cuda:{self._device}")
        with torch.cuda.device(self._device):
            if self._workspace is None:
                self._workspace = torch.empty(_lib.edt_workspace_bytes(self._shape), dtype=torch.uint8, device="cuda")
            ws = self._workspace
            run(self._grid.values_ptr, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)

    def update_from_points(self, points, min_points=1, radius=None, max_distance=None, signed=False):
        """re-run the transform of a cloud into the same samples, on the current stream"""
        min_points, radius, max_distance = _edt_scalars(self._shape, self._h, min_points, radius, max_distance, signed, cloud=True)
        _edt_points_rules(points)
        self._launch(points, "points", lambda v, ws, nb, st: _lib.edt_points_dev(
            points.data_ptr() if points.shape[0] else 0, points.shape[0], self._shape, self.origin, self._h, min_points, radius, max_distance, v,
            workspace_ptr=ws, workspace_bytes=nb, stream=st))

    def update_from_occupancy(self, occ, signed=True, radius=None, max_distance=None):
        """re-run the transform of an occupancy map of the grid's shape into the same samples, on the current stream"""
        import torch

        _, radius, max_distance = _edt_scalars(self._shape, self._h, 1, radius, max_distance, signed, cloud=False)
        _edt_tensor_rules(occ, "occ", torch.uint8, str(self._shape), lambda s: s == self._shape)
        self._launch(occ, "occ", lambda v, ws, nb, st: _lib.edt_occupancy_dev(
            occ.data_ptr(), self._shape, self._h, signed, radius, max_distance, v, workspace_ptr=ws, workspace_bytes=nb, stream=st))

    def to_host(self) -> SdfGrid:
        """-> an immutable SdfGrid of the samples as they are after everything enqueued so far on the current stream; synchronises it"""
        import torch

        with torch.cuda.device(self._device):
            values = self._grid.download(torch.cuda.current_stream().cuda_stream)
        return SdfGrid(values, self.origin, self.spacing)

    @property
    def shape(self):
        return self._shape

    @property
    def device_index(self) -> int:
        return self._device

    @property
    def values(self):
        raise AttributeError("a DeviceSdfGrid keeps its samples on the device and they may change: to_host() returns an SdfGrid with .values")

    def device_grid(self, device_index: int = 0) -> _lib.SdfGrid:
        if device_index != self._device:
            raise ValueError(f"this DeviceSdfGrid lives on cuda:{self._device} and cannot serve cuda:{device_index}: make one there, or "
                             "use to_host() for a grid that any device can take")
        return self._grid

    __hash__ = object.__hash__

    def __eq__(self, other):
        return self is other

    def __repr__(self):
        return (f"DeviceSdfGrid({'x'.join(str(k) for k in self.shape)} samples on cuda:{self._device}, origin {self.origin.tolist()}, "
                f"spacing {self._h})")


class SphereFit:
    """What `fit_spheres` found in one grid: plain data.

    centers     (n, 3) float64 in the grid's frame: origin + samples * spacing
    radii       (n,) float64: -value at the centre's sample + inflate
    samples     (n, 3) the index triples of the centres' samples, in the order the greedy rounds took them
    gains       (n,) the interior samples each sphere was the first to cover
    n_interior  samples with a negative value;  n_covered  those inside some sphere;  coverage  their ratio (1.0 where there are none)"""

    def __init__(self, centers, radii, samples, gains, n_interior, n_covered):
        self.centers, self.radii, self.samples, self.gains = centers, radii, samples, gains
        self.n_interior, self.n_covered = int(n_interior), int(n_covered)
        self.coverage = self.n_covered / self.n_interior if self.n_interior else 1.0

    def __len__(self):
        return len(self.radii)

    def __repr__(self):
        return f"SphereFit({len(self)} spheres, {self.n_covered} of {self.n_interior} interior samples covered)"


def _fit_scalars(min_radius, inflate, coverage):
    try:
        min_radius, inflate, coverage = float(min_radius), float(inflate), float(coverage)
    except (TypeError, ValueError):
        raise ValueError("min_radius, inflate and coverage must be numbers") from None
    if not (math.isfinite(min_radius) and min_radius >= 0):
        raise ValueError(f"min_radius must be finite and >= 0, got {min_radius}")
    if not (math.isfinite(inflate) and inflate >= 0):
        raise ValueError(f"inflate must be finite and >= 0, got {inflate}")
    if not 0.0 <= coverage <= 1.0:
        raise ValueError(f"coverage must lie in 0..1, got {coverage}")
    return min_radius, inflate, coverage


def _fit_rules(grids, max_spheres, min_radius, inflate, coverage):
    """the argument rules of fit_spheres -> (list of grids, k (n,) int32, the three scalars as floats)"""
    if isinstance(grids, SdfGrid):
        grids = [grids]
    try:
        grids = list(grids)
    except TypeError:
        raise ValueError("grids must be a collision.SdfGrid or a sequence of them") from None
    if not grids or not all(isinstance(g, SdfGrid) for g in grids):
        raise ValueError("grids must be a collision.SdfGrid or a non-empty sequence of them")
    if any(isinstance(g, DeviceSdfGrid) for g in grids):
        raise ValueError("fit_spheres reads the samples on the host: pass DeviceSdfGrid.to_host()")
    if len(grids) > _lib.SPHERE_FIT_MAX_BODIES:
        raise ValueError(f"one call fits at most {_lib.SPHERE_FIT_MAX_BODIES} grids, got {len(grids)}")
    try:
        k = np.array(np.broadcast_to(np.asarray(max_spheres), (len(grids),)))
    except ValueError:
        raise ValueError(f"max_spheres must be an int or one per grid ({len(grids)}), got {np.shape(max_spheres)}") from None
    if k.dtype.kind not in "iu" or (k < 1).any() or (k > _lib.SPHERE_MAX).any():
        raise ValueError(f"max_spheres must be integers in 1..{_lib.SPHERE_MAX}, got {np.asarray(max_spheres).tolist()}")
    for i, g in enumerate(grids):
        if max(g.shape) > _lib.SPHERE_FIT_MAX_DIM:
            raise ValueError(f"grid {i}: every dimension of a fitted grid is at most {_lib.SPHERE_FIT_MAX_DIM} samples, got {g.shape}")
        if not (g.spacing[0] == g.spacing[1] == g.spacing[2]):
            raise ValueError(f"grid {i}: a fitted grid has one spacing for its three axes (isotropic), got {g.spacing.tolist()}")
    return (grids, k.astype(np.int32), *_fit_scalars(min_radius, inflate, coverage))


def fit_spheres(grids, max_spheres, min_radius=0.0, inflate=0.0, coverage=1.0):
    """Spheres inside the bodies that signed-distance grids describe (include/dexr_sphere_fit.h): a greedy cover on the device, all
    grids in ONE call on the current CUDA device and stream.  Every round takes, per grid, the sample whose ball of radius
    -value + inflate covers the most interior samples (value < 0) that no earlier ball covers; it ends after `max_spheres` (an
    int or one per grid, 1..128) spheres, once `coverage` (0..1) of the interior samples are covered, or when nothing is gained.
    Samples shallower than `min_radius` are never centres.  With inflate = 0 and a grid of exact distances (`SdfGrid.from_mesh`)
    no sphere protrudes from the body; with inflate > 0 by at most that much.

    grids: one `SdfGrid` or a sequence of at most 64, each with ONE spacing for its three axes and at most 64 samples per axis
    (`link_grid` makes such a grid of a mesh).  -> a list of `SphereFit`, one per grid; a grid without an interior sample gives
    an empty one."""
    grids, k, min_radius, inflate, coverage = _fit_rules(grids, max_spheres, min_radius, inflate, coverage)
    import torch

    dims = np.array([g.shape for g in grids], dtype=np.int32)
    sizes = np.array([g.values.size for g in grids], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    spacing = np.array([g.spacing[0] for g in grids], dtype=np.float64)
    k_max = int(k.max())
    with torch.cuda.device(torch.cuda.current_device()):
        values = torch.from_numpy(np.concatenate([g.values.reshape(-1) for g in grids])).cuda()
        index = torch.empty((len(grids), k_max), dtype=torch.int32, device="cuda")
        gain = torch.empty((len(grids), k_max), dtype=torch.int32, device="cuda")
        count = torch.empty((len(grids), 3), dtype=torch.int32, device="cuda")
        ws_bytes = _lib.sphere_fit_workspace_bytes(dims)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        _lib.sphere_fit_dev(dims, spacing, offset, k, min_radius, inflate, coverage, values.numel(), values.data_ptr(), index.data_ptr(),
                            gain.data_ptr(), count.data_ptr(), ws.data_ptr(), ws_bytes, stream=torch.cuda.current_stream().cuda_stream)
        index, gain, count = index.cpu().numpy(), gain.cpu().numpy(), count.cpu().numpy()
    out = []
    for b, g in enumerate(grids):
        n = int(count[b, 2])
        flat = index[b, :n].astype(np.int64)
        samples = np.stack(np.unravel_index(flat, g.shape), -1).reshape(n, 3)
        centers = g.origin + samples * g.spacing
        radii = -g.values.reshape(-1)[flat].astype(np.float64) + inflate
        out.append(SphereFit(centers, radii, samples, gain[b, :n].copy(), count[b, 0], count[b, 1]))
    return out


def link_grid(mesh: TriangleMesh, max_dim: int = 48, padding_cells: int = 1):
    """`SdfGrid.from_mesh` of a link's mesh with the ONE spacing that makes the longest side of the padded box `max_dim` samples
    (2..64): spacing = longest extent / (max_dim - 1 - 2 padding_cells), `padding_cells` cells of padding on every side."""
    if not isinstance(mesh, TriangleMesh):
        raise ValueError("mesh must be a collision.TriangleMesh")
    if not (isinstance(max_dim, (int, np.integer)) and isinstance(padding_cells, (int, np.integer))):
        raise ValueError("max_dim and padding_cells must be integers")
    if padding_cells < 0 or max_dim > _lib.SPHERE_FIT_MAX_DIM or max_dim - 1 - 2 * padding_cells < 1:
        raise ValueError(f"max_dim must lie in {2 + 2 * padding_cells}..{_lib.SPHERE_FIT_MAX_DIM} with padding_cells = {padding_cells} >= 0, got {max_dim}")
    lo, hi = mesh.bounds
    h = float((hi - lo).max()) / (max_dim - 1 - 2 * padding_cells)  # (> 0: a mesh has a triangle with area)
    cells = np.clip(np.ceil((hi - lo) / h), 1, max_dim - 1 - 2 * padding_cells)  # (rounding must not add a cell to the longest side; a flat side keeps one)
    shape = tuple(int(c) + 1 + 2 * padding_cells for c in cells)
    centre = (lo + hi) / 2.0
    origin = centre - (np.array(shape) - 1) * h / 2.0
    return SdfGrid.from_mesh(mesh, origin=origin, spacing=h, shape=shape)


def _grid_distances(model, grid, x, fixed_qpos, obstacle_pos, obstacle_rot):
    import torch

    B = x.shape[0]
    xc, fixed = _inputs(x, fixed_qpos)
    pos, rot = _obstacle_pose(obstacle_pos, obstacle_rot)
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x.device):
        dist = torch.empty((B, model.n_sphere), dtype=torch.float32, device=x.device)
        if B > 0:
            model.grid_distances_dev(grid.device_grid(torch.cuda.current_device()), B, xc.data_ptr(), ptr(fixed), dist.data_ptr(), ptr(pos),
                                     ptr(rot), stream=torch.cuda.current_stream(x.device).cuda_stream)
    return dist


def _grid_penalty(model, grid, x, fixed_qpos, margin, obstacle_pos, obstacle_rot, want_grad=True, want_wrench=False):
    """one launch -> (E (B,), grad (B, n_in) or None, wrench (B, 6) or None)."""
    import torch

    B = x.shape[0]
    xc, fixed = _inputs(x, fixed_qpos)
    pos, rot = _obstacle_pose(obstacle_pos, obstacle_rot)
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x.device):
        e = torch.empty((B,), dtype=torch.float32, device=x.device)
        g = torch.empty((B, model.n_in), dtype=torch.float32, device=x.device) if want_grad else None
        wr = torch.empty((B, 6), dtype=torch.float32, device=x.device) if want_wrench else None
        if B > 0:
            model.grid_penalty_dev(grid.device_grid(torch.cuda.current_device()), B, xc.data_ptr(), ptr(fixed), float(margin), e.data_ptr(),
                                   ptr(g), ptr(wr), ptr(pos), ptr(rot), stream=torch.cuda.current_stream(x.device).cuda_stream)
    return e, g, wr


def grid_distances(optimizer, q, sphere_set: SphereSet, grid: SdfGrid, obstacle_pos=None, obstacle_rot=None, fixed_qpos=None):
    """Signed distance of every sphere of the set to the field of `grid` at the optimiser's variables: q (B, n_opt) float32 CUDA,
    obstacle_pos (B, 3) and obstacle_rot (B, 3, 3) float32 the world pose of the grid's frame per frame, or None (zero translation
    / identity: a shared scene) -> dist (B, S) float32 in the set's sphere order, negative where a sphere penetrates.  One
    trilinear lookup per sphere, whatever the shape.  No autograd graph."""
    pairs = _check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos, sphere_set,
                             grid, obstacle_pos, obstacle_rot, "q", grid=True)
    return _grid_distances(optimizer.sphere_model(sphere_set, pairs), grid, q, fixed_qpos, obstacle_pos, obstacle_rot)


def grid_penalty(optimizer, q, sphere_set: SphereSet, grid: SdfGrid, margin, obstacle_pos=None, obstacle_rot=None, fixed_qpos=None,
                 wrench: bool = False):
    """(E (B,), grad_q (B, n_opt)) float32 from ONE launch: E = sum_s max(0, margin - d_s)^2 over every sphere s of the set, d_s
    the signed distance of the sphere's surface to the field, and its gradient in q.  margin: a finite Python float >= 0
    (metres); obstacle_pos, obstacle_rot as in `grid_distances`.  With `wrench=True` -> (E, grad_q, wrench (B, 6)):
    dE/d(obstacle translation) and dE/d(a world-aligned small rotation of the obstacle about its origin).  No autograd graph:
    `autograd.grid_penalty` is the same launch with one."""
    pairs = _check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos, sphere_set,
                             grid, obstacle_pos, obstacle_rot, "q", margin, penalty=True, grid=True)
    e, g, wr = _grid_penalty(optimizer.sphere_model(sphere_set, pairs), grid, q, fixed_qpos, margin, obstacle_pos, obstacle_rot,
                             want_wrench=wrench)
    return (e, g, wr) if wrench else (e, g)


def robot_grid_distances(robot, qpos, sphere_set: SphereSet, grid: SdfGrid, obstacle_pos=None, obstacle_rot=None):
    """The same for a full robot qpos (B, robot.dof) in dof order; every joint is a column of its own."""
    pairs = _check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, grid, obstacle_pos, obstacle_rot, "qpos", grid=True)
    return _grid_distances(robot.sphere_model(sphere_set, pairs), grid, qpos, None, obstacle_pos, obstacle_rot)


def robot_grid_penalty(robot, qpos, sphere_set: SphereSet, grid: SdfGrid, margin, obstacle_pos=None, obstacle_rot=None, wrench: bool = False):
    """(E (B,), grad_qpos (B, robot.dof)[, wrench (B, 6)]) for a full robot qpos in dof order."""
    pairs = _check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, grid, obstacle_pos, obstacle_rot, "qpos", margin,
                             penalty=True, grid=True)
    e, g, wr = _grid_penalty(robot.sphere_model(sphere_set, pairs), grid, qpos, None, margin, obstacle_pos, obstacle_rot, want_wrench=wrench)
    return (e, g, wr) if wrench else (e, g)


# ---- the posture solve with an obstacle term: primitives (include/dexr_resolve_obstacles.h) or a grid (include/dexr_resolve_grid.h) ------
def _resolve_contacts(model_of, n_in, n_fixed, kin, robot, x0, what, fixed_qpos, sphere_set, obstacle, grid, margin, obstacle_margin, obstacle_pos,
                      obstacle_rot, obstacle_weight, prim_weight, damping, max_iters, posture_weight, q_ref, collision_weight, pair_weight,
                      link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits):
    """every rule (those of `_resolve`, then the obstacle side's), then one model and one launch.  obstacle: an ObstacleSet, or with
    `grid` an SdfGrid (which has no prim_weight: None)."""
    import torch

    named = _resolve_rules(n_in, x0, sphere_set, damping, max_iters, posture_weight, q_ref, collision_weight, link_names, target_pos,
                           target_rot, pos_weight, rot_weight, tol, max_step, limits)
    for n in link_names or ():
        kin.body_frame_index(n)  # ValueError on an unknown link
    if isinstance(obstacle_weight, bool) or not isinstance(obstacle_weight, (int, float)) or not math.isfinite(obstacle_weight) or obstacle_weight < 0:
        raise ValueError(f"obstacle_weight must be a finite Python float >= 0, got {obstacle_weight!r}")
    if obstacle_margin is not None and (isinstance(obstacle_margin, bool) or not isinstance(obstacle_margin, (int, float))
                                        or not math.isfinite(obstacle_margin) or obstacle_margin < 0):
        raise ValueError(f"obstacle_margin must be a finite Python float >= 0 or None (margin), got {obstacle_margin!r}")
    pairs = _check(n_in, n_fixed, kin, robot, x0, fixed_qpos, sphere_set, what, margin, pair_weight, penalty=True, poses=False)
    _check_obstacles(n_in, n_fixed, kin, robot, x0, fixed_qpos, sphere_set, obstacle, obstacle_pos, obstacle_rot, what, margin, prim_weight,
                     penalty=True, grid=grid)  # (ends with the device)
    if pair_weight is not None:
        named = named + [("pair_weight", pair_weight)]
    for name, t in named:
        if t.device != x0.device:
            raise ValueError(f"{name} is on {t.device}, {what} on {x0.device}: all tensors must be on one CUDA device")
    B = x0.shape[0]
    xc, fixed = _inputs(x0, fixed_qpos)
    c = lambda a: None if a is None else a.detach().contiguous()  # noqa: E731
    xr, tp, tr, wl, wa, pw, ow = (c(a) for a in (q_ref, target_pos, target_rot, pos_weight, rot_weight, pair_weight, prim_weight))
    pos, rot = _obstacle_pose(obstacle_pos, obstacle_rot)
    lo, hi = (None, None) if limits is None else (limits.detach()[:, 0].contiguous(), limits.detach()[:, 1].contiguous())
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x0.device):
        if isinstance(posture_weight, torch.Tensor):
            u = c(posture_weight)
        else:
            u = None if not posture_weight else torch.full((n_in,), float(posture_weight), dtype=torch.float32, device=x0.device)
        model = model_of(sphere_set, pairs, tuple(link_names or ()))
        q = torch.empty((B, model.n_in), dtype=torch.float32, device=x0.device)
        iters = torch.empty((B,), dtype=torch.int32, device=x0.device)
        energy = torch.empty((B, 4), dtype=torch.float32, device=x0.device)
        status = torch.empty((B,), dtype=torch.int32, device=x0.device)
        if B > 0:
            if grid:
                launch, handle, own = model.resolve_grid_dev, obstacle.device_grid(torch.cuda.current_device()), {}
            else:
                launch, handle, own = model.resolve_obstacles_dev, obstacle.device_set(torch.cuda.current_device()), dict(prim_weight_ptr=ptr(ow))
            launch(handle, B, xc.data_ptr(), ptr(fixed), float(margin), float(damping), int(max_iters), q.data_ptr(), iters.data_ptr(),
                   energy.data_ptr(), status.data_ptr(), x_ref_ptr=ptr(xr), posture_weight_ptr=ptr(u), n_target=len(link_names or ()),
                   target_pos_ptr=ptr(tp), target_rot_ptr=ptr(tr), pos_weight_ptr=ptr(wl), rot_weight_ptr=ptr(wa),
                   collision_weight=float(collision_weight), pair_weight_ptr=ptr(pw), lo_ptr=ptr(lo), hi_ptr=ptr(hi), tol=float(tol),
                   max_step=float(max_step), obstacle_pos_ptr=ptr(pos), obstacle_rot_ptr=ptr(rot),
                   obstacle_margin=float(margin if obstacle_margin is None else obstacle_margin), obstacle_weight=float(obstacle_weight),
                   stream=torch.cuda.current_stream(x0.device).cuda_stream, **own)
    return q, iters, energy, status


def resolve_collisions(optimizer, q0, sphere_set: SphereSet, obstacles: ObstacleSet, margin, obstacle_margin=None, obstacle_pos=None,
                       obstacle_rot=None, obstacle_weight=1.0, prim_weight=None, damping=_REQUIRED, max_iters=_REQUIRED, posture_weight=None,
                       q_ref=None, collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None, target_rot=None, pos_weight=None,
                       rot_weight=None, tol=0.0, max_step=0.0, limits=None, fixed_qpos=None):
    """`resolve_self_collision` with one more term: project postures out of self-penetration AND out of the primitives of
    `obstacles` -- a held object with a pose per frame, or a shared scene -- inside ONE launch, on

        E = E of resolve_self_collision + obstacle_weight * sum_s sum_m w_m max(0, obstacle_margin - d_sm)^2

    with d_sm of `obstacle_penalty`.  obstacle_margin: a finite Python float >= 0, None: `margin`; obstacle_pos (B, 3), obstacle_rot
    (B, 3, 3) float32 or None as in `obstacle_distances`, fixed during the solve; prim_weight (M,) float32 >= 0 or None (1).  Every
    other argument, the accept / reject rule and the damping are those of `resolve_self_collision`.  -> (q (B, n_opt) float32,
    iters (B) int32, energy (B, 4) float32: pose, posture, self-collision and obstacle term at q, status (B) int32, whose bit
    _lib.RESOLVE_CONTACTS_TRUNCATED says that a point had more than 256 active (sphere, primitive) contacts: the curvature used the
    first 256 in the set's sphere order, then the primitives' order).  No autograd graph."""
    return _resolve_contacts(optimizer.sphere_model, optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q0,
                             "q", fixed_qpos, sphere_set, obstacles, False, margin, obstacle_margin, obstacle_pos, obstacle_rot, obstacle_weight,
                             prim_weight, damping, max_iters, posture_weight, q_ref, collision_weight, pair_weight, link_names, target_pos,
                             target_rot, pos_weight, rot_weight, tol, max_step, limits)


def robot_resolve_collisions(robot, qpos0, sphere_set: SphereSet, obstacles: ObstacleSet, margin, obstacle_margin=None, obstacle_pos=None,
                             obstacle_rot=None, obstacle_weight=1.0, prim_weight=None, damping=_REQUIRED, max_iters=_REQUIRED,
                             posture_weight=None, q_ref=None, collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None,
                             target_rot=None, pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None):
    """The same for a full robot qpos (B, robot.dof) in dof order; every joint is a column of its own, limits (robot.dof, 2)."""
    return _resolve_contacts(robot.sphere_model, robot.dof, 0, robot.kin, robot, qpos0, "qpos", None, sphere_set, obstacles, False, margin,
                             obstacle_margin, obstacle_pos, obstacle_rot, obstacle_weight, prim_weight, damping, max_iters, posture_weight,
                             q_ref, collision_weight, pair_weight, link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step,
                             limits)


def resolve_grid_collisions(optimizer, q0, sphere_set: SphereSet, grid: SdfGrid, margin, obstacle_margin=None, obstacle_pos=None,
                            obstacle_rot=None, obstacle_weight=1.0, damping=_REQUIRED, max_iters=_REQUIRED, posture_weight=None, q_ref=None,
                            collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None, target_rot=None, pos_weight=None,
                            rot_weight=None, tol=0.0, max_step=0.0, limits=None, fixed_qpos=None):
    """`resolve_collisions` against an `SdfGrid` instead of primitives: project postures out of self-penetration AND out of the
    field of `grid` -- a held object with a pose per frame, or a shared scene, given as a mesh, a scan or a depth fusion -- inside
    ONE launch, on

        E = E of resolve_self_collision + obstacle_weight * sum_s max(0, obstacle_margin - d_s)^2

    with d_s of `grid_penalty`.  obstacle_margin: a finite Python float >= 0, None: `margin`; obstacle_pos (B, 3), obstacle_rot
    (B, 3, 3) float32 or None as in `grid_distances`, fixed during the solve.  Every other argument, the accept / reject rule and
    the damping are those of `resolve_self_collision`.  -> (q (B, n_opt) float32, iters (B) int32, energy (B, 4) float32: pose,
    posture, self-collision and grid term at q, status (B) int32).  A sphere has at most one contact with a grid: every contact
    enters the curvature and _lib.RESOLVE_CONTACTS_TRUNCATED is never set.  No autograd graph."""
    return _resolve_contacts(optimizer.sphere_model, optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q0,
                             "q", fixed_qpos, sphere_set, grid, True, margin, obstacle_margin, obstacle_pos, obstacle_rot, obstacle_weight, None,
                             damping, max_iters, posture_weight, q_ref, collision_weight, pair_weight, link_names, target_pos, target_rot,
                             pos_weight, rot_weight, tol, max_step, limits)


def robot_resolve_grid_collisions(robot, qpos0, sphere_set: SphereSet, grid: SdfGrid, margin, obstacle_margin=None, obstacle_pos=None,
                                  obstacle_rot=None, obstacle_weight=1.0, damping=_REQUIRED, max_iters=_REQUIRED, posture_weight=None,
                                  q_ref=None, collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None, target_rot=None,
                                  pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None):
    """The same for a full robot qpos (B, robot.dof) in dof order; every joint is a column of its own, limits (robot.dof, 2)."""
    return _resolve_contacts(robot.sphere_model, robot.dof, 0, robot.kin, robot, qpos0, "qpos", None, sphere_set, grid, True, margin,
                             obstacle_margin, obstacle_pos, obstacle_rot, obstacle_weight, None, damping, max_iters, posture_weight, q_ref,
                             collision_weight, pair_weight, link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits)


# ---- the posture solve against a scene: several posed bodies, sets and grids, in one launch (include/dexr_resolve_scene.h) ---------------
class SceneBody:
    """One body of a scene, plain data: `obstacle` an ObstacleSet or an SdfGrid; pos (B, 3), rot (B, 3, 3) float32 tensors or None
    (a world-fixed body: zero translation / the identity); margin a finite Python float >= 0 or None (the solve's `margin`); weight a
    finite Python float >= 0; prim_weight (M,) float32 >= 0 or None (1), an ObstacleSet alone.  Nothing is checked here: the solve
    that takes the body checks it."""

    def __init__(self, obstacle, pos=None, rot=None, margin=None, weight=1.0, prim_weight=None):
        self.obstacle, self.pos, self.rot, self.margin, self.weight, self.prim_weight = obstacle, pos, rot, margin, weight, prim_weight

    def __repr__(self):
        return (f"SceneBody({self.obstacle!r}, pos={'None' if self.pos is None else 'given'}, rot={'None' if self.rot is None else 'given'}, "
                f"margin={self.margin!r}, weight={self.weight!r}, prim_weight={'None' if self.prim_weight is None else 'given'})")


def _scene_rules(x0, bodies):
    """The argument rules of the bodies that look at no device: the list, then per body the type, the scalars, then types, dtypes
    and shapes of its tensors.  Returns the tensors by name, for the device rule that comes last."""
    import torch

    if isinstance(bodies, SceneBody) or not isinstance(bodies, (list, tuple)):
        raise ValueError("bodies must be a list of collision.SceneBody")
    if not 1 <= len(bodies) <= _lib.SCENE_MAXBODY:
        raise ValueError(f"a scene has 1..{_lib.SCENE_MAXBODY} bodies, got {len(bodies)}")
    B = x0.shape[0] if isinstance(x0, torch.Tensor) and x0.ndim == 2 else None
    named = []
    for b, body in enumerate(bodies):
        if not isinstance(body, SceneBody):
            raise ValueError(f"bodies[{b}] must be a collision.SceneBody, got {type(body).__name__}")
        if not isinstance(body.obstacle, (ObstacleSet, SdfGrid)):
            raise ValueError(f"bodies[{b}].obstacle must be a collision.ObstacleSet or a collision.SdfGrid, got {type(body.obstacle).__name__}")
        grid = isinstance(body.obstacle, SdfGrid)
        if grid and body.prim_weight is not None:
            raise ValueError(f"bodies[{b}] is an SdfGrid and has a prim_weight: a grid has no primitives to weigh")
        w, m = body.weight, body.margin
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w < 0:
            raise ValueError(f"bodies[{b}].weight must be a finite Python float >= 0, got {w!r}")
        if m is not None and (isinstance(m, bool) or not isinstance(m, (int, float)) or not math.isfinite(m) or m < 0):
            raise ValueError(f"bodies[{b}].margin must be a finite Python float >= 0 or None (margin), got {m!r}")
        mine = [(n, t, s) for n, t, s in ((f"bodies[{b}].pos", body.pos, (B, 3)), (f"bodies[{b}].rot", body.rot, (B, 3, 3))) if t is not None]
        if body.prim_weight is not None:
            mine.append((f"bodies[{b}].prim_weight", body.prim_weight, (body.obstacle.n_prim,)))
        for name, t, _ in mine:
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor")
        for name, t, _ in mine:
            if t.dtype != torch.float32:
                raise ValueError(f"{name} must be float32, got {t.dtype}")
        for name, t, shape in mine:
            if (B is not None or shape[0] is not None) and tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
        named += [(n, t) for n, t, _ in mine]
    return named


def _resolve_scene(model_of, n_in, n_fixed, kin, robot, x0, what, fixed_qpos, sphere_set, bodies, margin, damping, max_iters, posture_weight,
                   q_ref, collision_weight, pair_weight, link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits,
                   body_energy):
    """every rule (those of `_resolve`, then the bodies'), then one model and one launch."""
    import torch

    named = _resolve_rules(n_in, x0, sphere_set, damping, max_iters, posture_weight, q_ref, collision_weight, link_names, target_pos,
                           target_rot, pos_weight, rot_weight, tol, max_step, limits)
    for n in link_names or ():
        kin.body_frame_index(n)  # ValueError on an unknown link
    named = named + _scene_rules(x0, bodies)
    pairs = _check(n_in, n_fixed, kin, robot, x0, fixed_qpos, sphere_set, what, margin, pair_weight, penalty=True)  # (ends with the device)
    for name, t in named:
        if t.device != x0.device:
            raise ValueError(f"{name} is on {t.device}, {what} on {x0.device}: all tensors must be on one CUDA device")
    B, nb = x0.shape[0], len(bodies)
    xc, fixed = _inputs(x0, fixed_qpos)
    c = lambda a: None if a is None else a.detach().contiguous()  # noqa: E731
    xr, tp, tr, wl, wa, pw = (c(a) for a in (q_ref, target_pos, target_rot, pos_weight, rot_weight, pair_weight))
    held = [(c(body.pos), c(body.rot), c(body.prim_weight)) for body in bodies]  # (alive until the launch is enqueued)
    lo, hi = (None, None) if limits is None else (limits.detach()[:, 0].contiguous(), limits.detach()[:, 1].contiguous())
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x0.device):
        if isinstance(posture_weight, torch.Tensor):
            u = c(posture_weight)
        else:
            u = None if not posture_weight else torch.full((n_in,), float(posture_weight), dtype=torch.float32, device=x0.device)
        model = model_of(sphere_set, pairs, tuple(link_names or ()))
        q = torch.empty((B, model.n_in), dtype=torch.float32, device=x0.device)
        iters = torch.empty((B,), dtype=torch.int32, device=x0.device)
        energy = torch.empty((B, 4), dtype=torch.float32, device=x0.device)
        status = torch.empty((B,), dtype=torch.int32, device=x0.device)
        be = torch.empty((B, nb), dtype=torch.float32, device=x0.device) if body_energy else None
        if B > 0:
            dev = torch.cuda.current_device()
            recs = [(body.obstacle.device_grid(dev) if isinstance(body.obstacle, SdfGrid) else body.obstacle.device_set(dev), ptr(p), ptr(r),
                     None if body.margin is None else float(body.margin), float(body.weight), ptr(w)) for body, (p, r, w) in zip(bodies, held)]
            model.resolve_scene_dev(recs, B, xc.data_ptr(), ptr(fixed), float(margin), float(damping), int(max_iters), q.data_ptr(),
                                    iters.data_ptr(), energy.data_ptr(), status.data_ptr(), x_ref_ptr=ptr(xr), posture_weight_ptr=ptr(u),
                                    n_target=len(link_names or ()), target_pos_ptr=ptr(tp), target_rot_ptr=ptr(tr), pos_weight_ptr=ptr(wl),
                                    rot_weight_ptr=ptr(wa), collision_weight=float(collision_weight), pair_weight_ptr=ptr(pw), lo_ptr=ptr(lo),
                                    hi_ptr=ptr(hi), tol=float(tol), max_step=float(max_step), body_energy_ptr=ptr(be),
                                    stream=torch.cuda.current_stream(x0.device).cuda_stream)
    return (q, iters, energy, status, be) if body_energy else (q, iters, energy, status)


def resolve_scene_collisions(optimizer, q0, sphere_set: SphereSet, bodies, margin, damping=_REQUIRED, max_iters=_REQUIRED, posture_weight=None,
                             q_ref=None, collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None, target_rot=None,
                             pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None, fixed_qpos=None, body_energy=False):
    """`resolve_collisions` / `resolve_grid_collisions` against a SCENE: `bodies`, a list of 1..4 `SceneBody`, each an ObstacleSet or
    an SdfGrid with a pose per frame (or none), a margin and a weight of its own -- a hand holding an object that sits on a table, a
    world-fixed fixture and a held object, primitives and a scanned mesh together.  ONE launch descends on ONE energy

        E = E of resolve_self_collision + sum_b weight_b * (the obstacle term of body b with margin_b and its pose)

    where running the single-body solves one after the other would push the hand back into the body each of them does not know.
    Every other argument, the accept / reject rule and the damping are those of `resolve_self_collision`.  -> (q (B, n_opt) float32,
    iters (B) int32, energy (B, 4) float32: pose, posture, self-collision and the sum of the bodies' terms at q, status (B) int32)
    and, with body_energy=True, a fifth value (B, n_body) float32: each body's term at q.  The curvature uses the first 256 active
    contacts over all bodies together, in the set's sphere order, then the bodies' order, then a set's primitives' order; a point
    with more sets _lib.RESOLVE_CONTACTS_TRUNCATED -- grids count here, unlike in `resolve_grid_collisions`.  The matching penalty
    is the sum of `obstacle_penalty` / `grid_penalty` over the bodies.  No autograd graph."""
    return _resolve_scene(optimizer.sphere_model, optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q0, "q",
                          fixed_qpos, sphere_set, bodies, margin, damping, max_iters, posture_weight, q_ref, collision_weight, pair_weight,
                          link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits, body_energy)


def robot_resolve_scene_collisions(robot, qpos0, sphere_set: SphereSet, bodies, margin, damping=_REQUIRED, max_iters=_REQUIRED,
                                   posture_weight=None, q_ref=None, collision_weight=1.0, pair_weight=None, link_names=None, target_pos=None,
                                   target_rot=None, pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None, body_energy=False):
    """The same for a full robot qpos (B, robot.dof) in dof order; every joint is a column of its own, limits (robot.dof, 2)."""
    return _resolve_scene(robot.sphere_model, robot.dof, 0, robot.kin, robot, qpos0, "qpos", None, sphere_set, bodies, margin, damping,
                          max_iters, posture_weight, q_ref, collision_weight, pair_weight, link_names, target_pos, target_rot, pos_weight,
                          rot_weight, tol, max_step, limits, body_energy)


# ---- the other robot: the spheres of one posed robot against the spheres of another (include/dexr_cross.h) -----------------------------
def _optimizer_side(optimizer, q, sphere_set, fixed_qpos, tag):
    return (optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos, sphere_set, f"q_{tag}",
            optimizer.sphere_model)


def _robot_side(robot, qpos, sphere_set, tag):
    return robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, f"qpos_{tag}", robot.sphere_model


def _check_cross(side_a, side_b, pos_a, rot_a, pos_b, rot_b, margin=None, pair_weight=None, penalty=False):
    """Every argument rule in the order of `_check`, for both robots -- the sphere sets, the links, the pairs, the scalars, then types,
    dtypes and shapes, and last the device -- before anything touches the GPU.  Returns the two sphere models."""
    import torch

    pairs = []
    for side in (side_a, side_b):
        kin, robot, sphere_set = side[2], side[3], side[6]
        if not isinstance(sphere_set, SphereSet):
            raise ValueError("spheres_a and spheres_b must each be a collision.SphereSet")
        for n in sphere_set.table_links:
            kin.body_frame_index(n)  # ValueError on an unknown link
        pairs.append(_resolved_pairs(robot, sphere_set))
    if penalty and (isinstance(margin, bool) or not isinstance(margin, (int, float)) or not math.isfinite(margin) or margin < 0):
        raise ValueError(f"margin must be a finite Python float >= 0, got {margin!r}")
    q_a, q_b = side_a[4], side_b[4]
    B = q_a.shape[0] if isinstance(q_a, torch.Tensor) and q_a.ndim == 2 else None
    named = [(n, t, s) for n, t, s in (("pos_a", pos_a, (B, 3)), ("rot_a", rot_a, (B, 3, 3)), ("pos_b", pos_b, (B, 3)), ("rot_b", rot_b, (B, 3, 3)))
             if t is not None]
    if penalty and pair_weight is not None:
        named.append(("pair_weight", pair_weight, (side_a[6].n_sphere, side_b[6].n_sphere)))
    for name, t, _ in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    for name, t, _ in named:
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    for name, t, shape in named:
        if (B is not None or shape[0] is not None) and tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    tensors = []
    for (n_in, n_fixed, _, _, q, fixed_qpos, _, what, _), tag in ((side_a, "a"), (side_b, "b")):  # the rules of _check_poses, the device last
        if not isinstance(q, torch.Tensor):
            raise ValueError(f"{what} must be a torch tensor")
        both = [(what, q)]
        if fixed_qpos is not None:
            if not isinstance(fixed_qpos, torch.Tensor):
                raise ValueError(f"fixed_qpos_{tag} must be a torch tensor")
            both.append((f"fixed_qpos_{tag}", fixed_qpos))
        for name, t in both:
            if t.dtype != torch.float32:
                raise ValueError(f"{name} must be float32, got {t.dtype}")
        if q.ndim != 2 or q.shape[1] != n_in:
            raise ValueError(f"{what} must have shape (B, {n_in}), got {tuple(q.shape)}")
        if n_fixed > 0 and fixed_qpos is None:
            raise ValueError(f"the optimizer has {n_fixed} fixed joints: fixed_qpos_{tag} of shape ({q.shape[0]}, {n_fixed}) is required")
        if fixed_qpos is not None and tuple(fixed_qpos.shape) != (q.shape[0], n_fixed):
            raise ValueError(f"fixed_qpos_{tag} must have shape ({q.shape[0]}, {n_fixed}), got {tuple(fixed_qpos.shape)}")
        tensors += both
    if q_b.shape[0] != q_a.shape[0]:
        raise ValueError(f"{side_a[7]} has {q_a.shape[0]} frames, {side_b[7]} {q_b.shape[0]}: both robots need one row per frame")
    if q_a.device.type != "cuda":
        raise ValueError(f"the tensors must be CUDA (HIP) tensors, got device {q_a.device}")
    for name, t in tensors[1:] + [(n, t) for n, t, _ in named]:
        if t.device != q_a.device:
            raise ValueError(f"{name} is on {t.device}, {side_a[7]} on {q_a.device}: all tensors must be on one CUDA device")
    return side_a[8](side_a[6], pairs[0]), side_b[8](side_b[6], pairs[1])


def _cross_inputs(x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b):
    """the eight inputs of a cross launch, detached and contiguous (None where left out)."""
    xa, fa = _inputs(x_a, fixed_a)
    xb, fb = _inputs(x_b, fixed_b)
    return (xa, fa, xb, fb) + _obstacle_pose(pos_a, rot_a) + _obstacle_pose(pos_b, rot_b)


def _cross_ptrs(inputs):
    xa, fa, xb, fb, pa, ra, pb, rb = (0 if a is None else a.data_ptr() for a in inputs)
    return (xa, fa, xb, fb), dict(pos_a_ptr=pa, rot_a_ptr=ra, pos_b_ptr=pb, rot_b_ptr=rb)


def _cross_distances(model_a, model_b, x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b, nearest):
    import torch

    B, dev = x_a.shape[0], x_a.device
    inputs = _cross_inputs(x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b)
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        da = torch.empty((B, model_a.n_sphere), dtype=torch.float32, device=dev)
        db = torch.empty((B, model_b.n_sphere), dtype=torch.float32, device=dev)
        na = torch.empty((B, model_a.n_sphere), dtype=torch.int32, device=dev) if nearest else None
        nb = torch.empty((B, model_b.n_sphere), dtype=torch.int32, device=dev) if nearest else None
        if B > 0:
            head, poses = _cross_ptrs(inputs)
            model_a.cross_distances_dev(model_b, B, *head, da.data_ptr(), ptr(na), db.data_ptr(), ptr(nb), **poses,
                                        stream=torch.cuda.current_stream(dev).cuda_stream)
    return (da, na, db, nb) if nearest else (da, db)


def _cross_penalty(model_a, model_b, x_a, fixed_a, x_b, fixed_b, margin, pair_weight, pos_a, rot_a, pos_b, rot_b, want=(True,) * 5):
    """one launch -> (E (B,), grad_a, grad_b, wrench_a (B, 6), wrench_b (B, 6)), None where `want` (in that order) says so."""
    import torch

    B, dev = x_a.shape[0], x_a.device
    inputs = _cross_inputs(x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b)
    w = None if pair_weight is None else pair_weight.detach().contiguous()
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    shapes = ((B,), (B, model_a.n_in), (B, model_b.n_in), (B, 6), (B, 6))
    with torch.cuda.device(dev):
        out = [torch.empty(s, dtype=torch.float32, device=dev) if k else None for s, k in zip(shapes, want)]
        if B > 0:
            head, poses = _cross_ptrs(inputs)
            model_a.cross_penalty_dev(model_b, B, *head, float(margin), ptr(w), *[ptr(o) for o in out], **poses,
                                      stream=torch.cuda.current_stream(dev).cuda_stream)
    return tuple(out)


def _cross_distances_vjp(model_a, model_b, inputs, grad_dist_a, grad_dist_b, want_wrench=(False, False)):
    """the VJP launch on detached, contiguous `inputs` (_cross_inputs) -> (grad_a, grad_b, wrench_a or None, wrench_b or None)."""
    import torch

    xa, xb = inputs[0], inputs[2]
    B, dev = xa.shape[0], xa.device
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        ga, gb = torch.empty_like(xa), torch.empty_like(xb)  # (the kernel writes every entry)
        wa, wb = (torch.empty((B, 6), dtype=torch.float32, device=dev) if k else None for k in want_wrench)
        if B > 0:
            head, poses = _cross_ptrs(inputs)
            model_a.cross_distances_vjp_dev(model_b, B, *head, ptr(grad_dist_a), ptr(grad_dist_b), ga.data_ptr(), gb.data_ptr(), ptr(wa), ptr(wb),
                                            **poses, stream=torch.cuda.current_stream(dev).cuda_stream)
    return ga, gb, wa, wb


def cross_distances(optimizer_a, q_a, spheres_a: SphereSet, optimizer_b, q_b, spheres_b: SphereSet, pos_a=None, rot_a=None, pos_b=None,
                    rot_b=None, fixed_qpos_a=None, fixed_qpos_b=None, nearest: bool = False):
    """Signed distance of every sphere of robot A to the nearest sphere of robot B and the other way round, each robot at its own
    optimiser's variables and with its own base pose per frame: q_a (B, n_opt_a), q_b (B, n_opt_b) float32 CUDA; pos_* (B, 3) and
    rot_* (B, 3, 3) float32 the world pose of that robot's root per frame, or None (zero translation / identity) -> (dist_a (B, S_a),
    dist_b (B, S_b)) float32 in the sets' sphere orders, negative where two spheres interpenetrate; with `nearest=True` ->
    (dist_a, nearest_a, dist_b, nearest_b), nearest_* int32 the first sphere of the other set that attains the minimum.  The pair
    lists of the sets play no part; the two optimisers may be one.  No autograd graph."""
    ma, mb = _check_cross(_optimizer_side(optimizer_a, q_a, spheres_a, fixed_qpos_a, "a"), _optimizer_side(optimizer_b, q_b, spheres_b, fixed_qpos_b, "b"),
                          pos_a, rot_a, pos_b, rot_b)
    return _cross_distances(ma, mb, q_a, fixed_qpos_a, q_b, fixed_qpos_b, pos_a, rot_a, pos_b, rot_b, nearest)


def cross_penalty(optimizer_a, q_a, spheres_a: SphereSet, optimizer_b, q_b, spheres_b: SphereSet, margin, pos_a=None, rot_a=None, pos_b=None,
                  rot_b=None, pair_weight=None, fixed_qpos_a=None, fixed_qpos_b=None, wrench: bool = False):
    """(E (B,), dE/dq_a (B, n_opt_a), dE/dq_b (B, n_opt_b)) float32 from ONE launch: E = sum_s sum_t w_st max(0, margin - d_st)^2
    over every sphere s of A and every sphere t of B, d_st the signed distance of the two surfaces, and its gradient in both
    robots' variables.  margin: a finite Python float >= 0 (metres); pair_weight (S_a, S_b) float32 >= 0 or None (1), shared by
    the batch, a zero masks a pair; the poses as in `cross_distances`.  With `wrench=True` -> (E, dE/dq_a, dE/dq_b, wrench_a,
    wrench_b), each (B, 6): dE/d(translation of that base) and dE/d(a world-aligned small rotation of that base about its
    origin).  No autograd graph: `autograd.cross_penalty` is the same launch with one."""
    ma, mb = _check_cross(_optimizer_side(optimizer_a, q_a, spheres_a, fixed_qpos_a, "a"), _optimizer_side(optimizer_b, q_b, spheres_b, fixed_qpos_b, "b"),
                          pos_a, rot_a, pos_b, rot_b, margin, pair_weight, penalty=True)
    out = _cross_penalty(ma, mb, q_a, fixed_qpos_a, q_b, fixed_qpos_b, margin, pair_weight, pos_a, rot_a, pos_b, rot_b,
                         want=(True, True, True, wrench, wrench))
    return out if wrench else out[:3]


def robot_cross_distances(robot_a, qpos_a, spheres_a: SphereSet, robot_b, qpos_b, spheres_b: SphereSet, pos_a=None, rot_a=None, pos_b=None,
                          rot_b=None, nearest: bool = False):
    """The same for full robot qpos (B, robot.dof) in dof order; every joint is a column of its own."""
    ma, mb = _check_cross(_robot_side(robot_a, qpos_a, spheres_a, "a"), _robot_side(robot_b, qpos_b, spheres_b, "b"), pos_a, rot_a, pos_b, rot_b)
    return _cross_distances(ma, mb, qpos_a, None, qpos_b, None, pos_a, rot_a, pos_b, rot_b, nearest)


def robot_cross_penalty(robot_a, qpos_a, spheres_a: SphereSet, robot_b, qpos_b, spheres_b: SphereSet, margin, pos_a=None, rot_a=None,
                        pos_b=None, rot_b=None, pair_weight=None, wrench: bool = False):
    """(E (B,), dE/dqpos_a, dE/dqpos_b[, wrench_a, wrench_b]) for full robot qpos in dof order."""
    ma, mb = _check_cross(_robot_side(robot_a, qpos_a, spheres_a, "a"), _robot_side(robot_b, qpos_b, spheres_b, "b"), pos_a, rot_a, pos_b, rot_b,
                          margin, pair_weight, penalty=True)
    out = _cross_penalty(ma, mb, qpos_a, None, qpos_b, None, margin, pair_weight, pos_a, rot_a, pos_b, rot_b,
                         want=(True, True, True, wrench, wrench))
    return out if wrench else out[:3]


# ---- the posture solve against the other robot (include/dexr_resolve_cross.h) ----------------------------------------------------------
def _cross_resolve_rules(side_b, x0, n_sphere_a, cross_margin, w_x, other_pos, other_rot, cross_weight):
    """The rules of the other robot's arguments, none of which looks at a device: its sphere set and links, the two scalars, then
    types, dtypes and shapes of its tensors.  Returns (its pairs, its tensors by name for the device rule that comes last)."""
    import torch

    n_in, n_fixed, kin, robot, q_b, fixed_b, spheres_b, what = side_b[:8]
    if not isinstance(spheres_b, SphereSet):
        raise ValueError("spheres_b must be a collision.SphereSet")
    for n in spheres_b.table_links:
        kin.body_frame_index(n)  # ValueError on an unknown link
    pairs_b = _resolved_pairs(robot, spheres_b)
    if cross_margin is not None and (isinstance(cross_margin, bool) or not isinstance(cross_margin, (int, float)) or not math.isfinite(cross_margin)
                                     or cross_margin < 0):
        raise ValueError(f"cross_margin must be a finite Python float >= 0 or None (margin), got {cross_margin!r}")
    if isinstance(w_x, bool) or not isinstance(w_x, (int, float)) or not math.isfinite(w_x) or w_x < 0:
        raise ValueError(f"w_x must be a finite Python float >= 0, got {w_x!r}")
    B = x0.shape[0] if isinstance(x0, torch.Tensor) and x0.ndim == 2 else None
    named = [(n, t, s) for n, t, s in (("other_pos", other_pos, (B, 3)), ("other_rot", other_rot, (B, 3, 3)),
                                       ("cross_weight", cross_weight, (n_sphere_a, spheres_b.n_sphere))) if t is not None]
    for name, t, _ in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    both = [(what, q_b)] + ([] if fixed_b is None else [("fixed_qpos_b", fixed_b)])
    for name, t in both:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    for name, t in [(n, t) for n, t, _ in named] + both:
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    for name, t, shape in named:
        if (B is not None or shape[0] is not None) and tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    if q_b.ndim != 2 or q_b.shape[1] != n_in:
        raise ValueError(f"{what} must have shape (B, {n_in}), got {tuple(q_b.shape)}")
    if B is not None and q_b.shape[0] != B:
        raise ValueError(f"the first robot has {B} frames, {what} {q_b.shape[0]}: both robots need one row per frame")
    if n_fixed > 0 and fixed_b is None:
        raise ValueError(f"the other optimizer has {n_fixed} fixed joints: fixed_qpos_b of shape ({q_b.shape[0]}, {n_fixed}) is required")
    if fixed_b is not None and tuple(fixed_b.shape) != (q_b.shape[0], n_fixed):
        raise ValueError(f"fixed_qpos_b must have shape ({q_b.shape[0]}, {n_fixed}), got {tuple(fixed_b.shape)}")
    return pairs_b, [(n, t) for n, t, _ in named] + both


def _resolve_cross(side_a, side_b, margin, cross_margin, other_pos, other_rot, cross_weight, pair_weight, w_x, damping, max_iters, posture_weight,
                   q_ref, collision_weight, link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits):
    """every rule (those of `_resolve`, then the other robot's, the device last), then two models and one launch."""
    import torch

    n_in, n_fixed, kin, robot, x0, fixed_qpos, sphere_set, what, model_of = side_a
    named = _resolve_rules(n_in, x0, sphere_set, damping, max_iters, posture_weight, q_ref, collision_weight, link_names, target_pos,
                           target_rot, pos_weight, rot_weight, tol, max_step, limits)
    for n in link_names or ():
        kin.body_frame_index(n)  # ValueError on an unknown link
    pairs_b, named_b = _cross_resolve_rules(side_b, x0, sphere_set.n_sphere, cross_margin, w_x, other_pos, other_rot, cross_weight)
    pairs = _check(n_in, n_fixed, kin, robot, x0, fixed_qpos, sphere_set, what, margin, pair_weight, penalty=True)  # (ends with the device)
    for name, t in named + named_b:
        if t.device != x0.device:
            raise ValueError(f"{name} is on {t.device}, {what} on {x0.device}: all tensors must be on one CUDA device")
    B = x0.shape[0]
    xc, fixed = _inputs(x0, fixed_qpos)
    xb, fixed_b = _inputs(side_b[4], side_b[5])
    c = lambda a: None if a is None else a.detach().contiguous()  # noqa: E731
    xr, tp, tr, wl, wa, pw, op, orot, xw = (c(a) for a in (q_ref, target_pos, target_rot, pos_weight, rot_weight, pair_weight, other_pos, other_rot,
                                                          cross_weight))
    lo, hi = (None, None) if limits is None else (limits.detach()[:, 0].contiguous(), limits.detach()[:, 1].contiguous())
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x0.device):
        if isinstance(posture_weight, torch.Tensor):
            u = c(posture_weight)
        else:
            u = None if not posture_weight else torch.full((n_in,), float(posture_weight), dtype=torch.float32, device=x0.device)
        model = model_of(sphere_set, pairs, tuple(link_names or ()))
        model_b = side_b[8](side_b[6], pairs_b)
        q = torch.empty((B, model.n_in), dtype=torch.float32, device=x0.device)
        iters = torch.empty((B,), dtype=torch.int32, device=x0.device)
        energy = torch.empty((B, 4), dtype=torch.float32, device=x0.device)
        status = torch.empty((B,), dtype=torch.int32, device=x0.device)
        if B > 0:
            model.resolve_cross_dev(model_b, B, xc.data_ptr(), ptr(fixed), xb.data_ptr(), ptr(fixed_b), float(margin), float(damping),
                                    int(max_iters), q.data_ptr(), iters.data_ptr(), energy.data_ptr(), status.data_ptr(), x_ref_ptr=ptr(xr),
                                    posture_weight_ptr=ptr(u), n_target=len(link_names or ()), target_pos_ptr=ptr(tp), target_rot_ptr=ptr(tr),
                                    pos_weight_ptr=ptr(wl), rot_weight_ptr=ptr(wa), collision_weight=float(collision_weight),
                                    pair_weight_ptr=ptr(pw), lo_ptr=ptr(lo), hi_ptr=ptr(hi), tol=float(tol), max_step=float(max_step),
                                    other_pos_ptr=ptr(op), other_rot_ptr=ptr(orot), cross_margin=None if cross_margin is None else float(cross_margin),
                                    cross_weight=float(w_x), cross_pair_weight_ptr=ptr(xw), stream=torch.cuda.current_stream(x0.device).cuda_stream)
    return q, iters, energy, status


def resolve_cross_collisions(optimizer_a, q0_a, spheres_a: SphereSet, optimizer_b, q_b, spheres_b: SphereSet, margin, cross_margin=None,
                             other_pos=None, other_rot=None, cross_weight=None, pair_weight=None, w_x=1.0, damping=_REQUIRED,
                             max_iters=_REQUIRED, posture_weight=None, q_ref=None, collision_weight=1.0, link_names=None, target_pos=None,
                             target_rot=None, pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None, fixed_qpos_a=None,
                             fixed_qpos_b=None):
    """`resolve_self_collision` for robot A against a SECOND ROBOT held still: B stays at q_b (B, n_opt_b) with the pose other_pos
    (B, 3), other_rot (B, 3, 3) of its root IN A'S ROOT FRAME per frame (None: zero translation / identity) and acts as a body made of
    its spheres.  ONE launch descends on

        E = E of resolve_self_collision (A) + w_x * sum_s sum_t w_st max(0, cross_margin - d_st)^2

    over every sphere s of A and t of B, the energy of `cross_penalty`; only A's variables move.  cross_margin: a Python float >= 0
    or None (margin); cross_weight (S_a, S_b) float32 >= 0 or None (1), a zero masks a pair; w_x a Python float >= 0.  Every other
    argument, the accept / reject rule and the damping are those of `resolve_self_collision`, for A.  -> (q (B, n_opt_a) float32,
    iters (B) int32, energy (B, 4) float32: pose, posture, self-collision and the cross term at q, status (B) int32).  The curvature
    uses the first 256 active contacts in the order of A's spheres, then B's; a point with more sets
    _lib.RESOLVE_CONTACTS_TRUNCATED.  B's pair list plays no part; the two optimisers may be one.  No autograd graph."""
    return _resolve_cross(_optimizer_side(optimizer_a, q0_a, spheres_a, fixed_qpos_a, "a"), _optimizer_side(optimizer_b, q_b, spheres_b, fixed_qpos_b, "b"),
                          margin, cross_margin, other_pos, other_rot, cross_weight, pair_weight, w_x, damping, max_iters, posture_weight, q_ref,
                          collision_weight, link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits)


def robot_resolve_cross_collisions(robot_a, qpos0_a, spheres_a: SphereSet, robot_b, qpos_b, spheres_b: SphereSet, margin, cross_margin=None,
                                   other_pos=None, other_rot=None, cross_weight=None, pair_weight=None, w_x=1.0, damping=_REQUIRED,
                                   max_iters=_REQUIRED, posture_weight=None, q_ref=None, collision_weight=1.0, link_names=None, target_pos=None,
                                   target_rot=None, pos_weight=None, rot_weight=None, tol=0.0, max_step=0.0, limits=None):
    """The same for full robot qpos (B, robot.dof) in dof order; every joint is a column of its own, limits (robot_a.dof, 2)."""
    return _resolve_cross(_robot_side(robot_a, qpos0_a, spheres_a, "a"), _robot_side(robot_b, qpos_b, spheres_b, "b"), margin, cross_margin,
                          other_pos, other_rot, cross_weight, pair_weight, w_x, damping, max_iters, posture_weight, q_ref, collision_weight,
                          link_names, target_pos, target_rot, pos_weight, rot_weight, tol, max_step, limits)


def relative_pose(pos_a, rot_a, pos_b, rot_b):
    """the pose of B's root in A's root frame from two world poses, in torch on their device: (rot_a^T (pos_b - pos_a), rot_a^T rot_b)."""
    rt = rot_a.transpose(1, 2)
    return (rt @ (pos_b - pos_a).unsqueeze(-1)).squeeze(-1).contiguous(), (rt @ rot_b).contiguous()


def resolve_bimanual_collisions(optimizer_a, q_a, spheres_a: SphereSet, optimizer_b, q_b, spheres_b: SphereSet, margin, pos_a, rot_a, pos_b,
                                rot_b, sweeps=1, cross_margin=None, cross_weight=None, w_x=1.0, damping=_REQUIRED, max_iters=_REQUIRED,
                                args_a=None, args_b=None, fixed_qpos_a=None, fixed_qpos_b=None):
    """Two robots with world poses pos_* (B, 3), rot_* (B, 3, 3) float32 CUDA, both free: per sweep `resolve_cross_collisions` of A
    against B held, then of B against the new A, each in its own root frame (the relative pose and its inverse are formed in torch on
    the device: no host synchronisation between the launches).  args_a / args_b: dicts of the remaining keyword arguments of
    `resolve_self_collision` for that robot alone -- pair_weight, posture_weight, q_ref, collision_weight, link_names, target_pos,
    target_rot, pos_weight, rot_weight, tol, max_step, limits; each robot keeps its own self-pair list, limits, references and
    targets.  Both launches of a sweep use the same cross_weight (S_a, S_b) (transposed for the second), cross_margin and w_x, so the
    cross term is ONE symmetric energy: the sum of both robots' energies with the cross term counted once cannot rise from sweep
    to sweep.  -> ((q_a, iters_a, energy_a, status_a), (q_b, iters_b, energy_b, status_b)) of the last sweep."""
    import torch

    if isinstance(sweeps, bool) or not isinstance(sweeps, int) or sweeps < 1:
        raise ValueError(f"sweeps must be a Python int >= 1, got {sweeps!r}")
    args_a, args_b = dict(args_a or {}), dict(args_b or {})
    own = {"pair_weight", "posture_weight", "q_ref", "collision_weight", "link_names", "target_pos", "target_rot", "pos_weight", "rot_weight", "tol",
           "max_step", "limits"}
    for name, a in (("args_a", args_a), ("args_b", args_b)):
        if set(a) - own:
            raise ValueError(f"{name} holds {sorted(set(a) - own)}: it takes {sorted(own)}")
    B = q_a.shape[0] if isinstance(q_a, torch.Tensor) and q_a.ndim == 2 else None
    for name, t, shape in (("pos_a", pos_a, (B, 3)), ("rot_a", rot_a, (B, 3, 3)), ("pos_b", pos_b, (B, 3)), ("rot_b", rot_b, (B, 3, 3))):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if B is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    if isinstance(cross_weight, torch.Tensor) and cross_weight.ndim != 2:
        raise ValueError(f"cross_weight must have shape (S_a, S_b), got {tuple(cross_weight.shape)}")
    ab = relative_pose(pos_a, rot_a, pos_b, rot_b)  # B in A's root frame
    ba = relative_pose(pos_b, rot_b, pos_a, rot_a)  # A in B's
    wt = cross_weight.t().contiguous() if isinstance(cross_weight, torch.Tensor) else cross_weight
    if args_a.get("q_ref") is None:
        args_a["q_ref"] = q_a  # the posture term refers to the first point in every sweep: one energy
    if args_b.get("q_ref") is None:
        args_b["q_ref"] = q_b
    ra = rb = None
    for _ in range(sweeps):
        ra = resolve_cross_collisions(optimizer_a, q_a, spheres_a, optimizer_b, q_b, spheres_b, margin, cross_margin, ab[0], ab[1], cross_weight,
                                      w_x=w_x, damping=damping, max_iters=max_iters, fixed_qpos_a=fixed_qpos_a, fixed_qpos_b=fixed_qpos_b, **args_a)
        q_a = ra[0]
        rb = resolve_cross_collisions(optimizer_b, q_b, spheres_b, optimizer_a, q_a, spheres_a, margin, cross_margin, ba[0], ba[1], wt,
                                      w_x=w_x, damping=damping, max_iters=max_iters, fixed_qpos_a=fixed_qpos_b, fixed_qpos_b=fixed_qpos_a, **args_b)
        q_b = rb[0]
    return ra, rb


__all__ = ["SphereSet", "default_pairs", "sphere_distances", "self_collision_penalty", "robot_sphere_distances",
           "robot_self_collision_penalty", "resolve_self_collision", "robot_resolve_self_collision", "ObstacleSet", "obstacle_distances",
           "obstacle_penalty", "robot_obstacle_distances", "robot_obstacle_penalty", "resolve_collisions", "robot_resolve_collisions", "SdfGrid",
           "grid_distances", "grid_penalty", "robot_grid_distances", "robot_grid_penalty", "resolve_grid_collisions",
           "robot_resolve_grid_collisions", "TriangleMesh", "mesh_distances", "SceneBody", "resolve_scene_collisions",
           "robot_resolve_scene_collisions", "cross_distances", "cross_penalty", "robot_cross_distances", "robot_cross_penalty",
           "resolve_cross_collisions", "robot_resolve_cross_collisions", "relative_pose", "resolve_bimanual_collisions", "SphereFit", "fit_spheres", "link_grid",
           "DeviceSdfGrid"]

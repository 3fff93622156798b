"""Batched link Jacobians, link velocities, link wrenches and damped least-squares IK steps on the GPU
(include/dexr_jacobian.h, include/dexr_wrench.h, include/dexr_ik.h, csrc/dexr_pose.hip), for torch tensors.

``link_jacobians(optimizer, q, link_names)`` gives ``J = d(pose)/dq`` of any links at the optimiser's variables -- the matrix a
differential-IK or impedance step, a null-space projector, a manipulability measure or a contact Jacobian needs -- and
``link_velocities`` the contraction ``J qdot`` without forming the matrix.  Both run one kernel per table of 64 links on the
current torch stream.

    jlin[b, l, :, c] = sum_k mult_k (a_k x (p_l - o_k) | a_k)        jang[b, l, :, c] = sum_k mult_k (a_k | 0)
                                     revolute            prismatic                                  revolute prismatic

over the joints k on the chain of link l that column c drives: a mimic joint lands on the column of its source with its
multiplier.  ``frame="world"`` is the velocity of the link origin and the angular velocity in world axes (pinocchio's
LOCAL_WORLD_ALIGNED), ``frame="local"`` rotates both into the link's own axes (pinocchio's LOCAL, what
``RobotWrapper.compute_single_link_local_jacobian`` returns).

``link_wrenches(optimizer, q, link_names, force, torque)`` is the transposed product ``tau = sum_l Jlin_l^T force_l +
Jang_l^T torque_l`` -- joint torques of contact forces, a differential-IK step of the J^T kind -- again without the matrix.

``link_ik_step(optimizer, q, link_names, pos_err, rot_err, ..., damping=lam)`` is one damped least-squares
(Levenberg-Marquardt) step towards per-link displacements and small rotations,

    dq = (sum_l w_pos Jlin_l^T Jlin_l + w_rot Jang_l^T Jang_l + lam I)^-1 (sum_l w_pos Jlin_l^T pos_err_l + w_rot Jang_l^T rot_err_l),

built, factorised (Cholesky) and solved inside one kernel: neither J nor the normal matrix reaches memory.

``link_ik_solve(optimizer, q0, link_names, target_pos, target_rot, ..., damping=lam, max_iters=n, limits=lim)`` iterates that
step inside ONE kernel towards world pose targets, with joint limits (bound variables the step pushes outward are frozen) and
a per-frame stop: -> (q, iters, err) (include/dexr_ik_solve.h).

The outputs carry NO autograd graph: the functions of this module build no derivative of theirs (a VJP of the IK step is not
built either).  Where a loss needs
gradients, differentiate through ``autograd.link_poses`` (poses) or ``autograd.link_velocities`` (velocities, in q and qdot:
the kinematic Hessian contracted on both sides by a kernel of its own).
"""
from __future__ import annotations

from . import _lib
from .autograd import _check_poses

_FRAMES = {"world": _lib.JAC_WORLD_ALIGNED, "local": _lib.JAC_LOCAL}
_REQUIRED = object()  # damping of an IK step: an argument without a default that may still be passed by position


def _check(n_in, n_fixed, q, qdot, fixed_qpos, link_names, frame, kin, what="q", rows=(), weights=()):
    """Every argument rule -- the frame, types, dtypes, shapes, the link names and last the device -- before anything
    touches the GPU.  Returns the DEXR_JAC_* value of `frame`.  `qdot`: False where the call takes none.  `rows`: (name,
    tensor) pairs that must be float32 (B, L, 3) tensors on q's device, one row per link; `weights`: the same for (B, L)
    tensors, one value per link."""
    import torch

    if not isinstance(frame, str) or frame not in _FRAMES:
        raise ValueError(f"frame must be 'world' or 'local', got {frame!r}")
    if qdot is not False:
        if not isinstance(qdot, torch.Tensor):
            raise ValueError(f"the rate of {what} must be a torch tensor")
        if qdot.dtype != torch.float32:
            raise ValueError(f"the rate of {what} must be float32, got {qdot.dtype}")
        if isinstance(q, torch.Tensor) and tuple(qdot.shape) != tuple(q.shape):
            raise ValueError(f"the rate of {what} must have its shape {tuple(q.shape)}, got {tuple(qdot.shape)}")
    for name, t in rows:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if isinstance(q, torch.Tensor) and q.ndim == 2 and not isinstance(link_names, str) and \
                tuple(t.shape) != (q.shape[0], len(link_names), 3):
            raise ValueError(f"{name} must have shape ({q.shape[0]}, {len(link_names)}, 3), got {tuple(t.shape)}")
    for name, t in weights:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
        if isinstance(q, torch.Tensor) and q.ndim == 2 and not isinstance(link_names, str) and \
                tuple(t.shape) != (q.shape[0], len(link_names)):
            raise ValueError(f"{name} must have shape ({q.shape[0]}, {len(link_names)}), got {tuple(t.shape)}")
    if not isinstance(link_names, str):
        for n in link_names:
            kin.body_frame_index(n)  # ValueError on an unknown link
    _check_poses(n_in, n_fixed, q, fixed_qpos, link_names, what=what)  # (ends with the device)
    if qdot is not False and qdot.device != q.device:
        raise ValueError(f"the rate is on {qdot.device}, {what} on {q.device}: all tensors must be on one CUDA device")
    for name, t in tuple(rows) + tuple(weights):
        if t.device != q.device:
            raise ValueError(f"{name} is on {t.device}, {what} on {q.device}: all tensors must be on one CUDA device")
    return _FRAMES[frame]


def _chunks(names):
    names = list(names)
    return [names[c:c + 64] for c in range(0, len(names), 64)]


def _cat(parts):
    import torch

    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


def _jacobians(model_of, x, fixed_qpos, link_names, frame, angular):
    """chunks of 64 links -> one table and one launch each, results concatenated along the link axis."""
    import torch

    B = x.shape[0]
    xc = x.detach().contiguous()
    fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
    lin, ang = [], []
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        for names in _chunks(link_names):
            model = model_of(names)
            jl = torch.empty((B, model.n_link, 3, model.n_in), dtype=torch.float32, device=x.device)
            ja = torch.empty_like(jl) if angular else None
            if B > 0:
                model.jacobians_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), jl.data_ptr(),
                                    0 if ja is None else ja.data_ptr(), frame=frame, stream=stream)
            lin.append(jl)
            ang.append(ja)
    return _cat(lin), (_cat(ang) if angular else None)


def _velocities(model_of, x, xdot, fixed_qpos, link_names, frame, angular):
    import torch

    B = x.shape[0]
    xc, xd = x.detach().contiguous(), xdot.detach().contiguous()
    fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
    lin, ang = [], []
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        for names in _chunks(link_names):
            model = model_of(names)
            vl = torch.empty((B, model.n_link, 3), dtype=torch.float32, device=x.device)
            va = torch.empty_like(vl) if angular else None
            if B > 0:
                model.velocities_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), xd.data_ptr(), vl.data_ptr(),
                                     0 if va is None else va.data_ptr(), frame=frame, stream=stream)
            lin.append(vl)
            ang.append(va)
    return _cat(lin), (_cat(ang) if angular else None)


def _wrench_rows(force, torque):
    if force is None and torque is None:
        raise ValueError("force and torque are both None: at least one of them is required")
    return [(n, t) for n, t in (("force", force), ("torque", torque)) if t is not None]


def _wrenches(model_of, x, fixed_qpos, link_names, frame, force, torque):
    """chunks of 64 links -> one table and one launch each, the chunks' torques summed."""
    import torch

    B = x.shape[0]
    xc = x.detach().contiguous()
    fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
    tau = None
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        at = 0
        for names in _chunks(link_names):
            model = model_of(names)
            f, t = (None if a is None else a.detach()[:, at:at + len(names)].contiguous() for a in (force, torque))
            at += len(names)
            part = torch.empty((B, model.n_in), dtype=torch.float32, device=x.device)
            if B > 0:
                model.wrenches_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), 0 if f is None else f.data_ptr(),
                                   0 if t is None else t.data_ptr(), part.data_ptr(), frame=frame, stream=stream)
            tau = part if tau is None else tau + part
    return tau


def _ik_rows(pos_err, rot_err, pos_weight, rot_weight, damping, link_names):
    """the rules of an IK step that need no tensor looked at -> (rows, weights) for _check."""
    import math

    if pos_err is None and rot_err is None:
        raise ValueError("pos_err and rot_err are both None: at least one of them is required")
    if pos_weight is not None and pos_err is None:
        raise ValueError("pos_weight given without pos_err")
    if rot_weight is not None and rot_err is None:
        raise ValueError("rot_weight given without rot_err")
    if damping is _REQUIRED:
        raise ValueError("damping is required: a positive finite Python float (there is no default)")
    if isinstance(damping, bool) or not isinstance(damping, (int, float)) or not math.isfinite(damping) or damping <= 0:
        raise ValueError(f"damping must be a positive finite Python float, got {damping!r}")
    if not isinstance(link_names, str) and len(link_names) > 64:
        raise ValueError(f"an IK step takes at most 64 links (one pose table), got {len(link_names)}: the normal matrix "
                         "cannot be split across tables")
    rows = [(n, t) for n, t in (("pos_err", pos_err), ("rot_err", rot_err)) if t is not None]
    weights = [(n, t) for n, t in (("pos_weight", pos_weight), ("rot_weight", rot_weight)) if t is not None]
    return rows, weights


def _ik_step(model_of, x, fixed_qpos, link_names, frame, pos_err, rot_err, pos_weight, rot_weight, damping):
    """one table, one launch."""
    import torch

    B = x.shape[0]
    xc = x.detach().contiguous()
    fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
    el, ea, wl, wa = (None if a is None else a.detach().contiguous() for a in (pos_err, rot_err, pos_weight, rot_weight))
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        model = model_of(list(link_names))
        dq = torch.empty((B, model.n_in), dtype=torch.float32, device=x.device)
        if B > 0:
            model.ik_step_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), 0 if el is None else el.data_ptr(),
                              0 if ea is None else ea.data_ptr(), 0 if wl is None else wl.data_ptr(),
                              0 if wa is None else wa.data_ptr(), float(damping), dq.data_ptr(), frame=frame, stream=stream)
    return dq


def _ik_solve_rules(q0, link_names, target_pos, target_rot, pos_weight, rot_weight, damping, max_iters, tol, max_step, limits, n_in):
    """the rules of an IK solve beyond those of _check (the targets' types and shapes, the scalars, the limits) -> (rows,
    weights) for _check.  Nothing here looks at a device; the device rule of the targets and the limits comes after _check."""
    import math

    import torch

    if target_pos is None and target_rot is None:
        raise ValueError("target_pos and target_rot are both None: at least one of them is required")
    if pos_weight is not None and target_pos is None:
        raise ValueError("pos_weight given without target_pos")
    if rot_weight is not None and target_rot is None:
        raise ValueError("rot_weight given without target_rot")
    if damping is _REQUIRED:
        raise ValueError("damping is required: a positive finite Python float (there is no default)")
    if isinstance(damping, bool) or not isinstance(damping, (int, float)) or not math.isfinite(damping) or damping <= 0:
        raise ValueError(f"damping must be a positive finite Python float, got {damping!r}")
    if max_iters is _REQUIRED:
        raise ValueError("max_iters is required: a Python int in 1..256 (there is no default)")
    if isinstance(max_iters, bool) or not isinstance(max_iters, int) or not 1 <= max_iters <= 256:
        raise ValueError(f"max_iters must be a Python int in 1..256, got {max_iters!r}")
    for name, v in (("tol", tol), ("max_step", max_step)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite Python float >= 0, got {v!r}")
    if not isinstance(link_names, str) and len(link_names) > 64:
        raise ValueError(f"an IK solve takes at most 64 links (one pose table), got {len(link_names)}: the normal matrix "
                         "cannot be split across tables")
    if target_rot is not None:
        if not isinstance(target_rot, torch.Tensor):
            raise ValueError("target_rot must be a torch tensor")
        if target_rot.dtype != torch.float32:
            raise ValueError(f"target_rot must be float32, got {target_rot.dtype}")
        if isinstance(q0, torch.Tensor) and q0.ndim == 2 and not isinstance(link_names, str) and \
                tuple(target_rot.shape) != (q0.shape[0], len(link_names), 3, 3):
            raise ValueError(f"target_rot must have shape ({q0.shape[0]}, {len(link_names)}, 3, 3), got {tuple(target_rot.shape)}")
    if limits is not None:
        if not isinstance(limits, torch.Tensor):
            raise ValueError("limits must be a torch tensor")
        if limits.dtype != torch.float32:
            raise ValueError(f"limits must be float32, got {limits.dtype}")
        if tuple(limits.shape) != (n_in, 2):
            raise ValueError(f"limits must have shape ({n_in}, 2), lower and upper bound per variable, got {tuple(limits.shape)}")
    rows = [("target_pos", target_pos)] if target_pos is not None else []
    weights = [(n, t) for n, t in (("pos_weight", pos_weight), ("rot_weight", rot_weight)) if t is not None]
    return rows, weights


def _ik_solve(model_of, n_in, n_fixed, kin, x0, what, fixed_qpos, link_names, target_pos, target_rot, pos_weight, rot_weight, damping,
              max_iters, tol, max_step, limits):
    """every rule, then one table and one launch."""
    import torch

    rows, weights = _ik_solve_rules(x0, link_names, target_pos, target_rot, pos_weight, rot_weight, damping, max_iters, tol, max_step,
                                    limits, n_in)
    _check(n_in, n_fixed, x0, False, fixed_qpos, link_names, "world", kin, what=what, rows=rows, weights=weights)
    for name, t in (("target_rot", target_rot), ("limits", limits)):
        if t is not None and t.device != x0.device:
            raise ValueError(f"{name} is on {t.device}, {what} on {x0.device}: all tensors must be on one CUDA device")
    B = x0.shape[0]
    xc = x0.detach().contiguous()
    fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
    tp, tr, wl, wa = (None if a is None else a.detach().contiguous() for a in (target_pos, target_rot, pos_weight, rot_weight))
    lo, hi = (None, None) if limits is None else (limits.detach()[:, 0].contiguous(), limits.detach()[:, 1].contiguous())
    ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    with torch.cuda.device(x0.device):
        stream = torch.cuda.current_stream(x0.device).cuda_stream
        model = model_of(list(link_names))
        q = torch.empty((B, model.n_in), dtype=torch.float32, device=x0.device)
        iters = torch.empty((B,), dtype=torch.int32, device=x0.device)
        err = torch.empty((B,), dtype=torch.float32, device=x0.device)
        if B > 0:
            model.ik_solve_dev(B, xc.data_ptr(), ptr(fixed), ptr(tp), ptr(tr), ptr(wl), ptr(wa), ptr(lo), ptr(hi), float(damping),
                               int(max_iters), q.data_ptr(), iters.data_ptr(), err.data_ptr(), tol=float(tol), max_step=float(max_step),
                               stream=stream)
    return q, iters, err


def link_jacobians(optimizer, q, link_names, fixed_qpos=None, frame="world", angular=True):
    """Jacobians of `link_names` with respect to the optimiser's variables: q (B, n_opt) float32 CUDA -- what `retarget`
    returns --, fixed_qpos (B, n_fixed) or None -> (jlin (B, L, 3, n_opt), jang of the same shape or None), float32.  Mimic
    joints are folded onto their source's column; columns that move no joint above a link are exact zeros.
    `angular=False` neither computes nor allocates `jang`.  The outputs carry no autograd graph (first derivatives; their
    own derivative is not built)."""
    n_fixed = len(optimizer.idx_pin2fixed)
    f = _check(optimizer.opt_dof, n_fixed, q, False, fixed_qpos, link_names, frame, optimizer.robot.kin)
    return _jacobians(optimizer.pose_model, q, fixed_qpos, link_names, f, angular)


def link_velocities(optimizer, q, qdot, link_names, fixed_qpos=None, frame="world", angular=True):
    """Velocities of `link_names` for the rate qdot (B, n_opt) of the optimiser's variables at q: (lin (B, L, 3) velocity of
    the link origin, ang (B, L, 3) angular velocity or None), float32, = link_jacobians(...) @ qdot without the matrix.  Fixed
    joints are held still.  No autograd graph: `autograd.link_velocities` is the same forward, differentiable in q and qdot."""
    n_fixed = len(optimizer.idx_pin2fixed)
    f = _check(optimizer.opt_dof, n_fixed, q, qdot, fixed_qpos, link_names, frame, optimizer.robot.kin)
    return _velocities(optimizer.pose_model, q, qdot, fixed_qpos, link_names, f, angular)


def link_wrenches(optimizer, q, link_names, force=None, torque=None, fixed_qpos=None, frame="world"):
    """Joint torques of forces and torques on `link_names` at q: force, torque (B, L, 3) float32 or None (not both), in world
    axes at the link origin (`frame="world"`) or in the link's own axes (`"local"`) -> tau (B, n_opt) float32,
    = einsum(jlin, force) + einsum(jang, torque) of `link_jacobians` without the matrix.  Mimic joints add to their source's
    column, fixed joints take no torque.  The output carries no autograd graph (no gradient reaches q, force or torque)."""
    n_fixed = len(optimizer.idx_pin2fixed)
    f = _check(optimizer.opt_dof, n_fixed, q, False, fixed_qpos, link_names, frame, optimizer.robot.kin,
               rows=_wrench_rows(force, torque))
    return _wrenches(optimizer.pose_model, q, fixed_qpos, link_names, f, force, torque)


def link_ik_step(optimizer, q, link_names, pos_err=None, rot_err=None, pos_weight=None, rot_weight=None,
                 damping=_REQUIRED, fixed_qpos=None, frame="world"):
    """One damped least-squares step of the optimiser's variables at q (B, n_opt) float32 CUDA towards pos_err (B, L, 3), the
    desired displacement of each link origin, and / or rot_err (B, L, 3), a small rotation vector -- in world axes at the link
    origin (`frame="world"`) or in the link's own axes (`"local"`) -- weighted per frame and link by pos_weight, rot_weight
    (B, L) float32 >= 0 (None: 1) -> dq (B, n_opt) float32, the minimiser of
    1/2 sum_l (w_pos |Jlin_l dq - pos_err_l|^2 + w_rot |Jang_l dq - rot_err_l|^2) + 1/2 damping |dq|^2.
    `damping` is required: a positive finite Python float (there is no default on purpose).  Mimic joints fold onto their
    source's column, fixed joints do not move, columns no joint reads are exact zeros.  At most 64 links: the normal matrix
    lives in one kernel and cannot be split across tables.  The output carries no autograd graph (a VJP of the step is not
    built); clamp q + dq to the joint limits in torch."""
    rows, weights = _ik_rows(pos_err, rot_err, pos_weight, rot_weight, damping, link_names)
    n_fixed = len(optimizer.idx_pin2fixed)
    f = _check(optimizer.opt_dof, n_fixed, q, False, fixed_qpos, link_names, frame, optimizer.robot.kin, rows=rows, weights=weights)
    return _ik_step(optimizer.pose_model, q, fixed_qpos, link_names, f, pos_err, rot_err, pos_weight, rot_weight, damping)


def link_ik_solve(optimizer, q0, link_names, target_pos=None, target_rot=None, pos_weight=None, rot_weight=None,
                  damping=_REQUIRED, max_iters=_REQUIRED, tol=0.0, max_step=0.0, limits=None, fixed_qpos=None):
    """Inverse kinematics of the optimiser's variables to world pose targets, solved inside ONE launch: from q0 (B, n_opt)
    float32 CUDA, up to `max_iters` (1..256) damped least-squares steps of `link_ik_step` towards target_pos (B, L, 3), the
    world positions of the link origins, and / or target_rot (B, L, 3, 3), their world rotations, weighted per frame and link
    by pos_weight, rot_weight (B, L) float32 >= 0 (None: 1) -> (q (B, n_opt) float32, iters (B) int32, err (B) float32).
    The rotation error of a link is the rotation vector log(target_rot R^T) in world axes (an error of angle pi reads as 0:
    keep targets nearer than that).  A frame stops at the first iterate whose err = sqrt(sum_l w_pos |pos error|^2 + w_rot
    |rot error|^2) is <= tol, or at max_iters; `iters` is the number of steps it took and `err` the error at the q returned.
    limits (n_opt, 2) float32 or None are lower and upper bounds shared by the batch: a variable on a bound that the step
    would push outward is frozen before the solve (its step is exactly 0), and every iterate is clamped.  max_step > 0 scales
    a step so that its largest entry is max_step at most.  `damping` and `max_iters` are required (no defaults on purpose).
    Mimic joints fold onto their source's column, fixed joints do not move, variables no joint reads come back unchanged.  At
    most 64 links.  The outputs carry no autograd graph.  One step alone, with errors of your own: `link_ik_step`."""
    return _ik_solve(optimizer.pose_model, optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, q0, "q", fixed_qpos,
                     link_names, target_pos, target_rot, pos_weight, rot_weight, damping, max_iters, tol, max_step, limits)


def robot_link_ik_solve(robot, qpos0, link_names, target_pos=None, target_rot=None, pos_weight=None, rot_weight=None,
                        damping=_REQUIRED, max_iters=_REQUIRED, tol=0.0, max_step=0.0, limits=None):
    """(qpos (B, robot.dof), iters (B), err (B)) for a full robot qpos in dof order; every joint is a column of its own, limits
    (robot.dof, 2).  At most 64 links."""
    return _ik_solve(robot.pose_model, robot.dof, 0, robot.kin, qpos0, "qpos", None, link_names, target_pos, target_rot, pos_weight,
                     rot_weight, damping, max_iters, tol, max_step, limits)


def robot_link_jacobians(robot, qpos, link_names, frame="world", angular=True):
    """The same for a full robot qpos (B, robot.dof) in dof order: (jlin (B, L, 3, dof), jang or None).  Every joint is a
    column of its own here, mimic joints included (RobotWrapper does not know about them)."""
    f = _check(robot.dof, 0, qpos, False, None, link_names, frame, robot.kin, what="qpos")
    return _jacobians(robot.pose_model, qpos, None, link_names, f, angular)


def robot_link_velocities(robot, qpos, qvel, link_names, frame="world", angular=True):
    """(lin (B, L, 3), ang or None) for a full robot qpos and its rate qvel, both (B, robot.dof) in dof order."""
    f = _check(robot.dof, 0, qpos, qvel, None, link_names, frame, robot.kin, what="qpos")
    return _velocities(robot.pose_model, qpos, qvel, None, link_names, f, angular)


def robot_link_wrenches(robot, qpos, link_names, force=None, torque=None, frame="world"):
    """tau (B, robot.dof) for a full robot qpos in dof order; every joint is a column of its own."""
    f = _check(robot.dof, 0, qpos, False, None, link_names, frame, robot.kin, what="qpos", rows=_wrench_rows(force, torque))
    return _wrenches(robot.pose_model, qpos, None, link_names, f, force, torque)


def robot_link_ik_step(robot, qpos, link_names, pos_err=None, rot_err=None, pos_weight=None, rot_weight=None,
                       damping=_REQUIRED, frame="world"):
    """dq (B, robot.dof) for a full robot qpos in dof order; every joint is a column of its own.  At most 64 links."""
    rows, weights = _ik_rows(pos_err, rot_err, pos_weight, rot_weight, damping, link_names)
    f = _check(robot.dof, 0, qpos, False, None, link_names, frame, robot.kin, what="qpos", rows=rows, weights=weights)
    return _ik_step(robot.pose_model, qpos, None, link_names, f, pos_err, rot_err, pos_weight, rot_weight, damping)


__all__ = ["link_jacobians", "link_velocities", "link_wrenches", "link_ik_step", "link_ik_solve", "robot_link_jacobians",
           "robot_link_velocities", "robot_link_wrenches", "robot_link_ik_step", "robot_link_ik_solve"]

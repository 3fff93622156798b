"""Differentiable retargeting: ``q = retarget(optimizer, ref_value, last_qpos)`` as a torch autograd function.

The forward is the product solve (``optimizer.device_model()``, ``dexr_retarget_dev``: the same kernels and the same answers
as ``retarget_batch``) enqueued on the current torch stream.  The backward is the implicit-function VJP of the argmin at the
forward's answer (``dexr_retarget_vjp_dev``, MODE_VJP of the general kernel on ``optimizer.vjp_model()``): one exact Hessian,
one factorisation, one solve per frame -- no unrolling of the solver.

    v = H_SS^-1 dL/dq_S          H: exact Hessian of F = f + norm_delta |q - last|^2, S: variables not on a bound
    dL/dlast_qpos = 2 norm_delta v
    dL/dref_value[r] = (dT_r/dr)^T w_r Hess(SmoothL1)(e_r) (J_r v)

Variables that sit on a joint limit are held (zero gradient through them).  ``fixed_qpos``, the DexPilot ``state`` and the
config scalars get no gradient; the DexPilot weights and projection bits are piecewise constant in ref_value and are held.
Frames whose forward solve fell back to last_qpos (non-finite state) and frames whose Hessian is not positive definite at q get
zero gradients.

The task-space half: ``link_poses(optimizer, q, link_names)`` gives positions and rotations of any links at q
(``dexr_link_poses_dev``) and back-propagates through them with the closed-form VJP kernel (``dexr_link_poses_vjp_dev``), so
``keypoints -> retarget -> link_poses -> loss -> backward`` stays on the GPU.  ``link_velocities(optimizer, q, qdot,
link_names)`` does the same for the link velocities J(q) qdot: the forward is ``jacobians.link_velocities``, the backward one
kernel per 64 links (``dexr_link_velocities_vjp_dev``, include/dexr_wrench.h) that gives the gradient in qdot (J^T applied to
the cotangents) and in q (the kinematic Hessian contracted on both sides) without forming a matrix.
"""
from __future__ import annotations

STATUS_FALLBACK = 2  # == DEXR_STATUS_FALLBACK


def _check(optimizer, ref_value, last_qpos, fixed_qpos, state):
    """Every argument rule -- types, dtypes, shapes, then the device -- before anything touches the GPU."""
    import torch

    if not isinstance(ref_value, torch.Tensor) or not isinstance(last_qpos, torch.Tensor):
        raise ValueError("ref_value and last_qpos must be torch tensors")
    named = [("ref_value", ref_value), ("last_qpos", last_qpos)]
    if fixed_qpos is not None:
        if not isinstance(fixed_qpos, torch.Tensor):
            raise ValueError("fixed_qpos must be a torch tensor")
        named.append(("fixed_qpos", fixed_qpos))
    for name, t in named:
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if last_qpos.ndim != 2 or last_qpos.shape[1] != optimizer.opt_dof:
        raise ValueError(f"last_qpos must have shape (B, {optimizer.opt_dof}), got {tuple(last_qpos.shape)}")
    B = last_qpos.shape[0]
    n_ref = int(optimizer.compiled_model().n_ref)
    if tuple(ref_value.shape) != (B, n_ref, 3):
        raise ValueError(f"ref_value must have shape ({B}, {n_ref}, 3), got {tuple(ref_value.shape)}")
    n_fixed = len(optimizer.idx_pin2fixed)
    if n_fixed > 0 and fixed_qpos is None:
        raise ValueError(f"the optimizer has {n_fixed} fixed joints: fixed_qpos of shape ({B}, {n_fixed}) is required")
    if fixed_qpos is not None and tuple(fixed_qpos.shape) != (B, n_fixed):
        raise ValueError(f"fixed_qpos must have shape ({B}, {n_fixed}), got {tuple(fixed_qpos.shape)}")
    if state is not None:
        if not isinstance(state, torch.Tensor) or state.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or \
                tuple(state.shape) != (B,) or not state.is_contiguous():
            raise ValueError(f"state must be a contiguous int32 / uint32 torch tensor of shape ({B},)")
        named.append(("state", state))
    dev = last_qpos.device
    if dev.type != "cuda":
        raise ValueError(f"the tensors must be CUDA (HIP) tensors, got device {dev}")
    for name, t in named:
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, last_qpos on {dev}: all tensors must be on one CUDA device")


def _make_function():
    import torch

    class _Retarget(torch.autograd.Function):
        @staticmethod
        def forward(ctx, ref_value, last_qpos, fixed_qpos, state, optimizer):
            B = last_qpos.shape[0]
            ref = ref_value.detach().contiguous()
            last = last_qpos.detach().contiguous()
            fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
            # the bits the forward READS: the solve updates `state` in place, the backward needs them as they were
            state_in = None if state is None else state.clone()
            q = torch.empty_like(last)
            status = torch.zeros(B, dtype=torch.int32, device=last.device)
            stream = torch.cuda.current_stream(last.device).cuda_stream
            if B > 0:
                optimizer.device_model().retarget_dev(
                    B, ref.data_ptr(), 0 if fixed is None else fixed.data_ptr(), last.data_ptr(),
                    0 if state is None else state.data_ptr(), q.data_ptr(), status.data_ptr(),
                    opts=optimizer._options(), stream=stream)
            ctx.optimizer = optimizer
            ctx.has_fixed = fixed is not None
            ctx.has_state = state_in is not None
            saved = [ref, last, q, status] + ([fixed] if fixed is not None else []) + ([state_in] if state_in is not None else [])
            ctx.save_for_backward(*saved)
            return q

        @staticmethod
        def backward(ctx, grad_q):
            if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
                return None, None, None, None, None
            saved = list(ctx.saved_tensors)
            ref, last, q, status = saved[:4]
            rest = saved[4:]
            fixed = rest.pop(0) if ctx.has_fixed else None
            state_in = rest.pop(0) if ctx.has_state else None
            B = last.shape[0]
            gq = grad_q.detach().to(torch.float32).contiguous()
            gref = torch.zeros_like(ref)
            glast = torch.zeros_like(last)
            if B > 0:
                vstatus = torch.zeros(B, dtype=torch.int32, device=last.device)
                stream = torch.cuda.current_stream(last.device).cuda_stream
                ctx.optimizer.vjp_model().vjp_dev(
                    B, ref.data_ptr(), 0 if fixed is None else fixed.data_ptr(), last.data_ptr(),
                    0 if state_in is None else state_in.data_ptr(), q.data_ptr(), gq.data_ptr(), gref.data_ptr(),
                    glast.data_ptr(), vstatus.data_ptr(), stream=stream)
                # a forward that fell back to last_qpos returned no minimiser: no implicit gradient for that frame
                keep = (status != STATUS_FALLBACK).to(torch.float32)
                gref = gref * keep[:, None, None]
                glast = glast * keep[:, None]
            return (gref if ctx.needs_input_grad[0] else None, glast if ctx.needs_input_grad[1] else None, None, None, None)

    return _Retarget


_FN = None


def retarget(optimizer, ref_value, last_qpos, fixed_qpos=None, state=None):
    """Differentiable batched solve: ref_value (B, n_ref, 3), last_qpos (B, n_opt), fixed_qpos (B, n_fixed) or None -- float32
    CUDA tensors -- and the DexPilot projection bits `state` (B,) int32 (updated in place, as retarget_batch does; None: zero
    bits, not carried) -> q (B, n_opt) float32.  Gradients flow to ref_value and last_qpos."""
    global _FN
    _check(optimizer, ref_value, last_qpos, fixed_qpos, state)
    if _FN is None:
        _FN = _make_function()
    import torch

    with torch.cuda.device(last_qpos.device):
        return _FN.apply(ref_value, last_qpos, fixed_qpos, state, optimizer)


def ref_value_from_keypoints(optimizer, keypoints):
    """ref_value (B, n_ref, 3) from raw hand keypoints (B, n_keypoints, 3) in torch -- the gather retarget_keypoints_batch does
    inside the kernel: kp[task] - kp[origin] for vector / DexPilot rows, kp[idx] for position rows -- so that gradients reach
    the keypoints."""
    import torch

    hi = optimizer.target_link_human_indices
    if hi is None:
        raise ValueError("this optimizer carries no target_link_human_indices")
    if not isinstance(keypoints, torch.Tensor) or keypoints.ndim != 3 or keypoints.shape[2] != 3:
        raise ValueError("keypoints must be a (B, n_keypoints, 3) torch tensor")
    idx = torch.as_tensor(hi, dtype=torch.long, device=keypoints.device)
    if idx.ndim == 1:
        return keypoints[:, idx]
    return keypoints[:, idx[1]] - keypoints[:, idx[0]]


# ---- task space: link poses of q, differentiable ---------------------------------------------------------------------
def _check_poses(n_in, n_fixed, q, fixed_qpos, link_names, what="q"):
    """Every argument rule -- types, dtypes, shapes, then the device -- before anything touches the GPU."""
    import torch

    if not isinstance(q, torch.Tensor):
        raise ValueError(f"{what} must be a torch tensor")
    if isinstance(link_names, str) or len(link_names) == 0:
        raise ValueError("link_names must be a non-empty sequence of link names")
    named = [(what, q)]
    if fixed_qpos is not None:
        if not isinstance(fixed_qpos, torch.Tensor):
            raise ValueError("fixed_qpos must be a torch tensor")
        named.append(("fixed_qpos", fixed_qpos))
    for name, t in named:
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if q.ndim != 2 or q.shape[1] != n_in:
        raise ValueError(f"{what} must have shape (B, {n_in}), got {tuple(q.shape)}")
    B = q.shape[0]
    if n_fixed > 0 and fixed_qpos is None:
        raise ValueError(f"the optimizer has {n_fixed} fixed joints: fixed_qpos of shape ({B}, {n_fixed}) is required")
    if fixed_qpos is not None and tuple(fixed_qpos.shape) != (B, n_fixed):
        raise ValueError(f"fixed_qpos must have shape ({B}, {n_fixed}), got {tuple(fixed_qpos.shape)}")
    dev = q.device
    if dev.type != "cuda":
        raise ValueError(f"the tensors must be CUDA (HIP) tensors, got device {dev}")
    for name, t in named:
        if t.device != dev:
            raise ValueError(f"{name} is on {t.device}, {what} on {dev}: all tensors must be on one CUDA device")


def _make_pose_function():
    import torch

    class _LinkPoses(torch.autograd.Function):
        """One chunk of at most 64 links (one pose table).  Saves x (and fixed) only: the VJP kernel recomputes the walk."""

        @staticmethod
        def forward(ctx, x, fixed_qpos, model, rotations):
            B = x.shape[0]
            xc = x.detach().contiguous()
            fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
            pos = torch.empty((B, model.n_link, 3), dtype=torch.float32, device=x.device)
            rot = torch.empty((B, model.n_link, 3, 3), dtype=torch.float32, device=x.device) if rotations else None
            if B > 0:
                model.poses_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), pos.data_ptr(),
                                0 if rot is None else rot.data_ptr(), stream=torch.cuda.current_stream(x.device).cuda_stream)
            ctx.model = model
            ctx.has_fixed = fixed is not None
            ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None -> NULL for the kernel
            ctx.save_for_backward(*([xc] + ([fixed] if fixed is not None else [])))
            if rot is None:
                return pos
            return pos, rot

        @staticmethod
        def backward(ctx, grad_pos, grad_rot=None):
            if not ctx.needs_input_grad[0] or (grad_pos is None and grad_rot is None):
                return None, None, None, None
            saved = list(ctx.saved_tensors)
            x = saved[0]
            fixed = saved[1] if ctx.has_fixed else None
            B = x.shape[0]
            gp = None if grad_pos is None else grad_pos.detach().to(torch.float32).contiguous()
            gr = None if grad_rot is None else grad_rot.detach().to(torch.float32).contiguous()
            gx = torch.zeros_like(x)
            if B > 0:
                ctx.model.vjp_dev(B, x.data_ptr(), 0 if fixed is None else fixed.data_ptr(), 0 if gp is None else gp.data_ptr(),
                                  0 if gr is None else gr.data_ptr(), gx.data_ptr(),
                                  stream=torch.cuda.current_stream(x.device).cuda_stream)
            return gx, None, None, None

    return _LinkPoses


_POSE_FN = None


def _link_poses(model_of, x, fixed_qpos, link_names, rotations):
    """chunks of 64 links -> one table each, results concatenated along the link axis."""
    global _POSE_FN
    import torch

    if _POSE_FN is None:
        _POSE_FN = _make_pose_function()
    names = list(link_names)
    pos, rot = [], []
    with torch.cuda.device(x.device):
        for c in range(0, len(names), 64):
            out = _POSE_FN.apply(x, fixed_qpos, model_of(names[c:c + 64]), bool(rotations))
            if rotations:
                pos.append(out[0])
                rot.append(out[1])
            else:
                pos.append(out)
    if len(pos) == 1:
        return pos[0], (rot[0] if rotations else None)
    return torch.cat(pos, dim=1), (torch.cat(rot, dim=1) if rotations else None)


def link_poses(optimizer, q, link_names, fixed_qpos=None, rotations=True):
    """World poses of `link_names` at the optimiser's variables: q (B, n_opt) float32 CUDA -- what `retarget` returns --,
    fixed_qpos (B, n_fixed) or None -> (pos (B, L, 3), rot (B, L, 3, 3) or None), float32, rotations row-major in the
    URDF's own link frames.  Mimic joints follow their source.  Gradients flow to q only; `rotations=False` neither
    computes nor allocates `rot`."""
    n_fixed = len(optimizer.idx_pin2fixed)
    _check_poses(optimizer.opt_dof, n_fixed, q, fixed_qpos, link_names)
    for n in link_names:
        optimizer.robot.kin.body_frame_index(n)  # ValueError on an unknown link, before any launch
    return _link_poses(optimizer.pose_model, q, fixed_qpos, link_names, rotations)


def robot_link_poses(robot, qpos, link_names, rotations=True):
    """The same for a full robot qpos (B, robot.dof) in dof order -- what SeqRetargeting / DeviceSeqRetargeting return;
    float64 tensors are converted to float32 once."""
    import torch

    if isinstance(qpos, torch.Tensor) and qpos.dtype == torch.float64:
        qpos = qpos.to(torch.float32)
    _check_poses(robot.dof, 0, qpos, None, link_names, what="qpos")
    for n in link_names:
        robot.kin.body_frame_index(n)
    return _link_poses(robot.pose_model, qpos, None, link_names, rotations)


# ---- task space: link velocities of (q, qdot), differentiable in both ----------------------------------------------------
def _make_velocity_function():
    import torch
    from torch.autograd.function import once_differentiable

    class _LinkVelocities(torch.autograd.Function):
        """One chunk of at most 64 links (one pose table).  Saves x, xdot (and fixed): the VJP kernel recomputes the walk."""

        @staticmethod
        def forward(ctx, x, xdot, fixed_qpos, model, frame, angular):
            B = x.shape[0]
            xc, xd = x.detach().contiguous(), xdot.detach().contiguous()
            fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
            lin = torch.empty((B, model.n_link, 3), dtype=torch.float32, device=x.device)
            ang = torch.empty_like(lin) if angular else None
            if B > 0:
                model.velocities_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), xd.data_ptr(), lin.data_ptr(),
                                     0 if ang is None else ang.data_ptr(), frame=frame,
                                     stream=torch.cuda.current_stream(x.device).cuda_stream)
            ctx.model, ctx.frame = model, frame
            ctx.has_fixed = fixed is not None
            ctx.set_materialize_grads(False)  # an output the loss does not use arrives as None -> NULL for the kernel
            ctx.save_for_backward(*([xc, xd] + ([fixed] if fixed is not None else [])))
            if ang is None:
                return lin
            return lin, ang

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_lin, grad_ang=None):
            want_x, want_xd = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (want_x or want_xd) or (grad_lin is None and grad_ang is None):
                return None, None, None, None, None, None
            saved = list(ctx.saved_tensors)
            x, xd = saved[0], saved[1]
            fixed = saved[2] if ctx.has_fixed else None
            B = x.shape[0]
            gl = None if grad_lin is None else grad_lin.detach().to(torch.float32).contiguous()
            ga = None if grad_ang is None else grad_ang.detach().to(torch.float32).contiguous()
            gx = torch.empty_like(x) if want_x else None  # (the kernel writes every entry)
            gxd = torch.empty_like(x) if want_xd else None
            if B > 0:
                ctx.model.velocities_vjp_dev(B, x.data_ptr(), 0 if fixed is None else fixed.data_ptr(), xd.data_ptr(),
                                             0 if gl is None else gl.data_ptr(), 0 if ga is None else ga.data_ptr(),
                                             0 if gx is None else gx.data_ptr(), 0 if gxd is None else gxd.data_ptr(),
                                             frame=ctx.frame, stream=torch.cuda.current_stream(x.device).cuda_stream)
            return gx, gxd, None, None, None, None

    return _LinkVelocities


_VEL_FN = None


def _link_velocities(model_of, x, xdot, fixed_qpos, link_names, frame, angular):
    """chunks of 64 links -> one table each, results concatenated along the link axis (autograd sums the chunks' gradients)."""
    global _VEL_FN
    import torch

    if _VEL_FN is None:
        _VEL_FN = _make_velocity_function()
    names = list(link_names)
    lin, ang = [], []
    with torch.cuda.device(x.device):
        for c in range(0, len(names), 64):
            out = _VEL_FN.apply(x, xdot, fixed_qpos, model_of(names[c:c + 64]), frame, bool(angular))
            if angular:
                lin.append(out[0])
                ang.append(out[1])
            else:
                lin.append(out)
    if len(lin) == 1:
        return lin[0], (ang[0] if angular else None)
    return torch.cat(lin, dim=1), (torch.cat(ang, dim=1) if angular else None)


def link_velocities(optimizer, q, qdot, link_names, fixed_qpos=None, frame="world", angular=True):
    """`jacobians.link_velocities` with an autograd graph: (lin (B, L, 3), ang (B, L, 3) or None) of `link_names` for the rate
    qdot (B, n_opt) at q (B, n_opt), the same bits, and gradients flow to q and to qdot (not to fixed_qpos; once
    differentiable).  `frame="local"` expresses the velocities -- and hence their cotangents -- in the link's own axes."""
    from . import jacobians

    n_fixed = len(optimizer.idx_pin2fixed)
    f = jacobians._check(optimizer.opt_dof, n_fixed, q, qdot, fixed_qpos, link_names, frame, optimizer.robot.kin)
    return _link_velocities(optimizer.pose_model, q, qdot, fixed_qpos, link_names, f, angular)


def robot_link_velocities(robot, qpos, qvel, link_names, frame="world", angular=True):
    """The same for a full robot qpos and its rate qvel, both (B, robot.dof) float32 in dof order."""
    from . import jacobians

    f = jacobians._check(robot.dof, 0, qpos, qvel, None, link_names, frame, robot.kin, what="qpos")
    return _link_velocities(robot.pose_model, qpos, qvel, None, link_names, f, angular)


# ---- self-collision of a sphere set: distances and the fused penalty, differentiable in q -------------------------------------
def _make_sphere_functions():
    import torch
    from torch.autograd.function import once_differentiable

    class _SphereDistances(torch.autograd.Function):
        """Saves x (and fixed) only: the VJP kernel recomputes the walk and the normals."""

        @staticmethod
        def forward(ctx, x, fixed_qpos, model):
            B = x.shape[0]
            xc = x.detach().contiguous()
            fixed = None if fixed_qpos is None or fixed_qpos.shape[1] == 0 else fixed_qpos.detach().contiguous()
            dist = torch.empty((B, model.n_pair), dtype=torch.float32, device=x.device)
            if B > 0:
                model.distances_dev(B, xc.data_ptr(), 0 if fixed is None else fixed.data_ptr(), dist.data_ptr(), 0,
                                    stream=torch.cuda.current_stream(x.device).cuda_stream)
            ctx.model = model
            ctx.has_fixed = fixed is not None
            ctx.save_for_backward(*([xc] + ([fixed] if fixed is not None else [])))
            return dist

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_dist):
            if not ctx.needs_input_grad[0]:
                return None, None, None
            saved = list(ctx.saved_tensors)
            x = saved[0]
            fixed = saved[1] if ctx.has_fixed else None
            B = x.shape[0]
            gd = grad_dist.detach().to(torch.float32).contiguous()
            gx = torch.empty_like(x)  # (the kernel writes every entry)
            if B > 0:
                ctx.model.distances_vjp_dev(B, x.data_ptr(), 0 if fixed is None else fixed.data_ptr(), gd.data_ptr(), gx.data_ptr(),
                                            stream=torch.cuda.current_stream(x.device).cuda_stream)
            return gx, None, None

    class _SpherePenalty(torch.autograd.Function):
        """The forward launch gives E and dE/dx together where x needs a gradient; backward scales the saved gradient."""

        @staticmethod
        def forward(ctx, x, fixed_qpos, model, margin, pair_weight):
            from . import collision

            want = bool(ctx.needs_input_grad[0])
            e, g = collision._penalty(model, x, fixed_qpos, margin, pair_weight, want_grad=want)
            ctx.save_for_backward(*([g] if want else []))
            return e

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_e):
            if not ctx.needs_input_grad[0] or not ctx.saved_tensors:
                return None, None, None, None, None
            return grad_e.to(torch.float32)[:, None] * ctx.saved_tensors[0], None, None, None, None

    return _SphereDistances, _SpherePenalty


_SPHERE_FNS = None


def _sphere_fns():
    global _SPHERE_FNS
    if _SPHERE_FNS is None:
        _SPHERE_FNS = _make_sphere_functions()
    return _SPHERE_FNS


def sphere_distances(optimizer, q, sphere_set, fixed_qpos=None):
    """`collision.sphere_distances` with an autograd graph: dist (B, P) float32 of the set's sphere pairs at q (B, n_opt), the
    same bits; backward is the distance VJP kernel (dexr_sphere_distances_vjp_dev).  Gradients flow to q only; once
    differentiable."""
    import torch

    from . import collision

    pairs = collision._check(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos,
                             sphere_set, "q")
    with torch.cuda.device(q.device):
        return _sphere_fns()[0].apply(q, fixed_qpos, optimizer.sphere_model(sphere_set, pairs))


def self_collision_penalty(optimizer, q, sphere_set, margin, pair_weight=None, fixed_qpos=None):
    """`collision.self_collision_penalty` with an autograd graph: E (B,) float32 = sum_p w_p max(0, margin - d_p)^2.  Where q
    needs a gradient the forward launch computes E and dE/dq together (one launch, the same bits as the no-graph call) and
    backward is grad_E[:, None] * dE/dq.  Gradients flow to q only (not to pair_weight or fixed_qpos); once differentiable."""
    import torch

    from . import collision

    pairs = collision._check(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos,
                             sphere_set, "q", margin, pair_weight, penalty=True)
    with torch.cuda.device(q.device):
        return _sphere_fns()[1].apply(q, fixed_qpos, optimizer.sphere_model(sphere_set, pairs), float(margin), pair_weight)


def robot_sphere_distances(robot, qpos, sphere_set):
    """The same for a full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    pairs = collision._check(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, "qpos")
    with torch.cuda.device(qpos.device):
        return _sphere_fns()[0].apply(qpos, None, robot.sphere_model(sphere_set, pairs))


def robot_self_collision_penalty(robot, qpos, sphere_set, margin, pair_weight=None):
    """The same for a full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    pairs = collision._check(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, "qpos", margin, pair_weight, penalty=True)
    with torch.cuda.device(qpos.device):
        return _sphere_fns()[1].apply(qpos, None, robot.sphere_model(sphere_set, pairs), float(margin), pair_weight)


# ---- the spheres against an obstacle set: distances and the fused penalty, differentiable in q (and the obstacle's position) ------
def _make_obstacle_functions():
    import torch
    from torch.autograd.function import once_differentiable

    class _ObstacleDistances(torch.autograd.Function):
        """Saves x, fixed and the obstacle pose only: the VJP kernel recomputes the walk, the nearest primitive and its normal."""

        @staticmethod
        def forward(ctx, x, fixed_qpos, obstacle_pos, obstacle_rot, model, obstacles):
            from . import collision

            dist = collision._obstacle_distances(model, obstacles, x, fixed_qpos, obstacle_pos, obstacle_rot, False)
            xc, fixed = collision._inputs(x, fixed_qpos)
            pos, rot = collision._obstacle_pose(obstacle_pos, obstacle_rot)
            ctx.model, ctx.obstacles = model, obstacles
            ctx.have = [a is not None for a in (fixed, pos, rot)]
            ctx.save_for_backward(*[a for a in (xc, fixed, pos, rot) if a is not None])
            return dist

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_dist):
            if not ctx.needs_input_grad[0]:
                return (None,) * 6
            saved = list(ctx.saved_tensors)
            x = saved.pop(0)
            fixed, pos, rot = (saved.pop(0) if h else None for h in ctx.have)
            B = x.shape[0]
            gd = grad_dist.detach().to(torch.float32).contiguous()
            gx = torch.empty_like(x)  # (the kernel writes every entry)
            ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
            if B > 0:
                with torch.cuda.device(x.device):
                    ctx.model.obstacle_distances_vjp_dev(ctx.obstacles.device_set(torch.cuda.current_device()), B, x.data_ptr(), ptr(fixed),
                                                         gd.data_ptr(), gx.data_ptr(), ptr(pos), ptr(rot),
                                                         stream=torch.cuda.current_stream(x.device).cuda_stream)
            return (gx,) + (None,) * 5

    class _ObstaclePenalty(torch.autograd.Function):
        """The forward launch gives E, dE/dx and the wrench together where they are needed; backward scales what it saved."""

        @staticmethod
        def forward(ctx, x, fixed_qpos, obstacle_pos, obstacle_rot, model, obstacles, margin, prim_weight):
            from . import collision

            want_x = bool(ctx.needs_input_grad[0])
            want_p = obstacle_pos is not None and bool(ctx.needs_input_grad[2])
            e, g, wr = collision._obstacle_penalty(model, obstacles, x, fixed_qpos, margin, prim_weight, obstacle_pos, obstacle_rot,
                                                   want_grad=want_x, want_wrench=want_p)
            ctx.want = (want_x, want_p)
            ctx.save_for_backward(*[a for a in (g, wr) if a is not None])
            return e

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_e):
            saved = list(ctx.saved_tensors)
            ge = grad_e.to(torch.float32)[:, None]
            gx = ge * saved.pop(0) if ctx.want[0] else None
            gp = ge * saved.pop(0)[:, :3] if ctx.want[1] else None  # dE/d(obstacle translation): the force half of the wrench
            return (gx, None, gp) + (None,) * 5

    return _ObstacleDistances, _ObstaclePenalty


_OBSTACLE_FNS = None


def _obstacle_fns():
    global _OBSTACLE_FNS
    if _OBSTACLE_FNS is None:
        _OBSTACLE_FNS = _make_obstacle_functions()
    return _OBSTACLE_FNS


def _no_rot_grad(obstacle_rot):
    import torch

    if isinstance(obstacle_rot, torch.Tensor) and obstacle_rot.requires_grad:
        raise ValueError("obstacle_rot requires grad, but no gradient flows to a rotation matrix: detach it and call "
                         "collision.obstacle_penalty with wrench=True, whose last three columns are the torque dE/d(small world rotation)")


def obstacle_distances(optimizer, q, sphere_set, obstacles, obstacle_pos=None, obstacle_rot=None, fixed_qpos=None):
    """`collision.obstacle_distances` with an autograd graph: dist (B, S) float32, the same bits; backward is the distance VJP
    kernel (dexr_obstacle_distances_vjp_dev).  Gradients flow to q only; once differentiable."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos,
                                       sphere_set, obstacles, obstacle_pos, obstacle_rot, "q")
    with torch.cuda.device(q.device):
        return _obstacle_fns()[0].apply(q, fixed_qpos, obstacle_pos, obstacle_rot, optimizer.sphere_model(sphere_set, pairs), obstacles)


def obstacle_penalty(optimizer, q, sphere_set, obstacles, margin, obstacle_pos=None, obstacle_rot=None, prim_weight=None, fixed_qpos=None):
    """`collision.obstacle_penalty` with an autograd graph: E (B,) float32.  Where q or obstacle_pos needs a gradient the forward
    launch computes E, dE/dq and the wrench together (one launch, the same bits as the no-graph call); backward is
    grad_E[:, None] * dE/dq for q and grad_E[:, None] * wrench[:, :3] for obstacle_pos.  No gradient flows to obstacle_rot
    (one that requires grad is a ValueError: `collision.obstacle_penalty(..., wrench=True)` gives the torque), prim_weight or
    fixed_qpos; once differentiable."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos,
                                       sphere_set, obstacles, obstacle_pos, obstacle_rot, "q", margin, prim_weight, penalty=True)
    with torch.cuda.device(q.device):
        return _obstacle_fns()[1].apply(q, fixed_qpos, obstacle_pos, obstacle_rot, optimizer.sphere_model(sphere_set, pairs), obstacles,
                                        float(margin), prim_weight)


def robot_obstacle_distances(robot, qpos, sphere_set, obstacles, obstacle_pos=None, obstacle_rot=None):
    """The same for a full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, obstacles, obstacle_pos, obstacle_rot, "qpos")
    with torch.cuda.device(qpos.device):
        return _obstacle_fns()[0].apply(qpos, None, obstacle_pos, obstacle_rot, robot.sphere_model(sphere_set, pairs), obstacles)


def robot_obstacle_penalty(robot, qpos, sphere_set, obstacles, margin, obstacle_pos=None, obstacle_rot=None, prim_weight=None):
    """The same for a full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, obstacles, obstacle_pos, obstacle_rot, "qpos",
                                       margin, prim_weight, penalty=True)
    with torch.cuda.device(qpos.device):
        return _obstacle_fns()[1].apply(qpos, None, obstacle_pos, obstacle_rot, robot.sphere_model(sphere_set, pairs), obstacles,
                                        float(margin), prim_weight)


# ---- the spheres against a sampled signed-distance field: the obstacle functions with a grid on the other side ---------------------
def _make_grid_functions():
    import torch
    from torch.autograd.function import once_differentiable

    class _GridDistances(torch.autograd.Function):
        """Saves x, fixed and the obstacle pose only: the VJP kernel recomputes the walk, the cell and its gradient."""

        @staticmethod
        def forward(ctx, x, fixed_qpos, obstacle_pos, obstacle_rot, model, grid):
            from . import collision

            dist = collision._grid_distances(model, grid, x, fixed_qpos, obstacle_pos, obstacle_rot)
            xc, fixed = collision._inputs(x, fixed_qpos)
            pos, rot = collision._obstacle_pose(obstacle_pos, obstacle_rot)
            ctx.model, ctx.grid = model, grid
            ctx.have = [a is not None for a in (fixed, pos, rot)]
            ctx.save_for_backward(*[a for a in (xc, fixed, pos, rot) if a is not None])
            return dist

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_dist):
            if not ctx.needs_input_grad[0]:
                return (None,) * 6
            saved = list(ctx.saved_tensors)
            x = saved.pop(0)
            fixed, pos, rot = (saved.pop(0) if h else None for h in ctx.have)
            B = x.shape[0]
            gd = grad_dist.detach().to(torch.float32).contiguous()
            gx = torch.empty_like(x)  # (the kernel writes every entry)
            ptr = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
            if B > 0:
                with torch.cuda.device(x.device):
                    ctx.model.grid_distances_vjp_dev(ctx.grid.device_grid(torch.cuda.current_device()), B, x.data_ptr(), ptr(fixed),
                                                     gd.data_ptr(), gx.data_ptr(), ptr(pos), ptr(rot),
                                                     stream=torch.cuda.current_stream(x.device).cuda_stream)
            return (gx,) + (None,) * 5

    class _GridPenalty(torch.autograd.Function):
        """The forward launch gives E, dE/dx and the wrench together where they are needed; backward scales what it saved."""

        @staticmethod
        def forward(ctx, x, fixed_qpos, obstacle_pos, obstacle_rot, model, grid, margin):
            from . import collision

            want_x = bool(ctx.needs_input_grad[0])
            want_p = obstacle_pos is not None and bool(ctx.needs_input_grad[2])
            e, g, wr = collision._grid_penalty(model, grid, x, fixed_qpos, margin, obstacle_pos, obstacle_rot, want_grad=want_x,
                                               want_wrench=want_p)
            ctx.want = (want_x, want_p)
            ctx.save_for_backward(*[a for a in (g, wr) if a is not None])
            return e

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_e):
            saved = list(ctx.saved_tensors)
            ge = grad_e.to(torch.float32)[:, None]
            gx = ge * saved.pop(0) if ctx.want[0] else None
            gp = ge * saved.pop(0)[:, :3] if ctx.want[1] else None  # dE/d(obstacle translation): the force half of the wrench
            return (gx, None, gp) + (None,) * 4

    return _GridDistances, _GridPenalty


_GRID_FNS = None


def _grid_fns():
    global _GRID_FNS
    if _GRID_FNS is None:
        _GRID_FNS = _make_grid_functions()
    return _GRID_FNS


def grid_distances(optimizer, q, sphere_set, grid, obstacle_pos=None, obstacle_rot=None, fixed_qpos=None):
    """`collision.grid_distances` with an autograd graph: dist (B, S) float32, the same bits; backward is the distance VJP kernel
    (dexr_grid_distances_vjp_dev).  Gradients flow to q only; once differentiable."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos,
                                       sphere_set, grid, obstacle_pos, obstacle_rot, "q", grid=True)
    with torch.cuda.device(q.device):
        return _grid_fns()[0].apply(q, fixed_qpos, obstacle_pos, obstacle_rot, optimizer.sphere_model(sphere_set, pairs), grid)


def grid_penalty(optimizer, q, sphere_set, grid, margin, obstacle_pos=None, obstacle_rot=None, fixed_qpos=None):
    """`collision.grid_penalty` with an autograd graph: E (B,) float32.  Where q or obstacle_pos needs a gradient the forward launch
    computes E, dE/dq and the wrench together (one launch, the same bits as the no-graph call); backward is grad_E[:, None] *
    dE/dq for q and grad_E[:, None] * wrench[:, :3] for obstacle_pos.  No gradient flows to obstacle_rot (one that requires grad
    is a ValueError: `collision.grid_penalty(..., wrench=True)` gives the torque), to fixed_qpos or to the samples; once
    differentiable."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(optimizer.opt_dof, len(optimizer.idx_pin2fixed), optimizer.robot.kin, optimizer.robot, q, fixed_qpos,
                                       sphere_set, grid, obstacle_pos, obstacle_rot, "q", margin, penalty=True, grid=True)
    with torch.cuda.device(q.device):
        return _grid_fns()[1].apply(q, fixed_qpos, obstacle_pos, obstacle_rot, optimizer.sphere_model(sphere_set, pairs), grid, float(margin))


def robot_grid_distances(robot, qpos, sphere_set, grid, obstacle_pos=None, obstacle_rot=None):
    """The same for a full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, grid, obstacle_pos, obstacle_rot, "qpos", grid=True)
    with torch.cuda.device(qpos.device):
        return _grid_fns()[0].apply(qpos, None, obstacle_pos, obstacle_rot, robot.sphere_model(sphere_set, pairs), grid)


def robot_grid_penalty(robot, qpos, sphere_set, grid, margin, obstacle_pos=None, obstacle_rot=None):
    """The same for a full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    _no_rot_grad(obstacle_rot)
    pairs = collision._check_obstacles(robot.dof, 0, robot.kin, robot, qpos, None, sphere_set, grid, obstacle_pos, obstacle_rot, "qpos",
                                       margin, penalty=True, grid=True)
    with torch.cuda.device(qpos.device):
        return _grid_fns()[1].apply(qpos, None, obstacle_pos, obstacle_rot, robot.sphere_model(sphere_set, pairs), grid, float(margin))


# ---- the spheres of one posed robot against another's: differentiable in both q and both base positions ---------------------------
def _make_cross_functions():
    import torch
    from torch.autograd.function import once_differentiable

    class _CrossDistances(torch.autograd.Function):
        """Saves the inputs only: the VJP kernel recomputes both walks, the nearest spheres and their normals."""

        @staticmethod
        def forward(ctx, x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b, model_a, model_b):
            from . import collision

            da, db = collision._cross_distances(model_a, model_b, x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b, False)
            inputs = collision._cross_inputs(x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b)
            ctx.models = (model_a, model_b)
            ctx.have = [a is not None for a in inputs]
            ctx.save_for_backward(*[a for a in inputs if a is not None])
            return da, db

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_a, grad_b):
            from . import collision

            need = ctx.needs_input_grad
            if not (need[0] or need[2] or need[4] or need[6]):
                return (None,) * 10
            saved = list(ctx.saved_tensors)
            inputs = tuple(saved.pop(0) if h else None for h in ctx.have)
            c = lambda g: None if g is None else g.detach().to(torch.float32).contiguous()  # noqa: E731
            want_p = (bool(need[4]) and inputs[4] is not None, bool(need[6]) and inputs[6] is not None)
            ga, gb, wa, wb = collision._cross_distances_vjp(*ctx.models, inputs, c(grad_a), c(grad_b), want_wrench=want_p)
            return (ga if need[0] else None, None, gb if need[2] else None, None, wa[:, :3] if want_p[0] else None, None,
                    wb[:, :3] if want_p[1] else None, None, None, None)

    class _CrossPenalty(torch.autograd.Function):
        """The forward launch gives E and whichever of dE/dx_a, dE/dx_b and the two wrenches an input needs; backward scales what
        it saved."""

        @staticmethod
        def forward(ctx, x_a, fixed_a, x_b, fixed_b, pos_a, rot_a, pos_b, rot_b, model_a, model_b, margin, pair_weight):
            from . import collision

            need = ctx.needs_input_grad
            want = (True, bool(need[0]), bool(need[2]), pos_a is not None and bool(need[4]), pos_b is not None and bool(need[6]))
            out = collision._cross_penalty(model_a, model_b, x_a, fixed_a, x_b, fixed_b, margin, pair_weight, pos_a, rot_a, pos_b, rot_b,
                                           want=want)
            ctx.want = want
            ctx.save_for_backward(*[a for a in out[1:] if a is not None])
            return out[0]

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_e):
            saved = list(ctx.saved_tensors)
            ge = grad_e.to(torch.float32)[:, None]
            ga, gb, wa, wb = (saved.pop(0) if k else None for k in ctx.want[1:])
            s = lambda t: None if t is None else ge * t  # noqa: E731
            # dE/d(base translation): the force half of that base's wrench
            return (s(ga), None, s(gb), None, None if wa is None else ge * wa[:, :3], None, None if wb is None else ge * wb[:, :3], None) + \
                (None,) * 4

    return _CrossDistances, _CrossPenalty


_CROSS_FNS = None


def _cross_fns():
    global _CROSS_FNS
    if _CROSS_FNS is None:
        _CROSS_FNS = _make_cross_functions()
    return _CROSS_FNS


def cross_distances(optimizer_a, q_a, spheres_a, optimizer_b, q_b, spheres_b, pos_a=None, rot_a=None, pos_b=None, rot_b=None,
                    fixed_qpos_a=None, fixed_qpos_b=None):
    """`collision.cross_distances` with an autograd graph: (dist_a (B, S_a), dist_b (B, S_b)) float32, the same bits; backward is
    the distance VJP kernel (dexr_cross_distances_vjp_dev), one launch for both cotangents.  Gradients flow to q_a, q_b and -- the
    force halves of the VJP's wrenches -- to pos_a, pos_b; a rotation that requires grad is a ValueError; once differentiable."""
    import torch

    from . import collision

    _no_rot_grad(rot_a)
    _no_rot_grad(rot_b)
    ma, mb = collision._check_cross(collision._optimizer_side(optimizer_a, q_a, spheres_a, fixed_qpos_a, "a"),
                                    collision._optimizer_side(optimizer_b, q_b, spheres_b, fixed_qpos_b, "b"), pos_a, rot_a, pos_b, rot_b)
    with torch.cuda.device(q_a.device):
        return _cross_fns()[0].apply(q_a, fixed_qpos_a, q_b, fixed_qpos_b, pos_a, rot_a, pos_b, rot_b, ma, mb)


def cross_penalty(optimizer_a, q_a, spheres_a, optimizer_b, q_b, spheres_b, margin, pos_a=None, rot_a=None, pos_b=None, rot_b=None,
                  pair_weight=None, fixed_qpos_a=None, fixed_qpos_b=None):
    """`collision.cross_penalty` with an autograd graph: E (B,) float32.  The forward launch computes E and only what some input
    needs of dE/dq_a, dE/dq_b and the two wrenches (one launch, the same bits as the no-graph call); backward is grad_E[:, None] *
    dE/dq for q_a and q_b and grad_E[:, None] * wrench[:, :3] for pos_a and pos_b.  No gradient flows to a rotation (one that
    requires grad is a ValueError: `collision.cross_penalty(..., wrench=True)` gives the torques), pair_weight or fixed_qpos; once
    differentiable."""
    import torch

    from . import collision

    _no_rot_grad(rot_a)
    _no_rot_grad(rot_b)
    ma, mb = collision._check_cross(collision._optimizer_side(optimizer_a, q_a, spheres_a, fixed_qpos_a, "a"),
                                    collision._optimizer_side(optimizer_b, q_b, spheres_b, fixed_qpos_b, "b"), pos_a, rot_a, pos_b, rot_b,
                                    margin, pair_weight, penalty=True)
    with torch.cuda.device(q_a.device):
        return _cross_fns()[1].apply(q_a, fixed_qpos_a, q_b, fixed_qpos_b, pos_a, rot_a, pos_b, rot_b, ma, mb, float(margin), pair_weight)


def robot_cross_distances(robot_a, qpos_a, spheres_a, robot_b, qpos_b, spheres_b, pos_a=None, rot_a=None, pos_b=None, rot_b=None):
    """The same for full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    _no_rot_grad(rot_a)
    _no_rot_grad(rot_b)
    ma, mb = collision._check_cross(collision._robot_side(robot_a, qpos_a, spheres_a, "a"), collision._robot_side(robot_b, qpos_b, spheres_b, "b"),
                                    pos_a, rot_a, pos_b, rot_b)
    with torch.cuda.device(qpos_a.device):
        return _cross_fns()[0].apply(qpos_a, None, qpos_b, None, pos_a, rot_a, pos_b, rot_b, ma, mb)


def robot_cross_penalty(robot_a, qpos_a, spheres_a, robot_b, qpos_b, spheres_b, margin, pos_a=None, rot_a=None, pos_b=None, rot_b=None,
                        pair_weight=None):
    """The same for full robot qpos (B, robot.dof) float32 in dof order."""
    import torch

    from . import collision

    _no_rot_grad(rot_a)
    _no_rot_grad(rot_b)
    ma, mb = collision._check_cross(collision._robot_side(robot_a, qpos_a, spheres_a, "a"), collision._robot_side(robot_b, qpos_b, spheres_b, "b"),
                                    pos_a, rot_a, pos_b, rot_b, margin, pair_weight, penalty=True)
    with torch.cuda.device(qpos_a.device):
        return _cross_fns()[1].apply(qpos_a, None, qpos_b, None, pos_a, rot_a, pos_b, rot_b, ma, mb, float(margin), pair_weight)


__all__ = ["retarget", "ref_value_from_keypoints", "link_poses", "robot_link_poses", "link_velocities", "robot_link_velocities",
           "sphere_distances", "self_collision_penalty", "robot_sphere_distances", "robot_self_collision_penalty", "obstacle_distances",
           "obstacle_penalty", "robot_obstacle_distances", "robot_obstacle_penalty", "grid_distances", "grid_penalty", "robot_grid_distances",
           "robot_grid_penalty", "cross_distances", "cross_penalty", "robot_cross_distances", "robot_cross_penalty"]

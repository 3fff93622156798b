"""numpy restatement of the closed-form VJP of the link velocities (include/dexr_wrench.h), the yardstick of
tests/test_wrench_host.py and tests/test_gpu_wrench.py.  It shares no code with csrc/dexr_pose.hip: link by link it walks the
link's own joint chain (the walk of OracleRobot._walk, restated so that every operation runs in the asked `dtype`), keeps the
world axis a_k and origin o_k of every joint and the twist (V_k, W_k) of the joint's body at o_k after the joint's own
advance, and adds the link's share to every joint of the chain:

    world frame:  f = gv_l      m = gw_l      A = v_l x f + w_l x m
    local frame:  f = R_l gv_l  m = R_l gw_l  A = 0
    dL/dqd_k += a_k . (p_l x f + m - o_k x f)                                       revolute      a_k . f             prismatic
    dL/dq_k  += a_k . (A - V_k x f - W_k x m) + (W_k x a_k) . (p_l x f - o_k x f)   revolute      (W_k x a_k) . f     prismatic

No subtree sums, no slots, no source map: the result is in the full joint order of the robot (fold it with the chain rule
of the source map where a table has one)."""
import numpy as np

WORLD, LOCAL = 0, 1


def _dot(a, b):
    return (a * b).sum(-1)


def _rodrigues(axis, th, dtype):
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype)
    one = np.eye(3, dtype=dtype)
    return one[None] + np.sin(th)[:, None, None] * K[None] + (1 - np.cos(th))[:, None, None] * (K @ K)[None]


def _chain_walk(orc, q, qd, link, dtype):
    """-> R_l, p_l, v_l, w_l and per movable joint of the chain (dof index, type, a, o, V, W), everything in `dtype`."""
    B = q.shape[0]
    R = np.broadcast_to(np.eye(3, dtype=dtype), (B, 3, 3)).copy()
    p, v, w = (np.zeros((B, 3), dtype) for _ in range(3))  # v: velocity of the running body at the point p
    info = []
    for j in orc._chain(link):
        d = np.einsum("bij,j->bi", R, j.p0.astype(dtype))
        p, v = p + d, v + np.cross(w, d)
        R = R @ j.R0.astype(dtype)
        if j.type == "fixed":
            continue
        qi = orc.qidx[j.name]
        a = np.einsum("bij,j->bi", R, j.axis.astype(dtype))
        if j.type == "revolute":
            R = R @ _rodrigues(j.axis.astype(dtype), q[:, qi], dtype)
            w = w + qd[:, qi:qi + 1] * a
        else:
            d = a * q[:, qi:qi + 1]
            p, v = p + d, v + np.cross(w, d) + qd[:, qi:qi + 1] * a
        info.append((qi, j.type, a, p.copy(), v.copy(), w.copy()))
    return R, p, v, w, info


def link_velocities(orc, q, qd, links, frame=WORLD, dtype=np.float64):
    """(lin, ang) (B, L, 3) of the walk above: what the VJP below differentiates."""
    q, qd = np.atleast_2d(np.asarray(q, dtype)), np.atleast_2d(np.asarray(qd, dtype))
    lin, ang = [], []
    for name in links:
        R, _, v, w, _ = _chain_walk(orc, q, qd, name, dtype)
        if frame == LOCAL:
            v, w = np.einsum("bji,bj->bi", R, v), np.einsum("bji,bj->bi", R, w)
        lin.append(v)
        ang.append(w)
    return np.stack(lin, 1), np.stack(ang, 1)


def velocity_vjp(orc, q, qd, links, grad_lin=None, grad_ang=None, frame=WORLD, dtype=np.float64):
    """q, qd (B, dof); grad_lin, grad_ang (B, L, 3) or None -> (grad_q, grad_qd) (B, dof) in the full joint order."""
    q, qd = np.atleast_2d(np.asarray(q, dtype)), np.atleast_2d(np.asarray(qd, dtype))
    gq, gqd = np.zeros_like(q), np.zeros_like(q)
    zero = np.zeros((q.shape[0], 3), dtype)
    for li, name in enumerate(links):
        R, p, v, w, info = _chain_walk(orc, q, qd, name, dtype)
        f = zero if grad_lin is None else np.asarray(grad_lin, dtype)[:, li]
        m = zero if grad_ang is None else np.asarray(grad_ang, dtype)[:, li]
        if frame == LOCAL:
            f, m, A = np.einsum("bij,bj->bi", R, f), np.einsum("bij,bj->bi", R, m), zero
        else:
            A = np.cross(v, f) + np.cross(w, m)
        c = np.cross(p, f)
        for qi, typ, a, o, V, W in info:
            if typ == "revolute":
                arm = c - np.cross(o, f)
                gqd[:, qi] += _dot(a, arm + m)
                gq[:, qi] += _dot(a, A - np.cross(V, f) - np.cross(W, m)) + _dot(np.cross(W, a), arm)
            else:
                gqd[:, qi] += _dot(a, f)
                gq[:, qi] += _dot(np.cross(W, a), f)
    return gq, gqd


def wrenches(orc, q, links, force=None, torque=None, frame=WORLD, dtype=np.float64):
    """tau (B, dof) = sum_l Jlin_l^T force_l + Jang_l^T torque_l: the rate half of the VJP (it does not read qd)."""
    q = np.atleast_2d(np.asarray(q, dtype))
    return velocity_vjp(orc, q, np.zeros_like(q), links, force, torque, frame, dtype)[1]

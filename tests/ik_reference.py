"""numpy restatement of the damped least-squares IK step (include/dexr_ik.h), the yardstick of tests/test_ik_host.py and
tests/test_gpu_ik.py.  It shares no code with csrc/dexr_pose.hip: link by link it walks the link's own joint chain
(velocity_vjp_reference._chain_walk: a_k, o_k per joint of the chain, p_l, R_l of the link, every operation in the asked
`dtype`), writes the link's Jacobian columns

    Jlin[:, l, :, k] = a_k x (p_l - o_k)   revolute   |   a_k   prismatic          Jang[:, l, :, k] = a_k   |   0

(local frame: both multiplied by R_l^T on the left), forms the normal equations densely over ALL columns,

    H = sum_l w_lin Jlin_l^T Jlin_l + w_ang Jang_l^T Jang_l + damping I        g = sum_l w_lin Jlin_l^T e_lin_l + w_ang Jang_l^T e_ang_l,

and hands them to np.linalg.solve (LAPACK's pivoted LU).  No subtree ranges, no active columns, no Cholesky, no source map:
the result is in the full joint order of the robot unless `fold` is given, which maps the last axis of J (the chain rule of a
source map, e.g. pose_zoo.fold) BEFORE H is formed -- H is quadratic in J, so folding dx instead would be wrong."""
import numpy as np

import velocity_vjp_reference as vref

WORLD, LOCAL = vref.WORLD, vref.LOCAL


def jacobians(orc, q, links, frame=WORLD, dtype=np.float64):
    """(jlin, jang) (B, L, 3, dof) in `dtype`, in the asked frame."""
    q = np.atleast_2d(np.asarray(q, dtype))
    B = q.shape[0]
    zero = np.zeros_like(q)
    jl = np.zeros((B, len(links), 3, q.shape[1]), dtype)
    ja = np.zeros_like(jl)
    for li, name in enumerate(links):
        R, p, _, _, info = vref._chain_walk(orc, q, zero, name, dtype)
        for qi, typ, a, o, _, _ in info:
            if typ == "revolute":
                lin, ang = np.cross(a, p - o), a
            else:
                lin, ang = a, np.zeros_like(a)
            if frame == LOCAL:
                lin, ang = np.einsum("bji,bj->bi", R, lin), np.einsum("bji,bj->bi", R, ang)
            jl[:, li, :, qi] += lin
            ja[:, li, :, qi] += ang
    assert jl.dtype == dtype and ja.dtype == dtype
    return jl, ja


def normal_equations(orc, q, links, err_lin=None, err_ang=None, w_lin=None, w_ang=None, frame=WORLD, dtype=np.float64, fold=None,
                     jac=None):
    """(H without the damping (B, n, n), g (B, n)) in `dtype`; n = dof, or the width `fold` gives.  `jac`: what
    jacobians(orc, q, links, frame, dtype) returned, where a caller solves several error / weight forms at one q."""
    if err_lin is None and err_ang is None:
        raise ValueError("err_lin and err_ang are both None")
    jl, ja = jacobians(orc, q, links, frame, dtype) if jac is None else jac
    if fold is not None:
        jl, ja = np.asarray(fold(jl), dtype), np.asarray(fold(ja), dtype)
    B, L, _, n = jl.shape
    H, g = np.zeros((B, n, n), dtype), np.zeros((B, n), dtype)
    for J, e, w in ((jl, err_lin, w_lin), (ja, err_ang, w_ang)):
        if e is None:
            continue
        e = np.asarray(e, dtype)
        w = np.ones((B, L), dtype) if w is None else np.asarray(w, dtype)
        A = J.reshape(B, 3 * L, n)  # rows (l, r); batched matrix products instead of einsum: BLAS, in `dtype`
        wA = A * np.repeat(w, 3, axis=1)[:, :, None]
        H = H + np.matmul(A.transpose(0, 2, 1), wA)
        g = g + np.matmul(wA.transpose(0, 2, 1), e.reshape(B, 3 * L, 1))[..., 0]
    assert H.dtype == dtype and g.dtype == dtype
    return H, g


def ik_step(orc, q, links, err_lin=None, err_ang=None, w_lin=None, w_ang=None, damping=None, frame=WORLD, dtype=np.float64, fold=None,
            jac=None):
    """dx (B, n) in `dtype`."""
    H, g = normal_equations(orc, q, links, err_lin, err_ang, w_lin, w_ang, frame, dtype, fold, jac)
    H = H + dtype(damping) * np.eye(H.shape[-1], dtype=dtype)
    dx = np.linalg.solve(H, g[..., None])[..., 0]
    assert dx.dtype == dtype
    return dx


def link_positions(orc, q, links, dtype=np.float64):
    """(B, L, 3) world positions of the link origins from the same walk."""
    q = np.atleast_2d(np.asarray(q, dtype))
    zero = np.zeros_like(q)
    return np.stack([vref._chain_walk(orc, q, zero, name, dtype)[1] for name in links], 1)


def tracking_loop(orc, q0, q_star, links, damping, steps=8):
    """`steps` position-only steps x += dx with e = p(q*) - p(x) -> (iterates (steps + 1, B, dof), error norms (steps + 1, B))."""
    target = link_positions(orc, q_star, links)
    x = np.array(q0, np.float64)
    xs, errs = [x.copy()], []
    for _ in range(steps):
        e = target - link_positions(orc, x, links)
        errs.append(np.linalg.norm(e.reshape(len(x), -1), axis=1))
        x = x + ik_step(orc, x, links, err_lin=e, damping=damping)
        xs.append(x.copy())
    errs.append(np.linalg.norm((target - link_positions(orc, x, links)).reshape(len(x), -1), axis=1))
    return np.stack(xs), np.stack(errs)

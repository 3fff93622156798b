"""numpy restatement of the IK solve to link pose targets (include/dexr_ik_solve.h), the yardstick of
tests/test_ik_solve_host.py and tests/test_gpu_ik_solve.py.  It shares no code with csrc/dexr_pose.hip: the poses of an iterate
come link by link from the link's own joint chain (velocity_vjp_reference._chain_walk), H and g from
ik_reference.normal_equations (dense, over ALL columns), a frozen column is masked out of them (row and column of the
identity, g_i = 0) and np.linalg.solve (LAPACK's pivoted LU) gives the step.  No subtree ranges, no active columns, no
Cholesky, no loop-in-a-kernel: a plain Python loop over the iterations with a per-frame `stopped` mask.

A table with a source map (optimizer order, tests/pose_zoo.py) iterates in ITS variables: `full` maps them to the oracle's joint
vector, `fold` is the chain rule of that map on the last axis of a Jacobian (as in ik_reference)."""
import numpy as np

import ik_reference as ikr
import velocity_vjp_reference as vref


def link_poses(orc, q, links, dtype=np.float64):
    """(p (B, L, 3), R (B, L, 3, 3)) world poses of the links, every operation in `dtype`."""
    q = np.atleast_2d(np.asarray(q, dtype))
    zero = np.zeros_like(q)
    walks = [vref._chain_walk(orc, q, zero, name, dtype) for name in links]
    return np.stack([w[1] for w in walks], 1), np.stack([w[0] for w in walks], 1)


def rotation_error(target, R, dtype=np.float64):
    """(B, L, 3): the rotation vector of M = target R^T in world axes; v = 1/2 vee(M - M^T), c = (tr M - 1) / 2, s = |v|,
    v * (atan2(s, c) / s where s > 1e-6, else 1)."""
    M = np.matmul(np.asarray(target, dtype), np.swapaxes(R, -1, -2))
    v = dtype(0.5) * np.stack([M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]], -1)
    c = dtype(0.5) * (M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2] - dtype(1))
    s = np.sqrt((v * v).sum(-1))
    big = s > dtype(1e-6)
    k = np.where(big, np.arctan2(s, c) / np.where(big, s, dtype(1)), dtype(1)).astype(dtype)
    return v * k[..., None]


def active_columns(orc, q, links, fold=None, dtype=np.float64):
    """bool (n,): the columns some joint above a link reads (a revolute joint's angular column and a prismatic joint's linear
    column are unit vectors, never 0)."""
    jl, ja = ikr.jacobians(orc, q, links, ikr.WORLD, dtype)
    if fold is not None:
        jl, ja = fold(jl), fold(ja)
    return (np.abs(jl) + np.abs(ja)).max((0, 1, 2)) > 0


def ik_solve(orc, x0, links, tgt_pos=None, tgt_rot=None, w_lin=None, w_ang=None, lo=None, hi=None, damping=None, max_iters=None,
             tol=0.0, max_step=0.0, dtype=np.float64, full=None, fold=None):
    """-> (xs (max_iters + 1, B, n) the iterates, frozen (max_iters, B, n) bool the freeze decisions of each step, iters (B),
    errs (max_iters + 1, B) sqrt(E_k)).  A frame that has stopped repeats its last iterate and error and freezes nothing; its
    answer is xs[-1], errs[-1], iters."""
    if tgt_pos is None and tgt_rot is None:
        raise ValueError("tgt_pos and tgt_rot are both None")
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi go together")
    c = (lambda a: None if a is None else np.asarray(a, dtype))
    tgt_pos, tgt_rot, w_lin, w_ang, lo, hi = (c(a) for a in (tgt_pos, tgt_rot, w_lin, w_ang, lo, hi))
    full = (lambda x: x) if full is None else full
    x = np.array(np.atleast_2d(x0), dtype)
    B, n = x.shape
    L = len(links)
    one = np.ones((B, L), dtype)
    wl, wa = (one if w_lin is None else w_lin), (one if w_ang is None else w_ang)
    active = active_columns(orc, np.asarray(full(x), dtype), links, fold, dtype)
    stopped = np.zeros(B, bool)
    iters = np.zeros(B, np.int32)
    xs, frozen, errs = [], [], []
    eye = np.eye(n, dtype=dtype)
    for k in range(max_iters + 1):
        q = np.asarray(full(x), dtype)
        p, R = link_poses(orc, q, links, dtype)
        e_lin = None if tgt_pos is None else tgt_pos - p
        e_ang = None if tgt_rot is None else rotation_error(tgt_rot, R, dtype)
        E = np.zeros(B, dtype)
        if e_lin is not None:
            E = E + (wl * (e_lin * e_lin).sum(-1)).sum(-1)
        if e_ang is not None:
            E = E + (wa * (e_ang * e_ang).sum(-1)).sum(-1)
        err = np.sqrt(E)
        if k > 0:
            err = np.where(stopped, errs[-1], err)
        stop_now = ~stopped & ((E <= dtype(tol) * dtype(tol)) | (k == max_iters))
        iters[stop_now] = k
        stopped = stopped | stop_now
        xs.append(x.copy())
        errs.append(err.astype(dtype))
        if k == max_iters:
            break
        H, g = ikr.normal_equations(orc, q, links, e_lin, e_ang, w_lin if e_lin is not None else None, w_ang if e_ang is not None else None,
                                    ikr.WORLD, dtype, fold)
        H = H + dtype(damping) * eye
        F = np.zeros((B, n), bool)
        if lo is not None:
            F = ((x <= lo) & (g < 0)) | ((x >= hi) & (g > 0))
        F = F & ~stopped[:, None]
        g = np.where(F, dtype(0), g)
        H = np.where(F[:, :, None] | F[:, None, :], eye[None], H)
        dx = np.linalg.solve(H, g[..., None])[..., 0].astype(dtype)
        if max_step > 0:
            m = np.abs(dx).max(-1)
            dx = dx * np.where(m > dtype(max_step), dtype(max_step) / np.where(m > 0, m, dtype(1)), dtype(1)).astype(dtype)[:, None]
        v = x + dx
        if lo is not None:
            v = np.where(active[None], np.where(v < lo, lo, np.where(v > hi, hi, v)), v)
        x = np.where(stopped[:, None], x, v).astype(dtype)
        frozen.append(F)
    xs, errs = np.stack(xs), np.stack(errs)
    assert xs.dtype == dtype and errs.dtype == dtype
    return xs, np.stack(frozen), iters, errs

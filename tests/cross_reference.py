"""numpy restatement of the collision between two posed robots (include/dexr_cross.h), the yardstick of tests/test_cross_host.py
and tests/test_gpu_cross.py.  It shares no code with csrc/dexr_cross.hpp: per robot the sphere centres come from
collision_reference.centres and the point Jacobians

    Jpt_s[:, c] = Jlin_l[:, c] + Jang_l[:, c] x (c_s - p_l)

from ik_reference.jacobians, exactly as obstacle_reference.fields builds them; the base poses are applied densely
(C = pos + rot c, rot Jpt); d, n and h are dense over ALL (frame, sphere of A, sphere of B) entries -- no loop over spheres, no
nearest-only shortcut, no pair seen from two ends -- and every gradient goes through the dense Jacobians, with `fold` per side.
Every operation is in the asked `dtype`.

A robot is a `side`: dict(orc, q, links, rows, centers, radii, pos, rot, fold) with pos (B, 3) / rot (B, 3, 3) or None."""
import numpy as np

import collision_reference as cref
import ik_reference as ikr


def side(orc, q, links, rows, centers, radii, pos=None, rot=None, dtype=np.float64, fold=None, jacobian=True):
    """-> dict: C (B, S, 3) world centres, arm (B, S, 3) = C - pos, r (S,), jpt (B, S, 3, ncol) = rot Jpt (None without `jacobian`)."""
    q = np.asarray(q, dtype)
    c, pl = cref.centres(orc, q, links, rows, centers, dtype)
    B = c.shape[0]
    p = np.zeros((B, 3), dtype) if pos is None else np.asarray(pos, dtype)
    R = np.broadcast_to(np.eye(3, dtype=dtype), (B, 3, 3)) if rot is None else np.asarray(rot, dtype)
    arm = np.einsum("bij,bsj->bsi", R, c)
    jpt = None
    if jacobian:
        jl, ja = ikr.jacobians(orc, q, links, ikr.WORLD, dtype)
        r = np.asarray(rows)
        jpt = jl[:, r] + np.cross(ja[:, r], (c - pl)[..., None], axisa=2, axisb=2, axisc=2)
        if fold is not None:
            jpt = np.asarray(fold(jpt), dtype)
        jpt = np.einsum("bij,bsjc->bsic", R, jpt)
    out = dict(C=(arm + p[:, None]).astype(dtype), arm=arm.astype(dtype), r=np.asarray(radii, dtype), jpt=jpt)
    assert all(v is None or v.dtype == dtype for v in out.values())
    return out


def fields(A, Bs):
    """-> dict: s (B, S_a, S_b) centre distances, d (B, S_a, S_b) = s - (r_s + r_t), n (B, S_a, S_b, 3), zero where s == 0."""
    dtype = A["C"].dtype.type
    D = A["C"][:, :, None] - Bs["C"][:, None]
    s = np.sqrt((D * D).sum(-1))
    n = np.where(s[..., None] > 0, D / np.where(s > 0, s, dtype(1))[..., None], dtype(0)).astype(dtype)
    d = s - (A["r"][None, :, None] + Bs["r"][None, None])
    assert d.dtype == dtype and n.dtype == dtype
    return dict(s=s, d=d, n=n)


def distances(F):
    """-> (dist_a (B, S_a), nearest_a, dist_b (B, S_b), nearest_b): argmin is the first that attains the minimum."""
    d = F["d"]
    return d.min(2), d.argmin(2).astype(np.int32), d.min(1), d.argmin(1).astype(np.int32)


def _wrench(side_, f):
    return np.concatenate([f.sum(1), np.cross(side_["arm"], f).sum(1)], -1)


def _outputs(A, Bs, fa, fb):
    ga = None if A["jpt"] is None else np.einsum("bsr,bsrc->bc", fa, A["jpt"])
    gb = None if Bs["jpt"] is None else np.einsum("btr,btrc->bc", fb, Bs["jpt"])
    return ga, gb, _wrench(A, fa), _wrench(Bs, fb)


def distances_vjp(F, A, Bs, grad_a=None, grad_b=None):
    """-> (grad_xa, grad_xb, wrench_a, wrench_b) of sum grad_a dist_a + sum grad_b dist_b: a dense one-hot selection of the nearest
    entries, contracted with the normals."""
    d, n = F["d"], F["n"]
    dtype = d.dtype.type
    Sa, Sb = d.shape[1:]
    ga = np.zeros(d.shape[:2], dtype) if grad_a is None else np.asarray(grad_a, dtype)
    gb = np.zeros((d.shape[0], Sb), dtype) if grad_b is None else np.asarray(grad_b, dtype)
    pick_a = (np.arange(Sb)[None, None] == d.argmin(2)[:, :, None]).astype(dtype)  # (B, S_a, S_b): t is the nearest of s
    pick_b = (np.arange(Sa)[None, :, None] == d.argmin(1)[:, None]).astype(dtype)  # (B, S_a, S_b): s is the nearest of t
    k = ga[:, :, None] * pick_a + gb[:, None] * pick_b  # dL/dd_st
    fa = (k[..., None] * n).sum(2)
    fb = -(k[..., None] * n).sum(1)
    return _outputs(A, Bs, fa.astype(dtype), fb.astype(dtype))


def penalty(F, A, Bs, margin, pair_weight=None):
    """-> (E (B,), grad_xa, grad_xb, wrench_a (B, 6), wrench_b (B, 6), h (B, S_a, S_b))."""
    d, n = F["d"], F["n"]
    dtype = d.dtype.type
    w = np.ones(d.shape[1:], dtype) if pair_weight is None else np.asarray(pair_weight, dtype)
    h = np.maximum(dtype(0), dtype(margin) - d)
    E = (w * h * h).sum((1, 2))
    k = (dtype(-2) * w * h)[..., None] * n  # dE/dC^A_s of the pair
    fa, fb = k.sum(2), -k.sum(1)
    out = (E,) + _outputs(A, Bs, fa, fb) + (h,)
    assert all(v is None or v.dtype == dtype for v in out)
    return out

"""numpy restatement of the obstacle collision (include/dexr_obstacles.h), the yardstick of tests/test_obstacle_host.py and
tests/test_gpu_obstacles.py.  It shares no code with csrc/dexr_obstacles.hpp: the sphere centres come from
collision_reference.centres (link by link from the link's own joint chain), the signed distances and their analytic gradients are
dense over ALL (sphere, primitive) entries -- one vectorised expression per kind, no loop over spheres, no nearest-only shortcut
-- and the gradient in x goes through the dense point Jacobian

    Jpt_s[:, c] = Jlin_l[:, c] + Jang_l[:, c] x (c_s - p_l)

built from ik_reference.jacobians exactly as collision_reference.distance_jacobian builds it.  No subtree ranges, no forces
parked anywhere.  Every operation is in the asked `dtype`.

`kinds` (M,) and `params` (M, 16) are the primitives as dexr_obstacle_set_create takes them; `opos` (B, 3) / `orot` (B, 3, 3)
the obstacle pose per frame or None.  `links`, `rows`, `centers`, `radii`, `q`, `fold` as in collision_reference."""
import numpy as np

import collision_reference as cref
import ik_reference as ikr

SPHERE, CAPSULE, BOX, HALFSPACE = 0, 1, 2, 3


def _unit(D, dtype):
    s = np.sqrt((D * D).sum(-1))
    g = np.where(s[..., None] > 0, D / np.where(s > 0, s, dtype(1))[..., None], dtype(0)).astype(dtype)
    return s, g


def sdf(kinds, params, y, dtype=np.float64):
    """y (..., 3) points of the obstacle frame -> (sdf (..., M), grad (..., M, 3)), grad zero where there is no direction."""
    y = np.asarray(y, dtype)
    out_d, out_g = [], []
    for kind, v in zip(np.asarray(kinds), np.asarray(params, np.float64)):
        v = v.astype(dtype)
        if kind == SPHERE:
            s, g = _unit(y - v[:3], dtype)
            d = s - v[3]
        elif kind == CAPSULE:
            a, ab = v[:3], v[3:6] - v[:3]
            l2 = (ab * ab).sum()
            t = np.clip(((y - a) * ab).sum(-1) / l2, dtype(0), dtype(1)) if l2 > 0 else np.zeros(y.shape[:-1], dtype)
            s, g = _unit(y - (a + t[..., None] * ab), dtype)
            d = s - v[6]
        elif kind == BOX:
            c, h, R = v[:3], v[3:6], v[6:15].reshape(3, 3)
            u = (y - c) @ R  # R^T (y - c)
            sign = np.where(u < 0, dtype(-1), dtype(1))
            qq = np.abs(u) - h
            mx, ax = qq.max(-1), qq.argmax(-1)  # argmax: the first largest
            inside = mx <= 0
            m = np.maximum(qq, dtype(0))
            ln = np.sqrt((m * m).sum(-1))
            g_out = sign * m / np.where(ln > 0, ln, dtype(1))[..., None]
            g_in = sign * (np.arange(3) == ax[..., None])
            gu = np.where(inside[..., None], g_in, g_out).astype(dtype)
            d = np.where(inside, mx, ln)
            g = gu @ R.T
        elif kind == HALFSPACE:
            d = (y * v[:3]).sum(-1) - v[3]
            g = np.broadcast_to(v[:3], y.shape)
        else:
            raise ValueError(f"unknown kind {kind}")
        out_d.append(d.astype(dtype))
        out_g.append(np.asarray(g, dtype))
    return np.stack(out_d, -1), np.stack(out_g, -2)


def fields(orc, q, links, rows, centers, radii, kinds, params, opos=None, orot=None, dtype=np.float64, fold=None, jacobian=True):
    """-> dict: c (B, S, 3) world centres, arm (B, S, 3) = c - p_o, d (B, S, M) = sdf_m(y_s) - r_s, n (B, S, M, 3) world normals,
    jpt (B, S, 3, ncol) the point Jacobians (None without `jacobian`)."""
    q = np.asarray(q, dtype)
    c, pl = cref.centres(orc, q, links, rows, centers, dtype)
    B = c.shape[0]
    p = np.zeros((B, 3), dtype) if opos is None else np.asarray(opos, dtype)
    R = np.broadcast_to(np.eye(3, dtype=dtype), (B, 3, 3)) if orot is None else np.asarray(orot, dtype)
    arm = c - p[:, None]
    y = np.einsum("bji,bsj->bsi", R, arm)
    d, g = sdf(kinds, params, y, dtype)
    d = d - np.asarray(radii, dtype)[None, :, None]
    n = np.einsum("bij,bsmj->bsmi", R, g)
    jpt = None
    if jacobian:
        jl, ja = ikr.jacobians(orc, q, links, ikr.WORLD, dtype)
        r = np.asarray(rows)
        jpt = jl[:, r] + np.cross(ja[:, r], (c - pl)[..., None], axisa=2, axisb=2, axisc=2)
        if fold is not None:
            jpt = np.asarray(fold(jpt), dtype)
    out = dict(c=c, arm=arm, d=d.astype(dtype), n=n.astype(dtype), jpt=jpt)
    assert all(v is None or v.dtype == dtype for v in out.values())
    return out


def distances(F):
    """-> (dist (B, S), nearest (B, S): the first primitive that attains the minimum)."""
    return F["d"].min(-1), F["d"].argmin(-1).astype(np.int32)


def distances_vjp(F, grad_dist):
    """grad_x (B, ncol) = sum_s grad_dist[b, s] n_{s, nearest} . Jpt_s."""
    near = F["d"].argmin(-1)
    nn = np.take_along_axis(F["n"], near[..., None, None], 2)[:, :, 0]
    return np.einsum("bs,bsr,bsrc->bc", np.asarray(grad_dist, F["d"].dtype), nn, F["jpt"])


def penalty(F, margin, prim_weight=None):
    """-> (E (B,), grad_x (B, ncol) or None without a Jacobian, wrench (B, 6), h (B, S, M))."""
    dtype = F["d"].dtype.type
    w = np.ones(F["d"].shape[-1], dtype) if prim_weight is None else np.asarray(prim_weight, dtype)
    h = np.maximum(dtype(0), dtype(margin) - F["d"])
    E = (w * h * h).sum((1, 2))
    f = ((dtype(-2) * w * h)[..., None] * F["n"]).sum(2)  # (B, S, 3): dE/dc_s
    grad = None if F["jpt"] is None else np.einsum("bsr,bsrc->bc", f, F["jpt"])
    wrench = np.concatenate([-f.sum(1), -np.cross(F["arm"], f).sum(1)], -1)
    assert E.dtype == dtype and wrench.dtype == dtype
    return E, grad, wrench, h

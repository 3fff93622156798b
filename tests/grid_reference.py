"""numpy restatement of the signed-distance-grid collision (include/dexr_sdf_grid.h), the yardstick of tests/test_grid_host.py and
tests/test_gpu_grid.py.  It shares no code with csrc/dexr_sdf_grid.hpp: the sphere centres come from collision_reference.centres,
the interpolant is the sum of the eight corner samples times the products of their weights (t or 1 - t per axis) and its
derivative the same sum with one weight replaced by +-1 -- not the nested a + t (b - a) of the kernel --, the cell coordinate is
(y - origin) / spacing, a division, and the gradient in x goes through the dense point Jacobian exactly as
obstacle_reference.fields builds it.  Every operation is in the asked `dtype`; the samples are float32 values widened to it.

`values` (nx, ny, nz), `origin` (3,), `spacing` (3,) are the grid as dexr_sdf_grid_create takes it; `opos` (B, 3) / `orot`
(B, 3, 3) the obstacle pose per frame or None.  `links`, `rows`, `centers`, `radii`, `q`, `fold` as in collision_reference."""
import numpy as np

import collision_reference as cref
import ik_reference as ikr


def sdf(values, origin, spacing, y, dtype=np.float64):
    """y (..., 3) points of the obstacle frame -> (sdf (...), grad (..., 3), gap (...): the distance in metres to the nearest
    place where the gradient jumps -- a cell face for a coordinate inside the grid's box, the plane of the box it left for one
    outside)."""
    V = np.asarray(values, np.float32).astype(dtype)
    n = np.array(V.shape)
    o, h = np.asarray(origin, np.float64).astype(dtype), np.asarray(spacing, np.float64).astype(dtype)
    y = np.asarray(y, dtype)
    u = (y - o) / h
    top = (n - 1).astype(dtype)
    with np.errstate(invalid="ignore"):
        uc = np.where(u > 0, np.where(u < top, u, top), dtype(0)).astype(dtype)  # (a NaN goes to 0)
    i = np.minimum(np.floor(uc).astype(np.int64), n - 2)
    t = (uc - i.astype(dtype)).astype(dtype)
    e = ((u - uc) * h).astype(dtype)
    one = dtype(1)
    v = np.zeros(y.shape[:-1], dtype)
    dv = np.zeros(y.shape, dtype)
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                s = V[i[..., 0] + cx, i[..., 1] + cy, i[..., 2] + cz]
                w = [t[..., a] if c else one - t[..., a] for a, c in enumerate((cx, cy, cz))]
                sign = [one if c else -one for c in (cx, cy, cz)]
                v = v + w[0] * w[1] * w[2] * s
                dv[..., 0] += sign[0] * w[1] * w[2] * s
                dv[..., 1] += w[0] * sign[1] * w[2] * s
                dv[..., 2] += w[0] * w[1] * sign[2] * s
    ln = np.sqrt((e * e).sum(-1))
    with np.errstate(invalid="ignore"):
        out = np.where(ln[..., None] > 0, e / np.where(ln > 0, ln, one)[..., None], dtype(0))
        grad = np.where(u == uc, dv / h, dtype(0)) + out
        inside = u == uc
        gap = np.where(inside, np.abs(u - np.round(u)), np.abs(u - uc)) * h
    return (v + ln).astype(dtype), grad.astype(dtype), gap.min(-1).astype(np.float64)


def fields(orc, q, links, rows, centers, radii, values, origin, spacing, opos=None, orot=None, dtype=np.float64, fold=None, jacobian=True):
    """-> dict: c (B, S, 3) world centres, arm (B, S, 3) = c - p_o, y (B, S, 3), d (B, S) = sdf(y_s) - r_s, n (B, S, 3) world
    normals, gap (B, S), outside (B, S): y_s is outside the grid's box, jpt (B, S, 3, ncol) the point Jacobians (None without
    `jacobian`)."""
    q = np.asarray(q, dtype)
    c, pl = cref.centres(orc, q, links, rows, centers, dtype)
    B = c.shape[0]
    p = np.zeros((B, 3), dtype) if opos is None else np.asarray(opos, dtype)
    R = np.broadcast_to(np.eye(3, dtype=dtype), (B, 3, 3)) if orot is None else np.asarray(orot, dtype)
    arm = c - p[:, None]
    y = np.einsum("bji,bsj->bsi", R, arm)
    d, g, gap = sdf(values, origin, spacing, y, dtype)
    d = d - np.asarray(radii, dtype)[None, :]
    n = np.einsum("bij,bsj->bsi", R, g)
    hi = np.asarray(origin, np.float64) + (np.array(np.shape(values)) - 1) * np.asarray(spacing, np.float64)
    outside = ((y < np.asarray(origin, np.float64)) | (y > hi)).any(-1)
    jpt = None
    if jacobian:
        jl, ja = ikr.jacobians(orc, q, links, ikr.WORLD, dtype)
        r = np.asarray(rows)
        jpt = jl[:, r] + np.cross(ja[:, r], (c - pl)[..., None], axisa=2, axisb=2, axisc=2)
        if fold is not None:
            jpt = np.asarray(fold(jpt), dtype)
    out = dict(c=c, arm=arm, y=y.astype(dtype), d=d.astype(dtype), n=n.astype(dtype), jpt=jpt)
    assert all(v is None or v.dtype == dtype for v in out.values())
    out.update(gap=gap, outside=outside)
    return out


def distances(F):
    """-> dist (B, S)."""
    return F["d"]


def distances_vjp(F, grad_dist):
    """grad_x (B, ncol) = sum_s grad_dist[b, s] n_s . Jpt_s."""
    return np.einsum("bs,bsr,bsrc->bc", np.asarray(grad_dist, F["d"].dtype), F["n"], F["jpt"])


def penalty(F, margin):
    """-> (E (B,), grad_x (B, ncol) or None without a Jacobian, wrench (B, 6), h (B, S))."""
    dtype = F["d"].dtype.type
    h = np.maximum(dtype(0), dtype(margin) - F["d"])
    E = (h * h).sum(1)
    f = (dtype(-2) * h)[..., None] * F["n"]  # (B, S, 3): dE/dc_s
    grad = None if F["jpt"] is None else np.einsum("bsr,bsrc->bc", f, F["jpt"])
    wrench = np.concatenate([-f.sum(1), -np.cross(F["arm"], f).sum(1)], -1)
    assert E.dtype == dtype and wrench.dtype == dtype
    return E, grad, wrench, h


def polynomial(coef, y):
    """the global trilinear polynomial f(y) = a0 + b . y + c_xy x y + c_yz y z + c_xz x z + c_xyz x y z and its gradient, float64:
    coef = (a0, bx, by, bz, c_xy, c_yz, c_xz, c_xyz)"""
    a0, bx, by, bz, cxy, cyz, cxz, cxyz = (float(v) for v in coef)
    x, yy, z = (np.asarray(y, np.float64)[..., a] for a in range(3))
    f = a0 + bx * x + by * yy + bz * z + cxy * x * yy + cyz * yy * z + cxz * x * z + cxyz * x * yy * z
    g = np.stack([bx + cxy * yy + cxz * z + cxyz * yy * z, by + cxy * x + cyz * z + cxyz * x * z, bz + cyz * yy + cxz * x + cxyz * x * yy], -1)
    return f, g

"""numpy restatement of the sphere-pair self-collision (include/dexr_spheres.h), the yardstick of tests/test_collision_host.py and
tests/test_gpu_collision.py.  It shares no code with csrc/dexr_spheres.hpp: the poses come link by link from the link's own
joint chain (ik_solve_reference.link_poses), distances and the energy are dense over all pairs, and the gradients come from
the dense link Jacobians of ik_reference.jacobians through the point-Jacobian formula

    Jpt_s[:, c] = Jlin_l[:, c] + Jang_l[:, c] x (c_s - p_l)          dd_p/dx_c = n_p . (Jpt_i[:, c] - Jpt_j[:, c]).

No subtree ranges, no incidence lists, no forces: a (B, P, n) matrix dd/dx, contracted.  Every operation is in the asked `dtype`.

`links` are the link names of the TABLE (distinct), `rows` (S,) the row of each sphere in them, `centers` (S, 3), `radii` (S,),
`pairs` (P, 2).  `q` is the oracle's full joint vector; a table with a source map passes `fold`, the chain rule of that map on
the last axis (as in ik_reference)."""
import numpy as np

import ik_reference as ikr
import ik_solve_reference as isr


def centres(orc, q, links, rows, centers, dtype=np.float64):
    """-> (c (B, S, 3) world centres, p (B, S, 3) the origin of each sphere's link)."""
    p, R = isr.link_poses(orc, q, links, dtype)
    rows = np.asarray(rows)
    c = p[:, rows] + np.einsum("bsij,sj->bsi", R[:, rows], np.asarray(centers, dtype))
    assert c.dtype == dtype
    return c, p[:, rows]


def distances(orc, q, links, rows, centers, radii, pairs, dtype=np.float64):
    """-> (dist (B, P), c (B, S, 3), n (B, P, 3) the unit vector from sphere j to sphere i, 0 where the centres coincide)."""
    c, _ = centres(orc, q, links, rows, centers, dtype)
    pairs, r = np.asarray(pairs), np.asarray(radii, dtype)
    D = c[:, pairs[:, 0]] - c[:, pairs[:, 1]]
    s = np.sqrt((D * D).sum(-1))
    dist = s - r[pairs[:, 0]] - r[pairs[:, 1]]
    n = np.where(s[..., None] > 0, D / np.where(s > 0, s, dtype(1))[..., None], dtype(0)).astype(dtype)
    assert dist.dtype == dtype
    return dist, c, n


def distance_jacobian(orc, q, links, rows, centers, radii, pairs, dtype=np.float64, fold=None):
    """dd/dx (B, P, n): n = dof, or the width `fold` gives."""
    _, c, n = distances(orc, q, links, rows, centers, radii, pairs, dtype)
    _, pl = centres(orc, q, links, rows, centers, dtype)
    jl, ja = ikr.jacobians(orc, q, links, ikr.WORLD, dtype)
    rows, pairs = np.asarray(rows), np.asarray(pairs)
    arm = c - pl  # (B, S, 3)
    # Jpt (B, S, 3, dof): Jlin + Jang x arm, column by column
    jpt = jl[:, rows] + np.cross(ja[:, rows], arm[..., None], axisa=2, axisb=2, axisc=2)
    if fold is not None:
        jpt = np.asarray(fold(jpt), dtype)
    dd = np.einsum("bpr,bprc->bpc", n, jpt[:, pairs[:, 0]] - jpt[:, pairs[:, 1]])
    assert dd.dtype == dtype
    return dd


def distances_vjp(orc, q, links, rows, centers, radii, pairs, grad_dist, dtype=np.float64, fold=None):
    """grad_x (B, n) = sum_p grad_dist[b, p] dd_p/dx."""
    dd = distance_jacobian(orc, q, links, rows, centers, radii, pairs, dtype, fold)
    return np.einsum("bp,bpc->bc", np.asarray(grad_dist, dtype), dd)


def penalty(orc, q, links, rows, centers, radii, pairs, margin, pair_weight=None, dtype=np.float64, fold=None):
    """-> (E (B,), grad_x (B, n), h (B, P)): h = max(0, margin - d), E = sum w h^2, grad = sum -2 w h dd/dx."""
    dist = distances(orc, q, links, rows, centers, radii, pairs, dtype)[0]
    w = np.ones(len(pairs), dtype) if pair_weight is None else np.asarray(pair_weight, dtype)
    h = np.maximum(dtype(0), dtype(margin) - dist)
    E = (w * h * h).sum(-1)
    g = distances_vjp(orc, q, links, rows, centers, radii, pairs, dtype(-2) * w * h, dtype, fold)
    assert E.dtype == dtype and g.dtype == dtype
    return E, g, h

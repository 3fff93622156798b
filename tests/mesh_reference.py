"""The yardstick of the mesh distance kernels: the definition of include/dexr_mesh_sdf.h in vectorised numpy, with a dtype switch,
and the meshes of the tests, generated in code.

`sdf(vertices, faces, points, dtype)` -> (signed distance, winding number), both float64 arrays holding values computed in `dtype`:
the per-triangle records a, ab = b - a, ac = c - a are made in float64 and rounded to `dtype`, the seven regions are tested in the
header's order, every Omega_t is evaluated in `dtype` and the winding sum is accumulated in float64 in triangle order (a cumulative
sum) in both precisions, as the kernel does.  numpy does not fuse multiply-add; the kernel does, where its source says fma(): the
float32 gate of the GPU tests is the distance between this file's float32 and float64 runs, which is of the size of that difference."""
import functools

import numpy as np

PAIRS_PER_CHUNK = 1 << 18  # point-triangle pairs held in memory at once


def records(vertices, faces, dtype=np.float64):
    v = np.asarray(vertices, np.float64)
    f = np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return a.astype(dtype), (b - a).astype(dtype), (c - a).astype(dtype)


def _dot(x, y):
    return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]


def pair_fields(a, ab, ac, p):
    """a, ab, ac (T, 3) and p (P, 3) of one dtype -> dict of (P, T) arrays in that dtype: q (squared distance), omega (solid angle),
    region (1..7, the header's numbering), v, w (barycentric coordinates of the closest point)."""
    one, zero = p.dtype.type(1), p.dtype.type(0)
    ap = p[:, None, :] - a[None]
    bp = ap - ab[None]
    cp = ap - ac[None]
    AB, AC = ab[None], ac[None]
    d1, d2, d3, d4, d5, d6 = _dot(AB, ap), _dot(AC, ap), _dot(AB, bp), _dot(AC, bp), _dot(AB, cp), _dot(AC, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
    region = np.select(conds, [1, 2, 3, 4, 5, 6], 7)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w6 = e43 / (e43 + e56)
        den = va + vb + vc
        vs = [zero * d1, one + zero * d1, d1 / (d1 - d3), zero * d1, zero * d1, one - w6, vb / den]
        ws = [zero * d1, zero * d1, zero * d1, one + zero * d1, d2 / (d2 - d6), w6, vc / den]
    v = np.choose(region - 1, vs)
    w = np.choose(region - 1, ws)
    e = ap - v[..., None] * AB - w[..., None] * AC
    q = _dot(e, e)
    A, B, C = -ap, -bp, -cp
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    det = (A[..., 0] * (B[..., 1] * C[..., 2] - B[..., 2] * C[..., 1]) + A[..., 1] * (B[..., 2] * C[..., 0] - B[..., 0] * C[..., 2])
           + A[..., 2] * (B[..., 0] * C[..., 1] - B[..., 1] * C[..., 0]))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    omega = p.dtype.type(2) * np.arctan2(det, den)
    assert q.dtype == p.dtype and omega.dtype == p.dtype
    return dict(q=q, omega=omega, region=region, v=v, w=w)


def sdf(vertices, faces, points, dtype=np.float64):
    """-> (dist (P,), winding (P,)) float64 arrays of values computed in `dtype`; a point that is not finite gives NaN in both."""
    a, ab, ac = records(vertices, faces, dtype)
    with np.errstate(over="ignore"):
        p = np.asarray(points, np.float64).reshape(-1, 3).astype(dtype)
    P, T = len(p), len(a)
    dist, wind = np.empty(P), np.empty(P)
    step = max(1, PAIRS_PER_CHUNK // T)
    for s in range(0, P, step):
        with np.errstate(invalid="ignore", over="ignore"):
            F = pair_fields(a, ab, ac, p[s:s + step])
            q = np.where(np.isnan(F["q"]), np.inf, F["q"]).min(1)  # (a NaN never wins)
            w = np.cumsum(F["omega"].astype(np.float64), axis=1)[:, -1] * 0.07957747154594767
            u = np.sqrt(q.astype(dtype)).astype(np.float64)
        ok = np.isfinite(p[s:s + step]).all(1)
        dist[s:s + step] = np.where(ok, np.where(w >= 0.5, -u, u), np.nan)
        wind[s:s + step] = np.where(ok, w.astype(dtype).astype(np.float64), np.nan)
    return dist, wind


def grid_points(n, origin, spacing):
    """(nx ny nz, 3) float64 in C order: origin + (ix, iy, iz) * spacing, product and sum each rounded once."""
    ax = [np.float64(origin[k]) + np.arange(n[k], dtype=np.float64) * np.float64(spacing[k]) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def cube(half_extents=(0.03, 0.02, 0.04), rotation=None, centre=(0.0, 0.0, 0.0)):
    """12 triangles, outward normals; vertex k has the signs of the bits of k (x: bit 0)."""
    h = np.asarray(half_extents, np.float64)
    s = np.array([[(k >> i & 1) * 2 - 1 for i in range(3)] for k in range(8)], np.float64)
    v = s * h
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]  # -x +x -y +y -z +z, counter-clockwise from outside
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    R = np.eye(3) if rotation is None else np.asarray(rotation, np.float64)
    return v @ R.T + np.asarray(centre, np.float64), f


def tetrahedron(r=0.05):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * (r / np.sqrt(3.0))
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def _icosphere(k):
    g = (1 + np.sqrt(5.0)) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(x, np.float64) / np.sqrt(1 + g * g) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(k):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v, f = np.array(v), np.array(f, np.int32)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


def icosphere(k, r=0.05):
    """20 * 4^k triangles on the sphere of radius r about the origin, outward normals."""
    v, f = _icosphere(k)
    return v * r, f.copy()


def open_icosphere(k=2, r=0.05, plane=0.6):
    """the icosphere without the faces whose centroid lies above z = plane * r (k = 2, plane 0.6: 260 of 320 faces stay)."""
    v, f = icosphere(k, r)
    keep = v[f].mean(1)[:, 2] <= plane * r
    return v, f[keep]

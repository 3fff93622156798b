"""Triangle meshes from files and from URDF primitives, with numpy alone (host plumbing, cold path).

``load_mesh(path)`` reads binary and ASCII STL and Wavefront OBJ and returns ``(vertices (V, 3) float64, faces (T, 3) int32)``.  STL
stores three coordinates per corner and no connectivity: the corners are welded by EXACT coordinates, so that a solid that was
written closed is closed again (``collision.TriangleMesh.is_closed``); nothing is welded by a tolerance.  OBJ: ``v`` and ``f`` lines,
polygons fanned from their first corner, negative (relative) indices, the ``v/vt/vn`` forms; everything else is skipped.  Any other
suffix is a ValueError naming the file.  ``save_stl`` and ``save_obj`` write what ``load_mesh`` reads.

``box_mesh``, ``cylinder_mesh`` and ``sphere_mesh`` tessellate the URDF primitives: closed, normals (b - a) x (c - a) outwards.  A
cylinder is a prism over a regular polygon INSCRIBED in its circle and the sphere an icosphere inscribed in its sphere: both lie
inside the primitive, so spheres fitted to them do too.

``link_mesh(elements)`` turns the ``(kind, params, origin)`` list of one link (``urdf.parse_collision_geometry``) into one mesh: every
element is tessellated or loaded, transformed by its origin and the lot concatenated.  The consequence for overlapping elements: the
winding-number sign of ``SdfGrid.from_mesh`` treats the union as inside (a point inside two elements has winding number 2), but the
unsigned distance also sees the faces buried in the overlap, so inscribed radii there come out smaller than the union's, never
larger."""
from __future__ import annotations

import os
import struct

import numpy as np


def _weld(corners):
    """corners (T, 3, 3) -> vertices (V, 3), faces (T, 3): equal coordinates become one vertex, in order of first appearance"""
    flat = np.ascontiguousarray(corners, dtype=np.float64).reshape(-1, 3) + 0.0  # (-0.0 and 0.0 are one coordinate)
    _, first, inverse = np.unique(flat, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return flat[first[order]], rank[np.asarray(inverse).reshape(-1)].reshape(-1, 3).astype(np.int32)


def _load_stl(path):
    with open(path, "rb") as f:
        data = f.read()
    if len(data) >= 84:
        (n,) = struct.unpack_from("<I", data, 80)
        if len(data) == 84 + 50 * n:  # binary: 80 bytes of header, the count, 50 bytes per triangle
            rec = np.frombuffer(data, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n, offset=84)
            return _weld(rec["v"])
    text = data.decode("ascii", errors="replace")
    if not text.lstrip().lower().startswith("solid"):
        raise ValueError(f"{path}: neither a binary STL of the length its header states nor an ASCII one")
    corners = [[float(t) for t in line.split()[1:4]] for line in text.splitlines() if line.strip().lower().startswith("vertex")]
    if not corners or len(corners) % 3:
        raise ValueError(f"{path}: {len(corners)} vertex lines are not a whole number of triangles")
    return _weld(np.array(corners).reshape(-1, 3, 3))


def _load_obj(path):
    vertices, faces = [], []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                vertices.append([float(t) for t in tok[1:4]])
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(vertices) + i)
                faces += [(idx[0], idx[j], idx[j + 1]) for j in range(1, len(idx) - 1)]
    if not vertices or not faces:
        raise ValueError(f"{path}: no vertices or no faces")
    return np.array(vertices, dtype=np.float64), np.array(faces, dtype=np.int32)


def load_mesh(path):
    """-> (vertices (V, 3) float64, faces (T, 3) int32) of a .stl (binary or ASCII) or .obj file"""
    suffix = os.path.splitext(str(path))[1].lower()
    if suffix == ".stl":
        return _load_stl(path)
    if suffix == ".obj":
        return _load_obj(path)
    raise ValueError(f"{path}: only .stl and .obj meshes are read, not {suffix or 'a file without a suffix'}")


def save_stl(path, vertices, faces, binary: bool = True):
    tri = np.asarray(vertices, dtype=np.float64)[np.asarray(faces)]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    if binary:
        rec = np.zeros(len(tri), dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
        rec["n"], rec["v"] = nrm, tri
        with open(path, "wb") as f:
            f.write(b"\0" * 80 + struct.pack("<I", len(tri)) + rec.tobytes())
        return
    with open(path, "w") as f:
        f.write("solid mesh\n")
        for n, t in zip(nrm, tri):
            f.write(f"facet normal {n[0]!r} {n[1]!r} {n[2]!r}\n outer loop\n")
            f.write("".join(f"  vertex {float(c[0])!r} {float(c[1])!r} {float(c[2])!r}\n" for c in t))
            f.write(" endloop\nendfacet\n")
        f.write("endsolid mesh\n")


def save_obj(path, vertices, faces):
    with open(path, "w") as f:
        f.write("".join(f"v {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n" for v in np.asarray(vertices, dtype=np.float64)))
        f.write("".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in np.asarray(faces).tolist()))


# ---- the URDF primitives ----------------------------------------------------------------------------------------------------------------
def box_mesh(size):
    """the box of full extents `size` (3,) about the origin: 8 vertices, 12 triangles"""
    h = np.asarray(size, dtype=np.float64).reshape(3) / 2.0
    v = np.array([[(k >> i & 1) * 2 - 1 for i in range(3)] for k in range(8)], dtype=np.float64) * h
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]  # -x +x -y +y -z +z, counter-clockwise from outside
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)


def cylinder_mesh(radius, length, segments: int = 32):
    """the prism over the regular `segments`-gon inscribed in the circle, axis z, centred: 2 segments + 2 vertices, 4 segments triangles"""
    n = int(segments)
    if n < 3:
        raise ValueError(f"a cylinder needs at least 3 segments, got {segments}")
    a = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(a), radius * np.sin(a)], -1)
    lo, hi = np.concatenate([ring, np.full((n, 1), -length / 2.0)], 1), np.concatenate([ring, np.full((n, 1), length / 2.0)], 1)
    v = np.concatenate([lo, hi, [[0.0, 0.0, -length / 2.0], [0.0, 0.0, length / 2.0]]])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, n + j), (i, n + j, n + i), (2 * n, j, i), (2 * n + 1, n + i, n + j)]
    return v, np.array(f, dtype=np.int32)


def sphere_mesh(radius, level: int = 2):
    """the icosphere of 20 * 4^level triangles inscribed in the sphere about the origin"""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [np.array(x, dtype=np.float64) / np.sqrt(1.0 + g * g) for x in
         ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1))]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(level)):
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
    return np.array(v) * float(radius), np.array(f, dtype=np.int32)


def link_mesh(elements):
    """[(kind, params, origin 4x4), ...] of one link -> (vertices, faces) of all elements in the link's frame, concatenated"""
    vs, fs, base = [], [], 0
    for kind, params, origin in elements:
        if kind == "box":
            v, f = box_mesh(params)
        elif kind == "cylinder":
            v, f = cylinder_mesh(params[0], params[1])
        elif kind == "sphere":
            v, f = sphere_mesh(params[0])
        elif kind == "mesh":
            v, f = load_mesh(params[0])
            scale = np.asarray(params[1], dtype=np.float64)
            v = v * scale
            if np.prod(scale) < 0:  # a mirror turns every triangle over
                f = f[:, ::-1]
        else:
            raise ValueError(f"unknown collision geometry {kind!r}")
        T = np.asarray(origin, dtype=np.float64)
        vs.append(v @ T[:3, :3].T + T[:3, 3])
        fs.append(np.asarray(f, dtype=np.int64) + base)
        base += len(v)
    if not vs:
        raise ValueError("a link without collision geometry has no mesh")
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


__all__ = ["load_mesh", "save_stl", "save_obj", "box_mesh", "cylinder_mesh", "sphere_mesh", "link_mesh"]

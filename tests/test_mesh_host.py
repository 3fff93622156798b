"""CPU tests of the mesh distance interface (include/dexr_mesh_sdf.h, dex_retargeting_amd/collision.py): the export list against the
header, the place and the contents of the fragment, the argument rules (every one a ValueError / DEXR_ERR_INVALID before any device
call), the host-side mesh properties, the fitted box of SdfGrid.from_mesh, the yardstick tests/mesh_reference.py against closed
forms, and the conditions that tests/test_gpu_mesh.py relies on, on the point sets it uses (case(name), computed once and shared).

SIGN_GAP = 1e-6 m: where 0 < |d_ref| < SIGN_GAP the sign (and the winding number, which jumps by one across the surface) of a
float32 run may differ from the reference's; at most 1 % of every point set may lie there.  Points with d_ref = 0 exactly (the cube
lattices put samples on faces, edges and corners) have no sign to compare.  WIND_BAND = 1e-3: on an open mesh the sign is also left
out where |w_ref - 0.5| < WIND_BAND; at most 1 % of the open icosphere's points may lie there."""
import functools
import os
import re

import numpy as np
import pytest

import mesh_reference as mr
from testutil import REPO
from dex_retargeting_amd import _lib, collision

HEADER = os.path.join(REPO, "include", "dexr_mesh_sdf.h")
FRAGMENT = os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_mesh_sdf.hpp")
SIGN_GAP, WIND_BAND = 1e-6, 1e-3
TILE = _lib.MESH_TILE
# a cube whose faces, edges and corners lie on a dyadic lattice: half extents of two cells per axis
CUBE_H = np.array([2.0 ** -6, 2.0 ** -7, 2.0 ** -5])
CUBE_HALF = 2 * CUBE_H
CUBE_N = (9, 7, 11)
CUBE_O = -np.array([4, 3, 5]) * CUBE_H
TURN = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])  # x -> y -> z -> x: exact
TURN_C = np.array([2.0 ** -6, -(2.0 ** -5), 2.0 ** -7])
TRIANGLE = (np.array([[0.0, 0.0, 0.0], [0.04, 0.0, 0.0], [0.0, 0.03, 0.0]]), np.array([[0, 1, 2]], np.int32))
# (x, y) above each of the seven regions of TRIANGLE, in the header's order
REGION_XY = [(-0.01, -0.01), (0.06, -0.01), (0.02, -0.01), (-0.005, 0.05), (-0.01, 0.015), (0.03, 0.03), (0.01, 0.01)]
TET_GRIDS = {"tet_2x2x2": ((2, 2, 2), np.array([-0.04, -0.04, -0.04]), np.array([0.08, 0.08, 0.08])),
             "tet_5x7x9": ((5, 7, 9), np.array([-0.06, -0.05, -0.07]), np.array([0.03, 0.017, 0.0175]))}
PREFIXES = (TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 1280)


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _seeded(seed, n, half=0.1):
    return _r32(np.random.default_rng(seed).uniform(-half, half, (n, 3)))


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def multi_launch_shape(n_triangle):
    """the smallest cube of samples that needs three launches against a mesh of n_triangle triangles"""
    per = _lib.mesh_points_per_launch(n_triangle)
    n = int(np.ceil((2 * per + 1) ** (1.0 / 3.0)))
    while n ** 3 <= 2 * per:
        n += 1
    while (n - 1) ** 3 > 2 * per:
        n -= 1
    return (n, n, n)


MULTI_O, MULTI_BOX = np.full(3, -0.08), 0.16


def multi_launch_grid():
    v, f = mr.icosphere(4)
    n = multi_launch_shape(len(f))
    return n, MULTI_O, np.full(3, MULTI_BOX / (n[0] - 1))


def _points_of(name):
    """(vertices, faces, points (P, 3) float32-representable, open mesh?) of a point set of the GPU tests"""
    if name == "triangle":
        designed = [(x, y, z) for x, y in REGION_XY for z in (0.01, -0.02)] + [(x, y, 0.0) for x, y in REGION_XY[:6]]
        return (*TRIANGLE, np.concatenate([_r32(designed), _seeded(3, 200, 0.04)]), True)
    if name in ("cube", "cube_turn"):
        lattice = mr.grid_points(CUBE_N, CUBE_O, CUBE_H)
        if name == "cube":
            return (*mr.cube(CUBE_HALF), lattice, False)
        return (*mr.cube(CUBE_HALF, TURN, TURN_C), lattice @ TURN.T + TURN_C, False)
    if name == "cube_rot":
        return (*mr.cube((0.03, 0.02, 0.04), _rotation(5), (0.01, -0.02, 0.005)), _seeded(6, 1500), False)
    if name in TET_GRIDS:
        return (*mr.tetrahedron(), _r32(mr.grid_points(*TET_GRIDS[name])), False)
    if name.startswith("ico3_"):
        T = int(name.split("_")[1])
        v, f = mr.icosphere(3)
        return v, f[:T], _seeded(7, 400), T < len(f)
    if name == "open2":
        return (*mr.open_icosphere(), _seeded(8, 2000), True)
    assert name == "multi"
    n, o, h = multi_launch_grid()
    idx = np.sort(np.random.default_rng(9).choice(n[0] * n[1] * n[2], 256, replace=False))
    ijk = np.stack(np.unravel_index(idx, n), -1)
    return (*mr.icosphere(4), _r32(o + ijk * h), False)


POINT_SETS = ["triangle", "cube", "cube_turn", "cube_rot", "tet_2x2x2", "tet_5x7x9"] + [f"ico3_{T}" for T in PREFIXES] + ["open2", "multi"]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of a point set: v, f, p, open, mesh (collision.TriangleMesh), d64, w64, d32, w32 (the yardstick's two runs); read-only"""
    v, f, p, is_open = _points_of(name)
    assert np.array_equal(p, _r32(p))
    d64, w64 = mr.sdf(v, f, p, np.float64)
    d32, w32 = mr.sdf(v, f, p, np.float32)
    out = dict(v=v, f=f, p=p, d64=d64, w64=w64, d32=d32, w32=w32)
    for a in out.values():
        a.setflags(write=False)
    return dict(out, open=is_open, mesh=collision.TriangleMesh(v, f))


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    exports = _lib.MESH_SDF_EXPORTS
    assert declared == set(exports) and len(exports) == 7 and len(set(exports)) == 7
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS, _lib.WRENCH_EXPORTS, _lib.IK_EXPORTS, _lib.IK_SOLVE_EXPORTS, _lib.SPHERE_EXPORTS,
                  _lib.RESOLVE_EXPORTS, _lib.OBSTACLE_EXPORTS, _lib.RESOLVE_OBSTACLE_EXPORTS, _lib.SDF_GRID_EXPORTS, _lib.RESOLVE_GRID_EXPORTS):
        assert not set(exports) & set(other)
    lib = _lib.load()
    for name in exports:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h != "dexr_mesh_sdf.h":
            assert not _declared(os.path.join(REPO, "include", h)) & declared, h
    text = open(HEADER).read()
    assert int(re.search(r"#define DEXR_MESH_MAX_VERTICES \(1 << (\d+)\)", text).group(1)) == 20 and _lib.MESH_MAX_VERTICES == 1 << 20
    assert int(re.search(r"#define DEXR_MESH_MAX_TRIANGLES \(1 << (\d+)\)", text).group(1)) == 20 and _lib.MESH_MAX_TRIANGLES == 1 << 20
    assert int(re.search(r"#define DEXR_MESH_TILE (\d+)", text).group(1)) == _lib.MESH_TILE
    assert int(re.search(r"#define DEXR_MESH_BLOCK_POINTS (\d+)", text).group(1)) == _lib.MESH_BLOCK_POINTS
    assert 1 << int(re.search(r"#define DEXR_MESH_PAIRS_PER_LAUNCH \(1ll << (\d+)\)", text).group(1)) == _lib.MESH_PAIRS_PER_LAUNCH
    assert '#include "dexr_sdf_grid.h"' in text and "DEXR_SDF_GRID_MAX_SAMPLES" in text
    assert not re.search(r"#define DEXR_SDF_GRID", text)  # the grid rules by the other header's macros, not restated
    for n in ("TriangleMesh", "mesh_distances", "SdfGrid"):
        assert n in collision.__all__
    for m in ("distances_dev", "distances", "sample_grid_dev", "sample_grid"):
        assert hasattr(_lib.TriangleMesh, m)
    assert _lib.mesh_points_per_launch(1) == _lib.MESH_PAIRS_PER_LAUNCH and _lib.mesh_points_per_launch(1 << 20) % _lib.MESH_BLOCK_POINTS == 0
    assert _lib.mesh_points_per_launch(_lib.MESH_MAX_TRIANGLES) * _lib.MESH_MAX_TRIANGLES <= _lib.MESH_PAIRS_PER_LAUNCH


def test_the_fragment_is_included_once_and_last_and_has_no_forbidden_construct():
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_mesh_sdf.hpp"') == 1 and pose.count("dexr_mesh_sdf.hpp") == 1
    assert pose.index('"dexr_mesh_sdf.hpp"') > pose.index('"dexr_resolve_grid.hpp"')
    assert pose.rindex('#include "') == pose.index('#include "dexr_mesh_sdf.hpp"')  # no include follows it
    src = open(FRAGMENT).read()
    assert "getenv" not in src and "atomic" not in src and "asm" not in src.replace("__restrict__", "")
    assert src.count('#include "') == 1 and '#include "dexr_mesh_sdf.h"' in src  # (a fragment: no unit of its own)
    for n in ("DEXR_MESH_TILE", "DEXR_MESH_BLOCK_POINTS", "DEXR_MESH_PAIRS_PER_LAUNCH", "DEXR_MESH_MAX_TRIANGLES", "DEXR_SDF_GRID_MAX_SAMPLES"):
        assert n in src  # the code reads the named constants, not numbers of its own
    assert "__shfl" not in src and "__reduce" not in src and "dpp" not in src  # no reduction across lanes


# ---- 2. the argument rules --------------------------------------------------------------------------------------------------------------
def _create(nv, v, nt, f, out=True):
    lib, C = _lib.load(), _lib.C
    v = None if v is None else np.ascontiguousarray(v, np.float64)
    f = None if f is None else np.ascontiguousarray(f, np.int32)
    h = C.c_void_p()
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = lib.dexr_mesh_create(nv, p(v, C.c_double), nt, p(f, C.c_int32), C.byref(h) if out else None)
    if rc == 0:
        lib.dexr_mesh_destroy(h)
    else:
        assert not h.value
    return rc, lib.dexr_last_error().decode()


def _malformed():
    """(word of the C message, word of the Python message, vertices, faces) of every malformed mesh"""
    v, f = mr.tetrahedron()
    out = []
    for bad in (-1, 4, 1 << 20):
        g = f.copy()
        g[2, 1] = bad
        out.append(("out of range", "face index", v, g))
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[3, 2] = bad
        out.append(("not finite", "finite", w, f))
    g = f.copy()
    g[1] = (0, 3, 3)  # two equal indices
    out.append(("no area", "no area", v, g))
    w = np.concatenate([v, [v[0] + 0.5 * (v[1] - v[0])]])  # a fifth vertex in the middle of the edge 0-1, exactly
    out.append(("no area", "no area", w, np.concatenate([f, [[0, 4, 1]]]).astype(np.int32)))
    return out


def test_mesh_create_validates_before_it_looks_for_a_device():
    v, f = mr.tetrahedron()
    for cword, _, bv, bf in _malformed():
        rc, msg = _create(len(bv), bv, len(bf), bf)
        assert rc == -1 and cword in msg, (rc, msg)
    for args in ((4, None, 4, f), (4, v, 4, None)):
        rc, msg = _create(*args)
        assert rc == -1 and "null" in msg
    assert _create(4, v, 4, f, out=False)[0] == -1
    big = np.zeros(((1 << 20) + 1, 3))
    for nv, nt in ((0, 4), (-1, 4), ((1 << 20) + 1, 4)):
        rc, msg = _create(nv, big, nt, f)
        assert rc == -1 and "vertices" in msg, msg
    for nt in (0, -1, (1 << 20) + 1):
        rc, msg = _create(4, v, nt, np.zeros(((1 << 20) + 1, 3), np.int32))
        assert rc == -1 and "triangles" in msg, msg
    rc, msg = _create(4, v, 4, f)  # well formed: only a device is missing, if it is
    assert rc in (0, -2), (rc, msg)
    # the other entry points refuse a null mesh and bad grids without a device
    lib, C = _lib.load(), _lib.C
    assert lib.dexr_mesh_info(None, None, None, None) == -1
    assert lib.dexr_mesh_distances_dev(None, 4, None, None, None, None) == -1 and b"null mesh" in lib.dexr_last_error()
    assert lib.dexr_mesh_distances(None, 4, None, None, None) == -1
    assert lib.dexr_mesh_sample_grid_dev(None, None, None, None, None, None) == -1
    assert lib.dexr_mesh_sample_grid(None, None, None, None, None) == -1 and b"null mesh" in lib.dexr_last_error()


def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    touched = []
    monkeypatch.setattr(_lib.TriangleMesh, "__init__", lambda self, *a, **k: touched.append("create"))
    monkeypatch.setattr(_lib.SdfGrid, "__init__", lambda self, *a, **k: touched.append("create grid"))
    for method in ("distances_dev", "distances", "sample_grid_dev", "sample_grid"):
        monkeypatch.setattr(_lib.TriangleMesh, method, lambda self, *a, _m=method, **k: touched.append(_m))
    M = collision.TriangleMesh
    v, f = mr.tetrahedron()
    for _, pword, bv, bf in _malformed():
        with pytest.raises(ValueError, match=pword):
            M(bv, bf)
    for bv, bf, word in ((v[:, :2], f, "vertices must have shape"), (v.reshape(-1), f, "vertices must have shape"), (v, f[:, :2], "faces must be"),
                         (v, f.astype(np.float64), "faces must be"), (np.zeros((0, 3)), f, "vertices"), (v, np.zeros((0, 3), np.int32), "triangles")):
        with pytest.raises(ValueError, match=word):
            M(bv, bf)
    with pytest.raises(ValueError, match="triangles"):  # every triangle dropped
        M(v, [[0, 1, 1], [2, 2, 3]], drop_degenerate=True)
    # drop_degenerate removes exactly the flat ones, in order
    g = np.concatenate([f[:2], [[0, 3, 3]], f[2:]])
    kept = M(v, g, drop_degenerate=True)
    assert kept == M(v, f) and hash(kept) == hash(M(v, f)) and kept != M(v, f[::-1]) and kept.n_triangle == 4 and kept.n_vertex == 4
    assert not kept.vertices.flags.writeable and not kept.faces.flags.writeable and kept.faces.dtype == np.int32
    assert np.array_equal(kept.bounds, [v.min(0), v.max(0)]) and "4 triangles" in repr(kept)
    # from_mesh
    mesh, inside_out, open_mesh = M(v, f), M(v, f[:, ::-1]), M(*mr.open_icosphere())
    F = collision.SdfGrid.from_mesh
    for kw, word in ((dict(), "spacing is required"), (dict(spacing=0.0), "spacing"), (dict(spacing=-0.01), "spacing"), (dict(spacing=np.nan), "spacing"),
                     (dict(spacing=[0.01, 0.01]), "spacing must be a scalar"), (dict(spacing=0.01, padding=-0.01), "padding"),
                     (dict(spacing=0.01, padding=np.inf), "padding"), (dict(spacing=0.01, precision="float16"), "precision"),
                     (dict(spacing=0.01, origin=0.0), "both"), (dict(spacing=0.01, shape=8), "both"), (dict(spacing=0.01, origin=0.0, shape=1), "dimension"),
                     (dict(spacing=0.01, origin=0.0, shape=(1025, 2, 2)), "dimension"), (dict(spacing=0.01, origin=np.nan, shape=4), "origin"),
                     (dict(spacing=1e-5), "dimension"), (dict(spacing=0.0002), "at most")):
        with pytest.raises(ValueError, match=word):
            F(mesh, **kw)
    with pytest.raises(ValueError, match="TriangleMesh"):
        F((v, f), spacing=0.01)
    with pytest.raises(ValueError, match="not closed"):
        F(open_mesh, spacing=0.01)
    with pytest.raises(ValueError, match="inside out"):
        F(inside_out, spacing=0.01)
    for p in ("float64", "float32"):
        with pytest.raises(ValueError, match="inside out"):
            F(inside_out, spacing=0.01, precision=p, origin=-0.05, shape=8)
    # mesh_distances: the device rule comes last
    good = torch.zeros((4, 5, 3), dtype=torch.float32)
    D = collision.mesh_distances
    for pts, word in ((good.numpy(), "torch tensor"), (good.double(), "float32"), (good[..., :2], "shape"), (torch.zeros((), dtype=torch.float32), "shape"),
                      (good, "CUDA")):
        with pytest.raises(ValueError, match=word):
            D(mesh, pts)
        with pytest.raises(ValueError, match=word):
            D(mesh, pts, winding=True)
    with pytest.raises(ValueError, match="TriangleMesh"):
        D((v, f), good)
    assert touched == []


# ---- 3. the host-side properties --------------------------------------------------------------------------------------------------------
def test_is_closed_and_volume():
    M = collision.TriangleMesh
    v, f = mr.cube((0.03, 0.02, 0.04), _rotation(2), (0.1, 0.2, -0.3))
    cube = M(v, f)
    assert cube.is_closed and abs(cube.volume - 8 * 0.03 * 0.02 * 0.04) <= 1e-15 and cube.n_triangle == 12 and cube.n_vertex == 8
    flipped = M(v, f[:, ::-1])
    assert flipped.is_closed and abs(flipped.volume + 8 * 0.03 * 0.02 * 0.04) <= 1e-15
    op = M(*mr.open_icosphere())
    assert op.n_triangle == 260 and not op.is_closed
    assert not M(v, np.concatenate([f, f[3:4]])).is_closed  # one face twice: its edges belong to three triangles
    g = f.copy()
    g[5] = g[5][::-1]  # one face turned over: closed as a surface, not consistently oriented
    assert not M(v, g).is_closed
    assert not M(v, f[:-1]).is_closed
    tet = M(*mr.tetrahedron(0.05))
    assert tet.is_closed and tet.volume > 0
    for k in range(4):
        s = M(*mr.icosphere(k, 0.05))
        assert s.n_triangle == 20 * 4 ** k and s.is_closed and 0 < s.volume < 4 / 3 * np.pi * 0.05 ** 3
    assert M(*mr.icosphere(3, 0.05)).volume > 0.99 * 4 / 3 * np.pi * 0.05 ** 3


def test_from_mesh_fits_the_box(monkeypatch):
    calls = []

    class Fake:
        def sample_grid(self, n, o, h):
            calls.append((tuple(n), np.array(o), np.array(h)))
            return np.zeros(n, np.float32)

    monkeypatch.setattr(collision.TriangleMesh, "device_mesh", lambda self, device_index=0: Fake())
    v, f = mr.cube((0.03, 0.02, 0.04), None, (0.01, 0.0, -0.02))
    mesh = collision.TriangleMesh(v, f)
    lo, hi = mesh.bounds
    assert np.allclose(lo, [-0.02, -0.02, -0.06], rtol=0, atol=1e-16) and np.allclose(hi, [0.04, 0.02, 0.02], rtol=0, atol=1e-16)
    for spacing, pad in ((0.01, 0.0), (0.007, 0.013), ([0.01, 0.005, 0.02], 0.02), (0.5, 0.0)):
        g = collision.SdfGrid.from_mesh(mesh, spacing=spacing, padding=pad)
        n, o, h = calls[-1]
        want_h = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
        want_n = tuple(int(k) + 1 for k in np.ceil((hi - lo + 2 * pad) / want_h))
        assert n == want_n == g.shape and np.array_equal(o, lo - pad) and np.array_equal(h, want_h)
        assert np.array_equal(g.origin, lo - pad) and np.array_equal(g.spacing, want_h)
        assert (o + (np.array(n) - 1) * h >= hi + pad - 1e-15).all()  # the box covers the padded bounds
    assert calls[-1][0] == (2, 2, 2)
    g = collision.SdfGrid.from_mesh(mesh, origin=[-0.1, -0.1, -0.1], spacing=0.05, shape=(5, 4, 3))
    assert calls[-1][0] == (5, 4, 3) == g.shape and np.array_equal(calls[-1][1], [-0.1, -0.1, -0.1])
    inside_out = collision.TriangleMesh(v, f[:, ::-1])
    want = tuple(int(k) + 1 for k in np.ceil((hi - lo) / 0.01))
    assert collision.SdfGrid.from_mesh(inside_out, spacing=0.01, allow_open=True).shape == want
    assert collision.SdfGrid.from_mesh(collision.TriangleMesh(v, f[:-1]), spacing=0.01, allow_open=True).shape == want


# ---- 4. the yardstick against closed forms ----------------------------------------------------------------------------------------------
def _box_params(half, R=None, c=(0, 0, 0)):
    v = np.zeros(16)
    v[:3], v[3:6], v[6:15] = c, half, (np.eye(3) if R is None else R).ravel()
    return v


def test_reference_cube_is_the_analytic_box_distance():
    half = np.array([0.03, 0.02, 0.04])
    v, f = mr.cube(half)
    pts = [mr.grid_points((9, 7, 11), [-0.05, -0.04, -0.06], [0.0125, 0.0135, 0.012]), np.random.default_rng(11).uniform(-0.1, 0.1, (2000, 3))]
    for p in pts:
        d, w = mr.sdf(v, f, p)
        want = collision._primitive_sdf(_lib.OBSTACLE_BOX, _box_params(half), p)
        e = float(np.abs(d - want).max())
        print(f"cube, {len(p)} points: max |reference - analytic box| = {e:.3e} (gate 1e-15), min |w - 0.5| = {np.abs(w - 0.5).min():.4f}")
        assert e <= 1e-15 and (np.abs(w - 0.5) > 0.49).all() and (d < 0).any() and (d > 0).any()
    R, c = _rotation(5), np.array([0.01, -0.02, 0.005])
    v, f = mr.cube(half, R, c)
    d, w = mr.sdf(v, f, pts[1])
    assert np.abs(d - collision._primitive_sdf(_lib.OBSTACLE_BOX, _box_params(half, R, c), pts[1])).max() <= 1e-15 and (np.abs(w - 0.5) > 0.49).all()


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_reference_icosphere_stays_within_its_inscribed_sphere_of_the_sphere(k):
    r = 0.05
    v, f = mr.icosphere(k, r)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    r_in = float(np.abs(np.einsum("ij,ij->i", n, a) / np.linalg.norm(n, axis=1)).min())  # the nearest face plane to the centre
    p = np.random.default_rng(12).uniform(-0.1, 0.1, (500, 3))
    d, w = mr.sdf(v, f, p)
    e = float(np.abs(d - (np.linalg.norm(p, axis=1) - r)).max())
    print(f"icosphere k = {k}: max |reference - (|p| - r)| = {e:.3e}, r - r_in = {r - r_in:.3e}")
    assert 0 < r - r_in and e <= r - r_in + 1e-15 and (np.abs(w - 0.5) > 0.49).all() and (d < 0).any()


def test_reference_hits_every_region_of_one_triangle_and_its_float32_run_follows():
    c = case("triangle")
    a, ab, ac = mr.records(c["v"], c["f"])
    F = mr.pair_fields(a, ab, ac, c["p"])
    n_designed = 3 * 7 - 1
    assert np.array_equal(F["region"][:14:2, 0], np.arange(1, 8)) and np.array_equal(F["region"][1:14:2, 0], np.arange(1, 8))
    assert np.array_equal(F["region"][14:n_designed, 0], np.arange(1, 7))  # in the plane, outside the triangle: d > 0
    assert len(set(F["region"][n_designed:, 0])) >= 5  # the seeded points spread over the regions too
    assert np.abs(c["d64"][:14:2] - np.hypot(0.01, [np.hypot(0.01, 0.01), np.hypot(0.02, 0.01), 0.01, np.hypot(0.005, 0.02), 0.01, 0.018, 0.0])).max() <= 1e-8
    assert (np.abs(c["w64"]) < 0.5).all() and c["w64"][12] < -0.15 and c["w64"][13] > 0.05  # a fraction of the sphere, signed by the side
    assert not c["w64"][14:n_designed].any()  # in the plane: no solid angle
    assert np.abs(np.abs(c["d32"]) - np.abs(c["d64"])).max() < 1e-7 and np.abs(c["w32"] - c["w64"]).max() < 1e-5
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], c["p"][12]])
    d, w = mr.sdf(c["v"], c["f"], bad)
    assert np.isnan(d[:3]).all() and np.isnan(w[:3]).all() and d[3] == c["d64"][12] and w[3] == c["w64"][12]


# ---- 5. the conditions the GPU tests rely on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POINT_SETS)
def test_point_sets_keep_clear_of_the_sign_gap(name):
    c = case(name)
    d, w = c["d64"], c["w64"]
    assert np.isfinite(d).all() and np.isfinite(w).all() and c["mesh"].n_triangle == len(c["f"])
    close = (np.abs(d) > 0) & (np.abs(d) < SIGN_GAP)
    band = np.abs(w - 0.5) < WIND_BAND
    print(f"{name}: {len(d)} points x {len(c['f'])} triangles, {int((d == 0).sum())} on the surface, {int(close.sum())} within SIGN_GAP, "
          f"{int(band.sum())} within WIND_BAND, {int((d < 0).sum())} inside; float32 run {np.abs(np.abs(c['d32']) - np.abs(d)).max():.3e} from float64")
    assert close.mean() <= 0.01
    if not c["open"]:
        off = np.abs(d) >= SIGN_GAP
        assert (np.abs(w[off] - 0.5) > 0.49).all() and c["mesh"].is_closed and c["mesh"].volume > 0
        assert (d > 0).any() and ((d < 0).any() or name == "tet_2x2x2")  # (the eight corners of one cell are all outside)
    if name == "open2":
        assert len(c["f"]) == 260 and band.mean() <= 0.01 and (d < 0).any() and ((w > 0.05) & (w < 0.95)).any()
    if name in ("cube", "cube_turn"):  # faces, edges and corners of the cube are samples
        assert (d == 0).sum() >= 8 + 12 + 6 and np.abs(np.abs(c["d32"]) - np.abs(d)).max() > 0
    if name.startswith("ico3_"):
        assert len(c["f"]) == int(name.split("_")[1]) and c["open"] == (len(c["f"]) < 1280)
    if name == "multi":
        n, o, h = multi_launch_grid()
        per = _lib.mesh_points_per_launch(len(c["f"]))
        assert 2 * per < n[0] ** 3 <= 3 * per and (n[0] - 1) ** 3 <= 2 * per and n[0] ** 3 <= _lib.SDF_GRID_MAX_SAMPLES
        first = (np.round((c["p"] - o) / h).astype(np.int64) @ np.array([n[1] * n[2], n[2], 1])) // per
        assert set(first) == {0, 1, 2}  # the seeded samples come from all three launches

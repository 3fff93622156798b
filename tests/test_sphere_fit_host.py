"""CPU tests of the sphere fit (include/dexr_sphere_fit.h, collision.fit_spheres / link_grid / SphereSet.from_meshes / from_urdf,
meshio, urdf.parse_collision_geometry): the symbol list against the header, the place and the contents of the fragment, the argument
rules (every one a DEXR_ERR_INVALID / ValueError before any device call), known answers of the yardstick
tests/sphere_fit_reference.py, the tessellators and mesh files, the URDF geometry, and the condition the GPU tests rely on: no body
of theirs has a sample within float32 rounding of the surface."""
import os
import re

import numpy as np
import pytest

import mesh_reference as mr
import sphere_fit_reference as sr
from testutil import REPO
from dex_retargeting_amd import _lib, collision, meshio
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from dex_retargeting_amd.urdf import parse_collision_geometry, parse_urdf

HEADER = os.path.join(REPO, "include", "dexr_sphere_fit.h")
FRAGMENT = os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_sphere_fit.hpp")


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    symbols = _lib.SPHERE_FIT_SYMBOLS
    assert declared == set(symbols) == {"dexr_sphere_fit_workspace_bytes", "dexr_sphere_fit_dev", "dexr_sphere_fit"} and len(symbols) == 3
    for n in dir(_lib):
        if n.endswith("EXPORTS") or (n.endswith("SYMBOLS") and n != "SPHERE_FIT_SYMBOLS"):
            assert not set(symbols) & set(getattr(_lib, n)), n
    lib = _lib.load()
    for name in symbols:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h != "dexr_sphere_fit.h":
            assert not _declared(os.path.join(REPO, "include", h)) & declared, h
    text = open(HEADER).read()
    for macro, value in (("MIN_DIM", _lib.SPHERE_FIT_MIN_DIM), ("MAX_DIM", _lib.SPHERE_FIT_MAX_DIM), ("MAX_BODIES", _lib.SPHERE_FIT_MAX_BODIES),
                         ("CHUNK", _lib.SPHERE_FIT_CHUNK)):
        assert int(re.search(rf"#define DEXR_SPHERE_FIT_{macro} (\d+)", text).group(1)) == value
    assert (_lib.SPHERE_FIT_MIN_DIM, _lib.SPHERE_FIT_MAX_DIM, _lib.SPHERE_FIT_MAX_BODIES) == (2, 64, 64)
    assert '#include "dexr_spheres.h"' in text and not re.search(r"#define\s+DEXR_SPHERE_MAX\b", text)  # the sphere limit is not restated
    for n in ("SphereFit", "fit_spheres", "link_grid"):
        assert n in collision.__all__
    assert hasattr(collision.SphereSet, "from_meshes") and hasattr(collision.SphereSet, "from_urdf")
    for n in ("sphere_fit_workspace_bytes", "sphere_fit_dev", "sphere_fit"):
        assert hasattr(_lib, n)


def test_the_fragment_is_in_its_place_and_stands_alone():
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_sphere_fit.hpp"') == 1 and pose.count("dexr_sphere_fit.hpp") == 1
    assert pose.index('"dexr_resolve_cross.hpp"') < pose.index('"dexr_sphere_fit.hpp"') < pose.index('"dexr_mesh_sdf.hpp"')
    assert pose.rindex('#include "') == pose.index('#include "dexr_mesh_sdf.hpp"')  # the mesh fragment stays the last include
    src = open(FRAGMENT).read()
    assert src.count('#include "') == 1 and '#include "dexr_sphere_fit.h"' in src  # (a fragment: no unit of its own)
    assert "getenv" not in src and "asm" not in src.replace("__restrict__", "") and "atomic" not in src.replace("no atomics", "")
    assert "mesh_" not in src and "DEXR_MESH" not in src and "dexr_mesh" not in src  # nothing of the mesh fragment
    for n in ("DEXR_SPHERE_FIT_MIN_DIM", "DEXR_SPHERE_FIT_MAX_DIM", "DEXR_SPHERE_FIT_MAX_BODIES", "DEXR_SPHERE_FIT_CHUNK", "DEXR_SPHERE_MAX", "__popcll",
              "__shared__"):
        assert n in src
    from dex_retargeting_amd import _build

    assert len(_build.OBJECTS) == 52 and not any("sphere_fit" in row[1] for row in _build.OBJECTS)


# ---- 2. the argument rules of the C entry points -----------------------------------------------------------------------------------------
def _call(entry, n_body=1, dims=((5, 7, 9),), spacing=(0.01,), offset=(0,), k=(4,), min_radius=0.0, inflate=0.0, coverage=1.0, n_values=315,
          values=True, outputs=True, workspace=True, workspace_bytes=None):
    """one call of dexr_sphere_fit_dev ("dev") or dexr_sphere_fit ("host") with fake non-null pointers where a device pointer is
    meant: every rule must be refused before one is followed"""
    lib, C = _lib.load(), _lib.C
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)  # noqa: E731
    d, s, o, kk = arr(dims, np.int32), arr(spacing, np.float64), arr(offset, np.int64), arr(k, np.int32)
    host_v = np.zeros(max(1, n_values), np.float32)
    out = [np.zeros(n_body * 128 if n_body > 0 else 1, np.int32) for _ in range(3)]
    p = _lib._ptr
    common = (n_body, p(d, C.c_int32), p(s, C.c_double), p(o, C.c_int64), p(kk, C.c_int32), min_radius, inflate, coverage, n_values)
    if entry == "host":
        rc = lib.dexr_sphere_fit(*common, p(host_v, C.c_float) if values else None, *(p(a, C.c_int32) if outputs else None for a in out))
    else:
        need = 0 if d is None or n_body < 1 else int(lib.dexr_sphere_fit_workspace_bytes(n_body, p(d, C.c_int32)))
        fake = 4096  # (never followed: the call is refused first)
        rc = lib.dexr_sphere_fit_dev(*common, fake if values else None, *(fake if outputs else None for _ in out), (fake if workspace is True else workspace),
                                     need if workspace_bytes is None else workspace_bytes, None)
    return rc, lib.dexr_last_error().decode()


BAD_CALLS = [
    (dict(n_body=0), "bodies"), (dict(n_body=65), "bodies"), (dict(n_body=-1), "bodies"), (dict(dims=None), "dims is NULL"),
    (dict(dims=((1, 7, 9),)), "dimension 0"), (dict(dims=((5, 65, 9),)), "dimension 1"), (dict(dims=((5, 7, 0),)), "dimension 2"),
    (dict(spacing=None), "NULL"), (dict(offset=None), "NULL"), (dict(k=None), "NULL"),
    (dict(spacing=(0.0,)), "spacing"), (dict(spacing=(-0.01,)), "spacing"), (dict(spacing=(np.nan,)), "spacing"), (dict(spacing=(np.inf,)), "spacing"),
    (dict(offset=(-1,)), "outside"), (dict(offset=(1,)), "outside"), (dict(n_values=314), "outside"), (dict(n_values=-1), "negative"),
    (dict(k=(0,)), "spheres"), (dict(k=(129,)), "spheres"), (dict(k=(-3,)), "spheres"),
    (dict(min_radius=-1e-9), "min_radius"), (dict(min_radius=np.nan), "min_radius"), (dict(min_radius=np.inf), "min_radius"),
    (dict(inflate=-1e-9), "inflate"), (dict(inflate=np.nan), "inflate"), (dict(inflate=np.inf), "inflate"),
    (dict(coverage=-0.01), "coverage"), (dict(coverage=1.01), "coverage"), (dict(coverage=np.nan), "coverage"),
    (dict(values=False), "null"), (dict(outputs=False), "null"),
]


@pytest.mark.parametrize("entry", ["dev", "host"])
def test_c_entry_points_validate_before_they_look_for_a_device(entry):
    for kw, word in BAD_CALLS:
        rc, msg = _call(entry, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    # the second of two bodies is checked like the first
    two = dict(n_body=2, dims=((5, 7, 9), (2, 2, 2)), spacing=(0.01, 0.02), offset=(0, 315), k=(4, 2), n_values=323)
    for kw, word in ((dict(dims=((5, 7, 9), (2, 2, 65))), "body 1"), (dict(spacing=(0.01, 0.0)), "body 1"), (dict(offset=(0, 316)), "body 1"),
                     (dict(k=(4, 200)), "body 1")):
        rc, msg = _call(entry, **{**two, **kw})
        assert rc == -1 and word in msg, (kw, rc, msg)
    if entry == "dev":
        need = _lib.sphere_fit_workspace_bytes([[5, 7, 9]])
        for kw, word in ((dict(workspace=None), "null"), (dict(workspace_bytes=need - 1), "needed"), (dict(workspace=4096 + 8), "aligned")):
            rc, msg = _call(entry, **kw)
            assert rc == -1 and word in msg, (kw, rc, msg)
    else:  # well formed: only a device is missing, if it is
        rc, msg = _call(entry)
        assert rc in (0, -2), (rc, msg)


def test_workspace_bytes_follow_the_dimensions():
    lib, C = _lib.load(), _lib.C
    one = _lib.sphere_fit_workspace_bytes([[64, 64, 64]])
    assert one >= 64 * 64 * 8 + 64 ** 3 * 4 and one % 16 == 0
    small = _lib.sphere_fit_workspace_bytes([[2, 2, 2]])
    assert small < one and _lib.sphere_fit_workspace_bytes([[2, 2, 2]] * 64) > small
    assert _lib.sphere_fit_workspace_bytes([[5, 7, 9], [9, 7, 5]]) == _lib.sphere_fit_workspace_bytes([[9, 7, 5], [5, 7, 9]])
    d = np.array([[2, 2, 65]], np.int32)
    assert lib.dexr_sphere_fit_workspace_bytes(1, d.ctypes.data_as(C.POINTER(C.c_int32))) == 0 and b"dimension" in lib.dexr_last_error()
    assert lib.dexr_sphere_fit_workspace_bytes(0, d.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    assert lib.dexr_sphere_fit_workspace_bytes(1, None) == 0
    with pytest.raises(_lib.DexrError, match="dimension"):
        _lib.sphere_fit_workspace_bytes(d)
    for bad in ([5, 7, 9], [[5, 7]]):
        with pytest.raises(ValueError, match="dims"):
            _lib.sphere_fit_workspace_bytes(bad)
    with pytest.raises(ValueError, match="spacing, offset and k"):
        _lib.sphere_fit([[5, 7, 9]], [0.01, 0.01], [0], [4], 0.0, 0.0, 1.0, np.zeros(315, np.float32))


# ---- 3. the argument rules of the Python fronts -------------------------------------------------------------------------------------------
def _grid(shape=(5, 7, 9), spacing=0.01):
    return collision.SdfGrid(np.ones(shape, np.float32), 0.0, spacing)


@pytest.fixture(scope="module")
def fixture_robot(tmp_path_factory):
    path = sr.write_urdf(str(tmp_path_factory.mktemp("fit_urdf")))
    return RobotWrapper(path), path


def test_python_fronts_raise_before_any_device_call(monkeypatch, fixture_robot):
    touched = []
    for n in ("sphere_fit_dev", "sphere_fit", "sphere_fit_workspace_bytes"):
        monkeypatch.setattr(_lib, n, lambda *a, _n=n, **k: touched.append(_n))
    monkeypatch.setattr(_lib.TriangleMesh, "__init__", lambda self, *a, **k: touched.append("mesh"))
    monkeypatch.setattr(collision.SdfGrid, "from_mesh", classmethod(lambda cls, *a, **k: touched.append("from_mesh")))
    F = collision.fit_spheres
    g = _grid()
    for args, kw, word in (((None, 4), {}, "SdfGrid"), (([], 4), {}, "non-empty"), (([g, "x"], 4), {}, "SdfGrid"), ((g.values, 4), {}, "SdfGrid"),
                           (([g] * 65, 4), {}, "at most 64"), ((g, 0), {}, "max_spheres"), ((g, 129), {}, "max_spheres"), ((g, 2.5), {}, "max_spheres"),
                           (([g, g], [4, 4, 4]), {}, "one per grid"), (([g, g], [4, 0]), {}, "max_spheres"),
                           ((_grid((5, 7, 65)), 4), {}, "at most 64"), ((_grid(spacing=[0.01, 0.01, 0.0125]), 4), {}, "isotropic"),
                           (([g, _grid(spacing=[0.02, 0.01, 0.01])], 4), {}, "grid 1"),
                           ((g, 4), dict(min_radius=-1.0), "min_radius"), ((g, 4), dict(min_radius=np.nan), "min_radius"), ((g, 4), dict(min_radius="a"), "numbers"),
                           ((g, 4), dict(inflate=-1e-9), "inflate"), ((g, 4), dict(inflate=np.inf), "inflate"),
                           ((g, 4), dict(coverage=1.5), "coverage"), ((g, 4), dict(coverage=-0.1), "coverage"), ((g, 4), dict(coverage=np.nan), "coverage")):
        with pytest.raises(ValueError, match=word):
            F(*args, **kw)
    mesh = collision.TriangleMesh(*mr.tetrahedron())
    L = collision.link_grid
    for args, word in ((((mr.tetrahedron()),), "TriangleMesh"), ((mesh, 65), "max_dim"), ((mesh, 2), "max_dim"), ((mesh, 48, -1), "max_dim"),
                       ((mesh, 4.0), "integers"), ((mesh, 8, 4), "max_dim")):
        with pytest.raises(ValueError, match=word):
            L(*args)
    robot, path = fixture_robot
    M = collision.SphereSet.from_meshes
    for args, kw, word in (((robot, {}), {}, "non-empty dict"), ((robot, [mesh]), {}, "dict"), ((robot, {"palm": mr.tetrahedron()}), {}, "TriangleMesh"),
                           ((robot, {"thumb": mesh}), {}, "no link 'thumb'"), ((robot, {"palm": mesh}), dict(spheres_per_link=0), "spheres_per_link"),
                           ((robot, {"palm": mesh}), dict(spheres_per_link=2.0), "spheres_per_link"),
                           ((robot, {"palm": mesh, "tip": mesh}), dict(spheres_per_link={"palm": 4}), "no count"),
                           ((robot, {"palm": mesh, "tip": mesh}), dict(spheres_per_link=65), "at most 128"),
                           ((robot, {"palm": mesh}), dict(coverage=2.0), "coverage"), ((robot, {"palm": mesh}), dict(inflate=-1.0), "inflate"),
                           ((robot, {"palm": mesh}), dict(max_dim=65), "max_dim")):
        with pytest.raises(ValueError, match=word):
            M(*args, **kw)
    U = collision.SphereSet.from_urdf
    with pytest.raises(ValueError, match="at most 128"):
        U(robot, path, spheres_per_link=33)
    bare = os.path.join(os.path.dirname(path), "bare.urdf")
    with open(bare, "w") as f:
        f.write(re.sub(r"<collision>.*?</collision>", "", sr.URDF, flags=re.S))
    with pytest.raises(ValueError, match="no link of the robot has"):
        U(robot, bare)
    assert touched == []


def test_link_grid_makes_the_longest_side_max_dim_samples(monkeypatch):
    calls = []

    def fake(cls, mesh, origin=None, spacing=None, shape=None, **kw):
        calls.append((np.array(origin), float(spacing), tuple(shape), kw))
        return collision.SdfGrid(np.ones(shape, np.float32), origin, spacing)

    monkeypatch.setattr(collision.SdfGrid, "from_mesh", classmethod(fake))
    half = np.array([0.03, 0.011, 0.02])
    mesh = collision.TriangleMesh(*mr.cube(half, None, (0.1, -0.2, 0.05)))
    for max_dim, pad in ((48, 1), (64, 1), (16, 0), (9, 3), (4, 1)):
        g = collision.link_grid(mesh, max_dim, pad)
        o, h, n, kw = calls[-1]
        inner = max_dim - 1 - 2 * pad
        assert kw == {} and n[0] == max_dim == max(n) and h == 0.06 / inner and g.shape == n
        lo, hi = mesh.bounds
        cells = np.array(n) - 1 - 2 * pad  # as few as hold the mesh (a cell more where the extent is a whole number of cells up to rounding)
        assert (cells * h >= hi - lo - 1e-12).all() and (((cells - 1) * h < hi - lo + 1e-12) | (cells == 1)).all() and (cells <= inner).all()
        end = o + (np.array(n) - 1) * h
        assert (o <= lo - pad * h + 1e-12).all() and (end >= hi + pad * h - 1e-12).all()  # the box holds the mesh and its padding
        assert np.allclose((o + end) / 2, [0.1, -0.2, 0.05], rtol=0, atol=1e-12)
    assert collision.link_grid(mesh).shape[0] == 48


# ---- 4. known answers of the yardstick ----------------------------------------------------------------------------------------------------
def test_reference_capsule_takes_three_spheres_on_the_axis_first():
    b = sr.body("capsule17")
    index, gain, count = sr.expected("capsule17", 5)
    ijk = np.stack(np.unravel_index(index, (17, 17, 17)), -1)
    assert gain.tolist() == [81, 81, 81, 24, 24] and count.tolist()[1:] == [81 * 3 + 48, 5]
    assert (ijk[:3, :2] == 8).all() and ijk[:3, 2].tolist() == [3, 8, 13]  # on the axis; of equal gains the lower index first
    assert (ijk[3:, :2] == 8).all()
    centers, radii = sr.spheres_of(b["values"], b["origin"], b["h"], index)
    assert np.allclose(centers[:3], [[0, 0, -0.02], [0, 0, 0.0], [0, 0, 0.02]], rtol=0, atol=1e-12) and np.allclose(radii[:3], 0.01, rtol=0, atol=1e-9)
    interior, m = sr.reach(b["values"], b["h"])
    assert m[8, 8, 8] == 6 and int(interior.sum()) == count[0]  # t = 2.5 cells: 81 samples in the ball
    # every sphere lies inside the capsule: inflate = 0
    assert (sr.capsule_field(centers, 0.01, 0.02) <= -radii + 1e-9).all()


def test_reference_stop_rules_and_candidate_rules():
    index, gain, count = sr.expected("outside", 4)
    assert (index == -1).all() and (gain == 0).all() and count.tolist() == [0, 0, 0]
    full = sr.expected("box_12x10x11", 16)
    assert full[2][2] == 16 and (np.diff(full[1]) <= 0).all() and full[1].sum() == full[2][1] <= full[2][0]
    for cov in (0.1, 0.25, 0.45):
        i, g, c = sr.expected("box_12x10x11", 16, 0.0, 0.0, cov)
        n = int(c[2])
        target = int(np.ceil(cov * c[0]))
        assert 0 < n < 16 and c[1] >= target and c[1] - g[n - 1] < target  # it stopped at the first round that reached the share
        assert np.array_equal(i[:n], full[0][:n]) and (i[n:] == -1).all() and (g[n:] == 0).all()
    assert sr.expected("box_12x10x11", 16, 0.0, 0.0, 0.0)[2].tolist() == [full[2][0], 0, 0]
    # min_radius removes candidates: the slab's interior samples are all shallower than half a cell
    b = sr.body("slab")
    assert sr.expected("slab", 4)[2].tolist() == [36, 4, 4] and sr.expected("slab", 4, 0.005)[2].tolist() == [36, 0, 0]
    deep = float(-b["values"].min())
    assert deep < 0.005
    i, g, c = sr.expected("box_12x10x11", 16, 0.012)
    _, m = sr.reach(sr.body("box_12x10x11")["values"], 0.004, 0.012)
    assert 0 < (m >= 0).sum() < (sr.body("box_12x10x11")["values"] < 0).sum() and (m.ravel()[i[i >= 0]] >= 0).all() and c[2] < 16
    # inflate reaches past the shape: more samples per sphere than interior ones could fill, the gains still count interior ones only
    i1, g1, c1 = sr.expected("box_12x10x11", 16, 0.0, 0.004)
    assert g1[0] > full[1][0] and full[2][1] < c1[1] <= c1[0] == full[2][0]
    # a NaN is not interior and spoils nothing else
    v = sr.body("box_12x10x11")["values"].copy()
    far = np.unravel_index(np.argmax(v), v.shape)
    v[far] = np.nan
    out = sr.fit(v, 0.004, 16)
    assert all(np.array_equal(a, b) for a, b in zip(out, full))
    inner = np.unravel_index(full[0][0], v.shape)
    v[inner] = np.nan
    out = sr.fit(v, 0.004, 16)
    assert out[2][0] == full[2][0] - 1 and out[0][0] != full[0][0]
    # a reach beyond every grid saturates instead of overflowing
    _, m = sr.reach(np.full((2, 2, 2), -3e38, np.float32), 1e-300)
    assert (m == sr.M_MAX).all()


@pytest.mark.parametrize("name", sr.BODIES)
def test_bodies_keep_clear_of_the_surface(name):
    b = sr.body(name)
    v = b["values"]
    print(f"{name}: {v.shape}, {int((v < 0).sum())} interior samples, the nearest sample {b['clear_of_zero']:.3e} from the surface")
    assert b["clear_of_zero"] > 1e-5 > 100 * np.spacing(np.float32(np.abs(v).max()))  # far above float32 rounding of any sample
    assert v.dtype == np.float32 and not v.flags.writeable and min(v.shape) >= _lib.SPHERE_FIT_MIN_DIM and max(v.shape) <= _lib.SPHERE_FIT_MAX_DIM
    if name.startswith("cube_9x9x"):
        assert (v[4, 4, :] < 0).all()  # the body runs through both faces of the grid along z
    if name == "box_2x2x2":
        assert (v < 0).all()


# ---- 5. tessellators and mesh files ---------------------------------------------------------------------------------------------------------
def test_tessellators_are_closed_with_the_volumes_of_their_polygons():
    M = collision.TriangleMesh
    box = M(*meshio.box_mesh((0.08, 0.06, 0.02)))
    assert box.is_closed and box.n_triangle == 12 and abs(box.volume - 0.08 * 0.06 * 0.02) <= 1e-18
    assert np.array_equal(box.bounds, [[-0.04, -0.03, -0.01], [0.04, 0.03, 0.01]])
    r, length = 0.01, 0.04
    for n in (3, 8, 32, 64):
        cyl = M(*meshio.cylinder_mesh(r, length, n))
        prism = 0.5 * n * r * r * np.sin(2 * np.pi / n) * length  # the regular n-gon inscribed in the circle
        assert cyl.is_closed and cyl.n_triangle == 4 * n and abs(cyl.volume - prism) <= 1e-15 and cyl.volume < np.pi * r * r * length
        assert np.abs(np.linalg.norm(cyl.vertices[:2 * n, :2], axis=1) - r).max() <= 1e-17 and np.abs(cyl.vertices[:, 2]).max() == length / 2
    assert M(*meshio.cylinder_mesh(r, length)).n_triangle == 128 and M(*meshio.cylinder_mesh(r, length)).volume > 0.99 * np.pi * r * r * length
    with pytest.raises(ValueError, match="segments"):
        meshio.cylinder_mesh(r, length, 2)
    ball = 4.0 / 3.0 * np.pi * 0.011 ** 3
    last = 0.0
    for level in range(4):
        s = M(*meshio.sphere_mesh(0.011, level))
        a, b, c = (s.vertices[s.faces[:, k]] for k in range(3))
        nrm = np.cross(b - a, c - a)
        r_in = float((np.einsum("ij,ij->i", nrm, a) / np.linalg.norm(nrm, axis=1)).min())  # the nearest face plane: that ball lies inside
        assert s.is_closed and s.n_triangle == 20 * 4 ** level and 0 < r_in < 0.011
        assert max(last, ball * (r_in / 0.011) ** 3) < s.volume < ball  # between the two balls, growing with the level
        assert np.abs(np.linalg.norm(s.vertices, axis=1) - 0.011).max() <= 1e-17
        last = s.volume
    assert M(*meshio.sphere_mesh(0.011)).n_triangle == 320 and M(*meshio.sphere_mesh(0.011)).volume == M(*meshio.sphere_mesh(0.011, 2)).volume


@pytest.mark.parametrize("solid", ["tetrahedron", "cube"])
def test_mesh_files_round_trip_to_closed_meshes(solid, tmp_path):
    v, f = mr.tetrahedron(0.05) if solid == "tetrahedron" else mr.cube((0.03, 0.02, 0.04), None, (0.01, -0.02, 0.005))
    want = collision.TriangleMesh(v, f)
    v32 = v.astype(np.float32).astype(np.float64)  # STL holds float32
    for name, write in (("b.stl", lambda p: meshio.save_stl(p, v, f, binary=True)), ("a.stl", lambda p: meshio.save_stl(p, v32, f, binary=False)),
                        ("m.obj", lambda p: meshio.save_obj(p, v, f))):
        path = str(tmp_path / name)
        write(path)
        got = collision.TriangleMesh(*meshio.load_mesh(path))
        assert got.is_closed and got.n_vertex == want.n_vertex and got.n_triangle == want.n_triangle
        ref = v if name.endswith(".obj") else v32
        assert np.array_equal(got.vertices[got.faces], ref[f])  # the same triangles, corner for corner, in order
        assert abs(got.volume - want.volume) <= 1e-6 * want.volume and got.volume > 0
    # OBJ: polygons are fanned, negative indices count from the end, texture / normal indices are skipped
    quad = str(tmp_path / "quads.obj")
    with open(quad, "w") as fh:
        fh.write("# a cube of quads\no cube\n")
        corners = [[(k >> i & 1) * 0.02 - 0.01 for i in range(3)] for k in range(8)]
        fh.write("".join(f"v {c[0]} {c[1]} {c[2]}\n" for c in corners) + "vn 0 0 1\nvt 0 0\n")
        for a, b, c, d in ((0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3)):
            fh.write(f"f {a + 1}/1/1 {b + 1}/1/1 {c + 1}/1/1 {d + 1}/1/1\n")
        fh.write("f -8 -6 -5 -7\nf 5//1 6//1 8//1 7//1\n")
    cube = collision.TriangleMesh(*meshio.load_mesh(quad))
    assert cube.is_closed and cube.n_triangle == 12 and abs(cube.volume - 0.02 ** 3) <= 1e-18
    for bad in ("mesh.dae", "mesh.ply", "mesh"):
        with pytest.raises(ValueError, match=re.escape(bad)):
            meshio.load_mesh(str(tmp_path / bad))
    broken = str(tmp_path / "broken.stl")
    with open(broken, "wb") as fh:
        fh.write(b"\0" * 80 + b"\x05\0\0\0" + b"\0" * 20)
    with pytest.raises(ValueError, match="broken.stl"):
        meshio.load_mesh(broken)


# ---- 6. the URDF's geometry ----------------------------------------------------------------------------------------------------------------
def test_parse_collision_geometry_reads_all_four_kinds(fixture_robot):
    robot, path = fixture_robot
    geo = parse_collision_geometry(path)
    assert list(geo) == ["palm", "proximal", "distal", "tip", "bare"] and geo["bare"] == [] and [len(geo[n]) for n in sr.URDF_LINKS] == [2, 1, 1, 1]
    (k0, p0, o0), (k1, p1, o1) = geo["palm"]
    assert k0 == "box" and np.array_equal(p0, [0.08, 0.06, 0.02]) and np.array_equal(o0[:3, 3], [0, 0, 0.01]) and np.array_equal(o0[:3, :3], np.eye(3))
    assert k1 == "cylinder" and p1 == (0.01, 0.04) and np.array_equal(o1[:3, 3], [0.05, 0, 0.01])
    assert np.allclose(o1[:3, :3], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], rtol=0, atol=1e-15)  # a quarter turn about y: the axis along x
    assert geo["proximal"][0][:2] == ("cylinder", (0.008, 0.04)) and np.array_equal(geo["proximal"][0][2][:3, 3], [0, 0, 0.02])
    kd, pd, od = geo["distal"][0]
    assert kd == "sphere" and pd == (0.011,) and abs(od[1, 2] + np.sin(0.3)) <= 1e-16
    kt, (fn, scale), ot = geo["tip"][0]
    assert kt == "mesh" and fn == os.path.join(os.path.dirname(path), "meshes", "tip.stl") and os.path.exists(fn) and np.array_equal(scale, [0.5, 0.5, 1.0])
    # package:// and plain relative names resolve against the URDF's directory, a missing scale is 1 1 1
    other = os.path.join(os.path.dirname(path), "other.urdf")
    with open(other, "w") as f:
        f.write('<robot name="r"><link name="a"><collision><geometry><mesh filename="package://pkg/meshes/a.obj"/></geometry></collision>'
                '<collision><geometry><mesh filename="/abs/b.stl" scale="2 2 2"/></geometry></collision></link>'
                '<link name="b"><collision><geometry/></collision></link></robot>')
    with pytest.raises(ValueError, match="link b"):
        parse_collision_geometry(other)
    with open(other, "w") as f:
        f.write('<robot name="r"><link name="a"><collision><geometry><mesh filename="package://pkg/meshes/a.obj"/></geometry></collision>'
                '<collision><geometry><mesh filename="/abs/b.stl" scale="2 2 2"/></geometry></collision></link></robot>')
    (_, (fa, sa), oa), (_, (fb, sb), _) = parse_collision_geometry(other)["a"]
    assert fa == os.path.join(os.path.dirname(path), "pkg", "meshes", "a.obj") and np.array_equal(sa, [1, 1, 1]) and np.array_equal(oa, np.eye(4))
    assert fb == "/abs/b.stl" and np.array_equal(sb, [2, 2, 2])
    # parse_urdf is untouched by the geometry
    assert parse_urdf(path).links == ["palm", "proximal", "distal", "tip", "bare"] and robot.dof == 3
    # the link meshes: elements transformed by their origins and concatenated
    palm = collision.TriangleMesh(*meshio.link_mesh(geo["palm"]))
    assert palm.n_triangle == 12 + 128 and np.allclose(palm.bounds, [[-0.04, -0.03, 0.0], [0.07, 0.03, 0.02]], rtol=0, atol=1e-15)
    assert not palm.is_closed or palm.volume > 0  # two closed solids: every edge still has two faces
    tip = collision.TriangleMesh(*meshio.link_mesh(geo["tip"]))
    t = 0.03 / np.sqrt(3.0)
    assert tip.is_closed and tip.volume > 0 and np.allclose(tip.bounds, [[-t / 2, -t / 2, 0.01 - t], [t / 2, t / 2, 0.01 + t]], rtol=0, atol=1e-8)
    mirrored = collision.TriangleMesh(*meshio.link_mesh([("mesh", (fn, np.array([-1.0, 1.0, 1.0])), np.eye(4))]))
    assert mirrored.is_closed and mirrored.volume > 0  # a mirror turns the triangles over, the normals stay outwards
    with pytest.raises(ValueError, match="no mesh"):
        meshio.link_mesh(geo["bare"])
    with pytest.raises(ValueError, match="unknown"):
        meshio.link_mesh([("capsule", (0.1, 0.2), np.eye(4))])

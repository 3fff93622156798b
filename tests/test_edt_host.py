"""CPU tests of the distance transform's interface (include/dexr_distance_transform.h, include/dexr_sdf_grid_dev.h,
collision.DeviceSdfGrid / SdfGrid.from_points / SdfGrid.from_occupancy): the symbol lists against the headers and the built library,
every argument rule raised with no device present, the raw ABI's refusals before any HIP call, the yardstick's own known answers
(tests/edt_reference.py; against scipy's distance_transform_edt where scipy is importable), and the inputs of the geometric GPU test
proven on the yardstick.  The grids and clouds of tests/test_gpu_edt.py are made here and shared from here."""
import functools
import math
import os
import re

import numpy as np
import pytest

import edt_reference as er
from dex_retargeting_amd import _lib, collision

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dexr_distance_transform.h")
GRID_HEADER = os.path.join(REPO, "include", "dexr_sdf_grid_dev.h")
FRAGMENT = os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_distance_transform.hpp")

# every shape at which a pass takes another path: the smallest, odd sizes, a z row and a strided row past one wave, the longest row in z
# and in x (the tile at the LDS limit), several blocks
GRIDS = [(2, 2, 2), (5, 7, 9), (3, 4, 65), (65, 3, 4), (3, 65, 4), (2, 2, 1024), (1024, 2, 2), (33, 17, 9)]
CLOUDS = ["empty", "one", "seeded", "one_voxel", "corners"]
H, ORIGIN = 0.01, (-0.1, 0.05, 0.2)
MARGIN_U = 1e-3  # u + 0.5 of every seeded point is at least this far from an integer


def seeded_points(n, count, seed, origin=ORIGIN, h=H):
    """count points, float32: voxel indices -1 .. n_a (the outermost ones are dropped) plus an offset in +-0.49, so that no
    voxelisation hinges on a rounding (checked)"""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(-1, k + 1, count) for k in n], 1)
    u = idx + rng.uniform(-0.49, 0.49, (count, 3))
    p = (np.asarray(origin) + u * h).astype(np.float32)
    _, _, ur = er.voxel_indices(p, n, origin, h)
    t = ur + 0.5
    assert np.abs(t - np.round(t)).min() >= MARGIN_U
    return p


@functools.lru_cache(maxsize=None)
def cloud(kind, n):
    """points (N, 3) float32 of one of CLOUDS on a grid of n, read-only"""
    n = tuple(n)
    centre = lambda idx: (np.asarray(ORIGIN) + np.asarray(idx, dtype=np.float64) * H)  # noqa: E731
    if kind == "empty":
        p = np.zeros((0, 3), np.float32)
    elif kind == "one":
        p = centre([n[0] - 1, 0, n[2] // 2])[None].astype(np.float32)
    elif kind == "seeded":
        p = seeded_points(n, 513, 7 + sum(n))
    elif kind == "one_voxel":  # 40 points, all in the voxel (1, 1, n_z - 1)
        rng = np.random.default_rng(11)
        p = (centre([1, 1, n[2] - 1]) + rng.uniform(-0.4, 0.4, (40, 3)) * H).astype(np.float32)
    else:  # one occupied voxel per corner
        p = np.array([centre([a, b, c]) for a in (0, n[0] - 1) for b in (0, n[1] - 1) for c in (0, n[2] - 1)]).astype(np.float32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def cloud_reference(kind, n, min_points=1, radius=0.0):
    """the yardstick on cloud(kind, n): (values, d2, count), computed once and shared, read-only"""
    out = er.from_points(cloud(kind, n), n, ORIGIN, H, min_points, radius)
    for a in out:
        a.setflags(write=False)
    return out


def exact_cloud(n):
    """points that sit exactly on sample positions: origin 0, h = 2^-6, points k h -- every step of the voxelisation is exact"""
    rng = np.random.default_rng(3)
    k = np.stack([rng.integers(0, m, 200) for m in n], 1)
    p = (k * 2.0 ** -6).astype(np.float32)
    assert np.array_equal(p.astype(np.float64), k * 2.0 ** -6)
    return p, k


def duplicate_cloud(n):
    """voxels with one, two and three points: min_points = 2 keeps the latter two"""
    rng = np.random.default_rng(5)
    flat = rng.choice(int(np.prod(n)), 30, replace=False)
    idx = np.stack(np.unravel_index(flat, n), 1)
    reps = np.arange(30) % 3 + 1
    vox = np.repeat(idx, reps, 0)
    p = (np.asarray(ORIGIN) + (vox + rng.uniform(-0.3, 0.3, vox.shape)) * H).astype(np.float32)
    return p, idx, reps


# the geometric test: a lattice of spacing BOX_S on the six faces of a box, a 17^3 grid around it
BOX_C, BOX_E, BOX_S, BOX_N, BOX_H = np.array([0.3, -0.2, 0.1]), np.array([0.03, 0.04, 0.02]), 0.01, (17, 17, 17), 0.01
BOX_O = BOX_C - 8 * BOX_H + BOX_H * np.array([0.3, -0.2, 0.4])  # (the lattice does not sit on the voxel centres)


def box_cloud():
    ax = [np.arange(-int(round(e / BOX_S)), int(round(e / BOX_S)) + 1) * BOX_S for e in BOX_E]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    on_face = (np.abs(np.abs(g) - BOX_E) < 1e-12).any(1)
    return (BOX_C + g[on_face]).astype(np.float32)


def box_bound():
    """|v_cloud - v_box| at a sample outside the box.  v_cloud (radius 0) is the distance to the centre of a voxel that holds a point,
    a centre at most h sqrt(3) / 2 from its point, so |v_cloud - d(nearest point)| <= h sqrt(3) / 2; every point of the surface has a
    lattice point within s / sqrt(2) (half the diagonal of a lattice cell), so d(box) <= d(nearest point) <= d(box) + s / sqrt(2)."""
    return BOX_H * math.sqrt(3) / 2 + BOX_S / math.sqrt(2) + 1e-6


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbol_lists_are_the_headers_and_the_library_exports_them():
    assert _declared(HEADER) == set(_lib.EDT_SYMBOLS) and len(_lib.EDT_SYMBOLS) == 5 == len(set(_lib.EDT_SYMBOLS))
    assert _declared(GRID_HEADER) == set(_lib.SDF_GRID_DEV_SYMBOLS) and len(_lib.SDF_GRID_DEV_SYMBOLS) == 3 == len(set(_lib.SDF_GRID_DEV_SYMBOLS))
    new = set(_lib.EDT_SYMBOLS) | set(_lib.SDF_GRID_DEV_SYMBOLS)
    assert len(new) == 8
    for name in dir(_lib):
        if name.endswith(("EXPORTS", "SYMBOLS")) and name not in ("EDT_SYMBOLS", "SDF_GRID_DEV_SYMBOLS"):
            assert not new & set(getattr(_lib, name)), name
    lib = _lib.load()
    for name in new:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h not in ("dexr_distance_transform.h", "dexr_sdf_grid_dev.h"):
            assert not _declared(os.path.join(REPO, "include", h)) & new, h
    text = open(HEADER).read()
    assert 1 << int(re.search(r"#define DEXR_EDT_NONE \(1 << (\d+)\)", text).group(1)) == _lib.EDT_NONE == er.NONE
    assert 1 << int(re.search(r"#define DEXR_EDT_MAX_POINTS \(1 << (\d+)\)", text).group(1)) == _lib.EDT_MAX_POINTS
    assert int(re.search(r"#define DEXR_EDT_TILE_BYTES (\d+)", text).group(1)) == _lib.EDT_TILE_BYTES <= 65536
    assert _lib.EDT_NONE > 3 * 1023 ** 2 and _lib.EDT_NONE + 3 * 1023 ** 2 < 2 ** 31  # above every distance, and three passes cannot overflow
    assert not re.search(r"#define DEXR_SDF_GRID", text) and "DEXR_SDF_GRID_MAX_SAMPLES" in text  # the grid limits are not restated
    assert "DeviceSdfGrid" in collision.__all__ and issubclass(collision.DeviceSdfGrid, collision.SdfGrid)
    assert issubclass(_lib.DeviceSdfGrid, _lib.SdfGrid)
    for m in ("from_points", "from_occupancy"):
        assert hasattr(collision.SdfGrid, m) and hasattr(collision.DeviceSdfGrid, m)
    for m in ("empty", "update_from_points", "update_from_occupancy", "to_host"):
        assert hasattr(collision.DeviceSdfGrid, m)


def test_the_fragment_is_included_once_before_the_mesh_fragment_and_atomics_stay_in_the_voxelisation():
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_distance_transform.hpp"') == 1 and pose.count("dexr_distance_transform.hpp") == 1
    assert pose.index('"dexr_sdf_grid.hpp"') < pose.index('"dexr_distance_transform.hpp"') < pose.index('"dexr_mesh_sdf.hpp"')
    src = open(FRAGMENT).read()
    assert "getenv" not in src and "asm" not in src.replace("__restrict__", "")
    assert src.count('#include "') == 1 and '#include "dexr_distance_transform.h"' in src  # (a fragment: no unit of its own)
    code = re.sub(r"//[^\n]*", "", src)
    assert code.count("atomic") == 1 and "atomicAdd(slot, 1)" in code  # the integer count, nowhere else
    assert "__shfl" not in code and "__reduce" not in code  # no reduction across lanes
    for name in ("DEXR_EDT_NONE", "DEXR_EDT_TILE_BYTES", "DEXR_EDT_MAX_POINTS", "DEXR_SDF_GRID_MAX_DIM", "DEXR_SDF_GRID_MAX_SAMPLES"):
        assert name in code  # the code reads the named constants, not numbers of its own


# ---- 2. every argument rule, with no device ------------------------------------------------------------------------------------------
def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    touched = []
    monkeypatch.setattr(_lib.DeviceSdfGrid, "__init__", lambda self, *a, **k: touched.append("create"))
    for f in ("edt_points_dev", "edt_occupancy_dev", "edt_workspace_bytes"):
        monkeypatch.setattr(_lib, f, lambda *a, _f=f, **k: touched.append(_f))
    D, G = collision.DeviceSdfGrid, collision.SdfGrid
    pts = torch.zeros((5, 3), dtype=torch.float32)  # CPU tensors: right in everything but the device
    occ = torch.zeros((3, 4, 5), dtype=torch.uint8)

    def points_raise(match, p=pts, origin=0.0, spacing=0.01, shape=(3, 4, 5), **kw):
        for front in (D.from_points, G.from_points):
            with pytest.raises(ValueError, match=match):
                front(p, origin, spacing, shape, **kw)

    def occ_raise(match, o=occ, origin=0.0, spacing=0.01, **kw):
        for front in (D.from_occupancy, G.from_occupancy):
            with pytest.raises(ValueError, match=match):
                front(o, origin, spacing, **kw)

    points_raise("CUDA")  # everything right but the device: the last rule
    occ_raise("CUDA")
    occ_raise("CUDA", signed=False, radius=0.0)
    # the grid
    points_raise("ONE spacing", spacing=(0.01, 0.01, 0.02))
    occ_raise("ONE spacing", spacing=(0.01, 0.02, 0.01))
    for bad in (0.0, -0.01, float("nan"), float("inf"), 1e-320):
        points_raise("spacing", spacing=bad)
        occ_raise("spacing", spacing=bad)
    for bad in ((1, 4, 5), (3, 4, 1025), (512, 512, 512), (3, 4), (3.0, 4.0, 5.0)):
        points_raise("shape|dimension", shape=bad)
    occ_raise("dimension", o=torch.zeros((1, 4, 5), dtype=torch.uint8))
    for bad in (float("nan"), (0.0, float("inf"), 0.0)):
        points_raise("origin", origin=bad)
        occ_raise("origin", origin=bad)
    points_raise("scalar or have shape", origin=(0.0, 0.0))
    # the scalars
    for bad in (0, -1, 1.5, True, None):
        points_raise("min_points", min_points=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        points_raise("radius", radius=bad)
        occ_raise("radius", signed=False, radius=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        points_raise("max_distance", max_distance=bad)
        occ_raise("max_distance", max_distance=bad)
    points_raise("numbers", radius="thick")
    occ_raise("no radius", signed=True, radius=0.005)
    points_raise("signed=True", signed=True)
    # the tensors
    points_raise("torch tensor", p=np.zeros((5, 3), np.float32))
    points_raise("float32", p=pts.double())
    points_raise(r"\(N, 3\)", p=torch.zeros((5, 4)))
    points_raise(r"\(N, 3\)", p=torch.zeros((15,)))
    points_raise("contiguous", p=torch.zeros((5, 6))[:, ::2])
    occ_raise("torch tensor", o=np.zeros((3, 4, 5), np.uint8))
    occ_raise("uint8", o=occ.bool())
    occ_raise("uint8", o=occ.float())
    occ_raise(r"\(nx, ny, nz\)", o=torch.zeros((12, 5), dtype=torch.uint8))
    occ_raise("contiguous", o=torch.zeros((3, 4, 10), dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError, match="ONE spacing"):
        D.empty((3, 4, 5), 0.0, (0.01, 0.02, 0.03))
    with pytest.raises(ValueError, match="dimension"):
        D.empty((3, 4, 1), 0.0, 0.01)
    assert touched == []
    # an existing device grid: the updates apply the same rules, and the shape of the map is the grid's
    g = D.__new__(D)
    g._shape, g._h, g._device, g._workspace = (3, 4, 5), 0.01, 0, None
    g.origin, g.spacing = np.zeros(3), np.full(3, 0.01)
    for kw, match in ((dict(min_points=0), "min_points"), (dict(radius=-1.0), "radius"), (dict(max_distance=0.0), "max_distance"),
                      (dict(signed=True), "signed=True"), ({}, "CUDA")):
        with pytest.raises(ValueError, match=match):
            g.update_from_points(pts, **kw)
    with pytest.raises(ValueError, match=r"\(3, 4, 5\)"):
        g.update_from_occupancy(torch.zeros((3, 4, 6), dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):
        g.update_from_occupancy(occ)
    assert touched == []
    # what a device grid is: an SdfGrid by type, itself by identity, bound to its device, without host samples
    assert isinstance(g, collision.SdfGrid) and g.shape == (3, 4, 5) and g == g and g != D.__new__(D) and hash(g) == object.__hash__(g)
    g._grid = object()
    assert g.device_grid(0) is g._grid
    with pytest.raises(ValueError, match=r"cuda:0.*cuda:1"):
        g.device_grid(1)
    with pytest.raises(AttributeError, match="to_host"):
        g.values
    with pytest.raises(ValueError, match="to_host"):
        collision.fit_spheres(g, 4)
    with pytest.raises(ValueError, match="to_host"):
        collision.fit_spheres([g], 4)
    with pytest.raises(ValueError, match="TriangleMesh"):
        collision.link_grid(g)
    assert "cuda:0" in repr(g) and touched == []


def test_raw_abi_refuses_bad_arguments_before_any_hip_call():
    lib, C = _lib.load(), _lib.C
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    n = np.array([3, 4, 5], np.int32)
    o = np.zeros(3)
    fake = C.c_void_p(4096)  # a non-null, 16-byte aligned address that a refused call never reads
    big = 1 << 20

    def points(N=1, n=n, o=o, h=0.01, mp=1, r=0.0, md=1.0, pts=fake, v=fake, ws=fake, nb=big):
        return lib.dexr_edt_points_dev(pts, N, None if n is None else n.ctypes.data_as(i32p), None if o is None else o.ctypes.data_as(f64p), h, mp, r,
                                       md, v, None, None, ws, nb, None)

    def occupancy(n=n, h=0.01, s=0, r=0.0, md=1.0, oc=fake, v=fake, ws=fake, nb=big):
        return lib.dexr_edt_occupancy_dev(oc, None if n is None else n.ctypes.data_as(i32p), h, s, r, md, v, None, ws, nb, None)

    bad_n = [None, np.array([1, 4, 5], np.int32), np.array([3, 1025, 5], np.int32), np.array([512, 512, 512], np.int32)]
    cases = [points(n=b) for b in bad_n] + [occupancy(n=b) for b in bad_n]
    cases += [points(N=-1), points(N=_lib.EDT_MAX_POINTS + 1), points(pts=None), points(o=None), points(o=np.array([0.0, np.nan, 0.0]))]
    cases += [f(h=b) for f in (points, occupancy) for b in (0.0, -1.0, float("nan"), float("inf"), 1e-320)]
    cases += [points(mp=0), points(mp=-3), occupancy(s=1, r=0.01)]
    cases += [f(r=b) for f in (points, occupancy) for b in (-1e-9, float("nan"), float("inf"))]
    cases += [f(md=b) for f in (points, occupancy) for b in (0.0, -1.0, float("nan"), float("inf"))]
    cases += [f(v=None) for f in (points, occupancy)] + [f(ws=None) for f in (points, occupancy)] + [occupancy(oc=None)]
    cases += [f(ws=C.c_void_p(4100)) for f in (points, occupancy)] + [f(nb=3 * 4 * 5 * 12 - 1) for f in (points, occupancy)]
    assert cases and all(rc == -1 for rc in cases), cases  # DEXR_ERR_INVALID
    assert b"workspace" in lib.dexr_last_error()
    # the host twins and the grid entries share the rules
    assert lib.dexr_edt_points(None, 1, n.ctypes.data_as(i32p), o.ctypes.data_as(f64p), 0.01, 1, 0.0, 1.0, None, None, None) == -1
    assert lib.dexr_edt_occupancy(None, n.ctypes.data_as(i32p), 0.01, 0, 0.0, 1.0, None, None) == -1
    out = C.c_void_p()
    h3 = np.full(3, 0.01)
    for nn, oo, hh in ((bad_n[1], o, h3), (n, np.array([0.0, np.inf, 0.0]), h3), (n, o, np.array([0.01, 0.0, 0.01]))):
        assert lib.dexr_sdf_grid_create_dev(nn.ctypes.data_as(i32p), oo.ctypes.data_as(f64p), hh.ctypes.data_as(f64p), None, None, C.byref(out)) == -1
        assert not out.value
    assert lib.dexr_sdf_grid_create_dev(n.ctypes.data_as(i32p), o.ctypes.data_as(f64p), h3.ctypes.data_as(f64p), None, None, None) == -1
    assert not lib.dexr_sdf_grid_values_dev(None) and lib.dexr_sdf_grid_download(None, None, None) == -1
    # the workspace size: three int32 per sample
    assert _lib.edt_workspace_bytes((3, 4, 5)) == 3 * 4 * 5 * 12 and _lib.edt_workspace_bytes((256, 256, 256)) == 12 << 24
    nb = C.c_size_t(7)
    assert lib.dexr_edt_workspace_bytes(bad_n[2].ctypes.data_as(i32p), C.byref(nb)) == -1 and nb.value == 0


# ---- 3. the yardstick's own known answers ----------------------------------------------------------------------------------------------
def test_reference_known_answers():
    n = (4, 5, 6)
    occ = np.zeros(n, bool)
    occ[1, 2, 3] = True
    ix, iy, iz = np.meshgrid(*[np.arange(k) for k in n], indexing="ij")
    want = (ix - 1) ** 2 + (iy - 2) ** 2 + (iz - 3) ** 2
    assert np.array_equal(er.d2_brute(occ), want) and er.d2_brute(occ).dtype == np.int32
    assert not er.d2_brute(np.ones(n, bool)).any() and (er.d2_brute(np.zeros(n, bool)) == er.NONE).all()
    v = er.unsigned_values(want, 0.5, 0.25, 1.0)
    assert v.dtype == np.float32 and v[1, 2, 3] == -0.25 and v[1, 2, 4] == 0.25 and v[3, 4, 5] == 0.75  # the clamp at 1.0, minus 0.25
    assert (er.unsigned_values(er.d2_brute(np.zeros(n, bool)), 0.5, 0.25, 3.0) == 2.75).all()
    s, to_occ, to_free = er.signed_values(occ, 0.5, 10.0)
    assert s[1, 2, 3] == -0.25 and s[1, 2, 4] == 0.25 and s[1, 1, 3] == 0.25 and to_free[1, 2, 3] == 1 and np.array_equal(to_occ, want)
    assert (er.signed_values(np.zeros(n, bool), 0.5, 10.0)[0] == 9.75).all() and (er.signed_values(np.ones(n, bool), 0.5, 10.0)[0] == -9.75).all()
    # the voxelisation: halves round up, the faces of the box, what is dropped
    p = np.array([[0.5, 0.0, 0.0], [0.4999, 0.0, 0.0], [-0.5, 0.0, 0.0], [-0.5001, 0.0, 0.0], [3.4999, 4.4, 5.4], [3.5, 0, 0], [np.nan, 0, 0],
                  [0, np.inf, 0], [0, 0, -np.inf], [1.0, 1.0, 1.0], [1.2, 0.8, 1.1]], np.float32)
    c = er.voxelise(p, n, (0.0, 0.0, 0.0), 1.0)
    assert c.dtype == np.int32 and c.sum() == 6 and c[1, 0, 0] == 1 and c[0, 0, 0] == 2 and c[3, 4, 5] == 1 and c[1, 1, 1] == 2
    _, d2, count = er.from_points(p, n, (0.0, 0.0, 0.0), 1.0, min_points=2)
    assert np.array_equal(count, c) and d2[0, 0, 0] == 0 and d2[1, 1, 1] == 0 and d2[1, 0, 0] == 1 and d2[3, 4, 5] == 4 + 9 + 16
    assert np.array_equal(er.ulp_distance(np.float32([1.0, -1.0, 0.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0, 1e-45])),
                          [1, 0, 0, 1])


@pytest.mark.parametrize("n", [(5, 7, 9), (33, 17, 9)])
def test_reference_against_scipy(n):
    ndi = pytest.importorskip("scipy.ndimage")
    occ = np.random.default_rng(sum(n)).uniform(size=n) < 0.02
    assert occ.any()
    d = ndi.distance_transform_edt(~occ)  # the distance of every nonzero (free) sample to the nearest zero (occupied) one
    assert np.array_equal(er.d2_brute(occ), np.rint(d * d).astype(np.int32)) and np.abs(d * d - np.rint(d * d)).max() < 1e-6


def test_shared_clouds_are_what_their_names_say():
    for n in GRIDS:
        _, d2, count = cloud_reference("corners", n)
        assert (count > 0).sum() == 8 and count.sum() == 8 and d2.max() < er.NONE
        assert cloud_reference("one_voxel", n)[2][1, 1, n[2] - 1] == 40 and cloud_reference("one", n)[2].sum() == 1
        assert (cloud_reference("empty", n)[1] == er.NONE).all()
        c = cloud_reference("seeded", n)[2]
        assert 0 < c.sum() < 513 and c.max() >= 1  # some points are outside and dropped
    p, idx, reps = duplicate_cloud((5, 7, 9))
    c = er.voxelise(p, (5, 7, 9), ORIGIN, H)
    assert np.array_equal(c[tuple(idx.T)], reps) and c.sum() == reps.sum()
    p, k = exact_cloud((5, 7, 9))
    assert np.array_equal(er.voxel_indices(p, (5, 7, 9), (0, 0, 0), 2.0 ** -6)[0], k)


def test_the_geometric_inputs_satisfy_their_bound_on_the_yardstick():
    p = box_cloud()
    v, d2, count = er.from_points(p, BOX_N, BOX_O, BOX_H, radius=0.0)
    assert count.sum() == len(p) and len(p) > 100  # every point lies in the grid: none is dropped
    box = collision.SdfGrid.from_obstacles(collision.ObstacleSet.boxes(BOX_C[None], BOX_E[None]), BOX_O, BOX_H, BOX_N)
    out = box.values > 0
    err = np.abs(v.astype(np.float64) - box.values)[out]
    print(f"outside samples {int(out.sum())}, max |v_cloud - v_box| = {err.max():.5f}, bound {box_bound():.5f}")
    assert out.sum() > 3000 and err.max() <= box_bound()
    assert v.max() < er.default_max_distance(BOX_N, BOX_H)  # the clamp plays no part

"""CPU tests of the signed-distance-grid collision's interface (include/dexr_sdf_grid.h, dex_retargeting_amd/collision.py): the
export list against the header, the place of the fragment in dexr_pose.hip, dexr_sdf_grid_create's validation (every malformed
input DEXR_ERR_INVALID before a device is looked for), collision.SdfGrid and the argument rules of the torch front (every one a
ValueError before any device call), the yardstick tests/grid_reference.py against central differences of its own float64 values
and against a closed form, SdfGrid.from_obstacles against tests/obstacle_reference.py, and the behaviour of the yardstick on the
inputs of tests/test_gpu_grid.py, so that the inputs are proven before a GPU sees them.

INPUTS (shared with the GPU tests).  obstacle_inputs(name) of tests/test_obstacle_host.py as they are: the eight fixture robots,
two spheres of radius 0.010 per link, B = 33, a seeded obstacle pose per frame (POSE_SEED = 64), every fourth frame 2 m away,
margin 0.010.  Two grids:
  GRID_A  SdfGrid.from_obstacles(obstacles(), -0.096, 0.012, 17): the nine-primitive test set sampled on 17^3, 19.2 cm across, the
          samples rounded to float32.  Spheres leave its box (the clamp branch) and come back.
  GRID_P  65^3 at spacing 0.05, centred (3.2 m across: every sphere of a frame that is not far is inside it, the largest |y| of
          these inputs is 1.03 m), the samples of ONE global trilinear polynomial.  The polynomial is stated in grid coordinates
          k = (y - origin) / spacing - 32, with coefficients that are multiples of 2^-19 (POLY), so that every sample is exact in
          float32: f(y) = a0 + b . k + c_xy kx ky + c_yz ky kz + c_xz kx kz + c_xyz kx ky kz.  Trilinear interpolation reproduces
          such a polynomial exactly in every cell: the interpolant is smooth across cell faces and has a closed form that knows
          nothing of cells (grid_reference.polynomial) -- a second, independent reference that needs no exclusion.

KINKS.  sdf is continuous; its gradient jumps across cell faces and the planes of the grid's box.  `gap` of the yardstick is an
entry's distance to the nearest of them.  The cotangent of every VJP is zero at entries with gap < FACE_GAP32 = 1e-5 m (at most 5 %
of the entries, asserted).  No active entry (h > 0) of GRID_A has gap < 1e-8 m, and at most one frame per robot has an active
entry with gap < FRAME_GAP32 = 1e-6 m -- a few times the float32 error of y at 1 m reach; the float32 comparison of grad and
wrench leaves such a frame out (near_face_frames).

CENTRAL DIFFERENCES (float64, step H = 1e-7), on entries and frames further than FD_GAP = 1e-5 m from a face: a step moves a
sphere by less than H x 0.5 m/rad, so it stays in its cell, where sdf is a polynomial.  A distance: |d| <= 2.5 m (the far
frames), so that the rounding of the difference is eps |d| / H = 5.5e-9, the centres add a few 1e-16 / H, and the truncation is
H^2 |d'''| / 6 with |d'''| of a trilinear cell below (2 / h^2) (0.5 m/rad)^3 = 1.8e3: 3e-12.  Gate GATE_D = 2e-8 per entry.  E:
at most 1 200 active entries of h^2 <= 0.07^2, E <= 6: rounding 1.3e-8; E is only C1: an entry within H |d'| of the margin adds
H times the jump 2 d'^2 <= 0.5 of its second derivative, 5e-8 per such entry.  Gate GATE_E = 2e-6, the sibling's (the
gradients themselves reach 1e-1)."""
import functools
import os
import re

import numpy as np
import pytest

import grid_reference as gref
import obstacle_reference as oref
from testutil import REPO
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, MARGIN, ROBOTS
from test_jacobian_host import SUBSET_CFG
from test_obstacle_host import obstacle_inputs, obstacles

HEADER = os.path.join(REPO, "include", "dexr_sdf_grid.h")
FRAGMENT = os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_sdf_grid.hpp")
INVALID, HIP = -1, -2
H, FD_GAP, GATE_D, GATE_E = 1e-7, 1e-5, 2e-8, 2e-6
FACE_GAP32, FRAME_GAP32, FACE_GAP64 = 1e-5, 1e-6, 1e-8
GD_SEED = 47
# a0, b (3), c_xy, c_yz, c_xz, c_xyz in grid coordinates, multiples of 2^-19: a slope of about 0.8 per metre, gently twisted
POLY = (-2.0 ** -6, 3 * 2.0 ** -7, -2 * 2.0 ** -7, 4 * 2.0 ** -7, 2.0 ** -14, -2.0 ** -14, 2.0 ** -15, 2.0 ** -19)
POLY_N, POLY_H = 65, 0.05


@functools.lru_cache(maxsize=None)
def grid_a():
    g = collision.SdfGrid.from_obstacles(obstacles(), -0.096, 0.012, 17)
    assert g.shape == (17, 17, 17) and g.values.dtype == np.float32
    return g


def polynomial_grid(n, spacing, exact=True):
    """n^3 samples of POLY at the grid coordinates k = i - (n - 1) / 2, centred on the origin of the obstacle frame.  With `exact`
    every sample must be a float32 value as it stands (it is for odd n <= 129)."""
    k = np.arange(n, dtype=np.float64) - (n - 1) / 2
    a0, bx, by, bz, cxy, cyz, cxz, cxyz = POLY
    x, y, z = k[:, None, None], k[None, :, None], k[None, None, :]
    f = a0 + bx * x + by * y + bz * z + cxy * x * y + cyz * y * z + cxz * x * z + cxyz * x * y * z  # (gref.polynomial, a slab less memory)
    v = f.astype(np.float32)
    assert not exact or np.array_equal(f, v), "the samples are not exact in float32"
    return collision.SdfGrid(v, -spacing * (n - 1) / 2, spacing)


@functools.lru_cache(maxsize=None)
def grid_p():
    return polynomial_grid(POLY_N, POLY_H)


def polynomial_of(grid, y):
    """the closed form of a polynomial_grid at points y of its frame: (f, grad in y)"""
    n = grid.shape[0]
    f, g = gref.polynomial(POLY, (np.asarray(y, np.float64) - grid.origin) / grid.spacing - (n - 1) / 2)
    return f, g / grid.spacing


GRIDS = {"A": grid_a, "P": grid_p}


def _geo(d, g):
    return d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"], g.values, g.origin, g.spacing


@functools.lru_cache(maxsize=None)
def masked_cotangent(name, which):
    """a seeded cotangent (B, S), float32-representable, zero at entries within FACE_GAP32 of a face: read-only"""
    d = obstacle_inputs(name)
    F = gref.fields(*_geo(d, GRIDS[which]()), d["pos"], d["rot"], jacobian=False)
    gd = np.random.default_rng(GD_SEED).standard_normal(F["d"].shape).astype(np.float32).astype(np.float64)
    g = np.where(F["gap"] >= FACE_GAP32, gd, 0.0)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def reference(name, which, dtype=np.float64):
    """the yardstick on obstacle_inputs(name) and GRID_A / GRID_P, computed once and shared, read-only: dict dist, vjp (of
    masked_cotangent), E, grad, wrench, h, gap, outside, y."""
    d = obstacle_inputs(name)
    F = gref.fields(*_geo(d, GRIDS[which]()), d["pos"], d["rot"], dtype)
    E, grad, wrench, h = gref.penalty(F, d["margin"])
    out = dict(dist=gref.distances(F), vjp=gref.distances_vjp(F, masked_cotangent(name, which)), E=E, grad=grad, wrench=wrench, h=h,
               gap=F["gap"], outside=F["outside"], y=F["y"])
    for k, v in out.items():
        assert v.dtype == (bool if k == "outside" else np.float64 if k == "gap" else dtype), k
        v.setflags(write=False)
    return out


def near_face_frames(r64):
    """(B,) bool: the frame has an active entry within FRAME_GAP32 of a face or clamp plane"""
    return ((r64["h"] > 0) & (r64["gap"] < FRAME_GAP32)).any(1)


def _declared(path):
    return set(re.findall(r"\b(dexr_[a-z0-9_]+)\s*\(", open(path).read()))


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_exports_are_the_header_and_the_library_exports_them():
    declared = _declared(HEADER)
    assert declared == set(_lib.SDF_GRID_EXPORTS) and len(_lib.SDF_GRID_EXPORTS) == 9 and len(set(_lib.SDF_GRID_EXPORTS)) == 9
    for other in (_lib.EXPORTS, _lib.POSE_EXPORTS, _lib.JAC_EXPORTS, _lib.WRENCH_EXPORTS, _lib.IK_EXPORTS, _lib.IK_SOLVE_EXPORTS,
                  _lib.SPHERE_EXPORTS, _lib.RESOLVE_EXPORTS, _lib.OBSTACLE_EXPORTS, _lib.RESOLVE_OBSTACLE_EXPORTS):
        assert not set(_lib.SDF_GRID_EXPORTS) & set(other)
    lib = _lib.load()
    for name in _lib.SDF_GRID_EXPORTS:
        assert hasattr(lib, name), f"libdexr.so does not export {name}"
    for h in sorted(os.listdir(os.path.join(REPO, "include"))):
        if h != "dexr_sdf_grid.h":
            assert not _declared(os.path.join(REPO, "include", h)) & declared, h
    text = open(HEADER).read()
    assert int(re.search(r"#define DEXR_SDF_GRID_MIN_DIM (\d+)", text).group(1)) == _lib.SDF_GRID_MIN_DIM == 2
    assert int(re.search(r"#define DEXR_SDF_GRID_MAX_DIM (\d+)", text).group(1)) == _lib.SDF_GRID_MAX_DIM == 1024
    assert int(re.search(r"#define DEXR_SDF_GRID_MAX_SAMPLES \(1 << (\d+)\)", text).group(1)) == 24 and _lib.SDF_GRID_MAX_SAMPLES == 1 << 24
    from dex_retargeting_amd import autograd as ag

    for n in ("grid_distances", "grid_penalty", "robot_grid_distances", "robot_grid_penalty"):
        assert n in collision.__all__ and n in ag.__all__
    assert "SdfGrid" in collision.__all__


def test_the_fragment_is_included_once_after_the_obstacle_resolve_and_has_no_forbidden_construct():
    pose = open(os.path.join(REPO, "dex_retargeting_amd", "csrc", "dexr_pose.hip")).read()
    assert pose.count('#include "dexr_sdf_grid.hpp"') == 1 and pose.count("dexr_sdf_grid.hpp") == 1
    assert pose.index('"dexr_sdf_grid.hpp"') > pose.index('"dexr_resolve_obstacles.hpp"')
    src = open(FRAGMENT).read()
    assert "getenv" not in src and "atomic" not in src and "asm" not in src.replace("__restrict__", "")
    assert src.count('#include "') == 1 and '#include "dexr_sdf_grid.h"' in src  # (a fragment: no unit of its own)


def _create(n, origin, spacing, values, out=True):
    lib = _lib.load()
    C = _lib.C
    n = None if n is None else np.ascontiguousarray(n, np.int32)
    origin = None if origin is None else np.ascontiguousarray(origin, np.float64)
    spacing = None if spacing is None else np.ascontiguousarray(spacing, np.float64)
    values = None if values is None else np.ascontiguousarray(values, np.float32)
    h = C.c_void_p()
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = lib.dexr_sdf_grid_create(p(n, C.c_int32), p(origin, C.c_double), p(spacing, C.c_double), p(values, C.c_float), C.byref(h) if out else None)
    if rc == 0:
        lib.dexr_sdf_grid_destroy(h)
    else:
        assert not h.value
    return rc, lib.dexr_last_error().decode()


def _malformed():
    """(word of the C message, word of the Python message, shape, origin, spacing, values or None: zeros) of every malformed grid"""
    ok = np.zeros((3, 4, 5), np.float32)
    out = []
    for shape in ((1, 4, 5), (3, 1, 5), (3, 4, 1), (1025, 2, 2), (2, 1025, 2), (2, 2, 1025)):
        out.append(("dimension", "dimension", shape, 0.0, 0.01, None))
    out.append(("samples", "samples", (1024, 1024, 17), 0.0, 0.01, None))
    for bad in (0.0, -0.01, np.nan, np.inf, -np.inf, 1e-320):  # (1 / 1e-320 is not finite)
        for a in range(3):
            s = np.full(3, 0.01)
            s[a] = bad
            out.append(("spacing", "spacing", ok.shape, 0.0, s, ok))
    for bad in (np.nan, np.inf, -np.inf):
        o = np.zeros(3)
        o[1] = bad
        out.append(("origin", "origin", ok.shape, o, 0.01, ok))
        v = ok.copy()
        v[2, 3, 4] = bad
        out.append(("sample", "samples must be finite", ok.shape, 0.0, 0.01, v))
    return out


def test_sdf_grid_create_validates_before_it_looks_for_a_device():
    big = np.zeros(1024 * 1024 * 17, np.float32)  # (shared: the C side must refuse the count before it reads a sample)
    b3 = lambda v: np.broadcast_to(np.asarray(v, np.float64), (3,))  # noqa: E731
    for cword, _, shape, origin, spacing, values in _malformed():
        v = big[:int(np.prod(shape))] if values is None else values
        rc, msg = _create(shape, b3(origin), b3(spacing), v)
        assert rc == INVALID and cword in msg, (rc, msg, cword, shape)
    ok = np.zeros((3, 4, 5), np.float32)
    for kw in (dict(n=None), dict(origin=None), dict(spacing=None), dict(values=None)):
        a = dict(n=ok.shape, origin=np.zeros(3), spacing=np.full(3, 0.01), values=ok)
        a.update(kw)
        rc, msg = _create(**a)
        assert rc == INVALID and "null" in msg
    assert _create(ok.shape, np.zeros(3), np.full(3, 0.01), ok, out=False)[0] == INVALID
    # the limits themselves are fine: one cell, the longest axis, an anisotropic spacing
    want = 0 if _lib.load().dexr_device_count() > 0 else HIP  # a well-formed input needs a device
    for shape, spacing in (((2, 2, 2), (0.01, 0.01, 0.01)), ((1024, 2, 2), (1e-3, 1.0, 10.0)), ((3, 4, 5), (0.03, 0.05, 0.11))):
        rc, msg = _create(shape, np.array([-1.0, 2.0, 0.5]), np.array(spacing), np.zeros(shape, np.float32))
        assert rc == want, (rc, msg)
    if want == HIP:
        with pytest.raises(_lib.DexrError, match="libdexr error -2"):
            _lib.SdfGrid(ok, np.zeros(3), np.full(3, 0.01))
    with pytest.raises(ValueError, match="shape"):
        _lib.SdfGrid(ok[0], np.zeros(3), np.full(3, 0.01))
    lib = _lib.load()
    assert lib.dexr_sdf_grid_info(None, None, None, None) == INVALID and b"null sdf grid" in lib.dexr_last_error()
    lib.dexr_sdf_grid_destroy(None)


# ---- 2. SdfGrid and the argument rules of the torch front ----------------------------------------------------------------------------
def test_sdf_grid_is_plain_hashable_data_with_the_rules_of_the_c_side(monkeypatch):
    G = collision.SdfGrid
    a = grid_a()
    b = G(a.values.copy(), a.origin.tolist(), a.spacing.copy())
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1 and a.shape == (17, 17, 17) and "17x17x17" in repr(a)
    assert a != G(a.values, a.origin, a.spacing * 2) and a != G(a.values, a.origin + 1e-3, a.spacing) and a != G(-a.values, a.origin, a.spacing)
    assert a != G(a.values.reshape(17, 289, 1).repeat(2, 2)[:, :17], a.origin, a.spacing)
    assert a.origin.tolist() == [-0.096] * 3 and a.spacing.tolist() == [0.012] * 3 and a.values.flags["C_CONTIGUOUS"]
    for arr in (a.values, a.origin, a.spacing):
        with pytest.raises(ValueError):
            arr[(0,) * arr.ndim] = 1.0
    # a Fortran-ordered or float64 input is the same grid: the ABI layout is C order, float32
    v = np.random.default_rng(1).standard_normal((3, 4, 5)).astype(np.float32)
    assert G(np.asfortranarray(v), 0.0, 0.1) == G(v.astype(np.float64), [0, 0, 0], [0.1] * 3) == G(v, 0.0, 0.1)
    b3 = lambda x: x  # noqa: E731
    for _, pyword, shape, origin, spacing, values in _malformed():
        if values is None and int(np.prod(shape)) > 1 << 20:
            values = np.broadcast_to(np.float32(0), shape)  # (no 68 MB array for a count that is refused)
        with pytest.raises(ValueError, match=pyword):
            G(np.zeros(shape, np.float32) if values is None else values, b3(origin), b3(spacing))
    for bad, word in ((lambda: G(np.zeros((3, 4)), 0.0, 0.1), "shape"), (lambda: G(np.zeros((3, 4, 5, 2)), 0.0, 0.1), "shape"),
                      (lambda: G(v, [0, 0], 0.1), "scalar or"), (lambda: G(v, 0.0, [0.1, 0.1]), "scalar or"),
                      (lambda: G(v.astype(np.float64) * 1e39, 0.0, 0.1), "finite"),
                      (lambda: G.from_obstacles(None, 0.0, 0.1, 4), "ObstacleSet"), (lambda: G.from_obstacles(obstacles(), 0.0, 0.1, 1), "dimension"),
                      (lambda: G.from_obstacles(obstacles(), 0.0, 0.1, (4, 4)), "scalar or"), (lambda: G.from_obstacles(obstacles(), 0.0, -0.1, 4), "spacing")):
        with pytest.raises(ValueError, match=word):
            bad()
    # the device copy: made once per grid (and device), kept with it
    made = []
    monkeypatch.setattr(_lib.SdfGrid, "__init__", lambda self, values, origin, spacing: made.append((values.shape, values.dtype)))
    t = G(v, 0.0, 0.1)
    assert t.device_grid(0) is t.device_grid(0) and t.device_grid(1) is not t.device_grid(0) and made == [((3, 4, 5), np.float32)] * 2


def test_argument_rules_raise_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    touched = []
    for cls in (_lib.SphereModel, _lib.PoseModel, _lib.SdfGrid):
        monkeypatch.setattr(cls, "__init__", lambda self, *a, **k: touched.append("create"))
    for method in ("grid_distances_dev", "grid_distances_vjp_dev", "grid_penalty_dev"):
        monkeypatch.setattr(_lib.SphereModel, method, lambda self, *a, _m=method, **k: touched.append(_m))
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    tips = ["link_15.0_tip", "link_3.0_tip", "link_7.0_tip", "base_link"]
    sset = collision.SphereSet(tips, np.zeros((4, 3)), np.full(4, 0.01))
    grid = grid_a()
    good = torch.zeros((4, 16), dtype=torch.float32)  # CPU tensors: right in everything but the device
    pos, rot = torch.zeros((4, 3), dtype=torch.float32), torch.eye(3, dtype=torch.float32).repeat(4, 1, 1)
    fronts = [lambda q, s, g, margin=0.01, **k: collision.grid_penalty(opt, q, s, g, margin, **k),
              lambda q, s, g, margin=0.01, **k: ag.grid_penalty(opt, q, s, g, margin, **k),
              lambda q, s, g, margin=0.01, **k: collision.robot_grid_penalty(opt.robot, q, s, g, margin, **k),
              lambda q, s, g, margin=0.01, **k: ag.robot_grid_penalty(opt.robot, q, s, g, margin, **k)]
    dists = [lambda q, s, g, **k: collision.grid_distances(opt, q, s, g, **k), lambda q, s, g, **k: ag.grid_distances(opt, q, s, g, **k),
             lambda q, s, g, **k: collision.robot_grid_distances(opt.robot, q, s, g, **k),
             lambda q, s, g, **k: ag.robot_grid_distances(opt.robot, q, s, g, **k)]

    def raises(fns, match=None, q=good, s=sset, g=grid, **kw):
        for f in fns:
            with pytest.raises(ValueError, match=match):
                f(q, s, g, **kw)

    # CPU tensors: the device rule, and it comes last (everything else is right here)
    raises(fronts + dists, "CUDA")
    raises(fronts + dists, "CUDA", obstacle_pos=pos, obstacle_rot=rot)
    raises(fronts, "CUDA", margin=0)
    raises(fronts, "CUDA", margin=1)  # Python ints are numbers too
    raises(fronts[::2], "CUDA", wrench=True)
    # dtype, shape, type of q
    raises(fronts + dists, "float32", q=good.double())
    for bad in (good[:, :15], good.reshape(-1), good[:, :, None]):
        raises(fronts + dists, "shape", q=bad)
    raises(fronts + dists, "torch tensor", q=good.numpy())
    # the sphere set and the grid
    raises(fronts + dists, "SphereSet", s=tips)
    raises(fronts + dists, "is not a link name", s=collision.SphereSet(["link_15.0_tip", "no_such_link"], np.zeros((2, 3)), [0.01, 0.01]))
    raises(fronts + dists, "SdfGrid", g=(grid.values, grid.origin, grid.spacing))
    raises(fronts + dists, "SdfGrid", g=obstacles())
    raises(fronts + dists, "SdfGrid", g=None)
    # margin: a finite Python float >= 0
    for bad in (-1e-9, -1, float("nan"), float("inf"), torch.tensor(0.01), None, "0.01", True):
        raises(fronts, "margin", margin=bad)
    # the obstacle pose: float32 tensors of one pose per frame
    raises(fronts + dists, "float32", obstacle_pos=pos.double())
    raises(fronts + dists, "float32", obstacle_rot=rot.double())
    raises(fronts + dists, "torch tensor", obstacle_pos=pos.numpy())
    raises(fronts + dists, "torch tensor", obstacle_rot=rot.numpy())
    for bad in (pos[:3], pos[:, :2], pos[0], torch.zeros((1, 3))):
        raises(fronts + dists, "obstacle_pos must have shape", obstacle_pos=bad)
    for bad in (rot[:3], rot.reshape(4, 9), rot[0], pos):
        raises(fronts + dists, "obstacle_rot must have shape", obstacle_rot=bad)
    # no gradient flows to a rotation matrix: the message names the way to the torque
    raises(fronts[1::2] + dists[1::2], "wrench=True", obstacle_rot=rot.clone().requires_grad_(True))
    # fixed_qpos: one too many, one missing, one of the wrong width
    raises(fronts[:2] + dists[:2], "fixed_qpos", fixed_qpos=torch.zeros((4, 1), dtype=torch.float32))
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    assert len(sub.idx_pin2fixed) == 6
    q10 = torch.zeros((4, 10), dtype=torch.float32)
    for fq, word in ((None, "fixed_qpos"), (torch.zeros((4, 5), dtype=torch.float32), "fixed_qpos"), (torch.zeros((4, 6), dtype=torch.float64), "float32"),
                     (torch.zeros((4, 6), dtype=torch.float32), "CUDA")):
        for f in (collision.grid_distances, ag.grid_distances):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sset, grid, fixed_qpos=fq)
        for f in (collision.grid_penalty, ag.grid_penalty):
            with pytest.raises(ValueError, match=word):
                f(sub, q10, sset, grid, 0.01, fixed_qpos=fq)
    assert touched == []


# ---- 3. the yardstick against itself ---------------------------------------------------------------------------------------------------
def test_reference_interpolates_the_samples_and_continues_them_outside():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((5, 3, 2)).astype(np.float32).astype(np.float64)
    o, h = np.array([-0.04, 0.1, 0.3]), np.array([0.03, 0.05, 0.11])
    idx = np.stack(np.meshgrid(np.arange(5), np.arange(3), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    d, g, gap = gref.sdf(v, o, h, o + idx * h)
    assert np.abs(d - v[idx[:, 0], idx[:, 1], idx[:, 2]]).max() < 1e-14  # on the samples (to the rounding of (y - o) / h)
    mid = o + (np.array([1, 1, 0]) + 0.5) * h
    d, g, gap = gref.sdf(v, o, h, mid)
    assert abs(d - v[1:3, 1:3, 0:2].mean()) < 1e-13 and abs(gap - 0.015) < 1e-13
    want = [(v[2, 1:3, :] - v[1, 1:3, :]).mean() / h[0], (v[1:3, 2, :] - v[1:3, 1, :]).mean() / h[1], (v[1:3, 1:3, 1] - v[1:3, 1:3, 0]).mean() / h[2]]
    assert np.abs(g - want).max() < 1e-13
    # 0.5 m beyond the +x face: the value on the face, the distance to it, the axis normal
    face = o + np.array([4, 0.5, 0.25]) * h
    d0, g0, _ = gref.sdf(v, o, h, face - np.array([1e-13, 0, 0]))
    d1, g1, gap1 = gref.sdf(v, o, h, face + np.array([0.5, 0, 0]))
    assert abs(d1 - d0 - 0.5) < 1e-12 and g1[0] == 1.0 and np.abs(g1[1:] - g0[1:]).max() < 1e-9 and abs(gap1 - 0.5 * h[1]) < 1e-13
    # beyond a corner: the corner sample and the distance to it, the unit vector from it; continuous across the planes of the box
    c = o + np.array([4, 2, 1]) * h
    e = np.array([0.3, -0.0, 0.4])
    d2, g2, _ = gref.sdf(v, o, h, c + np.array([0.3, 0.2, 0.4]))
    assert abs(d2 - v[4, 2, 1] - np.sqrt(0.29)) < 1e-12 and np.abs(g2 - np.array([0.3, 0.2, 0.4]) / np.sqrt(0.29)).max() < 1e-12 and e[1] == 0
    y = rng.uniform(-0.3, 0.6, (2000, 3))
    step = rng.standard_normal((2000, 3)) * 1e-9
    assert np.abs(gref.sdf(v, o, h, y + step)[0] - gref.sdf(v, o, h, y)[0]).max() < 1e-6  # (|grad| of random samples reaches 1e2)
    # a NaN clamps to cell 0 and stays a NaN in the distance; float32 runs in float32
    dn = gref.sdf(v, o, h, np.array([np.nan, 0.15, 0.3]))[0]
    assert np.isnan(dn)
    d32, g32, _ = gref.sdf(v, o, h, y.astype(np.float32), np.float32)
    assert d32.dtype == g32.dtype == np.float32 and np.abs(d32 - gref.sdf(v, o, h, y)[0]).max() < 1e-4


def test_reference_on_the_polynomial_grid_equals_the_closed_form():
    g = grid_p()
    assert g.shape == (65, 65, 65) and g.origin.tolist() == [-1.6] * 3 and all(float(c) == float(np.float32(c)) for c in POLY)
    y = np.random.default_rng(8).uniform(-1.59, 1.59, (20000, 3))
    d, grad, _ = gref.sdf(g.values, g.origin, g.spacing, y)
    f, fg = polynomial_of(g, y)
    print(f"polynomial grid: max |sdf - closed form| = {np.abs(d - f).max():.3e}, max |grad - closed form| = {np.abs(grad - fg).max():.3e} (gate 1e-12)")
    assert np.abs(d - f).max() <= 1e-12 and np.abs(grad - fg).max() <= 1e-12 and 0.5 < np.linalg.norm(fg, axis=-1).mean() < 1.5


@pytest.mark.parametrize("name", ["shadow_hand_right", "allegro_hand_right"])
@pytest.mark.parametrize("which", ["A", "P"])
def test_reference_gradients_equal_central_differences(name, which):
    d, grid = obstacle_inputs(name), GRIDS[which]()
    orc, q, links, rows, centers, radii = d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"]
    pos, rot, margin = d["pos"], d["rot"], d["margin"]

    def run(q_, pos_=pos):
        F = gref.fields(orc, q_, links, rows, centers, radii, grid.values, grid.origin, grid.spacing, pos_, rot, jacobian=False)
        return F["d"], gref.penalty(F, margin)[0]

    F = gref.fields(orc, q, links, rows, centers, radii, grid.values, grid.origin, grid.spacing, pos, rot)
    E, grad, wrench, h = gref.penalty(F, margin)
    smooth = F["gap"] >= FD_GAP  # entries
    keep = ~((h > 0) & ~smooth).any(1)  # frames
    # (an entry is within FD_GAP of a face with probability 3 x 2 FD_GAP / 0.012 = 0.5 %; a frame has some forty active entries)
    assert smooth.mean() > 0.95 and keep.mean() > 0.7 and (E[keep] > 0).any()
    dn = np.einsum("bsr,bsrc->bsc", F["n"], F["jpt"])  # d dist / dq
    worst = dict(dist_q=0.0, dist_p=0.0)
    fd = np.zeros_like(grad)
    for c in range(orc.dof):
        e = np.zeros(orc.dof)
        e[c] = H
        (dp, Ep), (dm, Em) = run(q + e), run(q - e)
        worst["dist_q"] = max(worst["dist_q"], float(np.abs((dp - dm) / (2 * H) - dn[..., c])[smooth].max()))
        fd[:, c] = (Ep - Em) / (2 * H)
    worst["E_q"] = float(np.abs(fd - grad)[keep].max())
    fd = np.zeros((B, 3))
    for i in range(3):
        e = np.zeros(3)
        e[i] = H
        (dp, Ep), (dm, Em) = run(q, pos + e), run(q, pos - e)
        worst["dist_p"] = max(worst["dist_p"], float(np.abs((dp - dm) / (2 * H) + F["n"][..., i])[smooth].max()))  # d dist / dp_o = -n
        fd[:, i] = (Ep - Em) / (2 * H)
    worst["E_p"] = float(np.abs(fd - wrench[:, :3])[keep].max())
    print(f"{name} GRID_{which}: max |d dist/dq - cd| = {worst['dist_q']:.3e}, |d dist/dp_o - cd| = {worst['dist_p']:.3e} (gate {GATE_D:.0e}); "
          f"|dE/dq - cd| = {worst['E_q']:.3e}, |wrench force - cd| = {worst['E_p']:.3e} (gate {GATE_E:.0e}); max |dE/dq| {np.abs(grad).max():.3e}; "
          f"{int((~smooth).sum())} entries and {int((~keep).sum())} frames left out")
    assert np.abs(grad).max() > 1e-3 and np.abs(wrench[:, :3]).max() > 1e-3
    assert max(worst["dist_q"], worst["dist_p"]) <= GATE_D and max(worst["E_q"], worst["E_p"]) <= GATE_E
    # the VJP is the contraction of the same entries
    gd = masked_cotangent(name, which)
    assert np.abs(gref.distances_vjp(F, gd) - np.einsum("bs,bsc->bc", gd, dn)).max() < 1e-12


# ---- 4. from_obstacles ties the two families together ----------------------------------------------------------------------------------
def test_a_sampled_half_space_is_the_half_space_inside_the_grid():
    """An affine function is interpolated exactly, so that what separates the grid of one half-space from the half-space is the
    rounding of the samples to float32 alone: none with an axis normal and a dyadic origin, spacing and offset (gate 1e-12), at
    most half an ulp of 0.35 = 1.5e-8 with a tilted normal (gate 1e-12 + the rounding that the test measures on the samples)."""
    lo, hi, h = np.array([-0.25, -0.125, -0.25]), np.array([0.25, 0.125, 0.25]), np.array([0.03125, 0.015625, 0.0625])
    y = np.random.default_rng(3).uniform(lo, hi, (5000, 3))
    for n, exact in (([0.0, -1.0, 0.0], True), ([0.6, 0.0, 0.8], False)):
        hs = collision.ObstacleSet.half_spaces([n], [-0.0625])
        g = collision.SdfGrid.from_obstacles(hs, lo, h, (17, 17, 9))
        assert g.shape == (17, 17, 9)
        pts = np.stack(np.meshgrid(*[g.origin[a] + np.arange(g.shape[a]) * g.spacing[a] for a in range(3)], indexing="ij"), -1)
        rounding = float(np.abs(g.values.astype(np.float64) - oref.sdf(hs.kinds, hs.params, pts)[0][..., 0]).max())
        assert (rounding == 0) == exact and rounding < 1.5e-8
        d, grad, _ = gref.sdf(g.values, g.origin, g.spacing, y)
        want, wg = oref.sdf(hs.kinds, hs.params, y)
        print(f"half-space {n}: the float32 samples are {rounding:.3e} from the float64 distances; max |interpolated - half-space| = "
              f"{np.abs(d - want[:, 0]).max():.3e}, max |grad - normal| = {np.abs(grad - wg[:, 0]).max():.3e}")
        assert np.abs(d - want[:, 0]).max() <= 1e-12 + rounding and np.abs(grad - wg[:, 0]).max() <= 1e-12 + 2 * rounding / h.min()
    # the union: the minimum over the primitives at every sample of GRID_A
    a, ob = grid_a(), obstacles()
    pts = np.stack(np.meshgrid(*[a.origin[i] + np.arange(17) * a.spacing[i] for i in range(3)], indexing="ij"), -1)
    assert np.array_equal(a.values, oref.sdf(ob.kinds, ob.params, pts)[0].min(-1).astype(np.float32))


# ---- 5. the inputs of the GPU tests ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_gpu_inputs_meet_the_conditions_the_gpu_gates_rest_on(name):
    d = obstacle_inputs(name)
    assert d["margin"] == MARGIN and d["far"].sum() == 8 and len(ROBOTS) == 8
    near = ~d["far"]
    # GRID_A
    r = reference(name, "A")
    active = r["h"] > 0
    n_active, frames, outside, active_outside = int(active.sum()), int(active.any(1).sum()), int(r["outside"].sum()), int((active & r["outside"]).sum())
    close_frames = int(near_face_frames(r).sum())
    masked = float((r["gap"] < FACE_GAP32).mean())
    print(f"{name} GRID_A: {n_active} active entries on {frames} frames, {outside} entries outside the box ({active_outside} of them active), "
          f"smallest gap of an active entry {r['gap'][active].min():.3e} m, {close_frames} frames with an active entry within {FRAME_GAP32:g} m, "
          f"{masked:.4f} of the cotangent masked, max E {r['E'].max():.3e}, max |grad| {np.abs(r['grad']).max():.3e}")
    assert 141 <= n_active <= 1198 and 22 <= frames <= 25 and 48 <= outside <= 2151 and 0 <= active_outside <= 172
    assert (r["gap"][active] >= FACE_GAP64).all() and close_frames <= 1 and masked <= 0.05
    assert close_frames == (1 if name in ("ability_hand_right", "arm_shadow_hand_right") else 0)
    assert (r["E"][d["far"]] == 0).all() and not r["grad"][d["far"]].any() and not r["wrench"][d["far"]].any() and r["outside"][d["far"]].all()
    assert np.isfinite(r["grad"]).all() and np.abs(r["grad"]).max() > 0 and np.abs(r["wrench"]).max() > 0
    # GRID_P: every sphere of a near frame inside, at least half the near frames active, the yardstick is the closed form there
    p = reference(name, "P")
    assert not p["outside"][near].any() and np.abs(p["y"][near]).max() <= 1.03 + 1e-9
    assert (p["h"][near] > 0).any(1).sum() * 2 >= near.sum() and (p["E"][d["far"]] == 0).all() and (p["gap"] < FACE_GAP32).mean() <= 0.05
    f, fg = polynomial_of(grid_p(), p["y"][near])
    assert np.abs(p["dist"][near] + d["radii"] - f).max() <= 1e-12
    print(f"{name} GRID_P: {int((p['h'] > 0).sum())} active entries on {int((p['h'] > 0).any(1).sum())} frames, max |y| {np.abs(p['y'][near]).max():.3f} m, "
          f"max E {p['E'].max():.3e}")

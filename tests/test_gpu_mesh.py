"""GPU tests of the mesh distance kernels (csrc/dexr_mesh_sdf.hpp, include/dexr_mesh_sdf.h): the float64 host entry and the float32
device entry against tests/mesh_reference.py on the point sets of tests/test_mesh_host.py (whose reference runs and conditions are
proven there on the CPU and shared from there), the grid entry against the point entry bit for bit, block sizes and batch
independence, isolation of non-finite points, the optional winding output, the multi-launch path, SdfGrid.from_mesh end to end
against SdfGrid.from_obstacles, the torch front and the raw ABI's argument errors.

GATES.  float64: | |got| - |reference64| | <= 1e-9 (GATE64), the sign equal wherever |d_ref| >= SIGN_GAP, the winding number within
1e-9 there (on the surface itself it jumps by one and the solid angle of the triangle under the point is +-2 pi by the sign of a
zero).  float32: max | |got32| - |reference64| | at most 8 x (GATE32) the distance between the reference's OWN float32 and float64
runs on that output, never a figure of the code under test; the sign equal outside SIGN_GAP and, on open meshes, outside
WIND_BAND; the winding number by the same 8 x rule off the surface.  The ratios are printed; those of the MI355X are in
docs/experiments/mesh_sdf.md."""
import numpy as np
import pytest

import mesh_reference as mr
from dex_retargeting_amd import _lib, collision
from test_mesh_host import (CUBE_H, CUBE_N, CUBE_O, POINT_SETS, SIGN_GAP, TET_GRIDS, WIND_BAND, _r32, case, multi_launch_grid)

pytestmark = pytest.mark.gpu
GATE64, GATE32 = 1e-9, 8.0
BLOCK = _lib.MESH_BLOCK_POINTS


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def dev(torch, mesh, p, winding=True):
    """the float32 device entry on a numpy (P, 3) array, the outputs pre-filled with NaN -> dist (P,), winding (P,) or None; float32"""
    pt = torch.tensor(np.ascontiguousarray(p, dtype=np.float32), device="cuda")
    P = pt.shape[0]
    d, w = _nan(torch, (P,)), (_nan(torch, (P,)) if winding else None)
    mesh.device_mesh(torch.cuda.current_device()).distances_dev(P, pt.data_ptr(), d.data_ptr(), 0 if w is None else w.data_ptr(),
                                                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.cpu().numpy(), (None if w is None else w.cpu().numpy())


def dev_grid(torch, mesh, n, o, h):
    buf = _nan(torch, tuple(n))
    mesh.device_mesh(torch.cuda.current_device()).sample_grid_dev(n, o, h, buf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _signs_agree(tag, c, got, band=True):
    """band: float32 on an open mesh, where the winding band is left out as well"""
    keep = np.abs(c["d64"]) >= SIGN_GAP
    if band and c["open"]:
        keep &= np.abs(c["w64"] - 0.5) >= WIND_BAND
    bad = keep & ((got < 0) != (c["d64"] < 0))
    assert not bad.any(), (tag, int(bad.sum()), c["p"][bad][:3], got[bad][:3], c["d64"][bad][:3])


def check64(tag, c, d, w):
    assert d.dtype == np.float64 and d.shape == c["d64"].shape and np.isfinite(d).all()
    e = float(np.abs(np.abs(d) - np.abs(c["d64"])).max())
    off = np.abs(c["d64"]) >= SIGN_GAP
    ew = float(np.abs(w - c["w64"])[off].max())
    print(f"{tag}: float64 max ||d| - |reference|| = {e:.3e}, max |w - reference| off the surface = {ew:.3e} (gates {GATE64:.0e})")
    assert e <= GATE64 and ew <= GATE64 and np.isfinite(w).all()
    _signs_agree(tag, c, d, band=False)


def check32(tag, c, d, w):
    assert d.dtype == np.float32 and d.shape == c["d64"].shape and np.isfinite(d).all() and np.isfinite(w).all()
    off = np.abs(c["d64"]) >= SIGN_GAP
    for k, got, r64, r32, keep in (("|d|", np.abs(d.astype(np.float64)), np.abs(c["d64"]), np.abs(c["d32"]), np.ones(len(d), bool)),
                                   ("w", w.astype(np.float64), c["w64"], c["w32"], off)):
        dist = float(np.abs(r32 - r64)[keep].max())
        e = float(np.abs(got - r64)[keep].max())
        ratio = e / dist if dist > 0 else (0.0 if e == 0 else float("inf"))
        print(f"{tag}: float32 max |{k} - reference64| = {e:.3e}, the reference's float32 run is {dist:.3e} from its float64 run "
              f"(error / reference distance {ratio:.2f}, gate {GATE32:g})")
        assert ratio <= GATE32, (tag, k, e, dist)
    _signs_agree(tag, c, d)


# ---- 1. parity on every point set: one triangle, the cubes, the grids, the tile boundaries, the open sphere ----------------------------
SETS = [n for n in POINT_SETS if n != "multi"]


@pytest.mark.parametrize("name", SETS)
def test_host_float64_against_the_reference(name, require_gpu):
    c = case(name)
    h = c["mesh"].device_mesh(0)
    assert (h.n_vertex, h.n_triangle) == (len(c["v"]), len(c["f"])) and np.array_equal(h.bounds, c["mesh"].bounds)
    d, w = h.distances(c["p"], winding=True)
    check64(name, c, d, w)


@pytest.mark.parametrize("name", SETS)
def test_device_float32_against_the_reference(name, require_gpu):
    torch = pytest.importorskip("torch")
    c = case(name)
    d, w = dev(torch, c["mesh"], c["p"])
    check32(name, c, d, w)


# ---- 2. the grid entry is the point entry on the same coordinates, in C order, bit for bit ---------------------------------------------
@pytest.mark.parametrize("name", ["tet_2x2x2", "tet_5x7x9", "cube"])
def test_grid_entry_is_the_point_entry_in_c_order(name, require_gpu):
    torch = pytest.importorskip("torch")
    c = case(name)
    n, o, h = TET_GRIDS[name] if name in TET_GRIDS else (CUBE_N, CUBE_O, CUBE_H)
    pts = mr.grid_points(n, o, h)  # float64, unrounded
    assert np.array_equal(_r32(pts), c["p"]) and len(set(np.asarray(h).tolist())) == (1 if name == "tet_2x2x2" else 3)
    g32 = dev_grid(torch, c["mesh"], n, o, h)
    d32, _ = dev(torch, c["mesh"], c["p"])
    assert g32.shape == tuple(n) and np.array_equal(g32.reshape(-1), d32)  # (the case's float32 gate has passed on d32)
    hm = c["mesh"].device_mesh(0)
    g64 = hm.sample_grid(n, o, h)
    d64 = hm.distances(pts)
    assert g64.dtype == np.float32 and g64.shape == tuple(n) and np.array_equal(g64.reshape(-1), d64.astype(np.float32))
    e = float(np.abs(np.abs(d64) - np.abs(mr.sdf(c["v"], c["f"], pts)[0])).max())
    print(f"{name}: float64 on the unrounded sample coordinates, max ||d| - |reference|| = {e:.3e} (gate {GATE64:.0e})")
    assert e <= GATE64


# ---- 3. block sizes, batch independence ------------------------------------------------------------------------------------------------
def test_block_sizes_and_batch_independence(require_gpu):
    torch = pytest.importorskip("torch")
    c = case("cube_rot")
    mesh, p = c["mesh"], c["p"]
    assert len(p) > 2 * BLOCK + 1
    full_d, full_w = dev(torch, mesh, p)
    check32("cube_rot, the whole batch", c, full_d, full_w)
    for P in (1, BLOCK - 1, BLOCK, BLOCK + 1):  # one point, one short of a block, a block, a block and a tail of one
        d, w = dev(torch, mesh, p[:P])
        assert np.array_equal(d, full_d[:P]) and np.array_equal(w, full_w[:P]), P
    for i in (0, BLOCK + 7, len(p) - 1):  # a point alone, wherever it sat
        d, w = dev(torch, mesh, p[i:i + 1])
        assert d[0] == full_d[i] and w[0] == full_w[i], i
    perm = np.random.default_rng(21).permutation(len(p))
    d, w = dev(torch, mesh, p[perm])
    assert np.array_equal(d, full_d[perm]) and np.array_equal(w, full_w[perm])
    hm = mesh.device_mesh(0)
    hd, hw = hm.distances(p, winding=True)
    for sl in (slice(0, 1), slice(BLOCK - 1, BLOCK + 1), slice(len(p) - 1, len(p))):
        d, w = hm.distances(p[sl], winding=True)
        assert np.array_equal(d, hd[sl]) and np.array_equal(w, hw[sl])
    assert hm.distances(np.zeros((0, 3))).shape == (0,)


# ---- 4. a non-finite point spoils only itself, 5. the winding output is optional -----------------------------------------------------------
def test_non_finite_points_spoil_only_themselves_and_winding_is_optional(require_gpu):
    torch = pytest.importorskip("torch")
    c = case("ico3_515")
    mesh, p = c["mesh"], c["p"]
    full_d, full_w = dev(torch, mesh, p)
    hm = mesh.device_mesh(0)
    hd, hw = hm.distances(p, winding=True)
    where = [(0, 0), (5, 1), (len(p) - 1, 2), (257, 0)]
    keep = np.ones(len(p), bool)
    keep[[i for i, _ in where]] = False
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        for i, k in where:
            q[i, k] = bad
        d, w = dev(torch, mesh, q)
        assert np.isnan(d[~keep]).all() and np.isnan(w[~keep]).all(), bad
        assert np.array_equal(d[keep], full_d[keep]) and np.array_equal(w[keep], full_w[keep]), bad
        d, w = hm.distances(q, winding=True)
        assert np.isnan(d[~keep]).all() and np.isnan(w[~keep]).all() and np.array_equal(d[keep], hd[keep]) and np.array_equal(w[keep], hw[keep]), bad
    huge = p.copy()
    huge[3] = (3e38, -3e38, 1e30)  # finite, beyond every square: its own entry alone
    d, w = dev(torch, mesh, huge)
    k3 = np.arange(len(p)) != 3
    assert np.array_equal(d[k3], full_d[k3]) and np.array_equal(w[k3], full_w[k3]) and not np.isfinite(d[3])
    torch.cuda.synchronize()
    # winding_out NULL: the distances keep their bits
    d, w = dev(torch, mesh, p, winding=False)
    assert w is None and np.array_equal(d, full_d)
    assert np.array_equal(hm.distances(p), hd)


# ---- 6. more than one launch -------------------------------------------------------------------------------------------------------------
def test_three_launches_are_the_point_entry_bit_for_bit(require_gpu):
    torch = pytest.importorskip("torch")
    c = case("multi")
    n, o, h = multi_launch_grid()
    total, T = n[0] * n[1] * n[2], len(c["f"])
    per = _lib.mesh_points_per_launch(T)
    assert 2 * per < total <= 3 * per and per * T <= _lib.MESH_PAIRS_PER_LAUNCH < (per + BLOCK) * T
    mesh = c["mesh"]
    g = dev_grid(torch, mesh, n, o, h).reshape(-1)
    assert np.isfinite(g).all()  # every sample of every launch is written
    pts = torch.tensor(mr.grid_points(n, o, h), dtype=torch.float64, device="cuda").to(torch.float32)
    d = collision.mesh_distances(mesh, pts)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), g)
    idx = np.round((c["p"] - o) / h).astype(np.int64) @ np.array([n[1] * n[2], n[2], 1])
    assert np.array_equal(_r32(mr.grid_points(n, o, h)[idx]), c["p"])
    got = g[idx]
    dist = float(np.abs(np.abs(c["d32"]) - np.abs(c["d64"])).max())
    e = float(np.abs(np.abs(got.astype(np.float64)) - np.abs(c["d64"])).max())
    print(f"three launches of {per} samples x {T} triangles ({n[0]}^3 = {total} samples): 256 seeded samples, float32 max ||d| - |reference64|| = {e:.3e}, "
          f"the reference's float32 run is {dist:.3e} from its float64 run (ratio {e / dist:.2f}, gate {GATE32:g})")
    assert e <= GATE32 * dist
    _signs_agree("multi", c, got)
    for k in (per - 1, per, 2 * per - 1, 2 * per, total - 1):  # the seams between the launches
        one = collision.mesh_distances(mesh, pts[k:k + 1])
        assert float(one[0]) == float(g[k]), k


# ---- 7. end to end: a grid from a mesh is the grid from the primitive it models ---------------------------------------------------------------
BOX_HALF, BOX_N, BOX_O, BOX_H = np.array([0.03, 0.02, 0.04]), (17, 17, 17), -0.0775, 0.01  # (no sample on the surface)


def _box_grids(precision="float64"):
    box = collision.ObstacleSet.boxes([[0.0, 0.0, 0.0]], [BOX_HALF])
    mesh = collision.TriangleMesh(*mr.cube(BOX_HALF))
    return collision.SdfGrid.from_obstacles(box, BOX_O, BOX_H, BOX_N), collision.SdfGrid.from_mesh(mesh, BOX_O, BOX_H, BOX_N, precision=precision)


def test_from_mesh_of_a_cube_is_from_obstacles_of_the_box(require_gpu):
    torch = pytest.importorskip("torch")
    from test_collision_host import robot_of
    from test_gpu_grid import compare32, dev_all, make_case
    from test_grid_host import masked_cotangent
    from test_obstacle_host import obstacle_inputs

    want, got = _box_grids()
    assert got.shape == want.shape == BOX_N and np.array_equal(got.origin, want.origin) and np.array_equal(got.spacing, want.spacing)
    ulp = np.spacing(np.abs(want.values))
    worst = float((np.abs(got.values.astype(np.float64) - want.values) / ulp).max())
    print(f"from_mesh(cube) against from_obstacles(box) on 17^3: {int((got.values != want.values).sum())} of {want.values.size} samples differ, "
          f"by at most {worst:.1f} float32 ulp (gate 1)")
    assert worst <= 1.0 and (got.values < 0).any() and (got.values > 0).any()
    # the penalty of a robot on both grids, each within the float32 gate of the grid tests against the yardstick of the box's grid
    name = "allegro_hand_right"
    d = obstacle_inputs(name)
    gd = masked_cotangent(name, "A")
    ref = make_case(d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"], want, d["pos"], d["rot"], np.where(gd == 0, 1.0, gd), d["margin"])
    assert (ref["r64"]["E"] > 0).any()
    model = robot_of(name)[0].sphere_model(d["sset"])
    for tag, grid in (("from_obstacles", want), ("from_mesh", got)):
        compare32(f"{name} on the {tag} grid", dev_all(model, grid, torch, d["q"], ref["gd"], d["margin"], None, d["pos"], d["rot"]), ref["r64"], ref["r32"])
    qt, pt, rt = (torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda") for a in (d["q"], d["pos"], d["rot"]))
    Ea, ga = collision.robot_grid_penalty(robot_of(name)[0], qt, d["sset"], want, d["margin"], pt, rt)
    Eb, gb = collision.robot_grid_penalty(robot_of(name)[0], qt, d["sset"], got, d["margin"], pt, rt)
    print(f"grid_penalty on the two grids: max |E difference| = {float((Ea - Eb).abs().max()):.3e} of max E {float(Ea.max()):.3e}, "
          f"max |gradient difference| = {float((ga - gb).abs().max()):.3e} of {float(ga.abs().max()):.3e}")
    assert bool((Ea > 0).any())


def test_from_mesh_float32_is_float64_within_the_float32_gate_and_fits_its_box(require_gpu):
    pytest.importorskip("torch")
    g64, g32 = _box_grids()[1], _box_grids("float32")[1]
    v, f = mr.cube(BOX_HALF)
    pts = mr.grid_points(BOX_N, np.full(3, BOX_O), np.full(3, BOX_H))
    r64, r32 = mr.sdf(v, f, pts)[0], mr.sdf(v, f, _r32(pts), np.float32)[0]
    a64, a32 = np.abs(g64.values.reshape(-1).astype(np.float64)), np.abs(g32.values.reshape(-1).astype(np.float64))
    dist = float(np.abs(np.abs(r32) - np.abs(r64)).max())  # (holds the rounding of the coordinates to float32 as well)
    e32, e64 = float(np.abs(a32 - np.abs(r64)).max()), float(np.abs(a64 - np.abs(r64.astype(np.float32).astype(np.float64))).max())
    print(f"from_mesh float32: max ||d| - |reference64|| = {e32:.3e}, the reference's float32 run is {dist:.3e} away (ratio {e32 / dist:.2f}, "
          f"gate {GATE32:g}); float64: {e64:.3e} from the rounded reference")
    assert e32 <= GATE32 * dist and e64 <= np.spacing(np.float32(0.2)) and np.array_equal(g64.values < 0, g32.values < 0)
    # the fitted box: an icosphere with padding
    mesh = collision.TriangleMesh(*mr.icosphere(2))
    g = collision.SdfGrid.from_mesh(mesh, spacing=[0.01, 0.0125, 0.02], padding=0.015)
    lo, hi = mesh.bounds
    assert np.array_equal(g.origin, lo - 0.015) and g.shape == tuple(int(k) + 1 for k in np.ceil((hi - lo + 0.03) / g.spacing))
    ref = mr.sdf(*mr.icosphere(2), mr.grid_points(g.shape, g.origin, g.spacing))[0]
    assert np.abs(g.values.reshape(-1) - ref).max() <= GATE64 + np.spacing(np.float32(0.1)) and (g.values < 0).any()


def test_open_and_inside_out_meshes_need_allow_open(require_gpu):
    pytest.importorskip("torch")
    v, f = mr.cube(BOX_HALF)
    inside_out, open_mesh = collision.TriangleMesh(v, f[:, ::-1]), collision.TriangleMesh(*mr.open_icosphere())
    for p in ("float64", "float32"):
        with pytest.raises(ValueError, match="inside out"):
            collision.SdfGrid.from_mesh(inside_out, BOX_O, BOX_H, BOX_N, precision=p)
        with pytest.raises(ValueError, match="not closed"):
            collision.SdfGrid.from_mesh(open_mesh, BOX_O, BOX_H, BOX_N, precision=p)
        g = collision.SdfGrid.from_mesh(inside_out, BOX_O, BOX_H, BOX_N, precision=p, allow_open=True)
        assert (g.values >= 0).all()  # what the refusal is for: every sample positive
        # ... and the same distances: turned faces have other records (a and c change places), so not the same bits, but each run is
        # within its gate of the yardstick on the cube as it was
        pts = mr.grid_points(BOX_N, np.full(3, BOX_O), np.full(3, BOX_H))
        r64 = np.abs(mr.sdf(v, f, pts)[0])
        gate = GATE64 + np.spacing(np.float32(0.2)) if p == "float64" else GATE32 * float(np.abs(np.abs(mr.sdf(v, f, _r32(pts), np.float32)[0]) - r64).max())
        assert np.abs(g.values.reshape(-1).astype(np.float64) - r64).max() <= gate
        g = collision.SdfGrid.from_mesh(open_mesh, BOX_O, BOX_H, BOX_N, precision=p, allow_open=True)
        assert (g.values < 0).any() and (g.values > 0).any()


# ---- 8. the torch front --------------------------------------------------------------------------------------------------------------------
def test_mesh_distances_front(require_gpu):
    torch = pytest.importorskip("torch")
    c = case("open2")
    mesh = c["mesh"]
    p = torch.tensor(c["p"][:20].reshape(4, 5, 3), dtype=torch.float32, device="cuda")
    raw_d, raw_w = dev(torch, mesh, c["p"][:20])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d = collision.mesh_distances(mesh, p)
        d2, w2 = collision.mesh_distances(mesh, p.clone().requires_grad_(True), winding=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert d.shape == (4, 5) and d.dtype == torch.float32 and not d.requires_grad and not d2.requires_grad and torch.equal(d, d2) and w2.shape == (4, 5)
    assert np.array_equal(d.cpu().numpy().reshape(-1), raw_d) and np.array_equal(w2.cpu().numpy().reshape(-1), raw_w)
    pn = torch.stack([p, p], 3)[..., 0]  # a view with the same values
    assert not pn.is_contiguous() and torch.equal(collision.mesh_distances(mesh, pn), d)
    assert torch.equal(collision.mesh_distances(mesh, p[0, 0]), d[0, 0]) and collision.mesh_distances(mesh, p[0, 0]).shape == ()
    e, ew = collision.mesh_distances(mesh, p[:0], winding=True)
    assert e.shape == (0, 5) and ew.shape == (0, 5)
    assert mesh.device_mesh(torch.cuda.current_device()) is mesh.device_mesh(torch.cuda.current_device())  # cached with the mesh


# ---- 9. argument errors through the raw ABI ------------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib, C = _lib.load(), _lib.C
    mesh = case("tet_5x7x9")["mesh"].device_mesh(torch.cuda.current_device())
    h = mesh.handle
    P = 8
    pts, dist, wind, vals = torch.zeros((P, 3), dtype=torch.float32, device="cuda"), _nan(torch, (P,)), _nan(torch, (P,)), _nan(torch, (2, 2, 2))

    def invalid(rc, word):
        assert rc == -1 and word in lib.dexr_last_error(), (rc, lib.dexr_last_error())

    D, G = lib.dexr_mesh_distances_dev, lib.dexr_mesh_sample_grid_dev
    invalid(D(None, P, pts.data_ptr(), dist.data_ptr(), wind.data_ptr(), None), b"null mesh")
    invalid(D(h, -1, pts.data_ptr(), dist.data_ptr(), wind.data_ptr(), None), b"negative")
    invalid(D(h, P, None, dist.data_ptr(), wind.data_ptr(), None), b"points is NULL")
    invalid(D(h, P, pts.data_ptr(), None, wind.data_ptr(), None), b"dist_out is NULL")
    assert D(h, 0, None, None, None, None) == 0 and lib.dexr_mesh_distances(h, 0, None, None, None) == 0  # P = 0: a no-op
    i3 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    d3 = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (3,))).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ok_n, ok_o, ok_h = np.array([2, 2, 2], np.int32), np.zeros(3), np.full(3, 0.01)
    keep = []  # (the arrays behind the pointers stay alive)

    def grid_rc(n, o, s, out=vals.data_ptr(), mesh_h=h):
        a, b, c_ = np.ascontiguousarray(n, np.int32), np.ascontiguousarray(np.broadcast_to(np.asarray(o, np.float64), (3,))), \
            np.ascontiguousarray(np.broadcast_to(np.asarray(s, np.float64), (3,)))
        keep.append((a, b, c_))
        return G(mesh_h, a.ctypes.data_as(C.POINTER(C.c_int32)), b.ctypes.data_as(C.POINTER(C.c_double)), c_.ctypes.data_as(C.POINTER(C.c_double)), out, None)

    invalid(grid_rc(ok_n, ok_o, ok_h, mesh_h=None), b"null mesh")
    invalid(grid_rc(ok_n, ok_o, ok_h, out=None), b"null")
    invalid(G(h, None, d3(0.0), d3(0.01), vals.data_ptr(), None), b"null")
    for n in ((1, 2, 2), (2, 2, 1), (1025, 2, 2)):
        invalid(grid_rc(n, ok_o, ok_h), b"dimension")
    invalid(grid_rc((1024, 1024, 17), ok_o, ok_h), b"samples")
    for bad in (0.0, -0.01, np.nan, np.inf, 1e-320):
        invalid(grid_rc(ok_n, ok_o, [0.01, bad, 0.01]), b"spacing")
    for bad in (np.nan, np.inf, -np.inf):
        invalid(grid_rc(ok_n, [0.0, 0.0, bad], ok_h), b"origin")
    z = np.zeros(8, np.float32)
    assert lib.dexr_mesh_sample_grid(h, i3((2, 2, 0)), d3(0.0), d3(0.01), z.ctypes.data_as(C.POINTER(C.c_float))) == -1
    zp, zd = np.zeros((P, 3)), np.full(P, np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    invalid(lib.dexr_mesh_distances(None, P, dp(zp), dp(zd), None), b"null mesh")
    invalid(lib.dexr_mesh_distances(h, -2, dp(zp), dp(zd), None), b"negative")
    invalid(lib.dexr_mesh_distances(h, P, None, dp(zd), None), b"points is NULL")
    invalid(lib.dexr_mesh_distances(h, P, dp(zp), None, None), b"dist_out is NULL")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dist, wind, vals)) and np.isnan(zd).all()  # nothing was launched
    nv, nt, b = C.c_int32(), C.c_int32(), np.zeros(6)
    assert lib.dexr_mesh_info(h, C.byref(nv), C.byref(nt), dp(b)) == 0 and (nv.value, nt.value) == (4, 4) and lib.dexr_mesh_info(h, None, None, None) == 0
    assert np.array_equal(b.reshape(2, 3), case("tet_5x7x9")["mesh"].bounds)
    with pytest.raises(ValueError, match="shape"):
        mesh.distances(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="shape"):
        mesh.sample_grid((2, 2), 0.0, 0.01)
    with pytest.raises(_lib.DexrError, match="dimension"):
        mesh.sample_grid((2, 2, 1), np.zeros(3), np.full(3, 0.01))

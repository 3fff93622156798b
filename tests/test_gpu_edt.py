"""GPU tests of the distance transform (csrc/dexr_distance_transform.hpp, include/dexr_distance_transform.h) and of the grid that lives
on the device (include/dexr_sdf_grid_dev.h, collision.DeviceSdfGrid), against tests/edt_reference.py on the grids and clouds of
tests/test_edt_host.py (whose reference runs are computed once there and shared).

GATES.  count and d2 are integers and must EQUAL the yardstick's.  The float32 samples lie within 1 float32 ulp of the yardstick's:
both sides compute in float64 from identical integers and round once, so they differ by float64 roundings (the square root), which
move a result across at most one float32 rounding boundary.  The geometric bound is derived in test_edt_host.box_bound.  Whatever
compares two runs of the kernels -- permutations, dropped points, host against device entries, a device grid against a host grid of
the same samples -- is bit for bit."""
import os

import numpy as np
import pytest

import edt_reference as er
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_edt_host import (BOX_C, BOX_E, BOX_H, BOX_N, BOX_O, CLOUDS, GRIDS, H, ORIGIN, box_bound, box_cloud, cloud, cloud_reference, duplicate_cloud,
                           exact_cloud)
from test_obstacle_host import obstacle_inputs

pytestmark = pytest.mark.gpu


def _dev(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _ws(torch, n):
    return torch.empty(_lib.edt_workspace_bytes(n), dtype=torch.uint8, device="cuda")


def dev_points(torch, p, n, origin=ORIGIN, h=H, min_points=1, radius=0.0, max_distance=None, want=(True, True)):
    """the device entry on a numpy cloud, every output pre-filled with what no run writes -> (values, d2 or None, count or None), numpy"""
    md = er.default_max_distance(n, h) if max_distance is None else max_distance
    pt = _dev(torch, np.asarray(p, np.float32).reshape(-1, 3))
    v = torch.full(n, float("nan"), dtype=torch.float32, device="cuda")
    d2 = torch.full(n, -7, dtype=torch.int32, device="cuda") if want[0] else None
    c = torch.full(n, -7, dtype=torch.int32, device="cuda") if want[1] else None
    ws = _ws(torch, n)
    _lib.edt_points_dev(pt.data_ptr() if len(pt) else 0, len(pt), n, origin, h, min_points, radius, md, v.data_ptr(), 0 if d2 is None else d2.data_ptr(),
                        0 if c is None else c.data_ptr(), ws.data_ptr(), ws.numel(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return v.cpu().numpy(), None if d2 is None else d2.cpu().numpy(), None if c is None else c.cpu().numpy()


def dev_occupancy(torch, occ, h=H, signed=False, radius=0.0, max_distance=None):
    n = tuple(occ.shape)
    md = er.default_max_distance(n, h) if max_distance is None else max_distance
    ot = _dev(torch, np.asarray(occ, np.uint8))
    v = torch.full(n, float("nan"), dtype=torch.float32, device="cuda")
    d2 = torch.full(n, -7, dtype=torch.int32, device="cuda")
    ws = _ws(torch, n)
    _lib.edt_occupancy_dev(ot.data_ptr(), n, h, signed, radius, md, v.data_ptr(), d2.data_ptr(), ws.data_ptr(), ws.numel(),
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return v.cpu().numpy(), d2.cpu().numpy()


def check_values(tag, got, want):
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), tag
    u = int(er.ulp_distance(got, want).max())
    print(f"{tag}: the samples are at most {u} float32 ulp from the reference's (gate 1)")
    assert u <= 1, tag


# ---- 1. count and d2 bit for bit, the samples within one ulp, on every grid and cloud ---------------------------------------------------
@pytest.mark.parametrize("kind", CLOUDS)
@pytest.mark.parametrize("n", GRIDS, ids=lambda n: "x".join(map(str, n)))
def test_clouds_against_the_reference(n, kind, require_gpu):
    torch = pytest.importorskip("torch")
    radius = H * np.sqrt(3) / 2
    want_v, want_d2, want_c = cloud_reference(kind, n, 1, radius)
    v, d2, c = dev_points(torch, cloud(kind, n), n, radius=radius)
    assert c.dtype == np.int32 and np.array_equal(c, want_c) and d2.dtype == np.int32 and np.array_equal(d2, want_d2)
    check_values(f"{n} {kind}", v, want_v)
    if kind == "empty":
        md = er.default_max_distance(n, H)
        assert (d2 == _lib.EDT_NONE).all() and (v == np.float32(md - radius)).all()
    # the optional outputs are optional: the same samples without them
    v2, _, _ = dev_points(torch, cloud(kind, n), n, radius=radius, want=(False, False))
    assert np.array_equal(v2, v)


def test_exact_cloud_duplicates_and_a_clamp_that_bites(require_gpu):
    torch = pytest.importorskip("torch")
    n = (5, 7, 9)
    p, k = exact_cloud(n)
    want = er.from_points(p, n, (0, 0, 0), 2.0 ** -6)
    got = dev_points(torch, p, n, origin=(0, 0, 0), h=2.0 ** -6)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and got[2].sum() == len(p) and (got[2][tuple(k.T)] > 0).all()
    check_values("exact", got[0], want[0])
    p, idx, reps = duplicate_cloud(n)
    for mp in (1, 2, 3, 4):
        want = er.from_points(p, n, ORIGIN, H, min_points=mp)
        got = dev_points(torch, p, n, min_points=mp)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[1][tuple(idx.T)] == 0, reps >= mp)  # exactly the voxels with mp points or more are occupied
        check_values(f"min_points {mp}", got[0], want[0])
    assert (got[1] == _lib.EDT_NONE).all()  # (no voxel holds four points)
    want = er.from_points(p, n, ORIGIN, H, radius=0.002, max_distance=0.025)
    got = dev_points(torch, p, n, radius=0.002, max_distance=0.025)
    check_values("clamped", got[0], want[0])
    clamped = want[1] * H * H > 0.025 ** 2 * 1.001  # the samples clearly past the clamp, by the reference's integers
    assert clamped.any() and (got[0][clamped] == np.float32(0.025 - 0.002)).all() and got[0].max() == np.float32(0.025 - 0.002)


@pytest.mark.parametrize("n", [(2, 2, 2), (5, 7, 9), (33, 17, 9), (3, 65, 4)], ids=lambda n: "x".join(map(str, n)))
def test_occupancy_unsigned_and_signed(n, require_gpu):
    torch = pytest.importorskip("torch")
    _, want_d2, count = cloud_reference("seeded", n)
    occ = (count >= 1).astype(np.uint8) * 3  # nonzero is occupied
    v, d2 = dev_occupancy(torch, occ, radius=0.001)
    assert np.array_equal(d2, want_d2)  # the d2 of the cloud that produces this occupancy
    assert np.array_equal(v, dev_points(torch, cloud("seeded", n), n, radius=0.001)[0])
    md = er.default_max_distance(n, H)
    for tag, o in (("seeded", occ), ("all free", np.zeros(n, np.uint8)), ("all occupied", np.ones(n, np.uint8)),
                   ("one free", np.where(np.arange(int(np.prod(n))).reshape(n) == 1, 0, 1).astype(np.uint8))):
        want_v, to_occ, _ = er.signed_values(o != 0, H, md)
        v, d2 = dev_occupancy(torch, o, signed=True)
        assert np.array_equal(d2, to_occ), tag
        check_values(f"{n} signed {tag}", v, want_v)
        assert ((v < 0) == (o != 0)).all()
    assert (v[o != 0] < 0).all() and v.min() >= -np.float32(md)


# ---- 2. independence: the order of the points, dropped points, the entry ---------------------------------------------------------------
def test_outputs_do_not_depend_on_order_dropped_points_or_the_entry(require_gpu):
    torch = pytest.importorskip("torch")
    n = (33, 17, 9)
    p = cloud("seeded", n)
    base = dev_points(torch, p, n, radius=0.003)
    perm = np.random.default_rng(1).permutation(len(p))
    lo, hi = np.asarray(ORIGIN), np.asarray(ORIGIN) + (np.asarray(n) - 1) * H
    mid = (lo + hi) / 2
    dropped = [[np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]], [mid[0], mid[1], -np.inf], [np.nan, np.nan, np.nan]]
    for a in range(3):  # one voxel outside each face
        for edge, sign in ((lo, -1.0), (hi, 1.0)):
            q = mid.copy()
            q[a] = edge[a] + sign * H
            dropped.append(q)
    more = np.concatenate([p[:100], np.asarray(dropped, np.float32), p[100:]])
    for tag, q in (("permuted", p[perm]), ("with dropped points", more)):
        got = dev_points(torch, q, n, radius=0.003)
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), tag
    host = _lib.edt_points(p, n, ORIGIN, H, 1, 0.003, er.default_max_distance(n, H))
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(host, base))
    empty = _lib.edt_points(np.zeros((0, 3), np.float32), n, ORIGIN, H, 1, 0.0, 0.5)
    assert (empty[0] == 0.5).all() and (empty[1] == _lib.EDT_NONE).all() and not empty[2].any()
    occ = (base[2] >= 1).astype(np.uint8)
    for signed in (False, True):
        hv, hd = _lib.edt_occupancy(occ, H, signed, 0.0, 0.3)
        dv, dd = dev_occupancy(torch, occ, signed=signed, max_distance=0.3)
        assert np.array_equal(hv, dv) and np.array_equal(hd, dd) and np.array_equal(hd, base[1])


# ---- 3. against geometry ------------------------------------------------------------------------------------------------------------------
def test_a_box_of_points_against_the_box_primitive(require_gpu):
    torch = pytest.importorskip("torch")
    cloud_grid = collision.SdfGrid.from_points(_dev(torch, box_cloud()), BOX_O, BOX_H, BOX_N, radius=0.0)
    box = collision.SdfGrid.from_obstacles(collision.ObstacleSet.boxes(BOX_C[None], BOX_E[None]), BOX_O, BOX_H, BOX_N)
    assert type(cloud_grid) is collision.SdfGrid and cloud_grid.shape == BOX_N and np.array_equal(cloud_grid.spacing, box.spacing)
    out = box.values > 0
    err = float(np.abs(cloud_grid.values.astype(np.float64) - box.values)[out].max())
    print(f"max |v_cloud - v_box| outside the box = {err:.5f} (bound {box_bound():.5f})")
    assert err <= box_bound()
    check_values("box", cloud_grid.values, er.from_points(box_cloud(), BOX_N, BOX_O, BOX_H)[0])
    # the default radius: never more than the true distance to the nearest kept point
    safe = collision.SdfGrid.from_points(_dev(torch, box_cloud()), BOX_O, BOX_H, BOX_N)
    check_values("box, default radius", safe.values, er.from_points(box_cloud(), BOX_N, BOX_O, BOX_H, radius=BOX_H * np.sqrt(3) / 2)[0])
    d_true = np.linalg.norm(np.stack(np.meshgrid(*[BOX_O[a] + np.arange(BOX_N[a]) * BOX_H for a in range(3)], indexing="ij"), -1)[..., None, :]
                            - box_cloud().astype(np.float64), axis=-1).min(-1)
    assert (safe.values <= d_true + 1e-7).all()
    occ = _dev(torch, (box.values <= 0).astype(np.uint8))
    signed = collision.SdfGrid.from_occupancy(occ, BOX_O, BOX_H)
    check_values("box occupancy", signed.values, er.signed_values(box.values <= 0, BOX_H, er.default_max_distance(BOX_N, BOX_H))[0])
    assert ((signed.values < 0) == (box.values <= 0)).all()


# ---- 4. the grid that lives on the device ---------------------------------------------------------------------------------------------------
GRID_N, GRID_H, GRID_O = (17, 17, 17), 0.01, -0.08
MARGIN = 0.01


def hand_clouds():
    rng = np.random.default_rng(23)
    out = []
    for r in (0.03, 0.045):
        u = rng.standard_normal((400, 3))
        out.append((u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0, r, (400, 1))).astype(np.float32))
    return out


def test_device_grid_feeds_every_consumer_like_a_host_grid_of_its_samples(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, "teleop/allegro_hand_right.yml")).build().optimizer
    d = obstacle_inputs("allegro_hand_right")
    sset = d["sset"]
    q, pos, rot = (_dev(torch, np.asarray(d[k], np.float32)) for k in ("q", "pos", "rot"))
    assert q.shape == (33, opt.opt_dof)
    p1, p2 = (_dev(torch, p) for p in hand_clouds())
    dev = collision.DeviceSdfGrid.from_points(p1, GRID_O, GRID_H, GRID_N)
    snap = dev.to_host()
    host = collision.SdfGrid(snap.values, snap.origin, snap.spacing)
    assert type(snap) is collision.SdfGrid and isinstance(dev, collision.SdfGrid) and dev.shape == host.shape == GRID_N
    assert np.array_equal(dev.origin, host.origin) and np.array_equal(dev.spacing, host.spacing) and dev.device_index == torch.cuda.current_device()
    check_values("hand cloud", snap.values, er.from_points(p1.cpu().numpy(), GRID_N, (GRID_O,) * 3, GRID_H, radius=GRID_H * np.sqrt(3) / 2)[0])

    def same(a, b):
        return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))

    on_dev = collision.grid_penalty(opt, q, sset, dev, MARGIN, pos, rot, wrench=True)
    on_host = collision.grid_penalty(opt, q, sset, host, MARGIN, pos, rot, wrench=True)
    assert same(on_dev, on_host) and bool((on_host[0] > 0).any()) and float(on_host[1].abs().max()) > 0
    assert torch.equal(collision.grid_distances(opt, q, sset, dev, pos, rot), collision.grid_distances(opt, q, sset, host, pos, rot))
    kw = dict(obstacle_pos=pos, obstacle_rot=rot, damping=1e-4, max_iters=4)
    r_dev = collision.resolve_grid_collisions(opt, q, sset, dev, MARGIN, **kw)
    r_host = collision.resolve_grid_collisions(opt, q, sset, host, MARGIN, **kw)
    assert same(r_dev, r_host) and not torch.equal(r_host[0], q)
    s_dev = collision.resolve_scene_collisions(opt, q, sset, [collision.SceneBody(dev, pos, rot)], MARGIN, damping=1e-4, max_iters=4)
    s_host = collision.resolve_scene_collisions(opt, q, sset, [collision.SceneBody(host, pos, rot)], MARGIN, damping=1e-4, max_iters=4)
    assert same(s_dev, s_host) and not torch.equal(s_host[0], q)
    grads = []
    for g in (dev, host):
        qg = q.clone().requires_grad_(True)
        ag.grid_penalty(opt, qg, sset, g, MARGIN, pos, rot).sum().backward()
        grads.append(qg.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], on_host[1])
    # an update and its consumer back to back on one side stream, no synchronise in between: the penalty sees the new samples
    fresh = collision.DeviceSdfGrid.from_points(p2, GRID_O, GRID_H, GRID_N)
    want = collision.grid_penalty(opt, q, sset, fresh, MARGIN, pos, rot, wrench=True)
    assert not torch.equal(want[0], on_host[0])
    # (a stream of torch's high-priority pool: it is as non-default as any, and it leaves alone the default pool's round-robin
    # position and the hardware queues of the default priority, on which the timing tests later in the suite depend)
    side = torch.cuda.Stream(priority=-1)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.update_from_points(p2)
        got = collision.grid_penalty(opt, q, sset, dev, MARGIN, pos, rot, wrench=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert same(got, want) and np.array_equal(dev.to_host().values, fresh.to_host().values)
    # ... and back, through an occupancy map of the first cloud's voxels, unsigned with the cloud's radius: the first samples again
    occ = _dev(torch, (er.voxelise(p1.cpu().numpy(), GRID_N, (GRID_O,) * 3, GRID_H) >= 1).astype(np.uint8))
    dev.update_from_occupancy(occ, signed=False, radius=GRID_H * np.sqrt(3) / 2)
    assert np.array_equal(dev.to_host().values, snap.values)
    # what a device grid refuses
    other = torch.cuda.current_device() + 1
    with pytest.raises(ValueError, match=f"cuda:{other - 1}.*cuda:{other}"):
        dev.device_grid(other)
    with pytest.raises(ValueError, match="to_host"):
        collision.fit_spheres(dev, 4)
    with pytest.raises(AttributeError, match="to_host"):
        dev.values
    assert dev == dev and dev != fresh and len({dev, fresh}) == 2
    # an empty 2x2x2 grid is a grid of zeros
    e_dev = collision.DeviceSdfGrid.empty((2, 2, 2), GRID_O, GRID_H)
    e_host = collision.SdfGrid(np.zeros((2, 2, 2), np.float32), GRID_O, GRID_H)
    assert not e_dev.to_host().values.any()
    assert torch.equal(collision.grid_distances(opt, q, sset, e_dev, pos, rot), collision.grid_distances(opt, q, sset, e_host, pos, rot))


def test_raw_grid_handle_copies_device_samples_and_serves_any_consumer(require_gpu):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(2)
    v = rng.standard_normal((3, 4, 5)).astype(np.float32)
    vt = _dev(torch, v)
    st = torch.cuda.current_stream().cuda_stream
    g = _lib.DeviceSdfGrid((3, 4, 5), np.zeros(3), np.full(3, 0.1), vt.data_ptr(), st)
    assert g.shape == (3, 4, 5) and g.values_ptr and isinstance(g, _lib.SdfGrid) and np.array_equal(g.download(st), v)
    z = _lib.DeviceSdfGrid((3, 4, 5), np.zeros(3), np.array([0.1, 0.2, 0.3]))
    assert not z.download().any()
    n, o, h = np.zeros(3, np.int32), np.zeros(3), np.zeros(3)
    C = _lib.C
    _lib.check(_lib.load().dexr_sdf_grid_info(z.handle, n.ctypes.data_as(C.POINTER(C.c_int32)), o.ctypes.data_as(C.POINTER(C.c_double)),
                                              h.ctypes.data_as(C.POINTER(C.c_double))))
    assert n.tolist() == [3, 4, 5] and h.tolist() == [0.1, 0.2, 0.3]

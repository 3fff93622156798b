"""GPU tests of the sphere fit kernels (include/dexr_sphere_fit.h) against tests/sphere_fit_reference.py.  Everything compared is an
integer -- flat indices, gains, counts -- so every comparison is np.array_equal: there is no tolerance.  The bodies are the smallest
at which each part can go wrong (tests/test_sphere_fit_host.py keeps their samples clear of the surface): odd sizes and a ragged last
chunk (5 x 7 x 9), ties (the capsule), rows of a full word, a word plus one bit and half a word with spheres clipped by the grid's
faces (9 x 9 x 64 / 33 / 32), the limits (64 x 5 x 5, 2 x 2 x 2), interior samples without a candidate (the slab under min_radius),
reach past the shape (inflate), several bodies of different shape, spacing and sphere count in one call, the sphere limit, a NaN.

End to end: a URDF with a box, a cylinder, a sphere and an STL mesh becomes a SphereSet whose spheres lie inside their links, within
the gate tests/test_gpu_mesh.py applies to float64-arithmetic grids."""
import numpy as np
import pytest

import mesh_reference as mr
import sphere_fit_reference as sr
from dex_retargeting_amd import _lib, collision, meshio
from dex_retargeting_amd.robot_wrapper import RobotWrapper
from dex_retargeting_amd.urdf import parse_collision_geometry
from test_gpu_mesh import GATE64

pytestmark = pytest.mark.gpu
H12 = 0.004  # the spacing of box_12x10x11

# (body, k, min_radius, inflate, coverage)
CASES = [
    ("tet_5x7x9", 8, 0.0, 0.0, 1.0), ("capsule17", 8, 0.0, 0.0, 1.0), ("cube_9x9x64", 16, 0.0, 0.0, 1.0), ("cube_9x9x33", 16, 0.0, 0.0, 1.0),
    ("cube_9x9x32", 16, 0.0, 0.0, 1.0), ("box_64x5x5", 16, 0.0, 0.0, 1.0), ("box_2x2x2", 4, 0.0, 0.0, 1.0), ("slab", 4, 0.005, 0.0, 1.0),
    ("slab", 8, 0.0, 0.0, 1.0), ("slab", 8, 0.0, 0.01, 1.0), ("box_12x10x11", 16, 0.0, 0.0, 1.0), ("box_12x10x11", 16, 0.0, H12, 1.0),
    ("box_12x10x11", 16, 0.012, 0.0, 1.0), ("box_12x10x11", 16, 0.0, 0.0, 0.45), ("box_12x10x11", 16, 0.0, 0.0, 0.0), ("outside", 4, 0.0, 0.0, 1.0),
    ("box_12x10x11", _lib.SPHERE_MAX, 0.0, 0.0, 1.0), ("box_2x2x2", _lib.SPHERE_MAX, 0.0, 0.0, 1.0),
]


def _host(names, k, min_radius=0.0, inflate=0.0, coverage=1.0, values=None):
    """the host entry on the named bodies in one call -> (index, gain, count)"""
    bodies = [sr.body(n) for n in names]
    vals = [b["values"] for b in bodies] if values is None else values
    sizes = [v.size for v in vals]
    return _lib.sphere_fit([v.shape for v in vals], [b["h"] for b in bodies], np.concatenate([[0], np.cumsum(sizes)[:-1]]), k, min_radius, inflate,
                           coverage, np.concatenate([v.reshape(-1) for v in vals]))


def _padded(ref, k_max):
    """a body's reference (index, gain, count) as its rows of a call whose largest sphere count is k_max"""
    index, gain, count = ref
    return (np.concatenate([index, np.full(k_max - len(index), -1, np.int32)]), np.concatenate([gain, np.zeros(k_max - len(gain), np.int32)]), count)


def _assert_equal(tag, got, want):
    for name, g, w in zip(("index", "gain", "count"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), f"{tag}: {name}\n got  {g.tolist()}\n want {w.tolist()}"


@pytest.mark.parametrize("name,k,min_radius,inflate,coverage", CASES)
def test_one_body_is_the_reference(name, k, min_radius, inflate, coverage, require_gpu):
    want = sr.expected(name, k, min_radius, inflate, coverage)
    index, gain, count = _host([name], [k], min_radius, inflate, coverage)
    print(f"{name} k = {k} min_radius = {min_radius} inflate = {inflate} coverage = {coverage}: {count[0].tolist()} (interior, covered, spheres), "
          f"gains {gain[0, :8].tolist()}")
    assert index.shape == gain.shape == (1, k) and count.shape == (1, 3)
    _assert_equal(name, (index[0], gain[0], count[0]), want)


def test_the_cases_reach_what_they_are_for():
    """(CPU arithmetic on the shared references: the shapes above do exercise the paths they are named for)"""
    assert sr.expected("slab", 4, 0.005, 0.0, 1.0)[2].tolist() == [36, 0, 0]  # interior, no candidate
    assert sr.expected("capsule17", 8)[1][:3].tolist() == [81, 81, 81]  # ties
    for nz in (64, 33, 32):
        index, gain, count = sr.expected(f"cube_9x9x{nz}", 16)
        iz = index[index >= 0] % nz
        assert iz.min() <= 2 and iz.max() >= nz - 3 and count[2] == 16  # spheres clipped by both faces along z, every round runs
    assert sr.expected("box_12x10x11", 16, 0.0, 0.0, 0.45)[2][2] < 16 and sr.expected("box_12x10x11", 16, 0.0, 0.0, 0.0)[2][2] == 0
    full = sr.expected("box_12x10x11", _lib.SPHERE_MAX)
    assert full[2][2] == _lib.SPHERE_MAX and full[2][1] < full[2][0] and full[1][-1] >= 1  # every one of the 128 rounds takes a sphere
    assert sr.expected("box_2x2x2", _lib.SPHERE_MAX)[2].tolist() == [8, 8, 2]
    assert sr.body("tet_5x7x9")["values"].size % _lib.SPHERE_FIT_CHUNK != 0 and sr.body("capsule17")["values"].size > 4 * _lib.SPHERE_FIT_CHUNK


def test_bodies_of_different_shape_spacing_and_count_share_one_call(require_gpu):
    names, k = ["box_2x2x2", "cube_9x9x64", "tet_5x7x9", "outside", "box_12x10x11"], [1, 16, 3, 5, 7]
    assert len({sr.body(n)["h"] for n in names}) >= 3 and len({sr.body(n)["values"].shape for n in names}) == len(names)
    index, gain, count = _host(names, k)
    assert index.shape == (5, 16) and count[0, 2] == 1 and count[1, 2] == 16 and count[3].tolist() == [0, 0, 0]
    for b, (n, kb) in enumerate(zip(names, k)):
        _assert_equal(f"{n} among five", (index[b], gain[b], count[b]), _padded(sr.expected(n, kb), 16))
        alone = _host([n], [kb])
        _assert_equal(f"{n} alone", (alone[0][0], alone[1][0], alone[2][0]), sr.expected(n, kb))
    # the order of the bodies does not matter
    back = _host(names[::-1], k[::-1])
    _assert_equal("reversed", tuple(a[::-1] for a in back), (index, gain, count))


def test_a_nan_sample_is_not_interior_and_spoils_nothing_else(require_gpu):
    b = sr.body("box_12x10x11")
    full = sr.expected("box_12x10x11", 16)
    v = b["values"].copy()
    v[np.unravel_index(np.argmax(v), v.shape)] = np.nan  # outside the body
    got = _host(["box_12x10x11"], [16], values=[v])
    _assert_equal("a NaN outside", tuple(a[0] for a in got), full)
    v[np.unravel_index(full[0][0], v.shape)] = np.nan  # the first winner's own sample
    got = _host(["box_12x10x11"], [16], values=[v])
    _assert_equal("a NaN inside", tuple(a[0] for a in got), sr.fit(v, b["h"], 16))
    assert got[2][0, 0] == full[2][0] - 1 and got[0][0, 0] != full[0][0]


def test_device_entry_is_the_host_entry_and_the_workspace_is_reusable(require_gpu):
    torch = pytest.importorskip("torch")
    names, k = ["capsule17", "box_64x5x5", "box_2x2x2"], [8, 16, 4]
    want = _host(names, k)
    bodies = [sr.body(n) for n in names]
    dims = np.array([b["values"].shape for b in bodies], np.int32)
    sizes = [b["values"].size for b in bodies]
    offset = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    values = torch.from_numpy(np.concatenate([b["values"].reshape(-1) for b in bodies])).cuda()
    ws_bytes = _lib.sphere_fit_workspace_bytes(dims)
    big = _lib.sphere_fit_workspace_bytes([[17, 17, 17], [64, 5, 5], [9, 9, 64]])
    ws = torch.full((max(ws_bytes, big),), 0xA5, dtype=torch.uint8, device="cuda")  # (contents irrelevant)
    stream = torch.cuda.current_stream().cuda_stream

    def run(k_of, vals, d, off, h):
        out = [torch.full((len(k_of), max(k_of)), 77, dtype=torch.int32, device="cuda") for _ in range(2)] + \
            [torch.full((len(k_of), 3), 77, dtype=torch.int32, device="cuda")]
        _lib.sphere_fit_dev(d, h, off, k_of, 0.0, 0.0, 1.0, vals.numel(), vals.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                            ws.data_ptr(), ws.numel(), stream=stream)
        torch.cuda.synchronize()
        return tuple(o.cpu().numpy() for o in out)

    spacing = [b["h"] for b in bodies]
    first = run(k, values, dims, offset, spacing)
    _assert_equal("device entry", first, want)
    # another set of bodies through the same workspace, then the first again
    other = sr.body("cube_9x9x64")
    ov = torch.from_numpy(other["values"].reshape(-1).copy()).cuda()
    got = run([16], ov, [other["values"].shape], [0], [other["h"]])
    _assert_equal("other bodies, same workspace", tuple(a[0] for a in got), sr.expected("cube_9x9x64", 16))
    _assert_equal("second call", run(k, values, dims, offset, spacing), first)
    # a body may start anywhere in the value buffer
    shifted = torch.cat([torch.full((5,), -1.0, device="cuda"), values])
    _assert_equal("offset", run(k, shifted, dims, offset + 5, spacing), first)


def test_fit_spheres_front(require_gpu):
    pytest.importorskip("torch")
    names, k = ["box_12x10x11", "outside", "capsule17"], [6, 3, 5]
    grids = [collision.SdfGrid(sr.body(n)["values"], sr.body(n)["origin"], sr.body(n)["h"]) for n in names]
    fits = collision.fit_spheres(grids, k, inflate=0.001)
    assert len(fits) == 3 and len(fits[1]) == 0 and fits[1].n_interior == 0 and fits[1].coverage == 1.0 and fits[1].centers.shape == (0, 3)
    for name, kb, g, fit in zip(names, k, grids, fits):
        index, gain, count = sr.expected(name, kb, 0.0, 0.001, 1.0)
        n = int(count[2])
        centers, radii = sr.spheres_of(g.values, g.origin, g.spacing[0], index, 0.001)
        assert len(fit) == n and np.array_equal(np.ravel_multi_index(tuple(fit.samples.T), g.shape), index[:n]) and np.array_equal(fit.gains, gain[:n])
        assert (fit.n_interior, fit.n_covered) == (count[0], count[1]) and fit.coverage == (count[1] / count[0] if count[0] else 1.0)
        assert np.array_equal(fit.centers, centers) and np.array_equal(fit.radii, radii) and fit.centers.dtype == fit.radii.dtype == np.float64
    one = collision.fit_spheres(grids[0], 6, inflate=0.001)
    assert len(one) == 1 and np.array_equal(one[0].centers, fits[0].centers)


def test_urdf_to_sphere_set_end_to_end(require_gpu, tmp_path):
    torch = pytest.importorskip("torch")
    path = sr.write_urdf(str(tmp_path))
    robot = RobotWrapper(path)
    max_dim = 20
    sset = collision.SphereSet.from_urdf(robot, path, spheres_per_link=4, max_dim=max_dim)
    assert sset.table_links == tuple(sr.URDF_LINKS) and 4 <= sset.n_sphere <= 16 and (sset.radii > 0).all()
    gate = GATE64 + np.spacing(np.float32(0.1))
    geo = parse_collision_geometry(path)
    for link in sr.URDF_LINKS:
        mesh = collision.TriangleMesh(*meshio.link_mesh(geo[link]), drop_degenerate=True)
        sel = np.array([n == link for n in sset.links])
        centers, radii = sset.centers[sel], sset.radii[sel]
        d = mr.sdf(mesh.vertices, mesh.faces, centers)[0]
        worst = float((d + radii).max())
        # the reference's fit of the same grid: the same spheres, the same coverage
        grid = collision.link_grid(mesh, max_dim)
        assert max(grid.shape) == max_dim and grid.spacing[0] == grid.spacing[1] == grid.spacing[2]
        index, gain, count = sr.fit(grid.values, grid.spacing[0], 4)
        fit = collision.fit_spheres(grid, 4)[0]
        want_c, want_r = sr.spheres_of(grid.values, grid.origin, grid.spacing[0], index)
        print(f"{link}: grid {grid.shape}, {len(radii)} spheres, radii {np.round(radii, 4).tolist()}, coverage {fit.coverage:.3f}, "
              f"max sdf(centre) + radius = {worst:.3e} (gate {gate:.3e})")
        assert worst <= gate  # inflate = 0: every sphere lies inside its link
        assert (fit.n_interior, fit.n_covered, len(fit)) == tuple(count) and fit.coverage == count[1] / count[0]
        assert np.array_equal(centers, want_c) and np.array_equal(radii, want_r)
    q = torch.zeros((3, robot.dof), dtype=torch.float32, device="cuda")
    q[1] = 0.4
    q[2] = -0.7
    d = collision.robot_sphere_distances(robot, q, sset)
    pairs = collision.default_pairs(robot, sset)
    assert d.shape == (3, len(pairs)) and len(pairs) > 0 and bool(torch.isfinite(d).all())
    # ... and the posture solve takes the set as it is: the README's path from a URDF to resolve_self_collision
    qr, iters, energy, status = collision.robot_resolve_self_collision(robot, q, sset, margin=0.005, damping=1e-4, max_iters=4)
    assert qr.shape == q.shape and bool(torch.isfinite(qr).all()) and bool(torch.isfinite(energy).all())
    # per-link counts, and a link whose fit is empty is named
    some = collision.SphereSet.from_urdf(robot, path, spheres_per_link={"palm": 6, "proximal": 2, "distal": 3, "tip": 1}, max_dim=max_dim)
    assert [some.links.count(n) for n in sr.URDF_LINKS] == [6, 2, 3, 1]
    with pytest.raises(ValueError, match="'tip'"):  # the tetrahedron is the one link without a sample 6 mm deep
        collision.SphereSet.from_urdf(robot, path, max_dim=max_dim, min_radius=0.006)

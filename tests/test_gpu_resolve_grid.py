"""GPU tests of the posture solve against a signed-distance grid (csrc/dexr_resolve_grid.hpp, include/dexr_resolve_grid.h): the
float64 host twin against tests/resolve_grid_reference.py, the float32 device entry point against the host twin, a distant grid
against dexr_sphere_resolve, the NULL pose, row independence and isolation, the smallest and an anisotropic grid, optimizer order,
the table limits with the header's byte formula and 128 spheres all in contact, the raw ABI's argument errors, the torch fronts and
retarget -> resolve against a held object given as a grid.

INPUTS and DECISION GUARDS: tests/test_resolve_grid_host.py (resolve_grid_inputs, reference; B = 33: three blocks of sixteen
frames, the last with one frame), whose reference runs are proven there on the CPU and shared from there.  A comparison against the
yardstick is made on the frames that are CLEAR at its guards -- its `gap` covers the cell faces of the active spheres too --; every
frame goes through the functional checks (finite, inside the limits, unread columns unchanged, the four-term E recomputed by the
yardstick in float64 does not rise).

GATES, those of tests/test_gpu_resolve.py: float64 1e-9 on x and the energies, iters and status equal; float32 max |x32 - x64| over
the clear frames at most GATE32 = 8 x the distance between the yardstick's own float32 and float64 runs there; E(answer) <= E(x0)
(1 + RISE), RISE = 1e-3 as derived there (the margins here are the same 1 cm, and a contact's h is formed from a distance of the same
size as a pair's)."""
import os

import numpy as np
import pytest

import grid_reference as gref
import ik_solve_reference as isr
import pose_zoo as zoo
import resolve_grid_reference as rgr
import resolve_reference as rr
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd import pose_tables as pt
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, ROBOTS, robot_of
from test_gpu_grid import awkward_grid
from test_gpu_resolve import GATE32, GATE64, RISE, _dev, _nan, _opt_case, _ptr, _target_case, compare64
from test_grid_host import grid_a
from test_resolve_grid_host import CASES, grid_problem, reference, reference_run, resolve_grid_inputs
from test_resolve_host import GUARD32, STEPS32, STEPS64, _f32, _r32
from test_resolve_obstacle_host import pose_seed, poses

pytestmark = pytest.mark.gpu
BITS = rgr.CONVERGED | rgr.STALLED | rgr.TRUNCATED  # DEXR_RESOLVE_CONTACTS_TRUNCATED is never set: not a known bit here
INVALID, UNSUPPORTED = -1, -3


def with_grid(d, grid, seed=None, far_every=4, **over):
    """a dict of another test's inputs with a grid and, with a seed, a pose per frame by the recipe of the host tests."""
    a = dict(d, grid=grid, omargin=d["margin"], wobs=1.0)
    if seed is not None:
        geo = dict(a, q=np.asarray(a["full"](a["q"]), np.float64)) if a.get("full") is not None else a
        a["pos"], a["rot"], a["far"] = poses(geo, seed, far_every)
    a.update(over)
    return a


def host_run(model, d, max_iters, fixed=None, **over):
    a = dict(d, **over)
    return model.resolve_grid(a["grid"].device_grid(0), a["q"], a["margin"], a["damping"], max_iters, fixed, a.get("x_ref"), a.get("u"),
                              a.get("tgt_pos"), a.get("tgt_rot"), a.get("w_pos"), a.get("w_rot"), a["wcol"], a.get("pair_weight"), a.get("lo"),
                              a.get("hi"), a["tol"], a["max_step"], n_target=a.get("n_target", 0), obstacle_pos=a.get("pos"),
                              obstacle_rot=a.get("rot"), obstacle_margin=a["omargin"], obstacle_weight=a["wobs"])


def dev_run(model, torch, d, max_iters, fixed=None, rows=slice(None), alias=False, **over):
    """-> (x, iters, energy, status) of dexr_sphere_resolve_grid_dev on the frames `rows` of d, the outputs pre-filled with NaN / -7;
    alias: x_out is x0's buffer."""
    a = dict(d, **over)
    cut = lambda v: None if v is None else v[rows]  # noqa: E731
    x0, tf, xr, tp, tr, wl, wa, op, orot = (_dev(torch, cut(v)) for v in (a["q"], fixed, a.get("x_ref"), a.get("tgt_pos"), a.get("tgt_rot"), a.get("w_pos"),
                                                                          a.get("w_rot"), a.get("pos"), a.get("rot")))
    u, pw, lo, hi = (_dev(torch, a.get(k)) for k in ("u", "pair_weight", "lo", "hi"))
    n = x0.shape[0]
    x = x0 if alias else _nan(torch, (n, model.n_in))
    iters, status = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    energy = _nan(torch, (n, 4))
    model.resolve_grid_dev(a["grid"].device_grid(0), n, _ptr(x0), _ptr(tf), a["margin"], a["damping"], max_iters, _ptr(x), _ptr(iters), _ptr(energy),
                           _ptr(status), x_ref_ptr=_ptr(xr), posture_weight_ptr=_ptr(u), n_target=a.get("n_target", 0), target_pos_ptr=_ptr(tp),
                           target_rot_ptr=_ptr(tr), pos_weight_ptr=_ptr(wl), rot_weight_ptr=_ptr(wa), collision_weight=a["wcol"],
                           pair_weight_ptr=_ptr(pw), lo_ptr=_ptr(lo), hi_ptr=_ptr(hi), tol=a["tol"], max_step=a["max_step"],
                           obstacle_pos_ptr=_ptr(op), obstacle_rot_ptr=_ptr(orot), obstacle_margin=a["omargin"], obstacle_weight=a["wobs"],
                           stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return x.cpu().numpy(), iters.cpu().numpy(), energy.cpu().numpy(), status.cpu().numpy()


def robot_model(name):
    return robot_of(name)[0].sphere_model(resolve_grid_inputs(name)["sset"])


def self_resolve(model, d, k, fixed=None):
    """dexr_sphere_resolve on the inputs of d: the solve without any obstacle."""
    return model.resolve(d["q"], d["margin"], d["damping"], k, fixed, d.get("x_ref"), d.get("u"), collision_weight=d["wcol"], lo=d.get("lo"),
                         hi=d.get("hi"), tol=d["tol"], max_step=d["max_step"])


def functional(tag, d, got, x0, active=None):
    """test_gpu_resolve.functional with the four-term energy: what holds on EVERY frame, clear or not."""
    x, iters, energy, status = (np.asarray(a) for a in got)
    x = x.astype(np.float64)
    assert energy.shape == (len(x), 4) and np.isfinite(x).all() and np.isfinite(energy).all() and not (status & ~BITS).any() and (iters >= 1).all(), tag
    P = grid_problem(d)
    if P.x_ref is None:
        P.x_ref = np.asarray(x0, np.float64)
    if active is None:
        active = isr.active_columns(P.orc, np.asarray(P.full(x0), np.float64), P.links, P.fold)
    if d.get("lo") is not None:
        assert ((x >= d["lo"]) & (x <= d["hi"]))[:, active].all(), tag
    assert np.array_equal(x[:, ~active], np.asarray(x0, np.float64)[:, ~active]), tag
    E0, E1 = P.energies(np.asarray(x0, np.float64))[0].sum(1), P.energies(x)[0].sum(1)
    worst = float((E1 - E0 * (1 + RISE)).max())
    print(f"{tag}: E {np.median(E0):.3e} -> {np.median(E1):.3e} (medians), max (E(answer) - E(x0) (1 + {RISE:g})) = {worst:.3e}")
    assert (E1 <= E0 * (1 + RISE)).all(), (tag, worst)
    return E0, E1


# ---- 1. the float64 host twin against the yardstick ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", CASES)
def test_host_float64_against_the_reference(name, which, require_gpu):
    assert len(ROBOTS) == 8 and B == 33 and len(CASES) == 10
    d, res = resolve_grid_inputs(name, which), reference(name, which=which)
    model = robot_model(name)
    assert (model.n_in, model.n_fixed, model.n_sphere, model.n_pair) == (d["orc"].dof, 0, d["sset"].n_sphere, len(d["pairs"]))
    assert (res["decisions"] == 1).any() and (res["decisions"] == 0).any() and (res["energy"][0, :, 3] > 0).any()
    for k in (1, 2, 3, STEPS64):
        got = host_run(model, d, k)
        compare64(f"{name} GRID_{which}", got, res, k)
        functional(f"{name} GRID_{which} float64 {k}", d, got, d["q"])


# ---- 2. the float32 device entry point against the host twin ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_host_twin(name, require_gpu):
    torch = pytest.importorskip("torch")
    d, r64, r32 = resolve_grid_inputs(name), reference(name), reference(name, np.float32, STEPS32)
    model = robot_model(name)
    ok = rgr.clear(r64, STEPS32, *GUARD32)
    assert 2 * ok.sum() >= B
    x64 = host_run(model, d, STEPS32)[0]
    got = dev_run(model, torch, d, STEPS32)
    assert got[0].dtype == np.float32 and got[0].shape == x64.shape and got[2].shape == (B, 4)
    dist = float(np.abs(r32["xs"][STEPS32].astype(np.float64) - r64["xs"][STEPS32])[ok].max())
    e = float(np.abs(got[0].astype(np.float64) - x64)[ok].max())
    ratio = e / dist if dist > 0 else (0.0 if e == 0 else float("inf"))
    print(f"{name}: {int(ok.sum())} of {B} frames clear at the float32 guards; float32 max |x - x64| = {e:.3e}, the yardstick's float32 run is "
          f"{dist:.3e} from its float64 run (error / reference distance {ratio:.2f}, gate {GATE32:g})")
    assert ratio <= GATE32, (name, e, dist)
    for k in (STEPS32, 16):  # every frame, clear or not
        g = got if k == STEPS32 else dev_run(model, torch, d, k)
        functional(f"{name} float32 {k}", d, g, d["q"])
        assert (g[1] <= k).all()


# ---- 3. a grid out of reach: the self-collision solve, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["allegro_hand_right", "shadow_hand_right"])
def test_a_distant_grid_leaves_the_self_collision_solve(name, require_gpu):
    torch = pytest.importorskip("torch")
    base = resolve_grid_inputs(name)
    pos, rot, far = poses(base, pose_seed(name), far_every=1)  # every frame 2 m away
    d = dict(base, pos=pos, rot=rot, far=far)
    g = d["grid"]
    F = gref.fields(d["orc"], d["q"], d["links"], d["rows"], d["centers"], d["radii"], g.values, g.origin, g.spacing, pos, rot, jacobian=False)
    assert far.all() and F["d"].min() >= 1.0 and F["outside"].all()  # the field is at least 1 m at every sphere, all outside the grid's box
    model = robot_model(name)
    got = host_run(model, d, STEPS64)
    want = self_resolve(model, d, STEPS64)
    assert not got[2][:, 3].any()  # E_obs == 0 exactly on every frame
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2][:, :3], want[2]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    assert (got[1] > 1).any() and (got[2][:, 2] > 0).any()  # (and the self-collision solve had work to do)
    g32 = dev_run(model, torch, d, STEPS32)
    assert not g32[2][:, 3].any()


# ---- 4. a NULL pose is zeros and the identity, bit for bit ------------------------------------------------------------------------------
def test_null_pose_equals_explicit_zeros_and_identities(require_gpu):
    torch = pytest.importorskip("torch")
    name = "allegro_hand_right"
    base = resolve_grid_inputs(name)
    model = robot_model(name)
    zero, eye = np.zeros((B, 3)), np.tile(np.eye(3), (B, 1, 1))
    runs = {}
    for tag, pos, rot in (("null", None, None), ("explicit", zero, eye), ("pos only", zero, None), ("rot only", None, eye)):
        d = dict(base, pos=pos, rot=rot)
        runs[tag] = (host_run(model, d, STEPS32), dev_run(model, torch, d, STEPS32))
    assert (runs["null"][0][2][:, 3] > 0).any() and (runs["null"][1][2][:, 3] > 0).any()  # a shared scene the hand touches
    for tag in ("explicit", "pos only", "rot only"):
        for a, b in zip(runs[tag], runs["null"]):
            assert all(np.array_equal(u, v) for u, v in zip(a, b)), tag
    functional("shared scene", dict(base, pos=None, rot=None), runs["null"][0], base["q"])


# ---- 5. rows are independent ------------------------------------------------------------------------------------------------------------
def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    name, k = "allegro_hand_right", 5
    d = resolve_grid_inputs(name)
    model = robot_model(name)
    full = dev_run(model, torch, d, k)
    assert not np.isnan(full[0]).any() and not np.isnan(full[2]).any() and (full[1] != -7).all() and (full[3] != -7).all()  # all overwritten
    assert (full[2][:, 3] > 0).any() and len(set(full[1].tolist())) > 1
    for rows in (slice(0, 1), slice(1, 17), slice(15, 33), slice(32, 33)):  # whole against slices: the same bits
        part = dev_run(model, torch, d, k, rows=rows)
        assert all(np.array_equal(u, v[rows]) for u, v in zip(part, full)), rows
    aliased = dev_run(model, torch, d, k, alias=True)
    assert all(np.array_equal(u, v) for u, v in zip(aliased, full))
    h64 = host_run(model, d, k)
    part = host_run(model, dict(d, q=d["q"][16:], pos=d["pos"][16:], rot=d["rot"][16:]), k)
    assert all(np.array_equal(u, v[16:]) for u, v in zip(part, h64))
    # a NaN in x0 of frame 7, a NaN in the obstacle position of frame 9, an infinity in that of frame 12 and one in the rotation of
    # frame 13 spoil those frames alone, which still end within k trials
    bad_q, bad_p, bad_r = d["q"].copy(), d["pos"].copy(), d["rot"].copy()
    bad_q[7, 3] = np.nan
    bad_p[9, 1] = np.nan
    bad_p[12, 0] = np.inf
    bad_r[13, 1, 2] = -np.inf
    got = dev_run(model, torch, dict(d, q=bad_q, pos=bad_p, rot=bad_r), k)
    keep = ~np.isin(np.arange(B), (7, 9, 12, 13))
    assert all(np.array_equal(u[keep], v[keep]) for u, v in zip(got, full))
    assert 1 <= got[1][7] <= k and np.isnan(got[0][7, 3]) and not (got[3][7] & ~BITS)
    for b in (9, 12, 13):  # (the answer is an accepted point: x0, the one point such a frame accepts)
        assert 1 <= got[1][b] <= k and not (got[3][b] & ~BITS) and np.array_equal(got[0][b], d["q"][b].astype(np.float32)), b
    assert np.isnan(got[2][9, 3])  # (an infinite pose may leave E_obs = 0 -- the field is +inf there -- with forces that are NaN)
    h = host_run(model, dict(d, q=bad_q, pos=bad_p, rot=bad_r), k)
    assert all(np.array_equal(u[keep], v[keep]) for u, v in zip(h, h64)) and (h[1][[7, 9, 12, 13]] <= k).all()
    # B = 0: a no-op, NULL pointers and all
    lib = _lib.load()
    assert lib.dexr_sphere_resolve_grid_dev(model.handle, 0, None, None, None, None, 0, None, None, None, None, 0.01, 1.0, None, None, None, 1e-4, 0.0,
                                            0.0, 4, d["grid"].device_grid(0).handle, None, None, 0.01, 1.0, None, None, None, None, None) == 0
    x, it, en, st = model.resolve_grid(d["grid"].device_grid(0), np.zeros((0, model.n_in)), 0.01, 1e-4, 4)
    assert x.shape == (0, model.n_in) and it.shape == (0,) and en.shape == (0, 4) and st.shape == (0,)


# ---- 6. edges of the grid ----------------------------------------------------------------------------------------------------------------
def on_the_last_sample(d, grid, frame=0, sphere=0):
    """the poses of d with frame `frame` moved so that sphere `sphere` of x0 sits on the grid's last sample (to float32 rounding of the
    position: the cell coordinate is n - 1 give or take 1e-6 cells, the clamp and the integer clamp meet there)."""
    c = gref.cref.centres(d["orc"], d["q"], d["links"], d["rows"], d["centers"])[0]
    last = grid.origin + (np.array(grid.shape) - 1) * grid.spacing
    pos = d["pos"].copy()
    pos[frame] = c[frame, sphere] - d["rot"][frame] @ last
    return _r32(pos)


@pytest.mark.parametrize("which", ["2x2x2", "5x3x2"])
def test_edges_of_the_grid_and_the_scalars(which, require_gpu):
    torch = pytest.importorskip("torch")
    name = "shadow_hand_right"
    base = resolve_grid_inputs(name)
    model = robot_model(name)
    grid = awkward_grid(which)
    assert grid.shape == tuple(int(v) for v in which.split("x"))
    d0 = dict(base, grid=grid)
    d0["pos"] = on_the_last_sample(d0, grid)
    F = grid_problem(d0).fields(d0["q"], False)
    u0 = (F["y"][0, 0] - grid.origin) / grid.spacing
    assert np.abs(u0 - (np.array(grid.shape) - 1)).max() < 1e-5  # a sphere on the last sample
    h0 = d0["omargin"] - F["d"]
    near = ~d0["far"]
    assert ((h0 > 0) & F["outside"])[near].any() and ((h0 > 0) & ~F["outside"])[near].any()  # contacts inside the box and in the clamp branch
    cases_ = {
        "as it stands": d0,
        "obstacle_weight and obstacle_margin given": dict(d0, wobs=_f32(0.75), omargin=_f32(0.02)),
        "obstacle_weight = 0": dict(d0, wobs=0.0),
    }
    for tag, d in cases_.items():
        tag = f"{which} {tag}"
        res = reference_run(d, STEPS32)
        got = host_run(model, d, STEPS32)
        ok = compare64(tag, got, res, STEPS32, need=1)
        functional(tag, d, got, d["q"])
        if d["wobs"] == 0:  # the self-collision solve, as in test 3: bit for bit, on every frame
            want = self_resolve(model, d, STEPS32)
            assert not got[2][:, 3].any()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2][:, :3], want[2]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
        else:
            assert (res["energy"][0, :, 3] > 0).any() and (got[2][:, 3] < res["energy"][0, :, 3])[res["energy"][0, :, 3] > 0].any()
        g32 = dev_run(model, torch, d, STEPS32)
        functional(tag + " float32", d, g32, d["q"])
        print(f"{tag}: {int(ok.sum())} of {B} frames clear")


# ---- 7. optimizer order: mimic joints fold, fixed joints move the geometry and are no variables ---------------------------------------
@pytest.mark.parametrize("rel", ["teleop/ability_hand_right.yml", "offline/inspire_hand_right.yml", "subset"])
def test_optimizer_order_folds_mimic_and_fixed_joints(rel, require_gpu):
    opt, prob, sset, pairs, d0, fx = _opt_case(rel, 311)
    d = with_grid(d0, grid_a(), 64)
    model = opt.sphere_model(sset)
    assert (model.n_in, model.n_fixed, model.n_pair) == (opt.opt_dof, len(opt.idx_pin2fixed), len(pairs))
    res = reference_run(d, STEPS32)
    assert (res["energy"][0, :, 3] > 0).any() and (res["decisions"] == 1).any()
    got = host_run(model, d, STEPS32, fixed=fx)
    compare64(rel, got, res, STEPS32, need=1)
    functional(rel, d, got, d["q"])
    if fx is not None:  # fixed joints move the geometry
        moved = host_run(model, d, STEPS32, fixed=fx + 0.05)
        assert np.abs(moved[2] - got[2]).max() > 1e-9


# ---- 8. table limits: the synthetic robots of tests/pose_zoo.py, and the header's byte formula ---------------------------------------
ZB, ZMARGIN, ZR = 9, 0.020, 0.010


def lds_bytes(n_slot, n_jx, n_act, n_link, n_in, n_sphere, n_pair, targets, v):
    """the LDS section of include/dexr_resolve_grid.h, evaluated."""
    n_tri = n_act * (n_act + 1) // 2
    values = (6 * n_jx + (11 * n_link if targets else 0) + 6 * n_sphere + 16 + max(n_tri, 16 * n_act + 16) + n_tri + 4 * n_act + 2 * n_in + 8 + 12 + 16) | 1
    return 128 + v * (12 * n_slot + values) + 4 * (_lib.RESOLVE_MAXACTIVE + 22) + 4 * 17 + 2 * ((n_sphere + 3) & ~3) + ((n_pair + 3) & ~3)


def _table_facts(blob):
    tab = zoo.pi.parse(blob)
    xj = [j for j in tab["joints"] if int(j["src_kind"]) == pt.SRC_X]
    return dict(n_slot=int(tab["h"]["n_slot"]), n_jx=len(xj), n_act=len({int(j["src_col"]) for j in xj}), n_link=len(tab["links"]), n_in=int(tab["h"]["n_in"]))


def everywhere_grid():
    """9^3 samples 0.5 m apart, 4 m across and centred: a gentle slope that is negative throughout -- every sphere of a robot within 2 m
    of the origin is in contact, and every contact has a direction."""
    k = np.arange(9, dtype=np.float64) - 4
    v = -0.25 + 0.02 * (k[:, None, None] + 0.5 * k[None, :, None] - 0.25 * k[None, None, :])
    assert v.max() < -0.1
    return collision.SdfGrid(v, -2.0, 0.5)


def test_table_limits_float64_solve_or_are_refused_by_the_formula(tmp_path, require_gpu):
    grid = everywhere_grid()
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "dexr_resolve_grid.h")).read()
    for piece in ("6 n_jx + L + 6 n_sphere + 16 + max(n_tri, 16 n_act + 16) + n_tri + 4 n_act + 2 n_in + 8 + 12 + 16) | 1",
                  "128 + v (12 n_slot + values) + 4 (DEXR_RESOLVE_MAXACTIVE + 22) + 4 * 17 + 2 ((n_sphere + 3) & ~3)", "((n_pair + 3) & ~3)",
                  "65 156 B", "37 424 B"):
        assert piece in text  # the formula evaluated here is the one the header states
    assert lds_bytes(8, 64, 64, 64, 256, 128, 8128, True, 8) == 65156 and lds_bytes(8, 64, 64, 64, 256, 128, 8128, True, 4) == 37424
    branches = set()
    for name, per_link, wide in (("chain64", 1, False), ("wide_map", 1, False), ("binary64_slots8", 2, False), ("binary64", 2, True)):
        m = zoo.build(name, tmp_path)
        blob, smap = m.blob, m.smap
        if wide:  # the 64 joints behind a source map of 256 columns, every fourth one read: the widest table the format holds
            smap = pt.SourceMap(256, 0, [(pt.SRC_X, 4 * k, 1.0, 0.0) for k in range(len(m.smap.entries))])
            blob = pt.compile_poses(m.kin, m.links, smap)
        L = len(m.links)
        rows = np.repeat(np.arange(L), per_link)
        S = len(rows)
        centers = _r32(np.random.default_rng(61).uniform(-0.01, 0.01, (S, 3)))
        radii = np.full(S, ZR)
        pairs = np.array([(i, j) for i in range(S) for j in range(i + 1, S)], np.int32)
        model = _lib.SphereModel(blob, rows, centers, radii, pairs)
        facts = _table_facts(blob)
        assert facts["n_in"] == model.n_in and facts["n_link"] == L
        nt = 3 if per_link == 2 else 0
        need = lds_bytes(n_sphere=S, n_pair=len(pairs), targets=nt > 0, v=8, **facts)
        x = _r32(np.random.default_rng(2043).uniform(-0.5, 0.5, (ZB, smap.n_in))) if wide else zoo.inputs(m, ZB, 2043)[0]
        fixed = None if wide else zoo.inputs(m, ZB, 2043)[1]
        d = dict(orc=m.orc, links=list(m.links), rows=rows, centers=centers, radii=radii, pairs=pairs, q=x, margin=_f32(ZMARGIN),
                 u=np.full(x.shape[1], _f32(1e-4)), damping=_f32(1e-4), max_step=_f32(0.2), tol=0.0, wcol=1.0,
                 full=lambda v, s=smap, f=fixed: zoo.full_q(s, v, f), fold=lambda J, s=smap: zoo.fold(s, J))
        if nt:
            tp, trot = isr.link_poses(m.orc, d["full"](_r32(x + 0.05)), list(m.links)[:nt])
            d.update(n_target=nt, tgt_pos=tp, tgt_rot=trot)
        d = with_grid(d, grid, pos=None, rot=None)
        if need > 64 * 1024:
            with pytest.raises(_lib.DexrError, match=rf"libdexr error {UNSUPPORTED}: .*needs {need} B of LDS per frame"):
                host_run(model, d, STEPS32, fixed=fixed)
            branches.add("refused")
            print(f"{name} x{per_link}{' behind 256 columns' if wide else ''}: {S} spheres, {len(pairs)} pairs, {need} B per frame: refused")
            continue
        res = reference_run(d, STEPS32)  # (the yardstick has no cap)
        ho = grid_problem(d, x_ref=x).energies(x)[1][1]
        assert (ho > 0).all() and ho.shape == (ZB, S, 1)  # every sphere is in contact
        assert (res["energy"][0, :, 2] > 0).all() and (res["decisions"] == 1).any()
        got = host_run(model, d, STEPS32, fixed=fixed)
        ok = compare64(f"{name} x{per_link}", got, res, STEPS32, need=1)
        unread = np.array([c % 4 != 0 for c in range(256)]) if wide else zoo.abs_mult(m).sum(0) == 0
        functional(f"{name} x{per_link}", d, got, x, active=~unread)
        assert not (got[3] & rgr.CONTACTS_TRUNCATED).any()
        branches.add("solved")
        print(f"{name} x{per_link}: {S} spheres, all in contact, {len(pairs)} pairs, {need} B per frame "
              f"({max(f for f in (1, 2, 4, 8, 16) if f == 1 or f * need <= 65536)} frames a block), {int(ok.sum())} of {ZB} frames clear")
        if per_link == 2:
            assert (S, len(pairs)) == (128, 8128)
    assert "solved" in branches


# ---- 9. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    model, d = _target_case()
    grid = grid_a().device_grid(0)
    n, n_in = 4, model.n_in
    x = torch.zeros((n, n_in), dtype=torch.float32, device="cuda")
    tp, tr, w = (torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((n, 5, 3), (n, 5, 3, 3), (n, 5)))
    lim = torch.zeros((n_in,), dtype=torch.float32, device="cuda")
    out, en = _nan(torch, (n, n_in)), _nan(torch, (n, 4))
    it, st = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    good = dict(m=model.handle, B=n, x0=x.data_ptr(), fixed=None, x_ref=None, u=None, n_target=5, tp=tp.data_ptr(), tr=tr.data_ptr(), wl=w.data_ptr(),
                wa=w.data_ptr(), margin=0.01, wcol=1.0, pw=None, lo=lim.data_ptr(), hi=lim.data_ptr(), damping=1e-4, max_step=0.2, tol=0.0,
                max_iters=4, g=grid.handle, opos=None, orot=None, omargin=0.01, wobs=1.0, x_out=out.data_ptr(), iters=it.data_ptr(),
                energy=en.data_ptr(), status=st.data_ptr())

    def invalid(word, **over):
        a = dict(good, **over)
        rc = lib.dexr_sphere_resolve_grid_dev(*[a[k] for k in good], None)
        msg = lib.dexr_last_error()
        assert rc == INVALID and word in msg, (rc, msg, over)

    invalid(b"null sphere model", m=None)
    invalid(b"null sdf grid", g=None)
    invalid(b"negative", B=-1)
    for bad in (-1e-6, float("nan"), float("inf")):
        invalid(b"obstacle_margin", omargin=bad)
        invalid(b"obstacle_weight", wobs=bad)
        invalid(b"margin", margin=bad)
        invalid(b"collision_weight", wcol=bad)
        invalid(b"tol", tol=bad)
        invalid(b"max_step", max_step=bad)
        invalid(b"damping", damping=bad)
    invalid(b"damping", damping=0.0)
    for bad in (0, -1, 257):
        invalid(b"max_iters", max_iters=bad)
    invalid(b"lo and hi", lo=None)
    invalid(b"lo and hi", hi=None)
    for bad in (-1, 65, model.n_sphere + 6):
        invalid(b"n_target", n_target=bad)
    invalid(b"target_pos and target_rot are both NULL", tp=None, tr=None, wl=None, wa=None)
    invalid(b"n_target is 0", n_target=0)
    invalid(b"pos_weight given without target_pos", tp=None)
    invalid(b"rot_weight given without target_rot", tr=None)
    invalid(b"x_out is NULL", x_out=None)
    invalid(b"x0 is NULL", x0=None)
    # the host twin keeps the same rules
    z = np.zeros((n, n_in))
    zo, ze, zi, zs = np.full((n, n_in), np.nan), np.full((n, 4), np.nan), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))  # noqa: E731
    hgood = dict(m=model.handle, B=n, x0=dp(z), fixed=None, x_ref=None, u=None, n_target=0, tp=None, tr=None, wl=None, wa=None, margin=0.01, wcol=1.0,
                 pw=None, lo=None, hi=None, damping=1e-4, max_step=0.2, tol=0.0, max_iters=4, g=grid.handle, opos=None, orot=None, omargin=0.01, wobs=1.0,
                 x_out=dp(zo), iters=ip(zi), energy=dp(ze), status=ip(zs))
    for word, over in ((b"null sphere model", dict(m=None)), (b"null sdf grid", dict(g=None)), (b"obstacle_margin", dict(omargin=-1.0)),
                       (b"obstacle_weight", dict(wobs=float("nan"))), (b"negative", dict(B=-2)), (b"margin", dict(margin=-1.0)),
                       (b"damping", dict(damping=float("nan"))), (b"max_iters", dict(max_iters=0)), (b"lo and hi", dict(lo=dp(z[0].copy()))),
                       (b"n_target", dict(n_target=99)), (b"both NULL", dict(n_target=2)), (b"x_out is NULL", dict(x_out=None)), (b"x0 is NULL", dict(x0=None))):
        a = dict(hgood, **over)
        rc = lib.dexr_sphere_resolve_grid(*[a[k] for k in hgood])
        assert rc == INVALID and word in lib.dexr_last_error(), (word, rc, lib.dexr_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(en).all()) and bool((it == -7).all()) and bool((st == -7).all())  # nothing was launched
    assert np.isnan(zo).all() and np.isnan(ze).all() and (zi == -7).all() and (zs == -7).all()
    for kw in (dict(x_ref=z[:, :-1]), dict(obstacle_pos=np.zeros((n, 2))), dict(obstacle_rot=np.zeros((n, 9))), dict(lo=np.zeros(n_in)),
               dict(pair_weight=np.zeros(model.n_pair + 1))):
        with pytest.raises(ValueError):
            model.resolve_grid(grid, z, 0.01, 1e-4, 4, **kw)
    with pytest.raises(ValueError, match="required"):
        model.resolve_grid(grid, z, 0.01, 1e-4)


# ---- 10. the torch fronts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_torch_fronts_equal_the_entry_points_bitwise(rel, require_gpu):
    torch = pytest.importorskip("torch")
    opt, prob, sset, pairs, d0, fx = _opt_case(rel, 321)
    grid = grid_a()
    d = with_grid(d0, grid, 64)
    n, k = B, 6
    q, f, pos, rot = _dev(torch, d["q"]), _dev(torch, fx), _dev(torch, d["pos"]), _dev(torch, d["rot"])
    tips = ["link_15.0_tip", "link_3.0_tip"]
    tp, trot = isr.link_poses(prob.robot, d["full"](_r32(d["q"] + 0.05)), tips)
    tpt, trt = _dev(torch, tp), _dev(torch, trot)
    wt = _dev(torch, np.random.default_rng(322).uniform(0.5, 2, (n, 2)))
    pw = _dev(torch, np.random.default_rng(323).uniform(0.5, 2.0, len(pairs)))
    lim = _dev(torch, np.stack([d["lo"], d["hi"]], 1))
    qref = _dev(torch, _r32(d["q"] + 0.01))
    ut = _dev(torch, np.random.default_rng(324).uniform(0, 1e-3, q.shape[1]))
    fresh = lambda width: (_nan(torch, (n, width)), torch.full((n,), -7, dtype=torch.int32, device="cuda"), _nan(torch, (n, 4)),  # noqa: E731
                           torch.full((n,), -7, dtype=torch.int32, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = side.cuda_stream
        dgrid = grid.device_grid(torch.cuda.current_device())
        # the defaults: obstacle_margin = margin, weight 1, a pose per frame
        got = collision.resolve_grid_collisions(opt, q, sset, grid, 0.01, obstacle_pos=pos, obstacle_rot=rot, damping=1e-4, max_iters=k, posture_weight=1e-3,
                                                fixed_qpos=f, limits=lim, max_step=0.2)
        model = opt.sphere_model(sset)
        u = torch.full((q.shape[1],), 1e-3, dtype=torch.float32, device="cuda")
        lo, hi = lim[:, 0].contiguous(), lim[:, 1].contiguous()
        wx, wi, we, ws = fresh(q.shape[1])
        model.resolve_grid_dev(dgrid, n, q.data_ptr(), _ptr(f), 0.01, 1e-4, k, wx.data_ptr(), wi.data_ptr(), we.data_ptr(), ws.data_ptr(),
                               posture_weight_ptr=u.data_ptr(), lo_ptr=lo.data_ptr(), hi_ptr=hi.data_ptr(), max_step=0.2, obstacle_pos_ptr=pos.data_ptr(),
                               obstacle_rot_ptr=rot.data_ptr(), obstacle_margin=0.01, obstacle_weight=1.0, stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(got, (wx, wi, we, ws))) and not got[0].requires_grad
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].shape == (n, 4) and got[3].dtype == torch.int32
        assert bool((we[:, 3] > 0).any()) and bool(torch.isfinite(wx).all())
        # everything at once, positionally, with targets: a model keyed by the target links; non-contiguous views with the same values
        qn, pn = torch.stack([q, q], 2)[:, :, 0], torch.stack([pos, pos], 2)[:, :, 1]
        assert not qn.is_contiguous() and not pn.is_contiguous()
        got = collision.resolve_grid_collisions(opt, qn, sset, grid, 0.01, 0.02, pn, rot, 0.75, 1e-4, k, ut, qref, 2.0, pw, tips, tpt, trt, wt, wt, 1e-7, 0.2,
                                                lim, f)
        tm = opt.sphere_model(sset, pairs, tips)
        assert tm is not model
        tm.resolve_grid_dev(dgrid, n, q.data_ptr(), _ptr(f), 0.01, 1e-4, k, wx.data_ptr(), wi.data_ptr(), we.data_ptr(), ws.data_ptr(),
                            x_ref_ptr=qref.data_ptr(), posture_weight_ptr=ut.data_ptr(), n_target=2, target_pos_ptr=tpt.data_ptr(),
                            target_rot_ptr=trt.data_ptr(), pos_weight_ptr=wt.data_ptr(), rot_weight_ptr=wt.data_ptr(), collision_weight=2.0,
                            pair_weight_ptr=pw.data_ptr(), lo_ptr=lo.data_ptr(), hi_ptr=hi.data_ptr(), tol=1e-7, max_step=0.2,
                            obstacle_pos_ptr=pos.data_ptr(), obstacle_rot_ptr=rot.data_ptr(), obstacle_margin=0.02, obstacle_weight=0.75, stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(got, (wx, wi, we, ws))) and bool((we[:, 0] > 0).all()) and bool((we[:, 3] > 0).any())
        # the robot twin over the full qpos, a shared scene (no pose)
        robot = opt.robot
        rl = robot.joint_limits
        qr = _dev(torch, np.random.default_rng(325).uniform(rl[:, 0], rl[:, 1], (n, robot.dof)))
        rlim = _dev(torch, rl)
        gr = collision.robot_resolve_grid_collisions(robot, qr, sset, grid, 0.01, damping=1e-4, max_iters=k, posture_weight=1e-3, limits=rlim)
        rm = robot.sphere_model(sset, pairs)
        ur = torch.full((robot.dof,), 1e-3, dtype=torch.float32, device="cuda")
        rlo, rhi = rlim[:, 0].contiguous(), rlim[:, 1].contiguous()
        rx, ri, re_, rs = fresh(robot.dof)
        rm.resolve_grid_dev(dgrid, n, qr.data_ptr(), 0, 0.01, 1e-4, k, rx.data_ptr(), ri.data_ptr(), re_.data_ptr(), rs.data_ptr(),
                            posture_weight_ptr=ur.data_ptr(), lo_ptr=rlo.data_ptr(), hi_ptr=rhi.data_ptr(), stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(gr, (rx, ri, re_, rs)))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e = torch.zeros((0, opt.opt_dof), device="cuda")
    out = collision.resolve_grid_collisions(opt, e, sset, grid, 0.01, damping=1e-4, max_iters=k, fixed_qpos=None if f is None else f[:0])
    assert out[0].shape == (0, opt.opt_dof) and out[1].shape == (0,) and out[2].shape == (0, 4) and out[3].shape == (0,)


# ---- 11. end to end ------------------------------------------------------------------------------------------------------------------------
def test_retarget_then_resolve_against_a_held_object_given_as_a_grid(require_gpu):
    torch = pytest.importorskip("torch")
    import test_gpu_link_poses as glp
    from dex_retargeting_amd import autograd as ag

    rel = "teleop/allegro_hand_right.yml"
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    n = 256
    hs = cases.human_set(prob, n)
    names = ["link_3.0_tip", "link_7.0_tip", "link_11.0_tip", "link_15.0_tip", "link_2.0", "link_6.0", "link_10.0", "link_14.0"]
    sset = collision.SphereSet(names, np.zeros((8, 3)), np.full(8, 0.012))
    kp = glp._t(hs["kp"], torch, dtype=torch.float32)
    last = glp._t(hs["last"], torch)
    fixed = glp._t(hs["fixed"], torch) if hs["fixed"].shape[1] else None
    q = ag.retarget(opt, ag.ref_value_from_keypoints(opt, kp), last, fixed, None).detach()
    # the held object: a ball of 3 cm and a short capsule through it, sampled on 65^3 at 2.5 mm, at the centroid of the frame's four
    # fingertip spheres
    obj = collision.ObstacleSet.spheres([[0.0, 0.0, 0.0]], [0.03]) + collision.ObstacleSet.capsules([[0.0, 0.0, -0.04]], [[0.0, 0.0, 0.04]], [0.015])
    grid = collision.SdfGrid.from_obstacles(obj, -0.08, 0.0025, 65)
    _, cen = collision.sphere_distances(opt, q, sset, fixed, centers=True)
    pos = cen[:, :4].mean(1).contiguous()
    margin, u = 0.005, 1e-3
    d0 = collision.grid_distances(opt, q, sset, grid, pos, None, fixed)
    x, iters, energy, status = collision.resolve_grid_collisions(opt, q, sset, grid, margin, obstacle_pos=pos, damping=1e-4, max_iters=16, posture_weight=u,
                                                                 fixed_qpos=fixed, max_step=0.2)
    d1 = collision.grid_distances(opt, x, sset, grid, pos, None, fixed)
    deep0, deep1 = float((-d0.min(1).values).max()), float((-d1.min(1).values).max())
    Eo0, _ = collision.grid_penalty(opt, q, sset, grid, margin, pos, None, fixed)
    Es0, _ = collision.self_collision_penalty(opt, q, sset, margin, None, fixed)
    Eo1, _ = collision.grid_penalty(opt, x, sset, grid, margin, pos, None, fixed)
    Es1, _ = collision.self_collision_penalty(opt, x, sset, margin, None, fixed)
    total0, total1 = (Eo0 + Es0).double(), (Eo1 + Es1).double() + u * ((x - q).double() ** 2).sum(1)
    print(f"retarget -> resolve against a held object: {int((d0.min(1).values < 0).sum())} of {n} frames start inside it, deepest penetration "
          f"{deep0 * 1e3:.2f} mm -> {deep1 * 1e3:.2f} mm, obstacle energy {float(Eo0.sum()):.3e} -> {float(Eo1.sum()):.3e}, iters "
          f"{torch.bincount(iters).tolist()}, status {torch.bincount(status, minlength=16).tolist()}")
    assert deep0 > 0 and deep1 < deep0 and bool(torch.isfinite(x).all())
    assert bool((total1 <= total0 * (1 + RISE)).all())  # total E does not rise (the kernel's own float32 sums against torch's)
    assert float(Eo1.sum()) < float(Eo0.sum()) and not bool((status & ~BITS).any()) and bool((iters >= 1).all()) and bool((iters <= 16).all())
    assert torch.equal(energy[:, 0], torch.zeros_like(energy[:, 0])) and torch.allclose(energy[:, 3], Eo1, rtol=1e-3, atol=1e-9)

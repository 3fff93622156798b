"""GPU tests of the collision-aware posture solve (csrc/dexr_resolve.hpp, include/dexr_resolve.h): the float64 host twin against
tests/resolve_reference.py, the float32 device entry point against the host twin, optimizer order, targets, row independence, the
table limits on the synthetic robots of tests/pose_zoo.py, the overflow of the active list, the raw ABI's argument errors and the
torch front.

INPUTS and DECISION GUARDS: tests/test_resolve_host.py (resolve_inputs, reference; B = 33), whose reference runs are proven there
on the CPU and shared from there.  A comparison against the yardstick is made on the frames that are CLEAR at its guards; every
other frame goes through the functional checks (finite, inside the limits, unread columns unchanged, E recomputed by the yardstick
in float64 does not rise).

GATES.  float64: 1e-9 on x and the energies, iters and status equal.  float32: max |x32 - x64| over the clear frames may be
GATE32 = 8 x the distance between the yardstick's OWN float32 and float64 runs on those frames.  E(answer) <= E(x0) (1 + 1e-3):
16 accepted steps times twice the 2e-5 relative error of a float32 h^2 at h = 1 cm, rounded up."""
import os

import numpy as np
import pytest

import ik_solve_reference as isr
import pose_zoo as zoo
import resolve_reference as rr
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, ROBOTS, robot_of
from test_gpu_link_jacobians import OPT_ORDER, _fold4, _opt_inputs, _optimizer_and_problem
from test_jacobian_host import SUBSET_CFG
from test_resolve_host import GUARD32, GUARD64, STEPS32, STEPS64, _f32, _r32, problem, reference, resolve_inputs

pytestmark = pytest.mark.gpu
GATE64, GATE32, RISE = 1e-9, 8.0, 1e-3
BITS = rr.CONVERGED | rr.STALLED | rr.TRUNCATED


# ---- the two entry points on the dict of resolve_inputs (keys a run does not have are absent: None) ---------------------------------
KEYS = ("x_ref", "tgt_pos", "tgt_rot", "w_pos", "w_rot", "pair_weight")


def host_run(model, d, max_iters, fixed=None, **over):
    a = dict(d, **over)
    return model.resolve(a["q"], a["margin"], a["damping"], max_iters, fixed, a.get("x_ref"), a.get("u"), a.get("tgt_pos"), a.get("tgt_rot"),
                         a.get("w_pos"), a.get("w_rot"), a["wcol"], a.get("pair_weight"), a.get("lo"), a.get("hi"), a["tol"], a["max_step"],
                         n_target=a.get("n_target", 0))


def _dev(torch, a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def dev_run(model, torch, d, max_iters, fixed=None, rows=slice(None), alias=False, **over):
    """-> (x, iters, energy, status) of dexr_sphere_resolve_dev on the frames `rows` of d, the outputs pre-filled with NaN / -7;
    alias: x_out is x0's buffer."""
    a = dict(d, **over)
    cut = lambda v: None if v is None else v[rows]  # noqa: E731
    x0, tf, xr, tp, tr, wl, wa = (_dev(torch, cut(v)) for v in (a["q"], fixed, a.get("x_ref"), a.get("tgt_pos"), a.get("tgt_rot"), a.get("w_pos"), a.get("w_rot")))
    u, pw, lo, hi = (_dev(torch, a.get(k)) for k in ("u", "pair_weight", "lo", "hi"))
    n = x0.shape[0]
    x = x0 if alias else _nan(torch, (n, model.n_in))
    iters, status = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    energy = _nan(torch, (n, 3))
    model.resolve_dev(n, _ptr(x0), _ptr(tf), a["margin"], a["damping"], max_iters, _ptr(x), _ptr(iters), _ptr(energy), _ptr(status),
                      x_ref_ptr=_ptr(xr), posture_weight_ptr=_ptr(u), n_target=a.get("n_target", 0), target_pos_ptr=_ptr(tp), target_rot_ptr=_ptr(tr),
                      pos_weight_ptr=_ptr(wl), rot_weight_ptr=_ptr(wa), collision_weight=a["wcol"], pair_weight_ptr=_ptr(pw), lo_ptr=_ptr(lo),
                      hi_ptr=_ptr(hi), tol=a["tol"], max_step=a["max_step"], stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return x.cpu().numpy(), iters.cpu().numpy(), energy.cpu().numpy(), status.cpu().numpy()


def ref_problem(d, dtype=np.float64):
    return problem(d, dtype, **{k: d[k] for k in KEYS + ("n_target", "full", "fold") if d.get(k) is not None})


def ref_run(d, max_iters, dtype=np.float64):
    return rr.resolve(ref_problem(d, dtype), d["q"], d["damping"], max_iters, d.get("lo"), d.get("hi"), d["tol"], d["max_step"])


def robot_model(name):
    return robot_of(name)[0].sphere_model(resolve_inputs(name)["sset"])


def compare64(tag, got, res, k, need=None):
    """the answer of max_iters = k against the yardstick's run on its clear frames; -> the clear mask."""
    x, iters, energy, status = got
    wx, wi, we, ws = rr.answer(res, k)
    ok = rr.clear(res, k, *GUARD64)
    assert x.shape == wx.shape and x.dtype == np.float64 and iters.dtype == np.int32 and status.dtype == np.int32 and energy.shape == we.shape
    ex, ee = float(np.abs(x - wx)[ok].max()), float(np.abs(energy - we)[ok].max())
    print(f"{tag}, {k} trials: {int(ok.sum())} of {len(ok)} frames clear; float64 max |x - reference| = {ex:.3e}, max |energy - reference| = {ee:.3e} "
          f"(gate {GATE64:.0e}); iters {np.bincount(iters).tolist()}, status {np.bincount(status, minlength=8).tolist()}")
    assert ok.sum() >= (len(ok) + 1) // 2 if need is None else ok.sum() >= need, tag
    assert ex <= GATE64 and ee <= GATE64, (tag, k, ex, ee)
    assert np.array_equal(iters[ok], wi[ok]) and np.array_equal(status[ok], ws[ok]), (tag, k)
    return ok


def functional(tag, d, got, x0, active=None):
    """what holds on EVERY frame, clear or not: finite outputs, known status bits, iters in range, active entries inside the limits,
    unread columns unchanged, and E recomputed in float64 by the yardstick at the answer is at most E(x0) (1 + RISE)."""
    x, iters, energy, status = (np.asarray(a) for a in got)
    x = x.astype(np.float64)
    assert np.isfinite(x).all() and np.isfinite(energy).all() and not (status & ~BITS).any() and (iters >= 1).all(), tag
    P = ref_problem(d)
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
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_host_float64_against_the_reference(name, require_gpu):
    assert len(ROBOTS) == 8
    d, res = resolve_inputs(name), reference(name)
    model = robot_model(name)
    assert (model.n_in, model.n_fixed, model.n_sphere, model.n_pair) == (d["orc"].dof, 0, d["sset"].n_sphere, len(d["pairs"]))
    dec = res["decisions"]
    assert (dec == 1).any() and (dec == 0).any()  # the runs hold accepted and rejected trials
    for k in (1, 2, 3, STEPS64):
        got = host_run(model, d, k)
        compare64(name, got, res, k)
        functional(f"{name} float64 {k}", d, got, d["q"])


# ---- 2. the float32 device entry point against the host twin ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ROBOTS))
def test_device_float32_against_the_host_twin(name, require_gpu):
    torch = pytest.importorskip("torch")
    d, r64, r32 = resolve_inputs(name), reference(name), reference(name, np.float32, STEPS32)
    model = robot_model(name)
    ok = rr.clear(r64, STEPS32, *GUARD32)
    assert 2 * ok.sum() >= B
    x64 = host_run(model, d, STEPS32)[0]
    got = dev_run(model, torch, d, STEPS32)
    assert got[0].dtype == np.float32 and got[0].shape == x64.shape
    dist = float(np.abs(r32["xs"][STEPS32].astype(np.float64) - r64["xs"][STEPS32])[ok].max())
    e = float(np.abs(got[0].astype(np.float64) - x64)[ok].max())
    ratio = e / dist if dist > 0 else (0.0 if e == 0 else float("inf"))
    print(f"{name}: {int(ok.sum())} of {B} frames clear at the float32 guards; float32 max |x - x64| = {e:.3e}, the yardstick's float32 run is "
          f"{dist:.3e} from its float64 run (error / reference distance {ratio:.2f}, gate {GATE32:g}); on the other frames max |x - x64| = "
          f"{float(np.abs(got[0].astype(np.float64) - x64)[~ok].max()) if (~ok).any() else 0.0:.3e}")
    assert ratio <= GATE32, (name, e, dist)
    for k in (STEPS32, 16):  # every frame, clear or not
        g = got if k == STEPS32 else dev_run(model, torch, d, k)
        functional(f"{name} float32 {k}", d, g, d["q"])
        assert (g[1] <= k).all()


# ---- 3. optimizer order: mimic joints fold, fixed joints move the geometry and are no variables ----------------------------------------
def _opt_case(rel, seed):
    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames]
    # default pairs skip neighbouring links: spheres of 3 cm, so that links two joints apart come inside the margin
    sset = collision.SphereSet(links, np.zeros((len(links), 3)), np.full(len(links), 0.030))
    pairs = collision.default_pairs(opt.robot, sset)
    x, fixed = (_r32(a) for a in _opt_inputs(prob, B, seed))
    fx = fixed if fixed.shape[1] else None
    d = dict(orc=prob.robot, links=links, rows=np.arange(len(links)), centers=np.zeros((len(links), 3)), radii=np.full(len(links), 0.030), pairs=pairs,
             q=x, margin=_f32(0.010), u=np.full(x.shape[1], _f32(1e-3)), damping=_f32(1e-4), max_step=_f32(0.2), tol=0.0, wcol=1.0,
             lo=_r32(x.min(0) - 0.05), hi=_r32(x.max(0) + 0.05), full=lambda v: prob.full_qpos(v, fixed), fold=lambda J: _fold4(prob, J))
    return opt, prob, sset, pairs, d, fx


@pytest.mark.parametrize("rel", ["teleop/ability_hand_right.yml", "offline/inspire_hand_right.yml", "subset"])
def test_optimizer_order_folds_mimic_and_fixed_joints(rel, require_gpu):
    assert rel == "subset" or rel in OPT_ORDER
    opt, prob, sset, pairs, d, fx = _opt_case(rel, 311)
    model = opt.sphere_model(sset)
    assert (model.n_in, model.n_fixed, model.n_pair) == (opt.opt_dof, len(opt.idx_pin2fixed), len(pairs))
    if rel == "subset":
        assert model.n_fixed == 6 and model.n_in == 10
    else:
        assert len(prob.idx_pin2mimic) > 0
    res = ref_run(d, STEPS32)
    assert (res["energy"][0, :, 2] > 0).any() and (res["decisions"] == 1).any()
    got = host_run(model, d, STEPS32, fixed=fx)
    compare64(rel, got, res, STEPS32)
    functional(rel, d, got, d["q"])
    if fx is not None:  # fixed joints move the geometry
        moved = host_run(model, d, STEPS32, fixed=fx + 0.05)
        assert np.abs(moved[2] - got[2]).max() > 1e-9


# ---- 4. targets ------------------------------------------------------------------------------------------------------------------------
def _target_case():
    """shadow hand, robot order: the five fingertips are target rows that carry NO sphere, spheres on every other link."""
    name = "shadow_hand_right"
    robot, orc = robot_of(name)
    links = [f.name for f in robot.kin.frames]
    tips = [n for n in links if n.endswith("tip")]
    assert len(tips) == 5
    body = [n for n in links if n not in tips]
    sset = collision.SphereSet(body, np.zeros((len(body), 3)), np.full(len(body), 0.010))
    pairs = collision.default_pairs(robot, sset, 2)
    table, rows = collision.resolve_table(sset, tips)
    assert table[:5] == tips and sorted(table[5:]) == sorted(body) and len(table) == len(links)
    base = resolve_inputs(name)
    rng = np.random.default_rng(47)
    q = base["q"]
    tgt_pos, tgt_rot = isr.link_poses(orc, _r32(np.clip(q + rng.uniform(-0.1, 0.1, q.shape), base["lo"], base["hi"])), tips)
    d = dict(base, links=table, rows=rows, centers=np.zeros((len(body), 3)), radii=np.full(len(body), 0.010), pairs=pairs, n_target=5,
             tgt_pos=tgt_pos, tgt_rot=tgt_rot, w_pos=_r32(rng.uniform(0.5, 2, (B, 5))), w_rot=_r32(0.01 * rng.uniform(0.5, 2, (B, 5))))
    return robot.sphere_model(sset, pairs, tips), d


def test_targets_on_links_without_spheres(require_gpu):
    torch = pytest.importorskip("torch")
    model, d = _target_case()
    assert model.n_sphere == len(d["rows"]) and model.n_pair == len(d["pairs"])
    cases_ = {"position and rotation targets": {}, "position targets alone": dict(tgt_rot=None, w_rot=None),
              "rotation targets alone, no weights": dict(tgt_pos=None, w_pos=None, w_rot=None),
              "targets only (collision_weight = 0)": dict(wcol=0.0),
              "targets absent on a table with target rows": dict(n_target=0, tgt_pos=None, tgt_rot=None, w_pos=None, w_rot=None)}
    for tag, over in cases_.items():
        a = dict(d, **over)
        res = ref_run(a, STEPS32)
        E = res["energy"]
        if a["n_target"]:
            assert (E[0, :, 0] > 0).all() and (E[-1, :, 0] < E[0, :, 0]).any()
        if a["wcol"] == 0:
            assert not E[:, :, 2].any()
        got = host_run(model, a, STEPS32)
        compare64(tag, got, res, STEPS32)
        functional(tag, a, got, a["q"])
    g32 = dev_run(model, torch, d, STEPS32)
    functional("targets float32", d, g32, d["q"])
    assert (g32[2][:, 0] > 0).all()


# ---- 5. rows are independent -----------------------------------------------------------------------------------------------------------
def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    name, n, k = "allegro_hand_right", 130, 5
    base = resolve_inputs(name)
    lim = np.stack([base["lo"], base["hi"]], 1)
    q = np.clip(_r32(np.random.default_rng(51).uniform(lim[:, 0], lim[:, 1], (n, len(lim)))), lim[:, 0], lim[:, 1])
    d = dict(base, q=q)
    model = robot_model(name)
    full = dev_run(model, torch, d, k)
    assert (full[2][:, 2] > 0).any() and len(set(full[1].tolist())) > 1 and np.isfinite(full[0]).all()
    for rows in (slice(0, 1), slice(1, 17), slice(17, 129), slice(129, 130)):  # whole against slices: the same bits
        part = dev_run(model, torch, d, k, rows=rows)
        assert all(np.array_equal(u, v[rows]) for u, v in zip(part, full)), rows
    aliased = dev_run(model, torch, d, k, alias=True)
    assert all(np.array_equal(u, v) for u, v in zip(aliased, full))
    # a NaN in row 7 spoils row 7 alone, which still returns within max_iters
    bad = q.copy()
    bad[7, 3] = np.nan
    got = dev_run(model, torch, dict(d, q=bad), k)
    keep = np.arange(n) != 7
    assert all(np.array_equal(u[keep], v[keep]) for u, v in zip(got, full))
    assert 1 <= got[1][7] <= k and np.isnan(got[0][7, 3]) and not (got[3][7] & ~BITS)
    # a frame free of collision with q_ref = q0 comes back exactly, after one trial, CONVERGED
    E3, _, dist = problem(d, x_ref=q).energies(q)
    free = (E3[:, 2] == 0) & (np.abs(d["margin"] - dist).min(1) > GUARD32[0])  # free in float32 as well
    assert free.sum() >= 8 and (~free).sum() >= 8
    for g in (full, host_run(model, d, k)):
        assert np.array_equal(g[0][free].astype(np.float64), q[free]) and (g[1][free] == 1).all() and (g[3][free] == rr.CONVERGED).all()
        assert not g[2][free].any() and (g[1][~free] > 1).any()
    # B = 0: a no-op, NULL pointers and all
    lib = _lib.load()
    assert lib.dexr_sphere_resolve_dev(model.handle, 0, None, None, None, None, 0, None, None, None, None, 0.01, 1.0, None, None, None, 1e-4, 0.0,
                                       0.0, 4, None, None, None, None, None) == 0
    x, it, en, st = model.resolve(np.zeros((0, model.n_in)), 0.01, 1e-4, 4)
    assert x.shape == (0, model.n_in) and it.shape == (0,) and en.shape == (0, 3) and st.shape == (0,)


# ---- 6. table limits: the synthetic robots of tests/pose_zoo.py ---------------------------------------------------------------------
ZB, ZMARGIN, ZR = 9, 0.020, 0.010


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("name", ["chain64", "binary64_slots8", "wide_map"])
def test_table_limits_float64(name, every, tmp_path, require_gpu):
    m = zoo.build(name, tmp_path)
    L = len(m.links)
    rows = np.arange(0, L, every)
    S = len(rows)
    centers = _r32(np.random.default_rng(61).uniform(-0.01, 0.01, (S, 3)))
    radii = np.full(S, ZR)
    pairs = np.array([(i, j) for i in range(S) for j in range(i + 1, S)], np.int32)
    model = _lib.SphereModel(m.blob, rows, centers, radii, pairs)
    assert (model.n_in, model.n_sphere, model.n_pair) == (zoo.FACTS[name]["n_in"], S, len(pairs))
    x, fixed, _ = zoo.inputs(m, ZB, 2043)
    d = dict(orc=m.orc, links=list(m.links), rows=rows, centers=centers, radii=radii, pairs=pairs, q=x, margin=_f32(ZMARGIN),
             u=np.full(x.shape[1], _f32(1e-4)), damping=_f32(1e-4), max_step=_f32(0.2), tol=0.0, wcol=1.0,
             full=lambda v: zoo.full_q(m.smap, v, fixed), fold=lambda J: zoo.fold(m.smap, J))
    res = ref_run(d, STEPS32)
    assert (res["energy"][0, :, 2] > 0).all() and (res["decisions"] == 1).any()
    got = host_run(model, d, STEPS32, fixed=fixed)
    ok = compare64(f"{name} every {every}", got, res, STEPS32, need=1)
    unread = zoo.abs_mult(m).sum(0) == 0
    functional(f"{name} every {every}", d, got, x, active=~unread)
    print(f"{name} every {every}: {S} spheres, {len(pairs)} pairs, {int((~unread).sum())} of {len(unread)} columns read, {int(ok.sum())} of {ZB} frames clear, "
          f"TRUNCATED on {int(((got[3] & rr.TRUNCATED) != 0).sum())}")
    if name == "wide_map":
        assert model.n_in == 256 and int(unread.sum()) == 233


# ---- 7. more active pairs than the list holds ----------------------------------------------------------------------------------------
def test_active_list_overflow_sets_truncated(require_gpu):
    name = "shadow_hand_right"
    robot, orc = robot_of(name)
    base = resolve_inputs(name)
    links = base["links"][:24]
    pairs = np.array([(i, j) for i in range(24) for j in range(i + 1, 24)], np.int32)
    assert len(pairs) == 276 > rr.MAXACTIVE
    for radius, truncated in ((0.3, True), (0.0, False)):
        radii = np.full(24, radius)
        sset = collision.SphereSet(links, np.zeros((24, 3)), radii, pairs)
        d = dict(base, links=links, rows=np.arange(24), centers=np.zeros((24, 3)), radii=radii, pairs=pairs, sset=sset)
        res = ref_run(d, STEPS32)
        active = (problem(d, x_ref=d["q"]).energies(d["q"])[1] > 0).sum(1)
        got = host_run(robot.sphere_model(sset), d, STEPS32)
        ok = compare64(f"overflow radius {radius}", got, res, STEPS32, need=1)
        functional(f"overflow radius {radius}", d, got, d["q"])
        print(f"radius {radius}: {active.min()} .. {active.max()} active pairs of 276 at x0, {int(ok.sum())} frames clear")
        if truncated:
            assert (active == 276).all() and ((got[3] & rr.TRUNCATED) != 0).all() and ((res["status"][-1] & rr.TRUNCATED) != 0).all()
            uncapped = rr.resolve(problem(d, max_active=10 ** 6), d["q"], d["damping"], 1, d["lo"], d["hi"], d["tol"], d["max_step"])
            assert np.abs(uncapped["xs"][1] - res["xs"][1]).max() > 1e-6  # the cap matters: the yardstick without it goes elsewhere
        else:
            assert (active <= rr.MAXACTIVE).all() and not (got[3] & rr.TRUNCATED).any()


# ---- 8. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    model, d = _target_case()
    n, n_in = 4, model.n_in
    x = torch.zeros((n, n_in), dtype=torch.float32, device="cuda")
    tp, tr, w = (torch.zeros(s, dtype=torch.float32, device="cuda") for s in ((n, 5, 3), (n, 5, 3, 3), (n, 5)))
    lim = torch.zeros((n_in,), dtype=torch.float32, device="cuda")
    out, en = _nan(torch, (n, n_in)), _nan(torch, (n, 3))
    it, st = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    INVALID = -1
    good = dict(m=model.handle, B=n, x0=x.data_ptr(), fixed=None, x_ref=None, u=None, n_target=5, tp=tp.data_ptr(), tr=tr.data_ptr(), wl=w.data_ptr(),
                wa=w.data_ptr(), margin=0.01, wcol=1.0, pw=None, lo=lim.data_ptr(), hi=lim.data_ptr(), damping=1e-4, max_step=0.2, tol=0.0,
                max_iters=4, x_out=out.data_ptr(), iters=it.data_ptr(), energy=en.data_ptr(), status=st.data_ptr())

    def invalid(word, **over):
        a = dict(good, **over)
        rc = lib.dexr_sphere_resolve_dev(*[a[k] for k in good], None)
        msg = lib.dexr_last_error()
        assert rc == INVALID and word in msg, (rc, msg, over)

    invalid(b"null sphere model", m=None)
    invalid(b"negative", B=-1)
    for bad in (-1e-6, float("nan"), float("inf")):
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
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.sphere_model(collision.SphereSet(["link_15.0_tip", "link_3.0_tip"], np.zeros((2, 3)), [0.01, 0.01], [(0, 1)]))
    assert ms.n_fixed == 6 and ms.n_in == 10
    invalid(b"fixed", m=ms.handle, n_target=0, tp=None, tr=None, wl=None, wa=None)
    # the host twin keeps the same rules
    z = np.zeros((n, n_in))
    zo, ze, zi, zs = np.full((n, n_in), np.nan), np.full((n, 3), np.nan), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))  # noqa: E731
    hgood = dict(m=model.handle, B=n, x0=dp(z), fixed=None, x_ref=None, u=None, n_target=0, tp=None, tr=None, wl=None, wa=None, margin=0.01, wcol=1.0,
                 pw=None, lo=None, hi=None, damping=1e-4, max_step=0.2, tol=0.0, max_iters=4, x_out=dp(zo), iters=ip(zi), energy=dp(ze), status=ip(zs))
    for word, over in ((b"null sphere model", dict(m=None)), (b"negative", dict(B=-2)), (b"margin", dict(margin=-1.0)), (b"damping", dict(damping=float("nan"))),
                       (b"max_iters", dict(max_iters=0)), (b"lo and hi", dict(lo=dp(z[0].copy()))), (b"n_target", dict(n_target=99)),
                       (b"both NULL", dict(n_target=2)), (b"x_out is NULL", dict(x_out=None)), (b"x0 is NULL", dict(x0=None))):
        a = dict(hgood, **over)
        rc = lib.dexr_sphere_resolve(*[a[k] for k in hgood])
        assert rc == INVALID and word in lib.dexr_last_error(), (word, rc, lib.dexr_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(en).all()) and bool((it == -7).all()) and bool((st == -7).all())  # nothing was launched
    assert np.isnan(zo).all() and np.isnan(ze).all() and (zi == -7).all() and (zs == -7).all()
    for kw in (dict(x_ref=z[:, :-1]), dict(posture_weight=np.zeros(n_in + 1)), dict(target_pos=np.zeros((n, 5, 2))), dict(lo=np.zeros(n_in)),
               dict(pair_weight=np.zeros(model.n_pair + 1))):
        with pytest.raises(ValueError):
            model.resolve(z, 0.01, 1e-4, 4, **kw)
    with pytest.raises(ValueError, match="required"):
        model.resolve(z, 0.01, 1e-4)


# ---- 9. the torch front ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "subset"])
def test_torch_front_equals_the_entry_points_bitwise(rel, require_gpu):
    torch = pytest.importorskip("torch")
    opt, prob, sset, pairs, d, fx = _opt_case(rel, 321)
    n, k = B, 6
    q, f = _dev(torch, d["q"]), _dev(torch, fx)
    tips = ["link_15.0_tip", "link_3.0_tip"]
    tp, trot = isr.link_poses(prob.robot, d["full"](_r32(d["q"] + 0.05)), tips)
    tpt, trt = _dev(torch, tp), _dev(torch, trot)
    wt = _dev(torch, np.random.default_rng(322).uniform(0.5, 2, (n, 2)))
    pw = _dev(torch, np.random.default_rng(323).uniform(0.5, 2.0, len(pairs)))
    lim = _dev(torch, np.stack([d["lo"], d["hi"]], 1))
    qref = _dev(torch, _r32(d["q"] + 0.01))
    ut = _dev(torch, np.random.default_rng(324).uniform(0, 1e-3, q.shape[1]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = side.cuda_stream
        # no targets: today's model of the set
        got = collision.resolve_self_collision(opt, q, sset, 0.01, 1e-4, k, 1e-3, fixed_qpos=f, limits=lim, max_step=0.2)
        model = opt.sphere_model(sset)
        assert opt.sphere_model(sset, pairs) is model
        u = torch.full((q.shape[1],), 1e-3, dtype=torch.float32, device="cuda")
        lo, hi = lim[:, 0].contiguous(), lim[:, 1].contiguous()
        wx, wi, we, ws = _nan(torch, tuple(q.shape)), torch.full((n,), -7, dtype=torch.int32, device="cuda"), _nan(torch, (n, 3)), torch.full((n,), -7, dtype=torch.int32, device="cuda")
        model.resolve_dev(n, q.data_ptr(), _ptr(f), 0.01, 1e-4, k, wx.data_ptr(), wi.data_ptr(), we.data_ptr(), ws.data_ptr(), posture_weight_ptr=u.data_ptr(),
                          lo_ptr=lo.data_ptr(), hi_ptr=hi.data_ptr(), max_step=0.2, stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(got, (wx, wi, we, ws))) and not got[0].requires_grad
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].shape == (n, 3) and got[3].dtype == torch.int32
        assert bool((we[:, 2] > 0).any()) and bool(torch.isfinite(wx).all())
        # everything at once, with targets: a model keyed by the target links
        got = collision.resolve_self_collision(opt, q, sset, 0.01, 1e-4, k, ut, qref, 2.0, pw, tips, tpt, trt, wt, wt, 1e-7, 0.2, lim, f)
        tm = opt.sphere_model(sset, pairs, tips)
        assert tm is not model and opt.sphere_model(sset, pairs, tuple(tips)) is tm
        tm.resolve_dev(n, q.data_ptr(), _ptr(f), 0.01, 1e-4, k, wx.data_ptr(), wi.data_ptr(), we.data_ptr(), ws.data_ptr(), x_ref_ptr=qref.data_ptr(),
                       posture_weight_ptr=ut.data_ptr(), n_target=2, target_pos_ptr=tpt.data_ptr(), target_rot_ptr=trt.data_ptr(), pos_weight_ptr=wt.data_ptr(),
                       rot_weight_ptr=wt.data_ptr(), collision_weight=2.0, pair_weight_ptr=pw.data_ptr(), lo_ptr=lo.data_ptr(), hi_ptr=hi.data_ptr(),
                       tol=1e-7, max_step=0.2, stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(got, (wx, wi, we, ws))) and bool((we[:, 0] > 0).all())
        # non-contiguous inputs: views with the same values
        qn, tn = torch.stack([q, q], 2)[:, :, 0], torch.stack([tpt, tpt], 3)[..., 1]
        assert not qn.is_contiguous() and not tn.is_contiguous()
        again = collision.resolve_self_collision(opt, qn, sset, 0.01, 1e-4, k, ut, qref, 2.0, pw, tips, tn, trt, wt, wt, 1e-7, 0.2, lim, f)
        assert all(torch.equal(a, b) for a, b in zip(again, got))
        # the robot twin over the full qpos
        robot = opt.robot
        rl = robot.joint_limits
        qr = _dev(torch, np.random.default_rng(325).uniform(rl[:, 0], rl[:, 1], (n, robot.dof)))
        rlim = _dev(torch, rl)
        tpr, _ = isr.link_poses(prob.robot, qr.cpu().numpy().astype(np.float64) + 0.05, tips)
        tprt = _dev(torch, tpr)
        gr = collision.robot_resolve_self_collision(robot, qr, sset, 0.01, 1e-4, k, 1e-3, link_names=tips, target_pos=tprt, limits=rlim)
        rm = robot.sphere_model(sset, pairs, tips)
        ur = torch.full((robot.dof,), 1e-3, dtype=torch.float32, device="cuda")
        rlo, rhi = rlim[:, 0].contiguous(), rlim[:, 1].contiguous()
        rx, re_ = _nan(torch, (n, robot.dof)), _nan(torch, (n, 3))
        rm.resolve_dev(n, qr.data_ptr(), 0, 0.01, 1e-4, k, rx.data_ptr(), wi.data_ptr(), re_.data_ptr(), ws.data_ptr(), posture_weight_ptr=ur.data_ptr(),
                       n_target=2, target_pos_ptr=tprt.data_ptr(), lo_ptr=rlo.data_ptr(), hi_ptr=rhi.data_ptr(), stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(gr, (rx, wi, re_, ws)))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e = torch.zeros((0, opt.opt_dof), device="cuda")
    out = collision.resolve_self_collision(opt, e, sset, 0.01, 1e-4, k, fixed_qpos=None if f is None else f[:0])
    assert out[0].shape == (0, opt.opt_dof) and out[1].shape == (0,) and out[2].shape == (0, 3) and out[3].shape == (0,)


def test_retarget_then_resolve_end_to_end(require_gpu):
    torch = pytest.importorskip("torch")
    import test_gpu_link_poses as glp
    from dex_retargeting_amd import autograd as ag

    rel = "teleop/allegro_hand_right.yml"
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    n = 256
    hs = cases.human_set(prob, n)
    # one sphere per fingertip and per middle link of a finger
    names = ["link_3.0_tip", "link_7.0_tip", "link_11.0_tip", "link_15.0_tip", "link_2.0", "link_6.0", "link_10.0", "link_14.0"]
    sset = collision.SphereSet(names, np.zeros((8, 3)), np.full(8, 0.020))
    kp = glp._t(hs["kp"], torch, dtype=torch.float32)
    last = glp._t(hs["last"], torch)
    fixed = glp._t(hs["fixed"], torch) if hs["fixed"].shape[1] else None
    q = ag.retarget(opt, ag.ref_value_from_keypoints(opt, kp), last, fixed, None).detach()
    margin, u = 0.010, 1e-3
    E0, _ = collision.self_collision_penalty(opt, q, sset, margin, None, fixed)
    x, iters, energy, status = collision.resolve_self_collision(opt, q, sset, margin, 1e-4, 16, u, fixed_qpos=fixed, max_step=0.2)
    E1, _ = collision.self_collision_penalty(opt, x, sset, margin, None, fixed)
    total0, total1 = E0.double(), E1.double() + u * ((x - q).double() ** 2).sum(1)
    print(f"retarget -> resolve: {int((E0 > 0).sum())} of {n} frames start in collision, collision energy {float(E0.sum()):.3e} -> {float(E1.sum()):.3e}, "
          f"iters {torch.bincount(iters).tolist()}, status {torch.bincount(status, minlength=8).tolist()}")
    assert bool((E0 > 0).any()) and bool(torch.isfinite(x).all())
    assert bool((total1 <= total0 * (1 + RISE)).all())  # total E does not rise (the kernel's own float32 sums against torch's)
    assert float(E1.sum()) < float(E0.sum()) and not bool((status & ~BITS).any()) and bool((iters >= 1).all()) and bool((iters <= 16).all())
    assert torch.equal(energy[:, 0], torch.zeros_like(energy[:, 0]))

"""GPU tests of the posture solve against a second posed robot (csrc/dexr_resolve_cross.hpp, include/dexr_resolve_cross.h): the
float64 host twin against tests/resolve_cross_reference.py, the float32 device entry point against the host twin, the solve against
three existing kernels (dexr_sphere_resolve with B out of reach, dexr_cross_penalty for E_x, the one-body scene solve on B
re-expressed as sphere primitives), the contract (NULL pose, row independence and isolation, aliasing, masked pairs, a robot against
its own handle), the contact cap inside a row of B's spheres and exactly between two spheres of A, the table limits with the header's
byte formula, the raw ABI's argument errors and the torch fronts, the alternating two-robot front among them.

INPUTS and DECISION GUARDS: tests/test_resolve_cross_host.py (cross_resolve_inputs, reference; B = 33: three blocks of sixteen frames,
the last with one frame), whose reference runs are proven there on the CPU and shared from there.  A comparison against the yardstick
is made on the frames that are CLEAR at its guards; every frame goes through the functional checks (finite, inside the limits, unread
columns unchanged, the four-term E recomputed by the yardstick in float64 does not rise).

GATES, those of tests/test_gpu_resolve.py, imported: float64 GATE64 on x and the four energies, iters and status equal; float32 max
|x32 - x64| over the clear frames at most GATE32 x the distance between the yardstick's own float32 and float64 runs there;
E(answer) <= E(x0) (1 + RISE)."""
import os

import numpy as np
import pytest

import collision_reference as cref
import ik_solve_reference as isr
import pose_zoo as zoo
import resolve_cross_reference as rxr
import resolve_reference as rr
from dex_retargeting_amd import _lib, collision
from test_collision_host import B, robot_of
from test_cross_host import place, wrapper_of
from test_gpu_resolve import GATE32, GATE64, RISE, _dev, _nan, _opt_case, _ptr, compare64
from test_gpu_resolve_grid import _table_facts
from dex_retargeting_amd import pose_tables as pt
from test_resolve_cross_host import PAIRS, cross_problem, cross_resolve_inputs, header_bytes, place_other, reference, reference_run
from test_resolve_host import GUARD32, GUARD64, STEPS32, STEPS64, _f32, _r32
from test_resolve_scene_host import body

pytestmark = pytest.mark.gpu
BITS = rxr.CONVERGED | rxr.STALLED | rxr.TRUNCATED | rxr.CONTACTS_TRUNCATED
INVALID, UNSUPPORTED = -1, -3


def models(case):
    d = cross_resolve_inputs(case)
    na, nb = PAIRS[case]
    return robot_of(na)[0].sphere_model(d["sset"]), wrapper_of(nb).sphere_model(d["b"]["sset"])


def host_run(ma, mb, d, max_iters, fixed=None, **over):
    """-> (x, iters, energy (B, 4), status) of dexr_sphere_resolve_cross on a dict of cross_resolve_inputs."""
    a = dict(d, **over)
    return ma.resolve_cross(mb, a["q"], a["q_b"], a["margin"], a["damping"], max_iters, fixed, a.get("fixed_b"), a.get("x_ref"), a.get("u"),
                            a.get("tgt_pos"), a.get("tgt_rot"), a.get("w_pos"), a.get("w_rot"), a["wcol"], a.get("pair_weight"), a.get("lo"), a.get("hi"),
                            a["tol"], a["max_step"], n_target=a.get("n_target", 0), other_pos=a.get("opos"), other_rot=a.get("orot"),
                            cross_margin=a["xmargin"], cross_weight=a["wx"], cross_pair_weight=a.get("xw"))


def dev_run(ma, mb, torch, d, max_iters, fixed=None, rows=slice(None), alias=False, **over):
    """the same of dexr_sphere_resolve_cross_dev on the frames `rows` of d, the outputs pre-filled with NaN / -7; alias: x_out is x0's
    buffer."""
    a = dict(d, **over)
    cut = lambda v: None if v is None else v[rows]  # noqa: E731
    x0, tf, xr, tp, tr, wl, wa, xb, fb, op, orot = (_dev(torch, cut(v)) for v in (a["q"], fixed, a.get("x_ref"), a.get("tgt_pos"), a.get("tgt_rot"), a.get("w_pos"),
                                                                                   a.get("w_rot"), a["q_b"], a.get("fixed_b"), a.get("opos"), a.get("orot")))
    u, pw, lo, hi, xw = (_dev(torch, a.get(k)) for k in ("u", "pair_weight", "lo", "hi", "xw"))
    n = x0.shape[0]
    x = x0 if alias else _nan(torch, (n, ma.n_in))
    iters, status = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    energy = _nan(torch, (n, 4))
    ma.resolve_cross_dev(mb, n, _ptr(x0), _ptr(tf), _ptr(xb), _ptr(fb), a["margin"], a["damping"], max_iters, _ptr(x), _ptr(iters), _ptr(energy),
                         _ptr(status), x_ref_ptr=_ptr(xr), posture_weight_ptr=_ptr(u), n_target=a.get("n_target", 0), target_pos_ptr=_ptr(tp),
                         target_rot_ptr=_ptr(tr), pos_weight_ptr=_ptr(wl), rot_weight_ptr=_ptr(wa), collision_weight=a["wcol"], pair_weight_ptr=_ptr(pw),
                         lo_ptr=_ptr(lo), hi_ptr=_ptr(hi), tol=a["tol"], max_step=a["max_step"], other_pos_ptr=_ptr(op), other_rot_ptr=_ptr(orot),
                         cross_margin=a["xmargin"], cross_weight=a["wx"], cross_pair_weight_ptr=_ptr(xw), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return x.cpu().numpy(), iters.cpu().numpy(), energy.cpu().numpy(), status.cpu().numpy()


def functional(tag, d, got, x0, active=None, rise=RISE):
    """test_gpu_resolve.functional with the four-term energy: what holds on EVERY frame, clear or not."""
    x, iters, energy, status = (np.asarray(a) for a in got)
    x = x.astype(np.float64)
    assert energy.shape == (len(x), 4) and np.isfinite(x).all() and np.isfinite(energy).all() and not (status & ~BITS).any() and (iters >= 1).all(), tag
    P = cross_problem(d)
    if P.x_ref is None:
        P.x_ref = np.asarray(x0, np.float64)
    if active is None:
        active = isr.active_columns(P.orc, np.asarray(P.full(x0), np.float64), P.links, P.fold)
    if d.get("lo") is not None:
        assert ((x >= d["lo"]) & (x <= d["hi"]))[:, active].all(), tag
    assert np.array_equal(x[:, ~active], np.asarray(x0, np.float64)[:, ~active]), tag
    E0, E1 = P.energies(np.asarray(x0, np.float64))[0].sum(1), P.energies(x)[0].sum(1)
    worst = float((E1 - E0 * (1 + rise)).max())
    print(f"{tag}: E {np.median(E0):.3e} -> {np.median(E1):.3e} (medians), max (E(answer) - E(x0) (1 + {rise:g})) = {worst:.3e}")
    assert (E1 <= E0 * (1 + rise)).all(), (tag, worst)
    return E0, E1


def same_bits(a, b):
    return all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


# ---- 1. the float64 host twin against the yardstick ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PAIRS))
def test_host_float64_against_the_reference(case, require_gpu):
    assert len(PAIRS) == 5 and B == 33
    d, res = cross_resolve_inputs(case), reference(case)
    ma, mb = models(case)
    assert (ma.n_in, ma.n_fixed, ma.n_sphere, ma.n_pair) == (d["orc"].dof, 0, d["sset"].n_sphere, len(d["pairs"])) and mb.n_sphere == len(d["b"]["radii"])
    assert (res["decisions"] == 1).any() and (res["decisions"] == 0).any() and 2 * (res["energy"][0, :, 3] > 0).sum() >= B
    for k in (1, 2, 3, STEPS64):
        got = host_run(ma, mb, d, k)
        compare64(case, got, res, k)
        functional(f"{case} float64 {k}", d, got, d["q"])


# ---- 2. the float32 device entry point against the host twin ------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PAIRS))
def test_device_float32_against_the_host_twin(case, require_gpu):
    torch = pytest.importorskip("torch")
    d, r64, r32 = cross_resolve_inputs(case), reference(case), reference(case, np.float32, STEPS32)
    ma, mb = models(case)
    ok = rxr.clear(r64, STEPS32, *GUARD32)
    assert 2 * ok.sum() >= B
    x64 = host_run(ma, mb, d, STEPS32)[0]
    got = dev_run(ma, mb, torch, d, STEPS32)
    assert got[0].dtype == np.float32 and got[0].shape == x64.shape and got[2].shape == (B, 4)
    dist = float(np.abs(r32["xs"][STEPS32].astype(np.float64) - r64["xs"][STEPS32])[ok].max())
    e = float(np.abs(got[0].astype(np.float64) - x64)[ok].max())
    ratio = e / dist if dist > 0 else (0.0 if e == 0 else float("inf"))
    print(f"{case}: {int(ok.sum())} of {B} frames clear at the float32 guards; float32 max |x - x64| = {e:.3e}, the yardstick's float32 run is "
          f"{dist:.3e} from its float64 run (error / reference distance {ratio:.2f}, gate {GATE32:g})")
    assert ratio <= GATE32, (case, e, dist)
    for k in (STEPS32, 16):  # every frame, clear or not
        g = got if k == STEPS32 else dev_run(ma, mb, torch, d, k)
        functional(f"{case} float32 {k}", d, g, d["q"])
        assert (g[1] <= k).all()


# ---- 3. against existing kernels, which are independent code ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["allegro_right_left", "shadow_right_left"])
def test_the_other_robot_out_of_reach_is_the_plain_solve_bit_for_bit(case, require_gpu):
    torch = pytest.importorskip("torch")
    import test_gpu_resolve as plain

    d = cross_resolve_inputs(case)
    ma, mb = models(case)
    away = dict(d, opos=_r32(d["opos"] + np.where(d["far"][:, None], 0.0, 10.0)))  # every frame 10 m away (the far frames are already)
    k = STEPS64
    got, want = host_run(ma, mb, away, k), plain.host_run(ma, d, k)
    assert same_bits((got[0], got[1], got[2][:, :3], got[3]), want) and not got[2][:, 3].any() and not np.signbit(got[2][:, 3]).any()
    g32, w32 = dev_run(ma, mb, torch, away, k), plain.dev_run(ma, torch, d, k)
    assert same_bits((g32[0], g32[1], g32[2][:, :3], g32[3]), w32) and not g32[2][:, 3].any() and not np.signbit(g32[2][:, 3]).any()
    assert (want[2][:, 2] > 0).any() and np.abs(want[0] - d["q"]).max() > 1e-3  # the plain solve had work to do


@pytest.mark.parametrize("case", ["shadow_allegro", "leap_same"])
def test_the_cross_energy_is_the_penalty_kernels(case, require_gpu):
    torch = pytest.importorskip("torch")
    d = dict(cross_resolve_inputs(case), wx=1.0)
    ma, mb = models(case)
    x, _, energy, _ = host_run(ma, mb, d, STEPS32)
    E = ma.cross_penalty(mb, x, d["q_b"], d["xmargin"], d["xw"], pos_b=d["opos"], rot_b=d["orot"], want_grad_a=False, want_grad_b=False,
                         want_wrench_a=False, want_wrench_b=False)[0]
    assert (E > 0).any() and np.allclose(energy[:, 3], E, rtol=1e-12, atol=0)
    x32, _, e32, _ = dev_run(ma, mb, torch, d, STEPS32)
    xa, xb, op, orot, xw = (_dev(torch, a) for a in (x32, d["q_b"], d["opos"], d["orot"], d["xw"]))
    e = _nan(torch, (B,))
    ma.cross_penalty_dev(mb, B, xa.data_ptr(), 0, xb.data_ptr(), 0, d["xmargin"], xw.data_ptr(), e.data_ptr(), 0, 0, pos_b_ptr=op.data_ptr(),
                         rot_b_ptr=orot.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.allclose(e32[:, 3], e.cpu().numpy(), rtol=1e-5, atol=0)
    print(f"{case}: E_x against dexr_cross_penalty: float64 max |difference| {np.abs(energy[:, 3] - E).max():.2e}, float32 "
          f"{np.abs(e32[:, 3] - e.cpu().numpy()).max():.2e}; max E_x {E.max():.3e}")


@pytest.mark.parametrize("case", ["allegro_right_left", "shadow_right_left"])
def test_one_held_posture_is_a_scene_of_sphere_primitives(case, require_gpu):
    """B held at ONE posture on all frames is a rigid body: its centres in its root frame become an ObstacleSet of sphere primitives,
    posed by other_pos / other_rot, and the parent's one-body scene solve is the same problem through other code.  The two headers
    place a body differently -- C = pos + rot c here and in dexr_cross.h, y = rot^T (C - pos) in dexr_obstacles.h -- which is one
    geometry only where rot is orthonormal: the inputs' rotations, rounded to float32, are orthonormal to 6e-8 and move a centre by
    1e-8 m between the two (measured: x apart by 4e-7 rad at a gate of 1e-9).  Both entry points are float64 host twins, so this
    test gives them the nearest rotations that are orthonormal in float64 (the polar factor of each)."""
    import test_gpu_resolve_scene as gs

    base = cross_resolve_inputs(case)
    b = base["b"]
    assert len(b["radii"]) <= _lib.OBSTACLE_MAX
    q_b = np.ascontiguousarray(np.tile(base["q_b"][:1], (B, 1)))
    U, _, Vt = np.linalg.svd(base["orot"])
    orot = np.ascontiguousarray(U @ Vt)
    assert np.abs(orot - base["orot"]).max() < 1e-6 and np.abs(orot @ orot.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    base = dict(base, orot=orot)
    d = dict(base, q_b=q_b, xw=None)
    cb = cref.centres(b["orc"], q_b[:1], b["links"], b["rows"], b["centers"])[0][0]
    oset = collision.ObstacleSet.spheres(cb, b["radii"])
    res = reference_run(d, STEPS64)
    ok = rxr.clear(res, STEPS64, *GUARD64)
    assert 2 * ok.sum() >= B and (res["energy"][0, :, 3] > 0).any()
    ma, mb = models(case)
    got = host_run(ma, mb, d, STEPS64)
    compare64(f"{case} one posture", got, res, STEPS64)
    want = gs.host_run(ma, dict(base, bodies=(body(oset, base["opos"], base["orot"], base["xmargin"], base["wx"]),)), STEPS64)
    ex, ee = float(np.abs(got[0] - want[0])[ok].max()), float(np.abs(got[2] - want[2][:, :4])[ok].max())
    print(f"{case}: against the one-body scene solve on {len(b['radii'])} sphere primitives, {int(ok.sum())} clear frames: max |x - x| = {ex:.3e}, "
          f"energies {ee:.3e} (gate {GATE64:.0e})")
    assert ex <= GATE64 and ee <= GATE64 and np.array_equal(got[1][ok], want[1][ok]) and np.array_equal(got[3][ok], want[3][ok])


# ---- 4. the contract --------------------------------------------------------------------------------------------------------------------
def test_null_pose_equals_explicit_zeros_and_identity(require_gpu):
    torch = pytest.importorskip("torch")
    case = "leap_same"
    base = cross_resolve_inputs(case)
    ma, mb = models(case)
    # B at A's origin with no pose: the two hands overlap and the spheres at the two base origins COINCIDE on every frame -- the
    # contact without a direction, which counts in E_x with h = margin_x + r_s + r_t and adds neither force nor curvature
    none = dict(base, opos=None, orot=None)
    expl = dict(base, opos=np.zeros((B, 3)), orot=np.tile(np.eye(3), (B, 1, 1)))
    res = reference_run(none, STEPS32)
    assert float(res["closest"]) == 0.0
    a, b = host_run(ma, mb, none, STEPS32), host_run(ma, mb, expl, STEPS32)
    assert same_bits(a, b) and (a[2][:, 3] > 0).all()
    compare64("coincident centres", a, res, STEPS32, need=1)
    a32, b32 = dev_run(ma, mb, torch, none, STEPS32), dev_run(ma, mb, torch, expl, STEPS32)
    assert same_bits(a32, b32) and np.isfinite(a32[0]).all()
    for half in (dict(opos=None), dict(orot=None)):
        assert same_bits(dev_run(ma, mb, torch, dict(base, **half), STEPS32),
                         dev_run(ma, mb, torch, dict(base, **{k: expl[k] for k in half}), STEPS32))


def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    case, k = "allegro_right_left", 5
    d = cross_resolve_inputs(case)
    ma, mb = models(case)
    full = dev_run(ma, mb, torch, d, k)
    assert not np.isnan(full[0]).any() and not np.isnan(full[2]).any() and (full[1] != -7).all() and (full[3] != -7).all()  # all overwritten
    assert (full[2][:, 3] > 0).any() and len(set(full[1].tolist())) > 1
    for rows in (slice(0, 1), slice(1, 17), slice(15, 33), slice(32, 33)):  # whole against slices: the same bits
        part = dev_run(ma, mb, torch, d, k, rows=rows)
        assert all(np.array_equal(u, v[rows]) for u, v in zip(part, full)), rows
    perm = np.random.default_rng(77).permutation(B)  # a permuted batch
    pd = dict(d, **{key: np.ascontiguousarray(d[key][perm]) for key in ("q", "q_b", "opos", "orot")})
    part = dev_run(ma, mb, torch, pd, k)
    assert all(np.array_equal(u, v[perm]) for u, v in zip(part, full))
    assert same_bits(dev_run(ma, mb, torch, d, k, alias=True), full)  # x_out aliasing x0
    h64 = host_run(ma, mb, d, k)
    part = host_run(ma, mb, dict(d, q=d["q"][16:], q_b=d["q_b"][16:], opos=d["opos"][16:], orot=d["orot"][16:]), k)
    assert all(np.array_equal(u, v[16:]) for u, v in zip(part, h64))
    # a NaN in x_b of frame 7 and a NaN in other_rot of frame 9 spoil those frames alone, which still end within k trials
    bad_q, bad_r = d["q_b"].copy(), d["orot"].copy()
    bad_q[7, 2] = np.nan
    bad_r[9, 1, 1] = np.nan
    bad = dict(d, q_b=bad_q, orot=bad_r)
    got = dev_run(ma, mb, torch, bad, k)
    keep = ~np.isin(np.arange(B), (7, 9))
    assert all(np.array_equal(u[keep], v[keep]) for u, v in zip(got, full))
    for f in (7, 9):
        assert 1 <= got[1][f] <= k and not (got[3][f] & ~BITS) and np.isnan(got[2][f, 3])
        assert np.array_equal(got[0][f], d["q"][f].astype(np.float32))  # (x0: the one point it accepts)
    h = host_run(ma, mb, bad, k)
    assert all(np.array_equal(u[keep], v[keep]) for u, v in zip(h, h64)) and (h[1][[7, 9]] <= k).all()
    # B = 0: a no-op, NULL pointers and all
    lib = _lib.load()
    z4, z3 = (None,) * 4, (None,) * 3
    assert lib.dexr_sphere_resolve_cross_dev(ma.handle, 0, *z4, 0, *z4, 0.01, 1.0, *z3, 1e-4, 0.0, 0.0, 4, mb.handle, *z4, 0.01, 1.0, None, *z4, None) == 0
    out = ma.resolve_cross(mb, np.zeros((0, ma.n_in)), np.zeros((0, mb.n_in)), 0.01, 1e-4, 4)
    assert out[0].shape == (0, ma.n_in) and out[1].shape == (0,) and out[2].shape == (0, 4) and out[3].shape == (0,)


def test_a_masked_pair_equals_its_absence(require_gpu):
    """cross_weight zero on every pair of one sphere of B against that sphere's absence from B's set: the same bits (no frame comes
    near the cap, where a masked contact would still take a place in the list)."""
    torch = pytest.importorskip("torch")
    case = "allegro_right_left"
    d = cross_resolve_inputs(case)
    ma, mb = models(case)
    P = cross_problem(d, x_ref=d["q"])
    hx = P.energies(d["q"])[1][1]
    j = int((hx > 0).sum((0, 1)).argmax())  # B's sphere with the most contacts at x0
    assert (hx[:, :, j] > 0).sum() >= 8 and (hx > 0).sum((1, 2)).max() < rxr.MAXCONTACT // 2
    xw = d["xw"].copy()
    xw[:, j] = 0.0
    keep = np.arange(len(d["b"]["radii"])) != j
    sb = d["b"]["sset"]
    less = collision.SphereSet([n for n, kp in zip(sb.links, keep) if kp], d["b"]["centers"][keep], d["b"]["radii"][keep], [(0, 1)])
    ml = wrapper_of(PAIRS[case][1]).sphere_model(less)
    assert ml.n_sphere == mb.n_sphere - 1
    masked, absent = host_run(ma, mb, dict(d, xw=xw), STEPS64), host_run(ma, ml, dict(d, xw=np.ascontiguousarray(d["xw"][:, keep])), STEPS64)
    assert same_bits(masked, absent)
    weighted = host_run(ma, mb, d, STEPS64)
    assert np.abs(weighted[0] - masked[0]).max() > 1e-6  # the sphere matters
    m32 = dev_run(ma, mb, torch, dict(d, xw=xw), STEPS32)
    a32 = dev_run(ma, ml, torch, dict(d, xw=np.ascontiguousarray(d["xw"][:, keep])), STEPS32)
    assert same_bits(m32, a32)


def test_a_robot_against_its_own_handle(require_gpu):
    torch = pytest.importorskip("torch")
    base = cross_resolve_inputs("leap_same")
    ma = models("leap_same")[0]
    own = dict(orc=base["orc"], links=base["links"], rows=base["rows"], centers=base["centers"], radii=base["radii"], sset=base["sset"])
    q_b = np.ascontiguousarray(base["q"][::-1])
    ca = cref.centres(base["orc"], base["q"], base["links"], base["rows"], base["centers"])[0]
    cb = cref.centres(base["orc"], q_b, base["links"], base["rows"], base["centers"])[0]
    opos, orot = place_other(ca, cb, 3, B)
    S = len(base["radii"])
    d = dict(base, b=own, q_b=q_b, opos=opos, orot=orot, xw=_r32(np.random.default_rng(78).uniform(0.5, 2, (S, S))))
    res = reference_run(d, STEPS32)
    assert (res["energy"][0, :, 3] > 0).sum() >= 4
    got = host_run(ma, ma, d, STEPS32)
    compare64("own handle", got, res, STEPS32, need=1)
    functional("own handle", d, got, d["q"])
    functional("own handle float32", d, dev_run(ma, ma, torch, d, STEPS32), d["q"])


# ---- 5. the cap -------------------------------------------------------------------------------------------------------------------------
def _inflated(case, n_b, radius, seed):
    """cross_resolve_inputs(case) with a synthetic B on the same robot: n_b spheres dealt round its links at seeded offsets, all of
    `radius`, so that every sphere of A is in contact with every sphere of B on the near frames."""
    base = cross_resolve_inputs(case)
    b = base["b"]
    L = len(b["links"])
    rows = np.arange(n_b) % L
    centers = _r32(np.random.default_rng(seed).uniform(-0.01, 0.01, (n_b, 3)))
    radii = np.full(n_b, radius)
    sset = collision.SphereSet([b["links"][r] for r in rows], centers, radii, [(0, 1)])
    S = len(base["radii"])
    nb = dict(orc=b["orc"], links=b["links"], rows=rows, centers=centers, radii=radii, sset=sset)
    return dict(base, b=nb, xw=_r32(np.random.default_rng(seed + 1).uniform(0.5, 2, (S, n_b)))), wrapper_of(PAIRS[case][1]).sphere_model(sset)


@pytest.mark.parametrize("n_b,where", [(44, "inside a row"), (64, "between two rows")])
def test_the_contact_cap(n_b, where, require_gpu):
    """Allegro right (22 spheres) against a synthetic left hand of n_b spheres of radius 0.5 m: on the near frames every (s, t) is
    active, 22 n_b contacts.  n_b = 44: the first 256 are five whole rows (220) and 36 of the caller's sphere 5 -- the cap falls INSIDE
    that sphere's row of B's spheres.  n_b = 64: 256 = 4 x 64 -- the cap falls exactly BETWEEN the caller's spheres 3 and 4.  The far
    frames have no contact and no bit."""
    torch = pytest.importorskip("torch")
    case = "allegro_right_left"
    d, mb = _inflated(case, n_b, 0.5, 81)
    ma = models(case)[0]
    S, near = len(d["radii"]), ~d["far"]
    hx = cross_problem(d, x_ref=d["q"]).energies(d["q"])[1][1]
    assert hx.shape == (B, S, n_b) and (hx[near] > 0).all() and not (hx[d["far"]] > 0).any() and S * n_b > rxr.MAXCONTACT
    first = np.cumsum((hx > 0).reshape(B, S * n_b), 1).reshape(B, S, n_b) <= rxr.MAXCONTACT
    if where == "inside a row":
        assert first[near][:, :5].all() and (first[near][:, 5].sum(1) == 36).all() and first[near][:, 5, :36].all() and not first[near][:, 6:].any()
    else:
        assert first[near][:, :4].all() and not first[near][:, 4:].any()
    res = reference_run(d, STEPS32)
    over = np.stack([(cross_problem(d, x_ref=d["q"]).energies(x)[1][1] > 0).sum((1, 2)) > rxr.MAXCONTACT for x in res["xs"]]).any(0)
    assert np.array_equal(over, near)
    got = host_run(ma, mb, d, STEPS32)
    ok = compare64(f"cap {where}", got, res, STEPS32, need=1)
    functional(f"cap {where}", d, got, d["q"])
    want_bit = (res["status"][-1] & rxr.CONTACTS_TRUNCATED) != 0
    assert np.array_equal(want_bit, near) and np.array_equal((got[3] & rxr.CONTACTS_TRUNCATED) != 0, want_bit)
    assert not (got[3] & rxr.TRUNCATED).any()  # the pair side keeps its own bit
    uncapped = reference_run(d, 1, max_contact=10 ** 6)
    assert (ok & near).any() and np.abs(uncapped["xs"][1] - res["xs"][1])[ok & near].max() > 1e-6  # the cap matters: without it the yardstick goes elsewhere
    g32 = dev_run(ma, mb, torch, d, STEPS32)
    functional(f"cap {where} float32", d, g32, d["q"])
    assert np.array_equal((g32[3] & rxr.CONTACTS_TRUNCATED) != 0, near)
    print(f"cap {where}: {S} x {n_b} = {S * n_b} contacts on {int(near.sum())} frames, {int(ok.sum())} frames clear")


# ---- 6. table limits: the synthetic robots of tests/pose_zoo.py, and the header's byte formula ---------------------------------------
ZB, ZR = 9, 0.010
ZOO_CASES = ("2 against 128", "128 against 2", "128 against 2 behind 256 columns with targets")


def _zoo_side(m, n_sphere, seed, wide=False):
    """one robot of a table-limit case, plain data: n_sphere spheres dealt round the links of the zoo member m (two: its first and its
    last link); wide: the member's joints behind a source map of 256 columns, every fourth one read."""
    L = len(m.links)
    rows = np.arange(n_sphere) % L if n_sphere > 2 else np.array([0, L - 1])
    centers = _r32(np.random.default_rng(seed).uniform(-0.01, 0.01, (n_sphere, 3)))
    pairs = np.array([(i, j) for i in range(n_sphere) for j in range(i + 1, n_sphere)], np.int32)
    blob, smap = m.blob, m.smap
    x, fixed = zoo.inputs(m, ZB, 2043 + seed)[:2]
    unread = zoo.abs_mult(m).sum(0) == 0
    if wide:
        smap = pt.SourceMap(256, 0, [(pt.SRC_X, 4 * k, 1.0, 0.0) for k in range(len(m.smap.entries))])
        blob = zoo._renumber_slots(pt.compile_poses(m.kin, m.links, smap))  # (the member's eight slots, as zoo.build numbers them)
        x, fixed = _r32(np.random.default_rng(2043 + seed).uniform(-0.5, 0.5, (ZB, 256))), None
        unread = np.array([c % 4 != 0 for c in range(256)])
    return dict(m=m, rows=rows, centers=centers, radii=np.full(n_sphere, ZR), pairs=pairs, x=x, fixed=fixed, blob=blob, smap=smap, unread=unread)


def zoo_case(tag, directory):
    """-> (a, b, d, run, need64, need32): the two sides, the yardstick's dict, the entry points' dict and the header's bytes."""
    big, small = zoo.build("binary64_slots8", directory), zoo.build("chain64", directory)
    wide = "256 columns" in tag
    a, b = (_zoo_side(small, 2, 1), _zoo_side(big, 128, 2)) if tag.startswith("2 ") else (_zoo_side(big, 128, 1, wide), _zoo_side(small, 2, 2))
    fa, fb = _table_facts(a["blob"]), _table_facts(b["blob"])
    fbig = fb if tag.startswith("2 ") else fa
    assert fbig["n_slot"] == 8 and fbig["n_jx"] == 64  # the 8-slot / 64-joint member is the side with the 128 spheres
    m, sa, sb, nt = a["m"], len(a["radii"]), len(b["radii"]), 3 if wide else 0
    need = [header_bytes(v, fa["n_jx"], fa["n_link"] if nt else 0, sa, fa["n_act"], fa["n_in"], len(a["pairs"]), sb, fa["n_slot"], fb["n_slot"]) for v in (8, 4)]
    d = dict(orc=m.orc, links=list(m.links), rows=a["rows"], centers=a["centers"], radii=a["radii"], pairs=a["pairs"], q=a["x"], margin=_f32(0.020),
             u=np.full(a["x"].shape[1], _f32(1e-4)), damping=_f32(1e-4), max_step=_f32(0.2), tol=0.0, wcol=1.0,
             full=lambda v, s=a["smap"], f=a["fixed"]: zoo.full_q(s, v, f), fold=lambda J, s=a["smap"]: zoo.fold(s, J),
             b=dict(orc=b["m"].orc, links=list(b["m"].links), rows=b["rows"], centers=b["centers"], radii=b["radii"]),
             q_b=zoo.full_q(b["smap"], b["x"], b["fixed"]), opos=_r32(np.tile((0.05, -0.02, 0.03), (ZB, 1))), orot=None, xmargin=_f32(1.0), wx=0.5,
             xw=_r32(np.random.default_rng(63).uniform(0.5, 2, (sa, sb))))
    if nt:
        tp, trot = isr.link_poses(m.orc, d["full"](_r32(a["x"] + 0.05)), list(m.links)[:nt])
        d.update(n_target=nt, tgt_pos=tp, tgt_rot=trot)
    run = dict(d, q_b=b["x"], fixed_b=b["fixed"])  # the entry points take B's variables, the yardstick its joint vector
    return a, b, d, run, need[0], need[1]


def test_table_limits_float64_solve_or_are_refused_by_the_formula(tmp_path, require_gpu):
    """2 spheres against 128 and 128 against 2, the 8-slot / 64-joint member of the zoo on the side that has the 128 (as B its eight
    slots and its 384 centre values are the cross term's share of the frame), and that robot as A behind 256 columns with targets:
    float64 solves, or is refused with exactly the header's byte count; float32 solves all three."""
    torch = pytest.importorskip("torch")
    branches = set()
    for tag in ZOO_CASES:
        a, b, d, run, need, need32 = zoo_case(tag, tmp_path)
        ma, mb = (_lib.SphereModel(s["blob"], s["rows"], s["centers"], s["radii"], s["pairs"]) for s in (a, b))
        hx = cross_problem(d, x_ref=a["x"]).energies(a["x"])[1][1]
        assert hx.shape == (ZB, len(a["radii"]), len(b["radii"])) and (hx > 0).mean() > 0.5
        if need > 64 * 1024:
            with pytest.raises(_lib.DexrError, match=rf"libdexr error {UNSUPPORTED}: .*need {need} B of LDS per frame"):
                host_run(ma, mb, run, STEPS32, fixed=a["fixed"])
            branches.add("refused")
            print(f"{tag}: {need} B per frame in float64: refused")
        else:
            res = reference_run(d, STEPS32)
            got = host_run(ma, mb, run, STEPS32, fixed=a["fixed"])
            ok = compare64(tag, got, res, STEPS32, need=1)
            functional(tag, d, got, a["x"], active=~a["unread"])
            branches.add("solved")
            print(f"{tag}: {need} B per frame in float64, {int(ok.sum())} of {ZB} frames clear")
        assert need32 <= 64 * 1024
        g32 = dev_run(ma, mb, torch, run, STEPS32, fixed=a["fixed"])  # float32 solves
        functional(tag + " float32", d, g32, a["x"], active=~a["unread"])
        assert (g32[2][:, 3] > 0).all()
    assert branches == {"solved", "refused"}


# ---- 7. argument errors through the raw ABI ------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    ma, mb = models("allegro_right_left")
    sub = _opt_case("subset", 311)
    msub = sub[0].sphere_model(sub[2])  # a table that reads fixed columns
    assert msub.n_fixed == 6
    n = 4
    x, xb = (torch.zeros((n, m.n_in), dtype=torch.float32, device="cuda") for m in (ma, mb))
    lim = torch.zeros((ma.n_in,), dtype=torch.float32, device="cuda")
    out, en = _nan(torch, (n, ma.n_in)), _nan(torch, (n, 4))
    it, st = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    good = dict(m=ma.handle, B=n, x0=x.data_ptr(), fixed=None, x_ref=None, u=None, n_target=0, tp=None, tr=None, wl=None, wa=None, margin=0.01, wcol=1.0,
                pw=None, lo=lim.data_ptr(), hi=lim.data_ptr(), damping=1e-4, max_step=0.2, tol=0.0, max_iters=4, other=mb.handle, x_b=xb.data_ptr(),
                fixed_b=None, opos=None, orot=None, margin_x=0.01, w_x=1.0, xw=None, x_out=out.data_ptr(), iters=it.data_ptr(), energy=en.data_ptr(),
                status=st.data_ptr())

    def invalid(word, B=n, **over):
        for b_ in (B, 0) if over.get("zero", True) else (B,):
            a = dict(good, B=b_, **{k: v for k, v in over.items() if k != "zero"})
            rc = lib.dexr_sphere_resolve_cross_dev(*[a[k] for k in good], None)
            msg = lib.dexr_last_error()
            assert rc == INVALID and word in msg, (rc, msg, over, b_)

    # the rules checked at B == 0 too: the models and the scalars
    invalid(b"null sphere model", m=None)
    invalid(b"null sphere model of the other robot", other=None)
    for bad in (-1e-6, float("nan"), float("inf")):
        invalid(b"margin_x", margin_x=bad)
        invalid(b"w_x", w_x=bad)
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
    for bad in (-1, 65):
        invalid(b"n_target", n_target=bad)
    # the rules of a batch that has frames
    invalid(b"negative", B=-1, zero=False)
    invalid(b"n_target is 0", tp=x.data_ptr(), zero=False)
    invalid(b"both NULL", n_target=2, zero=False)
    invalid(b"x_out is NULL", x_out=None, zero=False)
    invalid(b"x0 is NULL", x0=None, zero=False)
    invalid(b"x_b is NULL", x_b=None, zero=False)
    invalid(b"fixed_b must not be NULL", other=msub.handle, zero=False)
    # the host twin keeps the same rules
    z, zb = np.zeros((n, ma.n_in)), np.zeros((n, mb.n_in))
    zo, ze, zi, zs = np.full((n, ma.n_in), np.nan), np.full((n, 4), np.nan), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))  # noqa: E731
    hgood = dict(good, x0=dp(z), lo=None, hi=None, x_b=dp(zb), x_out=dp(zo), iters=ip(zi), energy=dp(ze), status=ip(zs))
    for word, over in ((b"null sphere model", dict(m=None)), (b"of the other robot", dict(other=None)), (b"margin_x", dict(margin_x=-1.0)),
                       (b"w_x", dict(w_x=float("nan"))), (b"negative", dict(B=-2)), (b"margin", dict(margin=-1.0)), (b"damping", dict(damping=float("nan"))),
                       (b"max_iters", dict(max_iters=0)), (b"lo and hi", dict(lo=dp(z[0].copy()))), (b"n_target", dict(n_target=99)),
                       (b"x_out is NULL", dict(x_out=None)), (b"x0 is NULL", dict(x0=None)), (b"x_b is NULL", dict(x_b=None)),
                       (b"fixed_b must not be NULL", dict(other=msub.handle, x_b=dp(np.zeros((n, msub.n_in)))))):
        a = dict(hgood, **over)
        rc = lib.dexr_sphere_resolve_cross(*[a[k] for k in hgood])
        assert rc == INVALID and word in lib.dexr_last_error(), (word, rc, lib.dexr_last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(en).all()) and bool((it == -7).all()) and bool((st == -7).all())
    assert np.isnan(zo).all() and np.isnan(ze).all() and (zi == -7).all() and (zs == -7).all()  # nothing was launched


# ---- 8. the torch fronts ------------------------------------------------------------------------------------------------------------------
def test_torch_fronts_equal_the_entry_points_bitwise(require_gpu):
    torch = pytest.importorskip("torch")
    opt, prob, sset, pairs, d0, fx = _opt_case("teleop/allegro_hand_right.yml", 341)
    opb, prb, ssb, pairs_b, db, fb = _opt_case("subset", 342)  # B has six fixed joints
    assert fx is None and fb is not None
    n, k = B, 6
    ca = cref.centres(prob.robot, d0["full"](d0["q"]), d0["links"], d0["rows"], d0["centers"])[0]
    cb = cref.centres(prb.robot, db["full"](db["q"]), db["links"], db["rows"], db["centers"])[0]
    pa, ra, pb, rb = place(ca, cb, 7, n, 0.02, 0.08)  # (3 cm spheres here)
    q, qb, fbt = _dev(torch, d0["q"]), _dev(torch, db["q"]), _dev(torch, fb)
    pat, rat, pbt, rbt = (_dev(torch, a) for a in (pa, ra, pb, rb))
    xw = _dev(torch, np.random.default_rng(343).uniform(0.5, 2, (sset.n_sphere, ssb.n_sphere)))
    pw = _dev(torch, np.random.default_rng(344).uniform(0.5, 2.0, len(pairs)))
    lim = _dev(torch, np.stack([d0["lo"], d0["hi"]], 1))
    limb = _dev(torch, np.stack([db["lo"], db["hi"]], 1))
    qref = _dev(torch, _r32(d0["q"] + 0.01))
    tips = ["link_15.0_tip", "link_3.0_tip"]
    tp, trot = isr.link_poses(prob.robot, d0["full"](_r32(d0["q"] + 0.05)), tips)
    tpt, trt = _dev(torch, tp), _dev(torch, trot)
    wt = _dev(torch, np.random.default_rng(345).uniform(0.5, 2, (n, 2)))
    op, orot = collision.relative_pose(pat, rat, pbt, rbt)
    want_r = np.einsum("bji,bjk->bik", ra, rb)
    assert np.abs(orot.cpu().numpy() - want_r).max() < 1e-6 and np.abs(op.cpu().numpy() - np.einsum("bji,bj->bi", ra, pb - pa)).max() < 1e-6

    def fresh(width):
        return (_nan(torch, (n, width)), torch.full((n,), -7, dtype=torch.int32, device="cuda"), _nan(torch, (n, 4)),
                torch.full((n,), -7, dtype=torch.int32, device="cuda"))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = side.cuda_stream
        ma, mb = opt.sphere_model(sset), opb.sphere_model(ssb)
        lo, hi = lim[:, 0].contiguous(), lim[:, 1].contiguous()
        # the defaults: cross_margin is margin, w_x 1, no weights
        got = collision.resolve_cross_collisions(opt, q, sset, opb, qb, ssb, 0.01, other_pos=op, other_rot=orot, damping=1e-4, max_iters=k,
                                                 posture_weight=1e-3, limits=lim, max_step=0.2, fixed_qpos_b=fbt)
        u = torch.full((q.shape[1],), 1e-3, dtype=torch.float32, device="cuda")
        wx_, wi, we, ws = fresh(q.shape[1])
        ma.resolve_cross_dev(mb, n, q.data_ptr(), 0, qb.data_ptr(), fbt.data_ptr(), 0.01, 1e-4, k, wx_.data_ptr(), wi.data_ptr(), we.data_ptr(), ws.data_ptr(),
                             posture_weight_ptr=u.data_ptr(), lo_ptr=lo.data_ptr(), hi_ptr=hi.data_ptr(), max_step=0.2, other_pos_ptr=op.data_ptr(),
                             other_rot_ptr=orot.data_ptr(), stream=sp)
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, (wx_, wi, we, ws))) and not got[0].requires_grad
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].shape == (n, 4) and got[3].dtype == torch.int32
        assert bool((we[:, 3] > 0).any()) and bool(torch.isfinite(wx_).all())
        # everything at once, the cross arguments positionally, with targets: a model keyed by the target links; a non-contiguous q
        qn = torch.stack([q, q], 2)[:, :, 0]
        assert not qn.is_contiguous()
        got = collision.resolve_cross_collisions(opt, qn, sset, opb, qb, ssb, 0.01, 0.02, op, orot, xw, pw, 0.75, 1e-4, k, u, qref, 2.0, tips, tpt, trt,
                                                 wt, wt, 1e-7, 0.2, lim, None, fbt)
        tm = opt.sphere_model(sset, pairs, tips)
        assert tm is not ma
        wx_, wi, we, ws = fresh(q.shape[1])
        tm.resolve_cross_dev(mb, n, q.data_ptr(), 0, qb.data_ptr(), fbt.data_ptr(), 0.01, 1e-4, k, wx_.data_ptr(), wi.data_ptr(), we.data_ptr(), ws.data_ptr(),
                             x_ref_ptr=qref.data_ptr(), posture_weight_ptr=u.data_ptr(), n_target=2, target_pos_ptr=tpt.data_ptr(),
                             target_rot_ptr=trt.data_ptr(), pos_weight_ptr=wt.data_ptr(), rot_weight_ptr=wt.data_ptr(), collision_weight=2.0,
                             pair_weight_ptr=pw.data_ptr(), lo_ptr=lo.data_ptr(), hi_ptr=hi.data_ptr(), tol=1e-7, max_step=0.2, other_pos_ptr=op.data_ptr(),
                             other_rot_ptr=orot.data_ptr(), cross_margin=0.02, cross_weight=0.75, cross_pair_weight_ptr=xw.data_ptr(), stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(got, (wx_, wi, we, ws))) and bool((we[:, 0] > 0).all()) and bool((we[:, 3] > 0).any())
        # the robot twin over the full qpos, B with no pose: the two hands share a root frame
        robot = opt.robot
        rl = robot.joint_limits
        qr = _dev(torch, np.random.default_rng(346).uniform(rl[:, 0], rl[:, 1], (n, robot.dof)))
        qr2 = _dev(torch, np.random.default_rng(347).uniform(rl[:, 0], rl[:, 1], (n, robot.dof)))
        gr = collision.robot_resolve_cross_collisions(robot, qr, sset, robot, qr2, sset, 0.01, damping=1e-4, max_iters=k, posture_weight=1e-3)
        rm = robot.sphere_model(sset, pairs)
        ur = torch.full((robot.dof,), 1e-3, dtype=torch.float32, device="cuda")
        rx, ri, re_, rs = fresh(robot.dof)
        rm.resolve_cross_dev(rm, n, qr.data_ptr(), 0, qr2.data_ptr(), 0, 0.01, 1e-4, k, rx.data_ptr(), ri.data_ptr(), re_.data_ptr(), rs.data_ptr(),
                             posture_weight_ptr=ur.data_ptr(), stream=sp)
        assert all(torch.equal(a, b) for a, b in zip(gr, (rx, ri, re_, rs))) and bool((re_[:, 3] > 0).all())
        # the alternating front, one sweep: its two explicit calls
        args_a, args_b = dict(limits=lim, posture_weight=1e-3, max_step=0.2, pair_weight=pw), dict(limits=limb, posture_weight=1e-3, max_step=0.2)
        both = collision.resolve_bimanual_collisions(opt, q, sset, opb, qb, ssb, 0.01, pat, rat, pbt, rbt, sweeps=1, cross_margin=0.02, cross_weight=xw,
                                                     w_x=0.75, damping=1e-4, max_iters=k, args_a=args_a, args_b=args_b, fixed_qpos_b=fbt)
        one = collision.resolve_cross_collisions(opt, q, sset, opb, qb, ssb, 0.01, 0.02, op, orot, xw, w_x=0.75, damping=1e-4, max_iters=k, q_ref=q,
                                                 fixed_qpos_b=fbt, **args_a)
        ip_, ir_ = collision.relative_pose(pbt, rbt, pat, rat)
        two = collision.resolve_cross_collisions(opb, qb, ssb, opt, one[0], sset, 0.01, 0.02, ip_, ir_, xw.t().contiguous(), w_x=0.75, damping=1e-4,
                                                 max_iters=k, q_ref=qb, fixed_qpos_a=fbt, **args_b)
        assert all(torch.equal(a, b) for a, b in zip(both[0], one)) and all(torch.equal(a, b) for a, b in zip(both[1], two))
        assert bool((both[0][2][:, 3] > 0).any()) and bool((both[1][1] >= 1).all())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    e = torch.zeros((0, opt.opt_dof), device="cuda")
    out = collision.resolve_cross_collisions(opt, e, sset, opb, qb[:0], ssb, 0.01, damping=1e-4, max_iters=k, fixed_qpos_b=fbt[:0])
    assert out[0].shape == (0, opt.opt_dof) and out[1].shape == (0,) and out[2].shape == (0, 4) and out[3].shape == (0,)


def test_bimanual_sweeps_do_not_raise_the_joint_energy(require_gpu):
    """Shadow right against Shadow left, both free, three sweeps: the joint energy -- each robot's own three terms and the cross term
    ONCE, recomputed by the yardsticks in float64 -- after each sweep is at most that before it times (1 + RISE); sweeps = 3 is three
    chained sweeps of one, bit for bit."""
    torch = pytest.importorskip("torch")
    opa, pra, ssa, pairs_a, da, fa = _opt_case("teleop/shadow_hand_right.yml", 351)
    opb, prb, ssb, pairs_b, db, fb = _opt_case("teleop/shadow_hand_left.yml", 352)
    assert fa is None and fb is None  # every joint of a Shadow hand is a variable
    n, k, xm, wx = B, 8, 0.01, 1.5
    ca = cref.centres(pra.robot, da["full"](da["q"]), da["links"], da["rows"], da["centers"])[0]
    cb = cref.centres(prb.robot, db["full"](db["q"]), db["links"], db["rows"], db["centers"])[0]
    pa, ra, pb, rb = place(ca, cb, 9, n, 0.02, 0.08)
    qa, qb = _dev(torch, da["q"]), _dev(torch, db["q"])
    pat, rat, pbt, rbt = (_dev(torch, a) for a in (pa, ra, pb, rb))
    lima, limb = _dev(torch, np.stack([da["lo"], da["hi"]], 1)), _dev(torch, np.stack([db["lo"], db["hi"]], 1))
    xw = _r32(np.random.default_rng(353).uniform(0.5, 2, (ssa.n_sphere, ssb.n_sphere)))
    kw = dict(cross_margin=xm, cross_weight=_dev(torch, xw), w_x=wx, damping=1e-4, max_iters=k)
    args_a, args_b = dict(limits=lima, posture_weight=1e-3, max_step=0.2, q_ref=qa), dict(limits=limb, posture_weight=1e-3, max_step=0.2, q_ref=qb)

    opos, orot = np.einsum("bji,bj->bi", ra, pb - pa), np.einsum("bji,bjk->bik", ra, rb)  # B in A's root frame, float64
    other = lambda x_b: rxr.Other(prb.robot, db["full"](x_b), db["links"], db["rows"], db["centers"], db["radii"], opos, orot)  # noqa: E731

    def joint_energy(xa, xb):
        xa, xb = xa.cpu().numpy().astype(np.float64), xb.cpu().numpy().astype(np.float64)
        PA = rxr.Problem(pra.robot, da["links"], 0, da["rows"], da["centers"], da["radii"], da["pairs"], da["margin"], other(xb), cross_margin=xm, w_x=wx,
                         cross_weight=xw, x_ref=da["q"], posture_weight=np.full(xa.shape[1], 1e-3), full=da["full"], fold=da["fold"])
        PB = rr.Problem(prb.robot, db["links"], 0, db["rows"], db["centers"], db["radii"], db["pairs"], db["margin"], x_ref=db["q"],
                        posture_weight=np.full(xb.shape[1], 1e-3), full=db["full"], fold=db["fold"])
        return PA.energies(xa)[0].sum(1) + PB.energies(xb)[0].sum(1)

    E = [joint_energy(qa, qb)]
    xa, xb = qa, qb
    for _ in range(3):
        ra_, rb_ = collision.resolve_bimanual_collisions(opa, xa, ssa, opb, xb, ssb, 0.01, pat, rat, pbt, rbt, sweeps=1, args_a=args_a, args_b=args_b, **kw)
        xa, xb = ra_[0], rb_[0]
        E.append(joint_energy(xa, xb))
    E = np.stack(E)
    print(f"bimanual Shadow right / left: joint energy per sweep (medians) {np.median(E, 1)}; max of E_after / E_before - 1 = "
          f"{float((E[1:] / E[:-1] - 1).max()):.3e} (gate {RISE:g})")
    assert (E[0] > 0).all() and (E[1:] <= E[:-1] * (1 + RISE)).all() and (E[-1] < E[0]).any()
    r3a, r3b = collision.resolve_bimanual_collisions(opa, qa, ssa, opb, qb, ssb, 0.01, pat, rat, pbt, rbt, sweeps=3, args_a=args_a, args_b=args_b, **kw)
    assert torch.equal(r3a[0], xa) and torch.equal(r3b[0], xb) and torch.equal(r3b[2], rb_[2])

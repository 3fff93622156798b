"""GPU tests of the collision between two posed robots (csrc/dexr_cross.hpp, include/dexr_cross.h): the float64 host entry points
and the float32 device entry points against tests/cross_reference.py in all three forms, optimizer order, the limits of the tables,
the bit-for-bit properties, the invariants of a pair of bodies, coincident spheres, isolation, the pair weights, the raw ABI's
argument errors, the torch front and autograd.

INPUTS.  The six pairs of tests/test_cross_host.py (cross_inputs: the "offset" sphere sets, B = 33: two blocks and a ragged tail, a
seeded pose per robot and frame), whose references and conditions are proven there on the CPU and shared from there.  Every other
case is built by build_case, which runs test_cross_host.make_case and asserts its conditions on its own float64 reference before a
GPU sees it.

GATES.  float64: 1e-9 absolute on every output (GATE64 of the sphere family).  float32: max |out32 - reference64| of an output may
be 8 x the distance between the reference's OWN float32 and float64 runs on that output (GATE32); where that distance is zero the
output must be exact zeros.  `nearest` is compared on clear entries (test_cross_host.clear_entries) and the cotangent of every VJP
is zero elsewhere.  The ratios are printed; those of the MI355X are in docs/experiments/cross_collision.md."""
import functools
import os

import numpy as np
import pytest

import collision_reference as cref
import cross_reference as xref
import pose_zoo as zoo
import test_gpu_link_poses as glp
from dex_retargeting_amd import _lib, collision
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_collision_host import B, MARGIN
from test_cross_host import FAR, FLOATS, PAIRS, conditions, cross_inputs, make_case, place, reference, side_inputs, sides, wrapper_of
from test_gpu_link_jacobians import _fold4, _opt_inputs, _optimizer_and_problem
from test_obstacle_host import _rotations

pytestmark = pytest.mark.gpu
GATE64, GATE32 = 1e-9, 8.0
INTS = ("nearest_a", "nearest_b")
OUTPUTS = FLOATS + INTS
PENALTY = ("E", "grad_a", "grad_b", "wrench_a", "wrench_b")


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _dev(torch, a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _nan(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _np(t):
    return None if t is None else t.cpu().numpy()


class Call:
    """one set of inputs of the two models: x_a, x_b (what the tables read), fixed_a, fixed_b, the four poses, as numpy float64."""

    def __init__(self, ma, mb, x_a, x_b, fixed_a=None, fixed_b=None, pos_a=None, rot_a=None, pos_b=None, rot_b=None):
        self.ma, self.mb, self.x_a, self.x_b, self.fixed_a, self.fixed_b = ma, mb, x_a, x_b, fixed_a, fixed_b
        self.poses = dict(pos_a=pos_a, rot_a=rot_a, pos_b=pos_b, rot_b=rot_b)

    def rows(self, idx):
        cut = lambda a: None if a is None else np.ascontiguousarray(a[idx])  # noqa: E731
        return Call(self.ma, self.mb, cut(self.x_a), cut(self.x_b), cut(self.fixed_a), cut(self.fixed_b), **{k: cut(v) for k, v in self.poses.items()})

    def swapped(self):
        p = self.poses
        return Call(self.mb, self.ma, self.x_b, self.x_a, self.fixed_b, self.fixed_a, p["pos_b"], p["rot_b"], p["pos_a"], p["rot_a"])

    # ---- float32 device entry points, the outputs pre-filled with NaN (nearest: -1) ----
    def _dev_inputs(self, torch):
        t = [_dev(torch, a) for a in (self.x_a, self.fixed_a, self.x_b, self.fixed_b)]
        p = {k: _dev(torch, v) for k, v in self.poses.items()}
        return t, p, [_ptr(a) for a in t], {f"{k}_ptr": _ptr(v) for k, v in p.items()}

    def dev_distances(self, torch, want=(True,) * 4):
        keep, keep_p, head, poses = self._dev_inputs(torch)
        n, Sa, Sb = len(self.x_a), self.ma.n_sphere, self.mb.n_sphere
        da, db = (_nan(torch, (n, S)) if k else None for S, k in ((Sa, want[0]), (Sb, want[2])))
        na, nb = (torch.full((n, S), -1, dtype=torch.int32, device="cuda") if k else None for S, k in ((Sa, want[1]), (Sb, want[3])))
        self.ma.cross_distances_dev(self.mb, n, *head, _ptr(da), _ptr(na), _ptr(db), _ptr(nb), **poses, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dict(dist_a=_np(da), nearest_a=_np(na), dist_b=_np(db), nearest_b=_np(nb))

    def dev_vjp(self, torch, ga, gb, wrench=True):
        keep, keep_p, head, poses = self._dev_inputs(torch)
        n = len(self.x_a)
        g = [_dev(torch, ga), _dev(torch, gb)]
        gxa, gxb = _nan(torch, (n, self.ma.n_in)), _nan(torch, (n, self.mb.n_in))
        wa, wb = (_nan(torch, (n, 6)) if wrench else None for _ in range(2))
        self.ma.cross_distances_vjp_dev(self.mb, n, *head, _ptr(g[0]), _ptr(g[1]), _ptr(gxa), _ptr(gxb), _ptr(wa), _ptr(wb), **poses,
                                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dict(vjp_a=_np(gxa), vjp_b=_np(gxb), vjp_wa=_np(wa), vjp_wb=_np(wb))

    def dev_penalty(self, torch, margin, w=None, want=(True,) * 5):
        keep, keep_p, head, poses = self._dev_inputs(torch)
        n = len(self.x_a)
        wd = _dev(torch, w)
        shapes = ((n,), (n, self.ma.n_in), (n, self.mb.n_in), (n, 6), (n, 6))
        out = [_nan(torch, s) if k else None for s, k in zip(shapes, want)]
        self.ma.cross_penalty_dev(self.mb, n, *head, margin, _ptr(wd), *[_ptr(o) for o in out], **poses, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dict(zip(PENALTY, (_np(o) for o in out)))

    def dev_all(self, torch, ga, gb, margin, w=None):
        return {**self.dev_distances(torch), **self.dev_vjp(torch, ga, gb), **self.dev_penalty(torch, margin, w)}

    # ---- float64 host entry points ----
    def _host(self):
        return dict(fixed_a=self.fixed_a, fixed_b=self.fixed_b, **self.poses)

    def host_all(self, ga, gb, margin, w=None):
        da, na, db, nb = self.ma.cross_distances(self.mb, self.x_a, self.x_b, **self._host())
        va, vb, vwa, vwb = self.ma.cross_distances_vjp(self.mb, self.x_a, self.x_b, ga, gb, **self._host())
        out = dict(dist_a=da, nearest_a=na, dist_b=db, nearest_b=nb, vjp_a=va, vjp_b=vb, vjp_wa=vwa, vjp_wb=vwb)
        out.update(zip(PENALTY, self.ma.cross_penalty(self.mb, self.x_a, self.x_b, margin, w, **self._host())))
        return out


def _compare_nearest(tag, got, want, case):
    for k, clear, n_oth in (("nearest_a", case["clear_a"], want["d"].shape[2]), ("nearest_b", case["clear_b"], want["d"].shape[1])):
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (tag, k)
        assert (got[k] >= 0).all() and (got[k] < n_oth).all(), (tag, k)
        assert np.array_equal(got[k][clear], want[k][clear]), (tag, k)


def compare64(tag, got, case):
    want = case["r64"]
    for k in FLOATS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float64, (tag, k)
        e = float(np.abs(got[k] - want[k]).max())
        print(f"{tag}: float64 max |{k} - reference| = {e:.3e} (gate {GATE64:.0e})")
        assert np.isfinite(got[k]).all() and e <= GATE64, (tag, k, e)
    _compare_nearest(tag, got, want, case)


def compare32(tag, got, case):
    """the gate of each output comes from the reference's own two runs, never from the code under test"""
    want64, want32 = case["r64"], case["r32"]
    for k in FLOATS:
        assert got[k].shape == want64[k].shape and got[k].dtype == np.float32, (tag, k)
        dist = float(np.abs(want32[k].astype(np.float64) - want64[k]).max())
        e = float(np.abs(got[k].astype(np.float64) - want64[k]).max())
        ratio = e / dist if dist > 0 else (0.0 if e == 0 else float("inf"))
        print(f"{tag}: float32 max |{k} - reference64| = {e:.3e}, the reference's float32 run is {dist:.3e} from its float64 run "
              f"(error / reference distance {ratio:.2f}, gate {GATE32:g})")
        assert np.isfinite(got[k]).all(), (tag, k)
        if dist == 0:
            assert not got[k].any(), (tag, k, "exact zeros expected")
        assert ratio <= GATE32, (tag, k, e, dist)
    _compare_nearest(tag, got, want64, case)


def pair_models(case):
    na, nb = PAIRS[case]
    ma = wrapper_of(na).sphere_model(side_inputs(na)["sset"])
    mb = ma if nb == na else wrapper_of(nb).sphere_model(side_inputs(nb)["sset"])
    return ma, mb


def pair_call(case):
    d = cross_inputs(case)
    ma, mb = pair_models(case)
    return d, Call(ma, mb, d["q_a"], d["q_b"], None, None, d["pos_a"], d["rot_a"], d["pos_b"], d["rot_b"])


# ---- 1. the six pairs: float64 host and float32 device, all three forms ---------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(PAIRS))
def test_host_float64_and_device_float32_against_the_reference(case, require_gpu):
    torch = pytest.importorskip("torch")
    assert len(PAIRS) == 6
    d, call = pair_call(case)
    ref = reference(case)
    ma, mb = call.ma, call.mb
    assert (ma.n_in, ma.n_sphere, mb.n_in, mb.n_sphere) == (d["a"]["orc"].dof, len(d["a"]["radii"]), d["b"]["orc"].dof, len(d["b"]["radii"]))
    assert (ma is mb) == (case == "leap_same")
    h64 = call.host_all(ref["ga"], ref["gb"], d["margin"], d["w"])
    compare64(case, h64, ref)
    d32 = call.dev_all(torch, ref["ga"], ref["gb"], d["margin"], d["w"])
    compare32(case, d32, ref)
    for out in (h64, d32):  # far apart: exact zeros
        assert all(not out[k][FAR].any() for k in PENALTY) and (out["dist_a"][FAR] > 5).all() and (out["E"] > 0).any()


# ---- 2. optimizer order: a fixed_qpos subset on one side, mimic joints on the other ---------------------------------------------------
ORDER_SEED = 0  # the first of the seeds 0, 1, 2, ... with which the conditions hold


def _order_side(rel, seed):
    opt, prob = _optimizer_and_problem(rel)
    links = [f.name for f in opt.robot.kin.frames]
    rows, cen, rad = np.arange(len(links)), np.zeros((len(links), 3)), np.full(len(links), 0.012)
    sset = collision.SphereSet(links, cen, rad)
    x, fixed = (_r32(a) for a in _opt_inputs(prob, B, seed))
    side = dict(orc=prob.robot, links=links, rows=rows, centers=cen, radii=rad, sset=sset)
    return opt, prob, side, x, fixed


def build_case(side_a, side_b, q_a, q_b, seed, n, margin=MARGIN, fold_a=None, fold_b=None, far=None):
    """inputs dict (as test_cross_host.cross_inputs) with seeded poses, weights and cotangents, and its references; the conditions
    of test_cross_host asserted."""
    ca = cref.centres(side_a["orc"], q_a, side_a["links"], side_a["rows"], side_a["centers"])[0]
    cb = cref.centres(side_b["orc"], q_b, side_b["links"], side_b["rows"], side_b["centers"])[0]
    pos_a, rot_a, pos_b, rot_b = place(ca, cb, seed, n)
    if far is not None:
        pos_b = pos_b.copy()
        pos_b[far] += np.array([10.0, -10.0, 10.0])
    rng = np.random.default_rng(seed + 1000)
    Sa, Sb = len(side_a["radii"]), len(side_b["radii"])
    d = dict(a=side_a, b=side_b, q_a=q_a, q_b=q_b, pos_a=pos_a, rot_a=rot_a, pos_b=_r32(pos_b), rot_b=rot_b, margin=margin,
             w=_r32(rng.uniform(0.5, 2.0, (Sa, Sb))), ga=_r32(rng.standard_normal((n, Sa))), gb=_r32(rng.standard_normal((n, Sb))))
    case = make_case(d, fold_a, fold_b)
    failed = conditions(d, case["r64"], case["clear_a"], case["clear_b"])
    assert failed is None, failed
    return d, case


@functools.lru_cache(maxsize=None)
def order_case():
    opt_a, prob_a, side_a, x_a, fixed_a = _order_side("subset", 231)
    opt_b, prob_b, side_b, x_b, fixed_b = _order_side("teleop/inspire_hand_right_dexpilot.yml", 232)
    assert fixed_a.shape[1] == 6 and len(prob_b.idx_pin2mimic) > 0 and fixed_b.shape[1] == 0
    d, case = build_case(side_a, side_b, prob_a.full_qpos(x_a, fixed_a), prob_b.full_qpos(x_b, fixed_b), ORDER_SEED, B,
                         fold_a=lambda J: _fold4(prob_a, J), fold_b=lambda J: _fold4(prob_b, J), far=FAR)
    return opt_a, opt_b, side_a, side_b, x_a, fixed_a, x_b, d, case


def test_optimizer_order_folds_mimic_and_fixed_joints(require_gpu):
    torch = pytest.importorskip("torch")
    opt_a, opt_b, side_a, side_b, x_a, fixed_a, x_b, d, case = order_case()
    ma, mb = opt_a.sphere_model(side_a["sset"]), opt_b.sphere_model(side_b["sset"])
    assert (ma.n_in, ma.n_fixed, mb.n_in, mb.n_fixed) == (opt_a.opt_dof, 6, opt_b.opt_dof, 0)
    call = Call(ma, mb, x_a, x_b, fixed_a, None, d["pos_a"], d["rot_a"], d["pos_b"], d["rot_b"])
    h64 = call.host_all(case["ga"], case["gb"], MARGIN, d["w"])
    compare64("subset against mimic", h64, case)
    d32 = call.dev_all(torch, case["ga"], case["gb"], MARGIN, d["w"])
    compare32("subset against mimic", d32, case)
    assert np.abs(case["r64"]["grad_a"]).max() > 0 and np.abs(case["r64"]["grad_b"]).max() > 0
    moved = Call(ma, mb, x_a, x_b, fixed_a + 0.05, None, **call.poses).host_all(case["ga"], case["gb"], MARGIN, d["w"])
    assert np.abs(moved["dist_a"] - h64["dist_a"]).max() > 1e-4  # fixed joints move the geometry
    # the torch front is the same launch, and so is the other order of the two robots
    qa, fa, qb, pa, ra, pb, rb, w = (_dev(torch, a) for a in (x_a, fixed_a, x_b, d["pos_a"], d["rot_a"], d["pos_b"], d["rot_b"], d["w"]))
    out = collision.cross_penalty(opt_a, qa, side_a["sset"], opt_b, qb, side_b["sset"], MARGIN, pa, ra, pb, rb, w, fa, wrench=True)
    assert all(np.array_equal(_np(o), d32[k]) for o, k in zip(out, PENALTY))
    out3 = collision.cross_penalty(opt_a, qa, side_a["sset"], opt_b, qb, side_b["sset"], MARGIN, pa, ra, pb, rb, w, fa)
    assert len(out3) == 3 and all(torch.equal(u, v) for u, v in zip(out3, out))
    dn = collision.cross_distances(opt_a, qa, side_a["sset"], opt_b, qb, side_b["sset"], pa, ra, pb, rb, fa, nearest=True)
    assert all(np.array_equal(_np(o), d32[k]) for o, k in zip(dn, ("dist_a", "nearest_a", "dist_b", "nearest_b"))) and dn[1].dtype == torch.int32
    dd = collision.cross_distances(opt_a, qa, side_a["sset"], opt_b, qb, side_b["sset"], pa, ra, pb, rb, fa)
    assert len(dd) == 2 and torch.equal(dd[0], dn[0]) and torch.equal(dd[1], dn[2])
    sw = collision.cross_distances(opt_b, qb, side_b["sset"], opt_a, qa, side_a["sset"], pb, rb, pa, ra, fixed_qpos_b=fa)
    assert torch.equal(sw[0], dd[1]) and torch.equal(sw[1], dd[0])


# ---- 3. the limits, on the synthetic robots of tests/pose_zoo.py ----------------------------------------------------------------------
# A sphere model holds at least one pair of two different spheres (dexr_sphere_model_create), so the smallest side is TWO spheres:
# "2 against 128" and "17 against 2" stand where one sphere was meant.
ZR, ZMARGIN = 0.010, 0.020
LIMITS = {"2 against 128": (2, 128, 9, 0), "128 against 128": (128, 128, 5, 0), "17 against 2": (17, 2, 9, 0), "B = 1": (128, 17, 1, 0)}
# (spheres of A, of B, frames, the first of the seeds 0, 1, 2, ... with which the conditions hold)


def _zoo_side(m, S, seed):
    """S spheres on the 64 links of a zoo member: two per link for S = 128 (one at the origin, one 5 .. 15 mm off it), else one off
    the origin of each of S seeded links."""
    L = len(m.links)
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((L, 3))
    off = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.005, 0.015, (L, 1))
    if S == 2 * L:
        rows, centers = np.repeat(np.arange(L), 2), np.stack([np.zeros((L, 3)), off], 1).reshape(2 * L, 3)
    else:
        rows = rng.permutation(L)[:S]
        centers = off[rows]
    return dict(orc=m.orc, links=m.links, rows=rows, centers=_r32(centers), radii=np.full(S, ZR))


def limit_case(which, directory, seed=None):
    Sa, Sb, n, case_seed = LIMITS[which]
    m = zoo.build("binary64_slots8", directory)
    side_a, side_b = _zoo_side(m, Sa, 301), _zoo_side(m, Sb, 302)
    x_a, fixed_a, _ = zoo.inputs(m, n, 2051)
    x_b, fixed_b, _ = zoo.inputs(m, n, 2052)
    fold = lambda J: zoo.fold(m.smap, J)  # noqa: E731
    d, case = build_case(side_a, side_b, zoo.full_q(m.smap, x_a, fixed_a), zoo.full_q(m.smap, x_b, fixed_b), case_seed if seed is None else seed, n,
                         ZMARGIN, fold, fold)
    return m, side_a, side_b, x_a, fixed_a, x_b, fixed_b, d, case


@pytest.mark.parametrize("which", sorted(LIMITS))
def test_limits_of_the_tables(which, tmp_path, require_gpu):
    torch = pytest.importorskip("torch")
    Sa, Sb, n, _ = LIMITS[which]
    m, side_a, side_b, x_a, fixed_a, x_b, fixed_b, d, case = limit_case(which, tmp_path)
    ma = _lib.SphereModel(m.blob, side_a["rows"], side_a["centers"], side_a["radii"], [(0, 1)])  # (the pair list plays no part)
    mb = _lib.SphereModel(m.blob, side_b["rows"], side_b["centers"], side_b["radii"], [(0, 1)])
    assert (ma.n_sphere, mb.n_sphere, ma.n_in) == (Sa, Sb, zoo.FACTS["binary64_slots8"]["n_in"]) and (case["r64"]["E"] > 0).any()
    call = Call(ma, mb, x_a, x_b, fixed_a, fixed_b, d["pos_a"], d["rot_a"], d["pos_b"], d["rot_b"])
    h64 = call.host_all(case["ga"], case["gb"], ZMARGIN, d["w"])
    compare64(which, h64, case)
    d32 = call.dev_all(torch, case["ga"], case["gb"], ZMARGIN, d["w"])
    compare32(which, d32, case)
    unread = zoo.abs_mult(m).sum(0) == 0
    for out in (h64, d32):
        assert all(not out[k][:, unread].any() for k in ("grad_a", "grad_b", "vjp_a", "vjp_b"))


# ---- 4. bit for bit ---------------------------------------------------------------------------------------------------------------------
def test_rows_are_independent_and_isolated(require_gpu):
    torch = pytest.importorskip("torch")
    case = "shadow_allegro"
    d, call = pair_call(case)
    ref = reference(case)
    ga, gb, w, margin = ref["ga"], ref["gb"], d["w"], d["margin"]
    full = call.dev_all(torch, ga, gb, margin, w)
    assert all(np.isfinite(full[k]).all() for k in FLOATS) and (full["E"] > 0).any()
    for b in (0, 15, 16, 31, 32):  # a frame alone: B = 1, from both blocks and the ragged tail
        one = call.rows(slice(b, b + 1)).dev_all(torch, ga[b:b + 1], gb[b:b + 1], margin, w)
        for k in OUTPUTS:
            assert np.array_equal(one[k][0], full[k][b]), (b, k)
    perm = np.random.default_rng(6).permutation(B)
    mixed = call.rows(perm).dev_all(torch, ga[perm], gb[perm], margin, w)
    for k in OUTPUTS:
        assert np.array_equal(mixed[k], full[k][perm]), k
    h = call.host_all(ga, gb, margin, w)
    h1 = call.rows(slice(20, 21)).host_all(ga[20:21], gb[20:21], margin, w)
    assert all(np.array_equal(h1[k][0], h[k][20]) for k in OUTPUTS)
    # a NaN in row 7 of x_b, or of pos_a, spoils row 7 alone
    keep = np.arange(B) != 7
    for which in ("x_b", "pos_a"):
        bad = call.rows(slice(None))
        a = (bad.x_b if which == "x_b" else bad.poses["pos_a"]).copy()
        a[7, 1] = np.nan
        if which == "x_b":
            bad.x_b = a
        else:
            bad.poses["pos_a"] = a
        got = bad.dev_all(torch, ga, gb, margin, w)
        # (a distance is a minimum: it stays finite where only some of the other robot's spheres are NaN)
        assert np.isnan(got["E"][7]) and all(np.isnan(got[k][7]).any() for k in ("grad_a", "grad_b", "wrench_a", "wrench_b")), which
        for k in OUTPUTS:
            assert np.array_equal(got[k][keep], full[k][keep]), (which, k)
    # each output requested alone equals the all-outputs call
    for i, k in enumerate(PENALTY):
        one = call.dev_penalty(torch, margin, w, want=tuple(j == i for j in range(5)))
        assert [one[j] is not None for j in PENALTY] == [j == k for j in PENALTY] and np.array_equal(one[k], full[k]), k
    for i, k in enumerate(("dist_a", "nearest_a", "dist_b", "nearest_b")):
        one = call.dev_distances(torch, want=tuple(j == i for j in range(4)))
        assert np.array_equal(one[k], full[k]), k
    nowr = call.dev_vjp(torch, ga, gb, wrench=False)
    assert nowr["vjp_wa"] is None and np.array_equal(nowr["vjp_a"], full["vjp_a"]) and np.array_equal(nowr["vjp_b"], full["vjp_b"])
    one_side = call.dev_vjp(torch, ga, None)  # a NULL cotangent is zeros
    zero = call.dev_vjp(torch, ga, np.zeros_like(gb))
    assert all(np.array_equal(one_side[k], zero[k]) for k in one_side)
    # B = 0: a no-op, NULL pointers and all
    lib, ha, hb = _lib.load(), call.ma.handle, call.mb.handle
    z = (None,) * 8
    assert lib.dexr_cross_distances_dev(ha, hb, 0, *z, None, None, None, None, None) == 0
    assert lib.dexr_cross_distances_vjp_dev(ha, hb, 0, *z, None, None, None, None, None, None, None) == 0
    assert lib.dexr_cross_penalty_dev(ha, hb, 0, *z, 0.01, None, None, None, None, None, None, None) == 0
    assert lib.dexr_cross_penalty(ha, hb, 0, *z, 0.01, None, None, None, None, None, None) == 0
    e0 = call.ma.cross_penalty(call.mb, np.zeros((0, call.ma.n_in)), np.zeros((0, call.mb.n_in)), 0.01)
    assert e0[0].shape == (0,) and e0[2].shape == (0, call.mb.n_in) and e0[4].shape == (0, 6)


def test_a_pose_left_out_is_zeros_and_the_identity(require_gpu):
    torch = pytest.importorskip("torch")
    case = "allegro_right_left"
    d, call = pair_call(case)
    ref = reference(case)
    zeros, eye = np.zeros((B, 3)), np.ascontiguousarray(np.broadcast_to(np.eye(3), (B, 3, 3)))
    for drop in (("pos_a",), ("rot_b",), ("rot_a", "pos_b"), ("pos_a", "rot_a", "pos_b", "rot_b")):
        none, full = call.rows(slice(None)), call.rows(slice(None))
        for k in drop:
            none.poses[k] = None
            full.poses[k] = zeros if k.startswith("pos") else eye
        a, b = none.dev_all(torch, ref["ga"], ref["gb"], d["margin"], d["w"]), full.dev_all(torch, ref["ga"], ref["gb"], d["margin"], d["w"])
        assert all(np.array_equal(a[k], b[k]) for k in OUTPUTS) and np.isfinite(a["E"]).all(), drop
        a, b = none.host_all(ref["ga"], ref["gb"], d["margin"], d["w"]), full.host_all(ref["ga"], ref["gb"], d["margin"], d["w"])
        assert all(np.array_equal(a[k], b[k]) for k in OUTPUTS), drop


def test_swapping_the_two_robots_swaps_the_outputs(require_gpu):
    torch = pytest.importorskip("torch")
    case = "shadow_allegro"
    d, call = pair_call(case)
    ref = reference(case)
    wt = np.ascontiguousarray(d["w"].T)
    for run, gate in ((lambda c, ga, gb, w: c.dev_all(torch, ga, gb, d["margin"], w), None), (lambda c, ga, gb, w: c.host_all(ga, gb, d["margin"], w), GATE64)):
        ab, ba = run(call, ref["ga"], ref["gb"], d["w"]), run(call.swapped(), ref["gb"], ref["ga"], wt)
        for k in ("dist", "nearest"):  # bit for bit
            assert np.array_equal(ab[f"{k}_a"], ba[f"{k}_b"]) and np.array_equal(ab[f"{k}_b"], ba[f"{k}_a"]), k
        if gate is not None:  # E and the gradients: the order of the sums changes
            assert np.abs(ab["E"] - ba["E"]).max() <= gate
            for u, v in (("grad_a", "grad_b"), ("wrench_a", "wrench_b"), ("vjp_a", "vjp_b"), ("vjp_wa", "vjp_wb")):
                assert np.abs(ab[u] - ba[v]).max() <= gate and np.abs(ab[v] - ba[u]).max() <= gate, u


# ---- 5. two bodies: action and reaction, rigid invariance (float64, to GATE64) -----------------------------------------------------------
def test_wrenches_cancel_and_a_common_rigid_motion_changes_nothing(require_gpu):
    case = "shadow_right_left"
    d, call = pair_call(case)
    ref = reference(case)
    out = call.host_all(ref["ga"], ref["gb"], d["margin"], d["w"])
    for wa, wb in ((out["wrench_a"], out["wrench_b"]), (out["vjp_wa"], out["vjp_wb"])):
        assert np.abs(wa[:, :3]).max() > 1e-3 and np.abs(wa[:, :3] + wb[:, :3]).max() <= GATE64
        ta = wa[:, 3:] + np.cross(d["pos_a"], wa[:, :3])
        tb = wb[:, 3:] + np.cross(d["pos_b"], wb[:, :3])
        print(f"max |F_a + F_b| = {np.abs(wa[:, :3] + wb[:, :3]).max():.3e}, max |tau_a + tau_b| about the world origin = {np.abs(ta + tb).max():.3e}")
        assert np.abs(ta + tb).max() <= GATE64
    # one rigid transform (T, R), in float64, on both bases
    rng = np.random.default_rng(9)
    R, T = _rotations(rng, B), rng.uniform(-0.5, 0.5, (B, 3))
    moved = Call(call.ma, call.mb, call.x_a, call.x_b, None, None, T + np.einsum("bij,bj->bi", R, d["pos_a"]), R @ d["rot_a"],
                 T + np.einsum("bij,bj->bi", R, d["pos_b"]), R @ d["rot_b"]).host_all(ref["ga"], ref["gb"], d["margin"], d["w"])
    for k in ("E", "grad_a", "grad_b", "dist_a", "dist_b"):
        e = float(np.abs(moved[k] - out[k]).max())
        print(f"a common rigid motion: max change of {k} = {e:.3e}")
        assert e <= GATE64, k
    assert np.abs(moved["wrench_a"][:, :3] - np.einsum("bij,bj->bi", R, out["wrench_a"][:, :3])).max() <= GATE64


# ---- 6. coincident spheres, pair weights ---------------------------------------------------------------------------------------------------
def test_coincident_spheres_give_energy_and_no_force_and_no_nan(require_gpu):
    torch = pytest.importorskip("torch")
    case = "leap_same"
    d, base = pair_call(case)
    call = Call(base.ma, base.ma, d["q_a"], d["q_a"], None, None, d["pos_a"], d["rot_a"], d["pos_a"], d["rot_a"])  # every sphere on its twin
    dd = dict(d, q_b=d["q_a"], pos_b=d["pos_a"], rot_b=d["rot_a"])
    A, Bs = sides(dd)
    S = len(d["a"]["radii"])
    diag = np.eye(S, dtype=bool)
    F = xref.fields(A, Bs)
    assert not F["s"][:, diag].any() and not F["n"][:, diag].any()
    want = dict(zip(PENALTY, xref.penalty(F, A, Bs, d["margin"], None)[:5]))
    A32, B32 = sides(dd, np.float32)
    want32 = dict(zip(PENALTY, xref.penalty(xref.fields(A32, B32), A32, B32, d["margin"], None)[:5]))
    off = np.where(diag, 0.0, 1.0)  # the same without the coincident pairs: they add energy and no force
    want_off = dict(zip(PENALTY, xref.penalty(F, A, Bs, d["margin"], off)[:5]))
    assert np.abs(want["grad_a"] - want_off["grad_a"]).max() == 0 and (want["E"] - want_off["E"] >= S * (d["margin"] + 0.02) ** 2 - 1e-12).all()
    for out, f32 in ((call.host_all(None, None, d["margin"]), False), (call.dev_all(torch, None, None, d["margin"]), True)):
        assert all(np.isfinite(out[k]).all() for k in FLOATS)
        for k in PENALTY:
            gate = GATE32 * float(np.abs(want32[k].astype(np.float64) - want[k]).max()) if f32 else GATE64
            assert gate > 0 and np.abs(out[k] - want[k]).max() <= gate, (k, f32)
        assert np.abs(out["dist_a"] + 0.02).max() < 1e-8 and np.abs(out["dist_b"] + 0.02).max() < 1e-8
        assert np.array_equal(out["nearest_a"], np.broadcast_to(np.arange(S, dtype=np.int32), (B, S)))
        assert np.array_equal(out["nearest_b"], out["nearest_a"])
    masked = call.host_all(None, None, d["margin"], off)
    full = call.host_all(None, None, d["margin"])
    for k in ("grad_a", "grad_b", "wrench_a", "wrench_b"):  # the coincident pairs add no force
        assert np.array_equal(masked[k], full[k]), k
    assert (full["E"] > masked["E"]).all()


def test_pair_weight_zeros_mask_exactly_those_pairs(require_gpu):
    torch = pytest.importorskip("torch")
    case = "inspire_ability"
    d, call = pair_call(case)
    ref = reference(case)
    active = (ref["r64"]["h"] > 0).any(0)  # (S_a, S_b): pairs active in some frame
    assert active.sum() > 20
    w = d["w"].copy()
    drop = active & (np.random.default_rng(12).uniform(size=active.shape) < 0.5)
    w[drop] = 0.0
    A, Bs = sides(d)
    A32, B32 = sides(d, np.float32)
    F = xref.fields(A, Bs)
    want = dict(zip(PENALTY, xref.penalty(F, A, Bs, d["margin"], w)[:5]))
    want32 = dict(zip(PENALTY, xref.penalty(xref.fields(A32, B32), A32, B32, d["margin"], w)[:5]))
    assert np.abs(want["E"] - ref["r64"]["E"]).max() > 1e-6
    got64 = dict(zip(PENALTY, call.ma.cross_penalty(call.mb, call.x_a, call.x_b, d["margin"], w, **call._host())))
    got32 = call.dev_penalty(torch, d["margin"], w)
    for k in PENALTY:
        assert np.abs(got64[k] - want[k]).max() <= GATE64, k
        gate = GATE32 * float(np.abs(want32[k].astype(np.float64) - want[k]).max())
        assert gate > 0 and np.abs(got32[k].astype(np.float64) - want[k]).max() <= gate, k
    # weights of zero everywhere: exact zeros
    none = call.dev_penalty(torch, d["margin"], np.zeros_like(w))
    assert all(not none[k].any() for k in PENALTY)


# ---- 7. argument errors through the raw ABI -----------------------------------------------------------------------------------------------
def test_raw_abi_argument_errors(require_gpu):
    torch = pytest.importorskip("torch")
    from test_jacobian_host import SUBSET_CFG

    lib = _lib.load()
    ma, mb = pair_models("shadow_allegro")
    n, Sa, Sb = 4, ma.n_sphere, mb.n_sphere
    xa = torch.zeros((n, ma.n_in), dtype=torch.float32, device="cuda")
    xb = torch.zeros((n, mb.n_in), dtype=torch.float32, device="cuda")
    g = torch.ones((n, Sa), dtype=torch.float32, device="cuda")
    da, e, gxa, gxb, wa = _nan(torch, (n, Sa)), _nan(torch, (n,)), _nan(torch, (n, ma.n_in)), _nan(torch, (n, mb.n_in)), _nan(torch, (n, 6))
    ha, hb = ma.handle, mb.handle
    INVALID = -1

    def invalid(rc, word=None):
        assert rc == INVALID
        msg = lib.dexr_last_error()
        assert len(msg) > 0 and (word is None or word in msg), msg

    D, V, P = lib.dexr_cross_distances_dev, lib.dexr_cross_distances_vjp_dev, lib.dexr_cross_penalty_dev
    p = lambda t: t.data_ptr()  # noqa: E731
    z4 = (None,) * 4
    invalid(D(None, hb, n, p(xa), None, p(xb), None, *z4, p(da), None, None, None, None), b"null sphere model")
    invalid(D(ha, None, n, p(xa), None, p(xb), None, *z4, p(da), None, None, None, None), b"null sphere model")
    invalid(D(ha, hb, -1, p(xa), None, p(xb), None, *z4, p(da), None, None, None, None), b"negative")
    invalid(D(ha, hb, n, None, None, p(xb), None, *z4, p(da), None, None, None, None), b"x is NULL")
    invalid(D(ha, hb, n, p(xa), None, None, None, *z4, p(da), None, None, None, None), b"x is NULL")
    invalid(D(ha, hb, n, p(xa), None, p(xb), None, *z4, None, None, None, None, None), b"every output is NULL")
    invalid(V(None, hb, n, p(xa), None, p(xb), None, *z4, p(g), None, p(gxa), p(gxb), None, None, None), b"null sphere model")
    invalid(V(ha, hb, n, p(xa), None, p(xb), None, *z4, p(g), None, None, p(gxb), None, None, None), b"grad_xa_out is NULL")
    invalid(V(ha, hb, n, p(xa), None, p(xb), None, *z4, p(g), None, p(gxa), None, p(wa), None, None), b"grad_xb_out is NULL")
    invalid(V(ha, hb, -2, p(xa), None, p(xb), None, *z4, p(g), None, p(gxa), p(gxb), None, None, None), b"negative")
    invalid(P(ha, None, n, p(xa), None, p(xb), None, *z4, 0.01, None, p(e), None, None, None, None, None), b"null sphere model")
    invalid(P(ha, hb, -3, p(xa), None, p(xb), None, *z4, 0.01, None, p(e), None, None, None, None, None), b"negative")
    invalid(P(ha, hb, n, p(xa), None, p(xb), None, *z4, 0.01, None, None, None, None, None, None, None), b"every output is NULL")
    invalid(P(ha, hb, n, None, None, p(xb), None, *z4, 0.01, None, p(e), None, None, None, None, None), b"x is NULL")
    for bad in (-1e-6, -1.0, float("nan"), float("inf"), -float("inf")):
        invalid(P(ha, hb, n, p(xa), None, p(xb), None, *z4, bad, None, p(e), p(gxa), p(gxb), p(wa), None, None), b"margin")
    # a model that reads fixed columns, on either side
    sub = RetargetingConfig.from_dict(dict(SUBSET_CFG)).build().optimizer
    ms = sub.sphere_model(collision.SphereSet(["link_15.0_tip", "link_3.0_tip"], np.zeros((2, 3)), [0.01, 0.01], [(0, 1)]))
    assert ms.n_fixed == 6 and ms.n_in == 10
    invalid(P(ms.handle, hb, n, p(xa), None, p(xb), None, *z4, 0.01, None, p(e), None, None, None, None, None), b"fixed")
    invalid(D(ha, ms.handle, n, p(xa), None, p(xb), None, *z4, p(da), None, None, None, None), b"fixed")
    # the host twins keep the same rules
    za, zb = np.zeros((n, ma.n_in)), np.zeros((n, mb.n_in))
    zd, ze, zxa, zxb = np.full((n, Sa), np.nan), np.full(n, np.nan), np.full((n, ma.n_in), np.nan), np.full((n, mb.n_in), np.nan)
    dp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))  # noqa: E731
    invalid(lib.dexr_cross_distances(None, hb, n, dp(za), None, dp(zb), None, *z4, dp(zd), None, None, None), b"null sphere model")
    invalid(lib.dexr_cross_distances(ha, hb, -2, dp(za), None, dp(zb), None, *z4, dp(zd), None, None, None), b"negative")
    invalid(lib.dexr_cross_distances(ha, hb, n, dp(za), None, None, None, *z4, dp(zd), None, None, None), b"x is NULL")
    invalid(lib.dexr_cross_distances(ha, hb, n, dp(za), None, dp(zb), None, *z4, None, None, None, None), b"every output is NULL")
    invalid(lib.dexr_cross_distances_vjp(ha, hb, n, dp(za), None, dp(zb), None, *z4, None, None, None, dp(zxb), None, None), b"grad_xa_out is NULL")
    invalid(lib.dexr_cross_distances_vjp(ha, hb, n, dp(za), None, dp(zb), None, *z4, None, None, dp(zxa), None, None, None), b"grad_xb_out is NULL")
    invalid(lib.dexr_cross_penalty(ha, hb, n, dp(za), None, dp(zb), None, *z4, 0.01, None, None, None, None, None, None), b"every output is NULL")
    for bad in (-1.0, float("nan"), float("inf")):
        invalid(lib.dexr_cross_penalty(ha, hb, n, dp(za), None, dp(zb), None, *z4, bad, None, dp(ze), dp(zxa), dp(zxb), None, None), b"margin")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (da, e, gxa, gxb, wa))  # nothing was launched
    assert all(np.isnan(a).all() for a in (zd, ze, zxa, zxb))


# ---- 8. autograd ---------------------------------------------------------------------------------------------------------------------------
def test_autograd_reaches_both_q_and_both_base_positions(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    opt_a, opt_b, side_a, side_b, x_a, fixed_a, x_b, d, case = order_case()
    sa, sb = side_a["sset"], side_b["sset"]
    qa, fa, qb, pa, ra, pb, rb, w = (_dev(torch, a) for a in (x_a, fixed_a, x_b, d["pos_a"], d["rot_a"], d["pos_b"], d["rot_b"], d["w"]))
    ma, mb = opt_a.sphere_model(sa), opt_b.sphere_model(sb)
    args = lambda qa_, qb_, pa_, pb_, ra_=ra, rb_=rb: (opt_a, qa_, sa, opt_b, qb_, sb, MARGIN, pa_, ra_, pb_, rb_, w, fa)  # noqa: E731
    E, ga, gb, wa, wb = collision.cross_penalty(*args(qa, qb, pa, pb), wrench=True)
    assert not E.requires_grad and bool((E > 0).any())
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    qag, qbg, pag, pbg = leaf(qa), leaf(qb), leaf(pa), leaf(pb)
    Eg = ag.cross_penalty(*args(qag, qbg, pag, pbg))
    assert Eg.requires_grad and torch.equal(Eg.detach(), E)
    Eg.sum().backward()
    assert torch.equal(qag.grad, ga) and torch.equal(qbg.grad, gb) and torch.equal(pag.grad, wa[:, :3]) and torch.equal(pbg.grad, wb[:, :3])
    assert float(pbg.grad.abs().max()) > 0
    scale = torch.linspace(0.5, 2.0, B, device="cuda")
    qbh = leaf(qb)  # one input alone: the forward computes that gradient only, the same bits
    (ag.cross_penalty(*args(qa, qbh, pa, pb)) * scale).sum().backward()
    assert torch.equal(qbh.grad, scale[:, None] * gb)
    pah = leaf(pa)
    (ag.cross_penalty(*args(qa, qb, pah, pb)) * scale).sum().backward()
    assert torch.equal(pah.grad, scale[:, None] * wa[:, :3])
    En = ag.cross_penalty(*args(qa, qb, pa, pb))
    assert torch.equal(En, E) and not En.requires_grad
    for bad in (dict(ra_=leaf(ra)), dict(rb_=leaf(rb))):
        with pytest.raises(ValueError, match="wrench=True"):
            ag.cross_penalty(*args(qa, qb, pa, pb, **bad))
        with pytest.raises(ValueError, match="wrench=True"):
            ag.cross_distances(opt_a, qa, sa, opt_b, qb, sb, pa, bad.get("ra_", ra), pb, bad.get("rb_", rb), fa)
    # the distances: the forward bits, backward is the VJP launch
    da, db = collision.cross_distances(opt_a, qa, sa, opt_b, qb, sb, pa, ra, pb, rb, fa)
    qad, qbd, pad, pbd = leaf(qa), leaf(qb), leaf(pa), leaf(pb)
    dag, dbg = ag.cross_distances(opt_a, qad, sa, opt_b, qbd, sb, pad, ra, pbd, rb, fa)
    assert torch.equal(dag.detach(), da) and torch.equal(dbg.detach(), db)
    ca, cb = _dev(torch, case["ga"]), _dev(torch, case["gb"])
    torch.autograd.backward([dag, dbg], [ca, cb])
    want = [_nan(torch, s) for s in ((B, ma.n_in), (B, mb.n_in), (B, 6), (B, 6))]
    ma.cross_distances_vjp_dev(mb, B, qa.data_ptr(), fa.data_ptr(), qb.data_ptr(), 0, ca.data_ptr(), cb.data_ptr(), *[t.data_ptr() for t in want],
                               pos_a_ptr=pa.data_ptr(), rot_a_ptr=ra.data_ptr(), pos_b_ptr=pb.data_ptr(), rot_b_ptr=rb.data_ptr(),
                               stream=torch.cuda.current_stream().cuda_stream)
    assert torch.equal(qad.grad, want[0]) and torch.equal(qbd.grad, want[1]) and torch.equal(pad.grad, want[2][:, :3]) and torch.equal(pbd.grad, want[3][:, :3])
    assert all(bool(torch.isfinite(t).all()) for t in want) and float(want[0].abs().max()) > 0 and float(want[3].abs().max()) > 0
    # the robot_* twins over the full qpos
    ra_, rb_ = opt_a.robot, opt_b.robot
    la, lb = ra_.joint_limits, rb_.joint_limits
    qra = _dev(torch, np.random.default_rng(233).uniform(la[:, 0], la[:, 1], (B, ra_.dof)))
    qrb = _dev(torch, np.random.default_rng(234).uniform(lb[:, 0], lb[:, 1], (B, rb_.dof)))
    out = collision.robot_cross_penalty(ra_, qra, sa, rb_, qrb, sb, MARGIN, pa, ra, pb, rb, w, wrench=True)
    wants = [_nan(torch, s) for s in ((B,), (B, ra_.dof), (B, rb_.dof), (B, 6), (B, 6))]
    ra_.sphere_model(sa).cross_penalty_dev(rb_.sphere_model(sb), B, qra.data_ptr(), 0, qrb.data_ptr(), 0, MARGIN, w.data_ptr(), *[t.data_ptr() for t in wants],
                                           pos_a_ptr=pa.data_ptr(), rot_a_ptr=ra.data_ptr(), pos_b_ptr=pb.data_ptr(), rot_b_ptr=rb.data_ptr(),
                                           stream=torch.cuda.current_stream().cuda_stream)
    assert all(torch.equal(u, v) for u, v in zip(out, wants))
    qrg = leaf(qrb)
    ag.robot_cross_penalty(ra_, qra, sa, rb_, qrg, sb, MARGIN, pa, ra, pb, rb, w).sum().backward()
    assert torch.equal(qrg.grad, wants[2])
    rd, cd = ag.robot_cross_distances(ra_, qra, sa, rb_, qrb, sb, pa, ra, pb, rb), collision.robot_cross_distances(ra_, qra, sa, rb_, qrb, sb, pa, ra, pb, rb)
    assert torch.equal(rd[0], cd[0]) and torch.equal(rd[1], cd[1])
    # empty batches
    e0 = collision.cross_penalty(opt_a, qa[:0], sa, opt_b, qb[:0], sb, MARGIN, fixed_qpos_a=fa[:0], wrench=True)
    assert e0[0].shape == (0,) and e0[1].shape == (0, opt_a.opt_dof) and e0[4].shape == (0, 6)


def test_two_hands_from_keypoints_to_cross_loss_end_to_end(require_gpu):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    rel = "teleop/allegro_hand_right.yml"
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    prob = cases.problem_from_config(rel)
    n = 64
    d = cases.human_set(prob, 2 * n)
    links = [f.name for f in opt.robot.kin.frames]
    S = len(links)
    sset = collision.SphereSet(links, np.zeros((S, 3)), np.full(S, 0.02))
    kps, lasts, qs = [], [], []
    for half in (slice(0, n), slice(n, 2 * n)):  # two retargets: the same robot stands in for both hands
        kp = glp._t(d["kp"][half], torch, dtype=torch.float32, requires_grad=True)
        last = glp._t(d["last"][half], torch, requires_grad=True)
        fixed = glp._t(d["fixed"][half], torch) if d["fixed"].shape[1] else None
        kps.append(kp)
        lasts.append(last)
        qs.append(ag.retarget(opt, ag.ref_value_from_keypoints(opt, kp), last, fixed, None))
    assert d["fixed"].shape[1] == 0
    pos_b = torch.tensor([[0.03, 0.02, 0.01]], device="cuda").repeat(n, 1).requires_grad_(True)  # the other hand 4 cm away, the same way up
    E = ag.cross_penalty(opt, qs[0], sset, opt, qs[1], sset, 0.01, None, None, pos_b, None)
    assert E.shape == (n,) and bool((E > 0).all())
    E.sum().backward()
    for kp in kps:
        assert bool(torch.isfinite(kp.grad).all()) and float(kp.grad.abs().max()) > 0
    assert bool(torch.isfinite(pos_b.grad).all()) and float(pos_b.grad.abs().max()) > 0 and all(bool(torch.isfinite(t.grad).all()) for t in lasts)

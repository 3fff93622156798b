"""CPU: the inputs of tests/objective_edges.py do what they are for, so that a green tests/test_gpu_objective_edges.py means
something.  Everything here is the oracle's arithmetic (float64 numpy); no GPU, no library call.

Run with -s to see, per (config, set), the share of residual rows past the Huber kink and the worst disagreement between the
oracle's minimisers from its two starts."""
import numpy as np
import pytest

import objective_edges as oe
from oracle import cases
from oracle.objectives import smooth_l1

GATE_RTOL, GATE_ATOL = 2e-6, 1e-9  # part A's gates (test_objective_matches_oracle_random_batch)


def _past_kink(rel, tag):
    """share of the residuals smooth_l1 sees, at the tracking starts, that lie past huber_delta"""
    prob = oe.problem(rel, tag)
    d = cases.reachable_set(prob, oe.B, 0.05)
    size = oe.residual_size(prob, d["last"].astype(np.float64), d["ref"], d["fixed"])
    return float((size >= prob.huber_delta).mean())


@pytest.mark.parametrize("rel", oe.CONFIGS)
def test_linear_and_quadratic_sets_reach_their_regions(rel):
    lin, quad = _past_kink(rel, "linear"), _past_kink(rel, "quadratic")
    print(f"{rel}: rows past the kink at the tracking starts: linear {lin:.3f}, quadratic {quad:.3f}, as shipped {_past_kink(rel, 'default'):.3f}")
    assert lin >= 0.8
    assert quad == 0.0


@pytest.mark.parametrize("rel,tag", oe.ALL_CASES)
def test_kink_rows_sit_where_intended(rel, tag):
    """The placed residuals lie within 2**-9 relative of huber_delta on the intended side AFTER the float32 rounding of the ref
    rows, every (term, side) occurs, and the last frame's residuals are at rounding level."""
    prob = oe.problem(rel, tag)
    k = oe.kink_inputs(rel, tag)
    size = oe.residual_size(prob, k["x"], k["ref"], k["fixed"])
    h = prob.huber_delta
    seen = set()
    for b in np.nonzero(k["row"] >= 0)[0]:
        got = np.atleast_1d(size[b, k["row"][b]]) / h - 1  # (three coordinates for position)
        assert np.all(np.abs(got) < 2.0 ** -9) and np.all(np.sign(got) == k["side"][b]), (b, got)
        seen.add((int(k["row"][b]), int(k["side"][b])))
    assert seen == {(t, s) for t in range(prob.n_ref) for s in (1, -1)}
    tail = size[oe.B - 1]
    if prob.kind == "dexpilot":  # (a projected pair row's target is not the FK value)
        tail = tail[prob.n_pair:]
    assert tail.max() <= np.spacing(np.abs(k["ref"][oe.B - 1]).max()) * max(1.0, prob.scaling) and k["row"][oe.B - 1] == -1  # float32 rounding of the row


def test_smooth_l1_is_c1_and_the_kink_rows_tell_the_branches_apart():
    """smooth_l1 is C1: value and derivative of the two branches meet at the kink, so a row 2**-10 past it costs nothing in
    conditioning.  AT the placed rows the branches differ by beta 2**-21 in value -- below part A's gate -- and by 2**-10 relative in
    the derivative -- 500 times the gate: a kernel that took the other branch there (<= for <, another field for the threshold)
    fails part A on the gradient."""
    for beta in (2e-3, 0.01, 0.02, 0.03, 0.5):
        lo, hi = np.nextafter(beta, 0), beta
        (v0, v1), (d0, d1) = smooth_l1(np.array([lo, hi]), beta)
        assert abs(v1 - v0) <= 4 * np.spacing(beta) and abs(d1 - d0) <= 4 * np.spacing(1.0)
        for side in (1, -1):
            d = beta * (1 + side * oe.KINK_EPS)
            quad, lin = (0.5 * d * d / beta, d / beta), (d - 0.5 * beta, 1.0)
            assert abs(quad[0] - lin[0]) == pytest.approx(beta * 2.0 ** -21, rel=1e-6)
            assert abs(quad[0] - lin[0]) < GATE_RTOL * smooth_l1(np.array([d]), beta)[0][0]
            assert abs(quad[1] - lin[1]) > 400 * GATE_RTOL


@pytest.mark.parametrize("rel,tag", oe.ALL_CASES)
def test_wrong_branch_at_a_kink_row_exceeds_the_gradient_gate(rel, tag):
    """... and on the frames themselves: the oracle's gradient with the kink row's derivative taken from the OTHER branch misses
    the gate of part A on most frames (a row whose Jacobian is nearly orthogonal to its residual shows nothing)."""
    prob = oe.problem(rel, tag)
    k = oe.kink_inputs(rel, tag)
    kw, _ = oe.dexpilot_kw(prob, k["ref"])
    _, g, _ = prob.evaluate(k["x"], k["ref"], k["fixed"], k["last"].astype(np.float64), **kw)
    moved = oe.kink_inputs(rel, tag, flip=True)  # the same rows on the other side of the kink
    kw2, _ = oe.dexpilot_kw(prob, moved["ref"])
    _, g2, _ = prob.evaluate(k["x"], moved["ref"], k["fixed"], k["last"].astype(np.float64), **kw2)
    placed = (k["row"] >= 0) & (k["row"] == moved["row"])
    # across the kink the derivative of the row changes by 2**-10 (quadratic side) or not at all (linear side): the gradients of the
    # two placements differ by about as much as a wrong branch would make them differ
    far = np.abs(g - g2).max(1) > GATE_RTOL * np.abs(g).max(1) + GATE_ATOL
    print(f"{rel} {tag}: {int((far & placed).sum())} of {int(placed.sum())} kink frames tell the sides apart by more than the gate")
    assert (far & placed).sum() >= 0.5 * placed.sum()


@pytest.mark.parametrize("rel", oe.DEXPILOT_CONFIGS)
def test_threshold_sets_are_complete_and_off_the_ties(rel):
    prob, dflt = oe.problem(rel, "dexpilot"), oe.problem(rel)
    len_s1 = prob.num_fingers - 1
    r = oe.threshold_rows(rel)
    prior = oe.unbits(r["state"], prob.n_pair)
    cells = {(int(c), bool(p), col < len_s1) for c, p, col in
             zip(r["cls"].ravel(), prior.ravel(), np.tile(np.arange(prob.n_pair), oe.B))}
    assert len(cells) == oe.N_CLASS * 2 * 2  # every (length class, prior bit, first / second stage row)
    assert oe.off_ties(prob, r["ref"]).all()
    k = oe.threshold_keypoints(rel)
    assert set(zip(k["pair"].tolist(), k["cls"].tolist())) == {(p, c) for p in range(prob.n_pair) for c in range(oe.N_CLASS)}
    assert set(oe.unbits(k["state"], prob.n_pair)[np.arange(oe.B), k["pair"]].tolist()) == {False, True}
    assert oe.off_ties(prob, k["ref"], skip=k["pair"]).all()
    want = oe.class_length(prob, k["cls"])
    got = np.linalg.norm(k["ref"][np.arange(oe.B), k["pair"]].astype(np.float64), axis=1)
    assert np.all(np.abs(got / want - 1) < 2.0 ** -16)  # the float32 subtraction of two keypoints keeps the placed length
    s = oe.threshold_sequences(rel)
    for name, ref, st in [("rows", r["ref"], r["state"]), ("keypoints", k["ref"], k["state"])] + \
            [(f"sequence frame {t}", s["ref"][t], None) for t in range(3)]:
        if st is None:  # walk the sequence with the float64 oracle's own bits
            st = s["state"] if name.endswith("0") else carried
        b32, b64 = oe.oracle_bits(prob, ref, st, np.float32), oe.oracle_bits(prob, ref, st, np.float64)
        assert np.array_equal(b32, b64), name  # 2**-12 is enough margin: float32 distances decide every bit as float64 ones do
        carried = b64
        differ = oe.unbits(b64 ^ oe.oracle_bits(dflt, ref, st, np.float64), prob.n_pair).mean()
        print(f"{rel} {name}: {differ:.3f} of the bits differ from what the default thresholds give")
        if name == "rows":
            assert differ >= 1.0 / 3.0
    # the middle frame of a sequence is decided by the carried bit: inside -> between keeps it set, outside -> between clear
    mid = oe.unbits(oe.oracle_bits(prob, s["ref"][1], oe.oracle_bits(prob, s["ref"][0], s["state"]), np.float64), prob.n_pair)
    chosen = mid[np.arange(oe.B), s["pair"]]
    first_stage = s["pair"] < len_s1
    assert np.array_equal(chosen[first_stage], (np.arange(oe.B) % 2 == 0)[first_stage])


@pytest.mark.parametrize("rel,tag", oe.SOLVE_CASES)
def test_oracle_minimiser_is_unique_on_every_tracking_frame(rel, tag):
    """Part C's 1 % allowance must not hide a failure: the oracle alone needs none -- from the tracking start and from a second
    seeded start 0.05 rad away it reaches the same point, to 1e-6 rad, on EVERY frame of every (config, set)."""
    t = oe.tracking(rel, tag)
    dx = np.abs(t["want"] - oe.second_start(rel, tag)).max(1)
    print(f"{rel} {tag}: worst |x(start 1) - x(start 2)| = {dx.max():.2e} rad (frame {int(dx.argmax())})")
    assert dx.max() < 1e-6


@pytest.mark.parametrize("rel", oe.DEXPILOT_CONFIGS)
def test_pinched_frames_project_both_stages_and_have_a_unique_minimiser(rel):
    """What brings non-default eta1 / eta2 into a SOLVE: every frame of pinch_tracking projects a first-stage pair, 16 of the 64
    a second-stage one, and the oracle's two starts agree to 1e-6 rad on every frame.  (Printed for contrast: what part C's
    tracking frames project per set -- nothing at the `dexpilot` set.)"""
    for tag, _ in oe.variants(rel, [s for s in oe.SETS if s != "free"]):
        st = oe.dexpilot_kw(oe.problem(rel, tag), oe.tracking(rel, tag)["d"]["ref"])[1]
        print(f"{rel} {tag}: part C's frames project {int(st.sum())} pairs")
    t = oe.pinch_tracking(rel)
    prob, st = t["prob"], t["projected"]
    len_s1 = prob.num_fingers - 1
    assert (prob.projected_dist[0], prob.projected_dist[-1]) == (5e-3, 1e-2) != (1e-4, 3e-2)
    s1, s2 = st[:, :len_s1], st[:, len_s1:]
    print(f"{rel} pinched frames ({t['tag']}): {int(s1.sum())} first-stage pairs on {int(s1.any(1).sum())} frames, "
          f"{int(s2.sum())} second-stage pairs on {int(s2.any(1).sum())} frames")
    assert s1.any(1).all() and s2.any(1).sum() == 16
    dx = np.abs(t["want"] - oe.second_start_of(t)).max(1)
    print(f"{rel} pinched frames: worst |x(start 1) - x(start 2)| = {dx.max():.2e} rad (frame {int(dx.argmax())})")
    assert dx.max() < 1e-6


@pytest.mark.parametrize("rel", oe.CONFIGS)
def test_component_tables_carry_the_float32_rounding_residue(rel):
    """Table v6: X_lo / mult_lo / off_lo / frame_off_lo hold what float32 dropped from the kinematic constants -- at most half
    an ulp of the stored field each, not all zero -- so that field + field_lo is the float64 constant the closure (dexr_eval)
    is compared against at rounding-level residuals."""
    comps = oe.build_optimizer(rel, "stiff").optimizer.compiled_model().comps
    seen = 0.0
    for hi, lo in (("X", "X_lo"), ("mult", "mult_lo"), ("off", "off_lo"), ("frame_off", "frame_off_lo")):
        a, b = comps[hi].astype(np.float64), comps[lo].astype(np.float64)
        assert np.all(np.abs(b) <= 0.5 * np.spacing(np.abs(comps[hi])).astype(np.float64) * (1 + 1e-6)), hi
        assert np.all(b[a == 0] == 0)
        seen = max(seen, float(np.abs(b).max()))
    assert 1e-10 < seen < 1e-7  # constants of ~0.05 m / ~1 rad lose 1e-9 .. 6e-8 to float32

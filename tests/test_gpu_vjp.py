"""GPU tests of the differentiable solve: MODE_VJP of the general kernel (dexr_retarget_vjp*) against the float64 reference
VJP (tests/vjp_reference.py) on every shipped config and on the arm + hand model only the general kernel serves, against
finite differences of the oracle's tight solve, through torch autograd, and the entry points' contracts."""
import json
import os

import numpy as np
import pytest

from testutil import REPO
from vjp_reference import Targets, excluded, held_mask, vjp_reference

from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases, solvers

pytestmark = pytest.mark.gpu
RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))

ALL = sorted(os.path.relpath(os.path.join(d, f), cases.CONFIG_DIR) for d, _, fs in os.walk(cases.CONFIG_DIR)
             for f in fs if f.endswith(".yml"))
GOLDEN = os.path.join(REPO, "tests", "golden", "vjp_excluded_counts.json")
FOUR = ["teleop/allegro_hand_right.yml", "teleop/shadow_hand_right_dexpilot.yml", "offline/leap_hand_right.yml",
        "teleop/schunk_svh_hand_right.yml"]


def _seq(rel):
    return RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build()


def _solve(opt, prob, B, seed=cases.SEED):
    """Product-path answers on B human-keypoint frames: (ref, fixed, last, state the forward read, q)."""
    d = cases.human_set(prob, B, seed=seed)
    st = np.zeros(B, np.uint32) if prob.kind == "dexpilot" else None
    st_in = None if st is None else st.copy()
    q = opt.retarget_batch(d["ref"], d["fixed"], d["last"], state=st)
    return d["ref"], d["fixed"], d["last"], st_in, q


def _rel(a, b):
    a = a.reshape(a.shape[0], -1).astype(np.float64)
    b = b.reshape(b.shape[0], -1)
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


def _compare(opt, prob, ref, fixed, last, st, q, seed=0):
    """GPU VJP at the GPU's q against the reference at that q: (excluded mask, worst relative errors on the kept frames)."""
    gq = np.random.default_rng(seed).standard_normal(q.shape).astype(np.float32)
    gref, glast, status = opt.vjp_model().vjp(ref, fixed, last, q, gq, state=st)
    wref, wlast, info = vjp_reference(prob, ref, fixed, last, q.astype(np.float64), gq, state=st, return_info=True)
    ex = excluded(info)
    keep = ~ex
    assert np.all(status[keep] == 0), np.flatnonzero(status[keep])
    er, el = _rel(gref, wref)[keep], _rel(glast, wlast)[keep]
    nz = np.linalg.norm(wlast.reshape(len(q), -1), axis=1)[keep] > 0  # (every variable held: both sides are 0)
    return ex, float(er[nz].max(initial=0.0)), float(el[nz].max(initial=0.0))


def test_vjp_matches_the_reference_on_every_config():
    counts = {}
    worst = {}
    B = 512
    for rel in ALL:
        seq = _seq(rel)
        prob = cases.problem_from_config(rel)
        ref, fixed, last, st, q = _solve(seq.optimizer, prob, B)
        ex, er, el = _compare(seq.optimizer, prob, ref, fixed, last, st, q)
        counts[rel] = int(ex.sum())
        worst[rel] = (er, el)
    # (reported with -s: the excluded counts per config are what tests/golden/vjp_excluded_counts.json pins)
    print(json.dumps(dict(excluded_of_512=counts, worst=worst), sort_keys=True))
    for rel in ALL:
        assert counts[rel] <= B // 50, (rel, counts[rel])
        assert worst[rel][0] <= 1e-5 and worst[rel][1] <= 1e-5, (rel, worst[rel])
    with open(GOLDEN) as f:
        pinned = json.load(f)["excluded_of_512"]
    for rel in ALL:
        assert counts[rel] <= pinned[rel], (rel, counts[rel], pinned[rel])


def test_vjp_on_the_arm_and_hand_model():
    from test_gpu_generic import arm_hand

    seq, prob = arm_hand("position")
    opt = seq.optimizer
    assert opt.opt_dof == 37 and opt.vjp_model().kernel()[0] == _lib.KERNEL_GENERAL
    B = 64
    d = cases.human_set(prob, B)
    q = opt.retarget_batch(d["ref"], d["fixed"], d["last"])
    ex, er, el = _compare(opt, prob, d["ref"], d["fixed"], d["last"], None, q)
    assert ex.sum() <= max(1, B // 50) and er <= 1e-5 and el <= 1e-5, (ex.sum(), er, el)


@pytest.mark.parametrize("rel", FOUR)
def test_vjp_is_the_derivative_of_the_solve(rel):
    """The VJP-derived directional derivative against central differences of the oracle's tight solve around the GPU's q."""
    seq = _seq(rel)
    prob = cases.problem_from_config(rel)
    B = 16
    h = 2.0 ** -13
    d = cases.human_set(prob, B)
    ref, fixed = d["ref"], d["fixed"]
    last = (np.round(d["last"] / h) * h).astype(np.float32)  # (last +- h dl stays exact in float32)
    st = np.zeros(B, np.uint32) if prob.kind == "dexpilot" else None
    q = seq.optimizer.retarget_batch(ref, fixed, last, state=None if st is None else st.copy())
    rng = np.random.default_rng(3)
    gq = rng.standard_normal(q.shape).astype(np.float32)
    gref, glast, status = seq.optimizer.vjp_model().vjp(ref, fixed, last, q, gq, state=st)
    assert np.all(status == 0)
    tg = Targets(prob, ref, st)
    dr = rng.standard_normal(ref.shape)
    dr /= np.linalg.norm(dr.reshape(B, -1), axis=1)[:, None, None]
    dl = rng.choice([-1.0, 1.0], size=last.shape)
    r64, l64 = ref.astype(np.float64), last.astype(np.float64)
    x0 = q.astype(np.float64)

    def tight(r, l):
        return solvers.solve_lm_batched(prob, r, fixed, l, x0=x0, tol=1e-12, newton=True, max_iter=200, **tg.kw_at(r))

    fd = np.einsum("bn,bn->b", gq, (tight(r64 + h * dr, l64 + h * dl) - tight(r64 - h * dr, l64 - h * dl)) / (2 * h))
    an = np.einsum("bij,bij->b", gref, dr) + np.einsum("bn,bn->b", glast, dl)
    scale = np.linalg.norm(gref.reshape(B, -1), axis=1) + np.linalg.norm(glast, axis=1)
    assert (np.abs(fd - an) / scale).max() <= 1e-3, np.abs(fd - an) / scale


# ---- torch autograd -------------------------------------------------------------------------------------------------------
def _t(a, torch, **kw):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", **kw)


@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "teleop/shadow_hand_right_dexpilot.yml"])
def test_autograd_forward_and_backward(rel):
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    seq = _seq(rel)
    opt = seq.optimizer
    prob = cases.problem_from_config(rel)
    B = 256
    ref, fixed, last, st, q_host = _solve(opt, prob, B)
    ref_t = _t(ref, torch, requires_grad=True)
    last_t = _t(last, torch, requires_grad=True)
    fixed_t = _t(fixed, torch) if fixed.shape[1] else None
    st_t = None if st is None else _t(st.astype(np.int32), torch)
    q_t = ag.retarget(opt, ref_t, last_t, fixed_t, st_t)
    assert np.array_equal(q_t.detach().cpu().numpy(), q_host)  # bitwise: the product solve
    gq = torch.randn(q_t.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    g_ref, g_last = torch.autograd.grad(q_t, (ref_t, last_t), gq)
    # the direct device call
    gr = torch.zeros_like(ref_t)
    gl = torch.zeros_like(last_t)
    stat = torch.zeros(B, dtype=torch.int32, device="cuda")
    st_in = None if st is None else _t(st.astype(np.int32), torch)
    q_c = _t(q_host, torch)
    opt.vjp_model().vjp_dev(B, ref_t.detach().data_ptr(), 0 if fixed_t is None else fixed_t.data_ptr(), last_t.detach().data_ptr(),
                            0 if st_in is None else st_in.data_ptr(), q_c.data_ptr(), gq.contiguous().data_ptr(), gr.data_ptr(),
                            gl.data_ptr(), stat.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(g_ref, gr) and torch.equal(g_last, gl)
    # host twin == device call, bitwise
    hr, hl, hs = opt.vjp_model().vjp(ref, fixed, last, q_host, gq.cpu().numpy(), state=st)
    assert np.array_equal(hr, gr.cpu().numpy()) and np.array_equal(hl, gl.cpu().numpy()) and np.array_equal(hs, stat.cpu().numpy())
    # gradients reach raw keypoints
    kp = _t(cases.human_set(prob, B)["kp"], torch, dtype=torch.float32, requires_grad=True)
    rv = ag.ref_value_from_keypoints(opt, kp)
    assert torch.equal(rv.detach(), ref_t.detach())
    q2 = ag.retarget(opt, rv, last_t.detach(), fixed_t, None if st is None else _t(st.astype(np.int32), torch))
    (g_kp,) = torch.autograd.grad(q2, kp, gq)
    (want,) = torch.autograd.grad(ag.ref_value_from_keypoints(opt, kp), kp, g_ref)
    assert torch.equal(g_kp, want) and bool(torch.isfinite(g_kp).all()) and float(g_kp.abs().max()) > 0


@pytest.mark.parametrize("rel", ["teleop/allegro_hand_right.yml", "teleop/shadow_hand_right_dexpilot.yml"])
def test_autograd_through_a_three_frame_chain(rel):
    """Three frames of 16 sequences: clamp to the joint limits and the LPFilter update in torch between frames; d loss / d
    (every frame's ref_value, the first last_qpos) against differences of the same chain run with the oracle's tight solve."""
    torch = pytest.importorskip("torch")
    from dex_retargeting_amd import autograd as ag

    seq = _seq(rel)
    opt = seq.optimizer
    prob = cases.problem_from_config(rel)
    S, T = 16, 3
    alpha = 0.5
    lim = prob.joint_limits
    frames = [cases.human_set(prob, S, seed=cases.SEED + t) for t in range(T)]
    refs = [f["ref"] for f in frames]
    fixed = frames[0]["fixed"]
    h = 2.0 ** -13
    last0 = (np.round(frames[0]["last"] / h) * h).astype(np.float32)
    dexp = prob.kind == "dexpilot"
    w = np.random.default_rng(9).standard_normal((S, prob.n_opt))
    # autograd chain
    lo_t, hi_t = _t(lim[:, 0].astype(np.float32), torch), _t(lim[:, 1].astype(np.float32), torch)
    ref_ts = [_t(r, torch, requires_grad=True) for r in refs]
    last_t0 = _t(last0, torch, requires_grad=True)
    st_t = _t(np.zeros(S, np.int32), torch) if dexp else None
    fixed_t = _t(fixed, torch) if fixed.shape[1] else None
    last_t, y = last_t0, None
    states = []
    for t in range(T):
        states.append(None if st_t is None else st_t.cpu().numpy().astype(np.uint32))
        q = ag.retarget(opt, ref_ts[t], last_t, fixed_t, st_t)
        y = q if y is None else y + alpha * (q - y)
        last_t = torch.clamp(q, lo_t, hi_t)
    loss = (y.double() * _t(w, torch)).sum()
    grads = torch.autograd.grad(loss, ref_ts + [last_t0])
    # the same chain with the oracle's tight solve (DexPilot bits held at the autograd run's)
    rng = np.random.default_rng(4)
    drs = [rng.standard_normal(r.shape) * 1e-1 for r in refs]
    dl = rng.choice([-1.0, 1.0], size=last0.shape)

    def chain(sign):
        last = last0.astype(np.float64) + sign * h * dl
        y = None
        for t in range(T):
            r = refs[t].astype(np.float64) + sign * h * drs[t]
            tg = Targets(prob, refs[t], states[t])
            x = solvers.solve_lm_batched(prob, r, fixed, last, tol=1e-12, newton=True, max_iter=200, **tg.kw_at(r))
            y = x if y is None else y + alpha * (x - y)
            last = np.clip(x, lim[:, 0], lim[:, 1]).astype(np.float32)  # (the forward's last_qpos rows are float32)
        return (y * w).sum(1)

    fd = (chain(1.0) - chain(-1.0)) / (2 * h)
    an = sum((g.cpu().numpy().astype(np.float64) * dr).reshape(S, -1).sum(1) for g, dr in zip(grads[:T], drs)) + \
        (grads[T].cpu().numpy() * dl).sum(1)
    scale = sum(np.linalg.norm((g.cpu().numpy() * dr).reshape(S, -1), axis=1) for g, dr in zip(grads[:T], drs)) + \
        np.linalg.norm(grads[T].cpu().numpy(), axis=1)
    assert (np.abs(fd - an) / scale).max() <= 1e-3, np.abs(fd - an) / scale


# ---- entry points -----------------------------------------------------------------------------------------------------------
def test_entry_points_ragged_batches_and_statuses():
    rel = "teleop/shadow_hand_right_dexpilot.yml"
    seq = _seq(rel)
    opt = seq.optimizer
    prob = cases.problem_from_config(rel)
    B = 4097
    ref, fixed, last, st, q = _solve(opt, prob, B)
    gq = np.random.default_rng(1).standard_normal(q.shape).astype(np.float32)
    m = opt.vjp_model()
    full = m.vjp(ref, fixed, last, q, gq, state=st)
    for b in (1, 63, 64, 65, 4097):
        part = m.vjp(ref[:b], fixed[:b], last[:b], q[:b], gq[:b], state=st[:b])
        for a, f in zip(part, full):
            assert np.array_equal(a, f[:b]), b
    # B = 0
    z = m.vjp(ref[:0], fixed[:0], last[:0], q[:0], gq[:0], state=st[:0])
    assert z[0].shape == (0,) + ref.shape[1:]
    # non-finite ref / q: status 2, zero outputs; the other frames are untouched
    r2, q2 = ref[:8].copy(), q[:8].copy()
    r2[1, 0, 0] = np.nan
    q2[2, 0] = np.inf
    gr, gl, s = m.vjp(r2, fixed[:8], last[:8], q2, gq[:8], state=st[:8])
    assert list(s[1:3]) == [2, 2] and not gr[1:3].any() and not gl[1:3].any()
    assert np.array_equal(gr[3:], full[0][3:8]) and np.array_equal(s[3:], full[2][3:8])
    # a handle on the fixed-size tables has no VJP mode
    with pytest.raises(_lib.DexrError, match="general kernel"):
        opt.device_model().vjp(ref[:4], fixed[:4], last[:4], q[:4], gq[:4], state=st[:4])
    assert held_mask(prob, q.astype(np.float64)).any()  # (the batch exercises the held set)

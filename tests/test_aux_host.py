"""CPU tests around the small kernels of dexr_aux.hip: the numpy references the GPU tests compare with
(tests/aux_reference.py) are themselves pinned -- the compose reference to the reference project's recorded results, the
key reference's threshold band to its cap -- and dexr_seq_compose_dev's argument checks, which return before any device
call, are exercised one by one."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import aux_reference as ar
from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.device_seq import DeviceSeqRetargeting
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from testutil import REPO

GOLD = os.path.join(REPO, "tests", "golden")
RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
SHADOW_DEXPILOT = "teleop/shadow_hand_right_dexpilot.yml"


# ---- fleet_partition ----------------------------------------------------------------------------------------------------
def test_fleet_partition_reference_on_a_hand_checked_case():
    counts, offsets, perm, n_bad = ar.fleet_partition([2, 0, 7, 2, -1, 1, 0, 3], 3)
    assert counts.tolist() == [2, 1, 2] and offsets.tolist() == [0, 2, 3]
    assert perm.tolist() == [1, 6, 5, 0, 3] and n_bad == 3


# ---- seq_compose --------------------------------------------------------------------------------------------------------
def dof_map_of(rel):
    """DeviceSeqRetargeting._dof_map without a device: it reads nothing but `.optimizer`."""
    seq = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build()
    opt = seq.optimizer
    return DeviceSeqRetargeting._dof_map(types.SimpleNamespace(optimizer=opt)), opt


@pytest.mark.parametrize("key", ["teleop__allegro_hand_right", "teleop__ability_hand_right", "offline__inspire_hand_right",
                                 "teleop__panda_gripper"])
def test_compose_reference_reproduces_the_recorded_wrapper_results(key):
    """aux_reference.seq_compose on the recorded optimiser answers == the reference project's own
    SeqRetargeting.retarget around a replaying stub (tests/golden/seq_wrapper_golden.npz) to 1e-12, in one call and in
    two calls that carry the filter: the GPU tests' reference is grounded in the original, not in the kernel."""
    g = np.load(os.path.join(GOLD, "seq_wrapper_golden.npz"))
    (kind, idx, mult, off), opt = dof_map_of(key.replace("__", "/") + ".yml")
    assert opt.robot.dof_joint_names == g[key + "__joint_names"].tolist()
    ans = g[key + "__answers"]  # (T, n_opt) float32
    want = g[key + "__robot_qpos"]
    T, n_q = want.shape
    alpha = float(g[key + "__alpha"])
    n_fixed = len(opt.idx_pin2fixed)
    fixed = np.zeros((T, 1, n_fixed), np.float32) if n_fixed else None
    out, filt = ar.seq_compose(kind, idx, mult, off, ans[:, None], fixed, alpha, np.zeros((1, n_q)), True)
    assert out.shape == (T, 1, n_q)
    assert np.abs(out[:, 0] - want).max() < 1e-12
    if 0 <= alpha <= 1:
        assert np.array_equal(filt[0], out[-1, 0])
    a, f1 = ar.seq_compose(kind, idx, mult, off, ans[:5, None], None if fixed is None else fixed[:5], alpha,
                           np.zeros((1, n_q)), True)
    b, _ = ar.seq_compose(kind, idx, mult, off, ans[5:, None], None if fixed is None else fixed[5:], alpha, f1, False)
    assert np.array_equal(np.concatenate([a, b]), out)


def test_compose_reference_on_a_hand_checked_case():
    """Two sequences, two frames, every kind of dof, numbers small enough to check by hand."""
    kind, idx = [0, 1, 2, 2], [1, 0, 0, 1]
    mult, off = [1.0, 1.0, 2.0, -1.0], [0.0, 0.0, 0.5, 0.25]
    qraw = np.array([[[9, 1], [9, 2]], [[9, 3], [9, 4]]], np.float32)     # (T, B, n_opt = 2): column 1 is read
    fixed = np.array([[[10], [20]], [[30], [40]]], np.float32)             # (T, B, n_fixed = 1)
    out, y = ar.seq_compose(kind, idx, mult, off, qraw, fixed, -1.0, None, True)
    assert y is None
    assert out[0].tolist() == [[1, 10, 2.5, -9.75], [2, 20, 4.5, -19.75]]
    assert out[1].tolist() == [[3, 30, 6.5, -29.75], [4, 40, 8.5, -39.75]]
    f0 = np.array([[0.0, 0, 0, 0], [2, 20, 4.5, -19.75]])
    out, y = ar.seq_compose(kind, idx, mult, off, qraw, fixed, 0.5, f0, False)
    assert out[0].tolist() == [[0.5, 5, 1.25, -4.875], [2, 20, 4.5, -19.75]]
    assert out[1].tolist() == [[1.75, 17.5, 3.875, -17.3125], [3, 30, 6.5, -29.75]]
    assert np.array_equal(y, out[1]) and f0[0, 0] == 0.0  # (the carried state is returned, the argument is left alone)
    out, y = ar.seq_compose(kind, idx, mult, off, qraw, fixed, 0.5, f0, True)
    assert out[0].tolist() == [[1, 10, 2.5, -9.75], [2, 20, 4.5, -19.75]]


# ---- dexpilot_keys ------------------------------------------------------------------------------------------------------
def ordering_inputs(prob, B):
    """The frames and incoming projection bits of the ordering tests (tests/test_gpu_fleet_order.py): frame b is frame
    b + 1 of the human keypoint set, its incoming bits are what the pre-amble makes of frame b from a cleared state --
    consecutive frames of the recording, so bits switch on, stay on and switch off."""
    kp = cases.human_keypoints(B + 1, seed=9)
    _, state_in, _ = ar.dexpilot_keys(prob, kp[:-1], np.zeros(B, np.uint32))
    return np.ascontiguousarray(kp[1:]), state_in


@pytest.mark.parametrize("B", [6000, 40000])
def test_key_reference_has_every_class_and_few_frames_at_a_threshold(B):
    """Shadow DexPilot on the ordering tests' inputs: all three key classes occur, and the frames the GPU tests exclude
    from the key comparison (a pair-row length within 1e-6 m of 0.03 or 0.05) stay under 0.5 % of the batch.
    Seen: B = 6 000 keys 194 / 675 / 5 131 and 5 near frames; B = 40 000 keys 1 276 / 4 625 / 34 099 and 13."""
    prob = cases.problem_from_config(SHADOW_DEXPILOT)
    kp, state_in = ordering_inputs(prob, B)
    key, new_bits, near = ar.dexpilot_keys(prob, kp, state_in)
    n = np.bincount(key, minlength=3)
    print(f"B={B}: keys {n.tolist()}, near {int(near.sum())}")
    assert len(n) == 3 and n.sum() == B and np.all(n > 0)
    assert near.mean() <= 0.005
    # the key restates the bits: 0 <=> a bit differs, 1 <=> unchanged and some bit set, 2 <=> unchanged and none set
    assert np.array_equal(key == 0, new_bits != state_in)
    assert np.array_equal(key == 1, (new_bits == state_in) & (new_bits != 0))
    assert np.all(new_bits < (1 << prob.n_pair))


def test_key_reference_flags_lengths_at_a_threshold():
    prob = cases.problem_from_config(SHADOW_DEXPILOT)
    idx = prob.target_link_human_indices
    kp = np.zeros((4, 21, 3), np.float32)
    kp[:, :, 0] = np.arange(21)[None] * 0.5  # every pair row far longer than any threshold ...
    o, t = int(idx[0][0]), int(idx[1][0])     # ... but pair row 0
    for b, length in enumerate((0.03 + 5e-7, 0.05 - 5e-7, 0.03 + 1e-4, 0.04)):
        kp[b, t] = kp[b, o] + np.array([length, 0, 0], np.float32)
    key, new_bits, near = ar.dexpilot_keys(prob, kp, np.array([0, 1, 0, 1], np.uint32))
    assert near.tolist() == [True, True, False, False]
    assert new_bits[2:].tolist() == [0, 1] and key[2:].tolist() == [2, 1]


# ---- dexr_seq_compose_dev: refusals -------------------------------------------------------------------------------------
def compose(B=2, T=2, n_q=3, n_opt=2, n_fixed=2, kind=(0, 1, 2), idx=(1, 0, 0), alpha=-1.0, fixed=True, filt=False):
    """One raw call of dexr_seq_compose_dev on small HOST arrays: every case below is refused (or is empty) before the
    entry point touches a pointer, so nothing is dereferenced and no device is needed."""
    n = max(n_q, 1)
    kind = np.resize(np.asarray(kind, np.int32), n)
    idx = np.resize(np.asarray(idx, np.int32), n)
    mult, off = np.ones(n), np.zeros(n)
    rows = max(B, 1) * max(T, 1)
    qraw = np.zeros(rows * max(n_opt, 1), np.float32)
    fx = np.zeros(rows * max(n_fixed, 1), np.float32)
    fl = np.zeros(max(B, 1) * n)
    out = np.full(rows * n, 7.0)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    vp = lambda a, on=True: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    rc = _lib.load().dexr_seq_compose_dev(B, T, n_q, n_opt, n_fixed, kind.ctypes.data_as(i32p), idx.ctypes.data_as(i32p),
                                          mult.ctypes.data_as(f64p), off.ctypes.data_as(f64p), vp(qraw), vp(fx, fixed),
                                          float(alpha), vp(fl, filt), 1, vp(out), None)
    assert np.all(out == 7.0) and np.all(fl == 0.0)
    _lib.check(rc)


REFUSALS = [
    (dict(n_q=0), r"n_q=0 outside 1\.\.64"),
    (dict(n_q=65, kind=(0,), idx=(0,)), r"n_q=65 outside 1\.\.64"),
    (dict(B=-1), "negative size"),
    (dict(T=-1), "negative size"),
    (dict(n_opt=-1), "negative size"),
    (dict(n_fixed=-1), "negative size"),
    (dict(kind=(0, 1, 3)), r"dof 2: malformed source \(kind 3, idx 0\)"),
    (dict(kind=(0, -1, 2)), r"dof 1: malformed source \(kind -1, idx 0\)"),
    (dict(idx=(2, 0, 0)), r"dof 0: malformed source \(kind 0, idx 2\)"),      # target column >= n_opt
    (dict(idx=(1, 2, 0)), r"dof 1: malformed source \(kind 1, idx 2\)"),      # fixed column >= n_fixed
    (dict(kind=(0, 2, 2), idx=(0, 0, 1)), r"dof 2: malformed source \(kind 2, idx 1\)"),  # a mimic of a mimic
    (dict(idx=(1, 0, 3)), r"dof 2: malformed source \(kind 2, idx 3\)"),      # mimic source >= n_q
    (dict(idx=(1, 0, -1)), r"dof 2: malformed source \(kind 2, idx -1\)"),
    (dict(fixed=False), "dof 1 is a fixed joint but fixed is NULL"),
    (dict(alpha=0.0), "low-pass coefficient was given but filter_inout is NULL"),
    (dict(alpha=0.3), "low-pass coefficient was given but filter_inout is NULL"),
    (dict(alpha=1.0), "low-pass coefficient was given but filter_inout is NULL"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{'-'.join(k)}" for i, (k, _) in enumerate(REFUSALS)])
def test_seq_compose_refuses_bad_arguments(kw, message):
    with pytest.raises(_lib.DexrError, match=message):
        compose(**kw)


@pytest.mark.parametrize("kw", [dict(B=0), dict(T=0), dict(B=0, T=0), dict(B=0, alpha=0.3, filt=True)])
def test_seq_compose_accepts_empty_batches(kw):
    compose(**kw)  # DEXR_OK: nothing to do, nothing written

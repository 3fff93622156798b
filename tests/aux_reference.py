"""Plain numpy references of the small kernels around the solve (dex_retargeting_amd/csrc/dexr_aux.hip): the stable
partition of a fleet batch by model id, the hard-frames-first keys of a DexPilot batch and the per-frame bookkeeping of
SeqRetargeting.  Test infrastructure only; float64, one obvious statement per step, nothing shared with the kernels."""
import numpy as np

from oracle import cases

# the two lengths the DexPilot pre-amble compares a pair row with (optimizer.py:466-476: project_dist and the second
# set's 0.03, escape_dist) for every config of this package
KEY_THRESHOLDS = (0.03, 0.05)
NEAR_BAND = 1e-6


def fleet_partition(model_id, n_models):
    """Stable partition of the frame indices by model id -> counts (n_models,), offsets (n_models,), perm (sum(counts),)
    = the concatenation over m of the frames of model m in batch order, n_bad = frames whose id is outside [0, n_models)."""
    model_id = np.asarray(model_id).astype(np.int64)
    segs = [np.flatnonzero(model_id == m) for m in range(n_models)]
    counts = np.array([len(s) for s in segs], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    perm = np.concatenate(segs).astype(np.int64) if segs else np.zeros(0, np.int64)
    n_bad = int(((model_id < 0) | (model_id >= n_models)).sum())
    assert len(perm) + n_bad == len(model_id)
    return counts, offsets, perm, n_bad


def state_to_proj(state_bits, n_pair):
    return ((np.asarray(state_bits).astype(np.uint32)[:, None] >> np.arange(n_pair, dtype=np.uint32)) & 1).astype(bool)


def proj_to_state(proj):
    return (proj.astype(np.uint32) << np.arange(proj.shape[1], dtype=np.uint32)).sum(1).astype(np.uint32)


def dexpilot_keys(prob, keypoints, state_bits):
    """The oracle's own projection pre-amble (prob.dexpilot_preamble on cases.ref_from_keypoints) on (B, 21, 3) keypoints
    and (B,) incoming projection bits -> key (B,) int, new_bits (B,) uint32, near (B,) bool.
    key: 0 a projection bit changes in this frame, 1 none changes and some projection is active, 2 neither.
    near: a pair-row length, formed in float64, lies within NEAR_BAND of a threshold -- the only frames on which a
    float32 length formed in another order of operations may legitimately fall on the other side."""
    state_bits = np.asarray(state_bits).astype(np.uint32)
    ref = cases.ref_from_keypoints(prob, np.asarray(keypoints))
    _, _, proj = prob.dexpilot_preamble(ref, state_to_proj(state_bits, prob.n_pair))
    new_bits = proj_to_state(proj)
    key = np.where(new_bits != state_bits, 0, np.where(new_bits != 0, 1, 2)).astype(np.int32)
    dist = np.linalg.norm(ref[:, : prob.n_pair].astype(np.float64), axis=2)
    near = np.zeros(len(state_bits), bool)
    for thr in KEY_THRESHOLDS:
        near |= (np.abs(dist - thr) <= NEAR_BAND).any(1)
    return key, new_bits, near


def seq_compose(kind, idx, mult, off, qraw, fixed, alpha, filt, first):
    """seq_retarget.py:125-133 for T frames of B sequences, frame after frame in float64: robot_qpos = zeros, the fixed
    joints, the target joints, the mimic joints from the composed vector (kinematics_adaptor.py:102-105), LPFilter.next
    (optimizer_utils.py:7-13).
    kind / idx / mult / off: the dof map of dexr_seq_compose_dev (0 target, 1 fixed, 2 mimic of dof idx);
    qraw (T, B, n_opt) float32; fixed (T, B, n_fixed) float32 or None; alpha in [0, 1] or anything else for no filter;
    filt (B, n_q) float64 carried filter output or None; first: the filters have not seen a frame yet.
    Returns (out (T, B, n_q) float64, new filter state (B, n_q) float64 or None when filt is None)."""
    kind, idx = np.asarray(kind), np.asarray(idx)
    mult, off = np.asarray(mult, dtype=np.float64), np.asarray(off, dtype=np.float64)
    qraw = np.asarray(qraw)
    T, B = qraw.shape[:2]
    n_q = len(kind)
    tgt, fix, mim = np.flatnonzero(kind == 0), np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
    use_filter = 0.0 <= alpha <= 1.0
    y = None if filt is None else np.array(filt, dtype=np.float64, copy=True)
    is_init = not first
    out = np.zeros((T, B, n_q))
    for t in range(T):
        q = np.zeros((B, n_q))
        if len(fix):
            q[:, fix] = np.asarray(fixed)[t][:, idx[fix]].astype(np.float64)
        q[:, tgt] = qraw[t][:, idx[tgt]].astype(np.float64)
        if len(mim):
            q[:, mim] = q[:, idx[mim]] * mult[mim] + off[mim]
        if use_filter:
            if not is_init:
                y = q.copy()
                is_init = True
            else:
                y = y + alpha * (q - y)
            q = y.copy()
        out[t] = q
    return out, y

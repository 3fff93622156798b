"""White-box GPU tests of the fleet bucketing and hard-frames-first ordering kernels (dexr_aux.hip: fleet_count_kernel,
fleet_offsets_kernel, fleet_scatter_kernel, fleet_segment_key_kernel, fleet_segment_gather_kernel).

dexr_retarget_multi_dev works in a caller-supplied workspace (MixedFleet._ws, a torch tensor), so what those kernels
write can be read back after a call and compared with plain numpy (tests/aux_reference.py): the counts, the bucket
offsets, the count of unknown ids, the index list itself (a STABLE partition: every model's frames in batch order), and
for a DexPilot bucket the key of every frame and the ordered index list.  The workspace layout lives in `Workspace` alone.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import aux_reference as ar
from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases
from test_aux_host import ordering_inputs

pytestmark = pytest.mark.gpu
RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))

MAX_MODELS = 16                     # DEXR_FLEET_MAX_MODELS (include/dexr.h)
SENTINEL = np.float32(-12345.678)   # no joint angle
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
LIGHT = ["teleop/allegro_hand_right.yml", "teleop/ability_hand_right.yml", "teleop/allegro_hand_left.yml",
         "teleop/ability_hand_left.yml"]
SHADOW = "teleop/shadow_hand_right_dexpilot.yml"


@pytest.fixture(scope="module", autouse=True)
def _gpu(require_gpu):
    yield


def build_optimizer(rel):
    return RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer


class Workspace:
    """The int32 words of a fleet workspace after a call on B frames (dexr_aux.hip, "workspace layout"): the bucketing
    workspace of W words and its index list, then what ordering one DexPilot bucket needs -- its keys, a second bucketing
    workspace with its list of POSITIONS, the ordered index list and its (offset, count) pair."""

    def __init__(self, ws_bytes_tensor, B):
        base = _lib.fleet_workspace_bytes(0)
        assert base % 4 == 0 and (base // 4 - 4) % 2 == 0
        assert _lib.fleet_workspace_bytes(B) - base == 16 * B
        W = self.W = (base // 4 - 4) // 2  # 2 W + 4 words without a frame
        w = self.words = ws_bytes_tensor[: _lib.fleet_workspace_bytes(B)].view(np.int32)
        self.B = B
        self.counts, self.bucket, self.bad = w[0:MAX_MODELS], w[32:32 + 2 * MAX_MODELS], int(w[64])
        self.perm = w[W:W + B]
        self.key = w[W + B:W + 2 * B]
        second = w[W + 2 * B:]
        self.counts2, self.bucket2, self.bad2 = second[0:MAX_MODELS], second[32:32 + 2 * MAX_MODELS], int(second[64])
        self.perm2 = w[2 * W + 2 * B:2 * W + 3 * B]
        self.operm = w[2 * W + 3 * B:2 * W + 4 * B]
        self.oseg = w[2 * W + 4 * B:2 * W + 4 * B + 2]


def run_fleet(torch, fleet, mid, kp, last, state=None, prefill=None):
    """One MixedFleet.retarget call on a sentinel-filled `out` -> (out, state, workspace bytes) as numpy arrays."""
    B = len(mid)
    if prefill is not None:
        fleet._ws = torch.full((_lib.fleet_workspace_bytes(B),), prefill, dtype=torch.uint8, device="cuda")
    out = torch.full((B, fleet.n_max), float(SENTINEL), dtype=torch.float32, device="cuda")
    st = None if state is None else torch.from_numpy(state.astype(np.int32)).cuda()
    fleet.retarget(mid, kp, last, st, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if st is None else st.cpu().numpy().astype(np.uint32), fleet._ws.cpu().numpy()


# ---- a. the partition ---------------------------------------------------------------------------------------------------
_light = []


def light_fleet(n):
    """n SEPARATELY built light models (register family, no DexPilot state, nothing forked to internal streams)."""
    from dex_retargeting_amd.fleet import MixedFleet

    while len(_light) < n:
        _light.append(build_optimizer(LIGHT[len(_light) % len(LIGHT)]))
    fleet = MixedFleet(_light[:n])
    for m in fleet.models:
        assert m.kernel()[0] in (_lib.KERNEL_REGISTER, _lib.KERNEL_REGISTER_CHAIN)
    return fleet


# wave (64), sweep (256) and chunk (2 048, or 2 304 for the largest batch) boundaries, first and last frame
EDGES = (0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2303, 2304, 2305, 4095, 4096)
BAD_IDS = (-1, None, 16, 17, INT32_MIN, INT32_MAX)  # None: n_models, the first id that is not a model


def id_patterns(B, N, seed):
    rng = np.random.default_rng(seed)
    b = np.arange(B, dtype=np.int64)
    pats = {"uniform": rng.integers(0, N, B), "one_model": np.full(B, N - 1), "sorted_runs": np.sort(rng.integers(0, N, B)),
            "b_mod_n": b % N, "wave_aligned": (b // 64) % N}
    bad_vals = np.array([N if v is None else v for v in BAD_IDS], dtype=np.int64)
    mixed = rng.integers(0, N, B)
    where = np.unique(np.concatenate([rng.integers(0, B, max(1, B // 10)), [e for e in EDGES if e < B], [B - 1]]))
    mixed[where] = bad_vals[np.arange(len(where)) % len(bad_vals)]
    assert np.all((mixed[where] < 0) | (mixed[where] >= N))
    pats["with_bad_ids"] = mixed
    return {k: v.astype(np.int32) for k, v in pats.items()}


def check_partition(ws, out, mid, fleet, label):
    N = len(fleet.models)
    counts, offsets, perm, n_bad = ar.fleet_partition(mid, N)
    assert np.array_equal(ws.counts[:N], counts), label
    assert np.array_equal(ws.bucket[0:2 * N:2], offsets), label
    assert np.array_equal(ws.bucket[1:2 * N:2], counts), label
    assert ws.bad == n_bad, label
    for m in range(N):  # segment by segment, so that a failure names the model
        seg = slice(int(offsets[m]), int(offsets[m] + counts[m]))
        assert np.array_equal(ws.perm[seg], perm[seg]), (label, m)
    bits, sent = out.view(np.int32), SENTINEL.view(np.int32)
    valid = (mid >= 0) & (mid < N)
    assert np.all(bits[~valid] == sent), label  # unknown ids: rows left untouched
    n_opt = np.array(fleet.n_opt)[np.where(valid, mid, 0)]
    answer = valid[:, None] & (np.arange(fleet.n_max)[None] < n_opt[:, None])
    assert np.all(bits[answer] != sent) and np.all(np.isfinite(out[answer])), label  # every answer written ...
    assert np.all(bits[~answer] == sent), label                                      # ... and nothing else


def partition_case(torch, N, B, patterns=None):
    fleet = light_fleet(N)
    kp_small = torch.from_numpy(cases.human_keypoints(512, seed=9)).cuda()
    kp = kp_small.repeat((B + 511) // 512, 1, 1)[:B].contiguous()  # a small human set, tiled on the device
    last = torch.zeros((B, fleet.n_max), dtype=torch.float32, device="cuda")
    pats = id_patterns(B, N, seed=1000 * N + B % 997)
    for name in patterns or pats:
        mid_np = pats[name]
        mid = torch.from_numpy(mid_np).cuda()
        label = (N, B, name)
        runs = [run_fleet(torch, fleet, mid, kp, last, prefill=pf) for pf in (None, None, 0x7f)]
        ws = Workspace(runs[0][2], B)
        check_partition(ws, runs[0][0], mid_np, fleet, label)
        n_valid = int(ws.counts[:N].sum())
        for out_r, _, ws_r in runs[1:]:  # the same call again, and in a workspace full of 0x7f: the same result ...
            w = Workspace(ws_r, B)
            assert np.array_equal(out_r.view(np.int32), runs[0][0].view(np.int32)), label
            assert np.array_equal(w.perm[:n_valid], ws.perm[:n_valid]), label
            assert np.array_equal(w.counts[:N], ws.counts[:N]) and np.array_equal(w.bucket[:2 * N], ws.bucket[:2 * N]), label
            assert w.bad == ws.bad, label  # ... and the count of unknown ids does not accumulate
        del mid, runs
    del kp, last, fleet


SMALL_B = [1, 255, 256, 257, 2047, 2048, 2049, 32769, 40000]


@pytest.mark.parametrize("B", SMALL_B)
@pytest.mark.parametrize("N", [1, 3, 16])
def test_fleet_bucketing_is_a_stable_partition(N, B):
    """counts, bucket, bad and every model's index-list segment equal the numpy stable partition; rows of unknown ids keep
    the sentinel and every valid row is solved.  Batch sizes: the 2 048-frame chunk edge and the 256-frame sweep edge,
    32 769 (17 blocks: the first size at which fleet_offsets_kernel sums more than one block per group), 40 000; id
    patterns: see id_patterns.  Every pattern runs twice, then once more in a workspace prefilled with 0x7f bytes."""
    torch = pytest.importorskip("torch")
    partition_case(torch, N, B)


@pytest.mark.parametrize("B", [2097152, 2097153])
def test_fleet_bucketing_at_the_block_table_limit(B):
    """2 097 152 frames: 1 024 blocks of 2 048, the whole per-block table (64 blocks per group in fleet_offsets_kernel);
    one frame more: the first chunk other than 2 048 (2 304 frames, 911 blocks, the last one ragged).  The smallest
    batches that reach those two states; 16 models, ids with unknown ones mixed in and sorted runs."""
    torch = pytest.importorskip("torch")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    partition_case(torch, 16, B, patterns=("with_bad_ids", "sorted_runs"))
    torch.cuda.synchronize()
    print(f"fleet bucketing B={B}: {time.perf_counter() - t0:.1f} s wall")
    torch.cuda.empty_cache()


# ---- b. hard frames first -----------------------------------------------------------------------------------------------
_ordered = {}


def ordered_fleet():
    from dex_retargeting_amd.fleet import MixedFleet

    if not _ordered:
        _ordered["opts"] = [build_optimizer(LIGHT[0]), build_optimizer(SHADOW)]  # the DexPilot bucket starts at an offset
        _ordered["prob"] = cases.problem_from_config(SHADOW)
    return MixedFleet(_ordered["opts"]), _ordered["opts"], _ordered["prob"]


@pytest.mark.parametrize("B", [6000, 40000])
def test_fleet_orders_the_dexpilot_bucket_hard_frames_first(B):
    """Allegro + Shadow DexPilot with longest_first = 2, ~45 % of the ids each and ~10 % unknown; frames and incoming
    projection bits as checked on the CPU (test_aux_host.py).  In the workspace after the call: the key of every position
    of the Shadow bucket equals the numpy pre-amble's key of that frame (but on the few frames with a length within 1e-6 m
    of a threshold, where the device's float32 length may fall on the other side), -1 beyond the bucket; the ordered list
    is the three key classes in key order, each in bucket order; (offset, count) = (0, bucket size).  The schedule changes
    nothing else: answers and returned bits equal the longest_first = 0 run bit for bit, and the bits equal the pre-amble's.
    B = 6 000: three blocks in both bucketing passes, the bucket ends inside the second; B = 40 000: 20 blocks."""
    torch = pytest.importorskip("torch")
    fleet, opts, prob = ordered_fleet()
    shadow = opts[1].device_model()
    assert shadow.kernel()[0] == _lib.KERNEL_WIDE
    kp_np, bits_in = ordering_inputs(prob, B)
    want_key, want_bits, near = ar.dexpilot_keys(prob, kp_np, bits_in)
    rng = np.random.default_rng(B)
    mid_np = rng.choice(np.array([0, 1, 2, -1, 17, INT32_MAX], np.int64), B, p=[0.45, 0.45, 0.04, 0.03, 0.02, 0.01]).astype(np.int32)
    is_shadow = mid_np == 1
    state_in = np.where(is_shadow, bits_in, 0).astype(np.uint32)  # frames of other models carry no bits
    last_np = np.zeros((B, fleet.n_max), np.float32)
    for m, o in enumerate(opts):
        lim = np.asarray(o.robot.joint_limits)[o.idx_pin2target]
        last_np[mid_np == m, : o.opt_dof] = lim.mean(1).astype(np.float32)
    mid, kp, last = (torch.from_numpy(a).cuda() for a in (mid_np, kp_np, last_np))
    before = shadow.get_tuning().longest_first
    try:
        shadow.tune(longest_first=2)
        out, state, ws_bytes = run_fleet(torch, fleet, mid, kp, last, state=state_in, prefill=0x7f)
        shadow.tune(longest_first=0)
        out0, state0, ws0_bytes = run_fleet(torch, fleet, mid, kp, last, state=state_in, prefill=0x7f)
    finally:
        shadow.tune(longest_first=before)
    ws, ws0 = Workspace(ws_bytes, B), Workspace(ws0_bytes, B)
    # the first pass, as in the partition tests
    counts, offsets, perm, n_bad = ar.fleet_partition(mid_np, 2)
    assert np.array_equal(ws.counts[:2], counts) and ws.bad == n_bad and np.array_equal(ws.perm[: len(perm)], perm)
    off, cnt = int(ws.bucket[2]), int(ws.bucket[3])
    assert (off, cnt) == (int(offsets[1]), int(counts[1])) and 0.4 * B < cnt < 0.5 * B
    frames = ws.perm[off:off + cnt]
    assert np.array_equal(frames, np.flatnonzero(is_shadow))
    # without the ordering nothing below is written: the prefill is still there
    filler = np.int32(0x7f7f7f7f)
    assert np.all(ws0.key == filler) and np.all(ws0.operm == filler) and np.all(ws0.oseg == filler)
    # keys
    key = ws.key
    assert np.all(key[cnt:] == -1)
    assert np.all((key[:cnt] >= 0) & (key[:cnt] <= 2))
    differs = key[:cnt] != want_key[frames]
    seen = np.bincount(key[:cnt], minlength=3)
    print(f"B={B}: bucket of {cnt}, device keys {seen.tolist()}, near a threshold {int(near[frames].sum())} "
          f"({near[frames].mean():.5f}), keys differing there {int(differs.sum())}")
    assert np.all(seen > 0)
    assert not np.any(differs & ~near[frames]), np.flatnonzero(differs & ~near[frames])[:10]
    # the second bucketing pass sorts the POSITIONS by key, stably; positions beyond the bucket are its unknown ids
    assert np.array_equal(ws.counts2[:3], seen) and ws.bad2 == B - cnt
    assert np.array_equal(ws.bucket2[0:6:2], np.concatenate([[0], np.cumsum(seen)[:-1]]))
    pos_sorted = np.concatenate([np.flatnonzero(key[:cnt] == k) for k in range(3)])
    assert np.array_equal(ws.perm2[:cnt], pos_sorted)
    # the ordered list: hard frames first, every class in bucket order (from the device's own keys: exact)
    assert np.array_equal(ws.operm[:cnt], frames[pos_sorted])
    assert ws.oseg.tolist() == [0, cnt]
    # the returned bits, and what the schedule must not change
    ok = is_shadow & ~near
    assert np.array_equal(state[ok], want_bits[ok])
    assert np.all(state[~is_shadow] == 0)
    assert np.array_equal(state, state0)
    assert np.array_equal(out.view(np.int32), out0.view(np.int32))
    bits, sent = out.view(np.int32), SENTINEL.view(np.int32)
    assert np.all(bits[is_shadow][:, : opts[1].opt_dof] != sent) and np.all(bits[(mid_np < 0) | (mid_np > 1)] == sent)


# ---- c. refusals --------------------------------------------------------------------------------------------------------
def test_fleet_entry_point_refuses_bad_arguments():
    """dexr_retarget_multi_dev with real handles and real device buffers: each malformed call raises DexrError with the
    message of ITS check, and writes nothing."""
    torch = pytest.importorskip("torch")
    fleet, opts, prob = ordered_fleet()  # models[1] is a DexPilot model
    B = 300
    handles = [m.handle for m in fleet.models]
    mid = torch.from_numpy((np.arange(B) % 2).astype(np.int32)).cuda()
    kp = torch.from_numpy(cases.human_keypoints(B, seed=9)).cuda()
    last = torch.zeros((B, fleet.n_max), dtype=torch.float32, device="cuda")
    state = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = torch.full((B, fleet.n_max), float(SENTINEL), dtype=torch.float32, device="cuda")
    need = _lib.fleet_workspace_bytes(B)
    ws = torch.full((need,), 0x7f, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(models=handles, n_models=None, B=B, state_ptr=state.data_ptr(), ld=fleet.n_max, ws_bytes=need, precision=0):
        arr = (C.c_void_p * max(len(models), 1))(*models)
        opt = _lib.default_options(precision=precision)
        _lib.check(_lib.load().dexr_retarget_multi_dev(arr, len(models) if n_models is None else n_models, B, mid.data_ptr(),
                                                       kp.data_ptr(), None, 0, last.data_ptr(), ld, state_ptr or None,
                                                       out.data_ptr(), None, C.byref(opt), ws.data_ptr(), ws_bytes, stream))

    n_opt = [o.opt_dof for o in opts]
    refusals = [
        (dict(n_models=0), r"n_models=0 outside 1\.\.16"),
        (dict(models=(handles * 9)[:17]), r"n_models=17 outside 1\.\.16"),
        (dict(B=-1), "negative batch"),
        (dict(ws_bytes=need - 1), rf"workspace of {need - 1} B, {need} B needed"),
        (dict(precision=1), "fleet batches run the float32"),
        (dict(models=[handles[0], None]), r"models\[1\] is NULL"),
        (dict(state_ptr=0), r"models\[1\] is a DexPilot model but state is NULL"),
        (dict(ld=n_opt[1] - 1), rf"models\[1\] optimises {n_opt[1]} joints but rows are {n_opt[1] - 1} long"),
        (dict(ld=n_opt[0] - 1), rf"models\[0\] optimises {n_opt[0]} joints but rows are {n_opt[0] - 1} long"),
    ]
    for kw, message in refusals:
        with pytest.raises(_lib.DexrError, match=message):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == float(SENTINEL)).all()) and bool((ws == 0x7f).all()) and int(state.abs().sum()) == 0
    call()  # the well-formed call on the same buffers goes through
    torch.cuda.synchronize()
    assert bool((out[:, : min(n_opt)] != float(SENTINEL)).all())

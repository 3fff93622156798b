"""GPU: the float64 instantiation of the sixteen-lane kernel (dexr_tuning.kernel_f64 = DEXR_KERNEL_WIDE; Optimizer.f64_kernel).

  * the tuning contract: which values are accepted, which handles refuse WIDE, what dexr_model_kernel_f64 reports;
  * nothing else changes: float32 answers with and without the opt-in, and the float64 answers of an untouched handle;
  * parity against the float64 oracle on every shipped config the kernel serves (4 096 frames each, the tracking protocol of
    test_gpu_all_configs: frame b starts from the answer for frame b - 1, DexPilot bits carried), measured ceilings in
    tests/golden/parity_ceilings_f64_wide.json;
  * agreement with the register kernel's float64 rows;
  * a frame's float64 answer depends on its inputs alone -- not on the batch size, its row or the split of the batch;
  * fused sequences equal frame-by-frame float64 calls, bit for bit.
The per-config table and the measured counts are written to build/reports/ (f64_wide_parity.txt,
parity_ceilings_f64_wide_measured.json)."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest

import oracle_jobs
from testutil import REPO
from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases

pytestmark = pytest.mark.gpu
RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))
ALL = sorted(os.path.relpath(p, cases.CONFIG_DIR) for p in glob.glob(os.path.join(cases.CONFIG_DIR, "*", "*.yml")))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CEILINGS = json.load(open(os.path.join(GOLDEN, "parity_ceilings_f64_wide.json")))
CEILINGS_F32 = json.load(open(os.path.join(GOLDEN, "parity_ceilings.json")))
TOL = 1e-4
SHADOW_DP = "teleop/shadow_hand_right_dexpilot.yml"
LEAP_POS = "offline/leap_hand_right.yml"
SVH_DP = "teleop/schunk_svh_hand_right_dexpilot.yml"
SVH_VEC = "teleop/schunk_svh_hand_right.yml"
INSPIRE_DP = "teleop/inspire_hand_right_dexpilot.yml"
ERR_INVALID, ERR_UNSUPPORTED = -1, -3


def _optimizer(rel, f64_kernel=None, generic=False):
    opt = RetargetingConfig.load_from_file(os.path.join(cases.CONFIG_DIR, rel)).build().optimizer
    opt.use_generic_tables = generic
    opt.f64_kernel = f64_kernel
    return opt


def _wide_ok(model):
    n = ctypes.c_int32()
    return _lib.load().dexr_model_lane_plan(model._h, 0, ctypes.byref(n), None, None, None) == 0


def _set_kernel_f64(model, value):
    """raw return code of dexr_model_set_tuning with kernel_f64 = value"""
    t = model.get_tuning()
    t.kernel_f64 = value
    return _lib.load().dexr_model_set_tuning(model._h, ctypes.byref(t))


def _inputs(rel, n, seed=cases.SEED):
    """The tracking protocol of test_gpu_all_configs._gpu_solve: keypoints of n + 1 frames; frame b's regularisation target
    and start point is the (float32, default-handle) answer for frame b - 1, started from the middle of the joint range; the
    DexPilot bits are carried from that solve."""
    prob = cases.problem_from_config(rel)
    model = _optimizer(rel).device_model()
    kp = cases.human_keypoints(n + 1, seed=seed)
    mid = np.repeat(prob.joint_limits.mean(1)[None], n, 0).astype(np.float32)
    st = np.zeros(n, np.uint32) if prob.kind == "dexpilot" else None
    last = model.retarget(np.ascontiguousarray(kp[:-1]), None, mid, state=st, keypoints=True)
    ref = np.ascontiguousarray(cases.ref_from_keypoints(prob, kp[1:]), dtype=np.float32)
    return dict(prob=prob, ref=ref, last=last, st=st, kp=kp)


def _solve64(model, d, sl=slice(None), perm=None):
    idx = np.arange(len(d["last"]))[sl]
    if perm is not None:
        idx = idx[perm]
    st = None if d["st"] is None else d["st"][idx].copy()
    q, info = model.retarget_f64(d["ref"][idx], None, d["last"][idx], state=st, want_info=True)
    return q, info, st


# ---- 3. tuning contract -------------------------------------------------------------------------------------------------
def test_kernel_f64_tuning_contract(require_gpu):
    for rel in (SHADOW_DP, LEAP_POS, SVH_DP):
        m = _optimizer(rel).device_model()
        assert m.get_tuning().kernel_f64 == _lib.KERNEL_AUTO
        assert m.kernel_f64()[0] == _lib.KERNEL_REGISTER
        m.tune(kernel_f64=_lib.KERNEL_REGISTER)
        assert m.kernel_f64()[0] == _lib.KERNEL_REGISTER
        m.tune(kernel_f64=_lib.KERNEL_WIDE)
        fam, bucket = m.kernel_f64()
        assert fam == _lib.KERNEL_WIDE and bucket in (16, 24), (rel, fam, bucket)
        assert m.kernel()[0] == _lib.KERNEL_WIDE  # the float32 selection is untouched
        for bad in (1, 2, 3, 7):
            assert _set_kernel_f64(m, bad) == ERR_INVALID, (rel, bad)
        assert m.get_tuning().kernel_f64 == _lib.KERNEL_WIDE
        m.tune(kernel_f64=_lib.KERNEL_AUTO)
        assert m.kernel_f64()[0] == _lib.KERNEL_REGISTER
    # handles the sixteen-lane kernel does not serve: refused, tuning unchanged
    m = _optimizer("teleop/allegro_hand_right.yml").device_model()
    assert m.kernel()[1] == 4 and not _wide_ok(m)
    assert _set_kernel_f64(m, _lib.KERNEL_WIDE) == ERR_UNSUPPORTED
    assert m.get_tuning().kernel_f64 == _lib.KERNEL_AUTO and m.kernel_f64()[0] == _lib.KERNEL_REGISTER
    g = _optimizer(SHADOW_DP, generic=True).device_model()
    assert g.kernel()[0] == _lib.KERNEL_GENERAL
    assert _set_kernel_f64(g, _lib.KERNEL_WIDE) == ERR_UNSUPPORTED
    assert g.get_tuning().kernel_f64 == _lib.KERNEL_AUTO and g.kernel_f64()[0] == _lib.KERNEL_GENERAL
    # the Python opt-in survives a rebuilt handle
    opt = _optimizer(SHADOW_DP, f64_kernel="wide")
    assert opt.device_model().kernel_f64()[0] == _lib.KERNEL_WIDE
    opt.set_joint_limit(np.stack([opt._lower + 1e-3, opt._upper - 1e-3], 1))
    assert opt._model is None
    assert opt.device_model().kernel_f64()[0] == _lib.KERNEL_WIDE
    opt.f64_kernel = None
    assert opt.device_model().kernel_f64()[0] == _lib.KERNEL_REGISTER


# ---- 4. no existing behaviour changes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rel,n", [(SHADOW_DP, 4096), (SHADOW_DP, 2048), (SVH_VEC, 2048)])
def test_float32_answers_unchanged_by_the_opt_in(require_gpu, rel, n):
    prob = cases.problem_from_config(rel)
    kp = np.ascontiguousarray(cases.human_keypoints(n, seed=11))
    last = np.repeat(prob.joint_limits.mean(1)[None], n, 0).astype(np.float32)
    out = []
    for k64 in (None, "wide"):
        m = _optimizer(rel, f64_kernel=k64).device_model()
        st = np.zeros(n, np.uint32) if prob.kind == "dexpilot" else None
        q, info = m.retarget(kp, None, last, state=st, keypoints=True, want_info=True)
        out.append((q, info, st))
    (qa, ia, sa), (qb, ib, sb) = out
    assert np.array_equal(qa, qb)
    for k in ("status", "iters", "fval"):
        assert np.array_equal(ia[k], ib[k]), k
    if sa is not None:
        assert np.array_equal(sa, sb)


def test_precision1_of_an_untouched_handle_is_the_register_kernel(require_gpu):
    d = _inputs(SHADOW_DP, 1024)
    a = _optimizer(SHADOW_DP).device_model()
    b = _optimizer(SHADOW_DP).device_model()
    b.tune(kernel_f64=_lib.KERNEL_REGISTER)
    opts = _lib.default_options(precision=1)
    qs = []
    for m in (a, b):
        st = None if d["st"] is None else d["st"].copy()
        qs.append(m.retarget(d["ref"], None, d["last"], state=st, opts=opts))
        qs.append(m.retarget_f64(d["ref"], None, d["last"], state=None if d["st"] is None else d["st"].copy()))
    assert np.array_equal(qs[0], qs[2]) and np.array_equal(qs[1], qs[3])


# ---- 5. parity against the float64 oracle -------------------------------------------------------------------------------
def _parity_row(rel, n=4096):
    opt = _optimizer(rel)
    m = opt.device_model()
    if not _wide_ok(m):
        return None
    if _set_kernel_f64(m, _lib.KERNEL_WIDE) != 0:
        return dict(unsupported=True)
    d = _inputs(rel, n)
    st_in = None if d["st"] is None else d["st"].copy()
    q, info, _ = _solve64(m, d)
    return dict(unsupported=False, d=d, st_in=st_in, q=q, info=info, bucket=m.kernel_f64()[1])


@pytest.fixture(scope="module")
def parity(require_gpu):
    runs = {}
    for rel in ALL:
        r = _parity_row(rel)
        if r is not None:
            runs[rel] = r
    rows = {}
    with oracle_jobs.host_pool() as ex:
        live = [rel for rel in runs if not runs[rel]["unsupported"]]
        jobs = [(rel, slice(i, min(i + 512, 4096))) for rel in live for i in range(0, 4096, 512)]
        parts = list(ex.map(oracle_jobs.oracle_solve,
                            [(rel, runs[rel]["d"]["ref"][c], runs[rel]["d"]["last"][c],
                              None if runs[rel]["st_in"] is None else runs[rel]["st_in"][c], runs[rel]["q"][c]) for rel, c in jobs]))
        todo = []
        for rel in live:
            mine = [p for (r_, _), p in zip(jobs, parts) if r_ == rel]
            o = {k: np.concatenate([p[k] for p in mine]) for k in mine[0]}
            r = runs[rel]
            dq = np.abs(r["q"] - o["want"]).max(1)
            far = dq >= TOL
            worse = far & (o["F_gpu"] > o["F_want"] + 1e-10)
            rows[rel] = dict(dq=dq, far=far, worse=worse, status=r["info"]["status"], iters=r["info"]["iters"], bucket=r["bucket"])
            if far.any():
                sel = np.nonzero(far)[0]
                sel = sel[np.argsort(-dq[sel])][:64]
                todo.append((rel, sel, ex.submit(oracle_jobs.certify_local_minimum,
                                                 (rel, r["d"]["ref"][sel], r["d"]["last"][sel],
                                                  None if r["st_in"] is None else r["st_in"][sel], r["q"][sel]))))
        for rel, sel, fut in todo:
            rows[rel]["cert"] = (sel,) + tuple(fut.result())
    out = os.path.join(REPO, "build", "reports")  # (a build product: not in git)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "f64_wide_parity.txt"), "w") as f:
        f.write("# float64 sixteen-lane kernel (kernel_f64 = WIDE) vs the float64 oracle, 4 096 tracking frames per config\n")
        f.write(f"{'config':44s} {'grid':>4s} {'p50 dq':>9s} {'p99.9 dq':>9s} {'max dq':>9s} {'>=1e-4':>7s} {'worse':>6s} "
                f"{'cert moved':>10s} {'iters mean':>10s} {'max':>4s}\n")
        for rel in runs:
            if runs[rel]["unsupported"]:
                f.write(f"{rel:44s} not served (components of more than 24 joints)\n")
                continue
            w = rows[rel]
            f.write(f"{rel:44s} {w['bucket']:4d} {np.median(w['dq']):9.1e} {np.percentile(w['dq'], 99.9):9.1e} {w['dq'].max():9.1e} "
                    f"{int(w['far'].sum()):7d} {int(w['worse'].sum()):6d} {(w['cert'][1].max() if 'cert' in w else 0.0):10.1e} "
                    f"{w['iters'].mean():10.2f} {int(w['iters'].max()):4d}\n")
    json.dump({rel: {"far": int(w["far"].sum()), "worse": int(w["worse"].sum())} for rel, w in rows.items()},
              open(os.path.join(out, "parity_ceilings_f64_wide_measured.json"), "w"), indent=1)
    return runs, rows


def test_parity_covers_every_wide_config(parity):
    runs, rows = parity
    assert len(runs) >= 25, sorted(runs)
    for rel, r in runs.items():
        if r["unsupported"]:  # the 32-row joint grid has no float64 instantiation (dexr_launch.hpp)
            m = _optimizer(rel).device_model()
            assert not m.get_tuning().kernel_f64 == _lib.KERNEL_WIDE
            assert m.kernel()[1] == 32, rel
    assert set(rows) == set(CEILINGS), sorted(set(rows) ^ set(CEILINGS))


@pytest.mark.parametrize("rel", sorted(CEILINGS))
def test_parity_against_the_float64_oracle(parity, rel):
    w = parity[1][rel]
    assert (w["status"] != 2).all()
    n_far, n_worse = int(w["far"].sum()), int(w["worse"].sum())
    assert n_far <= CEILINGS[rel]["far"], (rel, n_far, np.sort(w["dq"])[-5:])
    assert n_worse <= CEILINGS[rel]["worse"], (rel, n_worse)
    assert n_worse <= CEILINGS_F32[rel]["worse"], (rel, n_worse, CEILINGS_F32[rel])
    if w["far"].any():
        sel, moved, dF = w["cert"]
        assert np.all(moved < TOL) and np.all(dF < 1e-7), (rel, moved.max(), dF.max())
    assert np.percentile(w["dq"][~w["far"]], 99.9) < 1e-5, (rel, np.percentile(w["dq"][~w["far"]], 99.9))


# ---- 6. agreement with the register kernel's float64 rows ---------------------------------------------------------------
@pytest.mark.parametrize("rel", [SHADOW_DP, LEAP_POS, INSPIRE_DP])
def test_wide_f64_agrees_with_register_f64(require_gpu, rel):
    d = _inputs(rel, 1024, seed=cases.SEED + 1)
    reg = _optimizer(rel).device_model()
    wide = _optimizer(rel, f64_kernel="wide").device_model()
    assert wide.kernel_f64()[0] == _lib.KERNEL_WIDE
    qr, ir, _ = _solve64(reg, d)
    qw, iw, _ = _solve64(wide, d)
    assert (iw["status"] != 2).all()
    dq = np.abs(qw - qr).max(1)
    diff = dq >= TOL
    assert np.percentile(dq[~diff], 99.9) < 1e-5, np.percentile(dq[~diff], 99.9)
    if diff.any():
        sel = np.nonzero(diff)[0][:64]
        moved, dF = oracle_jobs.certify_local_minimum((rel, d["ref"][sel], d["last"][sel],
                                                       None if d["st"] is None else d["st"][sel], qw[sel]))
        assert np.all(moved < TOL) and np.all(dF < 1e-7), (rel, int(diff.sum()), moved.max(), dF.max())


# ---- 7. shape invariance ------------------------------------------------------------------------------------------------
def test_answer_independent_of_batch_split_row_and_size(require_gpu):
    m = _optimizer(SHADOW_DP, f64_kernel="wide").device_model()
    d = _inputs(SHADOW_DP, 40000, seed=5)
    full, _, st_full = _solve64(m, d)  # 40 000 DexPilot frames: hard frames first (dexr_api.hip launch_wide)
    a, _, st_a = _solve64(m, d, slice(0, 20000))
    b, _, st_b = _solve64(m, d, slice(20000, 40000))
    assert np.array_equal(full, np.concatenate([a, b]))
    assert np.array_equal(st_full, np.concatenate([st_a, st_b]))
    perm = np.random.default_rng(3).permutation(4096)
    base, _, _ = _solve64(m, d, slice(0, 4096))
    qp, _, _ = _solve64(m, d, slice(0, 4096), perm=perm)
    back = np.empty_like(qp)
    back[perm] = qp
    assert np.array_equal(back, base)
    q2048, _, _ = _solve64(m, d, slice(0, 2048))
    assert np.array_equal(q2048, base[:2048])
    for i in (0, 777, 4095):
        q1, _, _ = _solve64(m, d, slice(i, i + 1))
        assert np.array_equal(q1, base[i:i + 1]), i


# ---- 8. sequences -------------------------------------------------------------------------------------------------------
def test_fused_sequence_equals_frame_by_frame_float64(require_gpu):
    torch = pytest.importorskip("torch")
    B, T = 256, 8
    m = _optimizer(SHADOW_DP, f64_kernel="wide").device_model()
    prob = cases.problem_from_config(SHADOW_DP)
    frames = torch.from_numpy(cases.human_keypoints(B * T, seed=9).reshape(T, B, 21, 3)).cuda().contiguous()
    last0 = torch.from_numpy(np.repeat(prob.joint_limits.mean(1)[None], B, 0).astype(np.float32)).cuda()
    n = last0.shape[1]
    opts = _lib.default_options(precision=1)
    # fused: T frames in one launch
    last_f = last0.clone()
    st_f = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    raw_f = torch.empty((T, B, n), dtype=torch.float32, device="cuda:0")
    m.retarget_seq_dev(B, T, frames.data_ptr(), 0, last_f.data_ptr(), st_f.data_ptr(), raw_f.data_ptr(), 0, 1e-3, opts)
    # frame by frame on the same handle: T launches of one frame each, last_qpos and the DexPilot bits carried
    last_s = last0.clone()
    st_s = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    raw_s = torch.empty((T, B, n), dtype=torch.float32, device="cuda:0")
    for t in range(T):
        fr = frames[t:t + 1].contiguous()
        m.retarget_seq_dev(B, 1, fr.data_ptr(), 0, last_s.data_ptr(), st_s.data_ptr(), raw_s[t].data_ptr(), 0, 1e-3, opts)
    torch.cuda.synchronize()
    assert torch.equal(raw_f, raw_s)
    assert torch.equal(last_f, last_s)
    assert torch.equal(st_f, st_s)

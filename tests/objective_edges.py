"""Shared inputs of tests/test_objective_edges_host.py (CPU) and tests/test_gpu_objective_edges.py (GPU): the objective at
NON-DEFAULT parameters, at the Huber kink and at the DexPilot thresholds.  Nothing here touches the GPU until a family
selector is called.

* parameter sets: every set is built twice from the same numbers -- the library's optimizer (RetargetingConfig overrides; for
  DexPilot huber_delta / norm_delta / eta1 / eta2 through the optimizer's constructor, which the config does not forward, like
  the reference) and an OracleProblem;
* kink inputs: evaluation points whose chosen residual row sits at huber_delta * (1 +- 2**-10);
* DexPilot threshold inputs: pair rows at project_dist / escape_dist * (1 +- 2**-12) and between the two, with seeded prior
  bits, as ref_value rows, as raw keypoints and as T = 3 sequences;
* family selectors: one per solve kernel family, each asserts through model.kernel() / model.kernel_f64() that the
  intended family serves the call.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from dex_retargeting_amd import _lib
from dex_retargeting_amd.constants import DEFAULT_URDF_DIR
from dex_retargeting_amd.retargeting_config import RetargetingConfig
from oracle import cases, solvers
from oracle.objectives import OracleProblem

RetargetingConfig.set_default_urdf_dir(str(DEFAULT_URDF_DIR))

B = 64
ALLEGRO, LEAP, SHADOW_DP, INSPIRE_DP, SVH = ("teleop/allegro_hand_right.yml", "offline/leap_hand_right.yml",
                                             "teleop/shadow_hand_right_dexpilot.yml", "teleop/inspire_hand_right_dexpilot.yml",
                                             "offline/schunk_svh_hand_right.yml")
CONFIGS = [ALLEGRO, LEAP, SHADOW_DP, INSPIRE_DP, SVH]
DEXPILOT_CONFIGS = [SHADOW_DP, INSPIRE_DP]
KIND = {ALLEGRO: "vector", LEAP: "position", SHADOW_DP: "dexpilot", INSPIRE_DP: "dexpilot", SVH: "position"}

# (family, config) pairs that family cannot serve, by name, with the reason; every other pair is tested
UNSERVED = {
    # the dedicated float32 tip kernel: per-finger vector models only (one term per 4-joint serial chain)
    ("tip32", LEAP): "position model", ("tip32", SHADOW_DP): "DexPilot model", ("tip32", INSPIRE_DP): "DexPilot model",
    ("tip32", SVH): "position model",
    # one frame per wave: models of ONE component (launch_wide_once: n_comp == 1)
    ("wide1", ALLEGRO): "four components",
    # the sixteen-lane kernel takes components of 5 to 32 joints: Allegro's four 4-joint fingers stay on the register kernel
    ("wide4", ALLEGRO): "4-joint components", ("wide64", ALLEGRO): "4-joint components",
    # reduced variables: at most 16 optimised variables per component
    ("reduced", ALLEGRO): "4-joint components: nothing to reduce", ("reduced", LEAP): "more than 16 variables in one component",
    ("reduced", SHADOW_DP): "more than 16 variables in one component",
}

# ---- parameter sets ---------------------------------------------------------------------------------------------------------------
# name -> list of (tag, parameters in the config's vocabulary); `kinds`: the objective kinds a set applies to
_DEXPILOT_SET = dict(project_dist=0.02, escape_dist=0.035, eta1=5e-3, eta2=1e-2, huber_delta=0.01, normal_delta=1e-3)
SETS = {
    "linear": dict(variants=[("linear", dict(huber_delta=2e-3))], kinds=("vector", "position", "dexpilot")),
    "quadratic": dict(variants=[("quadratic", dict(huber_delta=0.5))], kinds=("vector", "position", "dexpilot")),
    "stiff": dict(variants=[("stiff", dict(normal_delta=5e-2))], kinds=("vector", "position", "dexpilot")),
    "free": dict(variants=[("free", dict(normal_delta=0.0))], kinds=("vector", "position", "dexpilot")),
    "scaled": dict(variants=[("scaled0.7", dict(scaling_factor=0.7)), ("scaled1.6", dict(scaling_factor=1.6))],
                   kinds=("vector", "dexpilot")),
    "dexpilot": dict(variants=[("dexpilot", dict(_DEXPILOT_SET))], kinds=("dexpilot",)),
}


def variants(rel, sets=tuple(SETS)):
    """(tag, params) of every variant of `sets` that applies to config `rel`."""
    return [(tag, p) for s in sets if KIND[rel] in SETS[s]["kinds"] for tag, p in SETS[s]["variants"]]


ALL_CASES = [(rel, tag) for rel in CONFIGS for tag, _ in variants(rel)]
SOLVE_CASES = [(rel, tag) for rel in CONFIGS for tag, _ in variants(rel, [s for s in SETS if s != "free"])]  # part C
_PARAMS = {tag: p for s in SETS.values() for tag, p in s["variants"]}
# Pinched frames (pinch_tracking below): non-default eta1 / eta2 with thresholds wide enough that reachable poses project pairs of
# both stages.  Inspire's fingertips stay more than 0.04 m apart at every reachable pose, so its refs are shrunk by a larger
# scaling_factor (ref * scaling stays reachable).  (config -> tag, seed of the pose pool)
_PINCH_SET = dict(project_dist=0.03, escape_dist=0.045, eta1=5e-3, eta2=1e-2, huber_delta=0.01, normal_delta=1e-3)
_PARAMS.update({"pinch": _PINCH_SET, "pinch_s3": dict(_PINCH_SET, scaling_factor=3.0)})
PINCH = {SHADOW_DP: ("pinch", 0), INSPIRE_DP: ("pinch_s3", 6)}
_CTOR_ONLY = ("huber_delta", "normal_delta", "eta1", "eta2")  # DexPilot: not forwarded by the config


def build_optimizer(rel, tag):
    """A fresh SeqRetargeting of config `rel` at parameter variant `tag` (no GPU work until device_model()).
    The DexPilot branch mirrors RetargetingConfig._build_optimizer / build() (retargeting_config.py: the `dexpilot` case, the mimic
    adaptor and the LPFilter / SeqRetargeting lines) with the constructor keywords the config does not forward: keep the two in
    step."""
    params = _PARAMS[tag]
    path = os.path.join(cases.CONFIG_DIR, rel)
    if KIND[rel] != "dexpilot":
        return RetargetingConfig.load_from_file(path, dict(params)).build()
    from dex_retargeting_amd.kinematics_adaptor import MimicJointKinematicAdaptor
    from dex_retargeting_amd.optimizer import DexPilotOptimizer
    from dex_retargeting_amd.optimizer_utils import LPFilter
    from dex_retargeting_amd.retargeting_config import parse_mimic_joint
    from dex_retargeting_amd.robot_wrapper import RobotWrapper
    from dex_retargeting_amd.seq_retarget import SeqRetargeting

    cfg = RetargetingConfig.load_from_file(path, {k: v for k, v in params.items() if k not in _CTOR_ONLY})
    ctor = {("norm_delta" if k == "normal_delta" else k): v for k, v in params.items() if k in _CTOR_ONLY}
    robot = RobotWrapper(cfg.urdf_path)
    names = cfg.target_joint_names if cfg.target_joint_names is not None else robot.dof_joint_names
    opt = DexPilotOptimizer(robot, names, finger_tip_link_names=cfg.finger_tip_link_names, wrist_link_name=cfg.wrist_link_name,
                            target_link_human_indices=cfg.target_link_human_indices, scaling=cfg.scaling_factor,
                            project_dist=cfg.project_dist, escape_dist=cfg.escape_dist, **ctor)
    has_mimic, source, mimic, mult, off = parse_mimic_joint(robot)
    if has_mimic and not cfg.ignore_mimic_joint:
        opt.set_kinematic_adaptor(MimicJointKinematicAdaptor(robot, target_joint_names=names, source_joint_names=source,
                                                             mimic_joint_names=mimic, multipliers=mult, offsets=off))
    return SeqRetargeting(opt, has_joint_limits=cfg.has_joint_limits, lp_filter=LPFilter(cfg.low_pass_alpha))


@functools.lru_cache(maxsize=None)
def problem(rel, tag="default"):
    """The OracleProblem of config `rel` with the numbers of variant `tag` ("default": as shipped)."""
    params = {} if tag == "default" else _PARAMS[tag]
    if KIND[rel] != "dexpilot":
        return cases.problem_from_config(rel, **params)
    base = cases.problem_from_config(rel, **{k: v for k, v in params.items() if k not in _CTOR_ONLY})
    cfg = base.cfg
    p = OracleProblem(base.robot, "dexpilot", base.target_joint_names, wrist_link_name=cfg["wrist_link_name"],
                      finger_tip_link_names=cfg["finger_tip_link_names"], scaling=cfg.get("scaling_factor", 1.0),
                      project_dist=cfg.get("project_dist", 0.03), escape_dist=cfg.get("escape_dist", 0.05),
                      huber_delta=params.get("huber_delta"), norm_delta=params.get("normal_delta", 4e-3),
                      eta1=params.get("eta1", 1e-4), eta2=params.get("eta2", 3e-2), use_mimic=len(base.mimic) > 0,
                      has_joint_limits=base.has_joint_limits)
    p.cfg, p.low_pass_alpha = cfg, base.low_pass_alpha
    return p


_models = {}


def optimizer(rel, tag, generic=False):
    """Cached optimizer (one device handle each) of (config, variant); generic: compiled to the generic table format."""
    key = (rel, tag, generic)
    if key not in _models:
        opt = build_optimizer(rel, tag).optimizer
        opt.use_generic_tables = generic
        _models[key] = opt
    return _models[key]


# ---- bits -----------------------------------------------------------------------------------------------------------------------
def bits(proj):
    return (proj.astype(np.uint32) << np.arange(proj.shape[1], dtype=np.uint32)).sum(1).astype(np.uint32)


def unbits(state, n_pair):
    return ((np.asarray(state)[:, None] >> np.arange(n_pair, dtype=np.uint32)) & 1).astype(bool)


def dexpilot_kw(prob, ref, state_bits=None):
    """(weights / dexpilot_ref keywords of the oracle, projection state after the frame) -- ({}, None) for other kinds."""
    if prob.kind != "dexpilot":
        return {}, None
    proj0 = np.zeros((ref.shape[0], prob.n_pair), bool) if state_bits is None else unbits(state_bits, prob.n_pair)
    w, rv, st = prob.dexpilot_preamble(ref, proj0)
    return dict(weights=w, dexpilot_ref=rv), st


# ---- residuals, by the oracle -------------------------------------------------------------------------------------------------------
def residual_size(prob, x, ref, fixed, state_bits=None):
    """What smooth_l1 sees, float64: |residual| per row (B, n_ref) for vector / DexPilot, |residual| per coordinate
    (B, n_ref, 3) for position."""
    ref = np.asarray(ref)
    pos = prob.robot.link_positions(prob.full_qpos(x, fixed), prob.computed_links)
    if prob.kind == "position":
        return np.abs(pos - ref.astype(np.float64))
    vec = pos[:, prob.task_idx] - pos[:, prob.origin_idx]
    if prob.kind == "vector":
        tgt = (ref * ref.dtype.type(prob.scaling)).astype(np.float64)
    else:
        tgt = dexpilot_kw(prob, ref, state_bits)[0]["dexpilot_ref"]
    return np.linalg.norm(vec - tgt, axis=2)


# ---- kink inputs ------------------------------------------------------------------------------------------------------------------
KINK_EPS = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def kink_inputs(rel, tag, flip=False):
    """Frames of reachable_set(prob, B, 0.05) evaluated at x = last + 0.05 N(0, 1), with ONE ref row per frame moved along its
    residual's direction (float64, then rounded to float32) so that the residual smooth_l1 sees has size
    huber_delta * (1 + side * 2**-10): frame b carries term b mod n_ref, side +1 / -1 alternating per round over the terms
    (`flip` swaps the sides).  Position models apply smooth_l1 per coordinate: all three coordinates of the row are placed.
    A DexPilot pair row is only used while it stays unprojected (a projected row's target depends on its direction alone); where
    the move would project it the opposite direction is tried, and row[b] = -1 marks a frame left as it was.
    The LAST frame's ref rows are the float32-rounded FK values at x itself: residuals at rounding level (the zero-norm guard of
    the gradient).  Returns dict(ref, fixed, last, x, row (B,), side (B,))."""
    prob = problem(rel, tag)
    d = cases.reachable_set(prob, B, 0.05)
    lo, hi = prob.bounds
    x = np.clip(d["last"].astype(np.float64) + 0.05 * np.random.default_rng(41).standard_normal(d["last"].shape), lo, hi)
    pos = prob.robot.link_positions(prob.full_qpos(x, d["fixed"]), prob.computed_links)
    cur = pos if prob.kind == "position" else pos[:, prob.task_idx] - pos[:, prob.origin_idx]
    s = 1.0 if prob.kind == "position" else prob.scaling
    h = prob.huber_delta
    ref = d["ref"].astype(np.float64)
    row, side = np.full(B, -1), np.zeros(B, int)
    for b in range(B - 1):
        t = b % prob.n_ref
        sd = (1 if (b // prob.n_ref) % 2 == 0 else -1) * (-1 if flip else 1)
        size = h * (1 + sd * KINK_EPS)
        r = cur[b, t] - ref[b, t] * s
        step = np.where(r >= 0, 1.0, -1.0) * size if prob.kind == "position" else r / np.linalg.norm(r) * size
        for sign in (1.0, -1.0):
            cand = ref[b].copy()
            cand[t] = (cur[b, t] - sign * step) / s
            c32 = cand.astype(np.float32)
            if prob.kind == "dexpilot" and t < prob.n_pair and dexpilot_kw(prob, c32[None])[1][0, t]:
                continue
            ref[b], row[b], side[b] = cand, t, sd
            break
    ref[B - 1] = cur[B - 1] / s
    return dict(ref=np.ascontiguousarray(ref, dtype=np.float32), fixed=d["fixed"], last=d["last"], x=x, row=row, side=side)


# ---- DexPilot threshold inputs ------------------------------------------------------------------------------------------------------
THR_EPS = 2.0 ** -12
N_CLASS = 5  # below / above project_dist, between the thresholds, below / above escape_dist


def class_length(prob, c):
    p, e = prob.project_dist, prob.escape_dist
    return np.array([p * (1 - THR_EPS), p * (1 + THR_EPS), 0.5 * (p + e), e * (1 - THR_EPS), e * (1 + THR_EPS)])[c]


def _classes(rng, shape):
    """Length class and prior bit per pair row.  Not uniform: the cells where the non-default thresholds decide differently from
    the default ones (between the thresholds with the bit clear; past escape_dist with the bit set) are drawn more often, every
    cell often enough to occur."""
    cls = rng.choice(N_CLASS, size=shape, p=[0.1, 0.1, 0.35, 0.1, 0.35])
    likely = np.where(cls == 2, 0, np.where(cls == 4, 1, -1))
    prior = np.where((likely >= 0) & (rng.random(shape) < 0.8), likely, rng.integers(0, 2, shape))
    return cls, prior.astype(bool)


@functools.lru_cache(maxsize=None)
def threshold_rows(rel, tag="dexpilot"):
    """B ref_value frames (reachable_set's) whose EVERY pair row is rescaled (float64, then rounded to float32) to its class
    length; exact ties are left out on purpose -- the kernels hold the thresholds in float32, the oracle in float64, and a tie
    is decided by that rounding, not by the code under test.  Returns dict(ref, fixed, last, cls (B, n_pair), state (B,) uint32)."""
    prob = problem(rel, tag)
    d = cases.reachable_set(prob, B, 0.05)
    cls, prior = _classes(np.random.default_rng(43), (B, prob.n_pair))
    ref = d["ref"].astype(np.float64)
    pair = ref[:, :prob.n_pair]
    ref[:, :prob.n_pair] = pair / np.linalg.norm(pair, axis=2, keepdims=True) * class_length(prob, cls)[..., None]
    return dict(ref=np.ascontiguousarray(ref, dtype=np.float32), fixed=d["fixed"], last=d["last"], cls=cls, state=bits(prior))


def off_ties(prob, ref, skip=None):
    """(B,) bool: every pair row of the frame (but column skip[b]) keeps the 2**-12 relative margin to project_dist, escape_dist
    and the 0.03 m of the second-stage rule."""
    dist = np.linalg.norm(ref[:, :prob.n_pair].astype(np.float64), axis=2)
    ok = np.ones(dist.shape, bool)
    for thr in (prob.project_dist, prob.escape_dist, 0.03):
        ok &= np.abs(dist / thr - 1) > THR_EPS * (1 - 2.0 ** -8)  # (a placed row sits AT the margin, up to float32 rounding)
    if skip is not None:
        ok[np.arange(len(ok)), skip] = True
    return ok.all(1)


@functools.lru_cache(maxsize=None)
def threshold_keypoints(rel, tag="dexpilot"):
    """The same as raw (B, 21, 3) keypoints.  Several pairs share each fingertip, so per frame ONE pair is placed: tip(task) =
    tip(origin) + u L (u: the pair's own direction), pair and class walking round-robin over the candidate frames; a frame is
    kept only if every other pair keeps the 2**-12 margin.  Returns dict(kp, ref (the float32 rows the kernel forms), last, pair
    (B,), cls (B,), state (B,))."""
    prob = problem(rel, tag)
    idx = prob.target_link_human_indices
    cand = cases.human_keypoints(8 * B, seed=cases.SEED + 43)
    rng = np.random.default_rng(44)
    kps, pairs, clss = [], [], []
    for n in range(len(cand)):
        k = len(kps)
        p, c = k % prob.n_pair, (k // prob.n_pair) % N_CLASS
        kp = cand[n].astype(np.float64)
        v = kp[idx[1, p]] - kp[idx[0, p]]
        kp[idx[1, p]] = kp[idx[0, p]] + v / np.linalg.norm(v) * class_length(prob, c)
        kp = kp.astype(np.float32)
        if off_ties(prob, cases.ref_from_keypoints(prob, kp[None]), skip=np.array([p]))[0]:
            kps.append(kp), pairs.append(p), clss.append(c)
        if len(kps) == B:
            break
    assert len(kps) == B, "too few candidate frames keep the margin"
    kp = np.ascontiguousarray(np.stack(kps))
    last = np.repeat(prob.joint_limits.mean(1)[None], B, 0).astype(np.float32)
    return dict(kp=kp, ref=np.ascontiguousarray(cases.ref_from_keypoints(prob, kp), dtype=np.float32), last=last,
                pair=np.array(pairs), cls=np.array(clss), state=bits(rng.integers(0, 2, (B, prob.n_pair)).astype(bool)))


@functools.lru_cache(maxsize=None)
def threshold_sequences(rel, tag="dexpilot"):
    """T = 3 frames of B sequences of ref_value rows: the chosen pair (b mod n_pair) goes inside project_dist -> between the
    thresholds -> outside escape_dist in the even sequences and the reverse in the odd ones, so the bit of the middle frame is
    the CARRIED one; the other pair rows keep the classes of threshold_rows in all three frames.
    Returns dict(ref (3, B, n_ref, 3), last, pair (B,), state (B,))."""
    prob = problem(rel, tag)
    base = threshold_rows(rel, tag)
    ref = np.repeat(base["ref"][None].astype(np.float64), 3, 0)
    pair = np.arange(B) % prob.n_pair
    for b in range(B):
        walk = (0, 2, 4) if b % 2 == 0 else (4, 2, 0)
        for t, c in enumerate(walk):
            v = ref[t, b, pair[b]]
            ref[t, b, pair[b]] = v / np.linalg.norm(v) * class_length(prob, c)
    return dict(ref=np.ascontiguousarray(ref, dtype=np.float32), last=base["last"], pair=pair, state=base["state"].copy())


def oracle_bits(prob, ref, state_bits, dtype=np.float32):
    """The projection bits after one frame by the oracle, its distances computed in `dtype`."""
    return bits(prob.dexpilot_preamble(np.asarray(ref, dtype=dtype), unbits(state_bits, prob.n_pair))[2])


# ---- part C: tracking solves ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tracking(rel, tag):
    """reachable_set(prob, B, 0.05) of (config, variant) with the oracle's minimiser from the tracking starts (`want`).  Computed
    once, shared by the host and the GPU tests, read-only."""
    prob = problem(rel, tag)
    d = cases.reachable_set(prob, B, 0.05)
    kw, _ = dexpilot_kw(prob, d["ref"])
    want = solvers.solve_lm_batched(prob, d["ref"], d["fixed"], d["last"], newton=True, max_iter=100, **kw)
    for a in (want, d["ref"], d["fixed"], d["last"]):
        a.setflags(write=False)
    return dict(prob=prob, d=d, kw=kw, want=want)


def second_start(rel, tag):
    """... and the oracle's minimiser of the same frames from a second seeded start 0.05 rad away from the first."""
    return second_start_of(tracking(rel, tag))


@functools.lru_cache(maxsize=None)
def pinch_tracking(rel):
    """Part C's tracking frames project no pair at the `dexpilot` set (reachable fingertips are more than 0.02 m apart), so there
    eta1 / eta2 never reach a solve.  These frames do: from a pool of 4 096 reachable poses (tracking starts 0.05 rad away, prior
    bits clear, like part C) the first 16 whose refs project a second-stage pair and then the first 48 that project first-stage
    pairs only, at the PINCH parameters -- chosen by what the INPUTS project, never by how a solve went.  The pool's seed is the
    first for which the oracle's minimiser is unique on all 64 frames (test_objective_edges_host.py): pinches are bimodal on a few
    per cent of the poses (Inspire: the thumb pitch at either bound).  Same keys as tracking() plus `projected`."""
    tag, seed = PINCH[rel]
    prob = problem(rel, tag)
    pool = cases.reachable_set(prob, 4096, 0.05, seed=cases.SEED + seed)
    st = dexpilot_kw(prob, pool["ref"])[1]
    len_s1 = prob.num_fingers - 1
    second = st[:, len_s1:].any(1)
    sel = np.sort(np.concatenate([np.nonzero(second)[0][:16], np.nonzero(st[:, :len_s1].any(1) & ~second)[0]])[:B])
    assert len(sel) == B
    d = {k: np.ascontiguousarray(pool[k][sel]) for k in ("ref", "fixed", "last")}
    kw, st = dexpilot_kw(prob, d["ref"])
    want = solvers.solve_lm_batched(prob, d["ref"], d["fixed"], d["last"], newton=True, max_iter=100, **kw)
    for a in (want, d["ref"], d["fixed"], d["last"]):
        a.setflags(write=False)
    return dict(prob=prob, d=d, kw=kw, want=want, projected=st, tag=tag)


def second_start_of(t):
    """the oracle's minimiser of the frames of a tracking() record from a second seeded start 0.05 rad away"""
    prob, d = t["prob"], t["d"]
    lo, hi = prob.bounds
    x2 = np.clip(d["last"].astype(np.float64) + 0.05 * np.random.default_rng(47).standard_normal(d["last"].shape), lo, hi)
    return solvers.solve_lm_batched(prob, d["ref"], d["fixed"], d["last"], x0=x2, newton=True, max_iter=100, **t["kw"])


# ---- family selectors -------------------------------------------------------------------------------------------------------------
class Family:
    """One solve kernel family.  solver(rel, tag) returns solve(inp, fixed, last, state=None, keypoints=False) -> (B, n_opt)
    answers, which asserts through model.kernel() / model.kernel_f64() that the intended family serves the handle, makes the
    call and puts the handle's policy back; sequence(rel, tag) the same for the fused T-frame entry."""

    def __init__(self, name, tol, family, tune, f64=False, generic=False, device=False, sequences=True):
        self.name, self.tol, self.family, self.tune, self.f64 = name, tol, family, tune, f64
        self.generic, self.device, self.sequences = generic, device, sequences

    def serves(self, rel):
        return (self.name, rel) not in UNSERVED

    def _selected(self, rel, tag):
        """the handle, tuned to this family (DexrError where the family refuses the model)"""
        opt = optimizer(rel, tag, self.generic)
        model = opt.device_model()
        model.tune(**self.tune)
        got = model.kernel_f64()[0] if self.f64 else model.kernel()[0]
        assert got == self.family, f"{self.name} on {rel}: family {got} selected, {self.family} intended"
        if self.name == "wide1":  # one frame per wave: single-component models, batches up to sprint_max_batch (policy: 2 048)
            assert int(opt.compiled_model().header["n_comp"]) == 1
        if self.name == "tip32":  # the dedicated kernel: 4-joint chain with its tip pass
            assert model.kernel() == (_lib.KERNEL_REGISTER, 4, 2)
        return model

    @staticmethod
    def _restore(model):
        model.tune(kernel=_lib.KERNEL_AUTO, kernel_f64=_lib.KERNEL_AUTO, sprint_max_batch=-1)

    def solver(self, rel, tag, **solve_options):
        """solve_options: fields of dexr_solve_options to change (e.g. max_iter); none = the library's defaults"""
        def solve(inp, fixed, last, state=None, keypoints=False):
            model = self._selected(rel, tag)
            opts = _lib.default_options(**solve_options) if solve_options else None
            try:
                if self.device:
                    assert opts is None
                    return _solve_dev(model, inp, last, keypoints)
                if self.f64 and keypoints:  # (dexr_retarget_f64 takes ref rows only; the keypoint entry solves in float64 on request)
                    return model.retarget(inp, fixed, last, state=state, keypoints=True,
                                          opts=_lib.default_options(precision=1, **solve_options)).astype(np.float64)
                if self.f64:
                    return model.retarget_f64(inp, fixed, last, state=state, opts=opts)
                return model.retarget(inp, fixed, last, state=state, keypoints=keypoints, opts=opts).astype(np.float64)
            finally:
                self._restore(model)

        return solve

    def sequence(self, rel, tag):
        def solve_seq(ref_seq, last, state):
            """(T, B, n_ref, 3) ref_value rows -> state after the T frames (B,) uint32, through dexr_retarget_seq_dev"""
            import torch

            model = self._selected(rel, tag)
            try:
                dev = torch.device("cuda:0")
                T, nb = ref_seq.shape[:2]
                t_ref, t_last = torch.from_numpy(ref_seq).to(dev), torch.from_numpy(last.copy()).to(dev)
                t_state = torch.from_numpy(state.astype(np.int32)).to(dev)
                t_q = torch.zeros((T, nb, last.shape[1]), dtype=torch.float32, device=dev)
                model.retarget_seq_dev(nb, T, t_ref.data_ptr(), 0, t_last.data_ptr(), t_state.data_ptr(), t_q.data_ptr(),
                                       opts=_lib.default_options(precision=1) if self.f64 else None,
                                       stream=torch.cuda.current_stream().cuda_stream, keypoints=False)
                torch.cuda.synchronize()
                return t_state.cpu().numpy().astype(np.uint32)
            finally:
                self._restore(model)

        return solve_seq


def _solve_dev(model, inp, last, keypoints):
    """the device-pointer entry WITHOUT an fval pointer: the only call the dedicated float32 tip kernel serves"""
    import torch

    dev = torch.device("cuda:0")
    t_in, t_last = torch.from_numpy(np.ascontiguousarray(inp)).to(dev), torch.from_numpy(np.ascontiguousarray(last)).to(dev)
    t_q = torch.full(last.shape, float("nan"), dtype=torch.float32, device=dev)
    model.retarget_dev(last.shape[0], t_in.data_ptr(), 0, t_last.data_ptr(), 0, t_q.data_ptr(),
                       stream=torch.cuda.current_stream().cuda_stream, keypoints=keypoints)
    torch.cuda.synchronize()
    return t_q.cpu().numpy().astype(np.float64)


K = _lib
FAMILIES = [
    Family("register32", 1e-4, K.KERNEL_REGISTER, dict(kernel=K.KERNEL_REGISTER)),
    Family("register64", 1e-5, K.KERNEL_REGISTER, dict(kernel_f64=K.KERNEL_AUTO), f64=True),
    Family("wide4", 1e-4, K.KERNEL_WIDE, dict(kernel=K.KERNEL_WIDE, sprint_max_batch=0)),
    Family("wide1", 1e-4, K.KERNEL_WIDE, dict(kernel=K.KERNEL_WIDE, sprint_max_batch=-1)),
    Family("wide64", 1e-5, K.KERNEL_WIDE, dict(kernel_f64=K.KERNEL_WIDE), f64=True),
    Family("reduced", 1e-4, K.KERNEL_REDUCED, dict(kernel=K.KERNEL_REDUCED)),
    Family("general", 1e-4, K.KERNEL_GENERAL, dict(), generic=True),
    Family("tip32", 1e-4, K.KERNEL_REGISTER, dict(kernel=K.KERNEL_AUTO), device=True, sequences=False),
]
FAMILY = {f.name: f for f in FAMILIES}
SERVED = [(f.name, rel) for f in FAMILIES for rel in CONFIGS if f.serves(rel)]

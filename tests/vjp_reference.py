"""Float64 reference of the implicit-function VJP of the solve (dexr_retarget_vjp*), built from oracle/ only.

At a point x (the solve's answer):
    H      exact Hessian of F = f + norm_delta |x - last|^2: oracle.solvers._model(newton=True, exact_loss_hessian=True)
    M      d(grad_x F)/d ref, by central differences of the ANALYTIC gradient OracleProblem.evaluate(...) in ref (for DexPilot
           the pre-amble is applied inside the difference, with the projection bits held)
    S      free variables: x not on its box bound (within 4 float32 ulps of the bound, the kernel's rule)
    v_S = H_SS^-1 gq_S,  grad_ref = -M^T v,  grad_last = 2 norm_delta v
Differencing the analytic gradient keeps this independent of the kernel's closed form of M.
"""
from __future__ import annotations

import numpy as np

from oracle import solvers

ULP4 = 4.0 * np.finfo(np.float32).eps


def held_mask(prob, x):
    lo, hi = prob.bounds
    return (x <= lo + ULP4 * np.abs(lo)) | (x >= hi - ULP4 * np.abs(hi))


def proj_bits(prob, state, B):
    """(B, n_pair) bool from the uint32 projection bits (None: zeros)."""
    if state is None:
        return np.zeros((B, prob.n_pair), bool)
    st = np.asarray(state, dtype=np.uint32).reshape(B)
    return ((st[:, None] >> np.arange(prob.n_pair, dtype=np.uint32)[None]) & 1).astype(bool)


class Targets:
    """How the forward forms its targets from ref for one batch: the DexPilot pre-amble run once from `state` (weights and
    projection bits then held), the target map T(ref) in float64."""

    def __init__(self, prob, ref, state=None):
        self.prob = prob
        self.ref = np.asarray(ref)
        B = self.ref.shape[0]
        self.kw = {}
        if prob.kind == "dexpilot":
            w, rv, proj = prob.dexpilot_preamble(self.ref.astype(np.float32), proj_bits(prob, state, B))
            self.w, self.proj = w, proj
            self.kw = dict(weights=w, dexpilot_ref=rv)  # the forward's own (float32-rounded) targets at ref

    def kw_at(self, ref64):
        """Objective keyword arguments at a (perturbed, float64) ref with the pre-amble's bits held."""
        if self.prob.kind != "dexpilot":
            return {}
        p = self.prob
        r = np.asarray(ref64, dtype=np.float64)
        n = np.linalg.norm(r[:, :p.n_pair], axis=2, keepdims=True)
        projected = r[:, :p.n_pair] / (n + np.float64(np.float32(1e-6))) * p.projected_dist[None, :, None]
        t = r * p.scaling
        t[:, :p.n_pair] = np.where(self.proj[:, :, None], projected, t[:, :p.n_pair])
        return dict(weights=self.w, dexpilot_ref=t)

    def grad(self, x, ref64, fixed, last):
        _, g, _ = self.prob.evaluate(x, ref64, fixed, last, **self.kw_at(ref64))
        return g


def mixed_derivative(prob, tg: Targets, x, fixed, last, h=1e-7):
    """M (B, n_opt, n_ref * 3): d grad_x F / d ref by central differences of the analytic gradient."""
    ref64 = tg.ref.astype(np.float64)
    B, R, _ = ref64.shape
    M = np.zeros((B, x.shape[1], R * 3))
    for j in range(R * 3):
        e = np.zeros((R * 3,))
        e[j] = h
        e = e.reshape(R, 3)[None]
        M[:, :, j] = (tg.grad(x, ref64 + e, fixed, last) - tg.grad(x, ref64 - e, fixed, last)) / (2 * h)
    return M


def hessian(prob, tg: Targets, x, fixed, last):
    _, _, H = solvers._model(prob, x, tg.ref, fixed, np.asarray(last, dtype=np.float64), tg.kw, exact_loss_hessian=True,
                             newton=True)
    return H


def vjp_reference(prob, ref, fixed, last, x, gq, state=None, return_info=False):
    """(grad_ref (B,n_ref,3), grad_last (B,n_opt)) float64 [, info]: info has the held mask, cond(H_SS), the smallest SmoothL1
    kink distance, DexPilot threshold distance and near-bound distance per frame (the GPU test's exclusion criteria)."""
    x = np.asarray(x, dtype=np.float64)
    B, n = x.shape
    last64 = np.asarray(last, dtype=np.float32).astype(np.float64)
    gq = np.asarray(gq, dtype=np.float64)
    tg = Targets(prob, ref, state)
    H = hessian(prob, tg, x, fixed, last64)
    M = mixed_derivative(prob, tg, x, fixed, last64)
    held = held_mask(prob, x)
    v = np.zeros((B, n))
    cond = np.zeros(B)
    for b in range(B):
        S = ~held[b]
        if S.any():
            Hs = H[b][np.ix_(S, S)]
            v[b, S] = np.linalg.solve(Hs, gq[b, S])
            ev = np.linalg.eigvalsh(Hs)
            cond[b] = np.inf if ev[0] <= 0 else ev[-1] / ev[0]
        else:
            cond[b] = 1.0
    gref = -np.einsum("bn,bnj->bj", v, M).reshape(np.asarray(ref).shape)
    glast = 2 * prob.norm_delta * v
    if not return_info:
        return gref, glast
    return gref, glast, dict(held=held, cond=cond, kink=kink_distance(prob, tg, x, fixed),
                             threshold=threshold_distance(prob, tg.ref), bound=bound_distance(prob, x, held))


def kink_distance(prob, tg: Targets, x, fixed):
    """Per frame: min over terms of | |e| - beta | (vector kinds) or min over coordinates of | |e_i| - beta | (position)."""
    r, _, _, per_coord = solvers._terms(prob, x, tg.ref, fixed, tg.kw)
    beta = prob.huber_delta
    if per_coord:
        return np.abs(np.abs(r) - beta).reshape(r.shape[0], -1).min(1)
    return np.abs(np.linalg.norm(r, axis=2) - beta).min(1)


def threshold_distance(prob, ref):
    """Per frame: distance of the DexPilot pair rows' norms to the projection thresholds (inf for other kinds)."""
    B = np.asarray(ref).shape[0]
    if prob.kind != "dexpilot":
        return np.full(B, np.inf)
    d = np.linalg.norm(np.asarray(ref, dtype=np.float64)[:, :prob.n_pair], axis=2)
    len_s1 = prob.num_fingers - 1
    d1 = np.minimum(np.abs(d[:, :len_s1] - prob.project_dist), np.abs(d[:, :len_s1] - prob.escape_dist)).min(1)
    d2 = np.abs(d[:, len_s1:] - 0.03).min(1) if d.shape[1] > len_s1 else np.full(B, np.inf)
    return np.minimum(d1, d2)


def bound_distance(prob, x, held):
    """Per frame: the smallest distance of a variable that is NOT held to its bounds."""
    lo, hi = prob.bounds
    dist = np.minimum(np.abs(x - lo), np.abs(x - hi))
    return np.where(held, np.inf, dist).min(1)


def excluded(info, kink=1e-6, threshold=1e-5, bound=1e-6, cond=1e8):
    """The frames the comparison leaves out: within `kink` of the SmoothL1 kink, within `threshold` of a DexPilot threshold,
    within `bound` of a bound without sitting on it, or cond(H_SS) above `cond`."""
    return (info["kink"] < kink) | (info["threshold"] < threshold) | (info["bound"] < bound) | ~(info["cond"] <= cond)

"""numpy restatement of the collision-aware posture solve (include/dexr_resolve.h), the yardstick of tests/test_resolve_host.py and
tests/test_gpu_resolve.py.  It shares no code with csrc/dexr_resolve.hpp and is dense throughout: grad d comes from
collision_reference.distance_jacobian (a (B, P, n) matrix), the pose part of H and g from ik_reference.normal_equations over the
target links, the step from np.linalg.solve (LAPACK's pivoted LU) and the iteration is a plain Python loop with a per-frame
`stopped` mask.  No forces, no incidence lists, no active-column index, no Cholesky, no kept system: g and H are formed again
from the current point in every iteration (a rejected trial leaves the point where it was, so they are the same numbers).

    E = E_pose + E_post + E_col        g = -1/2 grad E        H = J^T W J + diag(u) + w_col sum_{first max_active active pairs} w_p dd_p dd_p^T

`links` are the link names of the TABLE (distinct); the first `n_target` of them are the target links, `rows` (S,) the row of each
sphere in the table.  A table with a source map iterates in ITS variables: `full` maps them to the oracle's joint vector, `fold`
is the chain rule of that map on the last axis of a Jacobian (as in ik_reference).  Every operation is in the asked `dtype`.

The run is returned trial by trial, so that the answer for every max_iters <= the one asked is read off one run (`answer`):
the loop is deterministic, its state after k trials does not depend on how many more are allowed."""
import numpy as np

import collision_reference as cref
import ik_reference as ikr
import ik_solve_reference as isr

LAM_UP, LAM_DOWN, MAXREJECT, MAXACTIVE = 8, 4, 12, 256
CONVERGED, STALLED, TRUNCATED = 1, 2, 4


class Problem:
    """the constant inputs of a run, every array in `dtype`."""

    def __init__(self, orc, links, n_target, rows, centers, radii, pairs, margin, x_ref=None, posture_weight=None, tgt_pos=None, tgt_rot=None,
                 w_pos=None, w_rot=None, collision_weight=1.0, pair_weight=None, dtype=np.float64, full=None, fold=None, max_active=MAXACTIVE):
        c = (lambda a: None if a is None else np.asarray(a, dtype))
        self.orc, self.links, self.n_target, self.rows, self.pairs = orc, list(links), int(n_target), np.asarray(rows), np.asarray(pairs)
        self.centers, self.radii, self.dtype = c(centers), c(radii), dtype
        self.margin, self.wcol = dtype(margin), dtype(collision_weight)
        self.x_ref, self.u, self.tgt_pos, self.tgt_rot, self.w_pos, self.w_rot = (c(a) for a in (x_ref, posture_weight, tgt_pos, tgt_rot, w_pos, w_rot))
        self.w = np.ones(len(self.pairs), dtype) if pair_weight is None else c(pair_weight)
        self.full = (lambda x: x) if full is None else full
        self.fold, self.max_active = fold, max_active
        if self.n_target and tgt_pos is None and tgt_rot is None:
            raise ValueError("target links without targets")

    def geo(self):
        return self.links, self.rows, self.centers, self.radii, self.pairs

    def pose_errors(self, q):
        """(e_lin, e_ang) (B, n_target, 3) or None each."""
        p, R = isr.link_poses(self.orc, q, self.links[:self.n_target], self.dtype)
        e_lin = None if self.tgt_pos is None else self.tgt_pos - p
        e_ang = None if self.tgt_rot is None else isr.rotation_error(self.tgt_rot, R, self.dtype)
        return e_lin, e_ang

    def energies(self, x):
        """-> (E3 (B, 3): pose, posture, collision; h (B, P); dist (B, P)) at x (B, n)."""
        dt = self.dtype
        q = np.asarray(self.full(x), dt)
        B = len(x)
        Ep = np.zeros(B, dt)
        if self.n_target:
            e_lin, e_ang = self.pose_errors(q)
            one = np.ones((B, self.n_target), dt)
            if e_lin is not None:
                Ep = Ep + ((one if self.w_pos is None else self.w_pos) * (e_lin * e_lin).sum(-1)).sum(-1)
            if e_ang is not None:
                Ep = Ep + ((one if self.w_rot is None else self.w_rot) * (e_ang * e_ang).sum(-1)).sum(-1)
        Eq = np.zeros(B, dt) if self.u is None else (self.u * (x - self.x_ref) ** 2).sum(-1)
        dist = cref.distances(self.orc, q, *self.geo(), dt)[0]
        h = np.maximum(dt(0), self.margin - dist)
        Ec = self.wcol * (self.w * h * h).sum(-1)
        E3 = np.stack([Ep, Eq, Ec], 1).astype(dt)
        return E3, h, dist

    def system(self, x, h):
        """-> (g (B, n), H (B, n, n) before the damping) at x, h = the hinge values there."""
        dt = self.dtype
        q = np.asarray(self.full(x), dt)
        B, n = x.shape
        g, H = np.zeros((B, n), dt), np.zeros((B, n, n), dt)
        if self.n_target:
            e_lin, e_ang = self.pose_errors(q)
            H, g = ikr.normal_equations(self.orc, q, self.links[:self.n_target], e_lin, e_ang, self.w_pos if e_lin is not None else None,
                                        self.w_rot if e_ang is not None else None, ikr.WORLD, dt, self.fold)
        if self.u is not None:
            g = g + self.u * (self.x_ref - x)
            H = H + np.diag(self.u)[None]
        dd = cref.distance_jacobian(self.orc, q, *self.geo(), dt, self.fold)  # (B, P, n)
        act = h > 0
        keep = act & (np.cumsum(act, 1) <= self.max_active)  # the first max_active active pairs, in pair-index order
        g = g + self.wcol * np.einsum("bp,bpc->bc", self.w * h, dd)
        wd = dd * (self.w * keep)[:, :, None]
        H = H + self.wcol * np.matmul(wd.transpose(0, 2, 1), dd)
        return g.astype(dt), H.astype(dt)


def resolve(P: Problem, x0, damping, max_iters, lo=None, hi=None, tol=0.0, max_step=0.0):
    """-> dict, every array indexed by the number k of trials taken so far (k = 0 .. max_iters) where it has that axis:
    xs (K+1, B, n) the accepted point, energy (K+1, B, 3) its energies, status (K+1, B), iters (K+1, B), decisions (K, B): 1
    accepted, 0 rejected, -1 the frame had stopped; gap (K+1, B) the smallest |margin - d_p| at any point evaluated so far, rel
    (K+1, B) the smallest |Et - E| / E at any decision so far (inf where E == 0); lam (K+1, B); frozen (K, B, n)."""
    dt = P.dtype
    if (lo is None) != (hi is None):
        raise ValueError("lo and hi go together")
    lo, hi = (None if a is None else np.asarray(a, dt) for a in (lo, hi))
    x = np.array(np.atleast_2d(x0), dt)
    if P.x_ref is None:
        P.x_ref = x.copy()
    B, n = x.shape
    eye = np.eye(n, dtype=dt)
    active = isr.active_columns(P.orc, np.asarray(P.full(x), dt), P.links, P.fold, dt)
    E3, h, dist = P.energies(x)
    E = (E3[:, 0] + E3[:, 1]) + E3[:, 2]
    lam = np.full(B, dt(damping), dt)
    rejects, iters, status = np.zeros(B, int), np.zeros(B, np.int32), np.zeros(B, np.int32)
    stopped = np.zeros(B, bool)
    status[(h > 0).sum(1) > P.max_active] |= TRUNCATED
    gap, rel = np.abs(P.margin - dist).min(1).astype(np.float64), np.full(B, np.inf)
    out = dict(xs=[x.copy()], energy=[E3.copy()], status=[status.copy()], iters=[iters.copy()], decisions=[], gap=[gap.copy()], rel=[rel.copy()],
               lam=[lam.copy()], frozen=[])
    for k in range(1, max_iters + 1):
        g, H = P.system(x, h)
        F = ~active[None] | np.zeros((B, n), bool)
        if lo is not None:
            F = F | ((x <= lo) & (g < 0)) | ((x >= hi) & (g > 0))
        g = np.where(F, dt(0), g)
        Hd = H + lam[:, None, None] * eye
        Hd = np.where(F[:, :, None] | F[:, None, :], eye[None], Hd)
        dx = np.linalg.solve(Hd, g[..., None])[..., 0].astype(dt)
        if max_step > 0:
            m = np.abs(dx).max(-1)
            dx = dx * np.where(m > dt(max_step), dt(max_step) / np.where(m > 0, m, dt(1)), dt(1)).astype(dt)[:, None]
        xt = (x + dx).astype(dt)
        if lo is not None:
            xt = np.where(active[None], np.where(xt < lo, lo, np.where(xt > hi, hi, xt)), xt)
        E3t, ht, dt_ = P.energies(xt)
        Et = (E3t[:, 0] + E3t[:, 1]) + E3t[:, 2]
        live = ~stopped
        acc = live & (Et <= E)
        rejd = live & ~acc
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(E > 0, np.abs(Et.astype(np.float64) - E) / E, np.inf)
        rel = np.where(live, np.minimum(rel, r), rel)
        gap = np.where(live, np.minimum(gap, np.abs(P.margin - dt_).min(1)), gap)
        status[live & ((ht > 0).sum(1) > P.max_active)] |= TRUNCATED
        iters[live] = k
        step = np.abs(xt - x).max(-1)
        x = np.where(acc[:, None], xt, x)
        E = np.where(acc, Et, E)
        E3 = np.where(acc[:, None], E3t, E3)
        h = np.where(acc[:, None], ht, h)
        lam = np.where(acc, np.maximum(lam / dt(LAM_DOWN), dt(damping)), np.where(rejd, lam * dt(LAM_UP), lam)).astype(dt)
        rejects = np.where(acc, 0, np.where(rejd, rejects + 1, rejects))
        conv = acc & (step <= dt(tol))
        stall = rejd & (rejects == MAXREJECT)
        status[conv] |= CONVERGED
        status[stall] |= STALLED
        out["decisions"].append(np.where(acc, 1, np.where(rejd, 0, -1)))
        out["frozen"].append(F & live[:, None] & active[None])
        stopped = stopped | conv | stall
        for key, v in (("xs", x), ("energy", E3), ("status", status), ("iters", iters), ("gap", gap), ("rel", rel), ("lam", lam)):
            out[key].append(v.copy())
    res = {key: np.stack(v) if len(v) else np.zeros((0, B)) for key, v in out.items()}
    assert res["xs"].dtype == dt and res["energy"].dtype == dt
    return res


def answer(res, k):
    """what a run with max_iters = k returns: (x (B, n), iters (B), energy (B, 3), status (B))."""
    return res["xs"][k], res["iters"][k], res["energy"][k], res["status"][k]


def clear(res, k, guard_d, guard_e):
    """bool (B,): the frames whose first k trials stayed away from every decision float rounding could flip: no pair within
    guard_d metres of the margin at any evaluated point, no accept test with |Et - E| / E within guard_e."""
    return (res["gap"][k] > guard_d) & (res["rel"][k] > guard_e)

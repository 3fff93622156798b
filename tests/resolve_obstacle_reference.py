"""numpy restatement of the collision-aware posture solve against obstacles (include/dexr_resolve_obstacles.h), the yardstick of
tests/test_resolve_obstacle_host.py and tests/test_gpu_resolve_obstacles.py.  It shares no code with
csrc/dexr_resolve_obstacles.hpp and is dense throughout: `Problem` is resolve_reference.Problem with the obstacle term on top, whose
distances, normals and point Jacobians over ALL (sphere, primitive) entries come from obstacle_reference.fields:

    E = ((E_pose + E_post) + E_col) + E_obs        E_obs = w_obs sum_{s,m} w_m h_sm^2        h_sm = max(0, obstacle_margin - d_sm)
    rows = einsum("bsmr,bsrc->bsmc", n, jpt)       g += w_obs sum_{s,m} w_m h_sm rows_sm
    H += w_obs sum over the first max_contact active (s, m), in the caller's sphere order then set order, of w_m rows_sm rows_sm^T

No forces, no masks, no contact list: the cap is a cumsum over the flattened (S * M) axis.  The run is returned trial by trial as
resolve_reference.resolve returns it, with four energies, and `gap` also covers |obstacle_margin - d_sm|."""
import numpy as np

import ik_solve_reference as isr
import obstacle_reference as oref
import resolve_reference as rr

LAM_UP, LAM_DOWN, MAXREJECT, MAXACTIVE, MAXCONTACT = rr.LAM_UP, rr.LAM_DOWN, rr.MAXREJECT, rr.MAXACTIVE, 256
CONVERGED, STALLED, TRUNCATED, CONTACTS_TRUNCATED = rr.CONVERGED, rr.STALLED, rr.TRUNCATED, 8


class Problem(rr.Problem):
    """the constant inputs of a run with obstacles, every array in `dtype`: those of resolve_reference.Problem (positional), then
    kinds (M,), params (M, 16) as dexr_obstacle_set_create takes them, and by keyword obstacle_margin (None: margin), opos (B, 3),
    orot (B, 3, 3) or None, obstacle_weight, prim_weight (M,) or None, max_contact."""

    def __init__(self, orc, links, n_target, rows, centers, radii, pairs, margin, kinds, params, obstacle_margin=None, opos=None, orot=None,
                 obstacle_weight=1.0, prim_weight=None, max_contact=MAXCONTACT, **kw):
        super().__init__(orc, links, n_target, rows, centers, radii, pairs, margin, **kw)
        dt = self.dtype
        self.kinds, self.params = np.asarray(kinds), np.asarray(params, np.float64)
        self.omargin = self.margin if obstacle_margin is None else dt(obstacle_margin)
        self.opos, self.orot = (None if a is None else np.asarray(a, dt) for a in (opos, orot))
        self.wobs, self.max_contact = dt(obstacle_weight), max_contact
        self.ow = np.ones(len(self.kinds), dt) if prim_weight is None else np.asarray(prim_weight, dt)

    def fields(self, x, jacobian):
        q = np.asarray(self.full(x), self.dtype)
        return oref.fields(self.orc, q, self.links, self.rows, self.centers, self.radii, self.kinds, self.params, self.opos, self.orot,
                           self.dtype, self.fold, jacobian)

    def energies(self, x):
        """-> (E4 (B, 4): pose, posture, self-collision, obstacle; (h (B, P), ho (B, S, M)); gap (B,): the smallest distance of any
        pair or contact from its margin) at x (B, n)."""
        dt = self.dtype
        E3, h, dist = super().energies(x)
        d = self.fields(x, False)["d"]
        ho = np.maximum(dt(0), self.omargin - d)
        Eo = self.wobs * (self.ow * ho * ho).sum((1, 2))
        gap = np.minimum(np.abs(self.margin - dist).min(1), np.abs(self.omargin - d).min((1, 2))).astype(np.float64)
        return np.concatenate([E3, Eo[:, None]], 1).astype(dt), (h, ho), gap

    def system(self, x, hs):
        """-> (g (B, n), H (B, n, n) before the damping) at x, hs = the two hinge arrays there."""
        dt = self.dtype
        h, ho = hs
        g, H = super().system(x, h)
        F = self.fields(x, True)
        rows = np.einsum("bsmr,bsrc->bsmc", F["n"], F["jpt"]).astype(dt)  # grad d_sm
        B, S, M, n = rows.shape
        act = (ho > 0).reshape(B, S * M)
        keep = (act & (np.cumsum(act, 1) <= self.max_contact)).reshape(B, S, M)  # the first max_contact, caller's sphere order then set order
        g = g + self.wobs * np.einsum("bsm,bsmc->bc", self.ow * ho, rows)
        wr = (rows * (self.ow * keep)[..., None]).reshape(B, S * M, n)
        H = H + self.wobs * np.matmul(wr.transpose(0, 2, 1), rows.reshape(B, S * M, n))
        return g.astype(dt), H.astype(dt)

    def counts(self, hs):
        return (hs[0] > 0).sum(1), (hs[1] > 0).sum((1, 2))


def _total(E4):
    return ((E4[:, 0] + E4[:, 1]) + E4[:, 2]) + E4[:, 3]


def resolve(P: Problem, x0, damping, max_iters, lo=None, hi=None, tol=0.0, max_step=0.0):
    """-> dict as resolve_reference.resolve: xs (K+1, B, n), energy (K+1, B, 4), status, iters (K+1, B), decisions (K, B): 1 accepted,
    0 rejected, -1 the frame had stopped; gap (K+1, B) the smallest |margin - d_p| or |obstacle_margin - d_sm| at any point evaluated
    so far, rel (K+1, B) the smallest |Et - E| / E at any decision so far (inf where E == 0); lam (K+1, B); frozen (K, B, n)."""
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
    E4, hs, gap = P.energies(x)
    E = _total(E4)
    lam = np.full(B, dt(damping), dt)
    rejects, iters, status = np.zeros(B, int), np.zeros(B, np.int32), np.zeros(B, np.int32)
    stopped = np.zeros(B, bool)

    def overflow(hs_, who):
        npair, ncon = P.counts(hs_)
        status[who & (npair > P.max_active)] |= TRUNCATED
        status[who & (ncon > P.max_contact)] |= CONTACTS_TRUNCATED

    overflow(hs, ~stopped)
    rel = np.full(B, np.inf)
    out = dict(xs=[x.copy()], energy=[E4.copy()], status=[status.copy()], iters=[iters.copy()], decisions=[], gap=[gap.copy()], rel=[rel.copy()],
               lam=[lam.copy()], frozen=[])
    for k in range(1, max_iters + 1):
        g, H = P.system(x, hs)
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
        E4t, hst, gapt = P.energies(xt)
        Et = _total(E4t)
        live = ~stopped
        acc = live & (Et <= E)
        rejd = live & ~acc
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(E > 0, np.abs(Et.astype(np.float64) - E) / E, np.inf)
        rel = np.where(live, np.minimum(rel, r), rel)
        gap = np.where(live, np.minimum(gap, gapt), gap)
        overflow(hst, live)
        iters[live] = k
        step = np.abs(xt - x).max(-1)
        x = np.where(acc[:, None], xt, x)
        E = np.where(acc, Et, E)
        E4 = np.where(acc[:, None], E4t, E4)
        hs = (np.where(acc[:, None], hst[0], hs[0]), np.where(acc[:, None, None], hst[1], hs[1]))
        lam = np.where(acc, np.maximum(lam / dt(LAM_DOWN), dt(damping)), np.where(rejd, lam * dt(LAM_UP), lam)).astype(dt)
        rejects = np.where(acc, 0, np.where(rejd, rejects + 1, rejects))
        conv = acc & (step <= dt(tol))
        stall = rejd & (rejects == MAXREJECT)
        status[conv] |= CONVERGED
        status[stall] |= STALLED
        out["decisions"].append(np.where(acc, 1, np.where(rejd, 0, -1)))
        out["frozen"].append(F & live[:, None] & active[None])
        stopped = stopped | conv | stall
        for key, v in (("xs", x), ("energy", E4), ("status", status), ("iters", iters), ("gap", gap), ("rel", rel), ("lam", lam)):
            out[key].append(v.copy())
    res = {key: np.stack(v) if len(v) else np.zeros((0, B)) for key, v in out.items()}
    assert res["xs"].dtype == dt and res["energy"].dtype == dt
    return res


answer, clear = rr.answer, rr.clear

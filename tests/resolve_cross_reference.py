"""numpy restatement of the collision-aware posture solve against a second posed robot (include/dexr_resolve_cross.h), the yardstick
of tests/test_resolve_cross_host.py and tests/test_gpu_resolve_cross.py.  It shares no code with csrc/dexr_resolve_cross.hpp and is
dense throughout: `Problem` is resolve_reference.Problem with the cross term on top, whose distances and normals over ALL
(frame, sphere of A, sphere of B) entries come from cross_reference.side / fields -- robot A without a base pose and with its point
Jacobians folded (`fold`), robot B held at q_b with the pose other_pos / other_rot in A's root frame:

    E = ((E_pose + E_post) + E_col) + E_x          E_x = w_x sum_{s,t} w_st h_st^2          h_st = max(0, cross_margin - d_st)
    rows = einsum("bstr,bsrc->bstc", n, jpt_a)     g += w_x sum_{s,t} w_st h_st rows_st                       (B does not move)
    H += w_x sum over the first max_contact active (s, t), A's caller's sphere order then B's, of w_st rows_st rows_st^T

No forces, no masks, no contact list: the hinge array (B, S_a, S_b) flattened is the defined contact order and the cap is a cumsum
over it.  resolve_obstacle_reference.resolve runs the iteration unchanged; the run is returned trial by trial with four energies,
and `gap` also covers |cross_margin - d_st|.  `closest` is the smallest centre distance of any active contact at any point the
problem was asked about (inf where none was active)."""
import numpy as np

import cross_reference as xref
import resolve_obstacle_reference as ror
import resolve_reference as rr

LAM_UP, LAM_DOWN, MAXREJECT, MAXACTIVE, MAXCONTACT = rr.LAM_UP, rr.LAM_DOWN, rr.MAXREJECT, rr.MAXACTIVE, ror.MAXCONTACT
CONVERGED, STALLED, TRUNCATED, CONTACTS_TRUNCATED = rr.CONVERGED, rr.STALLED, rr.TRUNCATED, ror.CONTACTS_TRUNCATED


class Other:
    """robot B, plain data: its oracle, its joint vectors q (B, dof), the links of its table, rows (S_b,), centers (S_b, 3), radii
    (S_b,); pos (B, 3), rot (B, 3, 3) or None: its pose in A's root frame."""

    def __init__(self, orc, q, links, rows, centers, radii, pos=None, rot=None):
        self.orc, self.q, self.links, self.rows, self.centers, self.radii, self.pos, self.rot = orc, q, list(links), rows, centers, radii, pos, rot


class Problem(rr.Problem):
    """the constant inputs of a run against another robot, every array in `dtype`: those of resolve_reference.Problem (positional),
    then `other`, and by keyword cross_margin (None: margin), w_x, cross_weight (S_a, S_b) or None, max_contact."""

    def __init__(self, orc, links, n_target, rows, centers, radii, pairs, margin, other, cross_margin=None, w_x=1.0, cross_weight=None,
                 max_contact=MAXCONTACT, **kw):
        super().__init__(orc, links, n_target, rows, centers, radii, pairs, margin, **kw)
        dt = self.dtype
        self.xmargin = self.margin if cross_margin is None else dt(cross_margin)
        self.wx, self.max_contact = dt(w_x), max_contact
        o = other
        self.side_b = xref.side(o.orc, o.q, o.links, o.rows, o.centers, o.radii, o.pos, o.rot, dt, None, False)  # B does not move
        Sa, Sb = len(self.radii), len(self.side_b["r"])
        self.xw = np.ones((Sa, Sb), dt) if cross_weight is None else np.asarray(cross_weight, dt)
        assert self.xw.shape == (Sa, Sb)
        self.closest = np.inf

    def fields(self, x, jacobian):
        q = np.asarray(self.full(x), self.dtype)
        A = xref.side(self.orc, q, self.links, self.rows, self.centers, self.radii, None, None, self.dtype, self.fold, jacobian)
        return A, xref.fields(A, self.side_b)

    def energies(self, x):
        """-> (E4 (B, 4): pose, posture, self-collision, cross; (h (B, P), hx (B, S_a, S_b)); gap (B,): the smallest distance of any
        pair or contact from its margin) at x (B, n)."""
        dt = self.dtype
        E3, h, dist = super().energies(x)
        F = self.fields(x, False)[1]
        d = F["d"]
        hx = np.maximum(dt(0), self.xmargin - d)
        Ex = self.wx * (self.xw * hx * hx).sum((1, 2))
        gap = np.minimum(np.abs(self.margin - dist).min(1), np.abs(self.xmargin - d).min((1, 2))).astype(np.float64)
        if (hx > 0).any():
            self.closest = min(self.closest, float(F["s"][hx > 0].min()))
        return np.concatenate([E3, Ex[:, None]], 1).astype(dt), (h, hx), gap

    def system(self, x, hs):
        """-> (g (B, n), H (B, n, n) before the damping) at x, hs = the two hinge arrays there."""
        dt = self.dtype
        h, hx = hs
        g, H = super().system(x, h)
        A, F = self.fields(x, True)
        rows = np.einsum("bstr,bsrc->bstc", F["n"], A["jpt"]).astype(dt)  # grad d_st
        B, Sa, Sb, n = rows.shape
        act = (hx > 0).reshape(B, Sa * Sb)
        keep = (act & (np.cumsum(act, 1) <= self.max_contact)).reshape(B, Sa, Sb)  # the first max_contact: A's sphere order, then B's
        g = g + self.wx * np.einsum("bst,bstc->bc", self.xw * hx, rows)
        wr = (rows * (self.xw * keep)[..., None]).reshape(B, Sa * Sb, n)
        H = H + self.wx * np.matmul(wr.transpose(0, 2, 1), rows.reshape(B, Sa * Sb, n))
        return g.astype(dt), H.astype(dt)

    def counts(self, hs):
        return (hs[0] > 0).sum(1), (hs[1] > 0).sum((1, 2))


resolve = ror.resolve
answer, clear = rr.answer, rr.clear

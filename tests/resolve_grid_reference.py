"""numpy restatement of the collision-aware posture solve against a signed-distance grid (include/dexr_resolve_grid.h), the yardstick
of tests/test_resolve_grid_host.py and tests/test_gpu_resolve_grid.py.  It shares no code with csrc/dexr_resolve_grid.hpp and is dense
throughout: `Problem` is resolve_reference.Problem with the grid term on top, whose distances, normals and point Jacobians over ALL
spheres come from grid_reference.fields:

    E = ((E_pose + E_post) + E_col) + E_obs        E_obs = w_obs sum_s h_s^2        h_s = max(0, obstacle_margin - d_s)
    rows = einsum("bsr,bsrc->bsc", n, jpt)         g += w_obs sum_s h_s rows_s      H += w_obs sum_{h_s > 0} rows_s rows_s^T

No forces, no flags, no contact list, no cap: a sphere has one contact at most.  The iteration is resolve_obstacle_reference.resolve
as it stands (the hinge array kept as (B, S, 1), `max_contact` beyond any count), so the run comes back trial by trial with four
energies.

FACE KINKS.  The gradient of the trilinear field jumps across cell faces and the planes of the grid's box, so the rows of an active
sphere near one are another descent's in a run that rounds differently.  `gap` is therefore the smallest of |margin - d_p|,
|obstacle_margin - d_s| and, over the spheres with h_s > 0 at the evaluated point, grid_reference.sdf's distance in metres to the
nearest such face or plane."""
import numpy as np

import grid_reference as gref
import resolve_obstacle_reference as ror
import resolve_reference as rr

LAM_UP, LAM_DOWN, MAXREJECT, MAXACTIVE = rr.LAM_UP, rr.LAM_DOWN, rr.MAXREJECT, rr.MAXACTIVE
CONVERGED, STALLED, TRUNCATED, CONTACTS_TRUNCATED = rr.CONVERGED, rr.STALLED, rr.TRUNCATED, ror.CONTACTS_TRUNCATED
NO_CAP = 1 << 30


class Problem(rr.Problem):
    """the constant inputs of a run against a grid, every array in `dtype`: those of resolve_reference.Problem (positional), then
    values (nx, ny, nz), origin (3,), spacing (3,) as dexr_sdf_grid_create takes them, and by keyword obstacle_margin (None:
    margin), opos (B, 3), orot (B, 3, 3) or None, obstacle_weight."""

    max_contact = NO_CAP

    def __init__(self, orc, links, n_target, rows, centers, radii, pairs, margin, values, origin, spacing, obstacle_margin=None, opos=None,
                 orot=None, obstacle_weight=1.0, **kw):
        super().__init__(orc, links, n_target, rows, centers, radii, pairs, margin, **kw)
        dt = self.dtype
        self.values, self.origin, self.spacing = np.asarray(values, np.float32), np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
        self.omargin = self.margin if obstacle_margin is None else dt(obstacle_margin)
        self.opos, self.orot = (None if a is None else np.asarray(a, dt) for a in (opos, orot))
        self.wobs = dt(obstacle_weight)

    def fields(self, x, jacobian):
        q = np.asarray(self.full(x), self.dtype)
        return gref.fields(self.orc, q, self.links, self.rows, self.centers, self.radii, self.values, self.origin, self.spacing, self.opos,
                           self.orot, self.dtype, self.fold, jacobian)

    def energies(self, x):
        """-> (E4 (B, 4): pose, posture, self-collision, grid; (h (B, P), ho (B, S, 1)); gap (B,)) at x (B, n)."""
        dt = self.dtype
        E3, h, dist = super().energies(x)
        F = self.fields(x, False)
        d = F["d"]
        ho = np.maximum(dt(0), self.omargin - d)
        Eo = self.wobs * (ho * ho).sum(1)
        face = np.where(ho > 0, F["gap"], np.inf).min(1)
        gap = np.minimum(np.minimum(np.abs(self.margin - dist).min(1), np.abs(self.omargin - d).min(1)).astype(np.float64), face)
        return np.concatenate([E3, Eo[:, None]], 1).astype(dt), (h, ho[..., None]), gap

    def system(self, x, hs):
        """-> (g (B, n), H (B, n, n) before the damping) at x, hs = the two hinge arrays there."""
        dt = self.dtype
        h, ho = hs[0], hs[1][..., 0]
        g, H = super().system(x, h)
        F = self.fields(x, True)
        rows = np.einsum("bsr,bsrc->bsc", F["n"], F["jpt"]).astype(dt)  # grad d_s
        g = g + self.wobs * np.einsum("bs,bsc->bc", ho, rows)
        wr = rows * (ho > 0)[..., None]
        H = H + self.wobs * np.matmul(wr.transpose(0, 2, 1), rows)
        return g.astype(dt), H.astype(dt)

    def counts(self, hs):
        return (hs[0] > 0).sum(1), (hs[1] > 0).sum((1, 2))


resolve = ror.resolve
answer, clear = rr.answer, rr.clear

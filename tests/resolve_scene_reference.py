"""numpy restatement of the collision-aware posture solve against a scene of several posed bodies (include/dexr_resolve_scene.h), the
yardstick of tests/test_resolve_scene_host.py and tests/test_gpu_resolve_scene.py.  It shares no code with
csrc/dexr_resolve_scene.hpp and is dense throughout: `Problem` is resolve_reference.Problem with one obstacle term per body on top.
A body's distances, normals and point Jacobians over ALL its (sphere, primitive) entries come from obstacle_reference.fields (a set)
or grid_reference.fields (a grid) with THAT body's pose, and a body's term is formed by the expressions of
resolve_obstacle_reference / resolve_grid_reference with that body's margin and weight:

    E = ((E_pose + E_post) + E_col) + E_obs        E_obs = (((E_0 + E_1) + E_2) + E_3)        g, H += every body's terms, in body order

The hinge arrays of the bodies are concatenated along the last axis, in body order then primitive order, to (B, S, M_total) -- a grid
has one column --, so that the flattened (S * M_total) axis is the defined contact order: the caller's sphere index, then the body,
then the primitive.  The cap is the cumsum of resolve_obstacle_reference over that axis, over all bodies together (grids take part),
and resolve_obstacle_reference.resolve runs the iteration as it stands.

`energies` returns (B, 4 + n_body): the four terms, then E_b of every body; resolve carries all of them trial by trial (its total
reads the first four alone).  `gap` covers every pair, every contact of every body and, for the active spheres of grid bodies, the
cell faces (as resolve_grid_reference does)."""
import numpy as np

import grid_reference as gref
import obstacle_reference as oref
import resolve_obstacle_reference as ror
import resolve_reference as rr

LAM_UP, LAM_DOWN, MAXREJECT, MAXACTIVE, MAXCONTACT = rr.LAM_UP, rr.LAM_DOWN, rr.MAXREJECT, rr.MAXACTIVE, ror.MAXCONTACT
CONVERGED, STALLED, TRUNCATED, CONTACTS_TRUNCATED = rr.CONVERGED, rr.STALLED, rr.TRUNCATED, ror.CONTACTS_TRUNCATED
MAXBODY = 4
NO_CAP = 1 << 30


class Body:
    """one body, plain data: a set (kinds (M,), params (M, 16), prim_weight (M,) or None) or a grid (values (nx, ny, nz), origin,
    spacing); pos (B, 3), rot (B, 3, 3) or None; margin (None: the solve's) and weight."""

    def __init__(self, kinds=None, params=None, values=None, origin=None, spacing=None, pos=None, rot=None, margin=None, weight=1.0,
                 prim_weight=None):
        if (kinds is None) == (values is None):
            raise ValueError("a body is a set or a grid")
        self.grid = values is not None
        if self.grid and prim_weight is not None:
            raise ValueError("a grid has no primitives to weigh")
        self.kinds, self.params = (None, None) if self.grid else (np.asarray(kinds), np.asarray(params, np.float64))
        self.values, self.origin, self.spacing = (np.asarray(values, np.float32), np.asarray(origin, np.float64),
                                                  np.asarray(spacing, np.float64)) if self.grid else (None, None, None)
        self.pos, self.rot, self.margin, self.weight, self.prim_weight = pos, rot, margin, weight, prim_weight
        self.width = 1 if self.grid else len(self.kinds)


class Problem(rr.Problem):
    """the constant inputs of a run against a scene, every array in `dtype`: those of resolve_reference.Problem (positional), then
    `bodies`, 1..MAXBODY of Body, and by keyword max_contact."""

    def __init__(self, orc, links, n_target, rows, centers, radii, pairs, margin, bodies, max_contact=MAXCONTACT, **kw):
        super().__init__(orc, links, n_target, rows, centers, radii, pairs, margin, **kw)
        dt = self.dtype
        bodies = list(bodies)
        if not 1 <= len(bodies) <= MAXBODY:
            raise ValueError(f"a scene has 1..{MAXBODY} bodies")
        self.bodies, self.max_contact = bodies, max_contact
        cast = lambda a: None if a is None else np.asarray(a, dt)  # noqa: E731
        self.pose = [(cast(b.pos), cast(b.rot)) for b in bodies]
        self.omargin = [self.margin if b.margin is None else dt(b.margin) for b in bodies]
        self.wobs = [dt(b.weight) for b in bodies]
        self.ow = [None if b.grid else (np.ones(b.width, dt) if b.prim_weight is None else np.asarray(b.prim_weight, dt)) for b in bodies]
        self.cols = np.cumsum([0] + [b.width for b in bodies])  # body b owns the columns cols[b] : cols[b + 1] of the hinge array

    def fields(self, b, x, jacobian):
        q = np.asarray(self.full(x), self.dtype)
        body, (pos, rot) = self.bodies[b], self.pose[b]
        if body.grid:
            return gref.fields(self.orc, q, self.links, self.rows, self.centers, self.radii, body.values, body.origin, body.spacing, pos, rot,
                               self.dtype, self.fold, jacobian)
        return oref.fields(self.orc, q, self.links, self.rows, self.centers, self.radii, body.kinds, body.params, pos, rot, self.dtype, self.fold,
                           jacobian)

    def energies(self, x):
        """-> (E (B, 4 + n_body): pose, posture, self-collision, E_obs, then E_b of every body; (h (B, P), ho (B, S, M_total)); gap (B,))
        at x (B, n)."""
        dt = self.dtype
        E3, h, dist = super().energies(x)
        gap = np.abs(self.margin - dist).min(1).astype(np.float64)
        hos, Ebs = [], []
        for b, body in enumerate(self.bodies):
            F = self.fields(b, x, False)
            d = F["d"]
            ho = np.maximum(dt(0), self.omargin[b] - d)
            if body.grid:
                Ebs.append(self.wobs[b] * (ho * ho).sum(1))
                gap = np.minimum(gap, np.abs(self.omargin[b] - d).min(1).astype(np.float64))
                gap = np.minimum(gap, np.where(ho > 0, F["gap"], np.inf).min(1))
                ho = ho[..., None]
            else:
                Ebs.append(self.wobs[b] * (self.ow[b] * ho * ho).sum((1, 2)))
                gap = np.minimum(gap, np.abs(self.omargin[b] - d).min((1, 2)).astype(np.float64))
            hos.append(ho)
        Eo = Ebs[0]
        for Eb in Ebs[1:]:
            Eo = Eo + Eb
        E = np.concatenate([E3, Eo[:, None], np.stack(Ebs, 1)], 1).astype(dt)
        return E, (h, np.concatenate(hos, 2)), gap

    def system(self, x, hs):
        """-> (g (B, n), H (B, n, n) before the damping) at x, hs = the two hinge arrays there."""
        dt = self.dtype
        h, ho = hs
        g, H = super().system(x, h)
        B, S, Mt = ho.shape
        act = (ho > 0).reshape(B, S * Mt)
        keep = (act & (np.cumsum(act, 1) <= self.max_contact)).reshape(B, S, Mt)  # the first max_contact of the defined order, all bodies together
        for b, body in enumerate(self.bodies):
            F = self.fields(b, x, True)
            hb, kb = ho[:, :, self.cols[b]:self.cols[b + 1]], keep[:, :, self.cols[b]:self.cols[b + 1]]
            if body.grid:
                rows = np.einsum("bsr,bsrc->bsc", F["n"], F["jpt"]).astype(dt)  # grad d_s
                g = g + self.wobs[b] * np.einsum("bs,bsc->bc", hb[..., 0], rows)
                wr = rows * kb
                H = H + self.wobs[b] * np.matmul(wr.transpose(0, 2, 1), rows)
            else:
                rows = np.einsum("bsmr,bsrc->bsmc", F["n"], F["jpt"]).astype(dt)  # grad d_sm
                M, n = rows.shape[2:]
                g = g + self.wobs[b] * np.einsum("bsm,bsmc->bc", self.ow[b] * hb, rows)
                wr = (rows * (self.ow[b] * kb)[..., None]).reshape(B, S * M, n)
                H = H + self.wobs[b] * np.matmul(wr.transpose(0, 2, 1), rows.reshape(B, S * M, n))
        return g.astype(dt), H.astype(dt)

    def counts(self, hs):
        return (hs[0] > 0).sum(1), (hs[1] > 0).sum((1, 2))


resolve = ror.resolve
clear = rr.clear


def answer(res, k):
    """what a run with max_iters = k returns: (x (B, n), iters (B), energy (B, 4), status (B), body_energy (B, n_body))."""
    return res["xs"][k], res["iters"][k], res["energy"][k][:, :4], res["status"][k], res["energy"][k][:, 4:]

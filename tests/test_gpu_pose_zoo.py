"""GPU tests of the four kernels of csrc/dexr_pose.hip (link poses, their VJP, link velocities, link Jacobians; float and
double) at the limits of the table format, on the synthetic robots of tests/pose_zoo.py: slot indices up to 7, 64 joints
driven by x with 64 links (blocks of 4, 8, 16 and 32 lanes and their ragged tails: docs/experiments/pose_zoo.md lists the
block shape of every member and kernel), n_in = 100 and 256 (all four words of the unused-column mask), SRC_CONST and
SRC_FIXED joints, a column that feeds eight joints, 40 ROOT restores, a chain of 64 joints and angles of several turns.
Every batch has B = 67 frames: a ragged tail of 3 at 4, 8, 16, 32 and 64 lanes per block.

The float64 host entry points are held to the project's gate 1e-10 max(1, max |want|) against OracleRobot at the full joint
vector q_k = mult_k in[col_k] + off_k, derivatives folded by the chain rule (pose_zoo.fold).

GATES OF THE FLOAT32 TESTS (pose_zoo.gates; derived, none is a measured figure; u = 2^-24).  The suite's bound for the
shipped robots is "~30 joints x 4 roundings x 6e-8" per position or rotation entry.  With the member's own depth d (the
longest joint chain of a requested link) and reach r (max |p| of the oracle):
    g_rot = max(4 d, 12) u    per entry of a link rotation or of a world joint axis
    g_pos = g_rot max(1, r)   per entry of a link position or of a world joint origin
The floor of 12 is the worst case of the shortest chain there is, one joint and the placement of its link, which the average
of 4 per joint undercuts below d = 3: an entry of Rx Rot(axis, q) = A + s Bm + (1 - c) C carries the rounding of three table
entries (3 u / 2), of s and c (2 u, an ulp each) and of two fma (u), 4.5 u; the product with the parent's rotation multiplies
that by at most |row|_1 <= sqrt(3) and rounds three times more, 9.3 u; the placement of the link adds sqrt(3) u / 2 + 1.5 u,
2.4 u: 11.7 u.  (The float32 twin of tests/test_pose_zoo_host.py, 2.2 u off on star40, sits over a quarter of 4 d u = 4 u.)
An entry of the world-aligned linear Jacobian that joints with multipliers m_i feed, sum m_i a_i x (p - o_i), errs by at most
|da| |p - o| + |dp| + |do| per joint, |p - o| <= 2 r:
    g_jlin = sum |m_i| (2 r g_rot + 2 g_pos),   g_jang = sum |m_i| g_rot,   g_drot = sum |m_i| 2 g_rot
(d rot[:, j] / d x = sum m_i a_i x rot[:, j]: |da| |rot[:, j]| + |a| |d rot[:, j]|), the sums over the joints of the link's
own chain that read the column: an entry no such joint feeds has gate 0 and must be an exact zero.  In the link's own axes
the entry is (R^T v)_i with v the world-aligned column: R^T dv is charged like the world entry and dR^T v adds at most
g_rot |v|_1 <= sqrt(3) g_rot |v|, |v| <= sum |m_i| 2 r for the linear and sum |m_i| for the angular block:
    g_jlin_local = g_jlin + sum |m_i| sqrt(3) g_rot 2 r,   g_jang_local = g_jang + sum |m_i| sqrt(3) g_rot.
A contraction is gated by the sum over its terms of |cotangent or rate| times the gate of the entry it multiplies: a velocity
by sum_c |xdot_c| g_j*[l, c], the VJP by sum_l (sum_r |grad_pos[l, r]|) g_jlin[l, c] + sum_l (sum_ij |grad_rot[l, i, j]|)
g_drot[l, c].  Every gate is applied entry by entry.  tests/test_pose_zoo_host.py shows that plain float32 numpy arithmetic
stays within a quarter of each; measured on the MI355X: docs/experiments/pose_zoo.md (for information, no test reads it)."""
import numpy as np
import pytest

import pose_zoo as zoo
from dex_retargeting_amd import _lib
from test_gpu_link_jacobians import _gate, to_local
from test_gpu_link_poses import CASES3

pytestmark = pytest.mark.gpu
WORLD, LOCAL = _lib.JAC_WORLD_ALIGNED, _lib.JAC_LOCAL
B = 67
ROWS = (0, 3, 63, 64, 66)
GUARD = 1024  # float32 values of NaN before and after every device output
NAN_BITS = 0x7FC00000


class Case:
    """one member: table, model handle, the B = 67 inputs (float32-representable, so that both arithmetic types and the oracle
    see the same numbers), what the oracle says, and the outputs of the entry points, each computed once."""

    def __init__(self, name, directory):
        self.m = m = zoo.build(name, directory)
        self.model = _lib.PoseModel(m.blob)
        self.x, self.fixed, self.xdot = zoo.inputs(m, B, 2024)
        rng = np.random.default_rng(2025)
        r32 = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
        L = len(m.links)
        self.gp, self.gr = r32(rng.standard_normal((B, L, 3))), r32(rng.standard_normal((B, L, 3, 3)))
        self._want = self._f64 = self._f32 = None
        self.guard_damage = []

    def grads(self, case):
        return (None if case == "rotation-only" else self.gp), (None if case == "position-only" else self.gr)

    @property
    def want(self):
        if self._want is None:
            w = zoo.expect(self.m, self.x, self.fixed)
            for case in CASES3:
                w["vjp " + case] = zoo.expect_vjp(self.m, w["q"], *self.grads(case))
            vl, va = np.einsum("blrc,bc->blr", w["jlin"], self.xdot), np.einsum("blrc,bc->blr", w["jang"], self.xdot)
            R = w["rot"]
            w.update({"jlin 0": w["jlin"], "jang 0": w["jang"], "jlin 1": to_local(R, w["jlin"]), "jang 1": to_local(R, w["jang"]),
                      "vlin 0": vl, "vang 0": va, "vlin 1": to_local(R, vl), "vang 1": to_local(R, va)})
            self.reach = float(np.abs(w["pos"]).max())
            self._want = w
        return self._want

    def host(self, rows=slice(None)):
        """the float64 host entry points on the frames `rows` -> the outputs by name."""
        x, xd = self.x[rows], self.xdot[rows]
        fx = None if self.fixed is None else self.fixed[rows]
        o = {}
        o["pos"], o["rot"] = self.model.poses(x, fx)
        for case in CASES3:
            gp, gr = self.grads(case)
            o["vjp " + case] = self.model.vjp(x, fx, None if gp is None else gp[rows], None if gr is None else gr[rows])
        for frame in (WORLD, LOCAL):
            o[f"jlin {frame}"], o[f"jang {frame}"] = self.model.jacobians(x, fx, frame=frame)
            o[f"vlin {frame}"], o[f"vang {frame}"] = self.model.velocities(x, xd, fx, frame=frame)
        return o

    def device(self, torch, rows=slice(None)):
        """the float32 device entry points on the frames `rows`, on a side stream, every output a slice of a larger tensor of
        NaN -> the outputs by name; guard values that changed are noted in `guard_damage`."""
        model, st = self.model, torch.cuda.Stream()
        n = len(range(B)[rows])
        L, nin = model.n_link, model.n_in
        bufs = {}

        def out(name, *shape):
            bufs[name] = (torch.full((int(np.prod(shape)) + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda"), shape)
            return bufs[name][0].data_ptr() + 4 * GUARD

        with torch.cuda.stream(st):
            dev = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a[rows], dtype=np.float32), device="cuda")  # noqa: E731
            x, fx, xd, gp, gr = (dev(a) for a in (self.x, self.fixed, self.xdot, self.gp, self.gr))
            ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
            sp = st.cuda_stream
            model.poses_dev(n, ptr(x), ptr(fx), out("pos", n, L, 3), out("rot", n, L, 3, 3), stream=sp)
            for case in CASES3:
                model.vjp_dev(n, ptr(x), ptr(fx), 0 if case == "rotation-only" else ptr(gp), 0 if case == "position-only" else ptr(gr),
                              out("vjp " + case, n, nin), stream=sp)
            for frame in (WORLD, LOCAL):
                model.jacobians_dev(n, ptr(x), ptr(fx), out(f"jlin {frame}", n, L, 3, nin), out(f"jang {frame}", n, L, 3, nin),
                                    frame=frame, stream=sp)
                model.velocities_dev(n, ptr(x), ptr(fx), ptr(xd), out(f"vlin {frame}", n, L, 3), out(f"vang {frame}", n, L, 3),
                                     frame=frame, stream=sp)
        st.synchronize()
        o = {}
        for name, (buf, shape) in bufs.items():
            bits = buf.view(torch.int32)
            if not bool((bits[:GUARD] == NAN_BITS).all()) or not bool((bits[-GUARD:] == NAN_BITS).all()):
                self.guard_damage.append(name)
            o[name] = buf[GUARD:-GUARD].reshape(shape).cpu().numpy()
        return o

    def f64(self):
        if self._f64 is None:
            self._f64 = self.host()
        return self._f64

    def f32(self, torch):
        if self._f32 is None:
            self._f32 = self.device(torch)
        return self._f32


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d, made = tmp_path_factory.mktemp("pose_zoo"), {}

    def get(name):
        if name not in made:
            made[name] = Case(name, d)
        return made[name]

    return get


KEYS = ["pos", "rot"] + ["vjp " + c for c in CASES3] + [f"{k} {f}" for f in (WORLD, LOCAL) for k in ("jlin", "jang", "vlin", "vang")]


# ---- 1. float64 host entry points against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("name", zoo.MEMBERS)
def test_host_float64_against_the_oracle(name, cases, require_gpu):
    c = cases(name)
    want, got = c.want, c.f64()
    assert sorted(got) == sorted(KEYS)
    line = []
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), (name, k)
        err = float(np.abs(got[k] - want[k]).max())
        line.append(f"{k} {err:.1e}")
        _gate(err, want[k], (name, k))
    print(f"{name}: float64 max |got - oracle|: " + ", ".join(line))
    fx = c.fixed
    for frame in (WORLD, LOCAL):
        only, none = c.model.jacobians(c.x, fx, frame=frame, angular=False)
        assert none is None and np.array_equal(only, got[f"jlin {frame}"]), (name, frame)
        # J xdot is the velocity
        for j, v in (("jlin", "vlin"), ("jang", "vang")):
            jv = np.einsum("blrc,bc->blr", got[f"{j} {frame}"], c.xdot)
            _gate(float(np.abs(jv - got[f"{v} {frame}"]).max()), want[f"{v} {frame}"], (name, frame, j + " xdot"))
    # J contracted with a cotangent is the VJP
    jg = np.einsum("blrc,blr->bc", got[f"jlin {WORLD}"], c.gp)
    _gate(float(np.abs(jg - got["vjp position-only"]).max()), want["vjp position-only"], (name, "jlin . grad_pos"))


# ---- 2. float32 device entry points against the oracle, under derived gates ---------------------------------------------------
def _f32_gates(c):
    g = zoo.gates(c.m, c.reach)
    G = {"pos": g["pos"], "rot": g["rot"]}
    for case in CASES3:
        G["vjp " + case] = zoo.contraction_gates(g, None, *c.grads(case))
    for frame, s in ((WORLD, ""), (LOCAL, "_local")):
        G[f"jlin {frame}"], G[f"jang {frame}"] = g["jlin" + s][None, :, None, :], g["jang" + s][None, :, None, :]
        G[f"vlin {frame}"], G[f"vang {frame}"] = zoo.contraction_gates(g, c.xdot, local=frame == LOCAL)
    return G


@pytest.mark.parametrize("name", zoo.MEMBERS)
def test_device_float32_against_the_oracle_under_derived_gates(name, cases, require_gpu):
    torch = pytest.importorskip("torch")
    c = cases(name)
    want, got = c.want, c.f32(torch)
    gates = _f32_gates(c)
    print(f"{name}: depth {c.m.depth}, reach {c.reach:.3f} m, g_rot {zoo.gates(c.m, c.reach)['rot']:.3e}; float32 max |got - oracle| "
          "(largest gate, largest error / gate):")
    bad = []
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32, (name, k)
        err = np.abs(got[k].astype(np.float64) - want[k])
        gate = np.broadcast_to(gates[k], err.shape)
        ok = np.isfinite(err).all() and bool((err <= gate).all())
        ratio = float(np.nanmax(np.where(gate > 0, err / np.maximum(gate, 1e-300), 0.0)))
        print(f"    {k:<18} {float(np.nanmax(err)):.3e}  ({float(gate.max()):.3e}, {ratio:.3f})")
        if not ok:
            bad.append((k, float(np.nanmax(err)), ratio))
    assert not bad, (name, bad)


# ---- 3. every entry written, nothing else touched, exact zeros where no joint reads ----------------------------------------------
@pytest.mark.parametrize("name", zoo.MEMBERS)
def test_every_entry_is_written_and_unread_columns_are_exact_zeros(name, cases, require_gpu):
    torch = pytest.importorskip("torch")
    c = cases(name)
    am = zoo.abs_mult(c.m)                  # (L, n_in): 0 where no joint above the link reads the column
    unread = np.flatnonzero(am.sum(0) == 0)
    if name == "two_trees100_a":
        assert set(range(50)) == set(unread.tolist())
    if name == "wide_map":
        assert len(unread) == 233 and {int(u) // 64 for u in unread} == {0, 1, 2, 3} and zoo.SHARED_COL not in unread
    if name == "star40":
        assert (am.sum(1) == 0).sum() == 3  # the base link and the two links fixed to it
    outs32 = c.f32(torch)
    assert c.guard_damage == [], (name, "values before or after an output were overwritten")
    for outs in (outs32, c.f64()):
        for k in KEYS:
            assert not np.isnan(outs[k]).any(), (name, k, "an entry was not written")
        for case in CASES3:
            g = outs["vjp " + case]
            assert np.array_equal(g[:, unread], np.zeros_like(g[:, unread])), (name, case)
            if case == "both":  # (a prismatic joint has no share in a rotation, a leaf's origin is its link's)
                assert (np.abs(g[:, am.sum(0) > 0]).max(0) > 0).all(), name
        dead = np.broadcast_to((am == 0)[None, :, None, :], outs[f"jlin {WORLD}"].shape)
        still = am.sum(1) == 0
        for frame in (WORLD, LOCAL):
            for k in ("jlin", "jang"):
                J = outs[f"{k} {frame}"]
                assert not J[dead].any(), (name, k, frame)
            for k in ("vlin", "vang"):
                assert not outs[f"{k} {frame}"][:, still].any(), (name, k, frame)


# ---- 4. a frame's answer does not depend on the batch it is in -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain64", "binary64"])
def test_rows_of_a_ragged_batch_equal_single_frame_calls_bitwise(name, cases, require_gpu):
    torch = pytest.importorskip("torch")
    c = cases(name)
    full64, full32 = c.f64(), c.f32(torch)
    for r in ROWS:
        one64, one32 = c.host(slice(r, r + 1)), c.device(torch, slice(r, r + 1))
        for k in KEYS:
            assert one64[k].shape[0] == one32[k].shape[0] == 1
            assert np.array_equal(one64[k][0], full64[k][r]), (name, "float64", k, r)
            assert np.array_equal(one32[k][0], full32[k][r]), (name, "float32", k, r)
    assert c.guard_damage == []


# ---- 5. the slot a fork is kept in does not change the arithmetic ------------------------------------------------------------
def test_slots_three_to_seven_give_the_bits_of_slots_zero_to_four(cases, require_gpu):
    torch = pytest.importorskip("torch")
    a, b = cases("binary64"), cases("binary64_slots8")
    ja, jb = a.m.tab["joints"], b.m.tab["joints"]
    assert int(b.m.tab["h"]["n_slot"]) == 8 and {int(s) for s in jb["save"] if s >= 0} == {3, 4, 5, 6, 7}
    assert np.array_equal(np.where(ja["save"] >= 0, 7 - ja["save"], ja["save"]), jb["save"])
    assert np.array_equal(a.x, b.x) and np.array_equal(a.gr, b.gr)
    for outs_a, outs_b, what in ((a.f64(), b.f64(), "float64"), (a.f32(torch), b.f32(torch), "float32")):
        for k in KEYS:
            assert np.array_equal(outs_a[k], outs_b[k]), (what, k)
    assert b.guard_damage == []

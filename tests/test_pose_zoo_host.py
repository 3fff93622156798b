"""CPU tests of the pose tables at the limits of their format, on the synthetic robots of tests/pose_zoo.py: what the compiled
table of every member looks like (joints, fork slots, input columns, ROOT restores, the refusal of more than 64 joints), the
numpy interpreter tests/pose_interp.py against OracleRobot on them (poses and VJP, source map of wide_map folded by the chain
rule), the slot walk against the parent walk bit for bit, and a float32 twin of the walk that shows the derived float32 gates
of tests/test_gpu_pose_zoo.py (derivation: that module's docstring) can be met by plain float32 arithmetic: its error against
the float64 oracle is at most a quarter of every gate."""
import numpy as np
import pytest

import pose_interp as pi
import pose_zoo as zoo
from dex_retargeting_amd import pose_tables as pt

B = 16


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    d = tmp_path_factory.mktemp("pose_zoo")
    return {name: zoo.build(name, d) for name in zoo.MEMBERS + [zoo.REFUSED]}


# ---- 1. the structure the table is meant to reach -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", zoo.MEMBERS)
def test_compiled_table_has_the_structure_the_member_is_for(name, members):
    m = members[name]
    tab, want = m.tab, zoo.FACTS[name]
    got = dict(n_joint=int(tab["h"]["n_joint"]), n_slot=int(tab["h"]["n_slot"]), n_in=int(tab["h"]["n_in"]),
               n_root=int((tab["joints"]["restore"] == pt.ROOT).sum()), n_base=int((tab["links"]["parent"] == -1).sum()),
               n_link=int(tab["h"]["n_link"]))
    assert got == want, name
    assert len(m.links) == want["n_link"] and m.kin.dof == (100 if "two_trees" in name or name == "wide_map" else want["n_joint"])
    slots = np.concatenate([tab["joints"]["save"], tab["joints"]["restore"]])
    assert sorted(set(slots[slots >= 0].tolist())) == (list(range(3, 8)) if name == "binary64_slots8" else list(range(want["n_slot"])))
    x_cols = set(tab["joints"]["src_col"][tab["joints"]["src_kind"] == pt.SRC_X].tolist())
    if name.startswith("chain64"):
        assert m.depth == 64 and (tab["joints"]["restore"][1:] == pt.CONTINUE).all()
        assert len(set(tab["links"]["parent"].tolist())) == 56 and (tab["joints"]["type"] == pt.PRISMATIC).sum() == 12
        lim = m.kin.joint_limits[[j.type == "revolute" for j in m.kin.joints]]
        assert (np.abs(lim) == 20.0).all() if name == "chain64_turns" else (lim == zoo.REV_LIMITS).all()
    if name.startswith("binary64"):
        assert m.depth == 7 and tab["joints"]["type"][0] == pt.PRISMATIC and len(set(tab["joints"]["type"].tolist())) == 2
    if name == "star40":
        assert len(set(m.links)) == 43 and "base" in m.links and m.depth == 1
    if name == "two_trees100_a":
        assert x_cols == set(range(50, 100))  # columns 0..49: in no joint's hands, one and a half mask words
    if name == "two_trees100_b":
        assert min(x_cols) < 50 and max(x_cols) >= 64 and len(x_cols) == 64
    if name == "wide_map":
        kinds = tab["joints"]["src_kind"]
        assert ((kinds == pt.SRC_X).sum(), (kinds == pt.SRC_FIXED).sum(), (kinds == pt.SRC_CONST).sum()) == (30, 16, 4)
        assert set(zoo.WIDE_X_COLS) < x_cols and len(x_cols) == 23 and all(any(c // 64 == w for c in x_cols) for w in range(4))
        shared = tab["joints"][(kinds == pt.SRC_X) & (tab["joints"]["src_col"] == zoo.SHARED_COL)]
        assert len(shared) == 8 and (shared["mult"] > 0).sum() == 4 and (shared["off"] != 0).all()
        fcols = set(tab["joints"]["src_col"][kinds == pt.SRC_FIXED].tolist())
        assert {0, 255} < fcols and len(fcols) == 16
        const = tab["joints"][kinds == pt.SRC_CONST]
        assert (const["off"] != 0).all() and (const["mult"] != 0).all()  # q = off: the multiplier of a constant is not used


def test_links_that_need_more_than_64_joints_are_refused(members):
    m = members[zoo.REFUSED]
    assert m.blob is None and len(m.links) == 64 and len(set(m.links)) == 64
    with pytest.raises(ValueError, match="a pose table holds 64"):
        pt.compile_poses(m.kin, m.links)
    pt.compile_poses(m.kin, m.links[:50])  # the first tree alone is fine


# ---- 2. interpreter against the oracle, slot walk against parent walk ---------------------------------------------------------
@pytest.mark.parametrize("name", zoo.MEMBERS)
def test_interpreted_table_equals_the_oracle_and_the_slot_walk_the_parent_walk(name, members):
    from test_gpu_link_poses import CASES3, _grads

    m = members[name]
    tab = m.tab
    x, fixed, _ = zoo.inputs(m, B, 1)
    want = zoo.expect(m, x, fixed)
    pos, rot = pi.poses(tab, x, fixed)
    e_pos, e_rot = np.abs(pos - want["pos"]).max(), np.abs(rot - want["rot"]).max()
    print(f"{name}: interpreter max |pos - oracle| = {e_pos:.3e}, |rot - oracle| = {e_rot:.3e}, reach {np.abs(want['pos']).max():.3f} m")
    assert e_pos <= 1e-12 and e_rot <= 1e-12, name
    rng = np.random.default_rng(2)
    for case in CASES3:
        gp, gr = _grads(rng, B, len(m.links), case)
        g = pi.vjp(tab, x, fixed, gp, gr)
        w = zoo.expect_vjp(m, want["q"], gp, gr)
        err = np.abs(g - w).max()
        print(f"{name} {case}: interpreter max |g - oracle| = {err:.3e} at max |g| = {np.abs(w).max():.3f}")
        assert err <= 1e-12, (name, case)
    Rs, ps, _ = pi._joint_frames(tab, pi.joint_values(tab, x, fixed))
    for k, (R, p) in enumerate(pi.walk_with_slots(tab, x, fixed)):
        assert np.array_equal(R, Rs[k]) and np.array_equal(p, ps[k]), (name, k)


# ---- 3. the float32 twin ----------------------------------------------------------------------------------------------------
def float32_twin(tab, x, fixed=None):
    """The walk of pose_interp with every value float32 -> per link (caller's order) p (B, L, 3) and R (B, L, 3, 3), and the
    world-aligned jlin = mult a x (p - o) | mult a and jang = mult a, (B, L, 3, n_in), formed in float32."""
    f = np.float32
    x = np.asarray(x, f)
    Bn, nin, L = x.shape[0], int(tab["h"]["n_in"]), len(tab["links"])
    I3 = np.eye(3, dtype=f)
    Rs, ps, axes = [], [], []
    for j in tab["joints"]:
        kind, col, par = int(j["src_kind"]), int(j["src_col"]), int(j["parent"])
        src = x[:, col] if kind == 0 else (np.asarray(fixed, f)[:, col] if kind == 1 else np.zeros(Bn, f))
        q = f(j["mult"]) * src + f(j["off"])
        X, a = j["X"].reshape(3, 4).astype(f), j["axis"].astype(f)
        Rp, pp = (Rs[par], ps[par]) if par >= 0 else (np.broadcast_to(I3, (Bn, 3, 3)), np.zeros((Bn, 3), f))
        R, p = Rp @ X[:, :3], pp + Rp @ X[:, 3]
        aw = R @ a
        if int(j["type"]) == 0:
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f)
            R = R @ (I3[None] + np.sin(q)[:, None, None] * K[None] + (f(1) - np.cos(q))[:, None, None] * (K @ K)[None])
        else:
            p = p + aw * q[:, None]
        Rs.append(R), ps.append(p), axes.append(aw)
    pos, rot = np.zeros((Bn, L, 3), f), np.zeros((Bn, L, 3, 3), f)
    jlin, jang = np.zeros((Bn, L, 3, nin), f), np.zeros((Bn, L, 3, nin), f)
    for l in tab["links"]:
        par, o, X = int(l["parent"]), int(l["out"]), l["X"].reshape(3, 4).astype(f)
        Rp, pp = (Rs[par], ps[par]) if par >= 0 else (np.broadcast_to(I3, (Bn, 3, 3)), np.zeros((Bn, 3), f))
        pos[:, o], rot[:, o] = pp + Rp @ X[:, 3], Rp @ X[:, :3]
        k = par
        while k >= 0:
            j = tab["joints"][k]
            if int(j["src_kind"]) == 0:
                c, mlt = int(j["src_col"]), f(j["mult"])
                if int(j["type"]) == 0:
                    jlin[:, o, :, c] += mlt * np.cross(axes[k], pos[:, o] - ps[k])
                    jang[:, o, :, c] += mlt * axes[k]
                else:
                    jlin[:, o, :, c] += mlt * axes[k]
            k = int(j["parent"])
    assert all(a.dtype == f for a in (pos, rot, jlin, jang))
    return pos, rot, jlin, jang


def _drot(jang, rot):
    """d rot[:, j] / d x_c = jang[:, c] x rot[:, j] -> (B, L, 3, 3, n_in), in the arithmetic of the arguments."""
    return np.cross(jang[:, :, :, None, :], rot[:, :, :, :, None], axis=2)


@pytest.mark.parametrize("name", zoo.MEMBERS)
def test_float32_twin_stays_within_a_quarter_of_every_gate(name, members):
    from test_gpu_link_jacobians import to_local

    m = members[name]
    x, fixed, _ = zoo.inputs(m, B, 3)
    want = zoo.expect(m, x, fixed)
    reach = float(np.abs(want["pos"]).max())
    g = zoo.gates(m, reach)
    pos, rot, jlin, jang = float32_twin(m.tab, x, fixed)
    loc = lambda R, J: np.einsum("blji,blj...->bli...", R, J)  # noqa: E731  (to_local in the arithmetic of its arguments)
    pairs = {
        "pos": (pos, want["pos"], g["pos"]), "rot": (rot, want["rot"], g["rot"]),
        "jlin": (jlin, want["jlin"], g["jlin"][None, :, None, :]), "jang": (jang, want["jang"], g["jang"][None, :, None, :]),
        "jlin local": (loc(rot, jlin), to_local(want["rot"], want["jlin"]), g["jlin_local"][None, :, None, :]),
        "jang local": (loc(rot, jang), to_local(want["rot"], want["jang"]), g["jang_local"][None, :, None, :]),
        "drot": (_drot(jang, rot), _drot(want["jang"], want["rot"]), g["drot"][None, :, None, None, :]),
    }
    line = []
    for what, (got, w, gate) in pairs.items():
        assert got.dtype == np.float32 and got.shape == w.shape, (name, what)
        err = np.abs(got - w)
        gate = np.broadcast_to(gate, err.shape)
        assert (err <= gate / 4).all(), (name, what, float(err.max()), float((err / np.maximum(gate, 1e-300)).max()))
        assert not err[gate == 0].any(), (name, what)  # an entry no joint feeds is an exact zero on both sides
        line.append(f"{what} {err.max():.2e} / {np.max(gate):.2e}")
    print(f"{name} (depth {m.depth}, reach {reach:.2f} m): float32 twin error / gate: " + ", ".join(line))

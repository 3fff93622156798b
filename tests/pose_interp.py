"""numpy float64 interpreter of a pose table blob (include/dexr_pose.h), written from the header's description and sharing
no code with dex_retargeting_amd/pose_tables.py or csrc/dexr_pose.hip: plain T_k = T_parent X_k Rot(axis, q) through the
`parent` field (the save / restore slots are checked separately by `walk_with_slots`), and the closed-form VJP
    dL/dq_k = a_k . (T0_k - o_k x F_k)  (revolute)   |   a_k . F_k  (prismatic)
with the wrench sums taken over the links whose chain contains joint k."""
import numpy as np

HEADER = np.dtype([("magic", "<u4"), ("version", "<u4"), ("n_joint", "<i4"), ("n_link", "<i4"), ("n_in", "<i4"),
                   ("n_fixed", "<i4"), ("n_slot", "<i4"), ("reserved", "<i4")])
JOINT = np.dtype([("parent", "<i4"), ("type", "<i4"), ("src_kind", "<i4"), ("src_col", "<i4"), ("restore", "<i4"),
                  ("save", "<i4"), ("link_begin", "<i4"), ("link_end", "<i4"), ("sub_link_end", "<i4"), ("reserved", "<i4"),
                  ("mult", "<f8"), ("off", "<f8"), ("X", "<f8", (12,)), ("axis", "<f8", (3,))])
LINK = np.dtype([("parent", "<i4"), ("out", "<i4"), ("X", "<f8", (12,))])


def parse(blob: bytes):
    h = np.frombuffer(blob[:HEADER.itemsize], HEADER)[0]
    assert int(h["magic"]) == 0x53505844 and int(h["version"]) == 1
    nj, nl = int(h["n_joint"]), int(h["n_link"])
    o = HEADER.itemsize
    joints = np.frombuffer(blob[o:o + nj * JOINT.itemsize], JOINT)
    o += nj * JOINT.itemsize
    links = np.frombuffer(blob[o:o + nl * LINK.itemsize], LINK)
    assert o + nl * LINK.itemsize == len(blob)
    return dict(h=h, joints=joints, links=links)


def joint_values(tab, x, fixed=None):
    x = np.atleast_2d(np.asarray(x, np.float64))
    q = np.zeros((x.shape[0], len(tab["joints"])))
    for k, j in enumerate(tab["joints"]):
        kind, col = int(j["src_kind"]), int(j["src_col"])
        src = x[:, col] if kind == 0 else (np.asarray(fixed, np.float64).reshape(x.shape[0], -1)[:, col] if kind == 1 else 0.0)
        q[:, k] = float(j["mult"]) * src + float(j["off"])
    return q


def _rodrigues(a, th):
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3)[None] + np.sin(th)[:, None, None] * K[None] + (1 - np.cos(th))[:, None, None] * (K @ K)[None]


def _joint_frames(tab, q):
    """per joint: world rotation R (B,3,3) and origin p (B,3) after the joint's own motion, and the world axis."""
    B = q.shape[0]
    Rs, ps, axes = [], [], []
    for k, j in enumerate(tab["joints"]):
        par = int(j["parent"])
        Rp = Rs[par] if par >= 0 else np.broadcast_to(np.eye(3), (B, 3, 3))
        pp = ps[par] if par >= 0 else np.zeros((B, 3))
        X = j["X"].reshape(3, 4)
        R = Rp @ X[:, :3]
        p = pp + Rp @ X[:, 3]
        a = R @ j["axis"]
        if int(j["type"]) == 0:
            R = R @ _rodrigues(j["axis"], q[:, k])
        else:
            p = p + a * q[:, k:k + 1]
        Rs.append(R)
        ps.append(p)
        axes.append(a)
    return Rs, ps, axes


def poses(tab, x, fixed=None):
    """-> pos (B, L, 3), rot (B, L, 3, 3) in the caller's link order."""
    q = joint_values(tab, x, fixed)
    B, L = q.shape[0], len(tab["links"])
    Rs, ps, _ = _joint_frames(tab, q)
    pos, rot = np.zeros((B, L, 3)), np.zeros((B, L, 3, 3))
    for l in tab["links"]:
        par, X = int(l["parent"]), l["X"].reshape(3, 4)
        Rp = Rs[par] if par >= 0 else np.broadcast_to(np.eye(3), (B, 3, 3))
        pp = ps[par] if par >= 0 else np.zeros((B, 3))
        pos[:, int(l["out"])] = pp + Rp @ X[:, 3]
        rot[:, int(l["out"])] = Rp @ X[:, :3]
    return pos, rot


def vjp(tab, x, fixed=None, grad_pos=None, grad_rot=None):
    """-> grad_x (B, n_in)."""
    q = joint_values(tab, x, fixed)
    B = q.shape[0]
    Rs, ps, axes = _joint_frames(tab, q)
    pos, rot = poses(tab, x, fixed)
    nj = len(tab["joints"])
    gx = np.zeros((B, int(tab["h"]["n_in"])))
    F, T0 = np.zeros((nj, B, 3)), np.zeros((nj, B, 3))
    for l in tab["links"]:
        o = int(l["out"])
        f = np.zeros((B, 3)) if grad_pos is None else np.asarray(grad_pos, np.float64)[:, o]
        t = np.cross(pos[:, o], f)
        if grad_rot is not None:
            G = np.asarray(grad_rot, np.float64)[:, o]
            for c in range(3):
                t = t + np.cross(rot[:, o, :, c], G[:, :, c])
        k = int(l["parent"])
        while k >= 0:
            F[k] += f
            T0[k] += t
            k = int(tab["joints"][k]["parent"])
    for k, j in enumerate(tab["joints"]):
        if int(j["src_kind"]) != 0:
            continue
        if int(j["type"]) == 0:
            g = np.einsum("bi,bi->b", axes[k], T0[k] - np.cross(ps[k], F[k]))
        else:
            g = np.einsum("bi,bi->b", axes[k], F[k])
        gx[:, int(j["src_col"])] += float(j["mult"]) * g
    return gx


def walk_with_slots(tab, x, fixed=None):
    """The kernel's walk: one running transform, fork transforms in `n_slot` numbered slots.  Returns the per-joint
    (R, p) it produces; equal to _joint_frames when the save / restore fields are right."""
    q = joint_values(tab, x, fixed)
    B = q.shape[0]
    slots = [None] * int(tab["h"]["n_slot"])
    R, p = None, None
    out = []
    for k, j in enumerate(tab["joints"]):
        r = int(j["restore"])
        if r == -2:
            R, p = np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3))
        elif r >= 0:
            R, p = slots[r]
        else:
            assert r == -1 and int(j["parent"]) == k - 1
        X = j["X"].reshape(3, 4)
        p = p + R @ X[:, 3]
        R = R @ X[:, :3]
        if int(j["type"]) == 0:
            R = R @ _rodrigues(j["axis"], q[:, k])
        else:
            p = p + (R @ j["axis"]) * q[:, k:k + 1]
        if int(j["save"]) >= 0:
            slots[int(j["save"])] = (R, p)
        out.append((R, p))
    return out

"""fp64 autograd reference of the task-map derivatives (x, xd = J qd, J, c = Jdot qd) of a frame's 4x4 transform and of its
Euler angles, for the tests: TEST INFRASTRUCTURE, CPU only.

It shares no derivation with the C oracle (oracle/rmp2_oracle.c: one recursion of velocities and bias accelerations, closed-form
H^-1 of the Euler map) or with the kernels: the forward map is the plain product of local transforms along the frame's ancestor
chain, and every derivative is torch.func autograd of that product (jvp / jacrev), one state at a time.  The constants are the
descriptor's own (`desc.robot`: parent, joint_type, q_index, axis, T_const as stored in fp32, cast up), so both sides see the same
numbers and x agrees to round-off.

What it cannot agree on to round-off are the derivatives: the descriptor's fp32 T_const rotations are off orthonormal by a few
1e-7, the recursion differentiates as if they were rigid (w x R, z x r), autograd differentiates the stored numbers.  `--measure`
prints that defect beside the deviations and writes profiles/kinematics_reference.json, the numbers the bounds of
tests/test_kinematics_reference_host.py and tests/test_gpu_fk_differentiation.py are literals of.

    python tests/kinematics_reference.py --measure
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from riemannian_motion_policies_amd import descriptor as D, urdf as U  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "kinematics_reference.json")
STATES = 4          # states per scene (the host tests and --measure use the first HOST_STATES of them)
HOST_STATES = 2
QD_MAX = 2.0
CY_HELD_F64 = 0.1   # Euler cases the f64 / f32 oracle comparisons of the host file hold
CY_HELD_F32 = 1e-2  # Euler cases an fp32 evaluation is held on (below, its theta_x / theta_z are noise: DESIGN.md)


# ---- the reference ----------------------------------------------------------------------------------------------------------

def constants(desc):
    """The robot table of a descriptor as fp64 tensors (the fp32 numbers, cast up)."""
    import torch
    rb = desc.robot
    F = rb.n_frames
    Tc = np.zeros((F, 4, 4))
    Tc[:, 3, 3] = 1.0
    for f in range(F):
        Tc[f, :3, :] = np.array([rb.T_const[f][k] for k in range(12)], np.float64).reshape(3, 4)
    return {"n_frames": F, "n_dof": rb.n_dof,
            "parent": [int(rb.parent[f]) for f in range(F)],
            "joint_type": [int(rb.joint_type[f]) for f in range(F)],
            "q_index": [int(rb.q_index[f]) for f in range(F)],
            "axis": torch.tensor([[rb.axis[f][k] for k in range(3)] for f in range(F)], dtype=torch.float64),
            "T_const": torch.tensor(Tc)}


def _chain(consts, frame):
    out = []
    f = frame
    while f >= 0:
        out.append(f)
        f = consts["parent"][f]
    return out[::-1]


def _variable(consts, f, q):
    """The joint's own 4x4: Rodrigues about the stored axis (not renormalised), a translation along it, or the identity."""
    import torch
    jt, j = consts["joint_type"][f], consts["q_index"][f]
    eye = torch.eye(4, dtype=torch.float64)
    if jt == U.JOINT_FIXED:
        return eye
    qv = q[j] if j >= 0 else torch.zeros((), dtype=torch.float64)   # a joint outside the order is held at 0
    u = consts["axis"][f]
    if jt == U.JOINT_REVOLUTE:
        z = torch.zeros((), dtype=torch.float64)
        K = torch.stack([torch.stack([z, -u[2], u[1]]), torch.stack([u[2], z, -u[0]]), torch.stack([-u[1], u[0], z])])
        R = torch.cos(qv) * torch.eye(3, dtype=torch.float64) + torch.sin(qv) * K + (1 - torch.cos(qv)) * torch.outer(u, u)
        top = torch.cat([R, torch.zeros(3, 1, dtype=torch.float64)], dim=1)
    else:
        top = torch.cat([torch.eye(3, dtype=torch.float64), (qv * u)[:, None]], dim=1)
    return torch.cat([top, eye[3:]], dim=0)


def fk_vec(consts, q, frame):
    """vec(T_frame) [16], row-major: the product of T_const @ T_variable(q) from the root down to `frame`."""
    import torch
    T = torch.eye(4, dtype=torch.float64)
    for f in _chain(consts, frame):
        T = T @ (consts["T_const"][f] @ _variable(consts, f, q))
    return T.reshape(16)


def euler_xyz(vec16):
    """(theta_x, theta_y, theta_z) of R = Rz Ry Rx: theta_y = -asin(r20), the guard |cos theta_y| < 1e-6 -> 1 on the value,
    atan2 of the divided entries."""
    import torch
    T = vec16.reshape(4, 4)
    ty = -torch.asin(T[2, 0])
    cy = torch.cos(ty)
    safe = torch.where(torch.abs(cy) < 1e-6, torch.ones_like(cy), cy)
    tz = torch.atan2(T[1, 0] / safe, T[0, 0] / safe)
    tx = torch.atan2(T[2, 1] / safe, T[2, 2] / safe)
    return torch.stack([tx, ty, tz])


def task_map(consts, frame, euler=False):
    if euler:
        return lambda q: euler_xyz(fk_vec(consts, q, frame))
    return lambda q: fk_vec(consts, q, frame)


def differentiate(desc, q, qd, frame, euler=False, consts=None):
    """(x [k], xd [k], J [k, n], c [k]) in fp64 at ONE state (q, qd [n]); k = 16, or 3 with euler=True."""
    import torch
    from torch.func import jacrev, jvp
    consts = consts or constants(desc)
    f = task_map(consts, frame, euler)
    qt = torch.as_tensor(np.asarray(q, np.float64))
    qdt = torch.as_tensor(np.asarray(qd, np.float64))
    x, xd = jvp(f, (qt,), (qdt,))
    J = jacrev(f)(qt)
    _, c = jvp(lambda y: jvp(f, (y,), (qdt,))[1], (qt,), (qdt,))
    return x.numpy(), xd.numpy(), J.numpy(), c.numpy()


def differentiate_batch(desc, q, qd, frame, euler=False, consts=None):
    """differentiate() over the rows of q, qd [B, n]: (x [B, k], xd [B, k], J [B, k, n], c [B, k])."""
    import torch
    from torch.func import jacrev, jvp, vmap
    consts = consts or constants(desc)
    f = task_map(consts, frame, euler)

    def one(a, b):   # differentiate() of one state, traced once for all rows
        x, xd = jvp(f, (a,), (b,))
        _, c = jvp(lambda y: jvp(f, (y,), (b,))[1], (a,), (b,))
        return x, xd, jacrev(f)(a), c

    qt = torch.as_tensor(np.asarray(q, np.float64))
    qdt = torch.as_tensor(np.asarray(qd, np.float64))
    return tuple(t.numpy() for t in vmap(one)(qt, qdt))


def orthonormality_defect(desc):
    """max over frames of |R^T R - I| of the stored fp32 T_const rotations."""
    Tc = constants(desc)["T_const"].numpy()[:, :3, :3]
    return float(np.abs(np.einsum("fji,fjk->fik", Tc, Tc) - np.eye(3)).max())


# ---- scenes -----------------------------------------------------------------------------------------------------------------

WRIST_ORDER = ["jz", "jy", "jx"]
WRIST_URDF = """<?xml version="1.0"?>
<robot name="wrist">
<link name="base"/><link name="lz"/><link name="ly"/><link name="lx"/><link name="tip"/>
<joint name="jz" type="revolute"><parent link="base"/><child link="lz"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/>
<limit lower="-2" upper="2" effort="1" velocity="1"/></joint>
<joint name="jy" type="revolute"><parent link="lz"/><child link="ly"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/>
<limit lower="-1.4" upper="1.4" effort="1" velocity="1"/></joint>
<joint name="jx" type="revolute"><parent link="ly"/><child link="lx"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/>
<limit lower="-2" upper="2" effort="1" velocity="1"/></joint>
<joint name="jtip" type="fixed"><parent link="lx"/><child link="tip"/><origin xyz="0.1 -0.2 0.3" rpy="0 0 0"/></joint>
</robot>
"""
WRIST_TIP = 3   # frame index of the fixed tip

# revolute -> prismatic -> revolute -> fixed tip, skew axes: the prismatic joint slides under a turning parent (2 w x zd u)
SANDWICH_ORDER = ["r1", "p2", "r3"]
SANDWICH_URDF = """<?xml version="1.0"?>
<robot name="sandwich">
<link name="base"/><link name="a"/><link name="b"/><link name="c"/><link name="tip"/>
<joint name="r1" type="revolute"><parent link="base"/><child link="a"/><origin xyz="0.1 0.05 0.2" rpy="0.3 -0.4 0.5"/>
<axis xyz="0.2672612419124244 0.5345224838248488 0.8017837257372732"/><limit lower="-2" upper="2" effort="1" velocity="1"/></joint>
<joint name="p2" type="prismatic"><parent link="a"/><child link="b"/><origin xyz="0.2 -0.1 0.15" rpy="-0.7 0.2 1.1"/>
<axis xyz="0.8017837257372732 -0.5345224838248488 0.2672612419124244"/><limit lower="-1" upper="1" effort="1" velocity="1"/></joint>
<joint name="r3" type="revolute"><parent link="b"/><child link="c"/><origin xyz="-0.15 0.2 0.1" rpy="1.2 0.6 -0.9"/>
<axis xyz="-0.5345224838248488 0.2672612419124244 0.8017837257372732"/><limit lower="-2" upper="2" effort="1" velocity="1"/></joint>
<joint name="jtip" type="fixed"><parent link="c"/><child link="tip"/><origin xyz="0.3 0.1 -0.2" rpy="0.4 0.5 0.6"/></joint>
</robot>
"""


class Scene:
    def __init__(self, name, path, order, seed):
        import dynamics_reference as DR
        self.name, self.path, self.order = name, path, list(order)
        self.table = U.compile_urdf(path, self.order)
        # (one identity-map leaf: the differentiation entry points use the robot table alone)
        self.desc = D.build_desc(self.table, [D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, [1.0, 0.005, 0.3])])
        self.q, self.qd, _ = DR.random_states(np.random.default_rng(seed), self.table, STATES, qd_max=QD_MAX)
        self.n_frames, self.n_dof = self.table.n_frames, self.table.n_dof


def scenes(tmp_dir):
    """The 22 random trees of dynamics_reference.random_trees(seed=0) (the 32-frame chain and the 16-dof tree among them), the
    z-y-x wrist and the prismatic sandwich, each with STATES states at |qd| <= QD_MAX."""
    import dynamics_reference as DR
    tmp_dir = str(tmp_dir)
    out = []
    for k, (path, order) in enumerate(DR.random_trees(tmp_dir, seed=0)):
        out.append(Scene(os.path.splitext(os.path.basename(path))[0], path, order, 100 + k))
    for name, text, order in (("wrist", WRIST_URDF, WRIST_ORDER), ("sandwich", SANDWICH_URDF, SANDWICH_ORDER)):
        path = os.path.join(tmp_dir, name + ".urdf")
        with open(path, "w") as f:
            f.write(text)
        out.append(Scene(name, path, order, 100 + len(out)))
    return out


def wrist_states(cys, seed=7):
    """(q, qd) [len(cys), 3] fp32 of the wrist (order jz, jy, jx) with cos(q_y) = cys[i] (q_y > 0 and < 0 alternate)."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1.5, 1.5, (len(cys), 3))
    q[:, 1] = [(-1.0) ** i * np.arccos(c) for i, c in enumerate(cys)]
    qd = rng.uniform(-QD_MAX, QD_MAX, (len(cys), 3))
    return q.astype(np.float32), qd.astype(np.float32)


def wrist_closed_form(q, qd):
    """The exact Euler map of the wrist's tip: x = (q_x, q_y, q_z), xd likewise, J the anti-diagonal permutation, c = 0."""
    q, qd = np.asarray(q, np.float64), np.asarray(qd, np.float64)
    J = np.broadcast_to(np.eye(3)[::-1], (len(q), 3, 3)).copy()
    return q[:, ::-1].copy(), qd[:, ::-1].copy(), J, np.zeros_like(q)


# ---- deviations under the scalings of the tests -----------------------------------------------------------------------------

NAMES = ("x", "xd", "J", "c")
POWERS_4X4 = (0, 0, 0, 0)
POWERS_EULER = (0, 1, 1, 2)        # a faithful fp64 evaluation: xd cy, J cy, c cy^2
POWERS_EULER_F32 = (1, 2, 2, 3)    # an fp32 evaluation loses one more power of cos theta_y


def deviation(got, ref, cy=1.0, powers=POWERS_4X4):
    """Per output: max |got - ref| cy^k / max(1, max |ref| cy^k) of one case."""
    out = []
    for g, r, k in zip(got, ref, powers):
        s = float(cy) ** k
        with np.errstate(invalid="ignore"):
            out.append(float(np.abs(np.asarray(g, np.float64) - r).max() * s / max(1.0, np.abs(r).max() * s)))
    return out


def euler_cy(x_ref):
    """|cos theta_y| of the reference's Euler angles [..., 3]."""
    return np.abs(np.cos(np.asarray(x_ref)[..., 1]))


def measure(tmp_dir, states=HOST_STATES):
    import oracle as O
    res = {"scenes": 0, "frames": 0, "states_per_scene": states, "qd_max": QD_MAX, "orthonormality_defect": 0.0,
           "cases_4x4": 0, "cases_euler": 0, "cases_euler_cy_ge_0.1": 0, "cases_euler_cy_ge_0.01": 0}
    worst = {k: [0.0] * 4 for k in ("f64_4x4", "f32_4x4", "f64_euler", "f32_euler", "f32_euler_fp32_scaling")}

    def up(key, dev):
        worst[key] = [max(a, b) for a, b in zip(worst[key], dev)]

    for sc in scenes(tmp_dir):
        res["scenes"] += 1
        res["orthonormality_defect"] = max(res["orthonormality_defect"], orthonormality_defect(sc.desc))
        consts = constants(sc.desc)
        q, qd = sc.q[:states], sc.qd[:states]
        for fr in range(sc.n_frames):
            res["frames"] += 1
            ref = differentiate_batch(sc.desc, q, qd, fr, False, consts)
            ref_e = differentiate_batch(sc.desc, q, qd, fr, True, consts)
            cy = euler_cy(ref_e[0])
            for prec in ("f64", "f32"):
                got = O.differentiate(sc.desc, q, qd, fr, prec)
                got_e = O.differentiate_euler(sc.desc, q, qd, fr, prec)
                for b in range(states):
                    up(prec + "_4x4", deviation([g[b] for g in got], [r[b] for r in ref]))
                    if cy[b] >= CY_HELD_F64:
                        up(prec + "_euler", deviation([g[b] for g in got_e], [r[b] for r in ref_e], cy[b], POWERS_EULER))
                    if prec == "f32" and cy[b] >= CY_HELD_F32:
                        up("f32_euler_fp32_scaling", deviation([g[b] for g in got_e], [r[b] for r in ref_e], cy[b], POWERS_EULER_F32))
            res["cases_4x4"] += states
            res["cases_euler"] += states
            res["cases_euler_cy_ge_0.1"] += int((cy >= CY_HELD_F64).sum())
            res["cases_euler_cy_ge_0.01"] += int((cy >= CY_HELD_F32).sum())
    for k, v in worst.items():
        res[k] = {n: float(f"{d:.3e}") for n, d in zip(NAMES, v)}
    res["orthonormality_defect"] = float(f"{res['orthonormality_defect']:.3e}")
    return res


if __name__ == "__main__":
    if "--measure" not in sys.argv[1:]:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        result = measure(tmp)
    print(json.dumps(result, indent=1))
    with open(PROFILE, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")

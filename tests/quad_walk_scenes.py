"""Robots and fleets of tests/test_gpu_quad_walk.py, and what the CPU says about them (tests/test_quad_walk_scenes.py pins it).

The walk of the quad step kernel (csrc/rmp2_quad.h kWalkAhead) fetches ahead of its use: {axis, ctl} two frames ahead, the
frame records in an even / odd rotation; the local transforms in front of it hand four frames to the four lanes of a quad.  What
can go wrong there depends on the PROGRAM the step walks -- its length against the fetch depth, where it returns to the base or
to a save slot, which joint types share a group of four frames -- so the robots here are written down as
tables, not drawn: a scene is (kinematic table, frames that carry an FK leaf), and the program follows from it (`program`, the
host's rule: ancestors of leaf frames, fixed frames without a leaf folded into their children, depth-first).

Every set is obstacle-free (clear states: q-double-dot resolves to the north-star clause of the accuracy gate) and carries
JointDamping and CSpaceBiasing, so the elimination resolves it."""
import dataclasses

import numpy as np

from quad_build_scenes import FLEETS, R_MAX   # 1, 17, 65: a lone quad, a partial wave, tail quads

SEED = 977
R, P, F = 1, 2, 0             # joint types as the tables write them below (checked against urdf.JOINT_* in _table)
SLOW_SINCOS = ((3, 0, 9000.0), (20, 2, -12000.0))   # (robot, dof, angle): beyond 8 192 rad, the library sincos under an exec mask

# the chain: 13 frames, 9 actuated dofs; frames 2 and 10 fixed (kept only under a leaf), frames 7 and 12 movable and not actuated
CHAIN_TYPES = (R, P, F, R, R, P, R, R, R, R, F, R, R)
CHAIN_DOF = (0, 1, -1, 2, 3, 4, 5, -1, 6, 7, -1, 8, -1)
CHAIN_PARENT = tuple(range(-1, 12))

# name -> (parent, joint types, dof of the frame, frames that carry an FK leaf)
ROBOTS = {
    # programs shorter than the fetch depth: every clamp active
    "len1": (CHAIN_PARENT, CHAIN_TYPES, CHAIN_DOF, (0,)),
    "len2": (CHAIN_PARENT, CHAIN_TYPES, CHAIN_DOF, (1,)),
    "len3": (CHAIN_PARENT, CHAIN_TYPES, CHAIN_DOF, (2,)),          # revolute, prismatic, fixed in one group of four
    # even and odd rotation tail; five frames = one group of four lanes and one frame
    "len4": (CHAIN_PARENT, CHAIN_TYPES, CHAIN_DOF, (3, 2)),        # revolute, prismatic, fixed, revolute
    "len5": (CHAIN_PARENT, CHAIN_TYPES, CHAIN_DOF, (4, 2)),
    # a long chain: a fourth frame for lane 0 of the local transforms (the Panda has three per lane), six full rotations and a tail
    "len13": (CHAIN_PARENT, CHAIN_TYPES, CHAIN_DOF, (12, 10, 2)),
    # no slot, back to the base on the first, second and last frame
    "forest0": ((-1, -1, 1, -1), (R, R, P, R), (0, 1, 2, 3), (0, 2, 3)),
    # one slot: saved on the first frame, restored on the last (three frames: every clamp active as well)
    "tree1a": ((-1, 0, 0), (R, R, P), (0, 1, 2), (1, 2)),
    # one slot: saved on the second frame, restored on the last
    "tree1b": ((-1, 0, 1, 1), (R, P, R, R), (0, 1, 2, 3), (2, 3)),
    # two slots: saved on the first and second frame, restored on the last two (five frames: odd tail)
    "tree2": ((-1, 0, 1, 1, 0), (R, R, R, P, R), (0, 1, 2, 3, 4), (2, 3, 4)),
}
# what `program` makes of them: (frames, save slots, restore per frame, save per frame); pinned by test_quad_walk_scenes.py
PROGRAMS = {
    "len1": (1, 0, (-2,), (-1,)),
    "len2": (2, 0, (-2, -1), (-1, -1)),
    "len3": (3, 0, (-2, -1, -1), (-1, -1, -1)),
    "len4": (4, 0, (-2, -1, -1, -1), (-1,) * 4),
    "len5": (5, 0, (-2, -1, -1, -1, -1), (-1,) * 5),
    "len13": (13, 0, (-2,) + (-1,) * 12, (-1,) * 13),
    "forest0": (4, 0, (-2, -2, -1, -2), (-1,) * 4),
    "tree1a": (3, 1, (-2, -1, 0), (0, -1, -1)),
    "tree1b": (4, 1, (-2, -1, -1, 0), (-1, 0, -1, -1)),
    "tree2": (5, 2, (-2, -1, -1, 1, 0), (0, 1, -1, -1, -1)),
}
TWO_DOF = ("two-joint", "two-joint-identity")   # the TwoJoint sets of configs.py: the two-dof template


def _table(parent, types, dof, rng):
    from riemannian_motion_policies_amd import urdf
    assert (urdf.JOINT_REVOLUTE, urdf.JOINT_PRISMATIC, urdf.JOINT_FIXED) == (R, P, F)
    n_f = len(parent)
    axis = rng.normal(size=(n_f, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    axis[::3] = np.eye(3)[np.arange(len(axis[::3])) % 3]          # every third joint about a coordinate axis
    axis[np.array(types) == F] = 0.0
    T = np.zeros((n_f, 4, 4), np.float32)
    for i in range(n_f):
        T[i, :3, :3] = urdf.rotation_from_rpy_reference_order(rng.uniform(-1.5, 1.5, 3) * (rng.random(3) < 0.6))
        T[i, :3, 3] = rng.uniform(-0.3, 0.3, 3)
        T[i, 3, 3] = 1.0
    order = [f"j{i}" for i in sorted((i for i in range(n_f) if dof[i] >= 0), key=lambda i: dof[i])]
    nan = np.full(n_f, np.nan, np.float32)
    return urdf.KinematicTable(frame_names=[f"j{i}" for i in range(n_f)], parent=np.array(parent, np.int32),
                               joint_type=np.array(types, np.int32), q_index=np.array(dof, np.int32), axis=axis.astype(np.float32),
                               T_const=T, has_collision=np.zeros(n_f, bool), order=order, link_names=[f"l{i}" for i in range(n_f)],
                               limits_lower=nan, limits_upper=nan.copy())


def program(table, leaf_frames):
    """The step's program as the host compiles it: (frames in visiting order, restore per frame, save per frame, slots)."""
    from riemannian_motion_policies_amd import urdf
    n_f = table.n_frames
    needed = np.zeros(n_f, bool)
    for f in leaf_frames:
        while f >= 0 and not needed[f]:
            needed[f] = True
            f = int(table.parent[f])
    keep = [f for f in range(n_f) if needed[f] and not (table.joint_type[f] == urdf.JOINT_FIXED and f not in leaf_frames)]
    new = {f: i for i, f in enumerate(keep)}
    parent = []
    for f in keep:
        p = int(table.parent[f])
        while p >= 0 and p not in new:
            p = int(table.parent[p])
        parent.append(new.get(p, -1))
    pruned = dataclasses.replace(table, frame_names=[table.frame_names[f] for f in keep], parent=np.array(parent, np.int32))
    order, restore, save, slots = pruned.depth_first_schedule()
    return [keep[i] for i in order], tuple(restore), tuple(save), slots


def _desc(table, leaf_frames, rng):
    from riemannian_motion_policies_amd import descriptor as D
    n = table.n_dof
    specs = [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, int(leaf_frames[0]),
                        [0.3, 0.6, 0.075, 0.05, 0.03, 1.0, 0.5, 1.0, 0.02], goal_len=3),
             D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, [1.0, 0.005, 0.3]),
             D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, [0.005, 1.0, 2.0, 0.5, 0.0001], vec_a=rng.uniform(-0.5, 0.5, n))]
    specs += [D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_FK_POSITION, int(f), [0.1, 0.5, 0.1], goal_len=3) for f in leaf_frames[1:]]
    return D.build_desc(table, specs, "auto")


def _resolved_two_joint_states(rng):
    """The first 65 of a pool of TwoJoint states that the REFERENCE resolves: the set has no inertia leaf, and near a stretched arm
    its 2 x 2 metric is so ill-conditioned that the oracle's own fp32 evaluation misses its fp64 one by more than clause A allows
    (1.5 x on one robot of the first 65 drawn).  Kept: the states where the two agree to a quarter of clause A -- decided by the
    oracle alone, as quad_build_scenes.panda_states sets its clearance."""
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    desc = Cf.config5_two_joint("auto")[1]
    pool = Cf.sample_two_joint_states(rng, 4 * R_MAX)
    a, b = (O.step(desc, pool["q"], pool["qd"], pool["goal"], precision=p, spheres=FAR)["qdd64"] for p in ("f32", "f64"))
    keep = np.nonzero(np.abs(a - b).max(axis=1) <= 0.25 * 1e-5 * np.maximum(1.0, np.abs(b).max(axis=1)))[0][:R_MAX]
    assert len(keep) == R_MAX
    return {k: np.ascontiguousarray(v[keep]) for k, v in pool.items()}


def make_sets():
    """name -> (descriptor, states of the 65-robot fleet); the smaller fleets are its first rows."""
    from riemannian_motion_policies_amd import configs as Cf
    sets = {}
    for i, (name, (parent, types, dof, leaf_frames)) in enumerate(ROBOTS.items()):
        # (the chain is one robot: the len* sets differ in their leaves alone)
        rng = np.random.default_rng(SEED if parent is CHAIN_PARENT else SEED + 1 + i)
        t = _table(parent, types, dof, rng)
        rng = np.random.default_rng(SEED + 100 + i)
        n = t.n_dof
        s = {"q": rng.uniform(-1.0, 1.0, (R_MAX, n)).astype(np.float32), "qd": rng.uniform(-0.1, 0.1, (R_MAX, n)).astype(np.float32),
             "goal": rng.uniform(-0.5, 0.5, (R_MAX, 3 * len(leaf_frames))).astype(np.float32)}
        for r, j, angle in SLOW_SINCOS:
            s["q"][r, j] = angle
        sets[name] = (_desc(t, leaf_frames, rng), s)
    rng = np.random.default_rng(SEED + 200)
    sets["two-joint"] = (Cf.config5_two_joint("auto")[1], _resolved_two_joint_states(rng))
    s = Cf.sample_two_joint_states(rng, R_MAX)
    s["goal"] = np.clip(s["q"] + rng.uniform(-0.4, 0.4, s["q"].shape), -3.0, 3.0).astype(np.float32)   # (a joint vector)
    sets["two-joint-identity"] = (Cf.exp04_two_joint("auto", with_damping=True)[1], s)
    return sets


def tables(name):
    """The robot's kinematic table and leaf frames (for `program`)."""
    parent, types, dof, leaf_frames = ROBOTS[name]
    rng = np.random.default_rng(SEED if parent is CHAIN_PARENT else SEED + 1 + list(ROBOTS).index(name))
    return _table(parent, types, dof, rng), leaf_frames


FAR = np.array([[1000.0, 0.0, 0.0, 0.1]], dtype=np.float32)   # the TwoJoint set has distance leaves: one sphere a kilometre away


def obstacle_kwargs(name):
    return {"spheres": FAR} if name == "two-joint" else {}


def system_bound(ref):
    """What tests/test_gpu_quad_builds.py test_general_flavour holds an exported M or f to (it writes the bound inline; the
    nine-dof cases of test_gpu_quad_walk.py run that function itself, this copy serves the two-dof template, whose build tag it
    does not accept)."""
    return 5e-6 * max(1.0, float(np.abs(ref).max()))

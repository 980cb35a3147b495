"""Sets of tests/test_gpu_quad_leaf_heads.py and what the CPU says about them (no GPU needed: tests/test_quad_leaf_head_scenes.py).

The four-wave plain-step builds of the quad kernel are the ones whose frame loop is reshaped for speed (csrc/rmp2_quad.h
kRegionPullback, kWalkAhead, kAncAtUse); what such a reshaping can get wrong is WHICH leaf's head -- its parameters -- or WHICH
frame's dof mask a frame works with.  A head taken from the wrong frame shows only where neighbouring leaves DIFFER and both have
pairs in range, and the cluttered set gives all eight obstacle leaves the same parameters: so the sets below give every obstacle
leaf its own, in patterns in which consecutive leaf frames repeat a head, change it and repeat it again; states, tables and lists
are those of tests/quad_build_scenes.py.

Everything is on the 9-dof Panda, with the identity leaves of the cluttered set (a symmetric set with an inertia leaf)."""
import numpy as np

import quad_build_scenes as S

FULL = np.float32(1.0000001)   # times a value: an fp32 number with low mantissa bits in use


def oa_params(i, full_mantissa=False):
    """ObstacleAvoidance parameters of variant i (0 = the cluttered set's): margin, the damping gains, P[3], P[5], the modulation
    radius P[7], P[8] and P[10] all move with i; the three length scales behind the reciprocals the host forms (P[2], P[6], P[9]) too."""
    from riemannian_motion_policies_amd import configs as Cf
    p = np.asarray(Cf.OBSTACLE_AVOIDANCE_PARAMS, dtype=np.float64).copy()
    p[0] = 0.002 * i                      # margin
    p[1] *= 1.0 + 0.10 * i                # damping_gain
    p[2] *= 1.0 + 0.05 * i                # damping_std
    p[3] *= 1.0 + 0.20 * i                # damping_robustness_eps
    p[4] *= 1.0 + 0.07 * i                # damping_velocity_gate_length_scale
    p[5] *= 1.0 + 0.05 * i                # repulsion_gain
    p[6] *= 1.0 + 0.04 * i                # repulsion_std
    p[7] -= 0.03 * i                      # metric_modulation_radius
    p[8] *= 1.0 + 0.10 * i                # metric_scalar
    p[9] *= 1.0 + 0.03 * i                # metric_exploder_std
    p[10] *= 1.0 + 0.30 * i               # metric_exploder_eps
    p = p.astype(np.float32)
    if full_mantissa:
        p = p * FULL + np.float32(0.0)
    return [float(x) for x in p]


F = {"j2": "panda_joint2", "j3": "panda_joint3", "j4": "panda_joint4", "j5": "panda_joint5", "j7": "panda_joint7",
     "hand": "panda_hand_joint", "f1": "panda_finger_joint1", "f2": "panda_finger_joint2", "grasp": "panda_grasptarget_hand"}
# set -> (FK leaves in descriptor order, solve).  ("d", frame, variant): ObstacleAvoidance; ("a", frame): TargetAttractor;
# ("p", frame): TargetPolicy on the frame's position.
SETS = {
    # every obstacle leaf its own head, the attractor last (nine leaf-bearing frames)
    "differ": ([("a", "grasp")] + [("d", f, i + 1) for i, f in enumerate(("j2", "j3", "j4", "j5", "j7", "hand", "f1", "f2"))], "auto"),
    "differ-pinv": ([("a", "grasp")] + [("d", f, 8 - i) for i, f in enumerate(("j2", "j3", "j4", "j5", "j7", "hand", "f1", "f2"))], "pinv"),
    # ... in fp32 values with every mantissa bit in use
    "differ-full": ([("a", "grasp")] + [("d", f, -(i + 1)) for i, f in enumerate(("j2", "j3", "j4", "j5", "j7", "hand", "f1", "f2"))], "auto"),
    # repeat patterns over consecutive leaf frames
    "AABA": ([("d", "j3", 1), ("d", "j4", 1), ("d", "j7", 5), ("d", "hand", 1), ("p", "grasp")], "auto"),
    "ABB": ([("p", "grasp"), ("d", "j3", 2), ("d", "j5", 6), ("d", "j7", 6)], "auto"),
    # one leaf-bearing frame, two FK leaves on it, in both orders; two frames, two different distance leaves on the first
    "one-ad": ([("a", "hand"), ("d", "hand", 3)], "auto"),
    "one-da": ([("d", "hand", 3), ("a", "hand")], "auto"),
    "two-dd": ([("d", "j7", 2), ("d", "j7", 7), ("a", "grasp")], "auto"),
    # the target leaf first, between distance frames (as a TargetPolicy), and two target leaves with their own goal offsets
    "target-first": ([("a", "j2"), ("d", "j3", 4), ("d", "j5", 4), ("d", "hand", 1)], "auto"),
    "target-between": ([("d", "j3", 4), ("p", "j5"), ("d", "j7", 4), ("d", "hand", 4)], "auto"),
    "two-targets": ([("d", "j3", 1), ("p", "j4"), ("d", "j7", 6), ("a", "grasp")], "auto"),
}
DIFFERING = ("differ", "differ-pinv", "differ-full", "AABA", "ABB", "target-first", "two-targets")
# The heads of the FK leaves in EXECUTION order (frame by frame in schedule order -- on the Panda chain: by frame index --, descriptor
# order inside a frame), one letter per distinct (kind, parameters), "|" between frames: what head_pattern() must give
PATTERN = {
    "differ": "A|B|C|D|E|F|G|H|I", "differ-pinv": "A|B|C|D|E|F|G|H|I", "differ-full": "A|B|C|D|E|F|G|H|I",
    "AABA": "A|A|B|A|C",
    "ABB": "A|B|B|C",
    "one-ad": "AB", "one-da": "AB", "two-dd": "AB|C",
    "target-first": "A|B|B|C",
    "target-between": "A|B|A|A",
    "two-targets": "A|B|C|D",
}


def specs_of(name):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf
    t = urdf.panda_table()
    fk, solve = SETS[name]
    specs = []
    for leaf in fk:
        fr = t.frame_index(F[leaf[1]])
        if leaf[0] == "a":
            specs.append(D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, fr, Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3))
        elif leaf[0] == "p":
            specs.append(D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_FK_POSITION, fr, Cf.TARGET_POLICY_PARAMS, goal_len=3))
        else:
            specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, fr, oa_params(abs(leaf[2]), leaf[2] < 0)))
    specs += [D.LeafSpec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, Cf.JOINT_VELOCITY_CAP_PARAMS),
              D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS),
              D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.CSPACE_BIASING_PARAMS, vec_a=Cf.CSPACE_BIASING_GOAL)]
    return t, specs, solve


def make_sets(tables):
    """name -> (descriptor, states of the 65-robot fleet): the Panda states of tests/quad_build_scenes.py; a second target leaf takes
    the first one's goal moved by a fixed offset."""
    from riemannian_motion_policies_amd import descriptor as D
    panda = S.panda_states(np.random.default_rng(S.SEED), tables["33"])
    out = {}
    for name in SETS:
        t, specs, solve = specs_of(name)
        desc = D.build_desc(t, specs, solve)
        goal = panda["goal"][:, :3]
        if desc.goal_floats == 6:
            goal = np.concatenate([goal, goal + np.array([0.1, -0.05, 0.08], dtype=np.float32)], axis=1)
        assert goal.shape[1] == desc.goal_floats, (name, desc.goal_floats)
        out[name] = (desc, {"q": panda["q"], "qd": panda["qd"], "goal": np.ascontiguousarray(goal.astype(np.float32))})
    return out


def head_pattern(desc):
    """The FK leaves' heads in execution order as letters (see PATTERN)."""
    from riemannian_motion_policies_amd import descriptor as D
    fk = sorted((int(desc.leaves[i].frame), i) for i in range(desc.n_leaves) if desc.leaves[i].taskmap != D.TASKMAP_IDENTITY)
    letters, out, last = {}, "", None
    for frame, i in fk:
        head = (int(desc.leaves[i].kind), tuple(np.array(list(desc.leaves[i].params), np.float32).view(np.uint32)))
        out += ("|" if last is not None and frame != last else "") + letters.setdefault(head, chr(ord("A") + len(letters)))
        last = frame
    return out


def in_range_frames(desc, s, spheres, R):
    """Frames of the set's distance leaves that have at least one pair in range on the first R robots, by the oracle's forward
    kinematics alone: |p - c| <= radius + margin + modulation radius of THAT leaf."""
    from riemannian_motion_policies_amd import descriptor as D
    org = S.origins(desc, s["q"][:R])
    sph = np.asarray(spheres, np.float64)
    frames = set()
    for c, i in enumerate(D.distance_leaf_indices(desc)):
        reach = float(desc.leaves[i].params[0]) + float(desc.leaves[i].params[7])
        d = np.linalg.norm(org[:, c, None, :] - sph[None, :, :3], axis=-1)
        if (d <= sph[None, :, 3] + reach).any():
            frames.add(int(desc.leaves[i].frame))
    return frames

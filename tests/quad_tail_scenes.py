"""Scenes of tests/test_gpu_quad_tail.py and what the CPU says about them (no GPU needed: tests/test_quad_tail_scenes.py).

The tail of the quad step -- the structured identity-leaf loop (csrc/rmp2_quad.h identity_leaves_lean), the elimination and its
certificate -- is what the four-wave builds reshape for speed (kTailOpaqueDof; tools/experiments/README.md).  What such a reshaping can get wrong is WHICH body a leaf
runs, which side of a select a lane takes, and whether a robot that must leave the fast pass (not certified, not finite) still
does.  So the scenes here walk the kinds in every order, put joint velocities on every branch of the velocity cap and
configurations on every branch of the c-space biasing, and mix certified, uncertified and non-finite robots in one wave.

Everything is on the 9-dof Panda with a target attractor and three obstacle leaves in front of the identity leaves; states, the
33-sphere table and the fleets are those of tests/quad_build_scenes.py."""
import itertools

import numpy as np

import quad_build_scenes as S

FLEETS, R_MAX = S.FLEETS, S.R_MAX
KINDS = ("damping", "cspace", "config_space", "cap")
# the weight of the configuration-space leaf of the "span" scene: with the velocity cap's diagonal d(v) it makes the identity
# part of the system w 1 1^T + (d(v) + W_SPAN - w) I, which is rank one where d(v) = w - W_SPAN (see span_states)
W_SPAN = 0.0625


def identity_specs(kinds, config_space_weight=None):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    cs = list(Cf.PANDA04_CONFIG_SPACE_BIASING_PARAMS)
    if config_space_weight is not None:
        cs[2] = config_space_weight
    table = {
        "cap": lambda: D.LeafSpec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, Cf.JOINT_VELOCITY_CAP_PARAMS),
        "damping": lambda: D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS),
        "cspace": lambda: D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.CSPACE_BIASING_PARAMS, vec_a=Cf.CSPACE_BIASING_GOAL),
        "config_space": lambda: D.LeafSpec(D.LEAF_CONFIG_SPACE_BIASING, D.TASKMAP_IDENTITY, -1, cs, vec_a=Cf.CSPACE_BIASING_GOAL),
    }
    return [table[k]() for k in kinds]


def build(kinds, solve, config_space_weight=None):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf
    t = urdf.panda_table()
    specs = [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("panda_grasptarget_hand"),
                        Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3)]
    specs += identity_specs(kinds, config_space_weight)
    for fr in Cf.CONTROL_POINT_FRAMES[:3]:
        specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr), Cf.OBSTACLE_AVOIDANCE_PARAMS))
    return D.build_desc(t, specs, solve)


def build_general(which, solve):
    """Symmetric sets that the four-wave lean builds send through the GENERAL identity loop, the cold side of the branch between the
    two loops: "dense" -- damping, the cap and a TargetPolicy on the identity map (a dense symmetric metric: the set is not structured);
    "arm7" -- the cap, damping and configuration-space biasing on the Panda's seven arm joints (fewer dofs than the nine-dof template:
    the loop's row and column tests against n_dof cut two padding rows)."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf
    t = urdf.panda_table() if which == "dense" else urdf.compile_urdf(urdf.PANDA_URDF, urdf.PANDA_ORDER[:7])
    n = t.n_dof
    specs = [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("panda_grasptarget_hand"),
                        Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3)]
    if which == "dense":
        specs += identity_specs(("damping", "cap"))
        specs.append(D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_IDENTITY, -1, Cf.PANDA04_TARGET_POLICY_PARAMS, goal_len=n))
    else:
        specs += [D.LeafSpec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, Cf.JOINT_VELOCITY_CAP_PARAMS),
                  D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS),
                  D.LeafSpec(D.LEAF_CONFIG_SPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.PANDA04_CONFIG_SPACE_BIASING_PARAMS,
                             vec_a=Cf.CSPACE_BIASING_GOAL[:7])]
    for fr in Cf.CONTROL_POINT_FRAMES[:3]:
        specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr), Cf.OBSTACLE_AVOIDANCE_PARAMS))
    return D.build_desc(t, specs, solve)


GENERAL_LOOP = ("general-dense", "general-arm7")   # scenes of the general identity loop in the lean builds


def cap_constants():
    """(cutoff, rlimit, P[1]) as the fp32 values the kernel and the oracle form (csrc/rmp2_device.h IdLeafRec)."""
    from riemannian_motion_policies_amd import configs as Cf
    p = np.array(Cf.JOINT_VELOCITY_CAP_PARAMS, np.float32)
    return np.float32(p[0] - p[1]), np.float32(p[1] - np.float32(1e-6)), p[1]


def cap_branches(qd):
    """Per (robot, joint), from the fp32 intermediates of rmp2.py:100-112: which side of every select of the velocity cap it takes."""
    cutoff, rlimit, _ = cap_constants()
    a = np.abs(qd.astype(np.float32))
    dv = (a - cutoff).astype(np.float32)
    # (dv == rlimit itself cannot happen with the cluttered set's parameters: |qd| and the cutoff 0.35 are multiples of 2^-25, so is
    # their difference, and rlimit = 0.15 - 1e-6 is an odd multiple of 2^-26.  "at" is the last fp32 step in front of the clamp.)
    return {"below": a < cutoff, "at": a == cutoff, "above": a > cutoff,
            "dv_at_rlimit": (dv <= rlimit) & (rlimit - dv < np.float32(3e-8)), "dv_beyond_rlimit": dv > rlimit,
            "zero": qd == 0, "negative": qd < 0, "positive": qd > 0}


def cspace_norm(q):
    """|q - goal| of the c-space biasing leaf in fp32, summed in the kernel's order."""
    from riemannian_motion_policies_amd import configs as Cf
    e = q.astype(np.float32) - np.array(Cf.CSPACE_BIASING_GOAL, np.float32)
    s2 = np.zeros(len(q), np.float32)
    for j in range(e.shape[1]):
        s2 = (s2 + e[:, j] * e[:, j]).astype(np.float32)
    return np.sqrt(s2).astype(np.float32)


def cap_branches_from_oracle(s):
    """The same sides, read off the ORACLE's reference-precision system of the velocity cap alone (its only leaf): the diagonal of M
    is the leaf's d_i = P[3] / (1 - ratio_i^2) and xo = M^-1 f its acceleration (rmp2.py:100-112).  d_i == P[3]: the joint is exactly at
    the cutoff (ratio 0); xo_i != 0: above it; otherwise below (at the cutoff the acceleration is -|P[2] * 0| = 0 as well); d_i equal
    to the diagonal of a probe joint far beyond the clamp: the clamp was taken; within a factor two under it: the last steps in front."""
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf
    desc = D.build_desc(urdf.panda_table(), identity_specs(("cap",)), "auto")
    probe = np.full((1, 9), 0.9, np.float32)
    q, qd = np.concatenate([s["q"], s["q"][:1]]), np.concatenate([s["qd"], probe])
    r = O.step(desc, q, qd)
    dg = np.diagonal(r["M"], axis1=1, axis2=2)
    xo = np.linalg.solve(r["M"], r["f"][..., None])[..., 0]
    clamp, w = dg[-1, 0], np.float64(np.float32(Cf.JOINT_VELOCITY_CAP_PARAMS[3]))
    dg, xo = dg[:-1], xo[:-1]
    at, above = dg == w, np.abs(xo) > 1e-6   # (f carries fp32 roundings of ~1e-7: the solve returns that for a zero)
    return {"below": ~at & ~above, "at": at, "above": above, "dv_at_rlimit": (dg < clamp) & (dg > 0.5 * clamp), "dv_beyond_rlimit": dg == clamp,
            "pushes_back": (np.sign(xo) == -np.sign(s["qd"]))[above].all()}


def cspace_sides_from_oracle(s):
    """Which side of the c-space leaf's select a robot takes, read off the oracle's system of that leaf alone: f_i = m (pos_i - P[2] qd_i),
    and |pos| is 0 at the goal, P[1] |q - goal| below the threshold and the constant P[1] P[3] beyond it (rmp2.py:212-226)."""
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf
    desc = D.build_desc(urdf.panda_table(), identity_specs(("cspace",)), "auto")
    r = O.step(desc, s["q"], s["qd"])
    P = Cf.CSPACE_BIASING_PARAMS
    pos = r["f"] / (P[0] + P[4]) + P[2] * s["qd"].astype(np.float64)
    pn = np.linalg.norm(pos, axis=1)
    far = np.abs(pn - P[1] * P[3]) < 1e-5
    return {"zero": pn < 1e-6, "near": (pn >= 1e-6) & ~far & (pn < P[1] * P[3]), "far": far}


def cap_edge_states(base):
    """Joint velocities on every branch of the cap, in a cycle of eight robots: all joints below the cutoff; one joint exactly at
    it (either sign); above it; dv on the last fp32 step in front of rlimit; beyond it (the clamp); all zero (sgn = 0); negative above the cutoff; the
    sampled velocities."""
    cutoff, rlimit, _ = cap_constants()
    at_rlimit = np.float32(cutoff + rlimit)
    while np.float32(at_rlimit - cutoff) > rlimit:   # the largest speed whose dv the clamp leaves alone
        at_rlimit = np.nextafter(at_rlimit, np.float32(0), dtype=np.float32)
    qd = base["qd"].copy()
    for r in range(len(qd)):
        j, sg = r % 9, np.float32(1 - 2 * ((r // 8) % 2))
        k = r % 8
        if k == 0:
            qd[r] = np.float32(0.3) * np.where(np.arange(9) % 2 == 0, 1, -1)
        elif k == 1:
            qd[r, j] = sg * cutoff
        elif k == 2:
            qd[r, j] = sg * np.float32(0.4)
        elif k == 3:
            qd[r, j] = sg * at_rlimit
        elif k == 4:
            qd[r, j] = sg * np.float32(0.6)
        elif k == 5:
            qd[r] = 0
        elif k == 6:
            qd[r] = -np.float32(0.45)
    return {"q": base["q"], "qd": np.ascontiguousarray(qd.astype(np.float32)), "goal": base["goal"]}


def cspace_edge_states(base):
    """Configurations on both sides of the c-space leaf's threshold P[3] = 0.5 and AT the goal (norm 0: the far side of the select is
    0 / 0 there), in a cycle of five robots: the goal itself; a step of norm 0.2 from it; 0.49; 0.51; the sampled state."""
    from riemannian_motion_policies_amd import configs as Cf
    goal = np.array(Cf.CSPACE_BIASING_GOAL, np.float32)
    q = base["q"].copy()
    rng = np.random.default_rng(S.SEED + 5)
    for r in range(len(q)):
        k = r % 5
        if k == 4:
            continue
        d = rng.normal(size=9)
        d /= np.linalg.norm(d)
        q[r] = goal + (np.float32((0.0, 0.2, 0.49, 0.51)[k]) * d).astype(np.float32)
    return {"q": np.ascontiguousarray(q.astype(np.float32)), "qd": base["qd"], "goal": base["goal"]}


def cap_diagonal(v):
    from riemannian_motion_policies_amd import configs as Cf
    p = Cf.JOINT_VELOCITY_CAP_PARAMS
    r = min(abs(v) - (p[0] - p[1]), p[1] - 1e-6) / p[1]
    return p[3] / (1.0 - r * r)


SPAN_DELTAS = (1e-1, -1e-1, 1e-2, -1e-2, 1e-3, -1e-3, 1e-4, -1e-4, 1e-5, -1e-5, 3e-2, -3e-2, 3e-3, -3e-3, 3e-4, -3e-4)


def span_states(base):
    """Every joint of robot r moves at the speed v_r (alternating signs) at which the velocity cap's diagonal d(v) -- negative below
    its pole, quirk Q4 -- leaves delta_r = d(v_r) + W_SPAN - w on the diagonal of the identity part w 1 1^T + delta I: sixteen
    values from 1e-1 down to 1e-5 of either sign in every wave.  Positive: positive definite, from well conditioned to a
    condition number of ~1e6; negative: indefinite, the elimination without row exchanges meets negative pivots and large multipliers,
    and the certificate of the strict step turns the robot away."""
    from riemannian_motion_policies_amd import configs as Cf
    w = Cf.JOINT_VELOCITY_CAP_PARAMS[3]
    qd = base["qd"].copy()
    for r in range(len(qd)):
        want = SPAN_DELTAS[r % 16]
        lo, hi = 0.0, 0.19   # d(v) falls from -0.0113 at v = 0 to -inf at the pole v = 0.2
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if cap_diagonal(mid) + W_SPAN - w > want:
                lo = mid
            else:
                hi = mid
        qd[r] = np.float32(lo) * np.where(np.arange(9) % 2 == 0, 1, -1)
    return {"q": base["q"], "qd": np.ascontiguousarray(qd.astype(np.float32)), "goal": base["goal"]}


SMALL_PIVOT = 2e-4   # M[0][0] of every fourth robot of the span fleet


def small_first_pivot(desc, s, kw):
    """Every fourth robot of the span fleet: the speed of joint 0 alone is moved until the velocity cap's (negative) diagonal
    leaves M[0][0] = SMALL_PIVOT.  The system stays indefinite and as well conditioned as its neighbours', but the elimination
    without row exchanges starts from a pivot 250 times smaller than the column under it: multipliers beyond 64 and negative pivots
    behind them, which the certificate of the strict step does not accept -- such a robot takes the careful pass, and its wave with
    it, while the fifteen others of the wave are settled in the fast one.  (A condition number large enough to fail the certificate
    -- about 1e10 -- cannot be had from these leaves short of fp32 noise: the identity part would have to cancel to 1e-11.)"""
    import oracle as O
    qd = s["qd"].copy()
    M00 = O.step(desc, s["q"], qd, s["goal"], **kw)["M"][:, 0, 0]
    for r in range(3, len(qd), 4):
        want = SMALL_PIVOT - (M00[r] - cap_diagonal(float(qd[r, 0])))
        lo, hi = 0.0, 0.1999   # d(v) falls from -0.0113 at v = 0 to -inf at the pole v = 0.2
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if cap_diagonal(mid) > want else (lo, mid)
        qd[r, 0] = np.float32(lo)
    return {"q": s["q"], "qd": np.ascontiguousarray(qd.astype(np.float32)), "goal": s["goal"]}


NAN_ROBOT, INF_ROBOT = 5, 9


def nonfinite_states(base):
    q, qd = base["q"].copy(), base["qd"].copy()
    q[NAN_ROBOT, 2] = np.nan
    qd[INF_ROBOT, 4] = np.inf
    return {"q": q, "qd": qd, "goal": base["goal"]}


def order_sets():
    """name -> kinds: each kind alone, every order of two and of three different kinds, and four leaves with one kind twice."""
    out = {"+".join(k): k for n in (1, 2, 3) for k in itertools.permutations(KINDS, n)}
    out["damping+cap+damping+cspace"] = ("damping", "cap", "damping", "cspace")
    return out


CONFIG3 = ("cap", "damping", "cspace")   # the identity leaves of the cluttered set, in its order


def make_scenes():
    """name -> dict(desc, s = states of the 65-robot fleet, kw = obstacle arguments (numpy), solve)."""
    from riemannian_motion_policies_amd import configs as Cf
    tables = S.make_tables()
    base = S.panda_states(np.random.default_rng(S.SEED), tables["33"])
    base = {k: np.ascontiguousarray(v[:, :3] if k == "goal" else v) for k, v in base.items()}
    near, far = {"spheres": tables["33"]}, {"spheres": tables["far"]}
    out = {}
    for i, (name, kinds) in enumerate(order_sets().items()):
        solve = ("auto", "pinv")[i % 2]
        out[name] = dict(desc=build(kinds, solve), s=base, kw=near, solve=solve)
    # the edge states keep away from the table: what they probe is the identity leaves
    out["cap-edges"] = dict(desc=build(CONFIG3, "auto"), s=cap_edge_states(base), kw=far, solve="auto")
    out["cap-edges-pinv"] = dict(desc=build(("cap", "config_space"), "pinv"), s=cap_edge_states(base), kw=far, solve="pinv")
    out["cspace-edges"] = dict(desc=build(("cspace", "damping"), "pinv"), s=cspace_edge_states(base), kw=far, solve="pinv")
    for name, kinds, solve in (("span", ("cap", "config_space"), "pinv"), ("span-auto", ("config_space", "cap"), "auto")):
        desc = build(kinds, solve, W_SPAN)
        out[name] = dict(desc=desc, s=small_first_pivot(desc, span_states(base), far), kw=far, solve=solve)
    out["nonfinite"] = dict(desc=build(CONFIG3, "pinv"), s=nonfinite_states(base), kw=near, solve="pinv")
    # the general identity loop in the lean builds; the velocities of the cap's edges, so that its row tests meet every branch
    edge = cap_edge_states(base)
    qg = np.clip(base["q"] + np.random.default_rng(S.SEED + 7).uniform(-0.4, 0.4, base["q"].shape), Cf.PANDA_Q_LOW, Cf.PANDA_Q_HIGH)
    dense = {"q": edge["q"], "qd": edge["qd"], "goal": np.ascontiguousarray(np.concatenate([base["goal"], qg], axis=1).astype(np.float32))}
    arm = {"q": np.ascontiguousarray(edge["q"][:, :7]), "qd": np.ascontiguousarray(edge["qd"][:, :7]), "goal": base["goal"]}
    out["general-dense"] = dict(desc=build_general("dense", "auto"), s=dense, kw=far, solve="auto")
    out["general-arm7"] = dict(desc=build_general("arm7", "pinv"), s=arm, kw=far, solve="pinv")
    return out


def references(scene):
    """(fp64 evaluation, fp32 envelope, reference-precision evaluation) of the 65-robot fleet, as tests/test_gpu_quad_builds.py
    takes them."""
    import oracle as O
    d, s, kw = scene["desc"], scene["s"], scene["kw"]
    return (O.step(d, s["q"], s["qd"], s["goal"], precision="f64", **kw), O.fp32_envelope(d, s["q"], s["qd"], s["goal"], **kw),
            O.step(d, s["q"], s["qd"], s["goal"], **kw))

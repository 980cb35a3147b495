"""The leaf policies at their branch points and poles: the catalogue of edge rows and its yardsticks (no test functions).

Every leaf formula exists in several hand-written copies (the lane-per-robot step and rmp2_leaf_kernel on rmp2_device.h's leaf_*
functions, the quad mapping's general and structured identity loops and its fast pair leaves, the hex mapping), and random states
meet `x == goal`, `qd == 0`, `q == limit`, `d == 0` or `|qd| == cutoff - region` with probability zero.  This module writes those
states down, one FLEET of R = 130 robots per leaf kind (a partial last wave at 64, 16 and 4 robots per wave), on three robots:

  panda      urdf.panda_table(), the full width of the 9-dof template
  gantry     tests/link_pair_scene.py: 4 dofs, world positions exact in fp32 -- tip = (qx + 0.5, qy, 0.75 + qz)
  two_joint  the planar arm of the 2-dof template

Edge rows sit one per hex group of four robots (slot k at row 4 k + (3 k + 1) % 4: every position of a group is used), between
seeded ordinary rows; `Fleet.inputs(plain=True)` is the same fleet with every edge row replaced by an ordinary one (the isolation tests).
(130 rows are nine quad waves of 16, fewer than any fleet has edge rows: edge rows do share a quad wave -- about four each, pole rows
beside others; what one row can do to another of its wave is what the isolation tests look at -- except in joint_limits_band_free,
which has ONE edge row per quad wave.  "Per joint" is read as one joint per case, in rotation (case k on joint k % n):
JointLimitAvoidance has every joint at its lower and at its upper limit, the band edge on joints 0, 3, 5, 7 and 0.3 rad beyond a limit
on joints 1, 4, 8.)  Every input is formed in np.float32 arithmetic from the fp32 parameters the descriptor stores, so that an fp32 and an fp64
evaluation see the same side of every branch.

Classes, decided on the oracle alone (classify): `pole` -- both oracle builds return a non-finite system or qdd; `regular` -- the
fp32-leaf build passes clause A or B of oracle.accuracy_gate against the fp64 build; `stiff` -- finite in both, outside A and B.
The class each row is EXPECTED in is written here (Fleet.expect); tests/test_leaf_edges_host.py fails when a row lands elsewhere.

Set shapes: `alone` -- the leaf on its own, the exported system is the leaf's own pulled-back (J^T A J, J^T A (xdd - Jd qd)) --
and `damped` -- the leaf beside JointDamping: full rank, the elimination paths and (structured kinds on the Panda) the lean loop.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import link_pair_scene as S  # noqa: E402

F32 = np.float32
R = 130
SHAPES = ("alone", "damped")


def steps(x, k):
    """x moved by k fp32 steps away from zero (k < 0: towards it); x != 0."""
    x = F32(x)
    return (x.view(np.int32) + np.int32(k)).view(F32)


def slot(k):
    """Row of the k-th edge case: one per hex group of 4, every position of a group in turn."""
    row = 4 * k + (3 * k + 1) % 4
    assert row < R, "more edge rows than hex groups"
    return row


# ---- robots ------------------------------------------------------------------------------------------------------------------
_TABLES = {}


def table(robot):
    if robot not in _TABLES:
        from riemannian_motion_policies_amd import urdf as U
        _TABLES[robot] = {"panda": U.panda_table, "two_joint": U.two_joint_table,
                          "gantry": lambda: U.compile_urdf(S.gantry_urdf_path(), S.GANTRY_ORDER)}[robot]()
    return _TABLES[robot]


def gantry_golden():
    """The gantry as the autograd oracle's kinematics takes it (the layout of tests/golden/kinematic_tables.json)."""
    names = ["jx", "jy", "jz", "jr", "tip"]
    return {"frame_names": names, "order": S.GANTRY_ORDER, "backward_paths": [names[:i + 1] for i in range(5)],
            "q_reordering": [0, 1, 2, 3, 4], "rpy": [[0.0, 0.0, 0.0]] * 5,
            "xyz": [[0, 0, 0.5], [0, 0, 0.25], [0, 0, 0], [0, 0, 0], [0.5, 0, 0]],
            "axis": [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 0]],
            "joint_type": ["prismatic", "prismatic", "prismatic", "revolute", "fixed"]}


def _limits(robot):
    from riemannian_motion_policies_amd import configs as Cf
    if robot == "panda":
        return np.asarray(Cf.PANDA_Q_LOW, F32), np.asarray(Cf.PANDA_Q_HIGH, F32)
    if robot == "two_joint":
        return np.asarray(Cf.TWO_JOINT_Q_LOW, F32), np.asarray(Cf.TWO_JOINT_Q_HIGH, F32)
    # (jr stays at 0, with a velocity: the tip's Jacobian column of jr is then EXACTLY half that of jy, in fp32 as in fp64, and both
    #  oracle builds drop the same singular value of a position leaf's rank-3 system on the gantry's 4 dofs)
    return np.asarray([-0.75, -0.25, -0.25, 0.0], F32), np.asarray([0.0, 0.25, 0.25, 0.0], F32)


def ordinary(robot, rng, rows, qd_max=0.1):
    """Seeded ordinary states: every joint in the middle 60 % of its range (outside every limit band), |qd| <= qd_max."""
    lo, hi = _limits(robot)
    span = hi - lo
    q = rng.uniform(lo + F32(0.2) * span, hi - F32(0.2) * span, (rows, len(lo))).astype(F32)
    qd = rng.uniform(-qd_max, qd_max, (rows, len(lo))).astype(F32)
    return q, qd


# ---- fleets ------------------------------------------------------------------------------------------------------------------
class Fleet:
    """One leaf kind's fleet.  specs(): the leaf's LeafSpec list (`alone`); q, qd, goal [R, .] fp32; obs: obstacle keyword arguments
    (numpy, as oracle.step takes them; engine.obstacles takes the same names); names[R] ('' on ordinary rows); expect: name -> class
    or (class alone, class damped); groups: name of an exact-structure property -> row indices."""

    def __init__(self, key, robot, kinds, specs, q, qd, goal=None, obs=None):
        self.key, self.robot, self.kinds, self._specs = key, robot, tuple(kinds), specs
        self.q0, self.qd0 = q.copy(), qd.copy()
        self.goal0 = None if goal is None else goal.copy()
        self.q, self.qd, self.goal = q, qd, goal
        self.obs = dict(obs or {})
        self.names = [""] * R
        self.expect = {}
        self.groups = {}
        self._k = 0
        self.shapes = SHAPES
        self.n = q.shape[1]

    def add(self, name, expect, q=None, qd=None, goal=None, groups=(), joint=None, row=None):
        """The next edge row.  q / qd / goal: a full row, or with `joint` the value of that joint alone (the rest stays ordinary)."""
        i = slot(self._k) if row is None else row
        self._k += row is None
        assert not self.names[i] and name not in self.expect, name
        for arr, val in ((self.q, q), (self.qd, qd), (self.goal, goal)):
            if val is None:
                continue
            if joint is None:
                arr[i] = np.asarray(val, F32)
            else:
                arr[i, joint] = F32(val)
        self.names[i] = name
        self.expect[name] = expect
        for g in groups:
            self.groups.setdefault(g, []).append(i)
        return i

    @property
    def edge(self):
        return np.array([bool(n) for n in self.names])

    def row(self, name):
        return self.names.index(name)

    def expected(self, shape):
        out = []
        for n in self.names:
            e = self.expect.get(n, "regular")
            out.append(e if isinstance(e, str) else e[SHAPES.index(shape)])
        return np.array(out)

    def specs(self, shape):
        from riemannian_motion_policies_amd import configs as Cf, descriptor as D
        sp = list(self._specs)
        if shape == "damped":
            sp.append(D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping"))
        return sp

    def desc(self, shape, solve="auto"):
        from riemannian_motion_policies_amd import descriptor as D
        return D.build_desc(table(self.robot), self.specs(shape), solve)

    def obstacles(self, plain=False):
        """Obstacle keyword arguments of the fleet (explicit pairs follow the rows: the plain fleet has its own)."""
        return getattr(self, "obs_plain", self.obs) if plain else self.obs

    def inputs(self, plain=False):
        """(q, qd, goal): the fleet, or with plain=True the same fleet with every edge row replaced by an ordinary one."""
        return (self.q0, self.qd0, self.goal0) if plain else (self.q, self.qd, self.goal)


def _spec(kind, taskmap, frame, params, **kw):
    from riemannian_motion_policies_amd import descriptor as D
    return D.LeafSpec(kind, taskmap, frame, params, **kw)


def velocity_cap(robot="panda", seed=101):
    """JointVelocityCap(0.5, 0.15, 5, 0.05): cutoff = fp32(0.5 - 0.15); quirk Q4's pole where |qd| - cutoff == -0.15 in fp32 (the
    clipped ratio is -1, 1 / (1 - ratio^2) = 1 / 0)."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    P = [F32(p) for p in Cf.JOINT_VELOCITY_CAP_PARAMS]
    cutoff = F32(P[0] - P[1])
    pole = F32(cutoff - P[1])
    assert F32(pole - cutoff) == -P[1]
    rng = np.random.default_rng(seed)
    q, qd = ordinary(robot, rng, R)
    n = q.shape[1]
    # ordinary rows of THIS fleet: each joint below the cutoff (|qd| <= 0.15) or beyond it (0.25 .. 0.45), clear of the pole
    mag = np.where(rng.random((R, n)) < 0.5, rng.uniform(0.0, 0.15, (R, n)), rng.uniform(0.25, 0.45, (R, n)))
    qd[:] = (mag * rng.choice([-1.0, 1.0], (R, n))).astype(F32)
    fl = Fleet("velocity_cap" + ("" if robot == "panda" else "_" + robot), robot, [D.LEAF_JOINT_VELOCITY_CAP],
               [_spec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, Cf.JOINT_VELOCITY_CAP_PARAMS, name="cap")], q, qd)
    below = rng.uniform(-0.1, 0.1, (R, n)).astype(F32)   # the other joints of a single-joint row: below the cutoff
    cases = [("zero_pos", F32(0.0), "regular"), ("zero_neg", F32(-0.0), "regular"),
             ("cutoff_pos", cutoff, "regular"), ("cutoff_neg", -cutoff, "regular"),
             ("cutoff_below", steps(cutoff, -1), "regular"), ("cutoff_above", steps(cutoff, 1), "regular"),
             ("cutoff_neg_below", -steps(cutoff, -1), "regular"), ("cutoff_neg_above", -steps(cutoff, 1), "regular"),
             ("pole", pole, "pole"), ("pole_neg", -pole, "pole"),
             # (the pole's neighbours and the clipped ratio: the metric is steep there -- |M| = 2.5e5 one step beside the pole, the
             #  fp32-leaf build 17 % off the fp64 one; 3.75e3 beyond vmax -- but diagonal, and qdd = f / M keeps clause A: regular)
             ("pole_minus_1", steps(pole, -1), "regular"), ("pole_plus_1", steps(pole, 1), "regular"),
             ("pole_minus_1024", steps(pole, -1024), "regular"), ("pole_plus_1024", steps(pole, 1024), "regular"),
             ("vmax", P[0], "regular"), ("beyond_vmax", F32(0.6), "regular"), ("beyond_vmax_neg", F32(-0.6), "regular")]
    for k, (name, v, cls) in enumerate(cases):
        j = k % n
        i = fl.add(name, cls, qd=below[slot(fl._k)])
        fl.qd[i, j] = v
        if abs(float(v)) < float(cutoff) and cls != "pole":
            fl.groups.setdefault("below_cutoff", []).append(i)
    fl.add("all_at_cutoff", "regular", qd=np.full(n, cutoff, F32) * np.where(np.arange(n) % 2, -1, 1).astype(F32))
    fl.add("all_beyond", "regular", qd=np.linspace(0.36, 0.45, n).astype(F32))
    fl.add("all_at_rest", "regular", qd=np.zeros(n, F32), groups=["below_cutoff"])
    fl.add("all_below", "regular", qd=below[0], groups=["below_cutoff"])
    return fl


def joint_damping(seed=102):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    rng = np.random.default_rng(seed)
    q, qd = ordinary("panda", rng, R)
    fl = Fleet("joint_damping", "panda", [D.LEAF_JOINT_DAMPING],
               [_spec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping")], q, qd)
    fl.shapes = ("alone",)          # (beside itself it is the same leaf twice: nothing another shape would take elsewhere)
    z = np.zeros(9, F32)
    fl.add("at_rest", "regular", qd=z, groups=["at_rest"])
    fl.add("at_rest_neg_zero", "regular", qd=-z, groups=["at_rest"])
    # (|qd|^2 = 1e-40 is a DENORMAL, |qd| = 1e-20: what v_rsq_f32 takes for 0; at 1e-30 and 1e-38 the square underflows to 0 and so does the norm)
    for j, v in ((0, 1e-20), (4, 1e-30), (8, -1e-20), (6, 1e-38)):
        e = z.copy()
        e[j] = F32(v)
        fl.add(f"joint{j}_at_{v:g}", "regular", qd=e)
    return fl


def cspace_biasing(seed=103):
    """CSpaceBiasing(ms, kp, kd, threshold 0.5, inertia): the position term switches at |q - goal| == threshold; at q == goal the
    unit vector of the far branch is 0 / 0, and the near branch must be the one chosen."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    rng = np.random.default_rng(seed)
    q, qd = ordinary("panda", rng, R)
    g = np.asarray(Cf.CSPACE_BIASING_GOAL, F32)
    q[:] = (g + rng.uniform(-0.3, 0.3, (R, 9)) * (rng.random((R, 1)) < 0.5) + rng.uniform(-0.1, 0.1, (R, 9))).astype(F32)
    fl = Fleet("cspace_biasing", "panda", [D.LEAF_CSPACE_BIASING],
               [_spec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.CSPACE_BIASING_PARAMS, vec_a=Cf.CSPACE_BIASING_GOAL, name="cspace")], q, qd)
    th = F32(Cf.CSPACE_BIASING_PARAMS[3])
    fl.add("at_goal", "regular", q=g)
    fl.add("at_goal_at_rest", "regular", q=g, qd=np.zeros(9, F32))
    for j in (0, 2, 4):        # goal[j] == 0: q[j] = +-threshold is |e| == threshold exactly, on a single joint
        for name, v in (("at", th), ("below", steps(th, -1)), ("above", steps(th, 1))):
            e = g.copy()
            e[j] = v if j != 2 else -v
            fl.add(f"threshold_{name}_joint{j}", "regular", q=e)
    e = g.copy()
    e[0], e[2] = F32(0.3), F32(0.4)      # |e| = fp32 sqrt(0.09 + 0.16): the threshold from two joints, to a rounding
    fl.add("threshold_two_joints", "regular", q=e)
    return fl


def config_space_biasing(seed=104):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    rng = np.random.default_rng(seed)
    q, qd = ordinary("panda", rng, R)
    g = np.asarray(Cf.PANDA04_Q0, F32)
    fl = Fleet("config_space_biasing", "panda", [D.LEAF_CONFIG_SPACE_BIASING],
               [_spec(D.LEAF_CONFIG_SPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.PANDA04_CONFIG_SPACE_BIASING_PARAMS, vec_a=Cf.PANDA04_Q0, name="csb")], q, qd)
    fl.add("at_goal", "regular", q=g)
    fl.add("at_rest", "regular", qd=np.zeros(9, F32))
    fl.add("at_goal_at_rest", "regular", q=g, qd=np.zeros(9, F32), groups=["zero_force"])
    fl.add("beside_goal", "regular", q=g + F32(2.0 ** -20))
    return fl


BAND = F32(0.15)    # rmp.py:333: the spline's support, as a fraction of the joint's range


def joint_limits(robot="panda", band_free=False, coincide=None, seed=105):
    """JointLimitAvoidance on the Panda's limits.  d = min(hi - q, q - lo) / (hi - lo); the weight is a cubic spline on d <= 0.15 with a
    double root at 0.15 and an exact 0 beyond: the COLUMN of a joint outside its band is exactly 0 (quirk Q2: the weight scales columns).
    band_free: every ordinary row is outside every band, and ONE row per quad wave of 16 is inside the band of one joint -- the
    wave-wide column skip of the quad mapping's general loop (rmp2_quad.h: __any(cw[j] != 0)).
    coincide = j: the descriptor's limits of joint j coincide (vec_a[j] == vec_b[j]): 0 / 0 on every row."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    rng = np.random.default_rng(seed)
    lo, hi = _limits(robot)
    n = len(lo)
    q, qd = ordinary(robot, rng, R)
    if not band_free:     # ordinary rows anywhere in the range: about a quarter of the joints inside a band
        q[:] = rng.uniform(lo + F32(0.02) * (hi - lo), hi - F32(0.02) * (hi - lo), (R, n)).astype(F32)
    va, vb = lo.copy(), hi.copy()
    if coincide is not None:
        vb[coincide] = va[coincide]
    key = "joint_limits" + ("_band_free" if band_free else "") + ("_coincide" if coincide is not None else "")
    fl = Fleet(key, robot, [D.LEAF_JOINT_LIMIT_AVOIDANCE],
               [_spec(D.LEAF_JOINT_LIMIT_AVOIDANCE, D.TASKMAP_IDENTITY, -1, Cf.JOINT_LIMIT_PARAMS, vec_a=va, vec_b=vb, name="limits")], q, qd)
    fl.lo, fl.hi = lo, hi
    if coincide is not None:     # d = 0 / 0 on joint `coincide` of EVERY row
        fl.names = [f"row{i}" for i in range(R)]
        fl.expect = {n: "pole" for n in fl.names}
        return fl
    if band_free:
        for w in range((R + 15) // 16):
            j = w % n
            row = min(16 * w + (5 * w + 3) % 16, R - 1)
            span = hi[j] - lo[j]
            fl.add(f"wave{w}_joint{j}_in_band", "regular", q=(lo[j] + F32(0.05) * span) if w % 2 else (hi[j] - F32(0.05) * span), joint=j, row=row)
        return fl
    for j in range(n):
        fl.add(f"joint{j}_at_lower", "regular", q=lo[j], joint=j)
        fl.add(f"joint{j}_at_upper", "regular", q=hi[j], joint=j)
    for j in (0, 3, 5, 7):
        span = hi[j] - lo[j]
        # (the weight has a double root at the band's edge: 1e-14 on one side, an exact 0 on the other, and the side hangs on the
        #  rounding of d.  Alone, the joint's column is the system's only one with that row: the rank flips between faithful
        #  evaluations and qdd with it -- stiff; beside the damping leaf the flip is 1e-14 of the metric)
        fl.add(f"joint{j}_band_edge", "regular" if j == 3 else ("stiff", "regular"), q=(lo[j] + BAND * span) if j % 2 else (hi[j] - BAND * span), joint=j)
    for j in (1, 4, 8):
        fl.add(f"joint{j}_beyond", "regular", q=(lo[j] - F32(0.3)) if j % 2 else (hi[j] + F32(0.3)), joint=j)
    fl.add("all_at_lower", "regular", q=lo)
    fl.add("all_at_upper", "regular", q=hi)
    fl.add("at_rest", "regular", qd=np.zeros(n, F32))
    mid = ((lo + hi) * F32(0.5)).astype(F32)
    fl.add("mid_range_at_rest", "regular", q=mid, qd=np.zeros(n, F32), groups=["zero_system"])
    fl.add("mid_range", "regular", q=mid, groups=["zero_metric"])
    return fl


def target_policy_identity(seed=106):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    rng = np.random.default_rng(seed)
    q, qd = ordinary("panda", rng, R)
    goal = (q + rng.uniform(-0.4, 0.4, q.shape)).astype(F32)
    fl = Fleet("target_policy_identity", "panda", [D.LEAF_TARGET_POLICY],
               [_spec(D.LEAF_TARGET_POLICY, D.TASKMAP_IDENTITY, -1, Cf.PANDA04_TARGET_POLICY_PARAMS, goal_len=9, name="target")], q, qd, goal)
    z = np.zeros(9, F32)
    for k in range(3):
        i = fl.add(f"at_goal_{k}", "regular")
        fl.goal[i] = fl.q[i]
    fl.add("at_rest", "regular", qd=z)
    i = fl.add("at_goal_at_rest", "regular", qd=z, groups=["identity_metric_zero_force"])
    fl.goal[i] = fl.q[i]
    i = fl.add("beside_goal", "regular")
    fl.goal[i] = fl.q[i] + F32(2.0 ** -20)
    i = fl.add("beside_goal_one_joint_at_rest", "regular", qd=z)
    fl.goal[i] = fl.q[i]
    fl.goal[i, 5] = fl.q[i, 5] + F32(2.0 ** -20)
    return fl


def _tip(q):
    """World position of the gantry's tip at jr = 0: exact in fp32 for dyadic q."""
    q = np.asarray(q, F32)
    return np.array([q[0] + F32(0.5), q[1], F32(0.75) + q[2]], F32)


def gantry_target(kind_name, seed=107):
    """TargetAttractor / TargetPolicy on the gantry's tip (an FK position)."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    rng = np.random.default_rng(seed)
    q, qd = ordinary("gantry", rng, R, qd_max=0.25)
    t = table("gantry")
    goal = rng.uniform([0.0, -0.5, 0.5], [1.0, 0.5, 1.25], (R, 3)).astype(F32)
    kind, P = {"target_attractor": (D.LEAF_TARGET_ATTRACTOR, Cf.TARGET_ATTRACTOR_PARAMS),
               "target_policy": (D.LEAF_TARGET_POLICY, Cf.TARGET_POLICY_PARAMS)}[kind_name]
    fl = Fleet(kind_name + "_gantry", "gantry", [kind],
               [_spec(kind, D.TASKMAP_FK_POSITION, t.frame_index("tip"), P, goal_len=3, name="target")], q, qd, goal)
    z = np.zeros(4, F32)
    for k, qq in enumerate(((-0.25, 0.125, 0.0, 0.0), (-0.5, -0.125, 0.125, 0.0))):
        fl.add(f"at_goal_{k}", "regular", q=qq, goal=_tip(qq))
    qq = (-0.375, 0.0, -0.125, 0.0)
    fl.add("at_goal_at_rest", "regular", q=qq, qd=z, goal=_tip(qq))
    fl.add("beside_goal_x", "regular", q=qq, goal=_tip(qq) + np.array([2.0 ** -20, 0, 0], F32))
    fl.add("beside_goal_xyz", "regular", q=qq, goal=_tip(qq) + F32(2.0 ** -20))
    fl.add("beside_goal_at_rest", "regular", q=qq, qd=z, goal=_tip(qq) - np.array([0, 2.0 ** -20, 0], F32))
    fl.add("at_rest", "regular", qd=z)
    return fl


Z_GATE = F32(17.328680)     # 25 ln 2: an fp32 sigmoid is 1 beyond (rmp2_device.h leaf_obstacle_avoidance)
OBSTACLE_TABLES = {          # name -> (records K, index of the live record, ragged lists?)
    "K1": (1, 0, False), "K33_first": (33, 0, False), "K33_last": (33, 32, False), "K64_first": (64, 0, False), "K64_last": (64, 63, False),
    "ragged_K33_first": (33, 0, True), "ragged_K64_last": (64, 63, True),
    "pairs": (1, 0, None),       # the K1 rows as explicit closest-point pairs; on the surface and on the centre p_link == p_obs
    # capsule tables: the capsule (1, -0.25, 0.75) - (1, 0.25, 0.75), r = 0.125, crosses the sphere's place -- a control point at
    # y = 0 has the sphere's centre for its nearest axis point: `on_centre` is ON THE AXIS, `on_surface` on the capsule's surface
    "capsule_K1": (1, 0, False), "capsule_K33_last": (33, 32, False), "capsule_ragged_K64_first": (64, 0, True),
}


def obstacle(table_name="K1", seed=108):
    """ObstacleAvoidance on the gantry's `jr` frame and tip against the sphere (1, 0, 0.75), r = 0.125, among culled fillers.  The
    curvature term of the distance map divides by the surface distance (taskmap.py:159): a control point ON the surface or the centre
    is a pole of the reference -- f and qdd NaN on every joint -- whatever the velocity; the gate is an exact 0 at and beyond the
    modulation radius 0.5 and for a point that recedes with z = xd / gate_len > 25 ln 2."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    K, at, ragged = OBSTACLE_TABLES[table_name]
    rng = np.random.default_rng(seed)
    q, qd = ordinary("gantry", rng, R, qd_max=0.25)
    t = table("gantry")
    specs = [_spec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr), Cf.OBSTACLE_AVOIDANCE_PARAMS, name="avoid_" + fr)
             for fr in ("jr", "tip")]
    tab = S.table_with(S.LIVE_CAPSULES["cross"] if table_name.startswith("capsule") else S.LIVE_SPHERE, K, at)
    obs = dict(spheres=tab)
    if ragged:    # every robot lists the whole table, each in an order of its own
        obs.update(csr_offset=np.arange(R + 1, dtype=np.int32) * K,
                   csr_index=np.concatenate([np.roll(np.arange(K, dtype=np.int32), r) for r in range(R)]))
    fl = Fleet("obstacle_" + table_name, "gantry", [D.LEAF_OBSTACLE_AVOIDANCE], specs, q, qd, obs=obs)
    fl.table_name = table_name
    z = np.zeros(4, F32)
    v = np.asarray(S.GANTRY_QD, F32)
    gl = F32(Cf.OBSTACLE_AVOIDANCE_PARAMS[4])
    xd_gate = F32(gl * Z_GATE)
    fl.add("tip_on_centre", "pole", q=(0.5, 0, 0, 0), qd=v)
    fl.add("tip_on_surface", "pole", q=(0.375, 0, 0, 0), qd=v)
    fl.add("tip_on_surface_tangential", "pole", q=(0.375, 0, 0, 0), qd=(0, 0.25, 0, 0))       # xd == 0, |v|^2 - xd^2 > 0: x / 0
    fl.add("tip_on_surface_normal", "pole", q=(0.375, 0, 0, 0), qd=(0.25, 0, 0, 0))           # |v|^2 - xd^2 == 0: 0 / 0
    fl.add("tip_on_surface_at_rest", "pole", q=(0.375, 0, 0, 0), qd=z)
    fl.add("jr_on_surface", "pole", q=(0.875, 0, 0, 0), qd=v)
    # (|f| = 1.4e6, the fp32-leaf build's qdd 4.8e-5 off the fp64 one's 1.4e3: steep, and within clause A)
    fl.add("tip_penetrating", "regular", q=(0.4375, 0, 0, 0), qd=v)
    fl.add("tip_at_radius", "regular", q=(-0.125, 0, 0, 0), qd=v, groups=["zero_leaf"])
    fl.add("tip_beyond_radius", "regular", q=(F32(-0.125) - F32(2.0 ** -10), 0, 0, 0), qd=v, groups=["zero_leaf"])
    fl.add("jr_at_radius", "regular", q=(1.625, 0, 0, 0), qd=v, groups=["zero_leaf"])
    fl.add("tip_in_range_at_rest", "regular", q=(0.125, 0, 0, 0), qd=z)
    fl.add("tip_in_range_tangential", "regular", q=(0.125, 0, 0, 0), qd=(0, 0.25, 0.125, 0))  # xd == 0 exactly, away from the surface
    fl.add("tip_receding_z_below", "regular", q=(0.125, 0, 0, 0), qd=(-steps(xd_gate, -64), 0, 0, 0))
    fl.add("tip_receding_z_above", "regular", q=(0.125, 0, 0, 0), qd=(-steps(xd_gate, 64), 0, 0, 0), groups=["zero_leaf"])
    fl.add("tip_approaching", "regular", q=(0.125, 0, 0, 0), qd=(0.25, 0, 0, 0))
    if ragged is None:
        fl.obs = explicit_pairs(fl.q, tab)
        fl.obs_plain = explicit_pairs(fl.q0, tab)
    return fl


def explicit_pairs(q, tab, keep_nan=False):
    """The sphere table as explicit closest-point pairs of the gantry's two control points (jr = 0: exact in fp32), one pair per leaf
    and record: p_link the frame origin, p_obs the sphere's surface point towards it -- the centre itself where the origin sits on it
    (a COINCIDENT pair, as on the surface)."""
    from riemannian_motion_policies_amd import configs as Cf
    q = np.asarray(q, F32)
    jr = np.stack([q[:, 0], q[:, 1], F32(0.75) + q[:, 2]], axis=1).astype(F32)
    org = np.stack([jr, jr + np.array([0.5, 0, 0], F32)], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        pl, po = Cf.pairs_from_spheres(org, tab)
    if not keep_nan:
        po = np.where(np.isfinite(po), po, pl)
    return dict(p_link=pl, p_obs=po)


def collision_avoidance(seed=109):
    """CollisionAvoidance on attached points of the two-joint arm (the exp-05 leaves: one per frame, one pair each, the `dist`
    interface: relative position, unit normal and distance are data).  The weight is a cubic spline with a double root at dist == r
    and an exact 0 beyond; the damping term needs n . xd < 0."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    rng = np.random.default_rng(seed)
    q, qd = ordinary("two_joint", rng, R, qd_max=0.3)
    t = table("two_joint")
    specs = [_spec(D.LEAF_COLLISION_AVOIDANCE, D.TASKMAP_FK_POINT, t.frame_index(fr), Cf.COLLISION_AVOIDANCE_PARAMS, name="collision_avoidance_for_" + fr)
             for fr in t.frame_names]
    rel, nv, dist = Cf.sample_point_pairs(rng, R, len(specs), 1)
    # ordinary rows keep clear of the spline's double root at r = 1.1 (the edge rows sit on it): well inside, or beyond
    dist[:] = np.where(rng.random(dist.shape) < 0.75, rng.uniform(0.05, 0.8, dist.shape), rng.uniform(1.2, 1.3, dist.shape)).astype(F32)
    fl = Fleet("collision_avoidance", "two_joint", [D.LEAF_COLLISION_AVOIDANCE], specs, q, qd)
    fl.obs_plain = dict(p_link=rel.copy(), p_obs=nv.copy(), dist=dist.copy())
    fl.obs = dict(p_link=rel, p_obs=nv, dist=dist)
    r = F32(Cf.COLLISION_AVOIDANCE_PARAMS[4])
    up = np.tile(np.array([0, 0, 1], F32), (len(specs), 1))        # the arm is planar: n . xd == 0 exactly
    for name, d, groups in (("dist_at_r", r, ()), ("dist_below_r", r - F32(2.0 ** -10), ()), ("dist_beyond_r", r + F32(2.0 ** -10), ("zero_leaf",)),
                            ("dist_one_step_beyond_r", steps(r, 1), ("zero_leaf",)), ("dist_zero", F32(0.0), ())):
        i = fl.add(name, "regular", groups=groups)
        dist[i] = d
    i = fl.add("normal_across_the_motion", "regular")
    nv[i] = up
    i = fl.add("normal_across_the_motion_dist_zero", "regular")
    nv[i], dist[i] = up, F32(0.0)
    i = fl.add("at_rest", "regular", qd=np.zeros(2, F32))
    i = fl.add("at_rest_dist_at_r", "regular", qd=np.zeros(2, F32))
    dist[i] = r
    return fl


_FLEETS = {}
BUILDERS = {
    "velocity_cap": lambda: velocity_cap("panda"),
    "velocity_cap_gantry": lambda: velocity_cap("gantry", seed=111),
    "velocity_cap_two_joint": lambda: velocity_cap("two_joint", seed=112),
    "joint_damping": joint_damping,
    "cspace_biasing": cspace_biasing,
    "config_space_biasing": config_space_biasing,
    "joint_limits": joint_limits,
    "joint_limits_band_free": lambda: joint_limits(band_free=True, seed=115),
    "joint_limits_coincide": lambda: joint_limits(coincide=4, seed=116),
    "collision_avoidance": collision_avoidance,
    "target_policy_identity": target_policy_identity,
    "target_attractor_gantry": lambda: gantry_target("target_attractor", seed=117),
    "target_policy_gantry": lambda: gantry_target("target_policy", seed=118),
}
BUILDERS.update({"obstacle_" + name: (lambda name=name: obstacle(name)) for name in OBSTACLE_TABLES})
# the four kinds the quad mapping's structured identity loop takes (rmp2.h rmp2_identity_records), Panda fleets
STRUCTURED = ("velocity_cap", "joint_damping", "cspace_biasing", "config_space_biasing")


def fleet(key):
    """The fleet of `key`, built once and left unchanged."""
    if key not in _FLEETS:
        _FLEETS[key] = BUILDERS[key]()
    return _FLEETS[key]


# ---- yardsticks: functions of the oracle only --------------------------------------------------------------------------------
def _finite(r):
    return np.isfinite(r["M"]).all(axis=(1, 2)) & np.isfinite(r["f"]).all(axis=1) & np.isfinite(r["qdd64"]).all(axis=1)


_REFS = {}


def references(key, shape, solve="auto", plain=False):
    """(fp32-leaf oracle result, fp64 oracle result) of a fleet, computed once and left unchanged."""
    import oracle as O
    k = (key, shape, solve, plain)
    if k not in _REFS:
        fl = fleet(key)
        q, qd, goal = fl.inputs(plain)
        d = fl.desc(shape, solve)
        obs = fl.obstacles(plain)
        _REFS[k] = (O.step(d, q, qd, goal, precision="f32", **obs), O.step(d, q, qd, goal, precision="f64", **obs))
    return _REFS[k]


def classify(key, shape):
    """Every row's class on the oracle: 'pole' (both builds non-finite), 'regular' (the fp32-leaf build passes A or B against the
    fp64 build), 'stiff' (finite in both, outside A and B); 'split' where the builds disagree on finiteness (no row may)."""
    import oracle as O
    r32, r64 = references(key, shape)
    f32, f64 = _finite(r32), _finite(r64)
    g = O.accuracy_gate(r32["qdd64"], r64)
    ab = g["each"]["a"] | g["each"]["b"]
    return np.where(~f32 & ~f64, "pole", np.where(f32 != f64, "split", np.where(ab, "regular", "stiff")))


def system_envelope(desc, q, qd, goal=None, samples: int = 16, seed: int = 0, **obstacle_kwargs):
    """The (M, f) analogue of oracle.fp32_envelope: per entry, the largest |system of the fp32-leaf build - system of the fp64 build|
    over the plain fp32 evaluation and `samples` more on inputs moved by one unit-scale fp32 rounding of random sign (the same
    jiggle, the same seed and draw order); the fp64 system stays on the unperturbed inputs.  Returns (envM [R, n, n], envf [R, n])."""
    import oracle as O
    rng = np.random.default_rng(seed)
    eps = np.float64(2.0 ** -23)

    def jiggle(a):
        a = np.ascontiguousarray(a, dtype=np.float32).astype(np.float64)
        return (a + rng.choice(np.array([-1.0, 1.0]), a.shape) * eps * np.maximum(np.abs(a), 1.0)).astype(np.float32)

    base = O.step(desc, q, qd, goal, precision="f64", **obstacle_kwargs)
    with np.errstate(invalid="ignore"):
        r = O.step(desc, q, qd, goal, precision="f32", **obstacle_kwargs)
        envM, envf = np.abs(r["M"] - base["M"]), np.abs(r["f"] - base["f"])
        for _ in range(samples):
            kw = {k: (jiggle(v) if k in ("spheres", "p_link", "p_obs", "dist") and v is not None else v) for k, v in obstacle_kwargs.items()}
            r = O.step(desc, jiggle(q), jiggle(qd), None if goal is None else jiggle(goal), precision="f32", **kw)
            envM, envf = np.fmax(envM, np.abs(r["M"] - base["M"])), np.fmax(envf, np.abs(r["f"] - base["f"]))
    return envM, envf


def system_bounds(ref64, envM, envf, rel=1e-5, factor=2.0):
    """Entrywise bounds of an exported system against the fp64 one: max(factor * envelope, rel * the entry's own row / column scale)
    -- factor: accuracy_gate's envelope_factor; rel: the north-star tolerance, for M at min(max_k |M|_ik, max_k |M|_kj), for f at
    max_k |f|_k.  A row or column that is exactly zero in fp64 gets the bound of its envelope alone."""
    M, f = np.abs(ref64["M"]), np.abs(ref64["f"])
    with np.errstate(invalid="ignore"):
        scale = np.minimum(M.max(axis=2)[:, :, None], M.max(axis=1)[:, None, :])
        return np.fmax(factor * envM, rel * scale), np.fmax(factor * envf, rel * f.max(axis=1)[:, None])


_ENVS = {}


def envelopes(key, shape, solve="auto"):
    """dict(qdd: oracle.fp32_envelope [R], M, f: system_envelope) of a fleet, computed once."""
    import oracle as O
    k = (key, shape, solve)
    if k not in _ENVS:
        fl = fleet(key)
        d = fl.desc(shape, solve)
        envM, envf = system_envelope(d, fl.q, fl.qd, fl.goal, **fl.obs)
        _ENVS[k] = dict(qdd=O.fp32_envelope(d, fl.q, fl.qd, fl.goal, **fl.obs), M=envM, f=envf)
    return _ENVS[k]

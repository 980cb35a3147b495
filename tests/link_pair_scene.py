"""Exact scenes for the link-capsule closest points at DEGENERATE geometry, and their fp64 reference.

Link geometry puts the control point of a distance leaf on the nearest point of the link's capsule to the obstacle (rmp2.h
rmp2_obstacles.link_capsules).  The closed form has special cases -- a sphere centred on the link's axis, crossing, parallel and
collinear axes, zero-length capsules, endpoint clamps, overlapping shapes -- that random obstacles hit with probability zero.
They are only well posed if the world geometry is EXACT in fp32 (else |X - Y| is 1e-15 instead of 0 and the normal is noise), so
the robots here have exact kinematics:

  gantry      jx, jy, jz prismatic along x, y, z; jr revolute about z, held at q = 0 with a velocity; a fixed tip 0.5 along x;
              zero rpy and dyadic origins.  Leaves: a target attractor on the tip, joint damping (M positive definite), obstacle
              avoidance on the jr frame (link capsule (0,0,0)-(0.5,0,0), r 0.0625) and on the tip (zero-length, r 0.0625).
              The link axis runs from (qx, qy, 0.75 + qz) to +0.5 in x.
  two-joint   the package's planar arm at q = (0, q2): link 1 lies exactly on x at z = float32(0.075).  config5_two_joint's
              leaves plus joint damping (the set alone is singular there).  The fixed normal +z pulls back to zero on a planar
              arm: this scene checks finiteness, status and route agreement, the gantry the convention's value.

Reference: configs.pairs_from_link_capsules in fp64 on the oracle's fp64 frames, then oracle.step on those explicit pairs.
Helpers for tests/test_link_pairs_host.py and tests/test_gpu_link_pair_degenerate.py only.
"""
import atexit
import os
import tempfile

import numpy as np

LINK_R = 0.0625
OBS_R = 0.125
FAR_Z = 40.0                      # fillers and "the table moved away": culled, an exact 0 from the leaf's own cutoff
MATTERS = 1e-3                    # a live row moves the oracle's fp64 qdd by more than this

GANTRY_URDF = """<?xml version="1.0"?>
<robot name="gantry">
  <link name="base"/><link name="lx"/><link name="ly"/><link name="lz"/><link name="lr"/><link name="ltip"/>
  <joint name="jx" type="prismatic"><parent link="base"/><child link="lx"/><origin xyz="0 0 0.5" rpy="0 0 0"/><axis xyz="1 0 0"/></joint>
  <joint name="jy" type="prismatic"><parent link="lx"/><child link="ly"/><origin xyz="0 0 0.25" rpy="0 0 0"/><axis xyz="0 1 0"/></joint>
  <joint name="jz" type="prismatic"><parent link="ly"/><child link="lz"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/></joint>
  <joint name="jr" type="revolute"><parent link="lz"/><child link="lr"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/></joint>
  <joint name="tip" type="fixed"><parent link="lr"/><child link="ltip"/><origin xyz="0.5 0 0" rpy="0 0 0"/></joint>
</robot>
"""
GANTRY_ORDER = ["jx", "jy", "jz", "jr"]

# name, (qx, qy, qz): the cases against the sphere (1, 0, 0.75, r 0.125); `reach` and `reach_near` bring the link's far end to
# the zero-length capsule record at (2, 0, 0.75)
GANTRY_ROWS = [
    ("cross_mid", (0.75, 0.0, 0.0)),     # centre on the axis, interior: surface distance r + lr, normal -+z
    ("cross_A", (1.0, 0.0, 0.0)),        # centre on endpoint A
    ("cross_B", (0.5, 0.0, 0.0)),        # centre on endpoint B; the point link of the tip sits on the centre too
    ("beyond_B", (0.25, 0.0, 0.0)),      # on the axis LINE, s clamps to 1
    ("beside", (0.75, 0.25, 0.0)),       # plain perpendicular pair
    ("overlap", (0.75, 0.125, 0.0)),     # shapes overlap, the normal flips
    ("above", (0.75, 0.0, 0.25)),        # normal along +-z without crossing (needs the downward velocity)
    ("far", (8.0, 0.0, 0.0)),            # culled
    ("reach", (1.5, 0.0, 0.0)),          # (capsule tables) endpoint B on the zero-length record
    ("reach_near", (1.25, 0.0, 0.0)),    # (capsule tables) endpoint B 0.25 short of it
]
# The obstacle leaf only weighs a pair that is being APPROACHED (velocity against the pair's normal): the crossing rows, whose
# normal is -z by the convention, rise; `above` descends; `overlap`, whose normal has flipped to -y, moves in +y.
GANTRY_QD = (0.125, -0.25, 0.25, 0.5)
GANTRY_QD_OF = {"overlap": (0.125, 0.25, 0.25, 0.5), "above": (0.125, -0.25, -0.25, 0.5)}
GANTRY_GOAL = (1.5, 0.5, 1.0)
# rows meant to be in range of each live record (rows_in_range asserts that each of them matters)
IN_RANGE = {
    "sphere": ["cross_mid", "cross_A", "cross_B", "beyond_B", "beside", "overlap", "above"],
    "cross": ["cross_mid", "cross_A", "cross_B", "beyond_B", "beside", "overlap", "above"],
    "parallel": ["cross_mid", "cross_A", "cross_B", "beyond_B", "beside", "above"],     # (`beside` lies ON it: collinear overlap)
    "point": ["reach", "reach_near"],
    "collinear": ["cross_mid", "cross_A", "reach", "reach_near"],                       # (cross_A touches its end, reach* lie on it)
}

LIVE_SPHERE = np.array([1.0, 0.0, 0.75, OBS_R], np.float32)
LIVE = {}   # name -> record, the sphere and the four capsules (filled below)
LIVE_CAPSULES = {
    "cross": np.array([1.0, -0.25, 0.75, OBS_R, 1.0, 0.25, 0.75, 0.0], np.float32),      # crosses the link
    "parallel": np.array([0.5, 0.25, 0.75, OBS_R, 1.5, 0.25, 0.75, 0.0], np.float32),   # den = 0 exactly
    "point": np.array([2.0, 0.0, 0.75, OBS_R, 2.0, 0.0, 0.75, 0.0], np.float32),        # zero length
    "collinear": np.array([1.5, 0.0, 0.75, OBS_R, 2.5, 0.0, 0.75, 0.0], np.float32),
}

LIVE.update(sphere=LIVE_SPHERE, **LIVE_CAPSULES)

_URDF_PATH = None


def gantry_urdf_path():
    global _URDF_PATH
    if _URDF_PATH is None or not os.path.exists(_URDF_PATH):
        fd, _URDF_PATH = tempfile.mkstemp(prefix="gantry_", suffix=".urdf")
        with os.fdopen(fd, "w") as f:
            f.write(GANTRY_URDF)
        atexit.register(lambda path=_URDF_PATH: os.path.exists(path) and os.unlink(path))
    return _URDF_PATH


def gantry(solve="auto"):
    """dict(desc, lc [2, 8], names, q, qd, goal [rows, .]) of the gantry scene."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    t = U.compile_urdf(gantry_urdf_path(), GANTRY_ORDER)
    specs = [
        D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("tip"), Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3, name="attractor"),
        D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping"),
        D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index("jr"), Cf.OBSTACLE_AVOIDANCE_PARAMS, name="avoid_jr"),
        D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index("tip"), Cf.OBSTACLE_AVOIDANCE_PARAMS, name="avoid_tip"),
    ]
    desc = D.build_desc(t, specs, solve)
    lc = np.array([[0, 0, 0, LINK_R, 0.5, 0, 0, 0], [0, 0, 0, LINK_R, 0, 0, 0, 0]], np.float32)
    n = len(GANTRY_ROWS)
    q = np.zeros((n, 4), np.float32)
    q[:, :3] = [r[1] for r in GANTRY_ROWS]
    qd = np.array([GANTRY_QD_OF.get(r[0], GANTRY_QD) for r in GANTRY_ROWS], np.float32)
    goal = np.tile(np.asarray(GANTRY_GOAL, np.float32), (n, 1))
    return dict(desc=desc, table=t, lc=lc, names=[r[0] for r in GANTRY_ROWS], q=q, qd=qd, goal=goal)


TWO_JOINT_Q2 = (0.5, 1.0, -1.5)
TWO_JOINT_Z = np.float32(0.075)
# spheres at link 1's height: on its axis, on its endpoints, beside it, overlapping it (radius 0.125, link radius 0.0625)
TWO_JOINT_SPHERES = np.array([[0.5, 0.0, TWO_JOINT_Z, OBS_R], [0.0, 0.0, TWO_JOINT_Z, OBS_R], [1.0, 0.0, TWO_JOINT_Z, OBS_R],
                              [0.5, -0.25, TWO_JOINT_Z, OBS_R], [0.25, -0.125, TWO_JOINT_Z, OBS_R],
                              [1.0, 0.0, TWO_JOINT_Z + np.float32(0.05), OBS_R]], np.float32)
# (the last one is centred on the origin of joint_2, endpoint A of link 2 whatever q2 is: a crossing pair on a frame that moves)
TWO_JOINT_SPHERE_NAMES = ["on_axis", "on_A", "on_B", "beside", "overlap", "on_joint_2"]


def two_joint(solve="auto"):
    """dict(desc, lc [3, 8], names, q, qd, goal) of the two-joint scene: one row per q2."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    t = U.two_joint_table()
    specs = [D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_FK_POSITION, t.frame_index("link_23"), Cf.TARGET_POLICY_PARAMS, goal_len=3, name="target"),
             D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping")]
    for fr in Cf.TWO_JOINT_CONTROL_POINT_FRAMES:
        specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr), Cf.OBSTACLE_AVOIDANCE_PARAMS,
                                name=f"collision_avoidance_for_{fr}"))
    desc = D.build_desc(t, specs, solve)
    lc = np.array([[0, 0, 0, LINK_R, 1, 0, 0, 0], [0, 0, 0, LINK_R, 1, 0, 0, 0], [0, 0, 0, LINK_R, 0, 0, 0, 0]], np.float32)
    n = len(TWO_JOINT_Q2)
    q = np.zeros((n, 2), np.float32)
    q[:, 1] = TWO_JOINT_Q2
    qd = np.tile(np.asarray([0.25, -0.5], np.float32), (n, 1))
    goal = np.tile(np.asarray([1.0, 1.0, 0.125], np.float32), (n, 1))
    return dict(desc=desc, table=t, lc=lc, names=[f"q2={v}" for v in TWO_JOINT_Q2], q=q, qd=qd, goal=goal)


def filler(width):
    """A record that every row culls: far above the scene."""
    rec = np.zeros(width, np.float32)
    rec[:4] = [0.0, 0.0, FAR_Z, OBS_R]
    if width == 8:
        rec[4:7] = [0.5, 0.0, FAR_Z]
    return rec


def table_with(live, K, at):
    """[K, 4 | 8]: `live` at index `at` (an index or a list of them) among fillers."""
    live = np.asarray(live, np.float32)
    tab = np.tile(filler(live.shape[0]), (K, 1))
    tab[np.atleast_1d(at)] = live
    return tab


def moved_away(table):
    tab = np.array(table, np.float32)
    tab[:, 2] += np.float32(FAR_Z)
    if tab.shape[1] == 8:
        tab[:, 6] += np.float32(FAR_Z)
    return tab


def tiled(s, R):
    """The scene's rows repeated to a fleet of R robots (row i % rows)."""
    idx = np.arange(R) % len(s["q"])
    return dict(s, q=s["q"][idx].copy(), qd=s["qd"][idx].copy(), goal=s["goal"][idx].copy(), names=[s["names"][i] for i in idx], row=idx)


def distance_frames(desc):
    from riemannian_motion_policies_amd import descriptor as D
    return [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]


def check_exact_kinematics(s, frames=None, origins_only=()):
    """The precondition of every test on these scenes: the oracle's fp32 forward kinematics equals its fp64 one BIT FOR BIT on the
    frames the degenerate pairs live on (all of the gantry's; `frames` whole and `origins_only` by their origin on the two-joint
    arm, whose second link turns by a q2 no fp32 cosine has exactly).  Returns the fp64 frames [R, F, 4, 4]."""
    import oracle as O
    T32 = O.forward_kinematics(s["desc"], s["q"], "f32")
    T64 = O.forward_kinematics(s["desc"], s["q"], "f64")
    F = T64.shape[1]
    whole = list(range(F)) if frames is None else list(frames)
    assert np.array_equal(T32[:, whole].astype(np.float64), T64[:, whole]), "the scene's kinematics are not exact in fp32"
    for f in origins_only:
        # (joint_2 sits at float32(0.075) + float32(0.05): one correctly rounded sum in fp32, the same number once the fp64 sum is rounded)
        assert np.array_equal(T32[:, f, :3, 3], T64[:, f, :3, 3].astype(np.float32)), "the scene's frame origins are not exact in fp32"
    return T64


def pairs64(s, table):
    """fp64 closed-form closest points of every (distance leaf, record): p_link, p_obs [R, C * K, 3] (returned as fp32, what
    oracle.step takes) and the surface gap |X - Y| - r - lr [R, C * K] in fp64."""
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    T = O.forward_kinematics(s["desc"], s["q"], "f64")[:, distance_frames(s["desc"])]
    pl, po = Cf.pairs_from_link_capsules(T, s["lc"], np.asarray(table, np.float32))
    # (the axis distance by the independent form below, for the "meant to be in range" classification)
    lc = s["lc"].astype(np.float64)
    A = T[:, :, :3, 3] + np.einsum("rcij,cj->rci", T[:, :, :3, :3], lc[:, 0:3])
    B = T[:, :, :3, 3] + np.einsum("rcij,cj->rci", T[:, :, :3, :3], lc[:, 4:7])
    tb = np.asarray(table, np.float64)
    Cc, Dd = tb[:, 0:3], (tb[:, 4:7] if tb.shape[1] == 8 else tb[:, 0:3])
    R, Cn, K = A.shape[0], A.shape[1], tb.shape[0]
    shape = (R, Cn, K, 3)
    X, Y = seg_seg_np(np.broadcast_to(A[:, :, None], shape).reshape(-1, 3), np.broadcast_to(B[:, :, None], shape).reshape(-1, 3),
                      np.broadcast_to(Cc[None, None], shape).reshape(-1, 3), np.broadcast_to(Dd[None, None], shape).reshape(-1, 3))
    axis = np.linalg.norm(X - Y, axis=-1).reshape(R, Cn, K)
    gap = axis - tb[None, None, :, 3] - lc[None, :, None, 3]
    return pl, po, gap.reshape(R, Cn * K)


def seg_seg_np(p1, q1, p2, q2):
    """Clamped nearest points of the segments p1-q1 and p2-q2 (rows [N, 3]) in fp64: X on the first, Y on the second."""
    p1, q1, p2, q2 = (np.asarray(v, np.float64) for v in (p1, q1, p2, q2))
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e = (d1 * d1).sum(-1), (d2 * d2).sum(-1)
    f, c, b = (d2 * r).sum(-1), (d1 * r).sum(-1), (d1 * d2).sum(-1)
    with np.errstate(all="ignore"):
        den = a * e - b * b
        s = np.where(den > 0, np.clip((b * f - c * e) / np.where(den > 0, den, 1.0), 0, 1), 0.0)
        t = np.where(e > 0, (b * s + f) / np.where(e > 0, e, 1.0), 0.0)
        s = np.where(t < 0, np.clip(-c / np.where(a > 0, a, 1.0), 0, 1), np.where(t > 1, np.clip((b - c) / np.where(a > 0, a, 1.0), 0, 1), s))
        t = np.clip(t, 0, 1)
        s = np.where(a > 0, s, 0.0)
        s = np.where((e > 0) | (a <= 0), s, np.clip(-c / np.where(a > 0, a, 1.0), 0, 1))
    return p1 + s[:, None] * d1, p2 + t[:, None] * d2


def capsule_pair_np(A, B, rl, Cc, Dd, ro):
    """fp64 fields of capsule pairs (rows): axis points X, Y, surface points p_link = X - rl n, p_obs = Y + ro n with n the unit
    vector of X - Y (+z where the axes intersect: the project's convention), the distance |p_link - p_obs| = ||X - Y| - rl - ro| and
    the normal (p_link - p_obs) / distance."""
    X, Y = seg_seg_np(A, B, Cc, Dd)
    n = X - Y
    nn = np.linalg.norm(n, axis=-1, keepdims=True)
    u = np.where(nn == 0, np.array([0.0, 0.0, 1.0]), n / np.where(nn == 0, 1.0, nn))
    rl, ro = np.asarray(rl, np.float64).reshape(-1, 1), np.asarray(ro, np.float64).reshape(-1, 1)
    gap = nn - rl - ro
    return dict(X=X, Y=Y, p_link=X - rl * u, p_obs=Y + ro * u, dist=np.abs(gap[:, 0]), gap=gap[:, 0],
                normal=np.where(gap < 0, -u, u), axis=nn[:, 0])


def gather_lists(pl, po, n_leaves, K, lists, fill):
    """Per-robot obstacle lists (list of index lists; repeats count twice) as explicit pairs: each list padded with the filler
    record `fill` (an exact 0 in the leaf) to the longest -> p_link, p_obs [R, n_leaves * L, 3]."""
    L = max(1, max(len(l) for l in lists))
    idx = np.array([list(l) + [fill] * (L - len(l)) for l in lists], np.int64)            # [R, L]
    cols = (np.arange(n_leaves)[None, :, None] * K + idx[:, None, :]).reshape(len(lists), -1)
    rows = np.arange(len(lists))[:, None]
    return pl[rows, cols], po[rows, cols]


def reference(s, table, lists=None, fill=None, extra=None):
    """oracle.step on the fp64 closed-form pairs of (scene rows, table).  lists: per-robot index lists into the table instead of
    the whole table.  extra = (p_link, p_obs [R, C, E, 3]): further pairs appended to each leaf's (self pairs)."""
    import oracle as O
    pl, po, _ = pairs64(s, table)
    Cn, K = len(s["lc"]), len(table)
    if lists is not None:
        pl, po = gather_lists(pl, po, Cn, K, lists, fill)
    if extra is not None:
        R = pl.shape[0]
        pl = np.concatenate([pl.reshape(R, Cn, -1, 3), extra[0]], axis=2).reshape(R, -1, 3)
        po = np.concatenate([po.reshape(R, Cn, -1, 3), extra[1]], axis=2).reshape(R, -1, 3)
    return O.step(s["desc"], s["q"], s["qd"], s["goal"], p_link=np.ascontiguousarray(pl, np.float32), p_obs=np.ascontiguousarray(po, np.float32))


def rows_in_range(s, table, expect):
    """Asserts on the oracle alone that every row of `expect` (names: the rows MEANT to be in range of `table`) matters: its fp64
    qdd moves by more than MATTERS when the table is moved away -- else the row would test nothing (re-aim it, do not drop it).
    Returns the mask of the rows that matter."""
    d = np.abs(reference(s, table)["qdd64"] - reference(s, moved_away(table))["qdd64"]).max(axis=1)
    weak = sorted({n for n, di in zip(s["names"], d) if n in expect and not di > MATTERS})
    assert not weak and set(expect) <= set(s["names"]), f"rows meant to be in range that do not matter: {weak}"
    return d > MATTERS

"""Exact hulls and a catalogue of DEGENERATE closest-point cases with closed-form answers, for the two hull routines
(rmp2_hull.h hull_closest: hull against sphere or capsule; hull_pair_closest: hull against hull) and the stages built on them.

Random states on the Panda meshes never put a centre ON a vertex, a segment IN a face plane or two faces exactly parallel; the
routines' special cases (GJK on flat and collinear simplices, the 1e-7 m touch threshold, the face rule, nearest pairs that are
a set) only run on geometry that is exact.  The hulls here have dyadic vertices and planes written down by hand, never left to
qhull's rounding: the unit cube {0, 1}^3, the cube scaled by 1/4, and the tetrahedron (0,0,0), (1,0,0), (0,1,0), (0,0,1), the
smallest legal hull (its slanted plane is float32(1/sqrt 3) (1, 1, 1 | 1): the routine is given, and the face rule's expected
answer is computed from, those stored numbers).

A catalogue row states, in advance and without looking at any routine's answer:
    sep   the signed separation of the AXIS and the hull: the distance apart, or -t_f* under the face rule; gap = sep - r
    u     the unit direction from the axis point towards the hull point, or None where the face rule TIES
    hp xp the two points where the nearest pair is unique, else None
    kind  "unique"  everything above is held
          "set"     the nearest pair is a set (parallel features): gap and u are held, the points by membership
          "tie"     the face rule ties between the faces `faces` (a point on a vertex or an edge, coincident hulls): gap is held,
                    u must be minus one of those faces' normals, the points by membership
                    `ends` (the grazing axis, whose tied faces meet it at DIFFERENT endpoints, both off the hull): the rule's
                    answer is one of a finite list, face f with x* = that face's endpoint and hp = x* + t_f n_f (which is not
                    on the hull: rmp2.h's p_link under the face rule is x* moved to the face's plane); held to the matching one
Membership: hp on the hull (no plane value above the bound), xp on the segment, hp - xp = (gap + r) u.

The GPU scene hangs the cube on the gantry of tests/link_pair_scene.py (prismatic x, y, z joints with dyadic origins: the frames
are exact in fp32), one robot row and one obstacle record per catalogue row.  Helpers for tests/test_link_hulls_host.py,
tests/test_self_hulls_host.py and tests/test_gpu_hull_degenerate.py only.
"""
import numpy as np

import link_pair_scene as LS

S2, S3 = np.sqrt(2.0), np.sqrt(3.0)
R_OBS = 0.125                     # the default radius; rows apart carry the radius that leaves a gap of 0.125 .. 0.25 (in reach of the leaves)

CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
CUBE_P = np.array([[1, 0, 0, 1], [-1, 0, 0, 0], [0, 1, 0, 1], [0, -1, 0, 0], [0, 0, 1, 1], [0, 0, -1, 0]], np.float64)
PX, MX, PY, MY, PZ, MZ = range(6)                      # the cube's faces in CUBE_P's order
SMALL_V, SMALL_P = CUBE_V * 0.25, CUBE_P * np.array([1, 1, 1, 0.25])
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
_T = np.float64(np.float32(1.0 / S3))
TET_P = np.array([[-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [_T, _T, _T, _T]], np.float64)
T_MX, T_MY, T_MZ, T_SLANT = range(4)
HULLS = {"cube": (CUBE_V, CUBE_P), "small": (SMALL_V, SMALL_P), "tet": (TET_V, TET_P)}

GRAZE_EPS = np.float64(np.float32(2e-7 * S2))         # the x shift that takes the grazing segment 2e-7 m off the cube's edge


def _row(name, hull, a, b, sep, u=None, hp=None, xp=None, kind="unique", faces=(), r=R_OBS, ends=None):
    f = lambda v: None if v is None else np.asarray(v, np.float64)   # noqa: E731
    return dict(name=name, hull=hull, a=f(a), b=f(a if b is None else b), r=float(r), sep=float(sep), u=f(u), hp=f(hp), xp=f(xp),
                kind=kind, faces=tuple(faces), ends=ends)


def link_catalogue():
    """The rows for hull_closest: hull against a point (b None) or a segment."""
    n1 = -np.array([1.0, 0, 1]) / S2
    rows = [
        # ---- a point
        _row("pt_on_vertex", "cube", (1, 1, 1), None, 0.0, kind="tie", faces=(PX, PY, PZ)),
        _row("pt_on_edge", "cube", (1, 0.5, 1), None, 0.0, kind="tie", faces=(PX, PZ)),
        _row("pt_on_face", "cube", (0.5, 0.5, 1), None, 0.0, (0, 0, -1), (0.5, 0.5, 1), (0.5, 0.5, 1)),
        _row("pt_at_centre", "cube", (0.5, 0.5, 0.5), None, -0.5, kind="tie", faces=(PX, MX, PY, MY, PZ, MZ)),
        _row("pt_inside", "cube", (0.875, 0.5, 0.5), None, -0.125, (-1, 0, 0), (1, 0.5, 0.5), (0.875, 0.5, 0.5)),
        _row("pt_above_face_foot_on_edge", "cube", (1, 0.5, 1.5), None, 0.5, (0, 0, -1), (1, 0.5, 1), (1, 0.5, 1.5), r=0.375),
        _row("pt_above_face_foot_on_corner", "cube", (1, 1, 1.5), None, 0.5, (0, 0, -1), (1, 1, 1), (1, 1, 1.5), r=0.375),
        _row("pt_off_edge", "cube", (1.5, 0.5, 1.5), None, S2 / 2, n1, (1, 0.5, 1), (1.5, 0.5, 1.5), r=0.5),
        _row("pt_off_corner", "cube", (1.5, 1.5, 1.5), None, S3 / 2, -np.ones(3) / S3, (1, 1, 1), (1.5, 1.5, 1.5), r=0.75),
        _row("sphere_r0_on_face", "cube", (0.5, 0.5, 1), None, 0.0, (0, 0, -1), (0.5, 0.5, 1), (0.5, 0.5, 1), r=0.0),
        _row("zero_length_capsule", "cube", (0.5, 0.25, 1.5), None, 0.5, (0, 0, -1), (0.5, 0.25, 1), (0.5, 0.25, 1.5), r=0.375),
        # ---- a segment apart from the hull
        _row("seg_par_face_inside", "cube", (0.25, 0.5, 1.5), (0.75, 0.5, 1.5), 0.5, (0, 0, -1), kind="set", r=0.375),
        _row("seg_par_face_overhang", "cube", (0.5, 0.5, 1.5), (2, 0.5, 1.5), 0.5, (0, 0, -1), kind="set", r=0.375),
        _row("seg_par_edge", "cube", (1.5, 0.25, 1.5), (1.5, 0.75, 1.5), S2 / 2, n1, kind="set", r=0.5),
        _row("seg_collinear_edge_beyond", "cube", (1, 1.5, 1), (1, 2.5, 1), 0.5, (0, -1, 0), (1, 1, 1), (1, 1.5, 1), r=0.375),
        _row("seg_perp_face", "cube", (0.5, 0.5, 1.25), (0.5, 0.5, 2), 0.25, (0, 0, -1), (0.5, 0.5, 1), (0.5, 0.5, 1.25)),
        _row("seg_perp_face_b_first", "cube", (0.5, 0.5, 2), (0.5, 0.5, 1.25), 0.25, (0, 0, -1), (0.5, 0.5, 1), (0.5, 0.5, 1.25)),
        _row("seg_far", "cube", (5, 0.5, 0.5), (5.5, 0.5, 3), 4.0, (-1, 0, 0), (1, 0.5, 0.5), (5, 0.5, 0.5)),
        # ---- a segment in contact with the hull
        _row("seg_on_edge", "cube", (1, 0.25, 1), (1, 0.75, 1), 0.0, kind="tie", faces=(PX, PZ)),
        _row("seg_in_face_plane", "cube", (0.25, 0.5, 1), (0.75, 0.5, 1), 0.0, (0, 0, -1), kind="set"),
        _row("seg_touch_face_at_end", "cube", (0.5, 0.5, 1), (0.5, 0.5, 2), 0.0, (0, 0, -1), (0.5, 0.5, 1), (0.5, 0.5, 1)),
        _row("seg_touch_face_at_b", "cube", (0.5, 0.5, 2), (0.5, 0.5, 1), 0.0, (0, 0, -1), (0.5, 0.5, 1), (0.5, 0.5, 1)),
        _row("seg_touch_edge_at_end", "cube", (1, 0.5, 1), (2, 0.5, 2), 0.0, kind="tie", faces=(PX, PZ)),
        _row("seg_touch_vertex_at_end", "cube", (1, 1, 1), (2, 2, 2), 0.0, kind="tie", faces=(PX, PY, PZ)),
        # (piercing along z at x = 0.75: the +x face needs 0.25 and BOTH endpoints attain its minimum; rmp2.h names no winner, so
        # either endpoint moved to the face's plane is the rule's answer -- neither is on the hull)
        _row("seg_pierce", "cube", (0.75, 0.5, -1), (0.75, 0.5, 2), -0.25, kind="tie", faces=(PX, PX), ends=("a", "b")),
        _row("seg_inside", "cube", (0.25, 0.75, 0.5), (0.5, 0.875, 0.5), -0.25, (0, -1, 0), (0.25, 1, 0.5), (0.25, 0.75, 0.5)),
        # the grazing pair: the axis touches the edge x = z = 1 at (1, 0.5, 1) -> the face rule, whose faces +x (at a)
        # and +z (at b) both need 0.5; the same axis GRAZE_EPS further along x is 2e-7 m clear of the edge -> GJK's pair
        _row("seg_graze", "cube", (0.5, 0.5, 1.5), (1.5, 0.5, 0.5), -0.5, kind="tie", faces=(PX, PZ), ends=("a", "b")),
        _row("seg_graze_near", "cube", (0.5 + GRAZE_EPS, 0.5, 1.5), (1.5 + GRAZE_EPS, 0.5, 0.5), GRAZE_EPS / S2, n1, (1, 0.5, 1),
             (1 + GRAZE_EPS / 2, 0.5, 1 + GRAZE_EPS / 2)),
        # ---- the tetrahedron
        _row("tet_pt_off_slant", "tet", (1, 1, 1), None, 2 / S3, -np.ones(3) / S3, np.ones(3) / 3, (1, 1, 1)),
        _row("tet_pt_off_edge", "tet", (1, 1, 0), None, S2 / 2, -np.array([1.0, 1, 0]) / S2, (0.5, 0.5, 0), (1, 1, 0)),
        _row("tet_pt_inside", "tet", (0.25, 0.25, 0.125), None, -0.125, (0, 0, 1), (0.25, 0.25, 0), (0.25, 0.25, 0.125)),
        _row("tet_pt_on_apex", "tet", (0, 0, 1), None, 0.0, kind="tie", faces=(T_MX, T_MY, T_SLANT)),
        _row("tet_seg_par_slant", "tet", (1.125, 0.875, 1), (0.875, 1.125, 1), 2 / S3, -np.ones(3) / S3, kind="set"),
    ]
    assert len({r["name"] for r in rows}) == len(rows)
    return rows


def nonfinite_link_rows():
    """(name, a, b, r): the finite segment of `seg_perp_face` with one value replaced."""
    a, b = (0.5, 0.5, 1.5), (1.5, 0.5, 1.5)
    out = []
    for bad, tag in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "minf")):
        out.append((f"{tag}_in_a", (bad, 0.5, 1.5), b, R_OBS))
        out.append((f"{tag}_in_b", a, (bad, 0.5, 1.5), R_OBS))
        out.append((f"{tag}_in_r", a, b, bad))
        out.append((f"{tag}_point", (0.5, bad, 1.5), (0.5, bad, 1.5), R_OBS))
    return out


def member_errors(P, a, b, r, hp, xp, u, gap):
    """The membership rules as errors: hp on the hull {n . x <= d} (the largest plane value above 0), xp on the segment a-b, and
    hp - xp = (gap + r) u.  With the gap held to the unique one they make (hp, xp) A nearest pair, whichever of a set."""
    ab = b - a
    s = float(np.clip((xp - a) @ ab / max(float(ab @ ab), 1e-300), 0.0, 1.0))
    return [max(0.0, float((P[:, :3] @ hp - P[:, 3]).max())), float(np.abs(a + s * ab - xp).max()),
            float(np.abs(hp - xp - (gap + r) * u).max())]


def candidates(row):
    """The answers the catalogue allows for a row, as (u, hp, xp) with hp = xp = None where the points are held by membership:
    one for a unique row and for a set; one per tied face for a tie -- with `ends`, fully determined ones: face f, x* = the
    endpoint named beside it, hp = x* + t_f n_f (rmp2.h names no winner where two endpoints or two faces attain the minimum)."""
    P = HULLS[row["hull"]][1]
    if row["kind"] == "unique":
        return [(row["u"], row["hp"], row["xp"])]
    if row["kind"] == "set":
        return [(row["u"], None, None)]
    if row["ends"] is None:
        return [(-P[f, :3], None, None) for f in row["faces"]]
    return [(-P[f, :3], row[e] - row["sep"] * P[f, :3], row[e]) for f, e in zip(row["faces"], row["ends"])]


def _candidate_errors(cand, P, a, b, r, hp, xp, u, gap):
    uc, hpc, xpc = cand
    errs = [float(np.abs(u - uc).max())]
    if hpc is not None:
        return errs + [float(np.abs(hp - hpc).max()), float(np.abs(xp - xpc).max())]
    return errs + member_errors(P, a, b, r, hp, xp, uc, gap)


def check_link_row(row, hp, xp, u, gap, tol):
    """Holds one answer of hull_closest (hull coordinates) to its catalogue row at `tol`: the gap, and the best of the row's
    candidates (its direction, and its points or the membership rules); returns the worst error / tol of what was held."""
    P = HULLS[row["hull"]][1]
    hp, xp, u = (np.asarray(v, np.float64) for v in (hp, xp, u))
    assert np.isfinite([*hp, *xp, *u, gap]).all(), (row["name"], hp, xp, u, gap)
    errs = min((_candidate_errors(c, P, row["a"], row["b"], row["r"], hp, xp, u, gap) for c in candidates(row)), key=max)
    errs = [abs(gap - (row["sep"] - row["r"]))] + errs
    worst = max(errs) / tol
    assert worst <= 1.0, (row["name"], row["kind"], errs, tol)
    return worst


def check_stage_answer(cands, P, a, b, r, gap, origin, point, pl, po, dd, tol, what=""):
    """Holds one pair of the hull STAGE (p_link, p_obs, dist in the leaf's output convention) to the best of `cands` at `tol`,
    with the candidate's own direction u -- nothing is recovered from the answer: dist = |gap|; FK_DISTANCE: p_link - p_obs =
    gap u, hp = p_link - origin, xp = p_obs - r u - origin; FK_POINT: p_obs = sign(gap) u, hp = p_link, xp = hp - (gap + r) u;
    then hp and xp against the candidate's points, or hp on the hull and xp on the segment a-b (hull coordinates).  Returns the
    worst error / tol."""
    pl, po = np.asarray(pl, np.float64), np.asarray(po, np.float64)
    best = None
    for uc, hpc, xpc in cands:
        if point:
            eu = np.abs(po - (1.0 if gap >= 0 else -1.0) * uc).max()
            hp = pl
            xp = hp - (gap + r) * uc
        else:
            eu = np.abs(pl - po - gap * uc).max()
            hp, xp = pl - origin, po - r * uc - origin
        if hpc is not None:
            errs = [eu, np.abs(hp - hpc).max(), np.abs(xp - xpc).max()]
        else:
            errs = [eu] + member_errors(P, a, b, r, hp, xp, uc, gap)[:2]
        if best is None or max(errs) < max(best):
            best = errs
    best = [abs(dd - abs(gap))] + [float(e) for e in best]
    worst = max(best) / tol
    assert worst <= 1.0, (what, best, tol)
    return worst


def nearest_pair_is_a_set(V, P, a, b, step=1e-2):
    """Decided from the geometry alone (the restatement's distances, no routine's answer): a segment a-b APART from the hull has
    a set of nearest pairs exactly when its distance to the hull stays at the minimum over a piece of the segment (the distance
    is convex along it) -- here: a point `step` along the segment from the nearest one is no further than 1e-9.  A segment that is
    not parallel to its nearest feature gains at least step^2 / (2 distance) > 5e-7 there at the distances of these scenes."""
    import hull_reference as H
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    L = float(np.linalg.norm(b - a))
    if L == 0.0:
        return False
    _, xp, _, g = H.hull_closest(V, P, a[None], b[None], [0.0])
    if g[0] <= 1e-7:
        return False
    d = (b - a) / L
    s = float((xp[0] - a) @ d)
    for ds in (-step, step):
        s2 = min(max(s + ds, 0.0), L)
        if abs(s2 - s) < 1e-6:
            continue
        x = (a + s2 * d)[None]
        if H.hull_closest(V, P, x, x, [0.0])[3][0] - g[0] <= 1e-9:
            return True
    return False


# ---- the GPU scene: the cube on the gantry ------------------------------------------------------------------------------------------
# tests/link_pair_scene.py's gantry: the jr frame sits at (qx, qy, 0.75 + qz) with the identity rotation, the tip 0.5 further in x.
# Pair leaf 0 (jr) carries the unit cube, pair leaf 1 (tip) the quarter cube FAR_HULL away in the tip's coordinates, so that every
# record of every table lies beyond it in all three coordinates: its nearest pairs are vertex against segment, unique.  One leaf
# is an FK_DISTANCE leaf and the other an FK_POINT leaf (`swap` exchanges them): both output conventions in one launch.
# A table holds one record per catalogue row of a CHUNK, record k displaced by SPACING k (1, 1, 1), and robot k puts its jr frame
# on that displacement: record k is in row k's catalogue position, every other record lies beyond the cube in all three
# coordinates (the catalogue's axes stay within [-1, 5.5]), where the nearest pair is a vertex against a segment again.  Dyadic
# throughout, coordinates below 64: frames, records and the dyadic answers are exact in fp32, a surd answer rounds by <= 1.9e-6.
SPACING = 8.0
CHUNK = 5
FAR_HULL = -40.0
GRAZE_SHIFT = np.array([GRAZE_EPS, 0.0, 0.0])


def gpu_rows(points):
    """The cube's catalogue rows a sphere table (`points`) or a capsule table can state, seg_graze_near first (see scene())."""
    rows = [r for r in link_catalogue() if r["hull"] == "cube" and (np.array_equal(r["a"], r["b"]) or not points)]
    return sorted(rows, key=lambda r: r["name"] != "seg_graze_near")


def chunks(rows, n=CHUNK):
    return [rows[i:i + n] for i in range(0, len(rows), n)]


def gantry_hulls():
    """urdf.LinkHulls of the two pair leaves, planes written down exactly."""
    from riemannian_motion_policies_amd import urdf as U
    far_v = SMALL_V + FAR_HULL
    far_p = np.array([[1, 0, 0, FAR_HULL + 0.25], [-1, 0, 0, -FAR_HULL], [0, 1, 0, FAR_HULL + 0.25], [0, -1, 0, -FAR_HULL],
                      [0, 0, 1, FAR_HULL + 0.25], [0, 0, -1, -FAR_HULL]], np.float64)
    return U.LinkHulls(np.array([0, 8, 16], np.int32), np.ascontiguousarray(np.concatenate([CUBE_V, far_v]), np.float32),
                       np.array([0, 6, 12], np.int32), np.ascontiguousarray(np.concatenate([CUBE_P, far_p]), np.float32))


def gantry_desc(swap=False, solve="auto"):
    """The gantry with an attractor, joint damping and the two pair leaves; leaf 0 (jr) FK_DISTANCE and leaf 1 (tip) FK_POINT, or
    the other way round with `swap`."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    t = U.compile_urdf(LS.gantry_urdf_path(), LS.GANTRY_ORDER)
    dist = lambda fr: D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr), Cf.OBSTACLE_AVOIDANCE_PARAMS, name=f"avoid_{fr}")   # noqa: E731
    point = lambda fr: D.LeafSpec(D.LEAF_COLLISION_AVOIDANCE, D.TASKMAP_FK_POINT, t.frame_index(fr), Cf.COLLISION_AVOIDANCE_PARAMS, name=f"avoid_{fr}")  # noqa: E731
    specs = [
        D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("tip"), Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3, name="attractor"),
        D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping"),
        point("jr") if swap else dist("jr"),
        dist("tip") if swap else point("tip"),
    ]
    return t, D.build_desc(t, specs, solve)


def scene(rows, capsules, ordinary=0, seed=0):
    """The table of `rows` (one record each, record k at SPACING k (1, 1, 1)) and a fleet: robot k < len(rows) in row k's catalogue
    position, then `ordinary` robots at random dyadic positions (multiples of 2^-10 within the table's extent: exact frames,
    nothing special about the geometry).  seg_graze_near cannot state 0.5 + GRAZE_EPS in an fp32 record: its record is seg_graze's
    and its ROBOT steps back by GRAZE_EPS in x, which fp32 holds exactly next to 0 -- so it must be row 0, where x is 0.
    Returns dict(table [K, 4 | 8], q, qd, goal, origin [R, 3] (the jr frame), rows)."""
    K = len(rows)
    D = SPACING * np.arange(K)[:, None] * np.ones(3)
    tab = np.zeros((K, 8 if capsules else 4), np.float32)
    origin = np.empty((K + ordinary, 3))
    qd = np.zeros((K + ordinary, 4), np.float32)
    for k, r in enumerate(rows):
        shift = GRAZE_SHIFT if r["name"] == "seg_graze_near" else np.zeros(3)
        assert k == 0 or not shift.any()
        a, b = r["a"] - shift + D[k], r["b"] - shift + D[k]
        assert capsules or np.array_equal(a, b)
        tab[k, :3], tab[k, 3] = a, r["r"]
        if capsules:
            tab[k, 4:7] = b
        assert np.array_equal(tab[k, :3].astype(np.float64), a) and (not capsules or np.array_equal(tab[k, 4:7].astype(np.float64), b))
        origin[k] = D[k] - shift
        # the obstacle leaf weighs a pair that is being approached, against the pair's normal (p_link - p_obs) / |.| = sign(gap) u:
        # apart, the hull moves towards the obstacle; in contact the normal has flipped and it moves on inwards -- whichever
        # face a tie takes (the centre, where all six tie, gets a skew velocity)
        P = HULLS[r["hull"]][1]
        u = r["u"] if r["u"] is not None else -np.mean([P[f, :3] for f in r["faces"]], axis=0)
        if r["name"] == "pt_at_centre":
            u = np.array([1.0, 0.5, 0.25])
        qd[k, :3] = -0.25 * (1.0 if r["sep"] - r["r"] >= 0 else -1.0) * u / np.abs(u).max()
    rng = np.random.default_rng(seed)
    origin[K:] = rng.integers(-2048, int(SPACING * K) * 1024 + 2048, size=(ordinary, 3)) / 1024.0
    qd[K:, :3] = rng.integers(-256, 257, size=(ordinary, 3)) / 1024.0
    qd[:, 3] = 0.5
    q = np.zeros((K + ordinary, 4), np.float32)
    q[:, :3] = origin - np.array([0.0, 0.0, 0.75])
    assert np.array_equal(q[:, :3].astype(np.float64), origin - np.array([0.0, 0.0, 0.75]))
    goal = np.ascontiguousarray(origin + np.array([1.5, 0.5, 0.25]), np.float32)
    return dict(table=tab, q=q, qd=qd, goal=goal, origin=origin, rows=list(rows))


def expected_pair(row, origin, point, r=None):
    """The closed form of a "unique" row in the stage's output convention: (p_link, p_obs, dist) -- FK_DISTANCE: the two points in
    the base frame, p_obs = xp + r u; FK_POINT: relative_position hp (frame), normal_vec sign(gap) u (base; the frames do not turn)."""
    r = row["r"] if r is None else r
    gap = row["sep"] - r
    if point:
        return row["hp"], (1.0 if gap >= 0 else -1.0) * row["u"], abs(gap)
    return row["hp"] + origin, row["xp"] + r * row["u"] + origin, abs(gap)


# ---- hull against hull ------------------------------------------------------------------------------------------------------------

def rot_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def rot_y(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])


def _prow(name, B, Rm, t, sep, u=None, pa=None, pb=None, kind="unique", normals=()):
    f = lambda v: None if v is None else np.asarray(v, np.float64)   # noqa: E731
    return dict(name=name, A="cube", B=B, Rm=np.asarray(Rm, np.float64), t=f(t), sep=float(sep), u=f(u), pa=f(pa), pb=f(pb), kind=kind,
                normals=tuple(np.asarray(n, np.float64) for n in normals))


def pair_catalogue():
    """The rows for hull_pair_closest: the unit cube A against a cube B placed by y = Rm y_B + t.  sep is the gap itself; u is the
    unit direction with pa - pb = gap u (-n* under the face rule); `normals` are the n* a tie may choose among.  Rows apart keep a
    gap of 0.18 .. 0.25, within the avoidance leaves' reach."""
    I = np.eye(3)
    ex, ey, ez = I
    c = S2 / 2
    # the existing pinned skew edge pair of test_restatement_pinned_on_unit_cubes: A's edge x = z = 1 against B's edge along (1, 0, -1)
    h = 0.25
    a_, n_ = np.array([1.0, 0, -1]) / S2, np.array([1.0, 0, 1]) / S2
    Rs = np.stack([a_, (n_ + ey) / S2, (n_ - ey) / S2], axis=1)
    mid = np.array([1.0, 0.5, 1.0])
    rows = [
        _prow("faces_apart_aligned", "cube", I, (0, 0, 1.25), 0.25, (0, 0, -1), kind="set"),
        _prow("faces_apart_offset_half", "cube", I, (0.5, 0.5, 1.25), 0.25, (0, 0, -1), kind="set"),
        _prow("faces_apart_rot45", "cube", rot_z(45), (0.5, -0.25, 1.25), 0.25, (0, 0, -1), kind="set"),
        _prow("edges_parallel_apart", "cube", I, (1.125, 0, 1.125), S2 / 8, -n_, kind="set"),
        _prow("edges_skew_apart", "cube", Rs, mid + h * n_ - 0.5 * a_, h, -n_, mid, mid + h * n_),
        _prow("vertices_apart", "cube", I, (1.125, 1.125, 1.125), S3 / 8, -np.ones(3) / S3, (1, 1, 1), (1.125, 1.125, 1.125)),
        # touching: A's face and B's face name the same n*, so u is unique though two faces tie; y* is any vertex of B's face
        _prow("touch_face", "cube", I, (0, 0, 1), 0.0, (0, 0, -1), kind="set"),
        _prow("touch_edge", "cube", I, (1, 0, 1), 0.0, kind="tie", normals=(ex, ez)),
        _prow("touch_vertex", "cube", I, (1, 1, 1), 0.0, kind="tie", normals=(ex, ey, ez)),
        # B turned 45 degrees about y rests its edge (1, ., 0) on A's +z face along x = 0.5
        _prow("edge_on_face", "cube", rot_y(45), (0.5 - c, 0, 1 + c), 0.0, (0, 0, -1), kind="set"),
        _prow("coincident", "cube", I, (0, 0, 0), -1.0, kind="tie", normals=(ex, -ex, ey, -ey, ez, -ez)),
        # a quarter cube inside A, nearest A's +x face (0.375; A's +x and B's -x name the same n*)
        _prow("contained", "small", I, (0.625, 0.375, 0.375), -0.375, (-1, 0, 0), kind="set"),
        _prow("far", "cube", I, (40, 40, 40), 39 * S3, -np.ones(3) / S3, (1, 1, 1), (40, 40, 40)),
    ]
    assert len({r["name"] for r in rows}) == len(rows)
    return rows


def nonfinite_pair_rows():
    """(name, Rm, t): the placement of `vertices_apart` with one value replaced."""
    out = []
    for bad, tag in ((np.nan, "nan"), (np.inf, "inf")):
        for i in range(3):
            t = np.array([1.5, 1.5, 1.5])
            t[i] = bad
            out.append((f"{tag}_in_t{i}", np.eye(3), t))
        Rm = np.eye(3)
        Rm[1, 2] = bad
        out.append((f"{tag}_in_Rm", Rm, np.array([1.5, 1.5, 1.5])))
    return out


def check_pair_row(row, pa, pb, u, gap, tol):
    """Holds one hull-pair answer (A's coordinates) to its catalogue row at `tol`; returns the worst error / tol."""
    (VA, PA), (VB, PB) = HULLS[row["A"]], HULLS[row["B"]]
    pa, pb, u = (np.asarray(v, np.float64) for v in (pa, pb, u))
    what = row["name"]
    assert np.isfinite([*pa, *pb, *u, gap]).all(), (what, pa, pb, u, gap)
    errs = [abs(gap - row["sep"])]
    if row["kind"] == "tie":
        errs.append(min(np.abs(u + n).max() for n in row["normals"]))
    elif row["kind"] != "member":                      # ("member": the caller holds the direction itself, at a bound of its own)
        errs.append(np.abs(u - row["u"]).max())
    if row["kind"] == "unique":
        errs += [np.abs(pa - row["pa"]).max(), np.abs(pb - row["pb"]).max()]
    else:
        errs.append(max(0.0, float((PA[:, :3] @ pa - PA[:, 3]).max())))                 # pa on A
        yb = row["Rm"].T @ (pb - row["t"])
        errs.append(max(0.0, float((PB[:, :3] @ yb - PB[:, 3]).max())))                 # pb on B
        errs.append(np.abs(pa - pb - gap * u).max())                                    # pa - pb = gap u
    worst = max(errs) / tol
    assert worst <= 1.0, (what, row["kind"], errs, tol)
    return worst


def check_self_answer(row, pA, point, pl, po, dd, tol):
    """Holds one pair of the hull SELF stage to its catalogue row at `tol`, with the row's own direction(s): dist = |gap|;
    FK_DISTANCE: p_link - p_obs = gap u, pa = p_link - pA, pb = p_obs - pA; FK_POINT: p_obs = sign(gap) u, pa = p_link,
    pb = pa - gap u; then the row's points, or pa on A and pb on B.  Returns the worst error / tol."""
    (VA, PA), (VB, PB) = HULLS[row["A"]], HULLS[row["B"]]
    gap = row["sep"]
    pl, po = np.asarray(pl, np.float64), np.asarray(po, np.float64)
    us = [row["u"]] if row["kind"] != "tie" else [-n for n in row["normals"]]
    best = None
    for uc in us:
        if point:   # (a row that TOUCHES has gap 0, and sign(g) of a placement that q rounds by 5e-7 is either)
            eu = min(np.abs(po - sg * uc).max() for sg in ((1.0, -1.0) if gap == 0 else (np.sign(gap),)))
            pa = pl
            pb = pa - gap * uc
        else:
            eu = np.abs(pl - po - gap * uc).max()
            pa, pb = pl - pA, po - pA
        if row["kind"] == "unique":
            errs = [eu, np.abs(pa - row["pa"]).max(), np.abs(pb - row["pb"]).max()]
        else:
            yb = row["Rm"].T @ (pb - row["t"])
            errs = [eu, max(0.0, float((PA[:, :3] @ pa - PA[:, 3]).max())), max(0.0, float((PB[:, :3] @ yb - PB[:, 3]).max()))]
        if best is None or max(errs) < max(best):
            best = errs
    best = [abs(dd - abs(gap))] + [float(e) for e in best]
    worst = max(best) / tol
    assert worst <= 1.0, (row["name"], point, best, tol)
    return worst


# ---- the GPU scenes for hull-versus-hull self pairs -----------------------------------------------------------------------------
# Two prismatic x-y-z branches from the base with zero origins: frame az sits at q[0:3] and frame bz at q[3:6], exactly.  Branch b
# carries four unit cubes: on bz itself, and on three fixed frames turned as the catalogue's rotated rows need (45 degrees about z,
# 45 degrees about y, the skew-edge rotation), each displaced by a TWIN_OFFSET that differs from the others in all three
# coordinates.  az carries the unit cube, the base the quarter cube.  Pair leaf 0 sits on az, pair leaf 1 on bz; self pairs
# (0, bz), (0, base), (0, brz), (0, bry), (0, brs), (1, base).  A catalogue row puts ITS body of branch b at the row's placement
# relative to az; every other body then stands beyond A's corner in all three coordinates (unique nearest pairs), and so does A
# from the base (HOME) -- except in the `contained` row, which puts A around the base's quarter cube.  The turned frames' rotations
# are fp32 roundings of the catalogue's (6e-8), and a surd placement rounds in q (5e-7): far below ATOL.
HOME = np.array([4.0, 4.0, 4.0])
TWIN_ORDER = ["ax", "ay", "az", "bx", "by", "bz"]
TWIN_OFFSET = {"bz": (0.0, 0.0, 0.0), "brz": (-8.0, -8.0, 8.0), "bry": (8.0, 8.0, 16.0), "brs": (16.0, -16.0, -8.0)}
_TWIN_PATH = None


def _rpy_of(Rm):
    """roll-pitch-yaw of a rotation in the order the project compiles a joint origin in, R = Rx(roll) Ry(pitch) Rz(yaw)
    (urdf.rotation_from_rpy_reference_order)."""
    return np.arctan2(-Rm[1, 2], Rm[2, 2]), np.arcsin(Rm[0, 2]), np.arctan2(-Rm[0, 1], Rm[0, 0])


def _twin_frame_of(row):
    """Which body of branch b states the row's rotation."""
    for name, Rm in (("bz", np.eye(3)), ("brz", rot_z(45)), ("bry", rot_y(45))):
        if np.allclose(row["Rm"], Rm, atol=1e-12):
            return name
    return "brs"


def _twin_urdf(Rs):
    fixed = ""
    for name, Rm in (("brz", rot_z(45)), ("bry", rot_y(45)), ("brs", Rs)):
        r, p, y = _rpy_of(Rm)
        o = TWIN_OFFSET[name]
        fixed += (f'  <joint name="{name}" type="fixed"><parent link="lb3"/><child link="l{name}"/>'
                  f'<origin xyz="{o[0]} {o[1]} {o[2]}" rpy="{r:.12f} {p:.12f} {y:.12f}"/></joint>\n')
    return f"""<?xml version="1.0"?>
<robot name="twin">
  <link name="base"/><link name="la1"/><link name="la2"/><link name="la3"/><link name="lb1"/><link name="lb2"/><link name="lb3"/>
  <link name="lbrz"/><link name="lbry"/><link name="lbrs"/>
  <joint name="ax" type="prismatic"><parent link="base"/><child link="la1"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/></joint>
  <joint name="ay" type="prismatic"><parent link="la1"/><child link="la2"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/></joint>
  <joint name="az" type="prismatic"><parent link="la2"/><child link="la3"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/></joint>
  <joint name="bx" type="prismatic"><parent link="base"/><child link="lb1"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/></joint>
  <joint name="by" type="prismatic"><parent link="lb1"/><child link="lb2"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/></joint>
  <joint name="bz" type="prismatic"><parent link="lb2"/><child link="lb3"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/></joint>
{fixed}</robot>
""".replace("\\n", "\n")


def _urdf_file(text, prefix):
    import atexit
    import os
    import tempfile
    fd, path = tempfile.mkstemp(prefix=prefix, suffix=".urdf")
    with os.fdopen(fd, "w") as f:
        f.write(text)
    atexit.register(lambda: os.path.exists(path) and os.unlink(path))
    return path


def pack_hulls(entries):
    """urdf.LinkHulls of [(V, P) or None] (None: an empty entry)."""
    from riemannian_motion_policies_amd import urdf as U
    V = [np.zeros((0, 3)) if e is None else e[0] for e in entries]
    P = [np.zeros((0, 4)) if e is None else e[1] for e in entries]
    vo = np.concatenate([[0], np.cumsum([len(v) for v in V])]).astype(np.int32)
    fo = np.concatenate([[0], np.cumsum([len(p) for p in P])]).astype(np.int32)
    return U.LinkHulls(vo, np.ascontiguousarray(np.concatenate(V), np.float32).reshape(-1, 3), fo,
                       np.ascontiguousarray(np.concatenate(P), np.float32).reshape(-1, 4))


def twin(swap=False, solve="auto"):
    """dict(table, desc, hulls, pairs, rows, own, q, qd, goal, pA, frames) of the twin gantry: one robot per row of
    pair_catalogue(), `own[k]` the index of row k's pair among the robot's self pairs; leaf 0 (az) is FK_DISTANCE and leaf 1 (bz)
    FK_POINT, or the other way round with `swap`."""
    global _TWIN_PATH
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    import os
    rows = pair_catalogue()
    if _TWIN_PATH is None or not os.path.exists(_TWIN_PATH):
        _TWIN_PATH = _urdf_file(_twin_urdf(next(r["Rm"] for r in rows if r["name"] == "edges_skew_apart")), "twin_")
    t = U.compile_urdf(_TWIN_PATH, TWIN_ORDER)
    dist = lambda fr: D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr), Cf.OBSTACLE_AVOIDANCE_PARAMS, name=f"avoid_{fr}")   # noqa: E731
    point = lambda fr: D.LeafSpec(D.LEAF_COLLISION_AVOIDANCE, D.TASKMAP_FK_POINT, t.frame_index(fr), Cf.COLLISION_AVOIDANCE_PARAMS, name=f"avoid_{fr}")  # noqa: E731
    specs = [
        D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("az"), Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3, name="attractor"),
        D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping"),
        point("az") if swap else dist("az"),
        dist("bz") if swap else point("bz"),
    ]
    desc = D.build_desc(t, specs, solve)
    fa = t.frame_index("az")
    bodies = ["bz", "brz", "bry", "brs"]
    fb = {n: t.frame_index(n) for n in bodies}
    entries = [None] * (t.n_frames + 1)
    entries[fa], entries[t.n_frames] = HULLS["cube"], HULLS["small"]
    for n in bodies:
        entries[fb[n]] = HULLS["cube"]
    pairs = [(0, fb["bz"]), (0, -1), (0, fb["brz"]), (0, fb["bry"]), (0, fb["brs"]), (1, -1)]
    index = {"bz": 0, "base": 1, "brz": 2, "bry": 3, "brs": 4}
    n = len(rows)
    pA, pB = np.tile(HOME, (n, 1)), np.tile(HOME, (n, 1))
    qd = np.zeros((n, 6), np.float32)
    own = []
    for k, r in enumerate(rows):
        if r["B"] == "small":          # the base's quarter cube inside A: A stands at -t, branch b at home
            pA[k] = -r["t"]
            own.append(index["base"])
        else:
            body = _twin_frame_of(r)
            pB[k] = HOME + r["t"] - np.asarray(TWIN_OFFSET[body])
            own.append(index[body])
        # A approaches the other body along the pair's normal (against sign(gap) u; a tie: towards the mean of its normals)
        m = np.mean(r["normals"], axis=0) if r["u"] is None else None
        u = r["u"] if r["u"] is not None else (-m if np.any(m) else np.array([1.0, 0.5, 0.25]))
        qd[k, :3] = -0.25 * (1.0 if r["sep"] >= 0 else -1.0) * u / np.abs(u).max()
    q = np.ascontiguousarray(np.concatenate([pA, pB], axis=1), np.float32)
    assert np.array_equal(q[:, :3].astype(np.float64), pA)
    goal = np.ascontiguousarray(pA + np.array([1.0, 0.5, 0.25]), np.float32)
    return dict(table=t, desc=desc, hulls=pack_hulls(entries), pairs=pairs, rows=rows, own=own, q=q, qd=qd, goal=goal, pA=pA, frames=(fa, fb))


def many_frames(n_children=22, seed=3):
    """A robot whose hull self pairs name n_children + 1 frames -- more than the 21 frame slots that fit 64 KiB of LDS at 64 robots
    per wave, so the self-hull stage halves its robots per wave: a prismatic x-y-z branch carrying the leaf's quarter cube, and a
    second prismatic branch with n_children fixed frames at random poses (generic: nearest pairs are unique), each a quarter cube."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    rng = np.random.default_rng(seed)
    links = "".join(f'<link name="c{i}"/>' for i in range(n_children))
    joints = ""
    for i in range(n_children):
        xyz = rng.uniform(-0.6, 0.6, 3)
        rpy = rng.uniform(-3.0, 3.0, 3)
        joints += (f'<joint name="f{i}" type="fixed"><parent link="lb"/><child link="c{i}"/>'
                   f'<origin xyz="{xyz[0]:.4f} {xyz[1]:.4f} {xyz[2]:.4f}" rpy="{rpy[0]:.4f} {rpy[1]:.4f} {rpy[2]:.4f}"/></joint>\\n')
    text = f"""<?xml version="1.0"?>
<robot name="many">
  <link name="base"/><link name="la1"/><link name="la2"/><link name="la3"/><link name="lb"/>{links}
  <joint name="ax" type="prismatic"><parent link="base"/><child link="la1"/><origin xyz="0 0 0" rpy="0.3 -0.2 0.5"/><axis xyz="1 0 0"/></joint>
  <joint name="ay" type="prismatic"><parent link="la1"/><child link="la2"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 1 0"/></joint>
  <joint name="az" type="prismatic"><parent link="la2"/><child link="la3"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="0 0 1"/></joint>
  <joint name="bx" type="prismatic"><parent link="base"/><child link="lb"/><origin xyz="0 0 0" rpy="0 0 0"/><axis xyz="1 0 0"/></joint>
  {joints}
</robot>
"""
    path = _urdf_file(text.replace("\\n", "\n"), "many_")
    t = U.compile_urdf(path, ["ax", "ay", "az", "bx"])
    specs = [
        D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("az"), Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3, name="attractor"),
        D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping"),
        D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index("az"), Cf.OBSTACLE_AVOIDANCE_PARAMS, name="avoid_az"),
    ]
    desc = D.build_desc(t, specs, "auto")
    entries = [None] * (t.n_frames + 1)
    children = [t.frame_index(f"f{i}") for i in range(n_children)]
    for f in [t.frame_index("az")] + children:
        entries[f] = HULLS["small"]
    entries[t.n_frames] = HULLS["small"]
    pairs = [(0, f) for f in children] + [(0, -1)]
    return dict(table=t, desc=desc, hulls=pack_hulls(entries), pairs=pairs, slots=1 + n_children)

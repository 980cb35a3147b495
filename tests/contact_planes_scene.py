"""The scenes of the half-space contacts (include/rmp2.h rmp2_dynamics_step_contacts_planes), with their fp64 reference and fp32
envelope (tests/contact_planes_reference.py), and the checks shared by tests/test_contact_planes_host.py and
tests/test_gpu_contact_planes.py.

Robots: the two-joint robot (N = 2), the Panda (N = 9) with urdf.contact_capsules, and one random tree of
test_contacts_host.tree_fleets' kind that has a save slot and a prismatic dof above a contact link.  The catalogue is a list of
GROUPS in the sense of tests/contacts_scene.py: a contact_cases-style dict of VARIANTS robots that share one state q, one sphere
table, one plane table, one capsule table and one box of limits -- what one call shares -- and differ in qd and u; with `planes`,
`group`, `label`, `ref` / `env` (one substep) and `ref_step` / `env_step` (STEP_SUBSTEPS substeps).  All groups run the
acceleration drive, against the fleet's effort limits (`flat`: without them, so that the demanded motion is the applied one).

Every plane's offset is taken from the group's own fp64 pose, so that the stated condition holds by construction (and is asserted
in tests/test_contact_planes_host.py).  The MAIN direction of a robot is the axis direction (+-x, +-y, +-z) along which the
joints move the lowest capsule end point most (the planar two-joint robot cannot move along z); the SIDE direction is the best
one on another axis.  An end's gap is n . X - d - r.

  floor     the main plane 1 mm below the lowest end; the robots move towards it.
  flat      a plane parallel to one link (normal perpendicular to its segment), 0.05 mm below BOTH ends, the capsules of other
            links that reach below it taken off (the two-joint robot's tip sphere is wider than its link); the robots move the link's two ends into it: both end rows are candidates and both multipliers are
            > 0 in the reference, which a single closest point cannot give.
  corner    the main plane and the side plane, each 0.1 mm from its lowest end; the robots move into both.
  mixed     the main plane 0.1 mm below the lowest end and a sphere 0.1 mm below an end of another link (in a table of four, the
            others far away); the robots move into both.
  buried    the main plane 2 cm ABOVE the lowest end's surface: g < 0, b = 0.
  overflow  eight copies of the main plane 1 mm apart, two of them equal (a tie), and the base table: more than 8 rows qualify.
  point     the lowest capsule replaced by one of zero length (a sphere); the main plane 1 mm below it: one row per plane.
  far       the base table and planes 50 m away: no plane candidate."""
import numpy as np

import contact_planes_reference as PR
import contacts_reference as CR
import forward_dynamics_reference as FR
import joint_stops_reference as JR

GROUPS = ("floor", "flat", "corner", "mixed", "buried", "overflow", "point", "far")
VARIANTS = 4
STEP_SUBSTEPS = 4
SEED = 1400
AXES = [np.array(v, float) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]


def _S():
    import test_contacts_host as S          # (imports pytest fixtures; kept out of the module's import time cycle)
    return S


def ends(c, q, caps=None):
    """[(frame, end, X [3], radius)] of every capsule end point at the state q, fp64 (a zero-length capsule: end 0 only)."""
    caps = c["caps"] if caps is None else caps
    R, p, _ = CR.poses(c["t"], np.asarray(q, np.float64)[None])
    out = []
    for f in CR.capsule_frames(caps):
        a, b = caps[f, 0:3].astype(np.float64), caps[f, 4:7].astype(np.float64)
        A = R[f][0] @ a + p[f][0]
        out.append((f, 0, A, float(caps[f, 3])))
        if (a != b).any():
            out.append((f, 1, A + R[f][0] @ (b - a), float(caps[f, 3])))
    return out


def lowest(c, q, n, caps=None):
    """(gap-less height n . X - r of the lowest end along n, its (frame, end))."""
    hs = [(float(n @ X) - r, (f, e)) for f, e, X, r in ends(c, q, caps)]
    return min(hs)


def plane_under(c, q, n, clearance, caps=None):
    """(n, d) with the lowest end along n at gap `clearance`."""
    h, _ = lowest(c, q, n, caps)
    return np.array([*n, h - clearance])


def _row(c, q, plane, frame, end, caps=None, spheres=None):
    """The fp64 row J of plane 0's pair (frame, end) at q."""
    pr = PR.plane_rows(c["t"], c["caps"] if caps is None else caps, plane[None], 0, q[None])
    k = list(pr["idx"]).index(PR.pair_index(c["t"].n_frames, 0, 1, frame, 0, end))
    return pr["J"][0, k]


def directions(c, q):
    """(main, side): see the head."""
    score = []
    for n in AXES:
        _, (f, e) = lowest(c, q, n)
        score.append(np.abs(_row(c, q, np.array([*n, 0.0]), f, e)).sum())
    order = np.argsort(score)[::-1]
    main = int(order[0])
    side = int(next(k for k in order if k // 2 != main // 2))
    return AXES[main], AXES[side]


def _into(rng, c, q, rows, variants=VARIANTS, per_joint=True):
    """(qd, u [variants, n]): velocities and demanded accelerations along -M^-1 sum(rows) -- the velocity that equal impulses on
    the rows take away, so that every one of them is wanted --, variant 0 at full size, the others scaled by factors in
    [0.3, 1] (per joint, or one factor per variant)."""
    n = c["t"].n_dof
    M = FR.mass_matrix(c["t"], c["inert"], np.asarray(q, np.float64)[None])[0]
    d = -np.linalg.solve(M, np.sum(rows, 0))
    d = d / max(np.abs(d).max(), 1e-12)
    scale = lambda: np.concatenate([np.ones((1, n)), rng.uniform(0.3, 1.0, (variants - 1, n if per_joint else 1)) * np.ones((1, n))])
    return (0.8 * d * scale()).astype(np.float32), (5.0 * d * scale()).astype(np.float32)


def _group(base, group, q, qd, u, spheres, planes, caps=None, lim="base"):
    S = _S()
    c = dict(name=base["name"], t=base["t"], inert=base["inert"], g=base["g"], caps=base["caps"] if caps is None else caps,
             drive=FR.ACCEL, lim=base["lim"] if isinstance(lim, str) else lim, limits=base["limits"], substeps=1, group=group, label=f"{base['name']}-{group}",
             spheres=np.ascontiguousarray(spheres, np.float32).reshape(-1, 4),
             planes=np.ascontiguousarray(planes, np.float32).reshape(-1, 4),
             q=np.ascontiguousarray(np.repeat(q[None], len(qd), 0), np.float32), qd=np.ascontiguousarray(qd, np.float32),
             u=np.ascontiguousarray(u, np.float32))
    step = lambda k, env: PR.dynamics_step(c["t"], c["inert"], c["caps"], c["spheres"], c["planes"], S.D_ACT, c["q"], c["qd"], c["u"],
                                           c["drive"], S.DT, k, c["lim"], c["limits"], c["g"], envelope=env)
    c["ref"], c["env"] = step(1, False), step(1, True)
    c["ref_step"], c["env_step"] = step(STEP_SUBSTEPS, False), step(STEP_SUBSTEPS, True)
    return c


def _flat_planes(c, q):
    """[(plane, frame, the other capsule frames that reach below the plane)], best first: planes parallel to a link with at least two dofs above it (one dof moves both ends along
    one row), 0.05 mm below both its ends, the normal turned about the segment; those with clearly independent end rows first, then those that fewer other
    links are below."""
    S = _S()
    t, caps = c["t"], c["caps"]
    es = ends(c, q)
    segs = {}
    for f, e, X, r in es:
        segs.setdefault(f, {})[e] = X
    found = []
    for f, se in segs.items():
        if 1 not in se:
            continue
        D = se[1] - se[0]
        a = np.cross(D, [0.3, 0.5, 0.8])
        a /= np.linalg.norm(a)
        b = np.cross(D, a)
        b /= np.linalg.norm(b)
        for ang in np.linspace(0, 2 * np.pi, 24, endpoint=False):
            n = np.cos(ang) * a + np.sin(ang) * b
            d = float(n @ se[0]) - float(caps[f, 3]) - 5e-5
            plane = np.array([*n, d])
            j0, j1 = _row(c, q, plane, f, 0), _row(c, q, plane, f, 1)
            sigma = float(np.linalg.svd(np.stack([j0, j1]), compute_uv=False)[-1])      # (two rows that one impulse cannot serve)
            below = sorted({g for g, e, X, r in es if g != f and float(n @ X) - d - r < 1e-3})
            if sigma > 1e-2:
                found.append(((sigma > 0.1, -len(below), sigma), plane, f, below))
    assert found, "no link to lay flat"
    return [(plane, f, below) for _, plane, f, below in sorted(found, key=lambda x: x[0], reverse=True)]


def both_ends_active(c):
    """bool [B]: the reference holds the flat link at both ends (both end rows candidates, both multipliers > 0)."""
    F, f = c["t"].n_frames, c["flat_frame"]
    want = [PR.pair_index(F, len(c["spheres"]), len(c["planes"]), f, 0, e) for e in (0, 1)]
    ref = c["ref"]
    return np.array([all(((ref["pair"][r] == w) & (ref["lam"][r] > 0)).any() for w in want) for r in range(len(c["q"]))])


def _sphere_under(c, q, plane, radius=0.05, clearance=1e-4):
    """(table [4, 4], the sphere's fp64 row): a sphere `clearance` below a capsule end of another link than the one the plane
    touches, along the plane's normal made perpendicular to that link -- the end whose row is most independent of the touching row, among those where the sphere
    is inside no link -- as record 2 of a table whose other records are far away."""
    n = plane[:3]
    _, (fa, ea) = lowest(c, q, n)
    ja = _row(c, q, plane, fa, ea)
    best = None
    es = ends(c, q)
    for f, e, X, r in es:
        if f == fa:
            continue
        other = [Y for g, e2, Y, _ in es if g == f and e2 != e]
        m = n.copy()
        if other:          # (perpendicular to the link, so that the end is the link's nearest point)
            D = other[0] - X
            m = n - (n @ D) / (D @ D) * D
            if np.linalg.norm(m) < 0.1:
                continue
            m /= np.linalg.norm(m)
        centre = X - m * (r + radius + clearance)
        one = np.array([[*centre, radius]], np.float32)
        pr = CR.pair_rows(c["t"], c["caps"], one, q[None])
        k = list(pr["idx"]).index(f)
        if pr["gap"].min() < 0.5 * clearance or pr["gap"][0, k] > 2 * clearance:
            continue
        sigma = float(np.linalg.svd(np.stack([ja, pr["J"][0, k]]), compute_uv=False)[-1])
        if best is None or sigma > best[0]:
            best = (sigma, one, pr["J"][0, k])
    assert best is not None and best[0] > 1e-2, "no end to put a sphere under"
    table = np.array([[30.0, 20.0, 10.0, 0.1], [-30.0, 5.0, 2.0, 0.2], best[1][0], [12.0, -7.0, 5.0, 0.05]], np.float32)
    return table, best[2]


def _base_cases(golden_dir, tmp_dir):
    """The three robots' base cases (acceleration drive), each with `r0`: a robot whose reference has an active sphere contact."""
    S = _S()
    out = [c for c in S.contact_cases(golden_dir, seed=500, fleets=(("panda", 64), ("two_joint", 64))) if c["drive"] == FR.ACCEL]
    out = sorted(out, key=lambda c: c["name"] != "two_joint")
    for name, t, inert, caps, q, qd, qdd, spheres in S.tree_fleets(tmp_dir):
        frames = CR.capsule_frames(caps)
        if int(t.depth_first_schedule()[3]) >= 1 and any(S.prismatic_ancestors(t, f) for f in frames):
            drive, u, lim = S.fleet_inputs(t, inert, S.H.GRAVITY, q, qd, qdd)[0]
            limits = JR.table_limits(t)
            ref = CR.dynamics_step(t, inert, caps, spheres, S.D_ACT, q, qd, u, drive, S.DT, 1, lim, limits, S.H.GRAVITY)
            out.append(dict(name=name, t=t, inert=inert, g=S.H.GRAVITY, caps=caps, spheres=spheres, q=q, qd=qd, u=u, drive=drive,
                            lim=lim, limits=limits, ref=ref, substeps=1, tree=True))
            break
    else:
        raise AssertionError("no tree with a save slot and a prismatic dof above a contact link")
    for c in out:
        c["r0"] = int(np.nonzero(c["ref"]["n_contact"] >= 1)[0][0])
    return out


_built = {}


def catalogue(golden_dir, tmp_dir):
    """The groups, robot by robot (two_joint, panda, the tree) in GROUPS' order; built once per process."""
    if "groups" not in _built:
        _built["groups"] = _catalogue(golden_dir, tmp_dir)
    return _built["groups"]


def _catalogue(golden_dir, tmp_dir):
    rng = np.random.default_rng(SEED)
    out = []
    for base in _base_cases(golden_dir, tmp_dir):
        q = base["q"][base["r0"]].astype(np.float64)
        q32 = base["q"][base["r0"]]
        main, side = directions(base, q)
        none = np.zeros((0, 4), np.float32)

        def touching(plane, caps=None):
            _, (f, e) = lowest(base, q, plane[:3], caps)
            return _row(base, q, plane, f, e, caps)

        def sphere_rows():
            ref = base["ref"]
            return [ref["J"][base["r0"], k] for k in range(int(ref["n_cand"][base["r0"]])) if ref["lam"][base["r0"], k] > 0]

        floor = plane_under(base, q, main, 1e-3)
        near = plane_under(base, q, main, 1e-4)
        qd, u = _into(rng, base, q, [touching(floor)])
        out.append(_group(base, "floor", q32, qd, u, none, floor))

        for flat, f, below in _flat_planes(base, q)[:24]:          # (the first on which the reference holds both ends in every variant)
            caps = base["caps"].copy()
            caps[below] = 0          # (a capsule that reaches below the plane would carry the link's end: it is taken off)
            qd, u = _into(rng, base, q, [_row(base, q, flat, f, 0), _row(base, q, flat, f, 1)], per_joint=False)
            g = dict(_group(base, "flat", q32, qd, u, none, flat, caps=caps, lim=None), flat_frame=f)
            if both_ends_active(g).all():
                break
        out.append(g)

        wall = plane_under(base, q, side, 1e-4)
        qd, u = _into(rng, base, q, [touching(near), touching(wall)], per_joint=False)
        out.append(_group(base, "corner", q32, qd, u, none, np.stack([near, wall])))

        table, srow = _sphere_under(base, q, near)
        qd, u = _into(rng, base, q, [touching(near), srow], per_joint=False)
        out.append(_group(base, "mixed", q32, qd, u, table, near))

        buried = plane_under(base, q, main, -0.02)
        qd, u = _into(rng, base, q, [touching(buried)])
        qd[1::2] = -qd[1::2]          # (and away from it)
        out.append(_group(base, "buried", q32, qd, u, none, buried))

        six = np.stack([plane_under(base, q, main, 1e-3 + 1e-3 * k) for k in (0, 1, 2, 2, 3, 4, 5, 6)])
        qd, u = _into(rng, base, q, [touching(floor)] + sphere_rows())
        out.append(_group(base, "overflow", q32, qd, u, base["spheres"], six))

        caps = base["caps"].copy()
        _, (fl, _e) = lowest(base, q, main)
        caps[fl, 4:7] = caps[fl, 0:3]
        dot = plane_under(base, q, main, 1e-3, caps)
        qd, u = _into(rng, base, q, [touching(dot, caps)])
        out.append(dict(_group(base, "point", q32, qd, u, none, dot, caps=caps), point_frame=fl))

        far = np.stack([plane_under(base, q, main, 50.0), plane_under(base, q, side, 50.0)])
        sel = np.arange(base["r0"], base["r0"] + VARIANTS) % len(base["q"])
        g = _group(base, "far", q32, base["qd"][sel], base["u"][sel], base["spheres"], far)
        out.append(g)
    return out


def active_records(c):
    """[B] sets of (kind, record) with a multiplier > 0 in the group's reference."""
    F, K, P = c["t"].n_frames, len(c["spheres"]), len(c["planes"])
    ref = c["ref"]
    return [{PR.split_pair(p, F, K, P)[0::2] for p, l in zip(ref["pair"][r], ref["lam"][r]) if p >= 0 and l > 0} for r in range(len(c["q"]))]


def for_robot(groups, name):
    return [c for c in groups if c["name"] == name]


def robots(groups):
    return list(dict.fromkeys(c["name"] for c in groups))


# ---- the checks ----------------------------------------------------------------------------------------------------------------

def per_robot_ratios(c, got, ref=None):
    """contacts_scene.per_robot_ratios with the plane pairs: dict(res, vel, force, gap) of [B] arrays against the one-substep
    reference."""
    S = _S()
    t, inert, g = c["t"], c["inert"], c["g"]
    ref = c["ref"] if ref is None else ref
    got = {k: np.asarray(got[k], np.float64) for k in ("q", "qd", "qdd", "stop", "contact")}
    res = CR.residual(t, inert, c["q"], c["qd"], got["qdd"], ref["tau"], got["stop"], got["contact"], g) / CR.residual_bracket(t, inert, c["q"], c["qd"], ref, g)
    vel = np.abs(got["qd"] - ref["qd"]).max(1) / CR.velocity_bracket(ref, c["qd"], S.DT)
    force = np.abs(got["stop"] + got["contact"] - ref["stop"] - ref["contact"]).max(1) / CR.force_bracket(ref)
    lg_ref, jn = PR.linearised_gaps(c, ref["qd"], ref["pair"], S.DT)
    lg_got, _ = PR.linearised_gaps(c, got["qd"], ref["pair"], S.DT)
    gap = np.nan_to_num(np.abs(lg_got - lg_ref) / gap_bracket(c, jn)).max(1)
    return dict(res=res, vel=vel, force=force, gap=gap)


def gap_bracket(c, jn):
    S = _S()
    return 1e-6 + S.DT * JR.velocity_bracket(c["ref"], c["qd"], S.DT)[:, None] * np.maximum(1.0, jn)


def step_ratios(c, got, ref=None):
    """[B]: the worse of |q - q_ref| and |qd - qd_ref| over forward_dynamics_reference.step_brackets after STEP_SUBSTEPS."""
    S = _S()
    ref = c["ref_step"] if ref is None else ref
    bq, bqd = CR.step_brackets(ref, S.DT, STEP_SUBSTEPS)
    return np.maximum(np.abs(got["q"] - ref["q"]).max(1) / bq, np.abs(got["qd"] - ref["qd"]).max(1) / bqd)


def kept(c, K):
    """4.12's kept rule, from the reference and the envelope alone: neither is capped and the envelope is within K / 4 on every
    one-substep bound."""
    ratios = per_robot_ratios(c, c["env"])
    ok = ~np.asarray(c["env"]["capped"], bool) & ~np.asarray(c["ref"]["capped"], bool)
    for k in ("res", "vel", "force", "gap"):
        ok &= ratios[k] <= 0.25 * K[k]
    return ok


def kept_step(c, K):
    e, r = c["env_step"], c["ref_step"]
    return kept(c, K) & ~np.asarray(e["capped"], bool) & ~np.asarray(r["capped"], bool) & (step_ratios(c, e) <= 0.25 * K["step"])


def hard_invariants(c, got, K, what):
    """On every robot, whatever ended the solver: finite outputs, the velocity box held exactly, lambda >= 0, empty slots 0 / -1,
    no candidate row below minus the gap bound, joints that started inside their limits end inside exactly."""
    S = _S()
    for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
        assert np.isfinite(got[k]).all(), (what, k)
    lam, pair = np.asarray(got["lam"], np.float64), np.asarray(got["pair"])
    assert (lam >= 0).all() and (lam[pair < 0] == 0).all(), what
    lo, hi = c["limits"]
    own = FR.owned_dofs(c["t"])
    for r in range(len(c["q"])):
        l, h = JR.velocity_box(c["q"][r].astype(np.float32), S.DT, lo, hi, own)
        assert (got["qd"][r] >= l).all() and (got["qd"][r] <= h).all(), (what, r)
    lg, jn = PR.linearised_gaps(c, got["qd"], pair, S.DT)
    br = K["gap"] * gap_bracket(c, jn)
    assert not (lg < -br).any(), (what, np.nanmin(lg + br))
    inside(c, got, what)


def inside(c, got, what):
    lo, hi = c["limits"]
    own = FR.owned_dofs(c["t"])
    q0, q1 = c["q"], got["q"]
    ins_lo, ins_hi = own & (q0 >= lo), own & (q0 <= hi)
    assert (q1[ins_lo] >= np.broadcast_to(lo, q1.shape)[ins_lo]).all() and (q1[ins_hi] <= np.broadcast_to(hi, q1.shape)[ins_hi]).all(), what


def check_group(c, got, K, what, worst=None):
    """The one-substep checks of a group: the candidate pair set of the reference, the hard invariants on every robot, the bounds
    K on the kept ones (and no RMP2_STOP_CAPPED there).  Adds the kept robots' worst ratios to `worst`; returns how many were kept."""
    assert np.array_equal(np.sort(got["pair"], 1), np.sort(c["ref"]["pair"], 1)), (what, got["pair"].tolist(), c["ref"]["pair"].tolist())
    assert np.array_equal((got["status"] & CR.OVERFLOW) != 0, c["ref"]["overflow"]), what
    hard_invariants(c, got, K, what)
    keep = kept(c, K)
    if keep.any():
        ratios = per_robot_ratios(c, got)
        for k in ("res", "vel", "force", "gap"):
            print(what, k, float(ratios[k][keep].max()))
            if worst is not None:
                worst[k] = max(worst.get(k, 0.0), float(ratios[k][keep].max()))
            assert (ratios[k][keep] <= K[k]).all(), (what, k, ratios[k].tolist())
        assert not (np.asarray(got["status"])[keep] & CR.CAPPED).any(), what
    return int(keep.sum())


def check_group_step(c, got, K, what, worst=None):
    """After STEP_SUBSTEPS substeps: finite, lambda >= 0, inside the limits; q / qd within K["step"] on kept_step's robots."""
    for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
        assert np.isfinite(got[k]).all(), (what, k)
    assert (np.asarray(got["lam"]) >= 0).all(), what
    inside(c, got, what)
    keep = kept_step(c, K)
    if keep.any():
        r = step_ratios(c, got)
        print(what, "step", float(r[keep].max()))
        if worst is not None:
            worst["step"] = max(worst.get("step", 0.0), float(r[keep].max()))
        assert (r[keep] <= K["step"]).all(), (what, r.tolist())
    return int(keep.sum())


# ---- the mixed fleet of tests/test_gpu_contact_planes.py ------------------------------------------------------------------------

MIXED_R = 130      # two full waves and two lanes


def mixed_fleet(groups, name, R=MIXED_R):
    """One fleet of R lanes of robot `name`: the catalogue's robots round-robin over the groups, so that neighbours come from
    different groups, starting over when the catalogue is used up.  dict(q, qd, u [R, n], lane_group, lane_robot [R], groups).  A
    launch shares the tables: the fleet is launched once per group with that group's tables, and the group's lanes are compared."""
    gs = for_robot(groups, name)
    order = [(g, r) for r in range(VARIANTS) for g in range(len(gs))]
    n = gs[0]["t"].n_dof
    q, qd, u = (np.zeros((R, n), np.float32) for _ in range(3))
    lane_group, lane_robot = np.zeros(R, int), np.zeros(R, int)
    for lane in range(R):
        g, r = order[lane % len(order)]
        q[lane], qd[lane], u[lane] = gs[g]["q"][r], gs[g]["qd"][r], gs[g]["u"][r]
        lane_group[lane], lane_robot[lane] = g, r
    return dict(name=name, q=q, qd=qd, u=u, lane_group=lane_group, lane_robot=lane_robot, groups=gs)


def lanes_of(fleet, g):
    """(the lanes of group g, those lanes' robots in the group)."""
    lanes = np.nonzero(fleet["lane_group"] == g)[0]
    return lanes, fleet["lane_robot"][lanes]


def rows_of(c, robots_):
    """The group with its robots repeated / reordered as `robots_`: every per-robot array of it, its references included."""
    B = len(c["q"])
    cut = lambda d: {k: (v[robots_] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == B else v) for k, v in d.items()}
    out = dict(c, q=c["q"][robots_], qd=c["qd"][robots_], u=c["u"][robots_])
    for k in ("ref", "env", "ref_step", "env_step"):
        out[k] = cut(c[k])
    return out

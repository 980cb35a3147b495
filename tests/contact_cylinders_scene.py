"""The scenes of the exact flat-capped cylinder contacts (include/rmp2.h rmp2_dynamics_step_contacts_cylinders), with their fp64
reference and fp32 envelope (tests/contact_cylinders_reference.py), and the checks shared by tests/test_contact_cylinders_host.py
and tests/test_gpu_contact_cylinders.py.

Robots: those of tests/contact_self_scene.py -- the two-joint robot (N = 2), the Panda (N = 9), one random tree with a save slot and
a prismatic dof, and slot_catalogue's tree without a save slot and tree with two.  A GROUP is, as there, VARIANTS robots that share
one state q, the obstacle tables, one table of link capsules, one pair list and one box of limits and differ in qd and u; with
`cylinders` [Y, 8], `planted` (frame, cylinder of the pair the group is about), `group`, `label`, `ref` / `env` (one substep) and
`ref_step` / `env_step` (STEP_SUBSTEPS substeps).

Every cylinder is placed from the group's own fp64 pose (_plant): a link with a segment (A, D, r_f), u = D / |D|, a unit direction e
perpendicular to u (6 of them), k = u x e; of the links and directions that give the stated regime in fp64 AND in the fp32
envelope, the one whose row moves the robot most (|J|_1 >= 0.2 first), then those where no other link is within d_act.  The
cylinders have radius CYL_R and half height CYL_H unless stated.  The robots move along -M^-1 J, into the contact.

  side          mid-segment against the lateral surface at mid-height: axis k, centre X0 + (r_f + gap + r) e, X0 = A + D / 2.
  cap           a link end over the flat end, the axis 0.3 r beside it, along the link or leaning 60 degrees off it beyond the end:
                s clamped, n = -+ the axis.
  rim           mid-segment against the rim, tangent to it: outward cap direction (e + k) / sqrt 2, radial (e - k) / sqrt 2 at the
                rim point X0 - (r_f + gap) e: the quartic case, normal e with equal axial and radial parts.
  tip, base     the link's far / near end against the lateral surface, the normal leaning beyond the end: s clamped at 1 / at 0 by
                the end tests.
  alongside     the link parallel to the axis beside the side: a flat minimum.  Where the robot has a frame whose z axis is the
                world's in every arithmetic (contact_capsules_scene.exact_z_frame): a vertical link capsule of length 1/8 beside a
                vertical cylinder that covers it -- the slope n . D is exactly 0 at s = 0 in fp64 and fp32, s = 0 (asserted).  Else
                (the trees): parallel to rounding, and the robots at rest without effort limits, so that a choice of X that is
                nobody's decides nothing.
  over_cap      the link parallel to the cap plane above it, inside the cap's disc (r = 0.1): a flat minimum, exact / at rest alike.
  on_axis       the link's far end on the cylinder's axis over the cap: rho = 0 -- exactly, in both arithmetics, where the robot has
                an exact frame on the world's z axis (the row has no lever there: at rest) -- point_cylinder's fixed perpendicular.
  pierced_side  the link's axis 1 cm inside the lateral surface at mid-height, mid-segment: sd < 0, n radial.
  pierced_cap   the link's far end 1 cm under the cap, 0.3 r beside the axis: sd < 0, n = -u.
  disc          `cap` with half height 0.
  mixed         contact_self_scene's `mixed` (a sphere, the floor, a post and a self pair, each 0.1 mm away) and a cylinder beside
                a link, 0.1 mm away: five kinds compete.
  overflow      nine cylinders behind each other, 1 mm apart, beside one link: cylinder rows among the kept and the dropped.
  graze         the rim's diagonal corner towards the link -- the cull's bound L is the gap itself there --, five cylinders at the
                gaps d_act - 4e-6, d_act + 4e-6, d_act + m -+ 8e-6 and d_act + 2 m - 4e-6 (4e-6: forty times the rounding of a
                gap): the gaps straddle d_act, the bounds L the cull's threshold d_act + m, each L within m of the threshold but
                the first record's, which is 4e-6 further (L <= g: a gap below d_act has its L below d_act).
  far           contact_self_scene's `far` and configs.EXP06_CYLINDERS 50 m away: every cylinder culled.
  buried        `side` 2 cm inside the link's capsule: g < 0 with the axis outside the solid."""
import numpy as np

import contact_capsules_scene as QS
import contact_cylinders_reference as YR
import contact_planes_scene as PS
import contact_self_scene as SS
import contacts_reference as CR
import forward_dynamics_reference as FR
import joint_stops_reference as JR
from riemannian_motion_policies_amd import configs as Cf

GROUPS = ("side", "cap", "rim", "tip", "base", "alongside", "over_cap", "on_axis", "pierced_side", "pierced_cap", "disc", "mixed",
          "overflow", "graze", "far", "buried")
PUSHED = ("side", "cap", "rim")
FLAT = ("alongside", "over_cap")
VARIANTS = PS.VARIANTS
STEP_SUBSTEPS = PS.STEP_SUBSTEPS
SEED, SLOT_SEED = 1700, 1701
CYL_R, CYL_H = 0.05, 0.15
GAP = 1e-3
NONE4, NONE8, NONE2 = QS.NONE4, QS.NONE8, SS.NONE2

_S = PS._S
for_robot, robots, lanes_of, MIXED_R, rows_of, mixed_fleet = PS.for_robot, PS.robots, PS.lanes_of, PS.MIXED_R, PS.rows_of, PS.mixed_fleet


def record(c, r, u, h):
    """The RMP2_PRIM_CYLINDER record (configs.cylinder_record's layout) of centre c, radius r, axis u (normalised here) and half height h."""
    return np.array([*c, r, *(np.asarray(u, np.float64) / np.linalg.norm(u)), h], np.float32)


def detail(c, q, cylinders, caps=None, dtype=np.float64):
    return YR.cylinder_rows(c["t"], c["caps"] if caps is None else caps, cylinders, 0, 0, 0, np.asarray(q, dtype)[None], dtype, detail=True)


def cull_bound(c, q, cylinders, caps=None, dtype=np.float32):
    """{(frame, y): (L, m)}: the cull's lower bound of the gap and its margin (rmp2_contacts.h), in `dtype`."""
    dtype = np.dtype(dtype)
    caps = np.asarray(c["caps"] if caps is None else caps, dtype)
    R, p, _ = CR.poses(c["t"], np.asarray(q, dtype)[None], dtype)
    out = {}
    for f in CR.capsule_frames(caps):
        A = (R[f][0] @ caps[f, 0:3] + p[f][0]).astype(dtype)
        D = (R[f][0] @ (caps[f, 4:7] - caps[f, 0:3])).astype(dtype)
        dd = (D * D).sum(dtype=dtype)
        for y, rec in enumerate(np.asarray(cylinders, dtype).reshape(-1, 8)):
            t = np.clip(((rec[0:3] - A) * D).sum(dtype=dtype) * (dtype.type(1) / dd if dd > 0 else dtype.type(0)), 0, 1).astype(dtype)
            dv = (A + t * D - rec[0:3]).astype(dtype)
            dist, rho = np.sqrt((dv * dv).sum(dtype=dtype)), np.sqrt(rec[3] * rec[3] + rec[7] * rec[7])
            out[(f, y)] = (float(dist - rho - caps[f, 3]), float(dtype.type(1e-4) * (1 + dist + rho)))
    return out


def _make(kind, A, D, rf, e, gap, r=CYL_R, h=CYL_H):
    """The record of `kind` against the segment (A, D, r_f) in the direction e: see the head."""
    u = D / np.linalg.norm(D)
    k = np.cross(u, e)
    X0, B = A + 0.5 * D, A + D
    if kind in ("side", "buried", "pierced_side"):
        return [record(X0 + (rf + gap + r) * e, r, k, h)]
    if kind in ("cap", "disc", "pierced_cap", "on_axis"):      # either end, the axis along the link or leaning 60 degrees off it
        off = 0.0 if kind == "on_axis" else 0.3 * r
        out = []
        for end, sign in ((B, 1.0), (A, -1.0)):
            for lean in ((1.0, 0.5) if sign > 0 else (0.5,)):
                m = sign * lean * u + np.sqrt(1 - lean * lean) * e
                out.append(record(end + (rf + gap + h) * m + off * k, r, m, h))
        return out
    if kind == "rim":
        w, er = (e + k) / np.sqrt(2), (e - k) / np.sqrt(2)
        return [record(X0 - (rf + gap) * e - h * w - r * er, r, w, h)]
    if kind == "graze":      # the diagonal corner (h w + r e_r) / rho towards the link
        rho = np.hypot(r, h)
        w, er = (h * e + r * k) / rho, (r * e - h * k) / rho
        return [record(X0 - (rf + gap) * e - h * w - r * er, r, w, h)]
    if kind in ("tip", "base"):
        end, sign = (B, 1.0) if kind == "tip" else (A, -1.0)
        m = 0.5 * sign * u + np.sqrt(0.75) * e
        return [record(end + (rf + gap + r) * m, r, np.cross(m, k) / np.linalg.norm(np.cross(m, k)), h)]
    if kind == "alongside":
        return [record(X0 + (rf + gap + r) * e, r, u, h)]
    if kind == "over_cap":
        return [record(X0 - (rf + gap + h) * e, r, e, h)]
    raise KeyError(kind)


REGIME = dict(
    side=lambda d: 0.2 < d["s"] < 0.8 and abs(d["a"]) < 0.1 * CYL_H and d["sd"] > 0,
    buried=lambda d: 0.2 < d["s"] < 0.8 and abs(d["a"]) < 0.1 * CYL_H and d["sd"] > 0,
    pierced_side=lambda d: 0.2 < d["s"] < 0.8 and abs(d["a"]) < 0.1 * CYL_H and d["sd"] < 0 and abs(d["nu"]) < 1e-3,
    cap=lambda d: d["s"] in (0.0, 1.0) and abs(abs(d["nu"]) - 1) < 1e-6 and d["sd"] > 0,
    disc=lambda d: d["s"] in (0.0, 1.0) and abs(abs(d["nu"]) - 1) < 1e-6 and d["sd"] > 0,
    on_axis=lambda d: d["s"] in (0.0, 1.0) and abs(abs(d["nu"]) - 1) < 1e-6 and d["sd"] > 0,
    pierced_cap=lambda d: d["s"] in (0.0, 1.0) and abs(abs(d["nu"]) - 1) < 1e-6 and d["sd"] < 0,
    rim=lambda d: 0.2 < d["s"] < 0.8 and 0.5 < abs(d["nu"]) < 0.9 and d["sd"] > 0,
    graze=lambda d: 0.2 < d["s"] < 0.8 and 0.1 < abs(d["nu"]) < 0.995 and d["sd"] > 0,
    tip=lambda d: d["s"] == 1.0 and abs(d["nu"]) < 1e-3 and d["sd"] > 0,
    base=lambda d: d["s"] == 0.0 and abs(d["nu"]) < 1e-3 and d["sd"] > 0,
    alongside=lambda d: abs(d["nu"]) < 1e-3 and d["sd"] > 0,
    over_cap=lambda d: abs(abs(d["nu"]) - 1) < 1e-6 and d["sd"] > 0)


def pair_detail(c, q, rec, f, caps=None, dtype=np.float64):
    """dict(s, gap, sd, X, Y, n, J, a: the axial coordinate of X, nu: n . axis) of the pair (frame f, the one record rec)."""
    d = detail(c, q, rec[None], caps, dtype)
    k = list(d["idx"]).index(YR.pair_index(c["t"].n_frames, 0, 0, 0, 1, f, 0))
    caps = c["caps"] if caps is None else caps
    out = {key: d[key][0, k] for key in ("s", "gap", "X", "Y", "n", "J")}
    out["s"], out["gap"] = float(out["s"]), float(out["gap"])
    out["sd"] = out["gap"] + float(np.asarray(caps, dtype)[f, 3])
    out["a"] = float((out["X"] - rec[0:3].astype(dtype)) @ rec[4:7].astype(dtype))
    out["nu"] = float(out["n"] @ rec[4:7].astype(dtype))
    out["others"] = np.delete(d["gap"][0], k)
    return out


def _plant(c, q, kind, gap, caps=None, r=CYL_R, h=CYL_H, frames=None):
    """(record [8], frame, the planted pair's fp64 row): see the head.  gap: the planted pair's gap g = sd - r_f."""
    D_ACT = _S().D_ACT
    best = None
    q32 = np.asarray(q, np.float32)
    for f, (A, D, rf) in QS.segments(c, q, caps).items():
        if not D.any() or (frames is not None and f not in frames):
            continue
        _, a, b = QS._frame_basis(D)
        for ang in np.linspace(0, 2 * np.pi, 6, endpoint=False):
            e = np.cos(ang) * a + np.sin(ang) * b
            for rec in _make(kind, A, D, rf, e, gap, r, h):
                d = pair_detail(c, q, rec, f, caps)
                if not REGIME[kind](d) or abs(d["gap"] - gap) > 2e-6 or not REGIME[kind](pair_detail(c, q32, rec, f, caps, np.float32)):
                    continue
                if len(d["others"]) and d["others"].min() < min(gap, 0.0) + 5e-4:      # (another link nearer than the planted one)
                    continue
                alone = not len(d["others"]) or d["others"].min() > D_ACT + 5e-3
                j1 = float(np.abs(d["J"]).sum())
                score = (j1 >= 0.2, alone, j1)
                if best is None or score > best[0]:
                    best = (score, rec, f, d["J"])
    assert best is not None and best[0][2] > 1e-2, ("nowhere to plant", c["name"], kind)
    return best[1], best[2], best[3]


def _group(base, group, q32, qd, u, cylinders, planted, caps=None, lim="base", spheres=NONE4, planes=NONE4, capsules=NONE8, pairs=NONE2,
           **more):
    S = _S()
    c = dict(name=base["name"], t=base["t"], inert=base["inert"], g=base["g"],
             caps=np.ascontiguousarray(base["caps"] if caps is None else caps, np.float32),
             drive=FR.ACCEL, lim=base["lim"] if isinstance(lim, str) else lim, limits=base["limits"], substeps=1, group=group,
             label=f"{base['name']}-{group}", planted=planted, pairs=np.ascontiguousarray(pairs, np.int32).reshape(-1, 2),
             spheres=np.ascontiguousarray(spheres, np.float32).reshape(-1, 4),
             planes=np.ascontiguousarray(planes, np.float32).reshape(-1, 4),
             capsules=np.ascontiguousarray(capsules, np.float32).reshape(-1, 8),
             cylinders=np.ascontiguousarray(cylinders, np.float32).reshape(-1, 8),
             q=np.ascontiguousarray(np.repeat(np.asarray(q32, np.float32)[None], len(qd), 0), np.float32),
             qd=np.ascontiguousarray(qd, np.float32), u=np.ascontiguousarray(u, np.float32), **more)
    step = lambda k, env: YR.dynamics_step(c["t"], c["inert"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["pairs"],
                                           c["cylinders"], S.D_ACT, c["q"], c["qd"], c["u"], c["drive"], S.DT, k, c["lim"], c["limits"],
                                           c["g"], envelope=env)
    c["ref"], c["env"] = step(1, False), step(1, True)
    c["ref_step"], c["env_step"] = step(STEP_SUBSTEPS, False), step(STEP_SUBSTEPS, True)
    return c


def _exact_flat(base, q, q32, fz, kind):
    """(caps, record, row): the exact vertical link capsule of contact_capsules_scene._exact_link on the exact frame fz and a
    cylinder on a grid beside it (alongside: vertical, covering it; over_cap: with a horizontal axis, its cap
    plane vertical, the link inside the cap's disc): n . D is exactly 0 in every arithmetic.  Of four horizontal directions along the
    coordinate axes (the record stays on the grid) the one whose row moves the robot most; other links within reach lose their capsules."""
    caps = QS._exact_link(base, q32, fz, 0.25)
    R, p, _ = CR.poses(base["t"], q32[None], np.float32)
    A = (R[fz][0] @ caps[fz, 0:3] + p[fz][0]).astype(np.float32).astype(np.float64)
    rf = float(caps[fz, 3])
    best = None
    for m in (np.array(v, float) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0))):
        zmid = np.round((A[2] + 0.0625) * 64) / 64
        if kind == "alongside":
            rec = record([*(A[:2] + (rf + 1e-4 + CYL_R) * m[:2]), zmid], CYL_R, [0, 0, 1], 0.25)
        else:
            rec = record([*(A[:2] + (rf + 1e-4 + CYL_H) * m[:2]), zmid], 0.125, -m, CYL_H)
        d = detail(base, q, rec[None], caps)
        k = list(d["idx"]).index(YR.pair_index(base["t"].n_frames, 0, 0, 0, 1, fz, 0))
        near = [YR.split_pair(int(i), base["t"].n_frames, 0, 0, 0, 1)[1] for j, i in enumerate(d["idx"]) if j != k and d["gap"][0, j] < _S().D_ACT + 5e-3]
        score = (-len(near), float(np.abs(d["J"][0, k]).sum()))
        if best is None or score > best[0]:
            best = (score, rec, d["J"][0, k], near)
    caps = caps.copy()
    caps[best[3]] = 0
    return caps, best[1], best[2]


def _groups_of(rng, bases, self_groups):
    out = []
    for base in bases:
        out.extend(_groups_of_base(rng, base, self_groups))
    return out


def _groups_of_base(rng, base, self_groups):
    S = _S()
    out = []
    t = base["t"]
    n = t.n_dof
    q32 = base["q"][base["r0"]]
    q = q32.astype(np.float64)
    into = lambda rows, **kw: PS._into(rng, base, q, rows, **kw)
    still = np.zeros((VARIANTS, n), np.float32)
    add = lambda group, qd, u, cyl, planted, **kw: out.append(_group(base, group, kw.pop("q32", q32), qd, u, cyl, planted, **kw))

    for kind in ("side", "cap", "rim", "tip", "base"):
        rec, f, row = _plant(base, q, kind, GAP)
        qd, u = into([row])
        add(kind, qd, u, rec, (f, 0))

    fz = QS.exact_z_frame(t)
    for kind in FLAT:
        if fz is not None:
            caps, rec, row = _exact_flat(base, q, q32, fz, kind)
            qd, u = into([row])
            add(kind, qd, u, rec, (fz, 0), caps=caps, exact=True)
        else:
            rec, f, row = _plant(base, q, kind, GAP, r=0.1 if kind == "over_cap" else CYL_R, h=0.3 if kind == "alongside" else CYL_H)
            add(kind, still, still, rec, (f, 0), lim=None, exact=False)

    fa = QS.exact_z_frame(t, on_axis=True)
    if fa is not None:      # the link on the world's z axis, the cylinder above it on the same axis: rho = 0 to the bit
        caps = QS._exact_link(base, q32, fa, 0.0)
        R, p, _ = CR.poses(t, q32[None], np.float32)
        top = (R[fa][0] @ caps[fa, 4:7] + p[fa][0]).astype(np.float32).astype(np.float64)
        rec = record([top[0], top[1], np.round((top[2] + caps[fa, 3] + CYL_H) * 64) / 64 + 1.0 / 1024], CYL_R, [0, 0, 1], CYL_H)
        add("on_axis", still, still, rec, (fa, 0), caps=caps, lim=None, exact=True)
    else:
        rec, f, row = _plant(base, q, "on_axis", GAP)
        qd, u = into([row])
        add("on_axis", qd, u, rec, (f, 0), exact=False)

    # pierced: the gap is -(depth + r_f) of the chosen link, so the links are tried one by one
    for kind in ("pierced_side", "pierced_cap"):
        found = None
        for f, (A, D, rf) in QS.segments(base, q).items():
            if not D.any():
                continue
            try:
                cand = _plant(base, q, kind, -0.01 - rf, frames=[f])
            except AssertionError:
                continue
            if found is None or np.abs(cand[2]).sum() > np.abs(found[2]).sum():
                found = cand
        assert found is not None, ("nowhere to pierce", base["name"], kind)
        rec, f, row = found
        qd, u = into([row])
        qd[1::2] = -qd[1::2]          # (and away from it)
        add(kind, qd, u, rec, (f, 0))

    rec, f, row = _plant(base, q, "disc", GAP, h=0.0)
    qd, u = into([row])
    add("disc", qd, u, rec, (f, 0))

    # mixed: contact_self_scene's mixed group and a cylinder beside one of its links, 0.1 mm away
    sm = next(c for c in self_groups if c["name"] == base["name"] and c["group"] == "mixed")
    qs32 = sm["q"][0]
    qs = qs32.astype(np.float64)
    sbase = dict(base, caps=sm["caps"])
    rec, f, row = _plant(sbase, qs, "side", 1e-4)
    r0 = sm["ref"]
    rows = [r0["J"][0, j] for j in range(int(r0["n_cand"][0]))] + [row]
    qd, u = PS._into(rng, sbase, qs, rows, per_joint=False)
    add("mixed", qd, u, rec, (f, 0), q32=qs32, caps=sm["caps"], spheres=sm["spheres"], planes=sm["planes"], capsules=sm["capsules"],
        pairs=sm["pairs"], self_planted=sm["planted"])

    rec, f, row = _plant(base, q, "side", GAP)
    nrm = pair_detail(base, q, rec, f)["n"]
    nine = np.stack([record(rec[0:3] - 1e-3 * j * nrm, rec[3], rec[4:7], rec[7]) for j in range(9)])
    qd, u = into([row])
    add("overflow", qd, u, nine, (f, 0))

    # graze: gaps around d_act, the cull's bound L around its threshold d_act + m (m is about 1.3e-4 here)
    found = None
    for f, (A, D, rf) in QS.segments(base, q).items():
        if not D.any():
            continue
        try:
            cand = _plant(base, q, "graze", S.D_ACT - 4e-6, frames=[f])
        except AssertionError:
            continue
        if found is None or np.abs(cand[2]).sum() > np.abs(found[2]).sum():
            found = cand
    assert found is not None, ("nowhere to graze", base["name"])
    rec, f, row = found
    nrm = pair_detail(base, q, rec, f)["n"]
    m = cull_bound(base, q32, rec[None])[(f, 0)][1]
    five = np.stack([record(rec[0:3] - off * nrm, rec[3], rec[4:7], rec[7]) for off in (0.0, 8e-6, m - 4e-6, m + 12e-6, 2 * m)])
    qd, u = into([row])
    add("graze", qd, u, five, (f, 0), margin=m)

    sf = next(c for c in self_groups if c["name"] == base["name"] and c["group"] == "far")
    far = Cf.EXP06_CYLINDERS.copy()
    far[:, 0] += 50.0
    add("far", sf["qd"], sf["u"], far, None, q32=sf["q"][0], caps=sf["caps"], spheres=sf["spheres"], pairs=sf["pairs"])

    rec, f, row = _plant(base, q, "buried", -0.02)
    qd, u = into([row])
    qd[1::2] = -qd[1::2]
    add("buried", qd, u, rec, (f, 0))
    return out


_built = {}


def catalogue(golden_dir, tmp_dir):
    """The groups, robot by robot (two_joint, panda, the tree) in GROUPS' order; built once per process."""
    if "groups" not in _built:
        _built["groups"] = _groups_of(np.random.default_rng(SEED), PS._base_cases(golden_dir, tmp_dir), SS.catalogue(golden_dir, tmp_dir))
    return _built["groups"]


def slot_catalogue(tmp_dir):
    """The groups again on contact_capsules_scene.slot_bases' tree without a save slot and tree with two."""
    if "slots" not in _built:
        _built["slots"] = _groups_of(np.random.default_rng(SLOT_SEED), QS.slot_bases(tmp_dir), SS.slot_catalogue(tmp_dir))
    return _built["slots"]


def counts(c):
    return c["t"].n_frames, len(c["spheres"]), len(c["planes"]), len(c["capsules"]), len(c["cylinders"])


def planted_pair(c):
    return YR.pair_index(*counts(c), *c["planted"])


def kinds(c, ref=None):
    """[B] lists of split_pair tuples of the reference's candidates."""
    ref = c["ref"] if ref is None else ref
    return [[YR.split_pair(p, *counts(c)) for p in row if p >= 0] for row in ref["pair"]]


def planted_active(c, got=None):
    """bool [B]: the planted pair is among the candidates with a multiplier > 0 (the reference's, or `got`'s)."""
    got = c["ref"] if got is None else got
    w = planted_pair(c)
    return np.array([((np.asarray(got["pair"][r]) == w) & (np.asarray(got["lam"][r]) > 0)).any() for r in range(len(c["q"]))])


def planted_detail(c, dtype=np.float64):
    f, y = c["planted"]
    return pair_detail(c, c["q"][0].astype(dtype), c["cylinders"][y], f, c["caps"], dtype)


# ---- the checks (tests/contact_self_scene.py's, over the five kinds of pairs) -----------------------------------------------------

gap_bracket = PS.gap_bracket
step_ratios = PS.step_ratios


def per_robot_ratios(c, got, ref=None):
    S = _S()
    t, inert, g = c["t"], c["inert"], c["g"]
    ref = c["ref"] if ref is None else ref
    got = {k: np.asarray(got[k], np.float64) for k in ("q", "qd", "qdd", "stop", "contact")}
    res = CR.residual(t, inert, c["q"], c["qd"], got["qdd"], ref["tau"], got["stop"], got["contact"], g) / CR.residual_bracket(t, inert, c["q"], c["qd"], ref, g)
    vel = np.abs(got["qd"] - ref["qd"]).max(1) / CR.velocity_bracket(ref, c["qd"], S.DT)
    force = np.abs(got["stop"] + got["contact"] - ref["stop"] - ref["contact"]).max(1) / CR.force_bracket(ref)
    lg_ref, jn = YR.linearised_gaps(c, ref["qd"], ref["pair"], S.DT)
    lg_got, _ = YR.linearised_gaps(c, got["qd"], ref["pair"], S.DT)
    gap = np.nan_to_num(np.abs(lg_got - lg_ref) / gap_bracket(c, jn)).max(1)
    return dict(res=res, vel=vel, force=force, gap=gap)


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
    no candidate row below minus the gap bound (the rows are feasible), joints that started inside their limits end inside."""
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
    lg, jn = YR.linearised_gaps(c, got["qd"], pair, S.DT)
    br = K["gap"] * gap_bracket(c, jn)
    assert not (lg < -br).any(), (what, np.nanmin(lg + br))
    status = np.asarray(got["status"])
    assert np.array_equal((status & CR.CONTACT_ACTIVE) != 0, (lam > 0).any(1)), what      # (the status bits)
    PS.inside(c, got, what)


def check_group(c, got, K, what, worst=None):
    """The one-substep checks of a group: the candidate pair set of the reference, the hard invariants on every robot, the bounds
    K on the kept ones (and no RMP2_STOP_CAPPED there).  Adds the kept robots' worst ratios to `worst`; returns how many were kept."""
    assert np.array_equal(np.sort(got["pair"], 1), np.sort(c["ref"]["pair"], 1)), (what, np.asarray(got["pair"]).tolist(), c["ref"]["pair"].tolist())
    assert np.array_equal((np.asarray(got["status"]) & CR.OVERFLOW) != 0, c["ref"]["overflow"]), what
    keep = kept(c, K)
    hard_invariants(c, got, K, what)
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
    PS.inside(c, got, what)
    keep = kept_step(c, K)
    if keep.any():
        r = step_ratios(c, got)
        print(what, "step", float(r[keep].max()))
        if worst is not None:
            worst["step"] = max(worst.get("step", 0.0), float(r[keep].max()))
        assert (r[keep] <= K["step"]).all(), (what, r.tolist())
    return int(keep.sum())

"""A seeded STRESS CATALOGUE for the contact solver (rmp2_contacts.h contacts_solve), with its fp64 reference and fp32 envelope.

The fleets of tests/test_contacts_host.py touch two or three spheres and have at most two joints near a limit; the states here
are the ones an active-set loop finds hard: many stops and several nearly parallel contact rows at once, rows that all block at
the start point, more rows than dofs, overflow of the candidate list.  Robots: the Panda (N = 9) and the two-joint robot
(N = 2), both drives.

The catalogue is a list of GROUPS.  A group is a contact_cases-style dict (test_contacts_host.contact_cases) of a few robots
that share one state q, one sphere table and one box of joint limits -- what one call of the device routine shares -- and
differ in qd and u; beside the fields of contact_cases it has `family`, `label`, `ref` (fp64, one substep), `env` (the fp32
envelope restatement, one substep) and `hard_only`.  Base states are robots with an active contact of
contact_cases(seed=500) at 64 robots per fleet.  Families:

  stops     the first nstop in {n/2, n} joints 1e-4 rad inside a limit on the side s_j = +-1 (random), every other limit at
            +-1e6; qd = 0.8 s, u = 5 s (variant 0; the others scale each joint by a factor in [0.3, 1]); no tau_limit; the
            fleet's own table.
  cluster   the same, the table replaced by 6 copies of the robot's strongest sphere, the centres jittered by N(0, 4 mm) -- and
            one group with 12 copies, where the candidate list overflows as well.
  buried    one and three spheres 2 cm into a link, velocities both ways; the case's own limits.
  overflow  twelve gaps 1 mm apart with one tie (test_device_overflow_keeps_the_eight_smallest_gaps' construction).
  coincident  two spheres on one spot.
  pocket    (two-joint) the end sphere in a pocket of five spheres: more rows want to be active than there are dofs.
  axis      (Panda) a sphere centred on a link's axis in the device's fp32 arithmetic.  hard_only: the fp64 reference's normal
            there is the rounding of its own pose chain, so only the hard invariants are asserted, as in
            test_device_sphere_centred_on_a_link_axis.
  locked    (Panda) the fingers with lower == upper and a sphere touching the hand.

per_robot_ratios / kept / hard_invariants are the checks shared by tests/test_contacts_stress_host.py and
tests/test_gpu_contacts_stress.py.  KEPT, decided without the device: the envelope is uncapped and within K / 4 of the reference
on every bound (the level of MEASURED).  Helpers for those two files only."""
import numpy as np

import contacts_reference as CR
import dynamics_reference as DR
import forward_dynamics_reference as FR
import joint_stops_reference as JR
import test_contacts_host as S
from test_contacts_host import D_ACT, DT, K_FORCE, K_GAP, K_RES, K_VEL

SEED = 900
WIDE = 1e6
N_VARIANTS = 5
FAMILIES = ("stops", "cluster", "buried", "overflow", "coincident", "pocket", "axis", "locked")


def _substeps(c, q, qd, u, substeps=1, envelope=False):
    return CR.dynamics_step(c["t"], c["inert"], c["caps"], c["spheres"], D_ACT, q, qd, u, c["drive"], DT, substeps, c["lim"],
                            c["limits"], c["g"], envelope=envelope)


def _group(base, family, label, q, qd, u, spheres, limits, lim, hard_only=False):
    c = dict(name=base["name"], t=base["t"], inert=base["inert"], g=base["g"], caps=base["caps"], drive=base["drive"], lim=lim,
             spheres=np.ascontiguousarray(spheres, np.float32).reshape(-1, 4), limits=limits, substeps=1, family=family,
             label=f"{base['name']}-{'accel' if base['drive'] == FR.ACCEL else 'torque'}-{family}-{label}", hard_only=hard_only,
             q=np.ascontiguousarray(q, np.float32), qd=np.ascontiguousarray(qd, np.float32), u=np.ascontiguousarray(u, np.float32))
    c["ref"] = _substeps(c, c["q"], c["qd"], c["u"])
    c["env"] = _substeps(c, c["q"], c["qd"], c["u"], envelope=True)
    return c


def _drive_input(base, q, qd, acc):
    """u of the group's drive that asks for the acceleration acc."""
    if base["drive"] == FR.ACCEL:
        return acc.astype(np.float32)
    return DR.rnea(base["t"], base["inert"], q, qd, acc, base["g"]).astype(np.float32)


def _strongest(base, r):
    k = int(base["ref"]["pair"][r, int(np.argmax(base["ref"]["lam"][r]))]) % len(base["spheres"])
    return base["spheres"][k].copy()


def _stop_box(q, signs, nstop):
    n = len(q)
    lo, hi = np.full(n, -WIDE, np.float32), np.full(n, WIDE, np.float32)
    for j in range(nstop):
        if signs[j] > 0:
            hi[j] = np.float32(q[j]) + np.float32(1e-4)
        else:
            lo[j] = np.float32(q[j]) - np.float32(1e-4)
    return lo, hi


def _pressed(rng, base, r, nstop, variants):
    """(q, qd, u [variants, n], limits) of base robot r pressed into a corner of nstop stops."""
    n = base["t"].n_dof
    s = rng.choice([-1.0, 1.0], n)
    scale = np.concatenate([np.ones((1, n)), rng.uniform(0.3, 1.0, (variants - 1, n))])
    q = np.repeat(base["q"][r:r + 1], variants, 0)
    qd = (0.8 * s * scale).astype(np.float32)
    acc = 5.0 * s * np.concatenate([np.ones((1, n)), rng.uniform(0.3, 1.0, (variants - 1, n))])
    return q, qd, _drive_input(base, q, qd, acc), _stop_box(base["q"][r], s, nstop)


def _both_ways(rng, base, r, variants):
    q = np.repeat(base["q"][r:r + 1], variants, 0)
    sign = np.where(np.arange(variants) % 2 == 0, 1.0, -1.0)[:, None]
    scale = np.concatenate([np.ones((2, base["t"].n_dof)), rng.uniform(0.3, 1.0, (variants - 2, base["t"].n_dof))])
    qd = (sign * scale * base["qd"][r]).astype(np.float32)
    return q, qd, np.repeat(base["u"][r:r + 1], variants, 0)


def _hand_sphere(rng, base, r):
    """A sphere touching the Panda's hand capsule (gap 0 .. 1 mm) with no link inside it."""
    t, caps = base["t"], base["caps"]
    hand = max(f for f in CR.capsule_frames(caps) if t.joint_type[f] != 2)      # the last capsule frame that is no finger
    q = base["q"][r:r + 1]
    R, p, _ = CR.poses(t, q)
    A = R[hand][0] @ caps[hand, 0:3].astype(np.float64) + p[hand][0]
    D = R[hand][0] @ (caps[hand, 4:7] - caps[hand, 0:3]).astype(np.float64)
    for _ in range(2000):
        d = rng.normal(size=3)
        if D @ D > 0:
            d = d - (d @ D) / (D @ D) * D
        d = d / np.linalg.norm(d)
        rk = rng.uniform(0.04, 0.08)
        c = A + 0.5 * D + d * (caps[hand, 3] + rk + rng.uniform(0.0, 0.001))
        one = np.array([[c[0], c[1], c[2], rk]], np.float32)
        pr = CR.pair_rows(t, caps, one, q)
        k = list(pr["idx"]).index(hand)
        if pr["gap"].min() > -1e-6 and pr["gap"][0, k] < 0.0015:
            return one
    raise AssertionError("no sphere on the hand found")


_built = {}


def catalogue(golden_dir, seed=SEED, variants=N_VARIANTS):
    """The groups, in a fixed order: per robot (panda, two_joint) and drive (accel, torque), family by family (built once per
    process; nothing changes a group but with_steps, which adds to it)."""
    if (seed, variants) not in _built:
        _built[(seed, variants)] = _catalogue(golden_dir, seed, variants)
    return _built[(seed, variants)]


def _catalogue(golden_dir, seed, variants):
    rng = np.random.default_rng(seed)
    out = []
    for base in S.contact_cases(golden_dir, seed=500, fleets=(("panda", 64), ("two_joint", 64))):
        t, n = base["t"], base["t"].n_dof
        act = np.nonzero(base["ref"]["n_contact"] >= 1)[0]
        rA, rB = int(act[0]), int(act[len(act) // 2])
        half = max(n // 2, 1)
        add = lambda *a, **k: out.append(_group(base, *a, **k))
        for r, nstop in ((rA, half), (rA, n), (rB, n)):
            q, qd, u, box = _pressed(rng, base, r, nstop, variants)
            add("stops", f"r{r}-{nstop}", q, qd, u, base["spheres"], box, None)
        for r, nstop, copies in ((rA, half, 6), (rB, n, 6), (rA, n, 12)):
            q, qd, u, box = _pressed(rng, base, r, nstop, variants)
            one = _strongest(base, r)
            table = np.tile(one, (copies, 1))
            table[:, :3] += rng.normal(0.0, 0.004, (copies, 3))
            add("cluster", f"r{r}-{nstop}-x{copies}", q, qd, u, table, box, None)
        for copies in (1, 3):
            one = _strongest(base, rA)
            table = np.tile(one, (copies, 1))
            table[1:, :3] += rng.normal(0.0, 0.004, (copies - 1, 3))
            table[:, 3] += 0.02
            q, qd, u = _both_ways(rng, base, rA, 4)
            add("buried", f"r{rA}-x{copies}", q, qd, u, table, base["limits"], base["lim"])
        one = _strongest(base, rA)
        table = np.tile(one, (12, 1)).astype(np.float32)
        table[:, 3] = one[3] - 0.001 * np.arange(12)
        table[5, 3] = table[4, 3]
        q, qd, u = _both_ways(rng, base, rA, 4)
        add("overflow", f"r{rA}", q, qd, u, table, base["limits"], base["lim"])
        few = np.nonzero((base["ref"]["n_contact"] >= 1) & (base["ref"]["n_cand"] <= 3))[0]
        rC = int(few[0])
        one = _strongest(base, rC)
        q, qd, u = _both_ways(rng, base, rC, 4)
        add("coincident", f"r{rC}", q, qd, u, np.stack([one, one]), base["limits"], base["lim"])
        if base["name"] == "two_joint":
            q = np.repeat(np.array([[0.4, -0.9]], np.float32), 4, 0)
            _, p, _ = CR.poses(t, q[:1])
            tip, rk = p[2][0], 0.05
            dirs = [np.array([np.cos(a), np.sin(a), 0.0]) for a in (0.3, 1.4, 2.6, 3.9, 5.1)]
            table = np.array([[*(tip + d * (base["caps"][2, 3] + rk + 1e-4)), rk] for d in dirs], np.float32)
            qd = np.array([[2.0, -1.5], [-2.0, 2.0], [0.5, 3.0], [-3.0, -3.0]], np.float32)
            add("pocket", "five", q, qd, _drive_input(base, q, qd, np.zeros((4, 2))), table, base["limits"], None)
        else:
            f = 3
            R32, p32, _ = CR.poses(t, base["q"][:1], np.float32)
            A32 = FR._mv(R32[f], base["caps"][f, 0:3][None].astype(np.float32)) + p32[f]
            add("axis", f"frame{f}", base["q"][:1], base["qd"][:1], base["u"][:1], np.array([[*A32[0], 0.05]], np.float32),
                base["limits"], base["lim"], hard_only=True)
            q, qd, u = _both_ways(rng, base, rA, 4)
            lo, hi = (x.copy() for x in base["limits"])
            for fr in range(t.n_frames):
                if t.joint_type[fr] == 2 and t.q_index[fr] >= 0:
                    lo[int(t.q_index[fr])] = hi[int(t.q_index[fr])] = base["q"][rA, int(t.q_index[fr])]
            add("locked", f"r{rA}", q, qd, u, _hand_sphere(rng, base, rA), (lo, hi), base["lim"])
    return out


def with_steps(groups, substeps=S.STEP_SUBSTEPS):
    """The groups with `ref_step` / `env_step` attached: reference and envelope after `substeps` substeps (computed once)."""
    for c in groups:
        if "ref_step" not in c:
            c["ref_step"] = _substeps(c, c["q"], c["qd"], c["u"], substeps)
            c["env_step"] = _substeps(c, c["q"], c["qd"], c["u"], substeps, envelope=True)
    return groups


def kept_step(c):
    """kept() for the several-substep check: also neither run capped in any substep, the envelope within K_STEP / 4."""
    bq, bqd = CR.step_brackets(c["ref_step"], DT, S.STEP_SUBSTEPS)
    e, r = c["env_step"], c["ref_step"]
    ratio = np.maximum((np.abs(e["q"] - r["q"]).max(1) / bq), (np.abs(e["qd"] - r["qd"]).max(1) / bqd))
    return kept(c) & ~np.asarray(e["capped"], bool) & ~np.asarray(r["capped"], bool) & (ratio <= 0.25 * S.K_STEP)


# ---- the checks ------------------------------------------------------------------------------------------------------------

def subset(c, rows):
    """The group restricted to the robots `rows` (a mask or indices), its reference and envelope with it."""
    B = len(c["q"])
    cut = lambda d: {k: (v[rows] if isinstance(v, np.ndarray) and v.ndim >= 1 and len(v) == B else v) for k, v in d.items()}
    out = dict(c, q=c["q"][rows], qd=c["qd"][rows], u=c["u"][rows], ref=cut(c["ref"]))
    if "env" in c:
        out["env"] = cut(c["env"])
    return out


def per_robot_ratios(c, got):
    """test_contacts_host.one_step_ratios per robot: dict(res, vel, force, gap) of [B] arrays."""
    t, inert, g, ref = c["t"], c["inert"], c["g"], c["ref"]
    got = {k: np.asarray(got[k], np.float64) for k in ("q", "qd", "qdd", "stop", "contact")}
    res = CR.residual(t, inert, c["q"], c["qd"], got["qdd"], ref["tau"], got["stop"], got["contact"], g) / CR.residual_bracket(t, inert, c["q"], c["qd"], ref, g)
    vel = np.abs(got["qd"] - ref["qd"]).max(1) / CR.velocity_bracket(ref, c["qd"], DT)
    force = np.abs(got["stop"] + got["contact"] - ref["stop"] - ref["contact"]).max(1) / CR.force_bracket(ref)
    lg_ref, jn = S.linearised_gaps(c, ref["qd"], ref["pair"])
    lg_got, _ = S.linearised_gaps(c, got["qd"], ref["pair"])
    gap = np.nan_to_num(np.abs(lg_got - lg_ref) / S.gap_bracket(c, jn)).max(1)
    return dict(res=res, vel=vel, force=force, gap=gap)


BOUNDS = dict(res=K_RES, vel=K_VEL, force=K_FORCE, gap=K_GAP)


def kept(c):
    """bool [B], from the reference and the envelope alone: neither is capped, and the envelope is within K / 4 on every bound."""
    if c["hard_only"]:
        return np.zeros(len(c["q"]), bool)
    ratios = per_robot_ratios(c, c["env"])
    ok = ~np.asarray(c["env"]["capped"], bool) & ~np.asarray(c["ref"]["capped"], bool)
    for k, K in BOUNDS.items():
        ok &= ratios[k] <= 0.25 * K
    return ok


def hard_invariants(c, got, what):
    """What holds on every robot, whatever ended the solver: finite outputs, the velocity box held exactly, no candidate row
    below -K_GAP x gap_bracket, lambda >= 0, empty slots 0 / -1, joints inside their limits end inside."""
    for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
        assert np.isfinite(got[k]).all(), (what, k)
    lam, pair = np.asarray(got["lam"], np.float64), np.asarray(got["pair"])
    assert (lam >= 0).all() and (lam[pair < 0] == 0).all(), what
    lo, hi = c["limits"]
    own = FR.owned_dofs(c["t"])
    for r in range(len(c["q"])):
        l, h = JR.velocity_box(c["q"][r].astype(np.float32), DT, lo, hi, own)
        assert (got["qd"][r] >= l).all() and (got["qd"][r] <= h).all(), (what, r)
    if not c["hard_only"]:      # (the rows of an `axis` group in fp64 are not the device's: see the head)
        lg, jn = S.linearised_gaps(c, got["qd"], pair)
        br = K_GAP * S.gap_bracket(c, jn)
        assert not (lg < -br).any(), (what, np.nanmin(lg + br))
    q0, q1 = c["q"], got["q"]
    ins_lo, ins_hi = own & (q0 >= lo), own & (q0 <= hi)
    assert (q1[ins_lo] >= np.broadcast_to(lo, q1.shape)[ins_lo]).all() and (q1[ins_hi] <= np.broadcast_to(hi, q1.shape)[ins_hi]).all(), what


def check_kept(c, got, keep, what):
    """On the kept robots: the bounds K_RES, K_VEL, K_FORCE, K_GAP and check_device_kkt, unchanged, and no RMP2_STOP_CAPPED.
    Returns the per-robot ratios of the kept robots (dict of arrays)."""
    if not keep.any():
        return {k: np.zeros(0) for k in BOUNDS}
    ck, gk = subset(c, keep), {k: np.asarray(v)[keep] for k, v in got.items()}
    ratios = per_robot_ratios(ck, gk)
    for k, K in BOUNDS.items():
        assert (ratios[k] <= K).all(), (what, k, ratios[k].tolist())
    S.check_device_kkt(ck, gk, what)
    assert not (gk["status"] & CR.CAPPED).any(), (what, (gk["status"] >> 8).tolist(), (gk["status"] & 15).tolist())
    return ratios


# ---- the mixed fleet of tests/test_gpu_contacts_stress.py -------------------------------------------------------------------

MIXED_R = 130      # two full waves and two lanes


def mixed_fleet(groups, name, drive, R=MIXED_R):
    """One fleet of R lanes from the groups of robot `name` and `drive`: dict(q, qd, u [R, n], lane_group / lane_robot [R]
    (-1: a clear robot), groups).  Every fourth lane (3, 7, ...) is a robot at least d_act + 0.05 m clear of every group's
    table -- the fast path in every launch; the other lanes take the catalogue's robots round-robin over the groups, so that
    neighbours come from different families, and start over when the catalogue is used up.  A launch shares one table and one
    box of limits: the fleet is launched once per group, with that group's, and the lanes of that group are compared."""
    gs = [c for c in groups if c["name"] == name and c["drive"] == drive]
    rank = [sum(1 for b in gs[:g] if b["family"] == c["family"]) for g, c in enumerate(gs)]      # (groups of one family apart)
    turn = sorted(range(len(gs)), key=lambda g: (rank[g], FAMILIES.index(gs[g]["family"])))
    order = [(g, r) for r in range(max(len(c["q"]) for c in gs)) for g in turn if r < len(gs[g]["q"])]
    t, n = gs[0]["t"], gs[0]["t"].n_dof
    rng = np.random.default_rng(SEED + 1)
    union = np.concatenate([c["spheres"] for c in gs])
    lo, hi = (np.clip(x.astype(np.float64), -3.0, 3.0) for x in JR.table_limits(t))
    n_clear = R // 4
    found = np.zeros((0, n), np.float32)
    while len(found) < n_clear:
        cand = (lo + (hi - lo) * rng.uniform(0.0, 1.0, (8 * n_clear, n))).astype(np.float32)
        found = np.concatenate([found, cand[CR.pair_rows(t, gs[0]["caps"], union, cand)["gap"].min(1) > D_ACT + 0.05]])
    q, qd, u = (np.zeros((R, n), np.float32) for _ in range(3))
    lane_group, lane_robot = np.full(R, -1), np.full(R, -1)
    k = 0
    for lane in range(R):
        if lane % 4 == 3:
            q[lane], qd[lane] = found[lane // 4], rng.uniform(-0.5, 0.5, n)
            u[lane] = _drive_input(gs[0], q[lane:lane + 1], qd[lane:lane + 1], rng.uniform(-1.0, 1.0, (1, n)))[0]
        else:
            g, r = order[k % len(order)]
            k += 1
            q[lane], qd[lane], u[lane] = gs[g]["q"][r], gs[g]["qd"][r], gs[g]["u"][r]
            lane_group[lane], lane_robot[lane] = g, r
    assert k >= len(order)          # every robot of the catalogue has a lane
    return dict(name=name, drive=drive, q=q, qd=qd, u=u, lane_group=lane_group, lane_robot=lane_robot, groups=gs)


def launch_case(fleet, g, rows=slice(None)):
    """The contact_cases-style dict of the fleet's launch for group g (its table, limits and tau_limit; no reference)."""
    c = fleet["groups"][g]
    return dict(c, q=fleet["q"][rows], qd=fleet["qd"][rows], u=fleet["u"][rows], ref=None, env=None)


def lanes_of(fleet, g):
    """(lanes, the group restricted to those lanes' robots, in lane order)."""
    lanes = np.nonzero(fleet["lane_group"] == g)[0]
    return lanes, subset(fleet["groups"][g], fleet["lane_robot"][lanes])


def step_invariants(c, got, what):
    """What holds after several substeps on every robot: finite outputs, lambda >= 0, empty slots 0 / -1, joints that started
    inside their limits are inside."""
    for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
        assert np.isfinite(got[k]).all(), (what, k)
    lam, pair = np.asarray(got["lam"], np.float64), np.asarray(got["pair"])
    assert (lam >= 0).all() and (lam[pair < 0] == 0).all(), what
    lo, hi = c["limits"]
    own = FR.owned_dofs(c["t"])
    q0, q1 = c["q"], got["q"]
    ins_lo, ins_hi = own & (q0 >= lo), own & (q0 <= hi)
    assert (q1[ins_lo] >= np.broadcast_to(lo, q1.shape)[ins_lo]).all() and (q1[ins_hi] <= np.broadcast_to(hi, q1.shape)[ins_hi]).all(), what

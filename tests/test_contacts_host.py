"""Obstacle contacts on the host: the fp64 restatement of tests/contacts_reference.py against its own KKT conditions and against
working-set enumeration, the fp32 envelope that the GPU bounds are taken from, and the device routine of rmp2_contacts.h run on
the CPU through a small driver (also once under the host sanitizers).  No GPU.

The bounds (fixed here, before any GPU run; per robot, after one substep unless said otherwise; brackets in contacts_reference):
    stationarity  max_j |rnea64(q, qd, qdd_dev) - tau_applied - stop_dev - contact_dev|_j <= K_RES (1e-4 + 1e-5 s),
                  s = joint_stops' scale extended by max|contact_ref|
    velocity      max_j |v_dev - v_ref|_j <= K_VEL (dt (1e-4 + 1e-5 max|qdd_ref|) + 2^-23 max(|qd|, |v_ref|))
    force         max_j |(stop + contact)_dev - (stop + contact)_ref|_j <= K_FORCE (1e-4 + 1e-5 max(max|stop_ref|, max|contact_ref|,
                  max_j sum_k |M_jk| |qdd_ref_k|))
    the step      |q_dev - q_ref|, |qd_dev - qd_ref| <= K_STEP x forward_dynamics_reference.step_brackets
    gap           |(g+ + dt J v)_dev - (g+ + dt J v)_ref| (g+ = max(g, 0)) <= K_GAP (1e-6 + dt velocity bracket max(1, sum_j |J_j|)) per candidate
Each K is 4 x the worst ratio of the fp32 ENVELOPE restatement against the fp64 reference on the fleets of this file, rounded up
to one significant figure; MEASURED lists the envelope's worst ratios, test_envelope_backs_the_bounds measures them again.
(Velocity, force and step are wider than the stops' 1, 0.3 and 7: a contact's bound is b = -g / dt, which divides the gap's fp32
rounding -- 2^-24 of a position of the order of a metre -- by dt, and the rows of two contacts on neighbouring links are nearly
parallel, so the Gram matrix of the working set multiplies that by its condition number; the brackets have no such term.)
Hard invariants carry no K: joints inside their limits end inside, lambda >= 0, empty slots are 0 / -1.

The iteration cap of the device routine (rmp2_contacts.h kContactMaxIter) is twice the fp64 loop's worst count over these fleets
(WORST_ITERS, asserted below), the stress catalogue of tests/contacts_scene.py and the random trees' fleets included."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contacts_reference as CR
import dynamics_reference as DR
import forward_dynamics_reference as FR
import joint_stops_reference as JR
import test_forward_dynamics_host as H
from test_inverse_dynamics_host import reference_robots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "riemannian_motion_policies_amd", "csrc")

MEASURED = dict(res=0.0537, vel=10.29, force=4.018, step=16.0, gap=0.1174)     # the envelope's worst ratios
K_RES, K_VEL, K_FORCE, K_STEP, K_GAP = 0.3, 50.0, 20.0, 70.0, 0.5
WORST_ITERS = 17
DT = H.DT
D_ACT = 0.03      # >= dt x the fleets' largest approach speed (joint rates up to 1 rad / s: below 3 m / s at any point of a link)
STEP_SUBSTEPS = 4
N_BASE = dict(panda=6, two_joint=3)      # base states per fleet (the planar robot's disk is covered by more)


def robot_capsules(name):
    from riemannian_motion_policies_amd import urdf as U
    if name == "panda":
        return U.contact_capsules(U.PANDA_URDF, U.panda_table())
    return U.contact_capsules(U.TWO_JOINT_URDF, U.two_joint_table())


def _unit(v):
    return v / np.linalg.norm(v)


def _ancestors(t, f):
    out = []
    while f >= 0:
        out.append(f)
        f = int(t.parent[f])
    return out


def default_link_filter(t, f, depth):
    """(links the joints can carry well clear; not the fingers, which sit within d_act of the hand and would triple its pairs)"""
    return depth(f) >= min(3, t.n_dof) and t.joint_type[f] != 2


def movable_link_filter(t, f, depth):
    """Any capsule frame with a movable ancestor (the random trees: few frames, many of them prismatic)."""
    return depth(f) >= 1


def contact_fleet(rng, t, inert, g, caps, B, n_spheres=16, n_base=6, dt=DT, link_filter=default_link_filter, tries=1000):
    """(q, qd, qdd [B, n] fp32, spheres [n_spheres, 4] fp32) of a fleet whose table is shared: n_base base states inside the limits
    (every second one with two joints within reach of a limit), two or three spheres touching links of each (gap 0 .. 1 mm, on the
    side a joint motion carries the link to), robots = a base state + noise of 2 mrad with random qd, qdd; every fourth robot is
    a random state at least d_act + 0.05 m clear of every sphere.  The table is padded with spheres far away."""
    lo, hi = JR.table_limits(t)
    lo64, hi64 = np.maximum(lo.astype(np.float64), -3.0), np.minimum(hi.astype(np.float64), 3.0)
    n = t.n_dof
    depth = lambda f: bin(int(sum(1 << int(t.q_index[a]) for a in _ancestors(t, f) if t.joint_type[a] != 0 and t.q_index[a] >= 0))).count("1")
    frames = [f for f in CR.capsule_frames(caps) if link_filter(t, f, depth)]
    if not frames:
        raise AssertionError("no link to touch")
    base_q = lo64 + (hi64 - lo64) * rng.uniform(0.2, 0.8, (n_base, n))
    for b in range(1, n_base, 2):
        for j in rng.choice(n, 2, replace=False):
            base_q[b, j] = hi64[j] - 0.002 if rng.uniform() < 0.5 else lo64[j] + 0.002
    R, p, z = CR.poses(t, base_q)
    spheres = []
    probe = lo64 + (hi64 - lo64) * rng.uniform(0.0, 1.0, (300, n))
    for b in range(n_base):
        used = []                                        # (a base state's spheres touch different links)
        for s in range(3 if b % 2 == 0 else 2):
            if len(spheres) >= n_spheres:
                break
            for _ in range(tries):      # (a sphere that some link can never get clear of is proposed again)
                free = [f_ for f_ in frames if f_ not in used] or frames
                f = free[rng.integers(len(free))]
                A = R[f][b] @ caps[f, 0:3].astype(np.float64) + p[f][b]
                D = R[f][b] @ (caps[f, 4:7] - caps[f, 0:3]).astype(np.float64)
                X = A + rng.uniform(0.2, 0.8) * D
                # a direction the joints can carry X in, made orthogonal to the segment
                cols, gfr = [], f
                while gfr >= 0:
                    if t.joint_type[gfr] != 0 and t.q_index[gfr] >= 0:
                        cols.append(np.cross(z[gfr][b], X - p[gfr][b]) if t.joint_type[gfr] == 1 else z[gfr][b])
                    gfr = int(t.parent[gfr])
                d = np.array(cols).T @ rng.normal(size=len(cols))
                if D @ D > 0:
                    d = d - (d @ D) / (D @ D) * D
                d = _unit(d if np.linalg.norm(d) > 1e-9 else np.cross(D, [0.3, 0.5, 0.8]) + 1e-3)
                rk = rng.uniform(0.04, 0.1)
                c = X + d * (caps[f, 3] + rk + rng.uniform(0.0, 0.001))
                one = np.array([[c[0], c[1], c[2], rk]], np.float32)
                # (nor one that another base state is deep inside: the fleets' contacts are touches, not burials)
                if (CR.pair_rows(t, caps, one, probe)["gap"].min(1).max() > D_ACT + 0.1
                        and CR.pair_rows(t, caps, one, base_q)["gap"].min() > -1e-6):
                    break
            else:
                raise AssertionError("no sphere found")
            spheres.append([c[0], c[1], c[2], rk])
            used.append(f)
    k = 0
    while len(spheres) < n_spheres:
        spheres.append([10.0 + k, -7.0, 5.0, 0.05])
        k += 1
    spheres = np.array(spheres, np.float32)
    q, qd, qdd = H.fleet_states(rng, t, inert, g, B)
    qd = (0.5 * qd).astype(np.float32)          # (rates up to 1 rad / s: the contract d_act >= dt x approach speed holds)
    q = np.clip(q, lo, hi).astype(np.float32)
    clear = np.nonzero(np.arange(B) % 4 == 3)[0]
    found = np.zeros((0, n), np.float32)
    for _ in range(50):                              # (rejection sampling, a batch at a time)
        if len(found) >= len(clear):
            break
        cand = (lo64 + (hi64 - lo64) * rng.uniform(0.0, 1.0, (4 * len(clear) + 64, n))).astype(np.float32)
        ok = CR.pair_rows(t, caps, spheres, cand)["gap"].min(1) > D_ACT + 0.05
        found = np.concatenate([found, cand[ok]])
    else:
        raise AssertionError("no clear state found")
    q[clear] = found[:len(clear)]
    for r in range(B):
        if r % 4 != 3:
            q[r] = np.clip(base_q[(r // 4 + r) % n_base] + rng.normal(0.0, 0.002, n), lo, hi).astype(np.float32)
    q = np.clip(q, lo, hi)
    return q, qd, qdd, spheres


def fleet_inputs(t, inert, g, q, qd, qdd):
    tau_ref = DR.rnea(t, inert, q, qd, qdd, g)
    return [(FR.ACCEL, qdd, H.median_limits(tau_ref)), (FR.TORQUE, tau_ref.astype(np.float32), None)]


FLEETS = (("panda", 240), ("two_joint", 240))


def contact_cases(golden_dir, seed=500, fleets=FLEETS, n_spheres=16, n_base=None, substeps=1):
    rng = np.random.default_rng(seed)
    out = []
    sizes = dict(fleets)
    for name, t, inert in reference_robots(golden_dir):
        if name not in sizes:
            continue
        g = (0.0, 0.0, -9.81)
        caps = robot_capsules(name)
        q, qd, qdd, spheres = contact_fleet(rng, t, inert, g, caps, sizes[name], n_spheres, n_base or N_BASE[name])
        limits = JR.table_limits(t)
        for drive, u, lim in fleet_inputs(t, inert, g, q, qd, qdd):
            ref = CR.dynamics_step(t, inert, caps, spheres, D_ACT, q, qd, u, drive, DT, substeps, lim, limits, g)
            out.append(dict(name=name, t=t, inert=inert, g=g, caps=caps, spheres=spheres, q=q, qd=qd, u=u, drive=drive, lim=lim,
                            limits=limits, ref=ref, substeps=substeps))
    return out


@pytest.fixture(scope="module")
def cases(golden_dir):
    return contact_cases(golden_dir)


@pytest.fixture(scope="module")
def steps(golden_dir):
    return contact_cases(golden_dir, seed=502, fleets=(("panda", 64), ("two_joint", 64)), substeps=STEP_SUBSTEPS)


# The fleets of tests/test_gpu_contacts.py: (seed, robots, spheres in the table, base states, substeps).  One lane, one wave plus
# a lane, several waves; tables of 1, 16 and 33 spheres; 1 and 4 substeps.
GPU_FLEETS = ((510, 1, 1, 1, 1), (511, 65, 16, None, 1), (512, 1024, 33, None, 1), (513, 65, 16, None, STEP_SUBSTEPS))


def gpu_cases(golden_dir):
    out = []
    for seed, R, K, n_base, substeps in GPU_FLEETS:
        for c in contact_cases(golden_dir, seed=seed, fleets=(("panda", R), ("two_joint", R)), n_spheres=K, n_base=n_base, substeps=substeps):
            out.append(dict(c, R=R, K=K))
    return out


def linearised_gaps(c, got_qd, pair):
    """max(g, 0) + dt J v per slot [B, 8] in fp64 from the case's state, for the pairs `pair` [B, 8] (-1: nan) and the velocity
    got_qd: the linearised gap, counted from where the pair stands when it starts in penetration (it may not go deeper)."""
    pr = CR.pair_rows(c["t"], c["caps"], c["spheres"], c["q"])
    pos = {int(i): k for k, i in enumerate(pr["idx"])}
    out = np.full(pair.shape, np.nan)
    jn = np.zeros(pair.shape)
    for r in range(len(pair)):
        for s in range(pair.shape[1]):
            if pair[r, s] >= 0:
                k = pos[int(pair[r, s])]
                out[r, s] = max(pr["gap"][r, k], 0.0) + DT * (pr["J"][r, k] @ np.asarray(got_qd[r], np.float64))
                jn[r, s] = np.abs(pr["J"][r, k]).sum()
    return out, jn


def gap_bracket(c, jn):
    return 1e-6 + DT * JR.velocity_bracket(c["ref"], c["qd"], DT)[:, None] * np.maximum(1.0, jn)


def one_step_ratios(c, got):
    """(stationarity, velocity, force, gap) worst ratios of `got` = dict(q, qd, qdd, tau, stop, contact) against the case's
    one-substep reference."""
    t, inert, g, ref = c["t"], c["inert"], c["g"], c["ref"]
    res = CR.residual(t, inert, c["q"], c["qd"], got["qdd"], ref["tau"], got["stop"], got["contact"], g) / CR.residual_bracket(t, inert, c["q"], c["qd"], ref, g)
    vel = np.abs(got["qd"] - ref["qd"]).max(1) / CR.velocity_bracket(ref, c["qd"], DT)
    force = np.abs(got["stop"] + got["contact"] - ref["stop"] - ref["contact"]).max(1) / CR.force_bracket(ref)
    lg_ref, jn = linearised_gaps(c, ref["qd"], ref["pair"])
    lg_got, _ = linearised_gaps(c, got["qd"], ref["pair"])
    gap = np.nan_to_num(np.abs(lg_got - lg_ref) / gap_bracket(c, jn)).max(1)
    return res.max(), vel.max(), force.max(), gap.max()


def step_ratio(c, got):
    bq, bqd = CR.step_brackets(c["ref"], DT, c["substeps"])
    return max((np.abs(got["q"] - c["ref"]["q"]).max(1) / bq).max(), (np.abs(got["qd"] - c["ref"]["qd"]).max(1) / bqd).max())


def check_device_kkt(c, got, what, K_GAP=K_GAP, K_FORCE=K_FORCE):
    """The KKT conditions from the device's own contact_pair / contact_lambda with the rows rebuilt in fp64: lambda >= 0; lambda
    above the force bound only on a pair whose linearised gap is within the gap bound of 0; no candidate below minus that bound;
    empty slots 0 / -1; joints inside their limits end inside."""
    lam, pair = np.asarray(got["lam"], np.float64), np.asarray(got["pair"])
    assert (lam >= 0).all() and (lam[pair < 0] == 0).all(), what
    lg, jn = linearised_gaps(c, got["qd"], pair)
    br = K_GAP * gap_bracket(c, jn)
    assert not (lg < -br).any(), (what, np.nanmin(lg + br))
    # lambda_c |J_c|_1 is the scale at which the contact enters the joint torques: clear of zero by the force bound
    strong = (pair >= 0) & (lam * np.maximum(jn, 1e-300) > (K_FORCE * CR.force_bracket(c["ref"]))[:, None])
    assert (np.abs(lg[strong]) <= br[strong]).all(), what
    lo, hi = c["limits"]
    own = FR.owned_dofs(c["t"])
    q0, q1 = c["q"], got["q"]
    ins_lo, ins_hi = own & (q0 >= lo), own & (q0 <= hi)
    assert (q1[ins_lo] >= np.broadcast_to(lo, q1.shape)[ins_lo]).all() and (q1[ins_hi] <= np.broadcast_to(hi, q1.shape)[ins_hi]).all(), what
    return int(strong.sum())


def input_conditions(cases):
    cat = lambda k: np.concatenate([c["ref"][k] for c in cases])
    nc, ns, cand = cat("n_contact"), cat("n_stop"), cat("n_cand")
    return dict(active=float((nc >= 1).mean()), two=float((nc >= 2).mean()), both=float(((nc >= 1) & (ns >= 1)).mean()),
                none=float((cand == 0).mean()), capped=int(cat("capped").sum()), overflow=int(cat("overflow").sum()),
                iters=int(cat("iters").max()))


# ---- contacts on random trees -------------------------------------------------------------------------------------------------
# The N = 9 instantiation with fewer than 9 dofs (padded), 0, 1 and 2 save slots, contact rows with prismatic ancestor columns
# (n . z_j) and branches whose anc_mask zeroes stored dofs.  The bounds' K's are the trees' own, by the same rule: 4 x the
# envelope's worst ratio on these fleets (MEASURED_TREES), rounded up to one significant figure.
MEASURED_TREES = dict(res=0.0597, vel=31.79, force=10.33, step=28.25, gap=0.2875)     # the envelope's worst ratios on the trees
K_TREES = dict(res=0.3, vel=200.0, force=50.0, step=200.0, gap=2.0)
TREE_R = 65


def random_capsules(rng, t):
    """[n_frames, 8] float32: per frame no capsule (20 %), a sphere (20 %) or a capsule, radius 0.03 .. 0.06."""
    caps = np.zeros((t.n_frames, 8), np.float32)
    for f in range(t.n_frames):
        kind = rng.uniform()
        a = rng.uniform(-0.05, 0.05, 3)
        b = a + rng.uniform(-0.15, 0.15, 3)
        if kind >= 0.2:
            caps[f, 0:3], caps[f, 3], caps[f, 4:7] = a, rng.uniform(0.03, 0.06), (a if kind < 0.4 else b)
    return caps


def prismatic_ancestors(t, f):
    """The dofs of the prismatic joints on the path from frame f to the base (f's own joint included)."""
    return {int(t.q_index[a]) for a in _ancestors(t, f) if t.joint_type[a] == 2 and t.q_index[a] >= 0}


TREE_ATTEMPTS = 3      # capsule draws per tree before it is left out (most trees are too small to get clear of a sphere they touch)
_tree_fleets = {}


def tree_fleets(tmp_dir, R=TREE_R):
    """[(name, table, inertials, caps, q, qd, qdd, spheres)]: the random trees of test_forward_dynamics_host.random_robots(seed=0)
    with at most 9 dofs on which the fleet builder succeeds, with random capsules (seeded per tree and attempt)."""
    if R not in _tree_fleets:
        out = []
        for k, (name, t, inert) in enumerate(H.random_robots(tmp_dir, seed=0)):
            if t.n_dof > 9:
                continue
            for attempt in range(TREE_ATTEMPTS):
                rng = np.random.default_rng(700 + k + 100 * attempt)
                caps = random_capsules(rng, t)
                try:
                    fleet = contact_fleet(rng, t, inert, H.GRAVITY, caps, R, 16, 4, link_filter=movable_link_filter, tries=60)
                except AssertionError:
                    continue
                out.append((name, t, inert, caps, *fleet))
                break
        _tree_fleets[R] = out
    return _tree_fleets[R]


_tree_cases = {}


def tree_cases(tmp_dir, substeps=1, R=TREE_R):
    """contact_cases on tree_fleets, the trees' gravity, both drives per tree; beside the usual fields `slots`, `prismatic` (how
    many prismatic dofs the contact links have among their ancestors) and `prismatic_row` (the most of them in one row)."""
    if (substeps, R) in _tree_cases:
        return _tree_cases[(substeps, R)]
    out = []
    for name, t, inert, caps, q, qd, qdd, spheres in tree_fleets(tmp_dir, R):
        limits = JR.table_limits(t)
        pris = [prismatic_ancestors(t, f) for f in CR.capsule_frames(caps)]
        for drive, u, lim in fleet_inputs(t, inert, H.GRAVITY, q, qd, qdd):
            ref = CR.dynamics_step(t, inert, caps, spheres, D_ACT, q, qd, u, drive, DT, substeps, lim, limits, H.GRAVITY)
            out.append(dict(name=name, t=t, inert=inert, g=H.GRAVITY, caps=caps, spheres=spheres, q=q, qd=qd, u=u, drive=drive, lim=lim,
                            limits=limits, ref=ref, substeps=substeps, R=R, K=len(spheres), slots=int(t.depth_first_schedule()[3]),
                            prismatic=len(set().union(*pris)), prismatic_row=max(len(p) for p in pris)))
    _tree_cases[(substeps, R)] = out
    return out


# ---- 1: the reference ----------------------------------------------------------------------------------------------------------

def test_fleets_meet_the_input_conditions_and_the_iteration_cap(cases, steps, golden_dir, tmp_path_factory):
    cond = input_conditions(cases)
    print(cond)
    assert cond["active"] >= 0.30 and cond["two"] >= 0.05 and cond["both"] >= 0.05 and cond["none"] >= 0.20, cond
    assert cond["capped"] == 0 and cond["overflow"] == 0, cond
    gpu = gpu_cases(golden_dir)
    worst = max(cond["iters"], input_conditions(steps)["iters"], input_conditions(gpu)["iters"])
    assert not any(c["ref"]["capped"].any() or c["ref"]["overflow"].any() for c in steps + gpu)
    assert worst == 7, worst                                      # (the touching fleets alone, as before the catalogue)
    import contacts_scene as CS                                  # (it imports this module)
    stress = CS.catalogue(golden_dir)
    assert not any(c["ref"]["capped"].any() for c in stress)
    tmp = tmp_path_factory.mktemp("trees")
    trees = tree_cases(tmp) + tree_cases(tmp, substeps=STEP_SUBSTEPS)
    assert not any(c["ref"]["capped"].any() for c in trees)
    steps4 = [c["ref_step"] for c in CS.with_steps(stress)]
    assert not any(r["capped"].any() for r in steps4)
    worst = max(worst, input_conditions(stress)["iters"], input_conditions(trees)["iters"], max(int(r["iters"].max()) for r in steps4))
    assert worst == WORST_ITERS, worst
    src = open(os.path.join(CSRC, "rmp2_contacts.h")).read()
    assert int(re.search(r"#define RMP2_CONTACT_MAX_ITER (\d+)\n", src).group(1)) == 2 * WORST_ITERS
    assert "constexpr int kContactMaxIter = RMP2_CONTACT_MAX_ITER;" in src


def _robot_problem(c, r):
    """(M, vstar, l, h, J, b) of robot r of a case, fp64."""
    ref = c["ref"]
    own = FR.owned_dofs(c["t"])
    l, h = JR.velocity_box(c["q"][r].astype(np.float64), DT, c["limits"][0], c["limits"][1], own)
    k = int(ref["n_cand"][r])
    return ref["M"][r], ref["vstar"][r], l, h, ref["J"][r, :k], -np.maximum(ref["gap"][r, :k], 0.0) / DT


def test_reference_meets_its_own_kkt_conditions(cases):
    worst = 0.0
    for c in cases:
        for r in np.nonzero(c["ref"]["n_cand"] > 0)[0]:
            M, vs, l, h, J, b = _robot_problem(c, r)
            s = CR.solve_qp(M, vs, l, h, J, b)
            assert not s["capped"]
            worst = max(worst, CR.kkt_residual(M, vs, l, h, J, b, s))
    print("worst KKT residual", worst)
    assert worst <= 1e-9


def test_reference_equals_working_set_enumeration(cases):
    rng = np.random.default_rng(7)
    worst, seen = 0.0, 0
    for c in cases:
        if c["name"] != "two_joint":
            continue
        for r in np.nonzero(c["ref"]["n_cand"] > 0)[0][:60]:
            M, vs, l, h, J, b = _robot_problem(c, r)
            v = CR.brute_force(M, vs, l, h, J, b)
            worst = max(worst, np.abs(v - c["ref"]["qd"][r]).max() / max(np.abs(vs).max(), 1e-12))
            seen += 1
    for _ in range(200):      # random SPD problems, <= 3 contact rows, n <= 3
        n, nc = int(rng.integers(1, 4)), int(rng.integers(0, 4))
        A = rng.normal(size=(n, n))
        M = A @ A.T + 0.1 * np.eye(n)
        vs = rng.normal(size=n) * 2
        l, h = -np.abs(rng.normal(size=n)) * (rng.uniform(size=n) < 0.8), np.abs(rng.normal(size=n)) * (rng.uniform(size=n) < 0.8)
        l[rng.uniform(size=n) < 0.2] = -np.inf
        h[rng.uniform(size=n) < 0.2] = np.inf
        J, b = rng.normal(size=(nc, n)), -np.abs(rng.normal(size=nc)) * (rng.uniform(size=nc) < 0.7)
        s = CR.solve_qp(M, vs, l, h, J, b)
        v = CR.brute_force(M, vs, l, h, J, b)
        assert not s["capped"]
        worst = max(worst, np.abs(v - s["v"]).max() / max(np.abs(vs).max(), 1e-12))
        seen += 1
    print("worst difference to enumeration", worst, "over", seen)
    assert seen >= 250 and worst <= 1e-9


# ---- 2: the envelope -----------------------------------------------------------------------------------------------------------

def envelope_ratios(cases, steps):
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0, gap=0.0)
    for c in cases:
        e = CR.substep(c["t"], c["inert"], c["caps"], c["spheres"], D_ACT, c["q"], c["qd"], c["u"], c["drive"], DT, c["lim"], c["limits"], c["g"], envelope=True)
        e = {k: np.asarray(e[k], np.float64) for k in ("q", "qd", "qdd", "tau", "stop", "contact")}
        for k, v in zip(("res", "vel", "force", "gap"), one_step_ratios(c, e)):
            worst[k] = max(worst[k], float(v))
    for c in steps:
        e = CR.dynamics_step(c["t"], c["inert"], c["caps"], c["spheres"], D_ACT, c["q"], c["qd"], c["u"], c["drive"], DT, c["substeps"], c["lim"], c["limits"], c["g"], envelope=True)
        worst["step"] = max(worst["step"], float(step_ratio(c, e)))
    return worst


def _round_up_1sf(x):
    e = 10.0 ** np.floor(np.log10(x))
    return float(np.ceil(x / e - 1e-9) * e)


def test_envelope_backs_the_bounds(cases, steps):
    worst = envelope_ratios(cases, steps)
    print("envelope worst ratios", worst)
    for k, K in (("res", K_RES), ("vel", K_VEL), ("force", K_FORCE), ("step", K_STEP), ("gap", K_GAP)):
        assert np.isclose(K, _round_up_1sf(4 * MEASURED[k])), (k, K, MEASURED[k])
        assert 4 * worst[k] <= K, (k, worst[k], K)


# ---- 3: the device routine on the CPU ------------------------------------------------------------------------------------------

def _build(tmp_path_factory, source, name, extra=()):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("driver") / name)
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", *extra, "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", source)], check=True, timeout=900)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver")


@pytest.fixture(scope="module")
def stops_driver(tmp_path_factory):
    return _build(tmp_path_factory, "joint_stops_driver.cpp", "joint_stops_driver")


@pytest.fixture(scope="module")
def plain_driver(tmp_path_factory):
    return _build(tmp_path_factory, "forward_dynamics_driver.cpp", "forward_dynamics_driver")


def run_driver(exe, tmp_path, c, substeps=1, spheres=None, limits="case", d_act=D_ACT, q=None, qd=None, u=None, caps=None,
               lists=None, planes=None):
    """The device routine on the CPU on a case (fields replaced by the keywords): contacts_reference.read_driver_output's dict.
    lists = (csr_offset, csr_index): the list form, spheres being the pool; planes = [P, 4] (P = 0 too): the plane form.  The one
    runner of the contact host tests.  A sanitizer report fails it: the exit status must be 0 and nothing may be written to
    stderr."""
    q, qd, u = (c[k] if x is None else x for k, x in (("q", q), ("qd", qd), ("u", u)))
    CR.write_driver_input(str(tmp_path / "in.bin"), c["t"], c["inert"], c["caps"] if caps is None else caps,
                          c["spheres"] if spheres is None else spheres, d_act, q, qd, u, c["drive"], c["lim"],
                          c["limits"] if limits == "case" else limits, DT, substeps, c["g"], lists=lists, planes=planes)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "contacts"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    return CR.read_driver_output(str(tmp_path / "out.bin"), len(q), c["t"].n_dof)


def flags_agree(c, status, K_FORCE=K_FORCE):
    """The device's flags against the reference's, where the reference is clear of the decision: a robot whose reference has a
    contact force above the force bound has RMP2_CONTACT_ACTIVE; one without a candidate in any substep has neither it nor
    overflow; nothing is capped or overflowed."""
    ref = c["ref"]
    assert not (status & (CR.CAPPED | CR.OVERFLOW)).any()
    clear = np.abs(ref["contact"]).max(1) > K_FORCE * CR.force_bracket(ref)
    assert ((status[clear] & CR.CONTACT_ACTIVE) != 0).all()
    assert ((status[~ref["any_cand"]] & CR.CONTACT_ACTIVE) == 0).all()
    assert ((status >> 8) <= 2 * WORST_ITERS).all()


def test_device_routine_on_the_cpu_within_half_of_each_bound(driver, cases, steps, tmp_path):
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0, gap=0.0)
    strong = 0
    for c in cases:
        d = run_driver(driver, tmp_path, c)
        for k, v in zip(("res", "vel", "force", "gap"), one_step_ratios(c, d)):
            worst[k] = max(worst[k], float(v))
        strong += check_device_kkt(c, d, c["name"])
        flags_agree(c, d["status"])
    for c in steps:
        d = run_driver(driver, tmp_path, c, substeps=c["substeps"])
        worst["step"] = max(worst["step"], float(step_ratio(c, d)))
        flags_agree(c, d["status"])
    print("CPU driver worst ratios", worst, "strong contacts", strong)
    assert strong >= 100
    for k, K in (("res", K_RES), ("vel", K_VEL), ("force", K_FORCE), ("step", K_STEP), ("gap", K_GAP)):
        assert worst[k] <= 0.5 * K, (k, worst[k], K)


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_device_fast_path_bit_for_bit(driver, stops_driver, plain_driver, cases, tmp_path):
    """Table far away: the stops' results; limits far too, or absent: the plain step's; in the mixed fleet the clear robots."""
    import test_joint_stops_host as SH
    far = np.array([[30.0, 20.0, 10.0, 0.1], [-30.0, 5.0, 2.0, 0.2]], np.float32)
    for c in cases:
        n = c["t"].n_dof
        for sub in (1, 3):
            s = SH.run_driver(stops_driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"], sub, c["g"])
            for table in (far, np.zeros((0, 4), np.float32)):
                d = run_driver(driver, tmp_path, c, substeps=sub, spheres=table)
                for k in ("q", "qd", "qdd", "tau", "stop"):
                    assert _bits_equal(d[k], s[k]), (c["name"], k)
                assert (d["status"] == s["status"]).all() and (d["contact"] == 0).all() and (d["lam"] == 0).all() and (d["pair"] == -1).all()
            wide = (np.full(n, -1e6, np.float32), np.full(n, 1e6, np.float32))
            H.FR.write_driver_input(str(tmp_path / "p.bin"), c["t"], c["inert"], c["q"], c["qd"], c["u"], 2, drive=c["drive"], lim=c["lim"], dt=DT, substeps=sub, gravity=c["g"])
            subprocess.run([plain_driver, str(tmp_path / "p.bin"), str(tmp_path / "po.bin")], check=True, timeout=300)
            plain = np.fromfile(tmp_path / "po.bin", np.float32)[:4 * len(c["q"]) * n].reshape(4, len(c["q"]), n)
            for lim_ in (wide, None):
                d = run_driver(driver, tmp_path, c, substeps=sub, spheres=far, limits=lim_)
                for i, k in enumerate(("q", "qd", "qdd", "tau")):
                    assert _bits_equal(d[k], plain[i]), (c["name"], k)
                assert (d["status"] == 0).all() and (d["stop"] == 0).all()
        # the mixed fleet: robots without a candidate equal the stops' step
        d = run_driver(driver, tmp_path, c)
        s = SH.run_driver(stops_driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"], 1, c["g"])
        clear = c["ref"]["n_cand"] == 0
        assert clear.sum() >= 0.2 * len(clear)
        for k in ("q", "qd", "qdd", "tau", "stop"):
            assert _bits_equal(d[k][clear], s[k][clear]), (c["name"], k)
        assert (d["pair"][clear] == -1).all() and (d["lam"][clear] == 0).all() and (d["contact"][clear] == 0).all()


def _panda(cases, drive=FR.ACCEL):
    return next(c for c in cases if c["name"] == "panda" and c["drive"] == drive)


def _two(cases, drive=FR.TORQUE):
    return next(c for c in cases if c["name"] == "two_joint" and c["drive"] == drive)


def test_device_overflow_keeps_the_eight_smallest_gaps(driver, cases, tmp_path):
    c = _panda(cases)
    r = int(np.nonzero(c["ref"]["n_contact"] >= 1)[0][0])
    k = int(c["ref"]["pair"][r, 0]) % len(c["spheres"])
    base = c["spheres"][k]
    table = np.tile(base, (12, 1)).astype(np.float32)
    table[:, 3] = base[3] - 0.001 * np.arange(12)          # twelve gaps 1 mm apart, all within d_act
    table[5, 3] = table[4, 3]                              # and one tie
    sel = slice(r, r + 1)
    ref = CR.substep(c["t"], c["inert"], c["caps"], table, D_ACT, c["q"][sel], c["qd"][sel], c["u"][sel], c["drive"], DT, c["lim"], c["limits"], c["g"])
    d = run_driver(driver, tmp_path, c, spheres=table, q=c["q"][sel], qd=c["qd"][sel], u=c["u"][sel])
    assert ref["overflow"][0] and d["status"][0] & CR.OVERFLOW
    assert sorted(d["pair"][0]) == sorted(ref["pair"][0]) and (d["pair"][0] >= 0).all()
    assert np.isfinite(d["qd"]).all()
    c1 = dict(c, q=c["q"][sel], qd=c["qd"][sel], spheres=table, ref=ref)
    check_device_kkt(c1, d, "overflow")
    assert np.abs(d["qd"] - ref["qd"]).max() <= K_VEL * CR.velocity_bracket(ref, c["qd"][sel], DT).max()


def test_device_two_coincident_spheres(driver, cases, tmp_path):
    """Two spheres on one spot: two identical rows.  The velocity is that of the one sphere; the force may be shared."""
    for c in (_panda(cases), _two(cases)):
        rs = np.nonzero((c["ref"]["n_contact"] >= 1) & (c["ref"]["n_cand"] <= 3))[0][:8]
        for r in rs:
            sel = slice(r, r + 1)
            k = int(c["ref"]["pair"][r, int(np.argmax(c["ref"]["lam"][r]))]) % len(c["spheres"])
            one = c["spheres"][k:k + 1]
            two = np.concatenate([one, one])
            d1 = run_driver(driver, tmp_path, c, spheres=one, q=c["q"][sel], qd=c["qd"][sel], u=c["u"][sel])
            d2 = run_driver(driver, tmp_path, c, spheres=two, q=c["q"][sel], qd=c["qd"][sel], u=c["u"][sel])
            ref = CR.substep(c["t"], c["inert"], c["caps"], one, D_ACT, c["q"][sel], c["qd"][sel], c["u"][sel], c["drive"], DT, c["lim"], c["limits"], c["g"])
            assert all(np.isfinite(d2[k_]).all() for k_ in ("q", "qd", "qdd", "stop", "contact", "lam"))
            assert not (d2["status"][0] & CR.CAPPED)
            bv = K_VEL * CR.velocity_bracket(ref, c["qd"][sel], DT).max()
            assert np.abs(d2["qd"] - ref["qd"]).max() <= bv and np.abs(d1["qd"] - ref["qd"]).max() <= bv
            assert np.abs(d2["contact"] - ref["contact"]).max() <= K_FORCE * CR.force_bracket(ref).max()


def test_device_more_active_rows_than_dofs(driver, cases, tmp_path):
    """The two-joint robot's end sphere pressed into a pocket of four spheres: more rows want to be active than there are dofs.
    The result is finite and feasible (no row violated beyond the gap bound), equal to the reference's velocity, and the
    working set never exceeds the dofs; RMP2_STOP_CAPPED may be set only if a row was refused."""
    c = _two(cases)
    t, caps = c["t"], c["caps"]
    q = np.array([[0.4, -0.9]], np.float32)
    R, p, z = CR.poses(t, q)
    tip = p[2][0]
    rk = 0.05
    dirs = [np.array([np.cos(a), np.sin(a), 0.0]) for a in (0.3, 1.4, 2.6, 3.9, 5.1)]
    table = np.array([[*(tip + d * (caps[2, 3] + rk + 1e-4)), rk] for d in dirs], np.float32)
    for qd0 in ([2.0, -1.5], [-2.0, 2.0], [0.5, 3.0], [-3.0, -3.0]):
        qd = np.array([qd0], np.float32)
        u = np.zeros((1, 2), np.float32)
        ref = CR.substep(t, c["inert"], caps, table, D_ACT, q, qd, u, FR.TORQUE, DT, None, c["limits"], c["g"])
        d = run_driver(driver, tmp_path, dict(c, lim=None, drive=FR.TORQUE), spheres=table, q=q, qd=qd, u=u)
        assert ref["n_cand"][0] >= 4 and not ref["capped"][0]
        assert all(np.isfinite(d[k]).all() for k in ("q", "qd", "qdd", "stop", "contact", "lam"))
        c1 = dict(c, q=q, qd=qd, spheres=table, ref=ref, lim=None)
        check_device_kkt(c1, d, "pocket")
        assert np.abs(d["qd"] - ref["qd"]).max() <= K_VEL * CR.velocity_bracket(ref, qd, DT).max()
        assert (d["lam"][0] > 0).sum() <= 2


def test_device_penetrating_start_is_not_pushed_out_and_goes_no_deeper(driver, cases, tmp_path):
    for c in (_panda(cases), _two(cases)):
        r = int(np.nonzero(c["ref"]["n_contact"] >= 1)[0][0])
        sel = slice(r, r + 1)
        k = int(c["ref"]["pair"][r, int(np.argmax(c["ref"]["lam"][r]))])
        table = c["spheres"][k % len(c["spheres"]):k % len(c["spheres"]) + 1].copy()
        table[0, 3] += 0.02                                             # 2 cm into the link
        for sign in (1.0, -1.0):
            qd = (sign * c["qd"][sel]).astype(np.float32)
            ref = CR.substep(c["t"], c["inert"], c["caps"], table, D_ACT, c["q"][sel], qd, c["u"][sel], c["drive"], DT, c["lim"], c["limits"], c["g"])
            d = run_driver(driver, tmp_path, c, spheres=table, q=c["q"][sel], qd=qd, u=c["u"][sel])
            assert ref["gap"][0, 0] < -0.015
            J = ref["J"][0, 0]
            rate = J @ d["qd"][0].astype(np.float64)
            bound = K_VEL * CR.velocity_bracket(ref, qd, DT)[0] * max(1.0, np.abs(J).sum())
            assert rate >= -bound                                       # no deeper
            assert abs(rate - J @ ref["qd"][0]) <= bound                # and not pushed out: the reference's own rate
            if ref["n_contact"][0]:
                assert abs(J @ ref["qd"][0]) <= 1e-9


def test_device_sphere_centred_on_a_link_axis(driver, cases, tmp_path):
    """The crossing convention: n = +z, gap = -(r_k + r_f)."""
    c = _panda(cases)
    sel = slice(0, 1)
    f = 3
    R, p, z = CR.poses(c["t"], c["q"][sel].astype(np.float32).astype(np.float64))
    pr0 = CR.pair_rows(c["t"], c["caps"], np.array([[0, 0, 0, 0.05]], np.float32), c["q"][sel], np.float32)
    # the fp32 centre of the segment's start: exactly on the axis in the device's arithmetic needs its own value; use t = 0
    R32, p32, _ = CR.poses(c["t"], c["q"][sel], np.float32)
    A32 = FR._mv(R32[f], c["caps"][f, 0:3][None].astype(np.float32)) + p32[f]
    table = np.array([[*A32[0], 0.05]], np.float32)
    ref = CR.substep(c["t"], c["inert"], c["caps"], table, D_ACT, c["q"][sel], c["qd"][sel], c["u"][sel], c["drive"], DT, c["lim"], c["limits"], c["g"], envelope=True)
    d = run_driver(driver, tmp_path, c, spheres=table, q=c["q"][sel], qd=c["qd"][sel], u=c["u"][sel])
    assert all(np.isfinite(d[k]).all() for k in ("q", "qd", "qdd", "stop", "contact", "lam"))
    assert f * 1 + 0 in d["pair"][0]
    # the +z row: J v >= 0 along +z at the point
    pr = CR.pair_rows(c["t"], c["caps"], table, c["q"][sel])
    k = list(pr["idx"]).index(f)
    Jz = np.zeros(c["t"].n_dof)
    g_ = f
    while g_ >= 0:
        if c["t"].joint_type[g_] == 1 and c["t"].q_index[g_] >= 0:
            Jz[int(c["t"].q_index[g_])] = np.cross(z[g_][0], pr["X"][0, k] - p[g_][0])[2]
        g_ = int(c["t"].parent[g_])
    assert Jz @ d["qd"][0].astype(np.float64) >= -K_VEL * CR.velocity_bracket(ref, c["qd"][sel], DT)[0] * max(1.0, np.abs(Jz).sum())


def test_device_non_finite_rows_and_tables(driver, cases, tmp_path):
    c = _panda(cases)
    q, qd, u = c["q"][:8].copy(), c["qd"][:8].copy(), c["u"][:8].copy()
    good = run_driver(driver, tmp_path, c, q=q, qd=qd, u=u)
    q[2, 1], qd[5, 0] = np.nan, np.inf
    d = run_driver(driver, tmp_path, c, q=q, qd=qd, u=u)
    bad = np.array([False, False, True, False, False, True, False, False])
    for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
        assert np.isnan(d[k][bad]).all() and _bits_equal(d[k][~bad], good[k][~bad]), k
    assert (d["pair"][bad] == -1).all() and np.array_equal(d["pair"][~bad], good["pair"][~bad])
    table = c["spheres"].copy()
    table[3, 1] = np.nan
    d = run_driver(driver, tmp_path, c, spheres=table, q=c["q"][:8], qd=c["qd"][:8], u=c["u"][:8])
    for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
        assert np.isnan(d[k]).all(), k


def test_driver_runs_clean_under_the_host_sanitizers(tmp_path_factory, cases, tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined on the host, run once on a mixed fleet."""
    exe = _build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_san",
                 ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"))
    c = _panda(cases)
    plain = run_driver(exe, tmp_path, c, substeps=2)
    assert np.isfinite(plain["qd"]).all()


# ---- 4: random trees ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trees")
    return tree_cases(tmp), tree_cases(tmp, substeps=STEP_SUBSTEPS)


def test_default_link_filter_keeps_the_existing_fleets_bytes(golden_dir):
    import hashlib
    c = contact_cases(golden_dir, seed=511, fleets=(("panda", 65),), n_spheres=16)[0]
    h = hashlib.sha256()
    for k in ("q", "qd", "u", "spheres"):
        h.update(np.ascontiguousarray(c[k]).tobytes())
    assert h.hexdigest() == "f8387f1c7479e37b32aa1be8dab8fa344f217c58a20f3e36bfa3c424521e8207"      # (taken before the parameter existed)


def tree_cover(one):
    """What the trees' fleets are for, asserted on the fleets and not on the trees' names."""
    dofs, slots = {c["t"].n_dof for c in one}, {c["slots"] for c in one}
    assert len({c["name"] for c in one}) >= 4
    assert 9 in dofs and any(3 <= n <= 8 for n in dofs) and {0, 1, 2} <= slots, (dofs, slots)
    assert max(c["prismatic"] for c in one) >= 3 and max(c["prismatic_row"] for c in one) >= 2
    for c in one:
        cond = input_conditions([c])
        assert cond["active"] >= 0.30 and cond["none"] >= 0.20 and cond["capped"] == 0 and cond["overflow"] == 0, (c["name"], cond)


def test_tree_fleets_cover_padded_dofs_slots_and_prismatic_columns(trees):
    tree_cover(trees[0])
    rows = 0      # contact rows with a prismatic column, and rows whose link's anc_mask leaves out a dof of the tree
    for c in trees[0]:
        J, k = c["ref"]["J"], c["ref"]["n_cand"]
        pris = sorted(set().union(*[prismatic_ancestors(c["t"], f) for f in CR.capsule_frames(c["caps"])]))
        rows += sum(int((J[r, :k[r]][:, pris] != 0).any(1).sum()) for r in range(len(k))) if pris else 0
    assert rows >= 100


def test_envelope_backs_the_tree_bounds(trees):
    worst = envelope_ratios(*trees)
    print("envelope worst ratios on the trees", worst)
    for k, K in K_TREES.items():
        assert np.isclose(K, _round_up_1sf(4 * MEASURED_TREES[k])), (k, K, MEASURED_TREES[k])
        assert np.isclose(worst[k], MEASURED_TREES[k], rtol=1e-3), (k, worst[k], MEASURED_TREES[k])


def test_device_routine_on_the_cpu_on_trees_within_half_of_each_tree_bound(driver, stops_driver, trees, tmp_path):
    import test_joint_stops_host as SH
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0, gap=0.0)
    strong = 0
    for c in trees[0]:
        d = run_driver(driver, tmp_path, c)
        for k, v in zip(("res", "vel", "force", "gap"), one_step_ratios(c, d)):
            worst[k] = max(worst[k], float(v))
        strong += check_device_kkt(c, d, c["name"], K_TREES["gap"], K_TREES["force"])
        flags_agree(c, d["status"], K_TREES["force"])
        s = SH.run_driver(stops_driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"], 1, c["g"])
        clear = c["ref"]["n_cand"] == 0
        assert clear.sum() >= 0.2 * len(clear)
        for k in ("q", "qd", "qdd", "tau", "stop"):
            assert _bits_equal(d[k][clear], s[k][clear]), (c["name"], k)
    for c in trees[1]:
        d = run_driver(driver, tmp_path, c, substeps=c["substeps"])
        worst["step"] = max(worst["step"], float(step_ratio(c, d)))
        flags_agree(c, d["status"], K_TREES["force"])
    print("CPU driver worst ratios on the trees", worst, "strong contacts", strong)
    assert strong >= 100
    for k, K in K_TREES.items():
        assert worst[k] <= 0.5 * K, (k, worst[k], K)


def test_contact_capsules_are_the_self_collision_rows_without_the_base():
    from riemannian_motion_policies_amd import urdf as U
    t = U.panda_table()
    caps = U.contact_capsules(U.PANDA_URDF, t)
    assert caps.shape == (t.n_frames, 8) and caps.dtype == np.float32
    assert np.array_equal(caps, U.self_collision_capsules(U.PANDA_URDF, t)[:t.n_frames])


def test_symbols_declared_bound_and_null_handle_refused(hip_lib):
    import ctypes as C
    lib = C.CDLL(hip_lib)
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    for sym in ("rmp2_set_contact_capsules", "rmp2_dynamics_step_contacts"):
        assert re.search(r"\bint " + sym + r"\(", hdr) and hasattr(lib, sym)
    assert "#define RMP2_CONTACT_ACTIVE 4u" in hdr and "#define RMP2_CONTACT_OVERFLOW 8u" in hdr and "#define RMP2_MAX_CONTACTS 8" in hdr
    assert re.search(r"#define RMP2_ABI_VERSION (\d+)", hdr).group(1) == "5"
    lib.rmp2_set_contact_capsules.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    assert lib.rmp2_set_contact_capsules(None, 0, None) == -1

"""Joint-limit stops on the host: the fp64 restatement of tests/joint_stops_reference.py against its own KKT conditions and
against brute-force enumeration, the fp32 envelope that the GPU bounds are taken from, the device routine of rmp2_joint_stops.h
run on the CPU through a small driver, urdf.read_joint_limits and the new C symbol.  No GPU.

The bounds (fixed here, before any GPU run; per robot, after one substep unless said otherwise):
    stationarity  max_j |rnea64(q, qd, qdd_dev) - tau_applied - stop_dev|_j <= K_RES2 (1e-4 + 1e-5 s),
                  s = max(max|tau_applied|, max|bias|, max_j sum_k |M_jk| |qdd_ref_k|, max|stop_ref|)
    velocity      max_j |v_dev - v_ref|_j <= K_VEL (dt (1e-4 + 1e-5 max|qdd_ref|) + 2^-23 max(|qd|, |v_ref|))
    stop torque   max_j |stop_dev - stop_ref|_j <= K_STOP (1e-4 + 1e-5 max(max|stop_ref|, max_j sum_k |M_jk| |qdd_ref_k|))
                  (velocity and stop torque on the Panda and the two-joint robot only, as K_QDD: the trees' cond(M) reaches 1e4)
    the step      |q_dev - q_ref|, |qd_dev - qd_ref| <= K_STEP2 x forward_dynamics_reference.step_brackets
Each K is 4 x the worst ratio of the fp32 ENVELOPE restatement against the fp64 reference on the fleets of this file, rounded up
to one significant figure.  Measured worst envelope ratios:
stationarity 0.215, velocity 0.229, stop torque 0.0594, step 1.709
(so K_RES2 = 0.9, K_VEL = 1, K_STOP = 0.3, K_STEP2 = 7; the step's is larger than the plain step's 0.446 because a dof on a stop has
v = (limit - q) / dt, which divides the rounding of q, 2^-24 |q|, by dt: the bracket has no such term).
test_envelope_backs_the_bounds measures them again.  Hard invariants carry no K: a joint that starts inside its limits ends
inside, one that starts outside does not move further out, a locked joint keeps its q, and stop_out has the multiplier's sign
wherever the reference has the stop strictly active (|stop_ref| above the stop-torque bound).

The iteration cap of the device routine (rmp2_joint_stops.h kStopMaxIter) is twice the fp64 loop's worst count over these
fleets (WORST_ITERS, asserted below)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import dynamics_reference as DR
import forward_dynamics_reference as FR
import joint_stops_reference as JR
import test_forward_dynamics_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "riemannian_motion_policies_amd", "csrc")

K_RES2, K_VEL, K_STOP, K_STEP2 = 0.9, 1.0, 0.3, 7.0
WORST_ITERS = 5
DT = H.DT
STEP_SUBSTEPS = 3


def stop_fleet(rng, t, inert, g, B, dt=DT):
    """(q, qd, qdd) [B, n] fp32 of H.fleet_states with q inside the table's limits.  Of every four robots two have every joint,
    with probability 1/3, put within |qd| dt of the limit it moves towards, one has a single such joint, and one is kept clear
    of its limits (its rates scaled so that no joint comes within reach of one): the fast path."""
    q, qd, qdd = H.fleet_states(rng, t, inert, g, B)
    lo, hi = JR.table_limits(t)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    clear = (np.arange(B) % 4 == 0)[:, None]
    single = (np.arange(B) % 4 == 1)[:, None] & (np.arange(q.shape[1]) == rng.integers(0, q.shape[1], B)[:, None])
    near = np.where((np.arange(B) % 4 == 1)[:, None], single, (rng.uniform(size=q.shape) < 1.0 / 3.0) & ~clear)
    r = rng.uniform(0.0, 0.9, q.shape)
    reach = r * np.abs(qd) * dt
    target = np.where(qd > 0, hi64 - reach, lo64 + reach)
    q = np.where(near & np.isfinite(target), target, q)
    q = np.clip(q, lo64, hi64).astype(np.float32)
    q = np.clip(q, lo, hi)                                             # (after the rounding as well)
    with np.errstate(invalid="ignore"):
        room = np.minimum(np.where(np.isfinite(hi), hi - q, np.inf), np.where(np.isfinite(lo), q - lo, np.inf))
    calm = np.minimum(1.0, 0.05 * room / (np.abs(qd) * dt + 1e-30)).min(1, keepdims=True)
    qd = np.where(clear, qd * calm, qd).astype(np.float32)
    return q, qd, qdd


def fleet_inputs(t, inert, g, q, qd, qdd):
    """[(drive, u, tau_limit)]: the acceleration drive against the fleet's median torques, and the torque drive without."""
    tau_ref = DR.rnea(t, inert, q, qd, qdd, g)
    return [(FR.ACCEL, qdd, H.median_limits(tau_ref)), (FR.TORQUE, tau_ref.astype(np.float32), None)]


def stop_cases(robots, seed=300, scale=5, only=None):
    """Per robot and drive: the fleet (B / scale states of H.all_robots' count), its limits and the fp64 substep."""
    rng = np.random.default_rng(seed)
    out = []
    for name, t, inert, g, B in robots:
        q, qd, qdd = stop_fleet(rng, t, inert, g, max(B // scale, 64))
        if only is not None and name not in only:
            continue
        limits = JR.table_limits(t)
        for drive, u, lim in fleet_inputs(t, inert, g, q, qd, qdd):
            ref = JR.substep(t, inert, q, qd, u, drive, DT, lim, limits, g)
            out.append(dict(name=name, t=t, inert=inert, g=g, q=q, qd=qd, u=u, drive=drive, lim=lim, limits=limits, ref=ref))
    return out


GPU_FLEETS = (("panda", 65), ("two_joint", 256), ("tree0.urdf", 65), ("dof16.urdf", 65))


def effort_limits(name, t):
    """tau_limit of the GPU fleets: the URDF's <limit effort=> (tests/dynamics_reference.py random_urdf writes effort="1")."""
    from riemannian_motion_policies_amd import urdf as U
    if name == "panda":
        return U.read_effort_limits(U.PANDA_URDF, U.PANDA_ORDER)
    if name == "two_joint":
        return U.read_effort_limits(U.TWO_JOINT_URDF, U.TWO_JOINT_ORDER)
    return np.ones(t.n_dof, np.float32)


def gpu_cases(robots, seed=310):
    """The fleets of tests/test_gpu_joint_stops.py's first test: both drives against the URDF effort limits, one substep."""
    rng = np.random.default_rng(seed)
    out = []
    sizes = dict(GPU_FLEETS)
    for name, t, inert, g, _ in robots:
        if name not in sizes:
            continue
        q, qd, qdd = stop_fleet(rng, t, inert, g, sizes[name])
        limits, lim = JR.table_limits(t), effort_limits(name, t)
        for drive, u, _ in fleet_inputs(t, inert, g, q, qd, qdd):
            ref = JR.substep(t, inert, q, qd, u, drive, DT, lim, limits, g)
            out.append(dict(name=name, t=t, inert=inert, g=g, q=q, qd=qd, u=u, drive=drive, lim=lim, limits=limits, ref=ref))
    return out


OUTSIDE_FLEETS = (("panda", 130), ("two_joint", 256), ("tree0.urdf", 130))


def outside_cases(robots, seed=311):
    """Fleets whose joints partly START OUTSIDE their limits (the issue's rule: such a joint is not pushed back, it only cannot
    move further out): stop_fleet, then on every second robot each joint is, with probability 1/3, put 0.005..0.1 beyond the
    limit nearer to it, whatever the sign of its rate -- some move inward, some outward.  Both drives, URDF effort limits."""
    rng = np.random.default_rng(seed)
    out = []
    sizes = dict(OUTSIDE_FLEETS)
    for name, t, inert, g, _ in robots:
        if name not in sizes:
            continue
        q, qd, qdd = stop_fleet(rng, t, inert, g, sizes[name])
        limits, lim = JR.table_limits(t), effort_limits(name, t)
        lo, hi = limits
        beyond = rng.uniform(0.005, 0.1, q.shape).astype(np.float32)
        pick = (rng.uniform(size=q.shape) < 1.0 / 3.0) & (np.arange(len(q)) % 2 == 1)[:, None] & np.isfinite(lo) & np.isfinite(hi)
        q = np.where(pick, np.where(q - lo < hi - q, lo - beyond, hi + beyond), q).astype(np.float32)
        for drive, u, _ in fleet_inputs(t, inert, g, q, qd, qdd):
            ref = JR.substep(t, inert, q, qd, u, drive, DT, lim, limits, g)
            out.append(dict(name=name, t=t, inert=inert, g=g, q=q, qd=qd, u=u, drive=drive, lim=lim, limits=limits, ref=ref))
    return out


def one_step_ratios(c, got, sel=None):
    """(stationarity, velocity, stop torque, step) worst ratios of `got` = dict(q, qd, qdd, tau, stop) against the case's
    reference over the robots of `sel`; velocity and stop torque nan off the Panda and the two-joint robot, the step nan off
    STEP_ROBOTS."""
    t, inert, g, ref = c["t"], c["inert"], c["g"], c["ref"]
    sel = np.ones(len(c["q"]), bool) if sel is None else sel
    res = JR.residual(t, inert, c["q"], c["qd"], got["qdd"], ref["tau"], got["stop"], g) / JR.residual_bracket(t, inert, c["q"], c["qd"], ref, g)
    out = [res[sel].max()]
    if c["name"] in ("panda", "two_joint"):
        out.append((np.abs(got["qd"] - ref["qd"]).max(1) / JR.velocity_bracket(ref, c["qd"], DT))[sel].max())
        out.append((np.abs(got["stop"] - ref["stop"]).max(1) / JR.stop_bracket(ref))[sel].max())
    else:
        out += [np.nan, np.nan]
    if c["name"] in STEP_ROBOTS:       # (the step's brackets are built on qdd's: not on the ill-conditioned trees)
        bq, bqd = JR.step_brackets(ref, DT, 1)
        out.append(max((np.abs(got["q"] - ref["q"]).max(1) / bq)[sel].max(), (np.abs(got["qd"] - ref["qd"]).max(1) / bqd)[sel].max()))
    else:
        out.append(np.nan)
    return out


def check_invariants(c, q1, stop, what, qd1=None):
    """The hard invariants of one substep from the case's state, and the signs of stop_out (where the reference's multiplier is
    clear of zero by the stop torque's bound: nearer to zero the device may rightly have dropped the dof).  With qd1 also the
    joints that start outside: where the reference leaves such a joint free and moving inward (by more than the velocity's
    bound) it is free on the device (stop exactly 0, q moved inward); where the reference holds it (strictly active, clear of
    zero) it stays where it is with qd = 0.  Returns the numbers of (inward free, outward held) joints seen."""
    lo, hi = c["limits"]
    q0 = c["q"]
    own = FR.owned_dofs(c["t"])
    inside_lo, inside_hi = own & (q0 >= lo), own & (q0 <= hi)
    assert (q1[inside_lo] >= np.broadcast_to(lo, q1.shape)[inside_lo]).all() and (q1[inside_hi] <= np.broadcast_to(hi, q1.shape)[inside_hi]).all(), what
    assert (q1[own & (q0 < lo)] >= q0[own & (q0 < lo)]).all() and (q1[own & (q0 > hi)] <= q0[own & (q0 > hi)]).all(), what
    locked = own & (lo == hi) & (q0 == lo)
    assert np.array_equal(q1[locked], q0[locked]), what
    ref = c["ref"]
    clear = np.abs(ref["stop"]) > (K_STOP * JR.stop_bracket(ref))[:, None]
    strict = (ref["strict"] != 0) & clear
    assert (np.sign(stop[strict]) == ref["strict"][strict]).all(), what
    if qd1 is None:
        return 0, 0
    outside = own & ((q0 < lo) | (q0 > hi))
    inward = np.where(q0 > hi, -ref["qd"], ref["qd"]) > (K_VEL * JR.velocity_bracket(ref, c["qd"], DT))[:, None]
    free = outside & inward & (ref["strict"] == 0) & (ref["stop"] == 0)
    assert (stop[free] == 0).all() and (np.where(q0 > hi, q0 - q1, q1 - q0)[free] > 0).all(), what
    held = outside & strict
    assert np.array_equal(q1[held], q0[held]) and (qd1[held] == 0).all(), what
    return int(free.sum()), int(held.sum())


def input_conditions(cases):
    """The fractions the issue sets on the inputs, over every state of every case (asserted by the caller)."""
    n_act = np.concatenate([c["ref"]["n_active"] for c in cases])
    fast = np.concatenate([c["ref"]["fast"] for c in cases])
    rel = np.concatenate([c["ref"]["released"] for c in cases])
    cap = np.concatenate([c["ref"]["capped"] for c in cases])
    return dict(one=float((n_act == 1).mean()), two=float((n_act >= 2).mean()), none=float(fast.mean()), released=float(rel.mean()),
                capped=int(cap.sum()), iters=int(max(c["ref"]["iters"].max() for c in cases)))


STEP_ROBOTS = ("panda", "two_joint", "tree0.urdf", "dof16.urdf")


def step_cases(robots, seed=301, states=128, substeps=STEP_SUBSTEPS):
    """The step's cases: four robots, both drives, 3 substeps of dt = 0.01, with the fp64 loop's result; and ("panda_locked") 65
    Pandas over 10 substeps with the fingers locked where they are (lower == upper == q)."""
    rng = np.random.default_rng(seed)
    out = []
    for name, t, inert, g, _ in list(robots) + [("panda_locked",) + tuple(robots[0][1:])]:
        if name not in STEP_ROBOTS + ("panda_locked",):
            continue
        locked = name == "panda_locked"
        q, qd, qdd = stop_fleet(rng, t, inert, g, 65 if locked else states)
        limits = JR.table_limits(t)
        if locked:
            substeps = 10
            q[:, 7:] = 0.02
            limits[0][7:], limits[1][7:] = 0.02, 0.02
        for drive, u, lim in fleet_inputs(t, inert, g, q, qd, qdd):
            ref = JR.dynamics_step(t, inert, q, qd, u, drive, DT, substeps, lim, limits, g)
            out.append(dict(name=name, t=t, inert=inert, g=g, q=q, qd=qd, u=u, drive=drive, lim=lim, limits=limits, ref=ref,
                            substeps=substeps, brackets=JR.step_brackets(ref, DT, substeps)))
    return out


def step_ratio(c, q_got, qd_got):
    bq, bqd = c["brackets"]
    return max((np.abs(q_got - c["ref"]["q"]).max(1) / bq).max(), (np.abs(qd_got - c["ref"]["qd"]).max(1) / bqd).max())


@pytest.fixture(scope="module")
def robots(golden_dir, tmp_path_factory):
    return H.all_robots(golden_dir, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def cases(robots):
    return stop_cases(robots) + gpu_cases(robots) + outside_cases(robots)


@pytest.fixture(scope="module")
def steps(robots):
    return step_cases(robots)


# ---- 1: the reference against itself ----------------------------------------------------------------------------------------

def test_inputs_meet_the_conditions_and_the_cap_is_twice_the_worst_count(cases, steps):
    assert len(cases) >= 42 and {c["t"].n_dof for c in cases} >= {2, 9, 12, 16}
    cond = input_conditions(cases)
    print("input conditions:", cond, "step cases' worst count:", max(int(s["ref"]["iters"].max()) for s in steps))
    assert cond["one"] >= 0.30 and cond["two"] >= 0.05 and cond["none"] >= 0.20 and cond["released"] >= 0.01 and cond["capped"] == 0, cond
    assert not any(s["ref"]["capped"].any() for s in steps)
    worst = max(cond["iters"], max(int(s["ref"]["iters"].max()) for s in steps))
    assert worst == WORST_ITERS
    hdr = open(os.path.join(CSRC, "rmp2_joint_stops.h")).read()
    assert int(re.search(r"constexpr int kStopMaxIter = (\d+);", hdr).group(1)) == 2 * WORST_ITERS


def test_reference_satisfies_the_kkt_conditions_on_every_state(cases):
    own_checked = 0
    for c in cases:
        ref, t = c["ref"], c["t"]
        own = FR.owned_dofs(t)
        for b in np.nonzero(~ref["fast"])[0]:
            l, h = JR.velocity_box(c["q"][b].astype(np.float64), DT, *c["limits"], own)
            assert JR.kkt_residual(ref["M"][b], ref["vstar"][b], l, h, ref["qd"][b]) <= 1e-9, (c["name"], b)
            own_checked += 1
        fast = ref["fast"]
        assert np.array_equal(ref["qd"][fast], ref["vstar"][fast]) and (ref["stop"][fast] == 0).all()
    assert own_checked > 1000


def test_reference_equals_brute_force_enumeration(cases, tmp_path):
    rng = np.random.default_rng(302)
    small = [c for c in cases if c["t"].n_dof <= 4]
    assert any(c["name"] == "two_joint" for c in small) and len({c["name"] for c in small}) >= 2
    checked = outside = 0
    for c in small:
        ref = c["ref"]
        own = FR.owned_dofs(c["t"])
        for b in np.nonzero(~ref["fast"])[0][:150]:
            l, h = JR.velocity_box(c["q"][b].astype(np.float64), DT, *c["limits"], own)
            want = JR.brute_force(ref["M"][b], ref["vstar"][b], l, h)
            assert np.abs(ref["qd"][b] - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (c["name"], b)
            checked += 1
            outside += int(((l == 0) & (h == 0)).sum() == 0 and ((c["q"][b] < c["limits"][0]) | (c["q"][b] > c["limits"][1])).any())
    # random SPD box problems, n <= 4, about half the dofs active
    for _ in range(300):
        n = int(rng.integers(2, 5))
        A = rng.normal(size=(n, n))
        M = A @ A.T + 0.05 * np.eye(n)
        vstar = rng.normal(size=n) * 2
        l, h = -rng.uniform(0, 1.5, n), rng.uniform(0, 1.5, n)
        lock = rng.uniform(size=n) < 0.1
        l, h = np.where(lock, 0.0, l), np.where(lock, 0.0, h)
        s = JR.solve_box(M, vstar, l.copy(), h.copy())
        assert not s["capped"]
        want = JR.brute_force(M, vstar, l, h)
        assert np.abs(s["v"] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
        checked += 1
    assert checked > 400 and outside > 50        # (states with a joint that starts outside its limits among them)


# ---- 2: the fp32 envelope: where the bounds come from -----------------------------------------------------------------------

def test_envelope_backs_the_bounds(cases, steps):
    worst = dict(res=0.0, vel=0.0, stop=0.0, step=0.0)
    for c in cases:
        e = JR.substep(c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], DT, c["lim"], c["limits"], c["g"], envelope=True)
        assert e["qd"].dtype == np.float32 and e["stop"].dtype == np.float32
        r = one_step_ratios(c, e)
        worst["res"] = max(worst["res"], r[0])
        worst["vel"], worst["stop"], worst["step"] = np.nanmax([worst["vel"], r[1]]), np.nanmax([worst["stop"], r[2]]), np.nanmax([worst["step"], r[3]])
    for s in steps:
        e = JR.dynamics_step(s["t"], s["inert"], s["q"], s["qd"], s["u"], s["drive"], DT, s["substeps"], s["lim"], s["limits"], s["g"],
                             envelope=True)
        worst["step"] = max(worst["step"], step_ratio(s, e["q"], e["qd"]))
    print("worst envelope ratios:", {k: round(float(v), 4) for k, v in worst.items()})
    assert 4 * worst["res"] <= K_RES2 and 4 * worst["vel"] <= K_VEL and 4 * worst["stop"] <= K_STOP and 4 * worst["step"] <= K_STEP2, worst


# ---- 3, 4: the device routine on the CPU ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("driver") / "joint_stops_driver")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "joint_stops_driver.cpp")], check=True, timeout=900)
    return exe


@pytest.fixture(scope="module")
def plain_driver(tmp_path_factory):
    """The existing step's driver, for the bit-for-bit comparison."""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("driver") / "forward_dynamics_driver")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "forward_dynamics_driver.cpp")], check=True, timeout=900)
    return exe


def run_driver(exe, tmp_path, t, inert, q, qd, u, drive, lim, limits, substeps=1, gravity=(0.0, 0.0, -9.81)):
    """dict(q, qd, qdd, tau, stop [B, n], status [B] uint32) of the device routine on the CPU."""
    JR.write_driver_input(str(tmp_path / "in.bin"), t, inert, q, qd, u, drive, lim, limits, DT, substeps, gravity)
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=300)
    B, n = len(q), t.n_dof
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    f = raw[:5 * B * n * 4].view(np.float32).reshape(5, B, n)
    return dict(q=f[0], qd=f[1], qdd=f[2], tau=f[3], stop=f[4], status=raw[5 * B * n * 4:].view(np.uint32))


def test_device_routine_on_the_cpu_within_half_of_each_bound(driver, cases, steps, tmp_path):
    worst = dict(res=0.0, vel=0.0, stop=0.0, step=0.0)
    most, seen = 0, [0, 0]
    for c in cases:
        d = run_driver(driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"], 1, c["g"])
        assert (d["status"] & JR.CAPPED == 0).all(), c["name"]
        most = max(most, int((d["status"] >> 8).max()))
        r = one_step_ratios(c, d)
        worst["res"] = max(worst["res"], r[0])
        worst["vel"], worst["stop"], worst["step"] = np.nanmax([worst["vel"], r[1]]), np.nanmax([worst["stop"], r[2]]), np.nanmax([worst["step"], r[3]])
        n_in, n_held = check_invariants(c, d["q"], d["stop"], c["name"], d["qd"])
        seen[0], seen[1] = seen[0] + n_in, seen[1] + n_held
    assert seen[0] > 100 and seen[1] > 100, seen     # joints that start outside: left free inward, held outward
    for s in steps:
        d = run_driver(driver, tmp_path, s["t"], s["inert"], s["q"], s["qd"], s["u"], s["drive"], s["lim"], s["limits"], s["substeps"], s["g"])
        assert (d["status"] & JR.CAPPED == 0).all(), s["name"]
        worst["step"] = max(worst["step"], step_ratio(s, d["q"], d["qd"]))
    print("worst driver ratios:", {k: round(float(v), 4) for k, v in worst.items()}, "most iterations:", most)
    assert worst["res"] <= K_RES2 / 2 and worst["vel"] <= K_VEL / 2 and worst["stop"] <= K_STOP / 2 and worst["step"] <= K_STEP2 / 2, worst


def test_device_far_limits_equal_the_existing_step_bit_for_bit(driver, plain_driver, cases, tmp_path):
    for c in [c for c in cases if c["name"] in ("panda", "two_joint", "tree1.urdf", "dof16.urdf")]:
        t, inert, g = c["t"], c["inert"], c["g"]
        q, qd, u = c["q"][:200], c["qd"][:200], c["u"][:200]
        n = t.n_dof
        for limits in ((np.full(n, -np.inf, np.float32), np.full(n, np.inf, np.float32)),
                       (np.full(n, -1e3, np.float32), np.full(n, 1e3, np.float32))):
            d = run_driver(driver, tmp_path, t, inert, q, qd, u, c["drive"], c["lim"], limits, 3, g)
            want = H.run_driver(plain_driver, tmp_path, t, inert, q, qd, u, 2, drive=c["drive"], lim=c["lim"], dt=DT, substeps=3, gravity=g)
            for k, name in enumerate(("q", "qd", "qdd", "tau")):
                assert np.array_equal(d[name], want[k], equal_nan=True), (c["name"], name)
            assert (d["stop"] == 0).all() and (d["status"] == 0).all(), c["name"]


# ---- 5: smaller checks -------------------------------------------------------------------------------------------------------

def test_device_status_flags_and_locked_joint(driver, cases, tmp_path):
    c = next(c for c in cases if c["name"] == "panda" and c["drive"] == FR.TORQUE)
    d = run_driver(driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"], 1, c["g"])
    assert np.array_equal((d["status"] & JR.ACTIVE) != 0, ~c["ref"]["fast"])
    fast = c["ref"]["fast"]
    assert (d["status"][fast] == 0).all() and (d["stop"][fast] == 0).all()
    lo, hi = (x.copy() for x in c["limits"])
    q = c["q"][:64].copy()
    q[:, 7:] = 0.02
    lo[7:], hi[7:] = 0.02, 0.02                                    # the fingers locked where they are
    d = run_driver(driver, tmp_path, c["t"], c["inert"], q, c["qd"][:64], c["u"][:64], c["drive"], c["lim"], (lo, hi), 3, c["g"])
    assert (d["q"][:, 7:] == np.float32(0.02)).all() and (d["qd"][:, 7:] == 0).all()


def test_device_unowned_dof_has_no_bound(driver, tmp_path):
    name, t, inert = H.unowned_dof_robot(tmp_path)
    assert list(FR.owned_dofs(t)) == [True, False, True]
    q, qd, qdd = DR.random_states(np.random.default_rng(303), t, 64)
    q[:, 1], qd[:, 1] = 0.5, 3.0                                   # dof 1, which no joint owns, far outside "its" limits and leaving
    lo, hi = np.array([-1e3, -0.1, -1e3], np.float32), np.array([1e3, 0.1, 1e3], np.float32)
    far = (np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32))
    for drive, u in ((FR.ACCEL, qdd), (FR.TORQUE, DR.rnea(t, inert, q, qd, qdd).astype(np.float32))):
        d = run_driver(driver, tmp_path, t, inert, q, qd, u, drive, None, (lo, hi), 2)
        w = run_driver(driver, tmp_path, t, inert, q, qd, u, drive, None, far, 2)
        for k in ("q", "qd", "qdd", "tau", "stop", "status"):
            assert np.array_equal(d[k], w[k]), k
        assert (d["status"] == 0).all() and (d["stop"] == 0).all()
        assert np.array_equal(d["qd"][:, 1], qd[:, 1]) and (d["q"][:, 1] > 0.5).all()      # its rate stays, its position coasts
    # and a stop on an owned dof beside it works as ever
    lo2, hi2 = lo.copy(), hi.copy()
    q[:, 2], qd[:, 2], hi2[2] = 0.299, 1.0, 0.3
    d = run_driver(driver, tmp_path, t, inert, q, qd, np.zeros_like(q), FR.ACCEL, None, (lo2, hi2), 1)
    assert (d["q"][:, 2] == np.float32(0.3)).all() and (d["status"] & JR.ACTIVE != 0).all() and (d["stop"][:, 1] == 0).all()
    assert np.array_equal(d["qd"][:, 1], qd[:, 1])


def test_read_joint_limits(tmp_path):
    from riemannian_motion_policies_amd import urdf as U
    lo, hi = U.read_joint_limits(U.PANDA_URDF, U.PANDA_ORDER)
    assert lo.dtype == np.float32 and hi.dtype == np.float32 and lo.shape == (9,) and hi.shape == (9,)
    assert np.allclose(lo, [-2.9671, -1.8326, -2.9671, -3.1416, -2.9671, -0.0873, -2.9671, 0.0, 0.0])
    assert np.allclose(hi, [2.9671, 1.8326, 2.9671, 0.0, 2.9671, 3.8223, 2.9671, 0.04, 0.04])
    tl, th = JR.table_limits(U.panda_table())
    assert np.array_equal(lo, tl) and np.array_equal(hi, th)
    t2 = U.two_joint_table()
    lo2, hi2 = U.read_joint_limits(U.TWO_JOINT_URDF, U.TWO_JOINT_ORDER)
    assert np.array_equal(lo2, JR.table_limits(t2)[0]) and np.array_equal(hi2, JR.table_limits(t2)[1]) and list(lo2) == [np.float32(-3.14)] * 2 and list(hi2) == [np.float32(3.14)] * 2
    path = str(tmp_path / "r.urdf")
    with open(path, "w") as f:
        f.write('<?xml version="1.0"?><robot name="r"><link name="base"/><link name="a"/><link name="b"/><link name="c"/>'
                '<joint name="j1" type="continuous"><parent link="base"/><child link="a"/><axis xyz="0 0 1"/>'
                '<limit lower="-1" upper="1" effort="3"/></joint>'
                '<joint name="j2" type="revolute"><parent link="a"/><child link="b"/><axis xyz="0 0 1"/></joint>'
                '<joint name="j3" type="revolute"><parent link="b"/><child link="c"/><axis xyz="0 0 1"/><limit upper="0.5"/></joint>'
                '</robot>')
    lo, hi = U.read_joint_limits(path, ["j3", "j1", "j2"])
    assert list(lo) == [-np.inf] * 3 and list(hi) == [0.5, np.inf, np.inf]
    with pytest.raises(ValueError, match="no joint named"):
        U.read_joint_limits(path, ["j4"])


def test_symbol_declared_bound_and_null_handle_refused(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    assert ("int rmp2_dynamics_step_stops(rmp2_handle *h, float *q, float *qd, const float *u, int32_t drive,\n"
            "                             const float *tau_limit, const float *q_lower, const float *q_upper, float dt, int32_t substeps,\n"
            "                             float *qdd_out, float *tau_out, float *stop_out, uint32_t *status_out, int32_t R, void *stream);") in hdr
    assert "#define RMP2_STOP_ACTIVE 1u" in hdr and "#define RMP2_STOP_CAPPED 2u" in hdr and "#define RMP2_ABI_VERSION 5" in hdr
    assert "l.rmp2_dynamics_step_stops.argtypes" in open(os.path.join(ROOT, "riemannian_motion_policies_amd", "_native.py")).read()
    assert '"rmp2_dynamics_step_stops"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import torch  # noqa: F401  (one HIP runtime per process: PyTorch's first, as _native.lib loads it)
    lib = C.CDLL(hip_lib)
    lib.rmp2_dynamics_step_stops.argtypes = [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_float, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]
    assert lib.rmp2_dynamics_step_stops(None, None, None, None, 1, None, None, None, 0.01, 1, None, None, None, None, 0, None) == -1

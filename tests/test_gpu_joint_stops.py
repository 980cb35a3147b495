"""Joint-limit stops on the GPU (include/rmp2.h rmp2_dynamics_step_stops, Engine.dynamics_step(q_limits=...)) against the fp64
restatement of tests/joint_stops_reference.py: fleets across the wave edges, far limits bit for bit against the step without
stops, driving into a stop, a 10-substep step with locked fingers, isolation of poisoned and singular robots, graph capture and
refusals.

The bounds were fixed before the first GPU run, from the fp32 envelope restatement measured on the CPU
(tests/test_joint_stops_host.py; K = 4 x the envelope's worst ratio, rounded up to one significant figure), per robot:
    stationarity  max_j |rnea64(q, qd, qdd_dev) - tau_applied - stop_dev|_j <= K_RES2 (1e-4 + 1e-5 s),   K_RES2 = 0.9 (envelope 0.215)
    velocity      max_j |v_dev - v_ref|_j <= K_VEL x joint_stops_reference.velocity_bracket,                K_VEL = 1    (envelope 0.229)
    stop torque   max_j |stop_dev - stop_ref|_j <= K_STOP x joint_stops_reference.stop_bracket,             K_STOP = 0.3 (envelope 0.0594)
                  (velocity and stop torque on the Panda and the two-joint robot only)
    the step      |q_dev - q_ref|, |qd_dev - qd_ref| <= K_STEP2 x step_brackets,                            K_STEP2 = 7  (envelope 1.709)
The device routine run on the CPU sits within half of each (worst ratios 0.235, 0.259, 0.036, 1.709).  The hard invariants carry
no K (test_joint_stops_host.check_invariants)."""
import numpy as np
import pytest

import forward_dynamics_reference as FR
import joint_stops_reference as JR
import test_forward_dynamics_host as H
import test_joint_stops_host as S
from test_joint_stops_host import DT, K_RES2, K_STEP2, K_STOP, K_VEL, WORST_ITERS

pytestmark = pytest.mark.gpu


def _engine(table, inert=None, gravity=(0.0, 0.0, -9.81)):
    from riemannian_motion_policies_amd import descriptor as D
    from riemannian_motion_policies_amd.engine import Engine
    eng = Engine(D.build_desc(table, []), 0)
    if inert is not None:
        eng.set_inertials(inert, gravity=gravity)
    return eng


def _dev(*xs):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in xs)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _step(eng, c, R, substeps=1, limits=None, q=None, qd=None, u=None):
    """dict(q, qd, qdd, tau, stop, status) of the stops step on the first R robots of the case."""
    import torch
    q, qd, u = _dev((c["q"] if q is None else q)[:R], (c["qd"] if qd is None else qd)[:R], (c["u"] if u is None else u)[:R])
    qdd, tau, stop = torch.empty_like(q), torch.empty_like(q), torch.full_like(q, 7.0)
    status = torch.full((len(q),), -1, dtype=torch.int32, device=q.device)
    eng.dynamics_step(q, qd, u, DT, substeps=substeps, drive="accel" if c["drive"] == FR.ACCEL else "torque", tau_limit=c["lim"],
                      qdd_out=qdd, tau_out=tau, q_limits=c["limits"] if limits is None else limits, stop_out=stop, status_out=status)
    return dict(q=_host(q), qd=_host(qd), qdd=_host(qdd), tau=_host(tau), stop=_host(stop), status=_host(status))


@pytest.fixture(scope="module")
def robots(golden_dir, tmp_path_factory):
    return H.all_robots(golden_dir, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def fleets(robots):
    return S.gpu_cases(robots)


@pytest.fixture(scope="module")
def panda(robots):
    name, t, inert, g, _ = robots[0]
    assert name == "panda"
    return t, inert


def _first(c, R):
    """The case cut to its first R robots (its reference is per robot)."""
    out = dict(c)
    for k in ("q", "qd", "u"):
        out[k] = c[k][:R]
    out["ref"] = {k: (v[:R] if isinstance(v, np.ndarray) else v) for k, v in c["ref"].items()}
    return out


# ---- 1: fleets across the wave edges, both drives, URDF effort limits ------------------------------------------------------

def test_one_substep_against_the_reference_across_fleet_sizes(fleets):
    assert {(c["name"], len(c["q"])) for c in fleets} == set(S.GPU_FLEETS) and len(fleets) == 8
    engines = {}
    active = 0
    for c in fleets:
        if c["name"] not in engines:
            engines[c["name"]] = _engine(c["t"], c["inert"], c["g"])
        eng = engines[c["name"]]
        assert int(c["ref"]["iters"].max()) <= WORST_ITERS
        for R in ((1, 63, 64, 65) if c["name"] == "panda" else (len(c["q"]),)):
            cc = _first(c, R)
            d = _step(eng, c, R)
            what = f"{c['name']} drive={c['drive']} R={R}"
            assert d["q"].shape == (R, c["t"].n_dof) and np.isfinite(d["q"]).all() and np.isfinite(d["stop"]).all(), what
            r = S.one_step_ratios(cc, d)
            print(f"{what}: stationarity {r[0]:.3f} (bound {K_RES2}), velocity {r[1]:.3f} ({K_VEL}), stop torque {r[2]:.3f} ({K_STOP})")
            assert r[0] <= K_RES2, (what, r)
            if c["name"] in ("panda", "two_joint"):
                assert r[1] <= K_VEL and r[2] <= K_STOP, (what, r)
            print(f"{what}: step {r[3]:.3f} (bound {K_STEP2})")
            assert c["name"] in S.STEP_ROBOTS and r[3] <= K_STEP2, (what, r)
            S.check_invariants(cc, d["q"], d["stop"], what, d["qd"])
            assert (d["status"] & JR.CAPPED == 0).all() and ((d["status"] >> 8) <= 2 * WORST_ITERS).all(), what
            fast = cc["ref"]["fast"]
            assert (d["stop"][fast] == 0).all(), what
            active += int((d["status"] & JR.ACTIVE != 0).sum())
    assert active > 300


def test_joints_that_start_outside_are_not_pushed_back_and_move_no_further_out(robots):
    fleets = S.outside_cases(robots)
    assert {(c["name"], len(c["q"])) for c in fleets} == set(S.OUTSIDE_FLEETS) and len(fleets) == 6
    seen = [0, 0]
    engines = {}
    for c in fleets:
        if c["name"] not in engines:
            engines[c["name"]] = _engine(c["t"], c["inert"], c["g"])
        lo, hi = c["limits"]
        assert ((c["q"] < lo) | (c["q"] > hi)).sum() > 50 and int(c["ref"]["iters"].max()) <= WORST_ITERS
        d = _step(engines[c["name"]], c, len(c["q"]))
        what = f"{c['name']} drive={c['drive']}, joints outside"
        r = S.one_step_ratios(c, d)
        print(f"{what}: stationarity {r[0]:.3f} (bound {K_RES2}), velocity {r[1]:.3f} ({K_VEL}), stop torque {r[2]:.3f} ({K_STOP}), step {r[3]:.3f} ({K_STEP2})")
        assert r[0] <= K_RES2 and r[3] <= K_STEP2, (what, r)
        if c["name"] in ("panda", "two_joint"):
            assert r[1] <= K_VEL and r[2] <= K_STOP, (what, r)
        n_in, n_held = S.check_invariants(c, d["q"], d["stop"], what, d["qd"])
        seen[0], seen[1] = seen[0] + n_in, seen[1] + n_held
        assert (d["status"] & JR.CAPPED == 0).all(), what
    assert seen[0] > 100 and seen[1] > 100, seen        # left free moving inward (stop exactly 0); held where they push outward


# ---- 2: far limits -----------------------------------------------------------------------------------------------------------

def test_far_limits_equal_the_step_without_stops_bit_for_bit(fleets):
    import torch
    for c in [c for c in fleets if c["name"] == "panda"]:
        eng = _engine(c["t"], c["inert"], c["g"])
        n = c["t"].n_dof
        drive = "accel" if c["drive"] == FR.ACCEL else "torque"
        q0, qd0, u = _dev(c["q"], c["qd"], c["u"])
        want = [q0.clone(), qd0.clone(), torch.empty_like(q0), torch.empty_like(q0)]
        eng.dynamics_step(want[0], want[1], u, DT, substeps=3, drive=drive, tau_limit=c["lim"], qdd_out=want[2], tau_out=want[3])
        for limits in ((np.full(n, -np.inf, np.float32), np.full(n, np.inf, np.float32)),
                       (np.full(n, -1e3, np.float32), np.full(n, 1e3, np.float32))):
            got = [q0.clone(), qd0.clone(), torch.empty_like(q0), torch.empty_like(q0)]
            stop = torch.full_like(q0, 7.0)
            status = torch.full((len(q0),), -1, dtype=torch.int32, device=q0.device)
            eng.dynamics_step(got[0], got[1], u, DT, substeps=3, drive=drive, tau_limit=c["lim"], qdd_out=got[2], tau_out=got[3],
                              q_limits=limits, stop_out=stop, status_out=status)
            torch.cuda.synchronize()
            assert len(q0) == 65 and not torch.equal(got[0], q0)
            for a, b in zip(got, want):
                assert torch.equal(a, b)
            assert bool((stop == 0).all()) and bool((status == 0).all())


# ---- 3: driving into a stop --------------------------------------------------------------------------------------------------

def test_two_joint_robot_driven_into_its_upper_stop_rests_on_it(robots):
    import torch
    name, t, inert, g, _ = robots[1]
    assert name == "two_joint"
    eng = _engine(t, inert, g)
    lo, hi = JR.table_limits(t)
    rng = np.random.default_rng(320)
    R = 64
    q = np.stack([hi[0] - rng.uniform(0.05, 0.3, R), rng.uniform(-1.0, 1.0, R)], 1).astype(np.float32)
    qd = np.zeros_like(q)
    grav = np.abs(FR.bias(t, inert, rng.uniform(-3.14, 3.14, (512, 2)), np.zeros((512, 2)), g)).max()
    tau = np.tile(np.array([5.0 * grav + 5.0, 0.0], np.float32), (R, 1))       # a constant torque that gravity never holds
    qg, qdg, ug = _dev(q, qd, tau)
    status = torch.zeros(R, dtype=torch.int32, device=qg.device)
    eng.dynamics_step(qg, qdg, ug, DT, substeps=299, drive="torque", q_limits=(lo, hi), status_out=status)
    q_pre, qd_pre = _host(qg).copy(), _host(qdg).copy()
    qdd, tapp, stop = torch.empty_like(qg), torch.empty_like(qg), torch.empty_like(qg)
    eng.dynamics_step(qg, qdg, ug, DT, substeps=1, drive="torque", q_limits=(lo, hi), qdd_out=qdd, tau_out=tapp, stop_out=stop)
    q1, qd1 = _host(qg), _host(qdg)
    assert (q1[:, 0] == hi[0]).all() and (qd1[:, 0] == 0).all()                 # on the limit, at rest, exactly
    assert (q1[:, 1] >= lo[1]).all() and (q1[:, 1] <= hi[1]).all()
    assert (_host(status) & JR.ACTIVE != 0).all() and (_host(status) & JR.CAPPED == 0).all()
    assert (_host(stop)[:, 0] < 0).all()                                        # the stop pushes back
    ref = JR.substep(t, inert, q_pre, qd_pre, tau, FR.TORQUE, DT, None, (lo, hi), g)
    assert int(ref["iters"].max()) <= WORST_ITERS
    ratio = JR.residual(t, inert, q_pre, qd_pre, _host(qdd), _host(tapp), _host(stop), g) / JR.residual_bracket(t, inert, q_pre, qd_pre, ref, g)
    print(f"driven into the stop: stationarity {ratio.max():.3f} (bound {K_RES2})")
    assert (ratio <= K_RES2).all(), float(ratio.max())


# ---- 4: ten substeps with locked fingers ------------------------------------------------------------------------------------

def test_ten_substeps_on_the_panda_with_locked_fingers(robots):
    cases = [s for s in S.step_cases(robots) if s["name"] == "panda_locked"]
    assert len(cases) == 2
    eng = _engine(cases[0]["t"], cases[0]["inert"], cases[0]["g"])
    for s in cases:
        assert s["substeps"] == 10 and len(s["q"]) == 65 and int(s["ref"]["iters"].max()) <= WORST_ITERS
        d = _step(eng, s, 65, substeps=10)
        ratio = S.step_ratio(s, d["q"], d["qd"])
        print(f"panda, locked fingers, drive={s['drive']}: step ratio {ratio:.3f} (bound {K_STEP2})")
        assert ratio <= K_STEP2, ratio
        assert (d["q"][:, 7:] == np.float32(0.02)).all() and (d["qd"][:, 7:] == 0).all()
        assert (d["status"] & JR.CAPPED == 0).all() and (d["status"] & JR.ACTIVE != 0).all()
        lo, hi = s["limits"]
        assert (d["q"] >= lo).all() and (d["q"] <= hi).all()


# ---- 5: isolation ------------------------------------------------------------------------------------------------------------

def test_poisoned_and_singular_robots_are_nan_and_leave_their_neighbours_alone(fleets, tmp_path):
    c = next(c for c in fleets if c["name"] == "panda" and c["drive"] == FR.TORQUE)
    eng = _engine(c["t"], c["inert"], c["g"])
    clean = _step(eng, c, 65, substeps=2)
    q, qd, u = c["q"].copy(), c["qd"].copy(), c["u"].copy()
    q[3, 2], qd[40, 0], u[64, 8] = np.nan, np.inf, np.nan
    bad = np.zeros(65, bool)
    bad[[3, 40, 64]] = True
    d = _step(eng, c, 65, substeps=2, q=q, qd=qd, u=u)
    for k in ("q", "qd", "qdd", "tau", "stop"):
        assert np.isnan(d[k][bad]).all() and np.array_equal(d[k][~bad], clean[k][~bad]), k
    assert np.array_equal(d["status"][~bad], clean["status"][~bad])
    # a singular model (a massless last link): in the acceleration drive nothing factors M until a stop is active, so the robots
    # that meet a stop are NaN and the others are those of the run with far limits
    name, t, inert = H.singular_robot(tmp_path)
    e = _engine(t, inert)
    rng = np.random.default_rng(321)
    R = 65
    q = rng.uniform(-1.0, 1.0, (R, 3)).astype(np.float32)
    qd = rng.uniform(-1.0, 1.0, (R, 3)).astype(np.float32)
    u = rng.uniform(-1.0, 1.0, (R, 3)).astype(np.float32)
    lo, hi = np.full(3, -2.0, np.float32), np.full(3, 2.0, np.float32)
    hit = np.zeros(R, bool)
    hit[[0, 17, 64]] = True
    q[hit, 1], qd[hit, 1], u[hit, 1] = 1.999, 1.0, 0.0                            # joint 1 runs into its upper stop
    s = dict(q=q, qd=qd, u=u, drive=FR.ACCEL, lim=None, limits=(lo, hi))
    far = _step(e, s, R, limits=(np.full(3, -np.inf, np.float32), np.full(3, np.inf, np.float32)))
    d = _step(e, s, R)
    assert np.isfinite(far["q"]).all() and np.array_equal(far["qdd"], u)
    for k in ("q", "qd", "qdd", "stop"):
        assert np.isnan(d[k][hit]).all(), k
    for k in ("q", "qd", "qdd", "tau"):
        assert np.array_equal(d[k][~hit], far[k][~hit]), k
    assert (d["stop"][~hit] == 0).all() and (d["status"][~hit] == 0).all()


# ---- 6: graph capture ----------------------------------------------------------------------------------------------------------

def test_graph_capture_replays_the_same_bytes(fleets):
    import torch
    c = next(c for c in fleets if c["name"] == "panda" and c["drive"] == FR.ACCEL)
    eng = _engine(c["t"], c["inert"], c["g"])
    q0, qd0, u = _dev(c["q"], c["qd"], c["u"])
    lim, lo, hi = _dev(c["lim"], *c["limits"])
    q, qd = q0.clone(), qd0.clone()
    qdd, tau, stop = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    status = torch.zeros(len(q), dtype=torch.int32, device=q.device)
    side = torch.cuda.Stream()

    def call():
        eng.dynamics_step(q, qd, u, DT, substeps=3, tau_limit=lim, qdd_out=qdd, tau_out=tau, q_limits=(lo, hi), stop_out=stop,
                          status_out=status)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    eager = [x.clone() for x in (q, qd, qdd, tau, stop, status)]
    assert bool((status & JR.ACTIVE != 0).any()) and not torch.equal(q, q0)
    g = torch.cuda.CUDAGraph()
    q.copy_(q0)
    qd.copy_(qd0)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):   # one stream, no parallel branches
        call()
    for x in (qdd, tau, stop, status):
        x.zero_()
    q.copy_(q0)
    qd.copy_(qd0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip((q, qd, qdd, tau, stop, status), eager):
        assert torch.equal(a, b)


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(panda):
    import torch
    from riemannian_motion_policies_amd import _native
    t, inert = panda
    eng = _engine(t, inert)
    q, qd, u = (torch.zeros((4, 9), device="cuda") for _ in range(3))
    lo, hi = JR.table_limits(t)
    swapped = lo.copy()
    swapped[2] = hi[2] + 1.0
    with pytest.raises(ValueError, match="lower <= upper"):
        eng.dynamics_step(q, qd, u, DT, q_limits=(swapped, hi))
    nan = hi.copy()
    nan[0] = np.nan
    with pytest.raises(ValueError, match="no NaN"):
        eng.dynamics_step(q, qd, u, DT, q_limits=(lo, nan))
    with pytest.raises(ValueError, match=r"must be \[9\]"):
        eng.dynamics_step(q, qd, u, DT, q_limits=(lo[:8], hi[:8]))
    with pytest.raises(ValueError, match=r"must be \[9\]"):
        eng.dynamics_step(q, qd, u, DT, q_limits=(torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")))
    with pytest.raises(ValueError, match="pair"):
        eng.dynamics_step(q, qd, u, DT, q_limits=lo)
    with pytest.raises(ValueError, match="stop_out must be"):
        eng.dynamics_step(q, qd, u, DT, q_limits=(lo, hi), stop_out=torch.zeros((3, 9), device="cuda"))
    with pytest.raises(ValueError, match="status_out"):
        eng.dynamics_step(q, qd, u, DT, q_limits=(lo, hi), status_out=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError, match="need q_limits"):
        eng.dynamics_step(q, qd, u, DT, stop_out=torch.zeros((4, 9), device="cuda"))
    with pytest.raises(_native.Rmp2Error, match="substeps"):
        eng.dynamics_step(q, qd, u, DT, substeps=0, q_limits=(lo, hi))
    with pytest.raises(_native.Rmp2Error, match="dt must be"):
        eng.dynamics_step(q, qd, u, 0.0, q_limits=(lo, hi))
    bare = _engine(t)
    with pytest.raises(_native.Rmp2Error, match="rmp2_set_inertials"):
        bare.dynamics_step(q, qd, u, DT, q_limits=(lo, hi))
    assert bool((q == 0).all())                                               # nothing ran


def test_host_limits_upload_once_per_value(panda, monkeypatch):
    import torch
    t, inert = panda
    eng = _engine(t, inert)
    q, qd, u = (torch.zeros((4, 9), device="cuda") for _ in range(3))
    lo, hi = JR.table_limits(t)
    eng.dynamics_step(q, qd, u, DT, q_limits=(lo, hi))
    first = eng._q_limits
    eng.dynamics_step(q, qd, u, DT, q_limits=(lo.copy(), hi.copy()))
    assert eng._q_limits is first
    eng.dynamics_step(q, qd, u, DT, q_limits=(lo - 1.0, hi))
    assert eng._q_limits is not first

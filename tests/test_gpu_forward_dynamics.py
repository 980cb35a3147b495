"""The plant on the GPU (include/rmp2.h rmp2_mass_matrix / rmp2_forward_dynamics / rmp2_dynamics_step) against the fp64
restatements of tests/forward_dynamics_reference.py: the reference robots across fleet sizes, random trees, the round trip
through the inverse dynamics, the saturated acceleration drive, the step against the fp64 loop, the singular robot and poisoned
rows, graph capture, untouched neighbours, refusals and the class surface.

The bounds were fixed before the first GPU run, from the fp32 envelope restatement measured on the CPU
(tests/test_forward_dynamics_host.py; K = 4 x the envelope's worst ratio, rounded up to one significant figure), per robot:
    residual     max_j |rnea64(q, qd, qdd_dev) - tau_applied|_j <= K_RES (1e-4 + 1e-5 s),      K_RES = 0.6  (envelope 0.128)
                 s = max(max|tau_applied|, max|bias|, max_j sum_k |M_jk| |qdd_ref_k|)
    mass matrix  max|M_dev - M_ref| <= K_M (1e-6 + 1e-5 max|M_ref|),                             K_M = 0.6    (envelope 0.128)
    qdd itself   max_j |qdd_dev - qdd_ref|_j <= K_QDD (1e-4 + 1e-5 max|qdd_ref|),               K_QDD = 2    (envelope 0.251)
                 (Panda and two-joint robot only: the trees' cond(M) reaches 1e4)
    the step     |q_dev - q_ref|, |qd_dev - qd_ref| <= K_STEP x step_brackets,                   K_STEP = 2   (envelope 0.446)
The device routines run on the CPU sit within half of each (worst ratios 0.117, 0.136, 0.245, 0.446)."""
import numpy as np
import pytest

import dynamics_reference as DR
import forward_dynamics_reference as FR
import test_forward_dynamics_host as H
from test_forward_dynamics_host import DT, K_M, K_QDD, K_RES, K_STEP
from test_inverse_dynamics_host import fixture_inertials

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


@pytest.fixture(scope="module")
def robots(golden_dir, tmp_path_factory):
    return H.all_robots(golden_dir, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def panda(robots):
    name, t, inert, g, _ = robots[0]
    assert name == "panda"
    return t, inert


@pytest.fixture(scope="module")
def panda_fleet(panda):
    """4 097 Panda states with their fp64 answers, shared by the tests (fleets of R robots are its first R rows)."""
    t, inert = panda
    q, qd, qdd = H.fleet_states(np.random.default_rng(200), t, inert, (0.0, 0.0, -9.81), 4097)
    tau_ref = DR.rnea(t, inert, q, qd, qdd)
    tau = tau_ref.astype(np.float32)
    fd = FR.forward_dynamics(t, inert, q, qd, tau)
    return dict(q=q, qd=qd, qdd=qdd, tau_ref=tau_ref, tau=tau, fd=fd, br=FR.residual_bracket(t, inert, q, qd, fd, tau),
                M=FR.mass_matrix(t, inert, q))


def _check_residual(t, inert, q, qd, qdd_dev, tapp, qdd_ref, g, what, bracket=None):
    br = FR.residual_bracket(t, inert, q, qd, qdd_ref, tapp, g) if bracket is None else bracket
    ratio = FR.residual(t, inert, q, qd, qdd_dev, tapp, g) / br
    print(f"{what}: residual ratio {ratio.max():.3f} (bound {K_RES})")
    assert np.isfinite(qdd_dev).all() and (ratio <= K_RES).all(), (what, float(ratio.max()))


def _check_qdd(qdd_dev, qdd_ref, what):
    ratio = np.abs(qdd_dev - qdd_ref).max(1) / FR.qdd_bracket(qdd_ref)
    print(f"{what}: qdd ratio {ratio.max():.3f} (bound {K_QDD})")
    assert (ratio <= K_QDD).all(), (what, float(ratio.max()))


def _check_mass(M_dev, M_ref, what):
    assert np.array_equal(M_dev, np.swapaxes(M_dev, 1, 2)), what          # symmetric bit for bit
    ratio = np.abs(M_dev - M_ref).reshape(len(M_ref), -1).max(1) / FR.mass_bracket(M_ref)
    print(f"{what}: mass matrix ratio {ratio.max():.3f} (bound {K_M})")
    assert (ratio <= K_M).all(), (what, float(ratio.max()))


# ---- 1, 2: forward dynamics and the mass matrix across the wave edges ------------------------------------------------------

def test_forward_dynamics_panda_and_two_joint_across_fleet_sizes(robots, panda, panda_fleet):
    t, inert = panda
    eng = _engine(t, inert)
    f = panda_fleet
    for R in (1, 63, 64, 65, 4097):
        got = _host(eng.forward_dynamics(*_dev(f["q"][:R], f["qd"][:R], f["tau"][:R])))
        assert got.shape == (R, 9)
        _check_residual(t, inert, f["q"][:R], f["qd"][:R], got, f["tau"][:R], f["fd"][:R], (0.0, 0.0, -9.81), f"panda R={R}", f["br"][:R])
        _check_qdd(got, f["fd"][:R], f"panda R={R}")
    name, t2, inert2, g, _ = robots[1]
    assert name == "two_joint"
    eng2 = _engine(t2, inert2)
    q, qd, qdd = H.fleet_states(np.random.default_rng(201), t2, inert2, g, 1000)
    tau = DR.rnea(t2, inert2, q, qd, qdd).astype(np.float32)
    ref = FR.forward_dynamics(t2, inert2, q, qd, tau)
    got = _host(eng2.forward_dynamics(*_dev(q, qd, tau)))
    _check_residual(t2, inert2, q, qd, got, tau, ref, g, "two_joint")
    _check_qdd(got, ref, "two_joint")


def test_mass_matrix_fleets_trees_unowned_and_dropped_joints(robots, panda, panda_fleet, tmp_path):
    from riemannian_motion_policies_amd import urdf as U
    t, inert = panda
    eng = _engine(t, inert)
    for R in (1, 63, 64, 65, 4097):
        got = _host(eng.mass_matrix(*_dev(panda_fleet["q"][:R])))
        assert got.shape == (R, 9, 9)
        _check_mass(got, panda_fleet["M"][:R], f"panda R={R}")
    rng = np.random.default_rng(202)
    dropped = 0
    for name, tt, ii, g, _ in robots[1:]:
        e = _engine(tt, ii, g)
        q, _, _ = DR.random_states(rng, tt, 256)
        _check_mass(_host(e.mass_matrix(*_dev(q))), FR.mass_matrix(tt, ii, q), name)
        # a movable joint missing from the order is held at 0: it has no row, and M is that of the tree with the joint welded
        dropped += any(tt.q_index[f] < 0 and tt.joint_type[f] != U.JOINT_FIXED for f in range(tt.n_frames))
        e.close()
    assert dropped >= 2
    name, tu, iu = H.unowned_dof_robot(tmp_path)
    e = _engine(tu, iu)
    q, qd, qdd = DR.random_states(rng, tu, 70)
    M = _host(e.mass_matrix(*_dev(q)))
    assert (M[:, 1, :] == [0.0, 1.0, 0.0]).all() and (M[:, :, 1] == [0.0, 1.0, 0.0]).all()      # the unowned dof's row is e_j
    _check_mass(M, FR.mass_matrix(tu, iu, q), name)
    tau = DR.rnea(tu, iu, q, qd, qdd).astype(np.float32)
    got = _host(e.forward_dynamics(*_dev(q, qd, tau)))
    assert (got[:, 1] == 0).all()
    _check_residual(tu, iu, q, qd, got, tau, FR.forward_dynamics(tu, iu, q, qd, tau), (0.0, 0.0, -9.81), name)


# ---- 3: random trees ---------------------------------------------------------------------------------------------------------

def test_forward_dynamics_random_trees(robots):
    rng = np.random.default_rng(203)
    trees = robots[2:]
    assert any(t.n_frames == 32 and t.n_dof == 12 for _, t, _, _, _ in trees) and any(t.n_dof == 16 for _, t, _, _, _ in trees)
    for name, t, inert, g, _ in trees:
        assert g == (0.5, -1.0, -9.81)
        eng = _engine(t, inert, g)
        q, qd, qdd = H.fleet_states(rng, t, inert, g, 256)
        tau = DR.rnea(t, inert, q, qd, qdd, g).astype(np.float32)
        got = _host(eng.forward_dynamics(*_dev(q, qd, tau)))
        _check_residual(t, inert, q, qd, got, tau, FR.forward_dynamics(t, inert, q, qd, tau, g), g, name)
        eng.close()


# ---- 4: the round trip on the device ---------------------------------------------------------------------------------------

def test_round_trip_through_the_inverse_dynamics_on_the_device(panda, panda_fleet):
    t, inert = panda
    eng = _engine(t, inert)
    q, qd, qdd = _dev(*(panda_fleet[k][:1024] for k in ("q", "qd", "qdd")))
    back = _host(eng.forward_dynamics(q, qd, eng.inverse_dynamics(q, qd, qdd)))
    _check_qdd(back, panda_fleet["qdd"][:1024].astype(np.float64), "round trip")


# ---- 5: the acceleration drive against limits --------------------------------------------------------------------------------

def test_acceleration_drive_saturates_some_robots_and_tracks_the_rest_bit_for_bit(panda, panda_fleet):
    import torch
    t, inert = panda
    eng = _engine(t, inert)
    f = panda_fleet
    q, qd, u, tau_ref = f["q"], f["qd"], f["qdd"], f["tau_ref"]
    lim = H.median_limits(tau_ref)
    sat, unsat, undecided = H.saturation_classes(tau_ref, lim, H.id_bound(tau_ref))
    assert sat.mean() >= 0.1 and unsat.mean() >= 0.1 and undecided.mean() <= 0.01, (sat.mean(), unsat.mean(), undecided.mean())
    ref_qdd, ref_tau = FR.evaluate(t, inert, q, qd, u, FR.ACCEL, lim)
    qg, qdg, ug = _dev(q, qd, u)
    q0, qd0 = qg.clone(), qdg.clone()
    qdd_out, tau_out = torch.empty_like(qg), torch.empty_like(qg)
    eng.dynamics_step(qg, qdg, ug, DT, tau_limit=lim, qdd_out=qdd_out, tau_out=tau_out)
    got, tapp = _host(qdd_out), _host(tau_out)
    assert np.array_equal(got[unsat], u[unsat])                                   # nothing saturates: qdd_des bit for bit
    assert H.unclamped_torques_within(tapp[~undecided], tau_ref[~undecided], lim, H.id_bound(tau_ref)[~undecided]).all()
    _check_residual(t, inert, q[sat], qd[sat], got[sat], ref_tau[sat], ref_qdd[sat], (0.0, 0.0, -9.81), "saturated")
    clamped = np.abs(tau_ref) > lim
    assert np.array_equal(np.abs(tapp)[clamped & sat[:, None]], np.broadcast_to(lim, tapp.shape)[clamped & sat[:, None]])
    # the state moved by the integrator from that qdd
    qd1 = _host(qdg)
    assert np.abs(qd1 - (_host(qd0) + np.float32(DT) * got)).max() <= 1e-6
    assert np.abs(_host(qg) - (_host(q0) + np.float32(DT) * qd1)).max() <= 1e-6
    # no limit at all, as None and as +inf: every robot tracks bit for bit
    for none in (None, np.full(9, np.inf, np.float32)):
        qg, qdg = q0.clone(), qd0.clone()
        eng.dynamics_step(qg, qdg, ug, DT, tau_limit=none, qdd_out=qdd_out)
        assert np.array_equal(_host(qdd_out), u)


# ---- 6: the step against the fp64 loop -------------------------------------------------------------------------------------

def test_dynamics_step_against_the_fp64_loop(robots, panda, panda_fleet):
    import torch
    engines = {}
    worst = 0.0
    for s in H.step_cases(robots):
        if s["name"] not in engines:
            engines[s["name"]] = _engine(s["t"], s["inert"], s["g"])
        eng = engines[s["name"]]
        q, qd, u = _dev(s["q"], s["qd"], s["u"])
        eng.dynamics_step(q, qd, u, DT, substeps=s["substeps"], drive="accel" if s["drive"] == FR.ACCEL else "torque", tau_limit=s["lim"])
        got_q, got_qd = _host(q), _host(qd)
        assert np.isfinite(got_q).all() and np.isfinite(got_qd).all()
        r = H.step_ratio(s, got_q, got_qd)
        worst = max(worst, r)
        assert r <= K_STEP, (s["name"], s["drive"], s["substeps"], r)
    print(f"step: worst ratio {worst:.3f} (bound {K_STEP})")
    assert len(engines) == 3
    # substeps = 3 is three calls with substeps = 1, bit for bit
    t, inert = panda
    eng = engines["panda"]
    f = panda_fleet
    lim = H.median_limits(f["tau_ref"])
    for drive, u, tl in (("accel", f["qdd"][:256], lim), ("torque", f["tau"][:256], None), ("torque", f["tau"][:256], lim)):
        q3, qd3, ug = _dev(f["q"][:256], f["qd"][:256], u)
        q1, qd1 = q3.clone(), qd3.clone()
        a3, t3, a1, t1 = (torch.empty_like(q3) for _ in range(4))
        eng.dynamics_step(q3, qd3, ug, DT, substeps=3, drive=drive, tau_limit=tl, qdd_out=a3, tau_out=t3)
        for _ in range(3):
            eng.dynamics_step(q1, qd1, ug, DT, substeps=1, drive=drive, tau_limit=tl, qdd_out=a1, tau_out=t1)
        torch.cuda.synchronize()
        for a, b in ((q3, q1), (qd3, qd1), (a3, a1), (t3, t1)):
            assert torch.equal(a, b), drive
    # a torque drive with u = inverse_dynamics(q, qd, a) lands on qd + dt a
    q, qd, a = _dev(*(f[k][:256] for k in ("q", "qd", "qdd")))
    tau = eng.inverse_dynamics(q, qd, a)
    eng.dynamics_step(q, qd, tau, DT, drive="torque")
    want_qd = f["qd"][:256].astype(np.float64) + DT * f["qdd"][:256].astype(np.float64)
    want_q = f["q"][:256].astype(np.float64) + DT * want_qd
    bq, bqd = FR.step_brackets(want_q, want_qd, f["qdd"][:256].astype(np.float64), DT, 1)
    assert (np.abs(_host(qd) - want_qd).max(1) <= K_STEP * bqd).all() and (np.abs(_host(q) - want_q).max(1) <= K_STEP * bq).all()


# ---- 7: the singular robot and poisoned rows -------------------------------------------------------------------------------

def test_singular_robot_and_non_finite_rows(panda, panda_fleet, tmp_path):
    import torch
    name, ts, inerts = H.singular_robot(tmp_path)
    eng = _engine(ts, inerts)
    q, qd, qdd = DR.random_states(np.random.default_rng(204), ts, 70)
    tau = np.ones_like(q)
    assert np.isnan(_host(eng.forward_dynamics(*_dev(q, qd, tau)))).all()
    qg, qdg, tg = _dev(q, qd, tau)
    eng.dynamics_step(qg, qdg, tg, DT, drive="torque")
    assert np.isnan(_host(qg)).all() and np.isnan(_host(qdg)).all()
    M = _host(eng.mass_matrix(*_dev(q)))                                  # the mass matrix is still returned
    _check_mass(M, FR.mass_matrix(ts, inerts, q), name)
    assert (M[:, 2, :] == 0).all()
    # one fleet with NaN / Inf planted in q, qd and tau of three robots
    t, inert = panda
    eng = _engine(t, inert)
    f = panda_fleet
    q, qd, tau = (f[k][:130].copy() for k in ("q", "qd", "tau"))
    q[5, 2], qd[70, 0], tau[129, 8] = np.nan, np.inf, np.nan
    bad = [5, 70, 129]
    good = np.setdiff1d(np.arange(130), bad)
    got = _host(eng.forward_dynamics(*_dev(q, qd, tau)))
    assert np.isnan(got[bad]).all() and np.isfinite(got[good]).all()
    _check_residual(t, inert, q[good], qd[good], got[good], tau[good], f["fd"][good], (0.0, 0.0, -9.81), "beside poisoned rows", f["br"][good])
    qg, qdg, tg = _dev(q, qd, tau)
    a, ta = torch.empty_like(qg), torch.empty_like(qg)
    eng.dynamics_step(qg, qdg, tg, DT, substeps=2, drive="torque", qdd_out=a, tau_out=ta)
    for x in (qg, qdg, a, ta):
        x = _host(x)
        assert np.isnan(x[bad]).all() and np.isfinite(x[good]).all()
    M = _host(eng.mass_matrix(*_dev(q)))
    assert np.isnan(M[5]).all() and np.isfinite(np.delete(M, 5, 0)).all()
    _check_mass(np.delete(M, 5, 0), np.delete(f["M"][:130], 5, 0), "beside a poisoned q")


# ---- 8: graph capture ----------------------------------------------------------------------------------------------------------

def _config3_inputs(R, seed):
    import torch
    from riemannian_motion_policies_amd import configs as Cf
    s = Cf.sample_panda_states(np.random.default_rng(seed), R)
    sph = Cf.sample_spheres(np.random.default_rng(seed + 1))
    return s, sph, (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))


def test_graph_capture_of_step_inverse_dynamics_and_dynamics_step_replays_bit_identically(panda):
    import torch
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    _, desc = Cf.config3()
    eng = Engine(desc, 0)
    eng.set_inertials(panda[1])
    s, sph, (q, qd, goal) = _config3_inputs(2048, 30)
    q0, qd0 = q.clone(), qd.clone()
    obs = eng.obstacles(spheres=torch.from_numpy(sph))
    lim = torch.from_numpy(U.read_effort_limits(U.PANDA_URDF, U.PANDA_ORDER)).cuda()
    side = torch.cuda.Stream()
    launch, qdd = eng.bind(q, qd, goal, obstacles=obs, stream=side.cuda_stream)
    tau, qdd_real, tau_app = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)

    def chain():
        launch()
        eng.inverse_dynamics(q, qd, qdd, out=tau)
        eng.dynamics_step(q, qd, qdd, DT, substeps=3, tau_limit=lim, qdd_out=qdd_real, tau_out=tau_app)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):   # eager, on the stream the graph is captured on
        chain()
    side.synchronize()
    eager = [x.clone() for x in (q, qd, qdd, tau, qdd_real, tau_app)]
    assert not torch.equal(q, q0) and bool(torch.isfinite(q).all())
    g = torch.cuda.CUDAGraph()
    q.copy_(q0)
    qd.copy_(qd0)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):   # one stream, no parallel branches
        chain()
    for x in (qdd, tau, qdd_real, tau_app):
        x.zero_()
    q.copy_(q0)
    qd.copy_(qd0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip((q, qd, qdd, tau, qdd_real, tau_app), eager):
        assert torch.equal(a, b)


# ---- 9: untouched neighbours -----------------------------------------------------------------------------------------------

def test_step_fk_rollout_and_inverse_dynamics_untouched(panda):
    import torch
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.engine import Engine
    _, desc = Cf.config3()
    inert = panda[1]
    s, sph, (q, qd, goal) = _config3_inputs(1024, 40)

    def run(eng):
        obs = eng.obstacles(spheres=torch.from_numpy(sph))
        step = eng.step(q, qd, goal, obstacles=obs).clone()
        fk = eng.forward_kinematics(q).clone()
        qr, qdr = q.clone(), qd.clone()
        last = eng.rollout(qr, qdr, goal, obstacles=obs, n_control_steps=2, substeps=3, dt=0.01).clone()
        tau = eng.inverse_dynamics(q, qd, step).clone()
        torch.cuda.synchronize()
        return step, fk, qr, qdr, last, tau

    fresh = Engine(desc, 0)
    fresh.set_inertials(inert)
    plain = run(fresh)
    eng = Engine(desc, 0)
    eng.set_inertials(inert)
    eng.mass_matrix(q)
    eng.forward_dynamics(q, qd, plain[5])
    qs, qds = q.clone(), qd.clone()
    eng.dynamics_step(qs, qds, plain[0], DT, substeps=2, tau_limit=np.full(9, 5.0, np.float32))
    between = run(eng)
    eng.dynamics_step(qs, qds, plain[5], DT, drive="torque")
    after = run(eng)
    for a, b, c in zip(plain, between, after):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert bool(torch.equal(q, torch.from_numpy(s["q"]).cuda()))      # (dynamics_step worked on the copies)


# ---- 10: refusals and the class surface --------------------------------------------------------------------------------------

def test_refusals(panda):
    import torch
    from riemannian_motion_policies_amd import _native
    t, inert = panda
    eng = _engine(t)
    lib, h = _native.lib(), eng._h
    q = torch.zeros((8, t.n_dof), device="cuda")
    out = torch.full_like(q, 7.0)
    M = torch.full((8, 9, 9), 7.0, device="cuda")
    p, o, m = q.data_ptr(), out.data_ptr(), M.data_ptr()
    # no inertials: each message names rmp2_set_inertials
    for rc in (lib.rmp2_mass_matrix(h, p, m, 8, None), lib.rmp2_forward_dynamics(h, p, p, p, o, 8, None),
               lib.rmp2_dynamics_step(h, p, p, p, 1, None, 0.01, 1, None, None, 8, None)):
        assert rc == -1 and b"rmp2_set_inertials" in lib.rmp2_last_error(h)
    with pytest.raises(_native.Rmp2Error, match="rmp2_set_inertials"):
        eng.forward_dynamics(q, q, q)
    eng.set_inertials(inert)
    # null pointers
    for rc in (lib.rmp2_mass_matrix(h, None, m, 8, None), lib.rmp2_mass_matrix(h, p, None, 8, None),
               lib.rmp2_forward_dynamics(h, None, p, p, o, 8, None), lib.rmp2_forward_dynamics(h, p, None, p, o, 8, None),
               lib.rmp2_forward_dynamics(h, p, p, None, o, 8, None), lib.rmp2_forward_dynamics(h, p, p, p, None, 8, None),
               lib.rmp2_dynamics_step(h, None, p, p, 1, None, 0.01, 1, None, None, 8, None),
               lib.rmp2_dynamics_step(h, p, None, p, 1, None, 0.01, 1, None, None, 8, None),
               lib.rmp2_dynamics_step(h, p, p, None, 1, None, 0.01, 1, None, None, 8, None)):
        assert rc == -1 and b"null" in lib.rmp2_last_error(h)
    # negative R, substeps < 1, a bad dt, an unknown drive
    step = lambda drive, dt, substeps, R: lib.rmp2_dynamics_step(h, p, p, p, drive, None, dt, substeps, None, None, R, None)
    for call, msg in ((lambda: lib.rmp2_mass_matrix(h, p, m, -1, None), b"mass matrix: R < 0"),
                      (lambda: lib.rmp2_forward_dynamics(h, p, p, p, o, -1, None), b"forward dynamics: R < 0"),
                      (lambda: step(1, 0.01, 1, -1), b"dynamics step: R < 0"),
                      (lambda: step(1, 0.01, 0, 8), b"substeps < 1"),
                      (lambda: step(1, 0.0, 1, 8), b"dt"),
                      (lambda: step(1, -0.01, 1, 8), b"dt"),
                      (lambda: step(1, float("nan"), 1, 8), b"dt"),
                      (lambda: step(1, float("inf"), 1, 8), b"dt"),
                      (lambda: step(2, 0.01, 1, 8), b"unknown drive 2"),
                      (lambda: step(-1, 0.01, 1, 8), b"unknown drive -1")):
        assert call() == -1 and msg in lib.rmp2_last_error(h), (msg, lib.rmp2_last_error(h))
    # R == 0 is a no-op, and no refused call wrote anything
    assert lib.rmp2_mass_matrix(h, None, None, 0, None) == 0 and lib.rmp2_forward_dynamics(h, None, None, None, None, 0, None) == 0
    assert lib.rmp2_dynamics_step(h, None, None, None, 1, None, 0.01, 1, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((M == 7.0).all()) and bool((q == 0).all())
    # the Engine's checks
    with pytest.raises(ValueError, match=r"\[R, 9\]"):
        eng.forward_dynamics(q[:, :8], q, q)
    with pytest.raises(ValueError, match=r"\[R, 9\]"):
        eng.mass_matrix(q[0])
    with pytest.raises(ValueError, match=r"\[R, 9\]"):
        eng.dynamics_step(q, q.clone(), q[:4], 0.01)
    with pytest.raises(ValueError, match="out must be"):
        eng.mass_matrix(q, out=torch.empty((8, 9), device="cuda"))
    with pytest.raises(ValueError, match="drive"):
        eng.dynamics_step(q, q.clone(), q, 0.01, drive="position")
    with pytest.raises(ValueError, match=r"tau_limit must be \[9\]"):
        eng.dynamics_step(q, q.clone(), q, 0.01, tau_limit=np.ones(8))
    with pytest.raises(ValueError, match=">= 0"):
        eng.dynamics_step(q, q.clone(), q, 0.01, tau_limit=-np.ones(9))
    with pytest.raises(ValueError, match="contiguous fp32"):
        eng.dynamics_step(q.double(), q.clone(), q, 0.01)
    with pytest.raises(_native.Rmp2Error, match="substeps"):
        eng.dynamics_step(q, q.clone(), q, 0.01, substeps=0)


def test_tau_limit_host_values_upload_once(panda, monkeypatch):
    import torch
    t, inert = panda
    eng = _engine(t, inert)
    q = torch.zeros((4, 9), device="cuda")
    lim = np.full(9, 3.0, np.float32)
    eng.dynamics_step(q.clone(), q.clone(), q, 0.01, tau_limit=lim)
    first = eng._tau_limit[1]
    eng.dynamics_step(q.clone(), q.clone(), q, 0.01, tau_limit=lim.copy())
    assert eng._tau_limit[1] is first
    eng.dynamics_step(q.clone(), q.clone(), q, 0.01, tau_limit=2 * lim)
    assert eng._tau_limit[1] is not first and bool((eng._tau_limit[1] == 6.0).all())


def test_class_surface(panda, golden_dir, tmp_path):
    import torch
    from riemannian_motion_policies_amd import urdf as U
    from riemannian_motion_policies_amd.kinematics import UrdfForwardKinematic
    t, inert = panda
    fk = UrdfForwardKinematic(U.PANDA_URDF, U.PANDA_ORDER)
    q, qd, qdd = DR.random_states(np.random.default_rng(50), t, 16)
    tau = DR.rnea(t, inert, q, qd, qdd).astype(np.float32)
    ref = FR.forward_dynamics(t, inert, q, qd, tau)
    Mref = FR.mass_matrix(t, inert, q)
    ine = fixture_inertials(golden_dir, "panda")
    host = fk.forward_dynamics(q, qd, tau, inertials=ine)                  # [R, n] host -> host
    assert isinstance(host, np.ndarray) and host.shape == (16, 9)
    _check_qdd(host, ref, "host [R, n]")
    one = fk.forward_dynamics(q[3], qd[3], tau[3], inertials=ine)          # [n] host -> [n] host
    assert isinstance(one, np.ndarray) and one.shape == (9,)
    _check_qdd(one[None], ref[3:4], "host [n]")
    dev = fk.forward_dynamics(*_dev(q, qd, tau), inertials=inert)          # a table works too
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.shape == (16, 9)
    _check_qdd(dev.cpu().numpy(), ref, "device [R, n]")
    dev1 = fk.forward_dynamics(*_dev(q[0], qd[0], tau[0]), inertials=ine)
    assert dev1.is_cuda and dev1.shape == (9,)
    g0 = fk.forward_dynamics(q, qd, tau, gravity=(0.0, 0.0, 0.0), inertials=ine)
    _check_qdd(g0, FR.forward_dynamics(t, inert, q, qd, tau, (0.0, 0.0, 0.0)), "no gravity")
    Mh = fk.mass_matrix(q, inertials=ine)
    assert isinstance(Mh, np.ndarray) and Mh.shape == (16, 9, 9)
    _check_mass(Mh, Mref, "host [R, n]")
    M1 = fk.mass_matrix(q[2], inertials=ine)
    assert M1.shape == (9, 9)
    _check_mass(M1[None], Mref[2:3], "host [n]")
    Md = fk.mass_matrix(*_dev(q), inertials=inert)
    assert Md.is_cuda and Md.shape == (16, 9, 9)
    assert fk.mass_matrix(*_dev(q[1]), inertials=ine).shape == (9, 9)
    # the package's URDF has no <inertial>: the default is a clear error
    with pytest.raises(ValueError, match="no <inertial>"):
        fk.forward_dynamics(q, qd, tau)
    with pytest.raises(ValueError, match="no <inertial>"):
        fk.mass_matrix(q)
    # a URDF that has them: read from the file by default
    path = str(tmp_path / "r.urdf")
    order = DR.random_urdf(np.random.default_rng(51), path, 6, massless=0.0)
    fk2 = UrdfForwardKinematic(path, order)
    t2 = fk2.table
    i2 = U.inertial_table(t2, U.read_inertials(path))
    q2, qd2, qdd2 = DR.random_states(np.random.default_rng(52), t2, 8)
    tau2 = DR.rnea(t2, i2, q2, qd2, qdd2).astype(np.float32)
    got = fk2.forward_dynamics(q2, qd2, tau2)
    _check_residual(t2, i2, q2, qd2, got, tau2, FR.forward_dynamics(t2, i2, q2, qd2, tau2), (0.0, 0.0, -9.81), "from the file")
    _check_mass(fk2.mass_matrix(q2), FR.mass_matrix(t2, i2, q2), "from the file")

"""Obstacle contacts on the GPU (include/rmp2.h rmp2_dynamics_step_contacts, Engine.dynamics_step(contacts=...)) against the fp64
restatement of tests/contacts_reference.py: Panda (N = 9) and the two-joint robot (N = 2), both drives; fleets of 1, 65 and 1024
robots (one lane, one wave plus a lane, several waves); tables of 1, 16 and 33 spheres; 1 and 4 substeps; the fast path bit for
bit; NaN containment; refusals; a graph capture of policy step + contact step.

The bounds were fixed before the first GPU run, from the fp32 envelope restatement measured on the CPU
(tests/test_contacts_host.py; K = 4 x the envelope's worst ratio, rounded up to one significant figure), per robot:
    stationarity  max_j |rnea64(q, qd, qdd_dev) - tau_applied - stop_dev - contact_dev|_j <= K_RES x residual_bracket,  K_RES = 0.3 (envelope 0.0537)
    velocity      max_j |v_dev - v_ref|_j <= K_VEL x velocity_bracket,                                                  K_VEL = 50  (envelope 10.29)
    force         max_j |(stop + contact)_dev - (stop + contact)_ref|_j <= K_FORCE x force_bracket,                     K_FORCE = 20 (envelope 4.018)
    the step      |q_dev - q_ref|, |qd_dev - qd_ref| <= K_STEP x step_brackets,                                         K_STEP = 70 (envelope 16.0)
    gap           KKT from the device's own contact_pair / contact_lambda, rows rebuilt in fp64: K_GAP x gap_bracket,   K_GAP = 0.5 (envelope 0.1174)
The device routine run on the CPU sits within half of each (worst ratios 0.083, 10.29, 4.68, 16.0, 0.117)."""
import numpy as np
import pytest

import contacts_reference as CR
import forward_dynamics_reference as FR
import joint_stops_reference as JR
import test_contacts_host as S
from test_contacts_host import D_ACT, DT, K_FORCE, K_RES, K_STEP, K_VEL, WORST_ITERS

pytestmark = pytest.mark.gpu


def _engine(c, capsules=True):
    from riemannian_motion_policies_amd import descriptor as D
    from riemannian_motion_policies_amd.engine import Engine
    eng = Engine(D.build_desc(c["t"], []), 0)
    eng.set_inertials(c["inert"], gravity=c["g"])
    if capsules:
        eng.set_contact_capsules(c["caps"])
    return eng


def _dev(*xs):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in xs)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _drive(c):
    return "accel" if c["drive"] == FR.ACCEL else "torque"


def _step(eng, c, substeps=1, spheres=None, limits="case", q=None, qd=None, u=None, d_act=D_ACT):
    """dict(q, qd, qdd, tau, stop, contact, lam, pair, status) of the contact step on the case (fields replaced by the keywords)."""
    import torch
    q, qd, u = _dev(c["q"] if q is None else q, c["qd"] if qd is None else qd, c["u"] if u is None else u)
    (sph,) = _dev((c["spheres"] if spheres is None else spheres).reshape(-1, 4))
    R = len(q)
    qdd, tau, stop, cont = torch.empty_like(q), torch.empty_like(q), torch.full_like(q, 7.0), torch.full_like(q, 7.0)
    lam = torch.full((R, 8), 7.0, device=q.device)
    pair = torch.full((R, 8), 5, dtype=torch.int32, device=q.device)
    status = torch.full((R,), -1, dtype=torch.int32, device=q.device)
    eng.dynamics_step(q, qd, u, DT, substeps=substeps, drive=_drive(c), tau_limit=c["lim"], qdd_out=qdd, tau_out=tau,
                      q_limits=c["limits"] if limits == "case" else limits, stop_out=stop, status_out=status, contacts=sph,
                      d_act=d_act, contact_out=cont, contact_lambda_out=lam, contact_pair_out=pair)
    return dict(q=_host(q), qd=_host(qd), qdd=_host(qdd), tau=_host(tau), stop=_host(stop), contact=_host(cont), lam=_host(lam),
                pair=_host(pair), status=_host(status).view(np.uint32))


def _plain(eng, c, substeps=1, limits=None):
    """(q, qd, qdd, tau[, stop, status]) tensors of the existing entry points on the case."""
    import torch
    q, qd, u = _dev(c["q"], c["qd"], c["u"])
    qdd, tau = torch.empty_like(q), torch.empty_like(q)
    if limits is None:
        eng.dynamics_step(q, qd, u, DT, substeps=substeps, drive=_drive(c), tau_limit=c["lim"], qdd_out=qdd, tau_out=tau)
        return dict(q=_host(q), qd=_host(qd), qdd=_host(qdd), tau=_host(tau))
    stop = torch.empty_like(q)
    status = torch.zeros(len(q), dtype=torch.int32, device=q.device)
    eng.dynamics_step(q, qd, u, DT, substeps=substeps, drive=_drive(c), tau_limit=c["lim"], qdd_out=qdd, tau_out=tau, q_limits=limits,
                      stop_out=stop, status_out=status)
    return dict(q=_host(q), qd=_host(qd), qdd=_host(qdd), tau=_host(tau), stop=_host(stop), status=_host(status).view(np.uint32))


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def fleets(golden_dir):
    return S.gpu_cases(golden_dir)


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(c):
        if c["name"] not in cache:
            cache[c["name"]] = _engine(c)
        return cache[c["name"]]
    return get


def _ids(c):
    return f"{c['name']}-{'accel' if c['drive'] == FR.ACCEL else 'torque'}-R{c['R']}-K{c['K']}-s{c['substeps']}"


def test_against_the_reference_across_fleet_and_table_sizes(fleets, engines):
    """Velocity, total constraint torque, stationarity and the device's own KKT conditions after one substep; q and qd after
    four."""
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0)
    strong = 0
    for c in fleets:
        d = _step(engines(c), c, substeps=c["substeps"])
        S.flags_agree(c, d["status"])
        if c["substeps"] == 1:
            res, vel, force, _ = S.one_step_ratios(c, d)
            print(_ids(c), "stationarity %.3g velocity %.3g force %.3g" % (res, vel, force))
            worst.update(res=max(worst["res"], res), vel=max(worst["vel"], vel), force=max(worst["force"], force))
            strong += S.check_device_kkt(c, d, _ids(c))
            assert ((d["status"] >> 8) <= 2 * WORST_ITERS).all()
        else:
            step = S.step_ratio(c, d)
            print(_ids(c), "step %.3g" % step)
            worst["step"] = max(worst["step"], step)
    print("worst ratios on the device", worst, "strong contacts", strong)
    assert strong >= 500
    assert worst["res"] <= K_RES and worst["vel"] <= K_VEL and worst["force"] <= K_FORCE and worst["step"] <= K_STEP, worst


def test_fast_path_bit_for_bit(fleets, engines):
    """Table far away (and K = 0): torch.equal with dynamics_step(q_limits=); limits far too, or absent: with the plain step; in
    the mixed fleets the robots without a candidate equal the stops' step."""
    far = np.array([[30.0, 20.0, 10.0, 0.1], [-30.0, 5.0, 2.0, 0.2]], np.float32)
    for c in fleets:
        if c["R"] == 1024:
            continue
        eng = engines(c)
        n = c["t"].n_dof
        sub = c["substeps"]
        s = _plain(eng, c, sub, c["limits"])
        for table in (far, np.zeros((0, 4), np.float32)):
            d = _step(eng, c, substeps=sub, spheres=table)
            for k in ("q", "qd", "qdd", "tau", "stop"):
                assert _bits(d[k], s[k]), (_ids(c), k)
            assert (d["status"] == s["status"]).all() and (d["contact"] == 0).all() and (d["lam"] == 0).all() and (d["pair"] == -1).all()
        p = _plain(eng, c, sub)
        for lim_ in ((np.full(n, -1e6, np.float32), np.full(n, 1e6, np.float32)), None):
            d = _step(eng, c, substeps=sub, spheres=far, limits=lim_)
            for k in ("q", "qd", "qdd", "tau"):
                assert _bits(d[k], p[k]), (_ids(c), k)
            assert (d["status"] == 0).all() and (d["stop"] == 0).all()
    seen = 0
    for c in fleets:            # the mixed fleets
        d = _step(engines(c), c, substeps=c["substeps"])
        s = _plain(engines(c), c, c["substeps"], c["limits"])
        clear = ~c["ref"]["any_cand"]
        seen += int(clear.sum())
        for k in ("q", "qd", "qdd", "tau", "stop"):
            assert _bits(d[k][clear], s[k][clear]), (_ids(c), k)
        assert (d["pair"][clear] == -1).all() and (d["lam"][clear] == 0).all() and (d["contact"][clear] == 0).all()
        assert (d["status"][clear] == s["status"][clear]).all()
    assert seen >= 500


def test_nan_rows_are_contained_and_a_nan_table_poisons_every_robot(fleets, engines):
    for name in ("panda", "two_joint"):
        c = next(c for c in fleets if c["name"] == name and c["R"] == 65 and c["substeps"] == 1)
        eng = engines(c)
        good = _step(eng, c)
        q, qd, u = c["q"].copy(), c["qd"].copy(), c["u"].copy()
        q[2, 1], qd[63, 0], u[64, 1] = np.nan, np.inf, -np.inf
        bad = np.zeros(65, bool)
        bad[[2, 63, 64]] = True
        d = _step(eng, c, q=q, qd=qd, u=u)
        for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
            assert np.isnan(d[k][bad]).all() and _bits(d[k][~bad], good[k][~bad]), (name, k)
        assert (d["pair"][bad] == -1).all() and np.array_equal(d["pair"][~bad], good["pair"][~bad])
        table = c["spheres"].copy()
        table[5, 2] = np.inf
        d = _step(eng, c, spheres=table)
        for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
            assert np.isnan(d[k]).all(), (name, k)


def test_refusals(fleets):
    import torch
    from riemannian_motion_policies_amd import _native
    c = next(c for c in fleets if c["name"] == "panda" and c["R"] == 65)
    eng = _engine(c)
    q, qd, u = (torch.zeros((4, 9), device="cuda") for _ in range(3))
    sph = torch.zeros((3, 4), device="cuda")
    with pytest.raises(_native.Rmp2Error, match="d_act"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, d_act=-0.1)
    with pytest.raises(_native.Rmp2Error, match="d_act"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, d_act=float("nan"))
    with pytest.raises(_native.Rmp2Error, match="K > 256"):
        eng.dynamics_step(q, qd, u, DT, contacts=torch.zeros((257, 4), device="cuda"), d_act=0.01)
    with pytest.raises(_native.Rmp2Error, match="substeps"):
        eng.dynamics_step(q, qd, u, DT, substeps=0, contacts=sph, d_act=0.01)
    with pytest.raises(_native.Rmp2Error, match="dt must be"):
        eng.dynamics_step(q, qd, u, float("inf"), contacts=sph, d_act=0.01)
    with pytest.raises(ValueError, match=r"\[K, 4\]"):
        eng.dynamics_step(q, qd, u, DT, contacts=torch.zeros((3, 8), device="cuda"), d_act=0.01)
    with pytest.raises(ValueError, match="contacts must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=torch.zeros((3, 4)), d_act=0.01)
    with pytest.raises(ValueError, match="need contacts"):
        eng.dynamics_step(q, qd, u, DT, contact_out=torch.zeros((4, 9), device="cuda"))
    with pytest.raises(ValueError, match="contact_pair_out"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, d_act=0.01, contact_pair_out=torch.zeros((4, 8), device="cuda"))
    with pytest.raises(ValueError, match="contact_lambda_out must be"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, d_act=0.01, contact_lambda_out=torch.zeros((4, 9), device="cuda"))
    with pytest.raises(_native.Rmp2Error, match="one record per frame"):
        eng.set_contact_capsules(c["caps"][:5])
    bare = _engine(c, capsules=False)
    with pytest.raises(_native.Rmp2Error, match="rmp2_set_contact_capsules"):
        bare.dynamics_step(q, qd, u, DT, contacts=sph, d_act=0.01)
    eng.set_contact_capsules(None)                                              # off again
    with pytest.raises(_native.Rmp2Error, match="rmp2_set_contact_capsules"):
        eng.dynamics_step(q, qd, u, DT, contacts=sph, d_act=0.01)
    assert bool((q == 0).all())                                                 # nothing ran


def test_sixteen_dof_robot_is_refused_as_unsupported(tmp_path):
    import torch
    import dynamics_reference as DR
    from riemannian_motion_policies_amd import _native, descriptor as D, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    path = str(tmp_path / "dof16.urdf")
    order = DR.random_urdf(np.random.default_rng(3), path, 16, n_dof=16, chain=True, massless=0.0, prismatic=0.0, fixed=0.0)
    t = U.compile_urdf(path, order)
    assert t.n_dof == 16
    eng = Engine(D.build_desc(t, []), 0)
    eng.set_inertials(U.inertial_table(t, U.read_inertials(path)))
    caps = np.zeros((t.n_frames, 8), np.float32)
    caps[:, 3] = 0.05
    eng.set_contact_capsules(caps)
    q, qd, u = (torch.zeros((2, 16), device="cuda") for _ in range(3))
    with pytest.raises(_native.Rmp2Error, match="more than 9 dofs"):
        eng.dynamics_step(q, qd, u, DT, contacts=torch.zeros((1, 4), device="cuda"), d_act=0.01)


def test_graph_capture_of_policy_step_and_contact_step_replays_twice(golden_dir):
    """The experiment loop's body -- the policy's step, then the plant's step with stops and contacts on the table the policy
    avoids -- captured once and replayed twice from the same state: the bytes of the eager run."""
    import torch
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    from test_inverse_dynamics_host import reference_robots
    _, desc = Cf.config3()
    eng = Engine(desc, 0)
    t = U.panda_table()
    eng.set_inertials(next(i for n, _, i in reference_robots(golden_dir) if n == "panda"))
    eng.set_contact_capsules(U.contact_capsules(U.PANDA_URDF, t))
    s = Cf.sample_panda_states(np.random.default_rng(40), 512)
    sph = torch.from_numpy(Cf.sample_spheres(np.random.default_rng(41))).cuda().contiguous()
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    q0, qd0 = q.clone(), qd.clone()
    obs = eng.obstacles(spheres=sph)
    lim = torch.from_numpy(U.read_effort_limits(U.PANDA_URDF, U.PANDA_ORDER)).cuda()
    lo, hi = (torch.from_numpy(x).cuda() for x in U.read_joint_limits(U.PANDA_URDF, U.PANDA_ORDER))
    side = torch.cuda.Stream()
    launch, qdd = eng.bind(q, qd, goal, obstacles=obs, stream=side.cuda_stream)
    outs = [torch.empty_like(q) for _ in range(4)]
    lam = torch.empty((512, 8), device="cuda")
    pair = torch.empty((512, 8), dtype=torch.int32, device="cuda")
    status = torch.empty(512, dtype=torch.int32, device="cuda")

    def chain():
        launch()
        eng.dynamics_step(q, qd, qdd, DT, substeps=3, tau_limit=lim, qdd_out=outs[0], tau_out=outs[1], q_limits=(lo, hi),
                          stop_out=outs[2], status_out=status, contacts=sph[:, :4], d_act=0.05, contact_out=outs[3],
                          contact_lambda_out=lam, contact_pair_out=pair)

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        chain()
    side.synchronize()
    everything = (q, qd, qdd, *outs, lam, pair, status)
    eager = [x.clone() for x in everything]
    assert not torch.equal(q, q0) and bool(torch.isfinite(q).all())
    g = torch.cuda.CUDAGraph()
    q.copy_(q0)
    qd.copy_(qd0)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):   # one stream, no parallel branches
        chain()
    for _ in range(2):
        for x in (*outs, lam, pair, status):
            x.zero_()
        q.copy_(q0)
        qd.copy_(qd0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(everything, eager):
            assert torch.equal(a, b)

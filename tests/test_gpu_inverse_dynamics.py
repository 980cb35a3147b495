"""Inverse dynamics on the GPU (include/rmp2.h rmp2_set_inertials / rmp2_inverse_dynamics) against the fp64 Newton-Euler
restatement (tests/dynamics_reference.py): the reference robots across fleet sizes, random trees, the chain behind rmp2_step's
own qdd, graph capture, switching, untouched control steps, refusals and the class surface.

The bound was fixed before the first run: per robot, max_j |tau_dev - tau_ref| <= 1e-4 + 1e-5 max_j |tau_ref| (N m or N)."""
import ctypes as C
import os

import numpy as np
import pytest

import dynamics_reference as DR
from test_inverse_dynamics_host import fixture_inertials, random_robots, within_gpu_bound

pytestmark = pytest.mark.gpu


def _engine(table):
    from riemannian_motion_policies_amd import descriptor as D
    from riemannian_motion_policies_amd.engine import Engine
    return Engine(D.build_desc(table, []), 0)


def _panda(golden_dir):
    from riemannian_motion_policies_amd import urdf as U
    t = U.panda_table()
    return t, U.inertial_table(t, fixture_inertials(golden_dir, "panda"))


def _check(t, inert, eng, q, qd, qdd, what, gravity=(0.0, 0.0, -9.81)):
    import torch
    tau = eng.inverse_dynamics(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (q, qd, qdd)))
    torch.cuda.synchronize()
    dev = tau.cpu().numpy()
    ref = DR.rnea(t, inert, q, qd, qdd, gravity)
    ok = within_gpu_bound(dev, ref)
    assert ok.all(), (what, int((~ok).sum()), float(np.abs(dev - ref).max()))
    return dev, ref


def test_panda_across_fleet_sizes(golden_dir):
    t, inert = _panda(golden_dir)
    eng = _engine(t)
    eng.set_inertials(inert)
    rng = np.random.default_rng(10)
    for R in (1, 63, 64, 65, 4097, 65536):
        q, qd, qdd = DR.random_states(rng, t, R)   # q across the joint limits, |qd| <= 2, |qdd| <= 10
        dev, ref = _check(t, inert, eng, q, qd, qdd, f"panda R={R}")
        if R == 65536:
            assert np.abs(ref).max() > 20.0


def test_two_joint_robot_and_gravity(golden_dir):
    from riemannian_motion_policies_amd import urdf as U
    t = U.two_joint_table()
    inert = U.inertial_table(t, fixture_inertials(golden_dir, "two_joint"))
    eng = _engine(t)
    rng = np.random.default_rng(11)
    q, qd, qdd = DR.random_states(rng, t, 1000)
    for g in ((0.0, 0.0, -9.81), (0.0, -9.81, 0.0), (0.0, 0.0, 0.0)):
        eng.set_inertials(inert, gravity=g)
        _check(t, inert, eng, q, qd, qdd, f"two_joint g={g}", gravity=g)


def test_random_trees(tmp_path):
    rng = np.random.default_rng(12)
    robots = random_robots(tmp_path, seed=3)
    assert any(t.n_frames == 32 for _, t, _ in robots) and any(t.n_dof == 16 for _, t, _ in robots)
    for name, t, inert in robots:
        eng = _engine(t)
        eng.set_inertials(inert, gravity=(0.5, -1.0, -9.81))
        q, qd, qdd = DR.random_states(rng, t, 1000)
        _check(t, inert, eng, q, qd, qdd, name, gravity=(0.5, -1.0, -9.81))
        eng.close()


def test_non_finite_input_poisons_only_its_robot(golden_dir):
    t, inert = _panda(golden_dir)
    eng = _engine(t)
    eng.set_inertials(inert)
    q, qd, qdd = DR.random_states(np.random.default_rng(13), t, 130)
    q[5, 2], qd[70, 0], qdd[129, 8] = np.nan, np.inf, np.nan
    import torch
    dev = eng.inverse_dynamics(*(torch.from_numpy(x).cuda() for x in (q, qd, qdd))).cpu().numpy()
    bad = [5, 70, 129]
    assert not np.isfinite(dev[bad]).all(axis=1).any()
    good = np.setdiff1d(np.arange(130), bad)
    assert np.isfinite(dev[good]).all()
    assert within_gpu_bound(dev[good], DR.rnea(t, inert, q[good], qd[good], qdd[good])).all()


def _config3_inputs(R, seed):
    import torch
    from riemannian_motion_policies_amd import configs as Cf
    s = Cf.sample_panda_states(np.random.default_rng(seed), R)
    sph = Cf.sample_spheres(np.random.default_rng(seed + 1))
    return s, sph, (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))


def test_on_the_steps_own_qdd_chained_on_one_stream(golden_dir):
    import torch
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.engine import Engine
    table, desc = Cf.config3()
    inert = _panda(golden_dir)[1]
    eng = Engine(desc, 0)
    eng.set_inertials(inert)
    s, sph, (q, qd, goal) = _config3_inputs(4096, 20)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        qdd = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=torch.from_numpy(sph)))
        tau = eng.inverse_dynamics(q, qd, qdd)
    torch.cuda.synchronize()
    qdd_h = qdd.cpu().numpy()
    assert np.isfinite(qdd_h).all()
    ref = DR.rnea(table, inert, s["q"], s["qd"], qdd_h)
    assert within_gpu_bound(tau.cpu().numpy(), ref).all()


def test_graph_capture_of_step_and_inverse_dynamics_replays_bit_identically(golden_dir):
    import torch
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.engine import Engine
    _, desc = Cf.config3()
    eng = Engine(desc, 0)
    eng.set_inertials(_panda(golden_dir)[1])
    s, sph, (q, qd, goal) = _config3_inputs(2048, 30)
    obs = eng.obstacles(spheres=torch.from_numpy(sph))
    side = torch.cuda.Stream()
    launch, qdd = eng.bind(q, qd, goal, obstacles=obs, stream=side.cuda_stream)
    tau = torch.empty_like(q)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):   # eager, on the stream the graph is captured on
        launch()
        eng.inverse_dynamics(q, qd, qdd, out=tau)
    side.synchronize()
    qdd_eager, tau_eager = qdd.clone(), tau.clone()
    qdd.zero_()
    tau.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):   # one stream, no parallel branches
        launch()
        eng.inverse_dynamics(q, qd, qdd, out=tau)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(qdd, qdd_eager) and torch.equal(tau, tau_eager)
    assert bool(torch.isfinite(tau).all())


def test_switching_off_refuses_again(golden_dir):
    import torch
    from riemannian_motion_policies_amd import _native
    t, inert = _panda(golden_dir)
    eng = _engine(t)
    q = torch.zeros((4, t.n_dof), device="cuda")
    with pytest.raises(_native.Rmp2Error, match="rmp2_set_inertials"):
        eng.inverse_dynamics(q, q, q)
    eng.set_inertials(inert)
    assert eng.has_inertials
    eng.inverse_dynamics(q, q, q)
    eng.set_inertials(None)
    assert not eng.has_inertials
    with pytest.raises(_native.Rmp2Error, match="rmp2_set_inertials"):
        eng.inverse_dynamics(q, q, q)
    eng.set_inertials(inert)   # and on again
    torch.cuda.synchronize()
    assert torch.isfinite(eng.inverse_dynamics(q, q, q)).all()


def test_control_steps_fk_and_rollout_untouched_by_the_table(golden_dir):
    import torch
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.engine import Engine
    _, desc = Cf.config3()
    inert = _panda(golden_dir)[1]
    s, sph, (q, qd, goal) = _config3_inputs(1024, 40)

    def run(eng):
        obs = eng.obstacles(spheres=torch.from_numpy(sph))
        step = eng.step(q, qd, goal, obstacles=obs).clone()
        fk = eng.forward_kinematics(q).clone()
        qr, qdr = q.clone(), qd.clone()
        last = eng.rollout(qr, qdr, goal, obstacles=obs, n_control_steps=2, substeps=3, dt=0.01).clone()
        torch.cuda.synchronize()
        return step, fk, qr, qdr, last

    plain = run(Engine(desc, 0))
    eng = Engine(desc, 0)
    eng.set_inertials(inert)
    with_table = run(eng)
    eng.inverse_dynamics(q, qd, torch.zeros_like(q))
    after = run(eng)
    for a, b, c in zip(plain, with_table, after):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_refusals(golden_dir):
    import torch
    from riemannian_motion_policies_amd import _native
    t, inert = _panda(golden_dir)
    eng = _engine(t)
    lib, h = _native.lib(), eng._h
    q = torch.zeros((8, t.n_dof), device="cuda")
    tau = torch.empty_like(q)
    # no inertials
    assert lib.rmp2_inverse_dynamics(h, q.data_ptr(), q.data_ptr(), q.data_ptr(), tau.data_ptr(), 8, None) == -1
    assert b"rmp2_set_inertials" in lib.rmp2_last_error(h)
    # the table's checks, each naming the frame
    ok = np.ascontiguousarray(inert, np.float32)
    assert lib.rmp2_set_inertials(h, t.n_frames - 1, ok.ctypes.data, None) == -1
    assert b"one record per frame" in lib.rmp2_last_error(h)
    assert lib.rmp2_set_inertials(h, t.n_frames, None, None) == -1
    for f, k, v, msg in ((3, 0, -1.0, b"frame 3: mass < 0"), (5, 5, -0.1, b"frame 5: Iyy < 0"), (2, 1, np.nan, b"frame 2: cx"),
                         (7, 9, np.inf, b"frame 7: Iyz")):
        bad = ok.copy()
        bad[f, k] = v
        assert lib.rmp2_set_inertials(h, t.n_frames, bad.ctypes.data, None) == -1, msg
        assert msg in lib.rmp2_last_error(h), (msg, lib.rmp2_last_error(h))
    nan_g = np.array([0.0, np.nan, -9.81], np.float32)
    assert lib.rmp2_set_inertials(h, t.n_frames, ok.ctypes.data, nan_g.ctypes.data) == -1
    assert lib.rmp2_set_inertials(h, -1, ok.ctypes.data, None) == -1
    # refused calls left the feature off
    assert lib.rmp2_inverse_dynamics(h, q.data_ptr(), q.data_ptr(), q.data_ptr(), tau.data_ptr(), 8, None) == -1
    assert lib.rmp2_set_inertials(h, t.n_frames, ok.ctypes.data, None) == 0
    # null pointers, negative R; R == 0 is a no-op
    for args in ((None, q.data_ptr(), q.data_ptr(), tau.data_ptr()), (q.data_ptr(), None, q.data_ptr(), tau.data_ptr()),
                 (q.data_ptr(), q.data_ptr(), None, tau.data_ptr()), (q.data_ptr(), q.data_ptr(), q.data_ptr(), None)):
        assert lib.rmp2_inverse_dynamics(h, *args, 8, None) == -1
        assert b"null" in lib.rmp2_last_error(h)
    assert lib.rmp2_inverse_dynamics(h, q.data_ptr(), q.data_ptr(), q.data_ptr(), tau.data_ptr(), -1, None) == -1
    tau.fill_(7.0)
    assert lib.rmp2_inverse_dynamics(h, None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((tau == 7.0).all())
    # the Engine's shape checks
    with pytest.raises(ValueError, match=r"\[R, 9\]"):
        eng.inverse_dynamics(q[:, :8], q, q)
    with pytest.raises(ValueError, match=r"\[n_frames, 10\]"):
        eng.set_inertials(np.zeros((t.n_frames, 9)))


def test_set_inertials_skips_an_unchanged_table(golden_dir, monkeypatch):
    t, inert = _panda(golden_dir)
    eng = _engine(t)
    calls = []
    real = eng._lib

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "rmp2_set_inertials":
                return fn
            return lambda *a: calls.append(a) or fn(*a)

    monkeypatch.setattr(eng, "_lib", Spy())
    eng.set_inertials(inert)
    eng.set_inertials(inert.copy())
    assert len(calls) == 1
    eng.set_inertials(inert, gravity=(0.0, 0.0, -1.0))
    assert len(calls) == 2


def test_class_surface(golden_dir, tmp_path):
    import torch
    from riemannian_motion_policies_amd import urdf as U
    from riemannian_motion_policies_amd.kinematics import UrdfForwardKinematic
    t, inert = _panda(golden_dir)
    fk = UrdfForwardKinematic(U.PANDA_URDF, U.PANDA_ORDER)
    q, qd, qdd = DR.random_states(np.random.default_rng(50), t, 16)
    ref = DR.rnea(t, inert, q, qd, qdd)
    ine = fixture_inertials(golden_dir, "panda")
    host = fk.inverse_dynamics(q, qd, qdd, inertials=ine)                  # [R, n] host -> host
    assert isinstance(host, np.ndarray) and host.shape == (16, 9) and within_gpu_bound(host, ref).all()
    one = fk.inverse_dynamics(q[3], qd[3], qdd[3], inertials=ine)          # [n] host -> [n] host
    assert isinstance(one, np.ndarray) and one.shape == (9,) and within_gpu_bound(one[None], ref[3:4]).all()
    dev = fk.inverse_dynamics(*(torch.from_numpy(x).cuda() for x in (q, qd, qdd)), inertials=inert)   # a table works too
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.shape == (16, 9)
    assert within_gpu_bound(dev.cpu().numpy(), ref).all()
    dev1 = fk.inverse_dynamics(*(torch.from_numpy(x[0]).cuda() for x in (q, qd, qdd)), inertials=ine)
    assert dev1.is_cuda and dev1.shape == (9,)
    g = fk.inverse_dynamics(q, qd, qdd, gravity=(0.0, 0.0, 0.0), inertials=ine)
    assert within_gpu_bound(g, DR.rnea(t, inert, q, qd, qdd, (0.0, 0.0, 0.0))).all()
    # the package's URDF has no <inertial>: the default is a clear error
    with pytest.raises(ValueError, match="no <inertial>"):
        fk.inverse_dynamics(q, qd, qdd)
    # a URDF that has them: read from the file by default
    path = str(tmp_path / "r.urdf")
    order = DR.random_urdf(np.random.default_rng(51), path, 6)
    fk2 = UrdfForwardKinematic(path, order)
    t2 = fk2.table
    q2, qd2, qdd2 = DR.random_states(np.random.default_rng(52), t2, 8)
    got = fk2.inverse_dynamics(q2, qd2, qdd2)
    assert within_gpu_bound(got, DR.rnea(t2, U.inertial_table(t2, U.read_inertials(path)), q2, qd2, qdd2)).all()

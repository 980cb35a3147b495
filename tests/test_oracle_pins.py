"""Pins of the CPU oracle (oracle/rmp2_oracle.c).  The reference path cannot run here
(TensorFlow/PyBullet absent, no golden vectors for qdd in the reference) -> the oracle is
"parity unpinned" against TensorFlow and is pinned instead by:
  * the committed golden vectors from the autograd-faithful PyTorch restatement,
  * SciPy rotation known answers (the reference's own SciPy-only tests, tests/test_kinematic_forwards.py:16-85),
  * the closed-form planar two-link arm, Panda FK known answers,
  * fp64 central finite differences of the fp64 oracle build for J and c = Jdot qd,
  * numpy.linalg.pinv with TensorFlow's rcond for the resolve step.
"""
import os

import numpy as np
import pytest

import oracle as O
from riemannian_motion_policies_amd import configs as Cf
from riemannian_motion_policies_amd import descriptor as D

ATOL = 1e-5


def _check(got, ref, what):
    err = np.abs(got - ref).max(axis=-1)
    tol = ATOL * np.maximum(1.0, np.abs(ref).max(axis=-1))
    assert (err <= tol).all(), f"{what}: worst {err.max():.3e}"


def test_golden_config1(golden_dir):
    g = np.load(os.path.join(golden_dir, "config1.npz"))
    _, d = Cf.config1()
    r = O.step(d, g["q"], g["qd"], g["goal"])
    assert np.abs(r["M"] - g["M"]).max() < 1e-6 and np.abs(r["f"] - g["f"]).max() < 1e-6
    assert r["status"][0] & D.STATUS_RANK_DROP  # exactly rank-1 start pose q = [0, 0] (quirk Q3)
    _check(r["qdd64"], g["qdd"], "config1")


def test_golden_config2(golden_dir):
    g = np.load(os.path.join(golden_dir, "config2.npz"))
    _, d = Cf.config2()
    r = O.step(d, g["q"], g["qd"], g["goal"])
    assert np.abs(r["M"] - g["M"]).max() < 1e-6 and np.abs(r["f"] - g["f"]).max() < 1e-6
    # the joint-limit band is exercised: the combined metric is visibly non-symmetric (quirk Q2)
    assert max(np.abs(m - m.T).max() for m in g["M"]) > 1e-3
    _check(r["qdd64"], g["qdd"], "config2")
    T = O.forward_kinematics(d, g["q"][:16])
    assert np.abs(T - g["fk_T"]).max() < 1e-6
    for fr in (3, 9, 11):
        x, xd, J, c = O.differentiate(d, g["q"][:16], g["qd"][:16], fr)
        for name, v in (("x", x), ("xd", xd), ("J", J), ("c", c)):
            assert np.abs(v - g[f"diff{fr}_{name}"]).max() < 1e-6, (fr, name)


def test_golden_config3_pairs_and_spheres(golden_dir):
    g = np.load(os.path.join(golden_dir, "config3.npz"))
    _, d = Cf.config3()
    pl, po = Cf.pairs_from_spheres(g["origins"], g["spheres"])
    rb = O.step(d, g["q"], g["qd"], g["goal"], p_link=pl, p_obs=po)        # reference-faithful interface
    _check(rb["qdd64"], g["qdd"], "config3 explicit pairs")
    ra = O.step(d, g["q"], g["qd"], g["goal"], spheres=g["spheres"])       # shared-sphere interface
    _check(ra["qdd64"], g["qdd"], "config3 spheres")


def test_golden_config5_ragged(golden_dir):
    g = np.load(os.path.join(golden_dir, "config5.npz"))
    for key, (_, d) in (("tj", Cf.config5_two_joint()), ("pd", Cf.config3())):
        r = O.step(d, g[f"{key}_q"], g[f"{key}_qd"], g[f"{key}_goal"], spheres=g[f"{key}_spheres"],
                   csr_offset=g[f"{key}_csr_offset"], csr_index=g[f"{key}_csr_index"])
        _check(r["qdd64"], g[f"{key}_qdd"], f"config5 {key}")
        off = g[f"{key}_csr_offset"]
        assert off[1] == off[0] and off[2] - off[1] == len(g[f"{key}_spheres"])  # k_r = 0 and k_r = K edge cases


def test_rotations_vs_scipy():
    """Single revolute joint about x / y / z / a skew axis: FK rotation == SciPy from_rotvec
    (restates tests/test_kinematic_forwards.py:16-37,61-85, tolerance 1e-6)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], list(np.array([1.0, 2.0, -2.0]) / 3.0)):
        d = D.Desc()
        d.abi_version, d.n_leaves = D.ABI_VERSION, 0
        d.robot.n_frames, d.robot.n_dof = 1, 1
        d.robot.parent[0], d.robot.joint_type[0], d.robot.q_index[0] = -1, 1, 0
        for k in range(3):
            d.robot.axis[0][k] = axis[k]
        for k, v in enumerate([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]):
            d.robot.T_const[0][k] = v
        ang = rng.uniform(0, 2 * np.pi, 8).astype(np.float32)
        T = O.forward_kinematics(d, ang[:, None])
        want = Rotation.from_rotvec(ang[:, None].astype(np.float64) * np.asarray(axis)[None]).as_matrix()
        assert np.abs(T[:, 0, :3, :3] - want).max() < 1e-6


def test_two_link_closed_form():
    """link_23 origin of the planar arm: x = c1 + c12, y = s1 + s12, z = 0.125; analytic J and Jdot qd."""
    _, d = Cf.config1()
    rng = np.random.default_rng(1)
    q = rng.uniform(-np.pi, np.pi, (32, 2)).astype(np.float32)
    qd = rng.uniform(-1, 1, (32, 2)).astype(np.float32)
    x, xd, J, c = O.differentiate(d, q, qd, 2, "f64")
    q1, q12 = q[:, 0].astype(np.float64), (q[:, 0].astype(np.float64) + q[:, 1])
    w1, w12 = qd[:, 0].astype(np.float64), (qd[:, 0].astype(np.float64) + qd[:, 1])
    assert np.abs(x[:, 3] - (np.cos(q1) + np.cos(q12))).max() < 1e-12
    assert np.abs(x[:, 7] - (np.sin(q1) + np.sin(q12))).max() < 1e-12
    assert np.abs(x[:, 11] - 0.125).max() < 1e-8  # 0.075 + 0.05 from the fp32 table
    assert np.abs(J[:, 3, 0] - (-np.sin(q1) - np.sin(q12))).max() < 1e-12
    assert np.abs(J[:, 3, 1] - (-np.sin(q12))).max() < 1e-12
    assert np.abs(J[:, 7, 0] - (np.cos(q1) + np.cos(q12))).max() < 1e-12
    assert np.abs(c[:, 3] - (-np.cos(q1) * w1 ** 2 - np.cos(q12) * w12 ** 2)).max() < 1e-12
    assert np.abs(c[:, 7] - (-np.sin(q1) * w1 ** 2 - np.sin(q12) * w12 ** 2)).max() < 1e-12


def test_panda_fk_known_answers():
    """grasp-target origin at q = 0 and at q_ready."""
    _, d = Cf.config2()
    T = O.forward_kinematics(d, np.zeros((1, 9), np.float32), "f64")
    assert np.abs(T[0, 11, :3, 3] - [0.088, 0.0, 0.821]).max() < 1e-6
    T = O.forward_kinematics(d, Cf.PANDA_Q_READY[None].astype(np.float32), "f64")
    assert np.abs(T[0, 11, :3, 3] - [0.484207, 0.0, 0.411038]).max() < 2e-6


def test_jacobian_and_curvature_finite_differences():
    """J and c = Jdot qd of vec(T_frame) against fp64 central differences of the FK itself."""
    _, d = Cf.config2()
    rng = np.random.default_rng(2)
    s = Cf.sample_panda_states(rng, 4)
    q = (np.round(s["q"].astype(np.float64) * 64) / 64).astype(np.float32)  # exactly representable +- h
    qd = s["qd"]
    h = 2.0 ** -10
    for fr in (5, 9, 10, 11):
        x, xd, J, c = O.differentiate(d, q, qd, fr, "f64")

        def fk(qq):
            return O.forward_kinematics(d, qq.astype(np.float32), "f64")[:, fr].reshape(len(qq), 16)
        Jfd = np.stack([(fk(q + h * np.eye(9)[j]) - fk(q - h * np.eye(9)[j])) / (2 * h) for j in range(9)], axis=2)
        assert np.abs(J - Jfd).max() < 5e-6
        assert np.abs(xd - np.einsum("rkj,rj->rk", J, qd.astype(np.float64))).max() < 1e-12
        # c = d/dt (J qd) at qdd = 0 = directional second derivative of x along qd.  Use a step t along qd.
        t = 2.0 ** -6
        qp = (q.astype(np.float64) + t * qd).astype(np.float64)
        qm = (q.astype(np.float64) - t * qd).astype(np.float64)
        # second difference needs sub-float32 steps: evaluate the oracle on float32-exact points only
        if np.array_equal(qp.astype(np.float32), qp) and np.array_equal(qm.astype(np.float32), qm):
            cfd = (fk(qp) - 2 * x + fk(qm)) / t ** 2
            assert np.abs(c - cfd).max() < 1e-4


def test_pinv_matches_numpy_with_tf_cutoff():
    rng = np.random.default_rng(3)
    for n, rank in ((9, 9), (9, 3), (2, 1), (7, 5)):
        B = rng.normal(size=(n, rank))
        M = B @ B.T if rank < n else rng.normal(size=(n, n))
        f = rng.normal(size=n)
        x, dropped = O.pinv_solve(M, f)
        want = np.linalg.pinv(M, rcond=10 * n * np.finfo(np.float64).eps) @ f
        assert dropped == n - rank
        assert np.abs(x - want).max() < 1e-9 * max(1.0, np.abs(want).max())


def test_fp32_noise_floor_is_below_tolerance_on_fixture_states(golden_dir):
    """The reference algorithm evaluated in fp64 vs fp32 on the fixture states: documents that an
    absolute 1e-5 is meaningful there (|qdd| = O(1), benign conditioning)."""
    g = np.load(os.path.join(golden_dir, "config3.npz"))
    _, d = Cf.config3()
    a = O.step(d, g["q"], g["qd"], g["goal"], spheres=g["spheres"], precision="f32")["qdd64"]
    b = O.step(d, g["q"], g["qd"], g["goal"], spheres=g["spheres"], precision="f64")["qdd64"]
    assert np.abs(a - b).max() < ATOL


def test_capsule_table_equals_explicit_closest_point_pairs(golden_dir):
    """The capsule primitive is the point-vs-capsule case of the reference's CPU closest-point stage
    (simulation.py:462-484).  Pin it two ways: (1) the closed-form nearest point against a brute-force scan of
    the capsule axis; (2) the oracle's fused capsule mode against its reference-faithful EXPLICIT_PAIRS mode fed
    with pairs computed independently in fp64 numpy."""
    g = np.load(os.path.join(golden_dir, "config3.npz"))
    _, d = Cf.config3()
    rng = np.random.default_rng(11)
    caps = Cf.sample_capsules(rng, 9)
    caps[0, 4:7] = caps[0, 0:3]                      # degenerate capsule == sphere
    origins = g["origins"]
    pl, po = Cf.pairs_from_capsules(origins, caps)
    # (1) brute force: no point of the axis is closer than the closed-form one
    ts = np.linspace(0.0, 1.0, 2001)[:, None]
    for k in range(caps.shape[0]):
        axis_pts = caps[k, 0:3][None, :] + ts * (caps[k, 4:7] - caps[k, 0:3])[None, :]
        for r in range(origins.shape[0]):
            for c in range(origins.shape[1]):
                best = np.linalg.norm(axis_pts - origins[r, c][None, :], axis=1).min() - caps[k, 3]
                mine = np.linalg.norm(pl[r, c * 9 + k] - po[r, c * 9 + k])
                assert mine <= best + 1e-6 and abs(mine - best) < 1e-4
    # (2) fused capsule mode == explicit pairs
    ra = O.step(d, g["q"], g["qd"], g["goal"], spheres=caps)
    rb = O.step(d, g["q"], g["qd"], g["goal"], p_link=pl, p_obs=po)
    scale = np.maximum(1.0, np.abs(rb["qdd64"]).max(axis=1, keepdims=True))
    assert (np.abs(ra["qdd64"] - rb["qdd64"]) / scale).max() < 2e-6
    # the degenerate capsule alone reproduces the sphere mode bit for bit
    rs = O.step(d, g["q"], g["qd"], g["goal"], spheres=caps[:1, :4])
    rc = O.step(d, g["q"], g["qd"], g["goal"], spheres=caps[:1])
    assert np.array_equal(rs["qdd"], rc["qdd"])


@pytest.mark.parametrize("key", ["tj", "pd"])
def test_golden_exp05_attached_point_leaves(golden_dir, key):
    """SURVEY 8(a) a11 + a21: chain [FK, TaskmapRelative4x4, 4x4->pos] with CollisionAvoidance; the analytic
    restatement (lever arm in J, xd and c) against the nested-autograd vectors."""
    g = np.load(os.path.join(golden_dir, "exp05.npz"))
    _, d = Cf.exp05_two_joint() if key == "tj" else Cf.exp05_panda()
    r = O.step(d, g[f"{key}_q"], g[f"{key}_qd"], g[f"{key}_goal"], p_link=g[f"{key}_rel"], p_obs=g[f"{key}_nvec"],
               dist=g[f"{key}_dist"])
    assert np.abs(r["M"] - g[f"{key}_M"]).max() < 5e-6 and np.abs(r["f"] - g[f"{key}_f"]).max() < 2e-6
    _check(r["qdd64"], g[f"{key}_qdd"], f"exp05 {key}")


def test_golden_euler_taskmap(golden_dir):
    """chain [FK(frame), TaskmapFrom4x4ToEuler]; analytic (H^-1 w, H^-1 J_w, H^-1(alpha - Hdot xd))
    against the nested-autograd vectors of the reference's expression; plus SciPy's 'xyz' Euler angles."""
    from scipy.spatial.transform import Rotation
    g = np.load(os.path.join(golden_dir, "euler.npz"))
    _, d = Cf.config2()
    T = O.forward_kinematics(d, g["q"], "f64")
    for fr in g["frames"]:
        x, xd, J, c = O.differentiate_euler(d, g["q"], g["qd"], int(fr))
        assert np.abs(x - g[f"f{fr}_x"]).max() < 2e-6
        assert np.abs(xd - g[f"f{fr}_xd"]).max() < 2e-6
        assert np.abs(J - g[f"f{fr}_J"]).max() < 5e-6
        assert np.abs(c - g[f"f{fr}_c"]).max() < 2e-6
        ref = Rotation.from_matrix(T[:, int(fr), :3, :3]).as_euler("xyz")      # tests/test_taskmaps.py:46
        assert np.abs(x - ref).max() < 2e-6


# ---- leaf kinds the BASELINE configs do not reach: identity-map TargetPolicy, ConfigurationSpaceBiasing ----------------
@pytest.mark.parametrize("key", ["tj", "tjd", "pdi", "p04"])
def test_golden_exp04_sets(golden_dir, key):
    """experiments/two_joint_robot/04_driving_into_jointlimits.py:46-52 (TargetPolicy on the IDENTITY map +
    JointLimitAvoidance) and experiments/franka_panda/04_nullspace_control.py:41-52 (TargetPolicy on FK + kind 8,
    ConfigurationSpaceBiasing): the C oracle against the autograd vectors."""
    g = np.load(os.path.join(golden_dir, "exp04.npz"))
    _, d = {"tj": lambda: Cf.exp04_two_joint(), "tjd": lambda: Cf.exp04_two_joint(with_damping=True),
            "pdi": Cf.exp04_panda_identity_target, "p04": Cf.panda04_nullspace}[key]()
    r = O.step(d, g[f"{key}_q"], g[f"{key}_qd"], g[f"{key}_goal"])
    assert np.abs(r["M"] - g[f"{key}_M"]).max() < 2e-6 and np.abs(r["f"] - g[f"{key}_f"]).max() < 2e-6
    if key in ("tj", "tjd", "pdi"):   # the joint-limit band is exercised: column-scaled, non-symmetric metric (quirk Q2)
        assert max(np.abs(m - m.T).max() for m in g[f"{key}_M"]) > 1e-3
    _check(r["qdd64"], g[f"{key}_qdd"], f"exp04 {key}")


def test_exp06_parameters_typed_from_the_script_not_from_configs(golden_dir):
    """Breaks the shared-configs.py blind spot: every other test builds the product's descriptor AND the oracle's
    leaves from riemannian_motion_policies_amd.configs / descriptor.LeafSpec, so a wrong parameter order there would be
    invisible.  Here the experiment-06 RMP set is typed in as the script's literal keyword arguments
    (experiments/franka_panda/06_cluttered_environment.py:70-114), ordered by the reference constructors' own signatures
    (rmp2.py:32-38, :87-89, :116-119, :141-155, :202-203), fed to the autograd oracle without touching configs.py or
    LeafSpec, and must reproduce the qdd of the path the committed golden was generated through (configs.py,
    tests/golden/make_fixtures.py) to 1e-9, evaluated in this process, and the committed golden qdd itself to 1e-6 (the oracle
    runs in fp32 like the reference, and another CPU's fp32 kernels round differently: up to ~1e-7 here)."""
    import json
    import torch_autodiff_oracle as TA
    g = np.load(os.path.join(golden_dir, "config3.npz"))
    gold = json.load(open(os.path.join(golden_dir, "kinematic_tables.json")))
    fk = TA.UrdfForwardKinematicTorch(gold["panda"])
    signature = {   # positional order of the reference constructors (goal / taskmap / name excluded)
        "TargetAttractor": ["accel_p_gain", "accel_d_gain", "accel_norm_eps", "metric_alpha_length_scale", "min_metric_alpha",
                            "max_metric_scalar", "min_metric_scalar", "proximity_metric_boost_scalar",
                            "proximity_metric_boost_length_scale"],
        "JointVelocityCap": ["max_velocity", "velocity_damping_region", "damping_gain", "metric_weight"],
        "JointDamping": ["accel_d_gain", "metric_scalar", "inertia"],
        "CSpaceBiasing": ["metric_scalar", "position_gain", "damping_gain", "robust_position_term_thresh", "inertia"],
        "ObstacleAvoidance": ["margin", "damping_gain", "damping_std_dev", "damping_robustness_eps",
                              "damping_velocity_gate_length_scale", "repulsion_gain", "repulsion_std_dev",
                              "metric_modulation_radius", "metric_scalar", "metric_exploder_std_dev", "metric_exploder_eps"],
    }
    script = [   # 06_cluttered_environment.py:70-114, as written there
        ("TargetAttractor", 1, 1, "panda_grasptarget_hand",
         dict(accel_p_gain=0.3, accel_d_gain=0.6, accel_norm_eps=0.075, metric_alpha_length_scale=0.05, min_metric_alpha=0.03,
              max_metric_scalar=1, min_metric_scalar=0.5, proximity_metric_boost_scalar=1.,
              proximity_metric_boost_length_scale=0.02), None),
        ("JointVelocityCap", 2, 0, None,
         dict(max_velocity=0.5, velocity_damping_region=0.15, damping_gain=5.0, metric_weight=0.05), None),
        ("JointDamping", 3, 0, None, dict(accel_d_gain=1, metric_scalar=0.005, inertia=0.3), None),
        ("CSpaceBiasing", 5, 0, None,
         dict(metric_scalar=0.005, position_gain=1, damping_gain=2, robust_position_term_thresh=0.5, inertia=0.0001),
         [0.0, -0.9, 0.0, -2.8, 0.0, 2.0, 0.7853981633974483, 0.02, 0.02]),
    ]
    obstacle_kwargs = dict(margin=0., damping_gain=50, damping_std_dev=0.04, damping_robustness_eps=0.01,
                           damping_velocity_gate_length_scale=0.01, repulsion_gain=800, repulsion_std_dev=0.01,
                           metric_modulation_radius=0.5, metric_scalar=1, metric_exploder_std_dev=0.02,
                           metric_exploder_eps=0.001)
    # 8 of the 10 collision frames, in frame order
    control_frames = ["panda_joint2", "panda_joint3", "panda_joint4", "panda_joint5", "panda_joint7", "panda_hand_joint",
                      "panda_finger_joint1", "panda_finger_joint2"]
    leaves = []
    for cls, kind, tm, frame, kw, vec_a in script:
        assert list(kw) == signature[cls]   # the script passes keywords in signature order; any drift shows here
        leaves.append({"kind": kind, "taskmap": tm, "frame": frame, "params": [float(np.float32(kw[k])) for k in signature[cls]],
                       "vec_a": vec_a, "vec_b": None, "goal_offset": 0 if cls == "TargetAttractor" else -1})
    for fr in control_frames:
        leaves.append({"kind": 4, "taskmap": 2, "frame": fr,
                       "params": [float(np.float32(obstacle_kwargs[k])) for k in signature["ObstacleAvoidance"]],
                       "vec_a": None, "vec_b": None, "goal_offset": -1})
    # explicit closest-point pairs straight from the fixture's origins / spheres (numpy, no configs helper)
    K = len(g["spheres"])
    c, rad = g["spheres"][:, :3].astype(np.float32), g["spheres"][:, 3:4].astype(np.float32)
    t3, d3 = Cf.config3()
    by_configs, dl = TA.leaves_from_desc(d3, t3.frame_names), D.distance_leaf_indices(d3)
    for r in range(6):
        pairs = {}
        for k in range(8):
            o = g["origins"][r, k].astype(np.float32)[None, :]
            diff = o - c
            dist = np.sqrt((diff * diff).sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)
            pairs[4 + k] = (np.repeat(o, K, 0), (c + rad * (diff / dist)).astype(np.float32))
        qdd, _, _ = TA.evaluate_one(fk, leaves, g["q"][r], g["qd"][r], g["goal"][r], pairs)
        # the golden's own path (make_fixtures.py: configs.py leaves, configs.py pairs) on this CPU's fp32 kernels
        pl, po = Cf.pairs_from_spheres(g["origins"][r:r + 1], g["spheres"])
        want, _, _ = TA.evaluate_one(fk, by_configs, g["q"][r], g["qd"][r], g["goal"][r],
                                     {li: (pl[0, k * K:(k + 1) * K], po[0, k * K:(k + 1) * K]) for k, li in enumerate(dl)})
        assert np.abs(qdd - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (r, qdd, want)
        assert np.abs(qdd - g["qdd"][r]).max() <= 1e-6 * max(1.0, np.abs(g["qdd"][r]).max()), (r, qdd, g["qdd"][r])


def test_link_capsule_closest_points_against_a_brute_force_scan():
    """The fp64 closed form the GPU stage is tested against (configs.pairs_from_link_capsules: segment-segment closest points
    of a link capsule and an obstacle primitive) against a brute-force scan of both axes (401 x 401 samples per pair):
    the distance between the returned surface points must equal the scanned minimum axis distance minus both radii."""
    from riemannian_motion_policies_amd import configs as Cf
    rng = np.random.default_rng(31)
    R, Cn, K = 3, 4, 5
    T = np.tile(np.eye(4), (R, Cn, 1, 1))
    for r in range(R):
        for c in range(Cn):
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            T[r, c, :3, :3] = Q * np.sign(np.linalg.det(Q))
            T[r, c, :3, 3] = rng.uniform(-0.5, 0.5, 3)
    lc = np.zeros((Cn, 8), np.float32)
    lc[:, 0:3] = rng.uniform(-0.2, 0.2, (Cn, 3))
    lc[:, 4:7] = rng.uniform(-0.2, 0.2, (Cn, 3))
    lc[:, 3] = rng.uniform(0.03, 0.08, Cn)
    lc[0, 4:7] = lc[0, 0:3]                                  # a degenerate link (a point)
    for tab in (Cf.sample_spheres(rng, K), Cf.sample_capsules(rng, K)):
        pl, po = Cf.pairs_from_link_capsules(T, lc, tab)
        u = np.linspace(0, 1, 401)
        for r in range(R):
            for c in range(Cn):
                A = T[r, c, :3, 3] + T[r, c, :3, :3] @ lc[c, 0:3]
                B = T[r, c, :3, 3] + T[r, c, :3, :3] @ lc[c, 4:7]
                X = A[None] + u[:, None] * (B - A)[None]
                for k in range(K):
                    C0 = tab[k, 0:3].astype(np.float64)
                    D0 = tab[k, 4:7].astype(np.float64) if tab.shape[1] == 8 else C0
                    Y = C0[None] + u[:, None] * (D0 - C0)[None]
                    dmin = np.sqrt(((X[:, None, :] - Y[None, :, :]) ** 2).sum(-1)).min()
                    got = np.linalg.norm(pl[r, c * K + k].astype(np.float64) - po[r, c * K + k])
                    assert abs(got - abs(dmin - lc[c, 3] - tab[k, 3])) < 2e-3, (r, c, k, got, dmin)


def test_structural_zero_columns_follow_the_autodiff_restatement(golden_dir):
    """Where a frame's origin lies on the axis of a revolute ancestor joint for every q, differentiating through the chain of
    LOCAL transforms (kinematics.py:243-270) gives a column of EXACT zeros -- the autodiff restatement of the reference shows
    it (torch_autodiff_oracle.py, same graph as TensorFlow's) -- and the pseudo-inverse of a set that gives the dof no other
    metric (the reference's Panda experiments 01-03: a target policy only) then returns exactly 0 for it.  The C oracle takes
    the same zero pattern (rmp2_oracle.c lever_zero_table): pinned here for every frame of both reference robots, and through the
    resolved q-double-dot of the experiment-01 set."""
    import json
    import torch
    import torch_autodiff_oracle as TA
    gold = json.load(open(os.path.join(golden_dir, "kinematic_tables.json")))
    for name, table_fn, sampler in (("panda", Cf.panda_table, Cf.sample_panda_states), ("two_joint", Cf.two_joint_table, Cf.sample_two_joint_states)):
        t = table_fn()
        fk = TA.UrdfForwardKinematicTorch(gold[name])
        desc = D.build_desc(t, [D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS)])
        s = sampler(np.random.default_rng(11), 2)
        found = 0
        for frame in t.frame_names:
            fi = t.frame_index(frame)
            for r in range(2):
                _, _, Jt, _ = fk.differentiate(torch.tensor(s["q"][r:r + 1]), torch.tensor(s["qd"][r:r + 1]), frame)
                Jt = Jt[0].numpy()[[3, 7, 11]]                                      # d position / d q   (taskmap.py:45-54)
                _, _, Jc, _ = O.differentiate(desc, s["q"][r:r + 1], s["qd"][r:r + 1], fi)
                Jc = Jc[0][[3, 7, 11]]
                zero_t, zero_c = (Jt == 0).all(axis=0), (Jc == 0).all(axis=0)
                assert (zero_t == zero_c).all(), f"{name} {frame}: autodiff zero columns {np.nonzero(zero_t)[0]}, C oracle {np.nonzero(zero_c)[0]}"
                assert np.abs(Jt - Jc).max() < 2e-6
                # columns of ancestors that are exactly zero: the structural ones
                anc = {t.q_index[j] for j in _ancestors(t, fi) if t.q_index[j] >= 0}
                found += sum(1 for d in anc if zero_c[d])
        assert found > 0 or name == "two_joint", f"{name}: no structural zero found"
    # experiment 01 on the Panda (experiments/franka_panda/01_target_rmp_only.py:46): joint 7, on whose axis the grasp target
    # sits, and the fingers resolve to exactly 0
    t = Cf.panda_table()
    desc = D.build_desc(t, [D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_FK_POSITION, t.frame_index("panda_grasptarget_hand"),
                                       Cf.PANDA04_TARGET_POLICY_PARAMS, goal_len=3)], "pinv")
    s = Cf.sample_panda_states(np.random.default_rng(3), 50)
    ref = O.step(desc, s["q"], s["qd"], s["goal"])
    assert (ref["M"][:, 6:, :] == 0).all() and (ref["M"][:, :, 6:] == 0).all() and (ref["f"][:, 6:] == 0).all() and (ref["qdd64"][:, 6:] == 0).all()
    fk = TA.UrdfForwardKinematicTorch(gold["panda"])
    qdd, M, f = TA.evaluate_one(fk, TA.leaves_from_desc(desc, t.frame_names), s["q"][0], s["qd"][0], s["goal"][0])
    assert (M[6:, :] == 0).all() and (M[:, 6:] == 0).all() and (qdd[6:] == 0).all()


def _ancestors(t, frame):
    out, j = [], frame
    while j >= 0:
        out.append(j)
        j = int(t.parent[j])
    return out


def test_pinv_of_a_non_finite_system_is_nan():
    """tf.linalg.pinv of a matrix holding NaN / Inf is NaN in every entry (its SVD is) [TF-doc]: a robot with a NaN joint position
    resolves to NaN on every joint (rmp.py:153-154).  Round 4 (tools/fuzz_parity.py): the C oracle's Jacobi sweeps compared with
    NaN -- every comparison false, read as "every singular value dropped" -- and answered 0."""
    _, desc = Cf.config2()
    s = Cf.sample_panda_states(np.random.default_rng(0), 4)
    s["q"][1, 2] = np.nan
    s["qd"][2, 3] = np.inf
    s["q"][3, :] = np.nan
    r = O.step(desc, s["q"], s["qd"], s["goal"])
    assert np.isfinite(r["qdd64"][0]).all() and r["status"][0] == 0
    assert np.isnan(r["qdd64"][1:]).all() and (r["status"][1:] & D.STATUS_NONFINITE).all()
    x, _ = O.pinv_solve(np.array([[1.0, np.nan], [0.0, 1.0]]), np.array([1.0, 1.0]))
    assert np.isnan(x).all()

"""The two identity-leaf loops of the quad mapping (csrc/rmp2_quad.h): the structured loop -- every identity leaf of the set is
m * I (JointDamping, CSpaceBiasing, configuration-space biasing) or the velocity cap, on a robot that uses every dof of the
9-dof template -- and the general loop, which keeps sets with a dense identity leaf (JointLimitAvoidance, TargetPolicy on the
identity map) and robots with fewer dofs than the template.  rmp2_last_kernel names the structured loop when a launch ran it;
both loops answer to the CPU oracle under the tolerance of tests/test_gpu_parity.py (1e-5, relative to max(1, |qdd|))."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ATOL = 1e-5
STRUCTURED = "identity leaves: structured loop, full width"


def _quad_engine(desc):
    """The quad mapping at any fleet size (RMP2_KERNEL is read when the handle is created)."""
    from riemannian_motion_policies_amd.engine import Engine
    old = os.environ.get("RMP2_KERNEL")
    os.environ["RMP2_KERNEL"] = "quad"
    try:
        return Engine(desc, 0)
    finally:
        if old is None:
            del os.environ["RMP2_KERNEL"]
        else:
            os.environ["RMP2_KERNEL"] = old


def _check(eng, desc, q, qd, goal, sph, what):
    import torch
    import oracle as O
    st = torch.zeros(len(q), dtype=torch.int32, device="cuda")
    out = eng.step(torch.from_numpy(q), torch.from_numpy(qd), torch.from_numpy(goal),
                   obstacles=eng.obstacles(spheres=torch.from_numpy(sph)), status=st)
    torch.cuda.synchronize()
    kernel = eng.last_kernel()
    assert "quad" in kernel, kernel
    ref = O.step(desc, q, qd, goal, spheres=sph)["qdd64"]
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got - ref).max(axis=1)
    tol = ATOL * np.maximum(1.0, np.abs(ref).max(axis=1))
    print(f"{what}: worst error {err.max():.3e}, worst error / tolerance {np.max(err / tol):.3f} [{kernel}]")
    assert (err <= tol).all(), f"{what}: worst {err.max():.3e} ({kernel})"
    return kernel


def _panda_inputs(R, seed):
    from riemannian_motion_policies_amd import configs as Cf
    rng = np.random.default_rng(seed)
    s = Cf.sample_panda_states(rng, R)
    sph = Cf.sample_spheres(rng)
    sph[:, 2] += 1.2  # above the arms: clearances stay out of the near-contact regime (tests/test_gpu_fleet_sizes.py)
    return s["q"], s["qd"], s["goal"], sph


def _panda_specs(identity):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    from riemannian_motion_policies_amd.urdf import panda_table
    t = panda_table()
    specs = [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("panda_grasptarget_hand"),
                        Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3)]
    kinds = {
        "cap": D.LeafSpec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, Cf.JOINT_VELOCITY_CAP_PARAMS),
        "damping": D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS),
        "cspace": D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.CSPACE_BIASING_PARAMS, vec_a=Cf.CSPACE_BIASING_GOAL),
        "config_space": D.LeafSpec(D.LEAF_CONFIG_SPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.PANDA04_CONFIG_SPACE_BIASING_PARAMS,
                                   vec_a=Cf.CSPACE_BIASING_GOAL),
        "limits": D.LeafSpec(D.LEAF_JOINT_LIMIT_AVOIDANCE, D.TASKMAP_IDENTITY, -1, Cf.JOINT_LIMIT_PARAMS,
                             vec_a=Cf.PANDA_Q_LOW, vec_b=Cf.PANDA_Q_HIGH),
    }
    specs += [kinds[k] for k in identity]
    for fr in Cf.CONTROL_POINT_FRAMES[:3]:
        specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr), Cf.OBSTACLE_AVOIDANCE_PARAMS))
    return t, specs


@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("R", [300, 20481])
def test_config3_takes_the_structured_loop(hip_lib, solve, R):
    """Config 3 (velocity cap, damping, c-space biasing): the structured loop at a small fleet (two waves per SIMD) and at a
    fleet of the default quad dispatch."""
    from riemannian_motion_policies_amd import configs as Cf
    _, desc = Cf.config3(solve)
    q, qd, goal, sph = _panda_inputs(R, 11 + R)
    eng = _quad_engine(desc)
    sub = np.unique(np.concatenate([np.arange(min(R, 150)), np.arange(max(0, R - 150), R)]))
    import torch
    out = eng.step(torch.from_numpy(q), torch.from_numpy(qd), torch.from_numpy(goal), obstacles=eng.obstacles(spheres=torch.from_numpy(sph)))
    torch.cuda.synchronize()
    assert STRUCTURED in eng.last_kernel(), eng.last_kernel()
    import oracle as O
    ref = O.step(desc, q[sub], qd[sub], goal[sub], spheres=sph)["qdd64"]
    err = np.abs(out.cpu().numpy()[sub] - ref).max(axis=1)
    tol = ATOL * np.maximum(1.0, np.abs(ref).max(axis=1))
    print(f"config3 {solve} R={R}: worst error {err.max():.3e}, worst error / tolerance {np.max(err / tol):.3f}")
    assert (err <= tol).all(), f"config3 {solve} R={R}: worst {err.max():.3e}"


@pytest.mark.parametrize("identity", [("damping",), ("config_space", "damping"), ("cap", "cspace", "config_space", "damping"),
                                      ("damping", "cap", "cap")])
def test_structured_only_sets(hip_lib, identity):
    """Every structured kind, alone and combined, in several orders: the structured loop, against the oracle."""
    from riemannian_motion_policies_amd import descriptor as D
    t, specs = _panda_specs(identity)
    desc = D.build_desc(t, specs)
    kernel = _check(_quad_engine(desc), desc, *_panda_inputs(300, 5), what="+".join(identity))
    assert STRUCTURED in kernel, kernel


@pytest.mark.parametrize("identity", [("limits", "damping", "cap"), ("damping", "cap", "limits"), ("cspace", "limits", "damping")])
def test_a_dense_identity_leaf_keeps_the_general_loop(hip_lib, identity):
    """Sets that mix a dense identity leaf (JointLimitAvoidance) with structured ones, the dense one first, last and in the
    middle: the general loop, in leaf order, against the oracle."""
    from riemannian_motion_policies_amd import descriptor as D
    t, specs = _panda_specs(identity)
    desc = D.build_desc(t, specs)
    kernel = _check(_quad_engine(desc), desc, *_panda_inputs(300, 6), what="+".join(identity))
    assert "structured loop" not in kernel, kernel


@pytest.mark.parametrize("order", ["dense_first", "dense_last"])
def test_identity_target_policy_keeps_the_general_loop(hip_lib, order):
    """TargetPolicy on the identity map (dense, symmetric metric: the set stays on the symmetric builds, which carry both
    loops) before and after structured leaves."""
    import torch
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    from riemannian_motion_policies_amd.urdf import panda_table
    t = panda_table()
    n = t.n_dof
    tp = D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_IDENTITY, -1, Cf.PANDA04_TARGET_POLICY_PARAMS, goal_len=n)
    rest = [D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS),
            D.LeafSpec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, Cf.JOINT_VELOCITY_CAP_PARAMS)]
    specs = [tp] + rest if order == "dense_first" else rest + [tp]
    specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(Cf.CONTROL_POINT_FRAMES[0]),
                            Cf.OBSTACLE_AVOIDANCE_PARAMS))
    desc = D.build_desc(t, specs)
    q, qd, _, sph = _panda_inputs(300, 7)
    rng = np.random.default_rng(8)
    goal = (q + rng.uniform(-0.4, 0.4, q.shape)).astype(np.float32)
    kernel = _check(_quad_engine(desc), desc, q, qd, goal, sph, what=order)
    assert "structured loop" not in kernel, kernel


@pytest.mark.parametrize("want_dofs", ["fewer", "nine"])
def test_random_tree_width_selects_the_loop(tmp_path, hip_lib, want_dofs):
    """Random trees on the 9-dof template: one that uses every dof takes the structured loop at full width, one with fewer dofs
    keeps the general loop (its row and column tests are run-time tests); both against the oracle."""
    from test_gpu_random_robots import _write_urdf
    from riemannian_motion_policies_amd import descriptor as D, urdf
    rng = np.random.default_rng(2024)
    path = str(tmp_path / "rnd.urdf")
    t = None
    for _ in range(400):
        movable = _write_urdf(path, rng, int(rng.integers(6, 13)), branch_prob=0.25)
        order = movable[:9] if want_dofs == "nine" else movable[: int(rng.integers(3, 8))]
        if len(order) < (9 if want_dofs == "nine" else 3):
            continue
        cand = urdf.compile_urdf(path, order)
        if cand.depth_first_schedule()[3] <= 2:
            t = cand
            break
    assert t is not None
    n, F = t.n_dof, t.n_frames
    assert (n == 9) if want_dofs == "nine" else (3 <= n < 9)
    frames = rng.choice(F, size=min(F, 3), replace=False)
    specs = [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, int(frames[0]),
                        [0.3, 0.6, 0.075, 0.05, 0.03, 1.0, 0.5, 1.0, 0.02], goal_len=3),
             D.LeafSpec(D.LEAF_JOINT_VELOCITY_CAP, D.TASKMAP_IDENTITY, -1, [0.5, 0.15, 5.0, 0.05]),
             D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, [1.0, 0.005, 0.3]),
             D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, [0.005, 1.0, 2.0, 0.5, 0.0001],
                        vec_a=rng.uniform(-0.5, 0.5, n))]
    for fr in frames:
        specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, int(fr),
                                [0.0, 50.0, 0.04, 0.01, 0.01, 800.0, 0.01, 0.5, 1.0, 0.02, 0.001]))
    R = 300
    q = rng.uniform(-1.0, 1.0, (R, n)).astype(np.float32)
    qd = rng.uniform(-0.6, 0.6, (R, n)).astype(np.float32)  # some joints beyond the velocity cap's cutoff
    goal = rng.uniform(-0.5, 0.5, (R, 3)).astype(np.float32)
    sph = np.concatenate([rng.uniform(-1, 1, (5, 3)) + [0, 0, 3.0], rng.uniform(0.05, 0.1, (5, 1))], axis=1).astype(np.float32)
    for solve in ("auto", "pinv"):
        desc = D.build_desc(t, specs, solve)
        kernel = _check(_quad_engine(desc), desc, q, qd, goal, sph, what=f"random tree, {n} dofs, {solve}")
        assert (STRUCTURED in kernel) == (n == 9), kernel

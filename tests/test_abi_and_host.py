"""C-ABI library loads and exports every symbol include/rmp2.h declares; host-side logic
(descriptor compiler, RmpCore registry, task-map classification, sharding).  No GPU compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from riemannian_motion_policies_amd import configs as Cf
from riemannian_motion_policies_amd import descriptor as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    declared = set(re.findall(r"\b(rmp2_[a-z_0-9]+)\s*\(", hdr))
    declared -= {"rmp2_handle"}
    assert {"rmp2_create", "rmp2_destroy", "rmp2_step", "rmp2_last_error", "rmp2_forward_kinematics",
            "rmp2_differentiate", "rmp2_differentiate_euler", "rmp2_closest_points", "rmp2_rollout", "rmp2_abi_version", "rmp2_sizeof_desc", "rmp2_sizeof_obstacles"} <= declared
    lib = C.CDLL(hip_lib)
    for sym in declared:
        assert hasattr(lib, sym), f"{sym} declared in include/rmp2.h but not exported"
    lib.rmp2_sizeof_desc.restype = C.c_size_t
    lib.rmp2_sizeof_obstacles.restype = C.c_size_t
    assert lib.rmp2_abi_version() == D.ABI_VERSION
    assert lib.rmp2_sizeof_desc() == C.sizeof(D.Desc)
    assert lib.rmp2_sizeof_obstacles() == C.sizeof(D.Obstacles)


def test_product_library_has_no_cpu_path_and_fails_loudly(hip_lib):
    """Without a HIP device rmp2_create must fail with RMP2_ERR_NO_DEVICE (no fallback);
    with a device it must succeed.  Also: bad ABI version is rejected."""
    import torch
    lib = C.CDLL(hip_lib)
    lib.rmp2_last_error.restype = C.c_char_p
    lib.rmp2_last_error.argtypes = [C.c_void_p]
    _, desc = Cf.config2()
    h = C.c_void_p()
    rc = lib.rmp2_create(C.byref(desc), 0, C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h
        lib.rmp2_destroy.argtypes = [C.c_void_p]
        lib.rmp2_destroy(h)
    else:
        assert rc == -3 and not h
        assert b"no usable HIP device" in lib.rmp2_last_error(None)
    desc.abi_version = 99
    assert lib.rmp2_create(C.byref(desc), 0, C.byref(h)) == -5


def test_product_never_imports_oracle():
    """The product package must not reference oracle/ (tier rule: oracle is test infrastructure)."""
    pkg = os.path.join(ROOT, "riemannian_motion_policies_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "oracle/" not in text.replace("oracle/ ", ""), f


def test_every_header_is_in_the_staleness_hash():
    """Every csrc/*.h is named in HIP_HEADERS (kernel_src_hash and rmp2_hip's stamp read that list), and every name there is a file:
    a header left out would let a stale library pass for current."""
    import __graft_entry__ as g
    on_disk = {f for f in os.listdir(g.CSRC) if f.endswith(".h")}
    assert on_disk and on_disk == set(g.HIP_HEADERS), (sorted(on_disk - set(g.HIP_HEADERS)), sorted(set(g.HIP_HEADERS) - on_disk))
    assert len(g.HIP_HEADERS) == len(set(g.HIP_HEADERS))
    for _, _, _, headers in g.HIP_UNITS:
        assert set(headers) <= on_disk


def test_descriptor_compiler_layout_and_validation():
    t, d = Cf.config3()
    assert d.n_leaves == 12 and d.goal_floats == 3
    assert D.distance_leaf_indices(d) == list(range(4, 12))
    assert [d.leaves[i].frame for i in range(4, 12)] == [t.frame_index(n) for n in Cf.CONTROL_POINT_FRAMES]
    assert d.leaves[0].goal_offset == 0 and d.leaves[1].goal_offset == -1
    assert abs(d.leaves[3].vec_a[3] - (-2.8)) < 1e-6
    with pytest.raises(ValueError):
        D.build_desc(t, [D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, Cf.CSPACE_BIASING_PARAMS,
                                    vec_a=[0.0] * 3)])
    with pytest.raises(ValueError):
        D.build_desc(t, [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, 99, Cf.TARGET_ATTRACTOR_PARAMS,
                                    goal_len=3)])


def test_class_surface_compiles_to_the_same_descriptor():
    """The reference-style object graph (06_cluttered_environment.py:64-116) must serialise to the
    same leaf records as configs.config3()."""
    from riemannian_motion_policies_amd import rmp, rmp2, taskmap, urdf
    from riemannian_motion_policies_amd.kinematics import UrdfForwardKinematic
    fk = UrdfForwardKinematic(urdf.PANDA_URDF, urdf.PANDA_ORDER)
    assert fk.frame_names == urdf.panda_table().frame_names and fk.n_joints == 9
    core = rmp.RmpCore()
    ee = taskmap.chain_taskmaps([taskmap.TaskmapByForwardKinematic(fk, frame='panda_grasptarget_hand'),
                                 taskmap.TaskmapFrom4x4ToPosition()])
    core.add_rmp(rmp2.TargetAttractor(goal=[0.2, -0.2, 0.5], accel_p_gain=0.3, accel_d_gain=0.6, accel_norm_eps=0.075,
                                      metric_alpha_length_scale=0.05, min_metric_alpha=0.03, max_metric_scalar=1,
                                      min_metric_scalar=0.5, proximity_metric_boost_scalar=1.,
                                      proximity_metric_boost_length_scale=0.02, taskmap=ee, name='attractor'))
    core.add_rmp(rmp2.JointVelocityCap(max_velocity=0.5, velocity_damping_region=0.15, damping_gain=5.0, metric_weight=0.05))
    core.add_rmp(rmp2.JointDamping(accel_d_gain=1, metric_scalar=0.005, inertia=0.3))
    core.add_rmp(rmp2.CSpaceBiasing(goal=Cf.CSPACE_BIASING_GOAL, metric_scalar=0.005, position_gain=1, damping_gain=2,
                                    robust_position_term_thresh=0.5, inertia=0.0001))
    for fr in Cf.CONTROL_POINT_FRAMES:
        tm = taskmap.chain_taskmaps([taskmap.TaskmapByForwardKinematic(fk, fr), taskmap.TaskmapSphereDistance()])
        core.add_rmp(rmp2.ObstacleAvoidance(margin=0., damping_gain=50, damping_std_dev=0.04, damping_robustness_eps=0.01,
                                            damping_velocity_gate_length_scale=0.01, repulsion_gain=800,
                                            repulsion_std_dev=0.01, metric_modulation_radius=0.5, metric_scalar=1,
                                            metric_exploder_std_dev=0.02, metric_exploder_eps=0.001, taskmap=tm,
                                            name=f'collision_avoidance_for_{fr}'))
    specs = [r.leaf_spec(lambda f: fk.table.frame_index(f.frame)) for r in core.rmps.values()]
    got = D.build_desc(fk.table, specs)
    _, want = Cf.config3()
    assert bytes(got) == bytes(want)
    # registry protocol (rmp.py:117-131)
    assert "attractor" in str(core) and "used RMPs" in str(core)
    core.remove_rmp_by_name("joint_damping")
    assert "joint_damping" not in core.rmps
    core.add_rmp(rmp2.JointDamping(1, 0.005, 0.3))          # same name overwrites / re-adds
    assert list(core.rmps)[-1] == "joint_damping"
    assert rmp.RmpCore().rmps == {} and rmp.RmpCore().rmps is not rmp.RmpCore().rmps
    assert "no RMPs in use" in str(rmp.RmpCore())


def test_exp05_object_graph_compiles_to_attached_point_leaves():
    """experiments/two_joint_robot/05_obstacle_avoidance.py:44-61 written against the class surface serialises to
    configs.exp05_two_joint(): TargetPolicy + one (CollisionAvoidance, FK_POINT) leaf per frame."""
    from riemannian_motion_policies_amd import rmp, taskmap, urdf
    from riemannian_motion_policies_amd.data_management import Datamanager
    from riemannian_motion_policies_amd.kinematics import UrdfForwardKinematic
    fk = UrdfForwardKinematic(urdf.TWO_JOINT_URDF, urdf.TWO_JOINT_ORDER)
    dm = Datamanager(fk)
    core = rmp.RmpCore()
    ee = taskmap.chain_taskmaps([taskmap.TaskmapByForwardKinematic(fk, frame='link_23'), taskmap.TaskmapFrom4x4ToPosition()])
    core.add_rmp(rmp.TargetPolicy(alpha=0.1, beta=0.1, c=0.1, goal=[1.4, -1.4, 0.1], name='target', taskmap=ee))
    for frame in fk.frame_names:
        tm = taskmap.chain_taskmaps([taskmap.TaskmapByForwardKinematic(fk, frame),
                                     taskmap.TaskmapRelative4x4(relative_pos=dm[frame]['relative_position']),
                                     taskmap.TaskmapFrom4x4ToPosition()])
        assert taskmap.classify(tm)[0] == D.TASKMAP_FK_POINT
        core.add_rmp(rmp.CollisionAvoidance(d=dm[frame]['distance'], vec=dm[frame]['normal_vec'], eta_rep=0.1 * np.e,
                                            nu_rep=0.3, eta_damp=1, nu_damp=0.3, r=1.1, c=1e5, taskmap=tm,
                                            name=f'collision_avoidance_for_{frame}'))
    specs = [r.leaf_spec(lambda f: fk.table.frame_index(f.frame)) for r in core.rmps.values()]
    got = D.build_desc(fk.table, specs)
    _, want = Cf.exp05_two_joint()
    assert bytes(got) == bytes(want)
    assert D.distance_leaf_indices(got) == [1, 2, 3]
    # TaskmapRelative4x4.forward is plain array code: T_ref @ [I | rel]
    rel = np.array([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0]], np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [1, 2, 3]
    out = taskmap.TaskmapRelative4x4(rel).forward(T.reshape(1, 16)).reshape(2, 4, 4)
    assert np.allclose(out[:, :3, 3], [[1, 2.1, 3], [0.8, 2, 3]]) and np.allclose(out[:, :3, :3], T[:3, :3])


def test_rmpcore_quick_signature_sees_every_mutation_that_changes_the_program():
    """RmpCore.evaluate recompiles when the policy set changes (rmp.py:127-131 registry; leaf parameters are plain mutable
    attributes in the reference).  The per-call check is a cheap signature: it must change with parameters, constant vectors,
    the task map, the FK frame and the registry -- and must NOT change with goals or obstacle data (per-call inputs)."""
    from riemannian_motion_policies_amd import rmp, rmp2, taskmap, urdf
    from riemannian_motion_policies_amd.kinematics import UrdfForwardKinematic
    fk = UrdfForwardKinematic(urdf.PANDA_URDF, urdf.PANDA_ORDER)
    core = rmp.RmpCore()
    fkm = taskmap.TaskmapByForwardKinematic(fk, frame='panda_grasptarget_hand')
    ee = taskmap.chain_taskmaps([fkm, taskmap.TaskmapFrom4x4ToPosition()])
    target = rmp2.TargetAttractor(goal=[0.2, -0.2, 0.5], accel_p_gain=0.3, accel_d_gain=0.6, accel_norm_eps=0.075,
                                  metric_alpha_length_scale=0.05, min_metric_alpha=0.03, max_metric_scalar=1,
                                  min_metric_scalar=0.5, proximity_metric_boost_scalar=1.,
                                  proximity_metric_boost_length_scale=0.02, taskmap=ee, name='attractor')
    damp = rmp2.JointDamping(accel_d_gain=1, metric_scalar=0.005, inertia=0.3)
    bias = rmp2.CSpaceBiasing(goal=Cf.CSPACE_BIASING_GOAL, metric_scalar=0.005, position_gain=1, damping_gain=2,
                              robust_position_term_thresh=0.5, inertia=0.0001)
    for r in (target, damp, bias):
        core.add_rmp(r)
    s0 = core._quick_signature(9)
    assert core._quick_signature(9) == s0
    target.goal = np.array([0.5, 0.1, 0.4], np.float32)            # a goal is an input, not part of the program
    assert core._quick_signature(9) == s0
    seen = {s0}

    def changed():
        s = core._quick_signature(9)
        fresh = s not in seen
        seen.add(s)
        return fresh
    damp.inertia = 0.31
    assert changed()
    bias.goal = np.asarray(Cf.CSPACE_BIASING_GOAL, np.float32) + np.float32(0.01)   # CSpaceBiasing's goal IS a constant vector
    assert changed()
    fkm.frame = 'panda_hand_joint'
    assert changed()
    target.taskmap = taskmap.chain_taskmaps([taskmap.TaskmapByForwardKinematic(fk, frame='panda_joint7'), taskmap.TaskmapFrom4x4ToPosition()])
    assert changed()
    core.remove_rmp_by_name(damp.name)
    assert changed()
    core.solve = "pinv"
    assert changed()
    assert core._quick_signature(7) not in seen


def test_arrayvar_lazy_values_and_owner_marks():
    """data_management.ArrayVar: assign_lazy defers the value to its first read and keeps the producer's mark through that
    read; any assign() by somebody else clears it (RmpCore steps fused only while every holder still carries the mark)."""
    from riemannian_motion_policies_amd.data_management import ArrayVar, as_array
    calls = []
    owner = object()
    v = ArrayVar(np.zeros((0, 3)))
    assert v.owner is None and v.value.shape == (0, 3)
    v.assign_lazy(lambda: calls.append(1) or np.arange(6, dtype=np.float64).reshape(2, 3), owner=owner)
    assert v.owner is owner and calls == []
    a = v.value
    assert calls == [1] and a.dtype == np.float32 and a.shape == (2, 3) and v.owner is owner
    assert v.value is a and calls == [1]                      # evaluated once
    assert np.array_equal(as_array(v), a) and np.array_equal(np.asarray(v), a)
    v.assign(np.ones((1, 3)))
    assert v.owner is None and v.numpy().shape == (1, 3)
    v.assign_lazy(lambda: np.full((1, 3), 7.0))
    v.value = np.zeros((4, 3))                                # (attribute-style assignment is an assign)
    assert v.owner is None and v.value.shape == (4, 3)


def test_unsupported_chains_raise():
    from riemannian_motion_policies_amd import rmp, taskmap, urdf
    from riemannian_motion_policies_amd.kinematics import UrdfForwardKinematic
    fk = UrdfForwardKinematic(urdf.TWO_JOINT_URDF, urdf.TWO_JOINT_ORDER)
    bad = taskmap.chain_taskmaps([taskmap.TaskmapByForwardKinematic(fk, 'link_23'), taskmap.TaskmapFrom4x4ToEuler()])
    with pytest.raises(NotImplementedError):
        taskmap.classify(bad)
    with pytest.raises(NotImplementedError):
        rmp.CollisionAvoidance(None, None, 1, 1, 1, 1, 1, 1, bad).leaf_spec(lambda f: 0)


def test_shard_bounds_and_balanced_split():
    from riemannian_motion_policies_amd.fleet import balanced_bounds, shard_bounds
    for total, world in ((524288, 8), (10, 4), (3, 8), (0, 2)):
        parts = [shard_bounds(total, world, r) for r in range(world)]
        assert sum(c for _, c in parts) == total
        assert all(parts[r][0] + parts[r][1] == parts[r + 1][0] for r in range(world - 1))
        assert max(c for _, c in parts) - min(c for _, c in parts) <= 1
    w = np.concatenate([np.full(100, 3 * 8.0), np.full(100, 8 * 32.0)])  # TwoJoint-like then Panda-like pair counts
    cuts = balanced_bounds(w, 4)
    loads = [w[cuts[r]:cuts[r + 1]].sum() for r in range(4)]
    assert cuts[0] == 0 and cuts[-1] == 200 and max(loads) - min(loads) <= 2 * w.max()


def test_mixed_fleet_plan_is_a_balanced_partition():
    """Config 5 across ranks: type-sorted fleet, contiguous cuts balanced by estimated work, every robot in
    exactly one shard, per-type ranges consistent with the cuts."""
    from riemannian_motion_policies_amd.fleet import MixedFleetShard
    rng = np.random.default_rng(5)
    total, world = 4096, 8
    counts = rng.integers(0, 33, size=total)
    cuts, ranges, work = MixedFleetShard.plan(total, world, counts)
    assert cuts[0] == 0 and cuts[-1] == total and all(cuts[r] <= cuts[r + 1] for r in range(world))
    n_tj = total // 2
    covered_tj = sum(hi - lo for lo, hi in (r["two_joint"] for r in ranges))
    covered_pd = sum(hi - lo for lo, hi in (r["panda"] for r in ranges))
    assert covered_tj == n_tj and covered_pd == total - n_tj
    for r in range(world):
        (a, b), (c, d) = ranges[r]["two_joint"], ranges[r]["panda"]
        assert (b - a) + (d - c) == cuts[r + 1] - cuts[r]
    assert all(cuts[r + 1] > cuts[r] for r in range(world)), "no rank may be left empty"
    assert max(cuts[r + 1] - cuts[r] for r in range(world)) > 1.5 * min(cuts[r + 1] - cuts[r] for r in range(world)), \
        "TwoJoint robots are cheaper: a time-balanced cut must NOT be an equal-count cut"
    # the full-size fleet on 8 ranks: cut by the measured time curves (fleet.MixedFleetShard.DEFAULT_CURVES) -- kernel time
    # moves in rounds of 16 384 robots, so the Pandas are spread thin and the cheap TwoJoint robots packed
    big = rng.integers(0, 33, size=262144)
    cuts8, ranges8, _ = MixedFleetShard.plan(262144, 8, big)
    est = MixedFleetShard.plan_by_curves(262144, 8, big, MixedFleetShard.DEFAULT_CURVES)[2]
    assert cuts8[-1] == 262144 and max(est) <= 1.1 * (sum(est) / 8) + 5.0
    assert sum(1 for r in ranges8 if r["two_joint"][1] > r["two_joint"][0]) <= 3 and \
        sum(1 for r in ranges8 if r["panda"][1] > r["panda"][0]) >= 5
    # the round-2 linear model stays available
    cutsl, _, workl = MixedFleetShard.plan(total, world, counts, cost=MixedFleetShard.DEFAULT_COST)
    loads = [workl[cutsl[r]:cutsl[r + 1]].sum() for r in range(world)]
    assert max(loads) <= workl.sum() / world + workl.max()      # balanced to within one robot
    # one rank: everything
    cuts1, ranges1, _ = MixedFleetShard.plan(total, 1, counts)
    assert cuts1 == [0, total] and ranges1[0] == {"two_joint": (0, n_tj), "panda": (0, total - n_tj)}


def test_bind_and_explicit_stream_refuse_tensors_that_would_be_copied():
    """Engine.bind() promises a launch on the CALLER's buffers; a tensor it would have to convert (wrong dtype, layout or
    device) must raise instead of being copied once and read stale forever after (the same for step(stream=...))."""
    import torch
    from riemannian_motion_policies_amd.engine import _is_resident, _require_resident
    dev = torch.device("cpu")
    ok = torch.zeros((4, 9), dtype=torch.float32)
    assert _is_resident(ok, dev)
    assert not _is_resident(ok.double(), dev)
    assert not _is_resident(torch.zeros((9, 4)).t(), dev)           # non-contiguous
    assert not _is_resident(np.zeros((4, 9), np.float32), dev)     # not a tensor
    assert not _is_resident(ok, torch.device("cuda", 0))            # wrong device
    _require_resident(dev, q=ok, goal=None)
    with pytest.raises(ValueError, match="qd must be a contiguous fp32 tensor"):
        _require_resident(dev, q=ok, qd=ok.double())


def test_bench_refuses_more_gpus_than_the_node_has():
    """`bench.py --gpus N` outside a launcher starts its own ranks; with fewer devices than asked for it must fail loudly,
    never benchmark fewer GPUs silently (round-1 finding)."""
    import subprocess
    import sys
    import torch
    have = torch.cuda.device_count()   # (does not initialise the GPU runtime)
    if have > 0:
        pytest.skip("starts a child process: only from a process on a box without GPUs (no fork + exec once a GPU is initialised)")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(have + 2), "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "not silently running on fewer" in r.stderr and r.stdout.strip() == ""


def test_validate_runs_the_program_compiler_without_a_gpu(hip_lib):
    """rmp2_validate = rmp2_create's host half (descriptor checks + program compiler), usable without a device: every
    shipped configuration compiles; broken descriptors are rejected with the code and message rmp2_create would give."""
    lib = C.CDLL(hip_lib)
    lib.rmp2_validate.argtypes = [C.POINTER(D.Desc)]
    lib.rmp2_last_error.restype = C.c_char_p
    lib.rmp2_last_error.argtypes = [C.c_void_p]
    for build in (Cf.config1, Cf.config2, Cf.config3, Cf.config5_two_joint, Cf.exp05_two_joint, Cf.exp05_panda,
                  Cf.exp04_two_joint, Cf.exp04_panda_identity_target, Cf.panda04_nullspace):
        for solve in ("auto", "pinv"):
            _, d = build(solve)
            assert lib.rmp2_validate(C.byref(d)) == 0, (build.__name__, lib.rmp2_last_error(None))
    _, d = Cf.config2()
    d.robot.q_index[2] = -2          # found by the sanitizer run (tools/asan_compile_program.sh): used to pass
    assert lib.rmp2_validate(C.byref(d)) == -1 and b"q_index" in lib.rmp2_last_error(None)
    _, d = Cf.config2()
    d.robot.parent[3] = 5
    assert lib.rmp2_validate(C.byref(d)) == -1 and b"topologically" in lib.rmp2_last_error(None)
    _, d = Cf.config3()
    d.leaves[5].frame = 99
    assert lib.rmp2_validate(C.byref(d)) == -1 and b"frame" in lib.rmp2_last_error(None)
    _, d = Cf.config3()
    d.leaves[1].taskmap = D.TASKMAP_FK_DISTANCE   # JointVelocityCap on a distance map: no such kernel
    d.leaves[1].frame = 3
    assert lib.rmp2_validate(C.byref(d)) == -2
    _, d = Cf.config3()
    d.abi_version = 7
    assert lib.rmp2_validate(C.byref(d)) == -5
    assert lib.rmp2_validate(None) == -1

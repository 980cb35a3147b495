"""The edge catalogue of tests/leaf_edge_cases.py on the CPU oracles: every row lands in the class the catalogue writes down, the two
builds of the C oracle (fp32 leaves / fp64) agree on every status word, and -- the two builds share their source -- the autograd
restatement of the reference's graph (oracle/torch_autodiff_oracle.py), which shares no derivation with it, agrees with the
fp32-leaf build on the system of every regular and stiff row and is non-finite on every pole row."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import leaf_edge_cases as L  # noqa: E402

FLEETS = list(L.BUILDERS)
# tests/test_oracle_cross_fuzz.py: the C oracle against the autograd restatement, relative to the system's scale
PIN_M, PIN_F = 2e-5, 2e-5


@pytest.mark.parametrize("key", FLEETS)
def test_every_row_lands_in_its_catalogued_class(key):
    fl = L.fleet(key)
    assert len(fl.q) == L.R and fl.edge.sum() >= 3
    for shape in fl.shapes:
        cls, want = L.classify(key, shape), fl.expected(shape)
        print(f"{key} {shape}: " + ", ".join(f"{c} {int((cls == c).sum())}" for c in ("regular", "stiff", "pole")))
        wrong = [(i, fl.names[i], want[i], cls[i]) for i in np.nonzero(cls != want)[0]]
        assert not wrong, f"{key} {shape}: (row, name, catalogued, on the oracle) {wrong[:8]}"
        r32, r64 = L.references(key, shape)
        bad = np.nonzero(r32["status"] != r64["status"])[0]
        assert bad.size == 0, f"{key} {shape}: the oracle builds disagree on the status of rows {bad[:8]}"
        from riemannian_motion_policies_amd import descriptor as D
        pole = cls == "pole"
        assert ((r64["status"][pole] & D.STATUS_NONFINITE) != 0).all() and ((r64["status"][~pole] & D.STATUS_NONFINITE) == 0).all()
        assert (~np.isfinite(r64["qdd64"][pole])).all(), f"{key} {shape}: a pole row with a finite joint"


def test_edge_rows_keep_apart():
    """One edge row per hex group of four; the plain fleet differs from the fleet on the edge rows only."""
    for key in FLEETS:
        fl = L.fleet(key)
        rows = np.nonzero(fl.edge)[0]
        if "coincide" in key:            # (the descriptor is the edge: every row is one)
            assert len(rows) == L.R
        elif "band_free" not in key:
            assert len(set(rows // 4)) == len(rows), key
        else:
            assert len(set(rows // 16)) == len(rows), key
        for a, b in zip(fl.inputs(), fl.inputs(plain=True)):
            if a is not None:
                assert np.array_equal(a[~fl.edge], b[~fl.edge], equal_nan=True), key
                assert a.dtype == np.float32


def test_exact_structure_on_the_oracle():
    """The exact statements tests/test_gpu_leaf_edges.py makes of the engine hold on both oracle builds."""
    from riemannian_motion_policies_amd import configs as Cf
    for r in L.references("joint_damping", "alone"):
        rows = L.fleet("joint_damping").groups["at_rest"]
        assert np.array_equal(r["M"][rows], np.broadcast_to(np.float32(Cf.JOINT_DAMPING_PARAMS[2]) * np.eye(9), (len(rows), 9, 9)))
        assert (r["f"][rows] == 0).all()
    for key in ("velocity_cap", "velocity_cap_gantry", "velocity_cap_two_joint"):
        for r in L.references(key, "alone"):
            rows = L.fleet(key).groups["below_cutoff"]
            assert (r["f"][rows] == 0).all(), key
            off = ~np.eye(L.fleet(key).n, dtype=bool)            # quirk Q4: w / (1 - 0) off the diagonal
            assert (r["M"][rows][:, off] == float(np.float32(Cf.JOINT_VELOCITY_CAP_PARAMS[3]))).all(), key
    for r in L.references("target_policy_identity", "alone"):
        rows = L.fleet("target_policy_identity").groups["identity_metric_zero_force"]
        assert np.array_equal(r["M"][rows], np.broadcast_to(np.eye(9), (len(rows), 9, 9))) and (r["f"][rows] == 0).all()
    fl = L.fleet("joint_limits")
    for r in L.references("joint_limits", "alone"):
        assert (r["M"][fl.groups["zero_system"] + fl.groups["zero_metric"]] == 0).all() and (r["f"][fl.groups["zero_system"]] == 0).all()
    for name in L.OBSTACLE_TABLES:
        fl = L.fleet("obstacle_" + name)
        for r in L.references(fl.key, "alone"):
            rows = [i for i in fl.groups["zero_leaf"] if fl.names[i] != "tip_receding_z_above"]
            assert (r["M"][rows] == 0).all() and (r["f"][rows] == 0).all(), name


def _autograd_rows(fl):
    """Every row.  (A sphere TABLE has a signed distance -- negative inside the sphere, clamped to
    0 by the leaf -- which no explicit pair restates: |p_link - p_obs| is 0.0625 on the penetrating row, whose restatement is the
    explicit-pair fleet's.)"""
    inside = "spheres" in fl.obs
    return [i for i in range(L.R) if not (inside and fl.names[i] == "tip_penetrating")]


# Of the obstacle fleets the restatement sees the sphere tables of 1 and 33 records and the explicit pairs: the other sphere tables and
# the ragged lists hold the same live record among fillers the leaf cuts to an exact 0.  NO capsule fleet is pinned against the
# restatement here: the autograd oracle has no capsule map, and the pairs it would be fed are the sphere's (the catalogue's capsule
# crosses the sphere's place); the C oracle's capsule closest points are pinned in tests/test_oracle_pins.py
# (test_capsule_table_equals_explicit_closest_point_pairs).
@pytest.mark.parametrize("key", [k for k in FLEETS if not k.startswith("obstacle_") or k in ("obstacle_K1", "obstacle_K33_last", "obstacle_pairs")])
def test_c_oracle_against_the_autograd_restatement(golden_dir, key):
    """The leaf functions target_attractor, joint_velocity_cap, joint_damping, cspace_biasing, obstacle_avoidance,
    joint_limit_avoidance, config_space_biasing, target_policy and collision_avoidance of the autograd oracle, each on its fleet's
    `alone` set: the system of the C oracle's fp32-leaf build within the cross-fuzz pins of the restatement's on every regular and
    stiff row, the restatement non-finite on every pole row.  (A sphere table reaches the restatement as the equivalent explicit
    pairs.)  A row whose SYSTEM fp32 does not determine to the pin -- decided on the C oracle alone: its own fp32-leaf build is further than
    the pin from its fp64 build on the same inputs -- cannot be pinned fp32 against fp32 (two faithful evaluations differ by as much); there the restatement is held to the fp64 system under the bound the engine gets
    (leaf_edge_cases.system_bounds).  Such rows are counted and printed: the velocity cap's rows beside its pole, where
    w / (1 - ratio^2) amplifies a rounding of ratio^2, and JointLimitAvoidance's at the double root of its spline."""
    import torch_autodiff_oracle as TA
    from riemannian_motion_policies_amd import descriptor as D
    fl = L.fleet(key)
    gold = json.load(open(os.path.join(golden_dir, "kinematic_tables.json")))
    fk = TA.UrdfForwardKinematicTorch(L.gantry_golden() if fl.robot == "gantry" else gold[fl.robot])
    desc = fl.desc("alone")
    leaves = TA.leaves_from_desc(desc, L.table(fl.robot).frame_names)
    r32, r64 = L.references(key, "alone")
    cls = L.classify(key, "alone")
    env = L.envelopes(key, "alone")
    bM, bf = L.system_bounds(r64, env["M"], env["f"])
    pairs, loose = None, []
    if fl.robot == "two_joint" and fl.obs:     # attached points: (relative position, normal, distance) per leaf
        dl = D.distance_leaf_indices(desc)
        pairs = lambda r: {li: (fl.obs["p_link"][r, k:k + 1], fl.obs["p_obs"][r, k:k + 1], fl.obs["dist"][r, k:k + 1]) for k, li in enumerate(dl)}  # noqa: E731
    elif fl.obs:
        # (the table's own pairs: NaN where the control point sits on the centre, as the table's are)
        pp = fl.obs if "p_link" in fl.obs else L.explicit_pairs(fl.q, fl.obs["spheres"], keep_nan=True)
        K = pp["p_link"].shape[1] // 2
        dl = D.distance_leaf_indices(desc)
        pairs = lambda r: {li: (pp["p_link"][r, k * K:(k + 1) * K], pp["p_obs"][r, k * K:(k + 1) * K]) for k, li in enumerate(dl)}  # noqa: E731
    worst = [0.0, 0.0]
    for r in _autograd_rows(fl):
        goal = None if fl.goal is None else fl.goal[r]
        with np.errstate(all="ignore"):
            _, M, f = TA.evaluate_one(fk, leaves, fl.q[r], fl.qd[r], goal, pairs=None if pairs is None else pairs(r)) \
                if cls[r] != "pole" else _evaluate_pole(TA, fk, leaves, fl, r, goal, pairs)
        if cls[r] == "pole":
            assert not (np.isfinite(M).all() and np.isfinite(f).all()), f"{key} row {r} {fl.names[r]!r}: the restatement is finite on a pole row"
            continue
        sM = np.abs(M).max()
        eM = np.abs(r32["M"][r] - M).max()
        ef = np.abs(r32["f"][r] - f).max()
        sf = max(np.abs(f).max(), 1e-6 * sM)
        if sM > 0:
            worst[0] = max(worst[0], eM / (PIN_M * sM))
        if sf > 0:
            worst[1] = max(worst[1], ef / (PIN_F * sf))
        if np.abs(r32["M"][r] - r64["M"][r]).max() > PIN_M * sM or np.abs(r32["f"][r] - r64["f"][r]).max() > PIN_F * sf:
            loose.append(fl.names[r] or r)
            with np.errstate(invalid="ignore"):
                assert (np.abs(M - r64["M"][r]) <= bM[r]).all(), f"{key} row {r} {fl.names[r]!r}: M of the restatement outside the fp64 system's bound"
                assert (np.abs(f - r64["f"][r]) <= bf[r]).all(), f"{key} row {r} {fl.names[r]!r}: f of the restatement outside the fp64 system's bound"
            continue
        assert eM <= PIN_M * sM, f"{key} row {r} {fl.names[r]!r}: M differs by {eM:.3e} (scale {sM:.3e})"
        assert ef <= PIN_F * sf, f"{key} row {r} {fl.names[r]!r}: f differs by {ef:.3e} (scale {sf:.3e})"
    print(f"{key}: rows held to the fp64 system instead of the pin: {loose}")
    print(f"{key}: worst |M_c - M_autograd| / pin {worst[0]:.3f}, f {worst[1]:.3f}")


def test_the_restatements_distance_keeps_its_values_off_the_obstacle():
    """oracle/torch_autodiff_oracle.py forms the distance of a pair as sqrt(sum x^2), tf.norm's own graph (non-finite derivatives ON the
    obstacle point), where it used torch.linalg.norm (subgradient 0 there).  Off the obstacle point nothing pinned moves: value, Jacobian
    and curvature of the two forms agree to fp32 rounding on random pairs -- and the golden fixtures the restatement generated
    (tests/test_oracle_pins.py: configs 3 and 5, exp-05) keep passing at their pins."""
    import torch
    import torch_autodiff_oracle as TA
    rng = np.random.default_rng(5)
    pl = torch.tensor(rng.uniform(-1, 1, (64, 3)), dtype=torch.float32)
    po = torch.tensor(rng.uniform(-1, 1, (64, 3)), dtype=torch.float32)
    T = torch.eye(4).reshape(1, 16).repeat(64, 1)
    T[:, [3, 7, 11]] = torch.tensor(rng.uniform(-1, 1, (64, 3)), dtype=torch.float32)
    Td = torch.tensor(rng.uniform(-0.3, 0.3, (64, 16)), dtype=torch.float32)
    tm = TA.TaskmapJointFrame4x4ToDistance(pl, po)
    new = TA.rmp_differentiate(tm.forward)(T, Td)

    def old_forward(inp):
        pos = inp.reshape(-1, 4, 4)[:, :3, 3]
        return torch.linalg.norm(pos + (pl - pos).detach() - po, dim=-1)[:, None]
    old = TA.rmp_differentiate(old_forward)(T, Td)
    for a, b in zip(new, old):
        assert torch.isfinite(a).all() and (a - b).abs().max() <= 2e-6 * max(1.0, float(b.abs().max()))


def _evaluate_pole(TA, fk, leaves, fl, r, goal, pairs):
    """evaluate_one on a pole row: numpy's pinv refuses a non-finite system, which is all this test wants to know."""
    try:
        return TA.evaluate_one(fk, leaves, fl.q[r], fl.qd[r], goal, pairs=None if pairs is None else pairs(r))
    except np.linalg.LinAlgError:
        n = fl.n
        return np.full(n, np.nan), np.full((n, n), np.nan), np.full(n, np.nan)


def test_coinciding_limits_are_a_pole_of_every_row(hip_lib):
    """A JointLimitAvoidance descriptor in which one joint's limits coincide: rmp2_validate takes it (the reference's constructor
    does too), and d = 0 / 0 makes every row a pole on both oracle builds."""
    from riemannian_motion_policies_amd import _native
    fl = L.joint_limits(coincide=4)
    lib = _native.lib()
    lib.rmp2_validate.argtypes = [C.POINTER(type(fl.desc("alone")))]
    for shape in L.SHAPES:
        d = fl.desc(shape)
        assert lib.rmp2_validate(C.byref(d)) == 0, lib.rmp2_last_error(None)
    import oracle as O
    for shape in L.SHAPES:
        for prec in ("f32", "f64"):
            r = O.step(fl.desc(shape), fl.q, fl.qd, precision=prec)
            assert (~np.isfinite(r["qdd64"])).all() and (r["status"] & 1).all(), (shape, prec)

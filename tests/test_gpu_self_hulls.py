"""Hull-versus-hull self pairs on the GPU (include/rmp2.h rmp2_set_self_collision_hulls): the stage against the fp64 brute-force
restatement (tests/hull_pair_reference.py), the finger pairs' symmetry, the bound by the capsules, the staged step against the CPU
oracle, bit-exact composition with the hull obstacle stage, switching, the staged routes sharing one handle, the refusals and the class
surface."""
import ctypes as C
import os

import numpy as np
import pytest

import hull_pair_reference as HP
import hull_reference as H
from test_gpu_self_collision import _engine, _explicit, _gate, _interleave, _setup, self_pairs_np

pytestmark = pytest.mark.gpu

ATOL = 1e-5


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _meshes(golden_dir):
    z = np.load(os.path.join(golden_dir, "panda_collision_meshes.npz"))
    return {str(n): (z[f"{n}.vertices"], z[f"{n}.xyz"], z[f"{n}.rpy"]) for n in z["links"]}


_HULLS = {}


def _hulls(golden_dir):
    if "h" not in _HULLS:
        from riemannian_motion_policies_amd import urdf as U
        _HULLS["h"] = U.self_collision_hulls(U.PANDA_URDF, U.panda_table(), _meshes(golden_dir))
    return _HULLS["h"]


def _leaf_hulls(desc, hulls):
    from riemannian_motion_policies_amd import descriptor as D
    return hulls.subset([desc.leaves[i].frame for i in D.distance_leaf_indices(desc)])


def _sorted_pairs(pairs):
    """The pairs in the stage's order (leaf ordinal, then as given)."""
    return [pairs[k] for k in sorted(range(len(pairs)), key=lambda k: pairs[k][0])]


def _on_hull(hull, T, p):
    """Largest plane value of base-frame points p [N, 3] against a hull placed by T [N, 4, 4] (~0: on the surface)."""
    x = np.einsum("nji,nj->ni", T[:, :3, :3], p - T[:, :3, 3])
    return (x @ hull.P[:, :3].T - hull.P[:, 3]).max(1)


def _face_points_ok(pl, po, rpl, rpo):
    """Face-rule points [N, 3] (base frame) against the restatement's: the same n* = unit(p_link - p_obs), and p_obs on the same
    support plane n* . y = min -- y* is any vertex of B attaining the min (a face of B ties all its vertices)."""
    n, rn = pl - po, rpl - rpo
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    rn = rn / np.linalg.norm(rn, axis=1, keepdims=True)
    return (np.abs(n - rn).max(1) <= 1e-4) & (np.abs(((po - rpo) * rn).sum(1)) <= ATOL)


def _near_contact(desc, pairs, caps, q, n):
    _, _, _, gap = self_pairs_np(desc, pairs, caps, q)
    return np.argsort(gap.min(1))[:n]


_REF = {}


def _reference(config, golden_dir, q, key):
    """self_hull_pairs_np on q, cached per (config, key) -- the brute force is the slow part of this file."""
    if (config, key) not in _REF:
        table, desc, pairs, caps = _setup(config)
        _REF[(config, key)] = HP.self_hull_pairs_np(desc, _hulls(golden_dir), _sorted_pairs(pairs), q)
    return _REF[(config, key)]


@pytest.mark.parametrize("config", ["config3", "exp05_panda"])
def test_stage_vs_restatement(torch_mod, config, golden_dir):
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    table, desc, pairs, caps = _setup(config)
    hulls = _hulls(golden_dir)
    eng = _engine(desc)
    eng.set_self_collision_hulls(pairs, hulls)
    assert eng.self_counts == [5, 4, 4, 5, 4, 6, 8, 8] and eng.has_self_hulls
    rng = np.random.default_rng(7)
    s = Cf.sample_panda_states(rng, 4096)
    pl, po, dd = (t.cpu().numpy() for t in eng.self_pairs(torch.from_numpy(s["q"])))
    assert pl.shape == (4096, 44, 3) and dd.shape == (4096, 44)
    assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all()
    sub = np.unique(np.r_[np.arange(32), _near_contact(desc, pairs, caps, s["q"], 16)])
    rpl, rpo, rdd, gap, face = _reference(config, golden_dir, s["q"][sub], "stage")
    assert np.abs(dd[sub] - rdd).max() <= ATOL
    sp = _sorted_pairs(pairs)
    dl = D.distance_leaf_indices(desc)
    T = O.forward_kinematics(desc, s["q"][sub], "f64")
    F = desc.robot.n_frames
    for j, (o, b) in enumerate(sp):
        leaf = desc.leaves[dl[o]]
        point = leaf.taskmap == D.TASKMAP_FK_POINT
        HA, HB = HP.Hull(*hulls.hull(leaf.frame)), HP.Hull(*hulls.hull(F if b < 0 else b))
        TA = T[:, leaf.frame]
        TB = np.broadcast_to(np.eye(4), TA.shape) if b < 0 else T[:, b]
        # the face rule's points are only as determined as n*: where two faces tie, either is the rule's answer
        margin = np.array([HP.face_margin(HA, HB, TA[r, :3, :3].T @ TB[r, :3, :3], TA[r, :3, :3].T @ (TB[r, :3, 3] - TA[r, :3, 3]))
                           if face[r, j] else np.inf for r in range(len(sub))])
        det = margin > 1e-3
        well = (np.abs(gap[:, j]) > 1e-3) & det
        if point:   # relative_position (A's frame), normal_vec (unique where the hulls are apart), distance
            assert np.abs(po[sub, j] - rpo[:, j])[well].max(initial=0) <= ATOL, j
            other = (np.abs(pl[sub, j] - rpl[:, j]).max(1) > ATOL) & ~face[:, j]
            if other.any():   # another nearest point of A (parallel faces): on A's surface, at distance dist from B's hull
                x = pl[sub, j][other].astype(np.float64)
                assert np.abs((x @ HA.P[:, :3].T - HA.P[:, 3]).max(1)).max() <= ATOL, j
                xw = np.einsum("nij,nj->ni", TA[other, :3, :3], x) + TA[other, :3, 3]
                xb = np.einsum("nji,nj->ni", TB[other, :3, :3], xw - TB[other, :3, 3])
                _, _, _, gb = H.hull_closest(HB.V, HB.P, xb, xb, np.zeros(len(xb)))
                assert np.abs(gb - rdd[other, j]).max() <= ATOL, j
            continue
        # distance leaves: the direction (unique where the hulls are apart) and points.  Parallel faces (the fingers) make
        # the nearest points of two hulls a set: where the device's differ from the restatement's they must be a nearest
        # pair as well -- on their hulls and |p_link - p_obs| = dist
        u = pl[sub, j] - po[sub, j]
        ru = rpl[:, j] - rpo[:, j]
        n, rn = np.linalg.norm(u, axis=1), np.linalg.norm(ru, axis=1)
        assert np.abs(n - rdd[:, j]).max() <= ATOL, j
        assert np.abs(u / n[:, None] - ru / rn[:, None])[well].max(initial=0) <= 1e-3, j
        fd = face[:, j] & det
        assert _face_points_ok(pl[sub, j][fd], po[sub, j][fd], rpl[fd, j], rpo[fd, j]).all(), j
        diff = np.maximum(np.abs(pl[sub, j] - rpl[:, j]).max(1), np.abs(po[sub, j] - rpo[:, j]).max(1))
        other = (diff > ATOL) & ~face[:, j]
        if other.any():
            assert np.abs(_on_hull(HA, TA[other], pl[sub, j][other].astype(np.float64))).max() <= ATOL, j
            assert np.abs(_on_hull(HB, TB[other], po[sub, j][other].astype(np.float64))).max() <= ATOL, j


def test_stage_without_finger_leaves(torch_mod, golden_dir):
    """Leaves on config 3's frames up to the hand but not on the fingers: the step's pruned program is a chain, while the unpruned
    one the stage walks saves the hand's frame for its three children.  The fingers, paired as B, must come out of that save."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    t = U.panda_table()
    desc = _desc_with_distance_frames(t, Cf.CONTROL_POINT_FRAMES[:6])
    leaf_frames = [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]
    pairs = U.self_collision_pairs(t, leaf_frames)
    assert any(b in (t.frame_index("panda_finger_joint1"), t.frame_index("panda_finger_joint2")) for _, b in pairs)
    hulls = _hulls(golden_dir)
    eng = _engine(desc)
    eng.set_self_collision_hulls(pairs, hulls)
    q = Cf.sample_panda_states(np.random.default_rng(13), 32)["q"]
    pl, po, dd = (t_.cpu().numpy() for t_ in eng.self_pairs(torch.from_numpy(q)))
    rpl, rpo, rdd, gap, face = HP.self_hull_pairs_np(desc, hulls, _sorted_pairs(pairs), q)
    assert np.abs(dd - rdd).max() <= ATOL
    n = np.linalg.norm(pl - po, axis=2)
    assert np.abs(n - rdd).max() <= ATOL


def _desc_with_distance_frames(t, frames):
    """config 3's leaf set with its distance leaves on `frames` only."""
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    specs = [
        D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, t.frame_index("panda_grasptarget_hand"),
                   Cf.TARGET_ATTRACTOR_PARAMS, goal_len=3, name="attractor"),
        D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, Cf.JOINT_DAMPING_PARAMS, name="joint_damping"),
    ]
    for fr in frames:
        specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, t.frame_index(fr),
                                Cf.OBSTACLE_AVOIDANCE_PARAMS, name=f"collision_avoidance_for_{fr}"))
    return D.build_desc(t, specs, "auto")


def test_stage_face_rule(torch_mod, golden_dir):
    """The face rule on the device: the base link's hull blown up fourfold, so that the links paired with the base overlap it."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    table, desc, pairs, caps = _setup("config3")
    meshes = _meshes(golden_dir)
    V, xyz, rpy = meshes["panda_link0"]
    meshes["panda_link0"] = (V * 4.0, xyz, rpy)
    hulls = U.self_collision_hulls(U.PANDA_URDF, U.panda_table(), meshes)
    eng = _engine(desc)
    eng.set_self_collision_hulls(pairs, hulls)
    q = Cf.sample_panda_states(np.random.default_rng(3), 64)["q"]
    pl, po, dd = (t.cpu().numpy() for t in eng.self_pairs(torch.from_numpy(q)))
    sp = _sorted_pairs(pairs)
    js = [j for j, (o, b) in enumerate(sp) if b == -1]
    rpl, rpo, rdd, gap, face = HP.self_hull_pairs_np(desc, hulls, [sp[j] for j in js], q)
    assert face.mean() > 0.04 and (~face).any()
    assert np.abs(dd[:, js] - rdd).max() <= ATOL
    import oracle as O
    from riemannian_motion_policies_amd import descriptor as D
    T = O.forward_kinematics(desc, q, "f64")
    F = desc.robot.n_frames
    HB = HP.Hull(*hulls.hull(F))
    dl = D.distance_leaf_indices(desc)
    for c, j in enumerate(js):
        fa = desc.leaves[dl[sp[j][0]]].frame
        HA = HP.Hull(*hulls.hull(fa))
        margin = np.array([HP.face_margin(HA, HB, T[r, fa, :3, :3].T, -T[r, fa, :3, :3].T @ T[r, fa, :3, 3]) for r in range(len(q))])
        det = face[:, c] & (margin > 1e-3)
        assert _face_points_ok(pl[det, j], po[det, j], rpl[det, c], rpo[det, c]).all(), j
        apart = ~face[:, c] & (gap[:, c] > 1e-3)
        assert np.abs(dd[apart, j] - np.linalg.norm(pl[apart, j] - po[apart, j], axis=1)).max(initial=0) <= ATOL, j


def test_finger_symmetry_and_capsule_bound(torch_mod, golden_dir):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, pairs, caps = _setup("config3")
    eng = _engine(desc)
    eng.set_self_collision_hulls(pairs, _hulls(golden_dir))
    rng = np.random.default_rng(19)
    q = torch.from_numpy(Cf.sample_panda_states(rng, 4096)["q"])
    _, _, dd = (t.cpu().numpy() for t in eng.self_pairs(q))
    sp = _sorted_pairs(pairs)
    i, k = sp.index((6, 10)), sp.index((7, 9))                     # left finger vs right, and right vs left
    assert np.abs(dd[:, i] - dd[:, k]).max() <= ATOL
    cap = _engine(desc)
    cap.set_self_collision(pairs, caps)
    cpl, cpo, cdd = (t.cpu().numpy() for t in cap.self_pairs(q))
    _, _, _, cgap = self_pairs_np(desc, pairs, caps, q.numpy()[:256])
    # capsules contain their hulls: where the capsules are apart so are the hulls, no nearer than the capsules
    apart = cgap > 1e-4
    assert (dd[:256][apart] >= cdd[:256][apart] - ATOL).all()


@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("kernel", ["hex", "quad", "lane"])
@pytest.mark.parametrize("config", ["config3", "exp05_panda"])
def test_step_vs_oracle(torch_mod, config, kernel, solve, golden_dir):
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, pairs, caps = _setup(config, solve)
    eng = _engine(desc, kernel)
    eng.set_self_collision_hulls(pairs, _hulls(golden_dir))
    rng = np.random.default_rng(11)
    R = 2048
    s = Cf.sample_panda_states(rng, R)
    qdd = eng.step(torch.from_numpy(s["q"]), torch.from_numpy(s["qd"]), torch.from_numpy(s["goal"])).cpu().numpy()
    point = config == "exp05_panda"
    sub = slice(0, 64)
    pl, po, dd, gap, _ = _reference(config, golden_dir, s["q"][sub], "step")
    kw = _explicit(pl, po, dd, eng.self_counts, point)
    args = (desc, s["q"][sub], s["qd"][sub], s["goal"][sub])
    ref = O.step(*args, **kw)
    ok = _gate(qdd[sub], ref, gap.min(axis=1), f"{config}/{kernel}/{solve}", spread=O.fp32_resolution(*args, **kw))
    # robots in deep self contact: held to the gate on the stage's own pairs (as test_gpu_self_collision.test_step_vs_oracle)
    bad = ~ok
    assert bad.mean() <= 0.05, f"{config}/{kernel}/{solve}: {bad.sum()} robots beyond the gate on fp64 pairs"
    if bad.any():
        qb = s["q"][sub][bad]
        dpl, dpo, ddd = (t.cpu().numpy() for t in eng.self_pairs(torch.from_numpy(qb)))
        kw2 = _explicit(dpl, dpo, ddd, eng.self_counts, point)
        args2 = (desc, qb, s["qd"][sub][bad], s["goal"][sub][bad])
        ref2 = O.step(*args2, **kw2)
        ok2 = _gate(qdd[sub][bad], ref2, np.zeros(bad.sum()), f"{config}/{kernel}/{solve} device pairs",
                    spread=O.fp32_resolution(*args2, **kw2))
        assert ok2.all(), f"{config}/{kernel}/{solve}: {(~ok2).sum()} robots beyond the gate on the stage's own pairs"


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
@pytest.mark.parametrize("R", [1, 3000])
def test_composition_bit_equal(torch_mod, prim, R, golden_dir):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, pairs, caps = _setup("config3")
    hulls = _hulls(golden_dir)
    rng = np.random.default_rng(23 + R)
    s = Cf.sample_panda_states(rng, R)
    tab = Cf.sample_spheres(rng, 32) if prim == "sphere" else Cf.sample_capsules(rng, 32)
    eng = _engine(desc)
    eng.set_self_collision_hulls(pairs, hulls)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    t = torch.from_numpy(tab).cuda()
    got = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=t))
    # host composition: the hull obstacle stage of a handle whose link hulls are the same leaf hulls, the hull self pairs,
    # interleaved per leaf, an explicit-pair step of a plain handle
    lh = _engine(desc)
    lh.set_link_hulls(_leaf_hulls(desc, hulls))
    opl, opo, _ = lh.closest_points_hulls(q, lh.obstacles(spheres=t))
    spl, spo, _ = eng.self_pairs(q)
    counts = eng.self_counts
    pl, po = _interleave(torch, opl, opo, 32, spl, spo, counts)
    plain = _engine(desc)
    want = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=pl, p_obs=po, pair_counts=[32 + c for c in counts]))
    torch.cuda.synchronize()
    assert torch.equal(got, want), (got - want).abs().max().item()
    # obstacle input NONE: the self pairs alone
    got0 = eng.step(q, qd, goal)
    want0 = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=spl, p_obs=spo, pair_counts=counts))
    torch.cuda.synchronize()
    assert torch.equal(got0, want0)


def test_switching(torch_mod, golden_dir):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, pairs, caps = _setup("config3")
    hulls = _hulls(golden_dir)
    rng = np.random.default_rng(9)
    s = Cf.sample_panda_states(rng, 5000)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    sp = torch.from_numpy(Cf.sample_spheres(rng, 32)).cuda()
    step = lambda e: e.step(q, qd, goal, obstacles=e.obstacles(spheres=sp))    # noqa: E731
    eng, fresh, on_caps, on_hulls = _engine(desc), _engine(desc), _engine(desc), _engine(desc)
    on_caps.set_self_collision(pairs, caps)
    on_hulls.set_self_collision_hulls(pairs, hulls)
    want_caps, want_hulls, want_fresh = step(on_caps), step(on_hulls), step(fresh)
    eng.set_self_collision_hulls(pairs, hulls)
    assert torch.equal(step(eng), want_hulls)
    eng.set_self_collision(pairs, caps)                           # capsules replace the hulls
    assert torch.equal(step(eng), want_caps) and not eng.has_self_hulls
    eng.set_self_collision_hulls(pairs, hulls)                    # and back
    assert torch.equal(step(eng), want_hulls)
    eng.set_self_collision_hulls([], hulls)                       # off: a fresh handle, bit for bit
    assert torch.equal(step(eng), want_fresh) and eng.self_counts is None
    eng.set_self_collision_hulls(pairs, hulls)
    eng.set_self_collision([], None)                              # off through the capsule call
    assert torch.equal(step(eng), want_fresh)
    assert not torch.equal(want_hulls, want_fresh) and not torch.equal(want_hulls, want_caps)
    with pytest.raises(ValueError):
        eng.step(q, qd, goal)        # distance leaves and no obstacles: refused again once the self pairs are off


def test_staged_routes_share_the_handle(torch_mod, golden_dir):
    """One handle through every staged route in turn: its one stage buffer grows and is reused, and its one set of hull arrays is
    overwritten, across routes.  Each step is bit-equal to a fresh handle set up for that route alone."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    table, desc, pairs, caps = _setup("config3")
    hulls = _hulls(golden_dir)
    rng = np.random.default_rng(31)
    s = Cf.sample_panda_states(rng, 3000)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    sp = torch.from_numpy(Cf.sample_spheres(rng, 32)).cuda()
    cyl = torch.from_numpy(Cf.sample_cylinders(rng, 16)).cuda()
    lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).cuda()
    routes = [   # (route, setup of the handle, its obstacles, robots)
        ("link hulls", lambda e: e.set_link_hulls(_leaf_hulls(desc, hulls)), lambda e: e.obstacles(spheres=sp), 3000),
        ("self collision on capsules", lambda e: e.set_self_collision(pairs, caps), lambda e: e.obstacles(spheres=sp), 3000),
        ("hull self pairs", lambda e: e.set_self_collision_hulls(pairs, hulls), lambda e: e.obstacles(spheres=sp), 3000),
        ("staged link capsules", lambda e: None,
         lambda e: e.obstacles(spheres=cyl, primitive="cylinder", link_capsules=lc), 3000),
        ("link hulls, smaller fleet", lambda e: e.set_link_hulls(_leaf_hulls(desc, hulls)), lambda e: e.obstacles(spheres=sp), 1000),
    ]
    eng = _engine(desc)
    for name, setup, obstacles, R in routes:
        eng.set_link_hulls(None)
        eng.set_self_collision([], None)
        setup(eng)
        got = eng.step(q[:R], qd[:R], goal[:R], obstacles=obstacles(eng))
        fresh = _engine(desc)
        setup(fresh)
        want = fresh.step(q[:R], qd[:R], goal[:R], obstacles=obstacles(fresh))
        torch.cuda.synchronize()
        assert torch.equal(got, want), (name, (got - want).abs().max().item())


def test_refusals(torch_mod, golden_dir):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    from riemannian_motion_policies_amd._native import ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, Rmp2Error
    table, desc, pairs, caps = _setup("config3")
    hulls = _hulls(golden_dir)
    rng = np.random.default_rng(5)
    R = 64
    s = Cf.sample_panda_states(rng, R)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    sp = torch.from_numpy(Cf.sample_spheres(rng, 8)).cuda()
    eng = _engine(desc)
    eng.set_self_collision_hulls(pairs, hulls)

    def refused(fn, words, code=ERR_UNSUPPORTED):
        with pytest.raises(Rmp2Error) as e:
            fn()
        assert getattr(e.value, "code", None) == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    off = torch.zeros(R + 1, dtype=torch.int32)
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp, csr_offset=off, csr_index=torch.zeros(0))),
            ["self collision", "RAGGED"])
    cyl = torch.from_numpy(Cf.sample_cylinders(rng, 4)).cuda()
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=cyl, primitive="cylinder")), ["self collision", "CYLINDER"])
    pl = torch.zeros((R, 8, 3), device="cuda")
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(p_link=pl, p_obs=pl + 1)), ["self collision", "EXPLICIT_PAIRS"])
    lc = torch.zeros((8, 8), device="cuda")
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp, link_capsules=lc)), ["link_capsules", "hull self pairs"])
    refused(lambda: eng.rollout(q.clone(), qd.clone(), goal, obstacles=eng.obstacles(spheres=sp), n_control_steps=1),
            ["self collision", "rmp2_rollout"])
    other = _engine(desc)
    o1, o2 = D.Outputs(), D.Outputs()
    out1, out2 = torch.empty_like(q), torch.empty_like(q)
    o1.qdd, o2.qdd = out1.data_ptr(), out2.data_ptr()
    ob = eng.obstacles(spheres=sp)
    rc = eng._lib.rmp2_step_pair(eng._h, q.data_ptr(), qd.data_ptr(), goal.data_ptr(), 3, C.byref(ob), C.byref(o1), R,
                                 other._h, q.data_ptr(), qd.data_ptr(), goal.data_ptr(), 3, C.byref(ob), C.byref(o2), R, None)
    assert rc == ERR_UNSUPPORTED and b"rmp2_step_pair" in eng._lib.rmp2_last_error(eng._h)
    # link hulls on a handle with hull self pairs, and hull self pairs on a handle with link hulls
    refused(lambda: eng.set_link_hulls(_leaf_hulls(desc, hulls)), ["link hulls", "self collision"])
    lh = _engine(desc)
    lh.set_link_hulls(_leaf_hulls(desc, hulls))
    refused(lambda: lh.set_self_collision_hulls(pairs, hulls), ["hull self pairs", "link hulls"])
    # a table on a set with attached-point leaves
    _, desc5, pairs5, _ = _setup("exp05_panda")
    e5 = _engine(desc5)
    e5.set_self_collision_hulls(pairs5, hulls)
    refused(lambda: e5.step(q, qd, goal, obstacles=e5.obstacles(spheres=sp)), ["self collision", "attached-point"])
    # argument checks: the entry count, B = the leaf's own frame, an empty entry named by a pair, the limits
    e3 = _engine(desc)
    vo, v, fo, p = (np.ascontiguousarray(a) for a in (hulls.vert_offset, hulls.verts, hulls.face_offset, hulls.planes))
    arr = np.ascontiguousarray([(D.distance_leaf_indices(desc)[a], b) for a, b in pairs], np.int32)
    fn = e3._lib.rmp2_set_self_collision_hulls
    assert fn(e3._h, len(pairs), arr.ctypes.data, len(vo) - 2, vo.ctypes.data, v.ctypes.data, fo.ctypes.data, p.ctypes.data) \
        == ERR_INVALID_ARGUMENT
    with pytest.raises(Rmp2Error) as e:
        e3.set_self_collision_hulls([(0, 1)], hulls)
    assert e.value.code == ERR_INVALID_ARGUMENT
    with pytest.raises(Rmp2Error) as e:
        e3.set_self_collision_hulls([(0, 7)], hulls)             # frame 7 (panda_joint8) has no collision shape: empty entry
    assert e.value.code == ERR_INVALID_ARGUMENT and "empty" in str(e.value)
    big = np.ascontiguousarray(np.concatenate([v[:vo[1]], np.tile(v[:1], (600, 1))]), np.float32)   # entry 0: 752 vertices
    vo2 = np.ascontiguousarray(np.r_[0, vo[1:] + 600], np.int32)
    big = np.ascontiguousarray(np.concatenate([big, v[vo[1]:]]), np.float32)
    assert fn(e3._h, len(pairs), arr.ctypes.data, len(vo2) - 1, vo2.ctypes.data, big.ctypes.data, fo.ctypes.data, p.ctypes.data) \
        == ERR_INVALID_ARGUMENT
    assert b"RMP2_MAX_HULL_VERTICES" in e3._lib.rmp2_last_error(e3._h)
    assert e3.self_counts is None


def test_class_surface(torch_mod, golden_dir):
    """RmpCore.update_distances / Datamanager.update_device with self_hulls=: each frame's holders hold its K obstacle pairs on
    its hull followed by its hull self pairs; core.evaluate (fused and explicit routes) gives the q'' of the staged rmp2_step."""
    torch = torch_mod
    import sys
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    try:
        from test_gpu_dropin import _experiment06_core, _import_compat
    finally:
        sys.path.pop(0)
    fkine, data_manager, core, target_rmp, ee = _experiment06_core(_import_compat())
    hulls = _hulls(golden_dir)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    R, K = 2000, 32
    s = Cf.sample_panda_states(rng, R)
    q, qd = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["qd"]).to(dev)
    target_rmp.goal = torch.from_numpy(s["goal"]).to(dev)
    tab = torch.from_numpy(Cf.sample_spheres(rng, K)).to(dev)
    with pytest.raises(ValueError):
        data_manager.update_device(core, q, tab, link_capsules=torch.zeros((8, 8), device=dev), self_hulls=hulls)
    with pytest.raises(ValueError):
        data_manager.update_device(core, q, tab, link_hulls=_leaf_hulls(core.engine_for(q).desc, hulls), self_hulls=hulls)
    data_manager.update_device(core, q, tab, self_hulls=hulls)
    fused = core.evaluate(q, qd)
    assert core._stage._arrays is None                     # the step formed every pair itself
    eng = core.engine_for(q)
    counts = eng.self_counts
    assert counts == [5, 4, 4, 5, 4, 6, 8, 8] and eng.has_self_hulls
    staged = eng.step(q, qd, target_rmp.goal, obstacles=eng.obstacles(spheres=tab))
    torch.cuda.synchronize()
    assert torch.equal(fused, staged)
    for i, fr in enumerate(Cf.CONTROL_POINT_FRAMES):
        st = data_manager[fr]
        assert tuple(st["pos_on_link_in_base_frame"].value.shape) == (R, K + counts[i], 3), fr
    # the self half of a frame's holder is rmp2_self_pairs' output, the obstacle half rmp2_closest_points_hulls'
    spl, _, _ = eng.self_pairs(q)
    key = eng._self_key
    h0 = data_manager[Cf.CONTROL_POINT_FRAMES[0]]["pos_on_link_in_base_frame"].value
    assert eng._self_key is key and eng.has_self_hulls and not eng.has_link_hulls   # the list stayed on the handle (no re-upload)
    assert torch.equal(h0[:, K:], spl[:, :counts[0]])
    lh = _engine(eng.desc)
    lh.set_link_hulls(_leaf_hulls(eng.desc, hulls))
    opl, _, _ = lh.closest_points_hulls(q, lh.obstacles(spheres=tab))
    assert torch.equal(h0[:, :K], opl[:, :K])
    # explicit route (the holders read): same arrays, same step
    explicit = core.evaluate(q.clone(), qd)
    torch.cuda.synchronize()
    assert torch.equal(explicit, staged)
    # and the core without self collision again: the engine's list is off
    data_manager.update_device(core, q, tab)
    plain = core.evaluate(q, qd)
    assert eng.self_counts is None and not torch.equal(plain, staged)

"""Convex-hull link geometry on the GPU: the hull stage against the fp64 brute-force restatement (tests/hull_reference.py),
the bound against the fitted capsules, the staged step against the CPU oracle, bit-exact composition, switching off, the
refusals and the class surface."""
import ctypes as C
import os

import numpy as np
import pytest

import hull_reference as H

pytestmark = pytest.mark.gpu

ATOL = 1e-5


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _engine(desc, kernel=None):
    from riemannian_motion_policies_amd.engine import Engine
    old = os.environ.get("RMP2_KERNEL")
    if kernel is not None:
        os.environ["RMP2_KERNEL"] = kernel
    try:
        return Engine(desc, 0)
    finally:
        if kernel is not None:
            if old is None:
                os.environ.pop("RMP2_KERNEL")
            else:
                os.environ["RMP2_KERNEL"] = old


def _hulls(golden_dir, table):
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    z = np.load(os.path.join(golden_dir, "panda_collision_meshes.npz"))
    meshes = {str(n): (z[f"{n}.vertices"], z[f"{n}.xyz"], z[f"{n}.rpy"]) for n in z["links"]}
    return U.link_hulls(table, Cf.CONTROL_POINT_FRAMES, meshes)


def _setup(config, golden_dir, solve="auto"):
    from riemannian_motion_policies_amd import configs as Cf
    table, desc = getattr(Cf, config)(solve)
    return table, desc, _hulls(golden_dir, table)


def _table(rng, prim, K=32):
    from riemannian_motion_policies_amd import configs as Cf
    return Cf.sample_spheres(rng, K) if prim == "sphere" else Cf.sample_capsules(rng, K)


def _compare(got, want, gap, what):
    pl, po, dd = got
    rpl, rpo, rdd = want
    assert np.abs(pl - rpl).max() <= ATOL, (what, np.abs(pl - rpl).max())
    assert np.abs(dd - rdd).max() <= ATOL, (what, np.abs(dd - rdd).max())
    # directions: an attached point's normal_vec is a unit vector from the obstacle's axis to the hull; the fp32 frames put up to
    # ~1e-6 m on the obstacle's position in the leaf frame (a metre of lever arm), so it is resolved to 1e-5 where the pair is
    # 10 cm apart or more (and it flips sign with the gap)
    well = np.abs(gap) > 0.1
    assert np.abs(po - rpo)[well].max() <= ATOL, (what, np.abs(po - rpo)[well].max())


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
@pytest.mark.parametrize("config", ["config3", "exp05_panda"])
def test_stage_geometry(torch_mod, golden_dir, config, prim):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, hulls = _setup(config, golden_dir)
    eng = _engine(desc)
    eng.set_link_hulls(hulls)
    rng = np.random.default_rng(3)
    R, K = 2048, 32
    s = Cf.sample_panda_states(rng, R)
    tab = _table(rng, prim, K)
    got = [t.cpu().numpy() for t in eng.closest_points_hulls(torch.from_numpy(s["q"]).cuda(),
                                                             eng.obstacles(spheres=torch.from_numpy(tab).cuda()))]
    assert got[0].shape == (R, 8 * K, 3) and all(np.isfinite(g).all() for g in got)
    sub = np.r_[0:48, 2000:2048] if prim == "capsule" else np.r_[0:128, 1920:2048]
    rpl, rpo, rdd, gap = H.stage_np(desc, hulls, s["q"][sub], tab, prim)
    _compare([g[sub] for g in got], (rpl, rpo, rdd), gap, f"{config}/{prim}")
    assert (gap < 0).any() and (gap > 0).any()        # both rules ran


def test_constructed_pairs(torch_mod, golden_dir):
    """Centre inside the hull, a segment piercing it, contact at a vertex, an edge and a face, the centre on the surface, far
    pairs: spheres and capsules placed in the leaf frame of robot 0 and moved to the base frame."""
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, hulls = _setup("config3", golden_dir)
    q = Cf.PANDA_Q_READY.astype(np.float32)[None]
    T = O.forward_kinematics(desc, q, "f64")[0]
    o = 0                                                      # panda_joint2's link
    leaf = desc.leaves[4 + o]
    Rm, t = T[leaf.frame][:3, :3], T[leaf.frame][:3, 3]
    V, P = (x.astype(np.float64) for x in hulls.hull(o))
    ctr = V.mean(0)
    f = int(np.argmin(P[:, 3] - P[:, :3] @ ctr))                # the face nearest the centroid: its foot point is on the hull
    n0, d0 = P[f, :3], P[f, 3]
    on_face = ctr + (d0 - n0 @ ctr) * n0
    vtx = V[np.argmax(V @ np.array([1.0, 2.0, 3.0]))]
    e_dir = np.array([0.3, -1.0, 0.2])
    edge_pt = V[np.argmax(V @ e_dir)]
    spheres = [
        (ctr, 0.05),                                            # centre inside
        (ctr + 0.01 * n0, 0.02),                                # centre inside, near a face
        (on_face + 0.03 * n0, 0.02),                            # outside a face
        (vtx + 0.05 * np.array([1.0, 2.0, 3.0]) / np.sqrt(14), 0.02),   # beyond a vertex
        (edge_pt + 0.04 * e_dir / np.linalg.norm(e_dir), 0.01),         # beyond an edge region
        (ctr + np.array([2.0, 0.5, -1.0]), 0.1),                # far
    ]
    caps = [
        (ctr - np.array([0.0, 0.0, 0.5]), ctr + np.array([0.0, 0.0, 0.5]), 0.03),   # piercing
        (ctr + 0.5 * n0 + [0.2, 0.0, 0.0], ctr + 0.5 * n0 - [0.2, 0.0, 0.0], 0.03),
        (ctr + [3.0, 0.0, 0.0], ctr + [3.0, 1.0, 0.0], 0.05),                        # far
    ]
    to_base = lambda x: Rm @ x + t                             # noqa: E731
    sph = np.asarray([[*to_base(c), r] for c, r in spheres], np.float32)
    cap = np.asarray([[*to_base(a), r, *to_base(b), 0.0] for a, b, r in caps], np.float32)
    eng = _engine(desc)
    eng.set_link_hulls(hulls)
    for tab, kind in ((sph, "sphere"), (cap, "capsule")):
        got = [x.cpu().numpy() for x in eng.closest_points_hulls(torch.from_numpy(q).cuda(), eng.obstacles(spheres=torch.from_numpy(tab).cuda()))]
        rpl, rpo, rdd, gap = H.stage_np(desc, hulls, q, tab, kind)
        _compare(got, (rpl, rpo, rdd), gap, kind)
        K = len(tab)
        g0 = gap[0, o * K:(o + 1) * K]
        if kind == "sphere":
            assert g0[0] < 0 and g0[2] > 0 and g0[5] > 0, g0
        else:
            assert g0[0] < 0 and g0[2] > 0, g0


def test_hull_distance_bounds_the_capsule_distance(torch_mod, golden_dir):
    """A fitted capsule contains its hull: every hull distance is at least the capsule distance."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    table, desc, hulls = _setup("config3", golden_dir)
    eng = _engine(desc)
    eng.set_link_hulls(hulls)
    rng = np.random.default_rng(4)
    s = Cf.sample_panda_states(rng, 2048)
    q = torch.from_numpy(s["q"]).cuda()
    lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).cuda()
    tab = _table(rng, "sphere", 64)
    t = eng.obstacles(spheres=torch.from_numpy(tab).cuda())
    pl, po, dd = eng.closest_points_hulls(q, t)
    cpl, cpo = eng.closest_points(q, t, link_capsules=lc)
    hd = (pl - po).norm(dim=-1).cpu().numpy()
    cd = (cpl - cpo).norm(dim=-1).cpu().numpy()
    # signed capsule gap: the capsule's surface point lies outside the sphere exactly when the two are apart
    ctr = np.tile(tab[:, :3], (8, 1))[None].astype(np.float64)
    cap_out = np.linalg.norm(cpl.cpu().numpy() - ctr, axis=-1) >= np.tile(tab[:, 3], 8)[None]
    hull_out = (dd.cpu().numpy() > 0) & (np.linalg.norm(pl.cpu().numpy() - ctr, axis=-1) >= np.tile(tab[:, 3], 8)[None])
    g_cap = np.where(cap_out, cd, -cd)
    g_hull = np.where(hull_out, hd, -hd)
    assert (g_hull[cap_out] >= g_cap[cap_out] - 1e-5).all(), (g_cap - g_hull)[cap_out].max()
    assert (g_hull[cap_out] > g_cap[cap_out] + 1e-3).mean() > 0.5        # the hull is measurably tighter


def _gate(qdd, ref, what, spread=None):
    import oracle as O
    verdict = O.accuracy_gate(qdd, {k: ref[k] for k in ("qdd64", "M", "f")}, spread=spread)
    return verdict["ok"]


@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("kernel", ["hex", "quad", "lane"])
@pytest.mark.parametrize("config", ["config3", "exp05_panda"])
def test_step_vs_oracle(torch_mod, golden_dir, config, kernel, solve):
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, hulls = _setup(config, golden_dir, solve)
    eng = _engine(desc, kernel)
    eng.set_link_hulls(hulls)
    rng = np.random.default_rng(11)
    R, K = 2048, 16
    s = Cf.sample_panda_states(rng, R)
    tab = Cf.sample_spheres(rng, K)
    qdd = eng.step(torch.from_numpy(s["q"]), torch.from_numpy(s["qd"]), torch.from_numpy(s["goal"]),
                   obstacles=eng.obstacles(spheres=torch.from_numpy(tab).cuda())).cpu().numpy()
    point = config == "exp05_panda"
    sub = slice(0, 400)
    pl, po, dd, gap = H.stage_np(desc, hulls, s["q"][sub], tab, "sphere")
    kw = dict(p_link=pl.astype(np.float32), p_obs=po.astype(np.float32), pair_counts=[K] * 8)
    if point:
        kw["dist"] = dd.astype(np.float32)
    args = (desc, s["q"][sub], s["qd"][sub], s["goal"][sub])
    ref = O.step(*args, **kw)
    ok = _gate(qdd[sub], ref, f"{config}/{kernel}/{solve}", spread=O.fp32_resolution(*args, **kw))
    bad = ~ok
    assert bad.mean() <= 0.05, f"{config}/{kernel}/{solve}: {bad.sum()} robots beyond the gate on fp64 pairs"
    if bad.any():   # robots in deep contact: held to the gate on the stage's OWN pairs (their geometry: test_stage_geometry)
        qb = torch.from_numpy(s["q"][sub][bad]).cuda()
        dpl, dpo, ddd = (t.cpu().numpy() for t in eng.closest_points_hulls(qb, eng.obstacles(spheres=torch.from_numpy(tab).cuda())))
        kw2 = dict(p_link=dpl, p_obs=dpo, pair_counts=[K] * 8)
        if point:
            kw2["dist"] = ddd
        args2 = (desc, s["q"][sub][bad], s["qd"][sub][bad], s["goal"][sub][bad])
        ref2 = O.step(*args2, **kw2)
        ok2 = _gate(qdd[sub][bad], ref2, "device pairs", spread=O.fp32_resolution(*args2, **kw2))
        assert ok2.all(), f"{config}/{kernel}/{solve}: {(~ok2).sum()} robots beyond the gate on the stage's own pairs"


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
@pytest.mark.parametrize("config", ["config3", "exp05_panda"])
def test_composition_bit_equal(torch_mod, golden_dir, config, prim):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, hulls = _setup(config, golden_dir)
    rng = np.random.default_rng(23)
    R = 3000
    s = Cf.sample_panda_states(rng, R)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    t = torch.from_numpy(_table(rng, prim)).cuda()
    eng = _engine(desc)
    eng.set_link_hulls(hulls)
    got = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=t))
    pl, po, dd = eng.closest_points_hulls(q, eng.obstacles(spheres=t))
    plain = _engine(desc)
    want = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=pl, p_obs=po, dist=dd if config == "exp05_panda" else None))
    torch.cuda.synchronize()
    assert torch.equal(got, want), (got - want).abs().max().item()


def test_off_is_a_fresh_handle(torch_mod, golden_dir):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, hulls = _setup("config3", golden_dir)
    rng = np.random.default_rng(9)
    s = Cf.sample_panda_states(rng, 5000)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    sp = torch.from_numpy(Cf.sample_spheres(rng, 32)).cuda()
    eng, fresh = _engine(desc), _engine(desc)
    eng.set_link_hulls(hulls)
    with_hulls = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp))
    eng.set_link_hulls(None)
    a = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp))
    b = fresh.step(q, qd, goal, obstacles=fresh.obstacles(spheres=sp))
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert not torch.equal(with_hulls, b)


def test_refusals(torch_mod, golden_dir):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    from riemannian_motion_policies_amd._native import ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, Rmp2Error
    table, desc, hulls = _setup("config3", golden_dir)
    rng = np.random.default_rng(5)
    R = 64
    s = Cf.sample_panda_states(rng, R)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    sp = torch.from_numpy(Cf.sample_spheres(rng, 8)).cuda()
    eng = _engine(desc)
    eng.set_link_hulls(hulls)

    def refused(fn, words, code=ERR_UNSUPPORTED):
        with pytest.raises(Rmp2Error) as e:
            fn()
        assert getattr(e.value, "code", None) == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    off = torch.zeros(R + 1, dtype=torch.int32)
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp, csr_offset=off, csr_index=torch.zeros(0))),
            ["link hulls", "RAGGED"])
    cyl = torch.from_numpy(Cf.sample_cylinders(rng, 4)).cuda()
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=cyl, primitive="cylinder")), ["link hulls", "CYLINDER"])
    refused(lambda: eng.closest_points_hulls(q, eng.obstacles(spheres=cyl, primitive="cylinder")), ["link hulls", "CYLINDER"])
    pl = torch.zeros((R, 8, 3), device="cuda")
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(p_link=pl, p_obs=pl + 1)), ["link hulls", "EXPLICIT_PAIRS"])
    lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).cuda()
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp, link_capsules=lc)), ["link_capsules", "link hulls"])
    refused(lambda: eng.rollout(q.clone(), qd.clone(), goal, obstacles=eng.obstacles(spheres=sp), n_control_steps=1),
            ["link hulls", "rmp2_rollout"])
    other = _engine(desc)
    o1, o2 = D.Outputs(), D.Outputs()
    out1, out2 = torch.empty_like(q), torch.empty_like(q)
    o1.qdd, o2.qdd = out1.data_ptr(), out2.data_ptr()
    ob = eng.obstacles(spheres=sp)
    rc = eng._lib.rmp2_step_pair(eng._h, q.data_ptr(), qd.data_ptr(), goal.data_ptr(), 3, C.byref(ob), C.byref(o1), R,
                                 other._h, q.data_ptr(), qd.data_ptr(), goal.data_ptr(), 3, C.byref(ob), C.byref(o2), R, None)
    assert rc == ERR_UNSUPPORTED and b"rmp2_step_pair" in eng._lib.rmp2_last_error(eng._h)
    # self collision and hulls: refused either way round
    pairs = U.self_collision_pairs(table, [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)])
    caps = U.self_collision_capsules(U.PANDA_URDF, table)
    refused(lambda: eng.set_self_collision(pairs, caps), ["self collision", "link hulls"])
    e2 = _engine(desc)
    e2.set_self_collision(pairs, caps)
    refused(lambda: e2.set_link_hulls(hulls), ["link hulls", "self collision"])
    # limits and argument checks (library side)
    n = 8
    vo = np.arange(n + 1, dtype=np.int32) * (U.MAX_HULL_VERTICES + 1)
    fo = np.arange(n + 1, dtype=np.int32) * 4
    v = np.zeros((vo[-1], 3), np.float32)
    p = np.tile(np.asarray([[1.0, 0.0, 0.0, 1.0]], np.float32), (fo[-1], 1))
    e3 = _engine(desc)
    assert e3._lib.rmp2_set_link_hulls(e3._h, n, vo.ctypes.data, v.ctypes.data, fo.ctypes.data, p.ctypes.data) == ERR_INVALID_ARGUMENT
    assert b"RMP2_MAX_HULL_VERTICES" in e3._lib.rmp2_last_error(e3._h)
    vo = np.arange(n + 1, dtype=np.int32) * 4
    fo = np.arange(n + 1, dtype=np.int32) * (U.MAX_HULL_FACES + 1)
    v = np.zeros((vo[-1], 3), np.float32)
    p = np.tile(np.asarray([[1.0, 0.0, 0.0, 1.0]], np.float32), (fo[-1], 1))
    assert e3._lib.rmp2_set_link_hulls(e3._h, n, vo.ctypes.data, v.ctypes.data, fo.ctypes.data, p.ctypes.data) == ERR_INVALID_ARGUMENT
    assert b"RMP2_MAX_HULL_FACES" in e3._lib.rmp2_last_error(e3._h)
    assert e3._lib.rmp2_set_link_hulls(e3._h, 3, vo.ctypes.data, v.ctypes.data, fo.ctypes.data, p.ctypes.data) == ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        e3.closest_points_hulls(q, e3.obstacles(spheres=sp))      # hulls off
    # obstacle input NONE steps as without hulls (refused the same way for a set with distance leaves)
    with pytest.raises(ValueError):
        eng.step(q, qd, goal)


def test_class_surface(torch_mod, golden_dir):
    """RmpCore.update_distances / Datamanager.update_device with link_hulls=: the holders hold the hull stage's pairs; evaluate
    (fused route, explicit route from the holders, one robot from host arrays) gives the q'' of the Engine's hull step."""
    torch = torch_mod
    import sys
    from riemannian_motion_policies_amd import configs as Cf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tests"))
    try:
        from test_gpu_dropin import _experiment06_core, _import_compat
    finally:
        sys.path.pop(0)
    fkine, data_manager, core, target_rmp, ee = _experiment06_core(_import_compat())
    hulls = _hulls(golden_dir, fkine.table)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    R, K = 2000, 32
    s = Cf.sample_panda_states(rng, R)
    q, qd = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["qd"]).to(dev)
    target_rmp.goal = torch.from_numpy(s["goal"]).to(dev)
    tab = torch.from_numpy(Cf.sample_spheres(rng, K)).to(dev)
    with pytest.raises(ValueError):
        data_manager.update_device(core, q, tab, link_capsules=torch.zeros((8, 8), device=dev), link_hulls=hulls)
    data_manager.update_device(core, q, tab, link_hulls=hulls)
    fused = core.evaluate(q, qd)
    assert core._stage._arrays is None                     # the step ran the hull stage itself
    eng = core.engine_for(q)
    staged = eng.step(q, qd, target_rmp.goal, obstacles=eng.obstacles(spheres=tab))
    torch.cuda.synchronize()
    assert torch.equal(fused, staged)
    pl, po, _ = eng.closest_points_hulls(q, eng.obstacles(spheres=tab))
    h0 = data_manager[Cf.CONTROL_POINT_FRAMES[0]]["pos_on_link_in_base_frame"].value
    assert torch.equal(h0, pl[:, :K])
    explicit = core.evaluate(q.clone(), qd)
    torch.cuda.synchronize()
    assert torch.equal(explicit, staged)
    data_manager.update_device(core, q[3], tab, link_hulls=hulls)
    target_rmp.goal = s["goal"][3]
    one = core.evaluate(s["q"][3], s["qd"][3])
    want = staged[3].cpu().numpy()
    assert one.shape == (9,) and np.abs(np.asarray(one) - want).max() <= ATOL * max(1.0, np.abs(want).max())
    # back to capsules: the engine's hulls are off
    target_rmp.goal = torch.from_numpy(s["goal"]).to(dev)
    data_manager.update_device(core, q, tab)
    plain = core.evaluate(q, qd)
    assert not eng.has_link_hulls and not torch.equal(plain, staged)

"""GPU parity for the capsule primitive and the stand-alone closest-point stage (first
"next" row: the reference's CPU stage simulation.py:462-484 feeding taskmap.py:115-138).

Checker: the C oracle (capsule mode pinned against brute force and against the reference-faithful explicit-pair
mode in tests/test_oracle_pins.py).  Tolerance as in test_gpu_parity.py for robots with >= 0.05 m clearance.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ATOL = 1e-5


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _clearance(desc, q, caps):
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    T = O.forward_kinematics(desc, q, "f64")
    frames = [desc.leaves[i].frame for i in range(desc.n_leaves) if desc.leaves[i].taskmap == 2]
    org = T[:, frames][:, :, :3, 3]
    pl, po = Cf.pairs_from_capsules(org, caps)
    return org, np.linalg.norm(pl.astype(np.float64) - po, axis=-1).min(axis=1) if caps.shape[0] else None


def _step(torch, eng, s, **obs):
    o = eng.obstacles(**{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in obs.items()})
    st = torch.zeros(s["q"].shape[0], dtype=torch.int32, device="cuda")
    out = eng.step(torch.from_numpy(s["q"]), torch.from_numpy(s["qd"]), torch.from_numpy(s["goal"]), obstacles=o,
                   status=st)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _gate(qdd, ref, clr, what, scale=1.0, resolution=None):
    """Robots with >= 0.05 m clearance: the north-star tolerance (times `scale`).  EVERY other robot: oracle.accuracy_gate
    (`ref` = the dict of oracle.step, `resolution` = oracle.fp32_resolution of the same robots) -- none is exempted."""
    import oracle as O
    ref64 = ref["qdd64"]
    e = np.abs(qdd.astype(np.float64) - ref64).max(axis=1)
    mag = np.maximum(1.0, np.abs(ref64).max(axis=1))
    clear = clr >= 0.05
    assert clear.sum() >= 20, what
    assert (e[clear] <= scale * ATOL * mag[clear]).all(), f"{what}: clear robots worst {e[clear].max():.2e}"
    rest = ~clear
    if rest.any():
        verdict = O.accuracy_gate(qdd[rest], {k: ref[k][rest] for k in ("qdd64", "M", "f")},
                                  spread=None if resolution is None else resolution[rest])
        assert verdict["ok"].all(), f"{what}: near-contact robots {O.gate_summary(verdict)}"


@pytest.mark.parametrize("kernel", ["hex", "quad", "lane"])
@pytest.mark.parametrize("K", [9, 300])
def test_capsule_table_vs_oracle(torch_mod, kernel, K):
    """Shared capsule table: K=9 is staged in LDS, K=300 exceeds the 256-record LDS table (global reads)."""
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.engine import Engine
    rng = np.random.default_rng(40 + K)
    R = 500
    s = Cf.sample_panda_states(rng, R)
    caps = Cf.sample_capsules(rng, K)
    if K > 100:   # dense table: short thin capsules, so that a share of the robots keeps >= 0.05 m clearance
        mid, half = 0.5 * (caps[:, 0:3] + caps[:, 4:7]), 0.05 * (caps[:, 4:7] - caps[:, 0:3])
        caps[:, 0:3], caps[:, 4:7], caps[:, 3] = mid - half, mid + half, 0.1 * caps[:, 3]
    caps[0, 4:7] = caps[0, 0:3]                       # one degenerate capsule (a == b)
    _, desc = Cf.config3()
    old = os.environ.get("RMP2_KERNEL")
    os.environ["RMP2_KERNEL"] = kernel
    try:
        eng = Engine(desc, 0)
    finally:
        if old is None:
            del os.environ["RMP2_KERNEL"]
        else:
            os.environ["RMP2_KERNEL"] = old
    qdd, _ = _step(torch_mod, eng, s, spheres=caps)
    ref = O.step(desc, s["q"], s["qd"], s["goal"], spheres=caps)
    _, clr = _clearance(desc, s["q"], caps)
    # K = 300: 2400 pairs per robot are summed in fp32, serially in the oracle (like the reference's reduce_sum) and in
    # 4- / 16-way partial sums in the quad / hex kernels: the association order alone moves qdd by ~2e-5
    _gate(qdd, ref, clr, f"capsules K={K} {kernel}", scale=3.0 if K > 100 else 1.0,
          resolution=O.fp32_resolution(desc, s["q"], s["qd"], s["goal"], spheres=caps))


def test_ragged_capsules_vs_oracle(torch_mod):
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.engine import Engine
    rng = np.random.default_rng(77)
    R, K = 333, 9
    s = Cf.sample_panda_states(rng, R)
    caps = Cf.sample_capsules(rng, K)
    off, idx = Cf.sample_ragged(rng, R, K)
    _, desc = Cf.config3()
    eng = Engine(desc, 0)
    qdd, _ = _step(torch_mod, eng, s, spheres=caps, csr_offset=off, csr_index=idx)
    ref = O.step(desc, s["q"], s["qd"], s["goal"], spheres=caps, csr_offset=off, csr_index=idx)
    _, clr_all = _clearance(desc, s["q"], caps)      # conservative: clearance to the whole table
    _gate(qdd, ref, clr_all, "ragged capsules",
          resolution=O.fp32_resolution(desc, s["q"], s["qd"], s["goal"], spheres=caps, csr_offset=off, csr_index=idx))


def _engine_with(desc, kernel):
    """Engine created under RMP2_KERNEL=kernel (read at rmp2_create)."""
    from riemannian_motion_policies_amd.engine import Engine
    old = os.environ.get("RMP2_KERNEL")
    os.environ["RMP2_KERNEL"] = kernel
    try:
        return Engine(desc, 0)
    finally:
        if old is None:
            del os.environ["RMP2_KERNEL"]
        else:
            os.environ["RMP2_KERNEL"] = old


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
def test_closest_point_stage_feeds_explicit_pairs(torch_mod, prim):
    """rmp2_closest_points writes exactly the arrays the reference's Datamanager holds; (i) they match an
    independent fp64 numpy computation, (ii) fed back as EXPLICIT_PAIRS they reproduce the fused table mode."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd.engine import Engine
    rng = np.random.default_rng(5)
    R, K = 257, 9
    s = Cf.sample_panda_states(rng, R)
    table = Cf.sample_capsules(rng, K) if prim == "capsule" else Cf.sample_spheres(rng, K)
    _, desc = Cf.config3()
    eng = Engine(desc, 0)
    tab = eng.obstacles(spheres=torch.from_numpy(table))
    p_link, p_obs = eng.closest_points(torch.from_numpy(s["q"]), tab)
    torch.cuda.synchronize()
    as_caps = table if prim == "capsule" else np.concatenate([table, table[:, :3], np.zeros((K, 1), np.float32)], axis=1)
    org, clr = _clearance(desc, s["q"], as_caps)
    pl_ref, po_ref = Cf.pairs_from_capsules(org, as_caps)
    assert p_link.shape == (R, 8 * K, 3)
    assert np.abs(p_link.cpu().numpy() - pl_ref).max() < 2e-6
    assert np.abs(p_obs.cpu().numpy() - po_ref).max() < 2e-6
    # the lane-per-robot form of the stage (RMP2_KERNEL=lane; the fallback beyond 32 distance leaves) writes the same arrays
    pl1, po1 = _engine_with(desc, "lane").closest_points(torch.from_numpy(s["q"]), tab)
    assert (pl1 - p_link).abs().max().item() == 0.0 and (po1 - p_obs).abs().max().item() < 1e-6
    fused, _ = _step(torch, eng, s, spheres=table)
    o = eng.obstacles(p_link=p_link, p_obs=p_obs)
    fed = eng.step(torch.from_numpy(s["q"]), torch.from_numpy(s["qd"]), torch.from_numpy(s["goal"]), obstacles=o)
    torch.cuda.synchronize()
    fed = fed.cpu().numpy()
    clear = clr >= 0.05
    mag = np.maximum(1.0, np.abs(fused).max(axis=1))
    # the explicit form re-derives d = |p - p_obs| from rounded surface points: a few fp32 ulp of |p| in d
    assert (np.abs(fed - fused).max(axis=1)[clear] <= 5e-5 * mag[clear]).all()


def test_closest_points_abi_errors(torch_mod):
    import ctypes as C
    torch = torch_mod
    from riemannian_motion_policies_amd import _native, configs as Cf, descriptor as D
    from riemannian_motion_policies_amd.engine import Engine
    _, desc = Cf.config3()
    eng = Engine(desc, 0)
    lib = _native.lib()
    q = torch.zeros((4, 9), device="cuda")
    out = torch.zeros((4, 8, 3), device="cuda")
    o = D.Obstacles()
    o.mode = D.OBS_RAGGED_SPHERES
    assert lib.rmp2_closest_points(eng._h, q.data_ptr(), C.byref(o), out.data_ptr(), out.data_ptr(), 4, None) == -1
    assert b"SHARED_SPHERES" in lib.rmp2_last_error(eng._h)
    sph = torch.zeros((1, 4), device="cuda")
    o = eng.obstacles(spheres=sph)
    o.primitive = 7
    assert lib.rmp2_closest_points(eng._h, q.data_ptr(), C.byref(o), out.data_ptr(), out.data_ptr(), 4, None) == -1
    qd = torch.zeros_like(q)
    res = D.Outputs()
    res.qdd = torch.zeros_like(q).data_ptr()
    g = torch.zeros((4, 3), device="cuda")
    assert lib.rmp2_step(eng._h, q.data_ptr(), qd.data_ptr(), g.data_ptr(), 3, C.byref(o), C.byref(res), 4, None) == -1
    assert b"primitive" in lib.rmp2_last_error(eng._h)


@pytest.mark.parametrize("prim", ["spheres", "capsules"])
@pytest.mark.parametrize("robot", ["panda", "two_joint"])
def test_closest_points_with_link_geometry(torch_mod, prim, robot):
    """rmp2_closest_points_links: per pair the nearest points of the LINK's capsule and the obstacle primitive (what the
    reference gets from PyBullet for the link's collision shape, simulation.py:462-484), against the fp64 closed form
    (itself pinned by a brute-force scan in tests/test_oracle_pins.py); the pairs then drive the explicit-pair step, whose
    result must equal the oracle's on the same pairs."""
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    rng = np.random.default_rng(77)
    R, K = 97, 9
    if robot == "panda":
        table, desc = Cf.config3()
        s = Cf.sample_panda_states(rng, R)
        lc = U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)
    else:
        table, desc = Cf.config5_two_joint()
        s = Cf.sample_two_joint_states(rng, R)
        lc = U.link_capsules(U.TWO_JOINT_URDF, table, Cf.TWO_JOINT_CONTROL_POINT_FRAMES)   # boxes / cylinders of the URDF
        assert np.allclose(lc[0], [0.05, 0, 0, 0.05, 0.95, 0, 0, 0])
    tab = Cf.sample_spheres(rng, K) if prim == "spheres" else Cf.sample_capsules(rng, K)
    tab[:, 2] += np.float32(0.9)     # above the arms: clear of contact, the pairs stay well conditioned
    if prim == "capsules":
        tab[:, 6] += np.float32(0.9)
    eng = Engine(desc, 0)
    t_dev = eng.obstacles(spheres=torch.from_numpy(tab))
    pl, po = eng.closest_points(torch.from_numpy(s["q"]), t_dev, link_capsules=torch.from_numpy(lc))
    T = O.forward_kinematics(desc, s["q"], precision="f64")
    frames = [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]
    pl_ref, po_ref = Cf.pairs_from_link_capsules(T[:, frames], lc, tab)
    # the DISTANCE of a pair is well conditioned; WHERE along two nearly parallel axes the nearest points sit is not (the
    # fitted Panda capsules meet the capsule table at every angle): 2e-6 for the distance, 2e-5 for the points
    pln, pon = pl.cpu().numpy(), po.cpu().numpy()
    assert np.abs(pln - pl_ref).max() < 2e-5 and np.abs(pon - po_ref).max() < 2e-5
    assert np.abs(np.linalg.norm(pln - pon, axis=-1) - np.linalg.norm(pl_ref.astype(np.float64) - po_ref, axis=-1)).max() < 2e-6
    pl1, po1 = _engine_with(desc, "lane").closest_points(torch.from_numpy(s["q"]), t_dev, link_capsules=torch.from_numpy(lc))
    assert (pl1 - pl).abs().max().item() < 1e-6 and (po1 - po).abs().max().item() < 1e-6   # lane-per-robot form of the stage
    # the control points really differ from the frame origins, pair by pair
    pl0, _ = eng.closest_points(torch.from_numpy(s["q"]), t_dev)
    assert (pl - pl0).abs().max().item() > 0.03
    # ... and feed the reference-faithful explicit-pair step
    qdd = eng.step(torch.from_numpy(s["q"]), torch.from_numpy(s["qd"]), torch.from_numpy(s["goal"]),
                   obstacles=eng.obstacles(p_link=pl, p_obs=po))
    torch.cuda.synchronize()
    ref = O.step(desc, s["q"], s["qd"], s["goal"], p_link=pl.cpu().numpy(), p_obs=po.cpu().numpy())
    ok = np.linalg.cond(ref["M"]) < 100 if robot == "two_joint" else np.ones(R, bool)
    err = np.abs(qdd.cpu().numpy() - ref["qdd64"]).max(axis=1)
    tol = 1e-5 * np.maximum(1.0, np.abs(ref["qdd64"]).max(axis=1))
    assert (err[ok] <= tol[ok]).all() and ok.sum() > R // 3, f"worst {err[ok].max():.2e}"
    if not ok.all():   # the ill-conditioned TwoJoint robots are bounded too (oracle.accuracy_gate: backward error / fp32 resolution)
        rest = ~ok
        kw = dict(p_link=pl.cpu().numpy()[rest], p_obs=po.cpu().numpy()[rest])
        verdict = O.accuracy_gate(qdd.cpu().numpy()[rest], {k: ref[k][rest] for k in ("qdd64", "M", "f")},
                                  spread=O.fp32_resolution(desc, s["q"][rest], s["qd"][rest], s["goal"][rest], **kw))
        assert verdict["ok"].all(), f"cond >= 100: {O.gate_summary(verdict)}"


@pytest.mark.parametrize("prim", ["spheres", "capsules"])
@pytest.mark.parametrize("robot,R", [("panda", 97), ("panda", 65536), ("two_joint", 333), ("two_joint", 40000)])
def test_link_geometry_fused_into_the_step(torch_mod, prim, robot, R):
    """rmp2_obstacles.link_capsules: the closest points of every (link capsule, obstacle) pair are formed INSIDE the step (table
    in LDS, in-range pairs only) instead of being written out by rmp2_closest_points_links and read back as explicit pairs.
    Same numbers as that two-kernel flow and as the oracle on the fp64 closed-form pairs; small grids (latency build) and
    fleets (two waves per SIMD), spheres and capsules, through a rollout as well."""
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    rng = np.random.default_rng(123)
    K = 32 if prim == "spheres" else 12   # (the capsules are half a metre long: a dozen of them is as crowded as the sphere clutter)
    if robot == "panda":
        table, desc = Cf.config3()
        s = Cf.sample_panda_states(rng, R)
        lc = U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)
    else:
        table, desc = Cf.config5_two_joint()
        s = Cf.sample_two_joint_states(rng, R)
        lc = U.link_capsules(U.TWO_JOINT_URDF, table, Cf.TWO_JOINT_CONTROL_POINT_FRAMES)
    tab = Cf.sample_spheres(rng, K) if prim == "spheres" else Cf.sample_capsules(rng, K)
    lift = np.float32(0.45 if prim == "spheres" else (0.6 if robot == "panda" else 0.35))   # partly above the arms: a mix of in-range and culled pairs, few contacts
    tab[:, 2] += lift
    if prim == "capsules":
        tab[:, 6] += lift
    eng = Engine(desc, 0)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    tab_t, lc_t = torch.from_numpy(tab).cuda(), torch.from_numpy(lc).cuda()
    st = torch.zeros(R, dtype=torch.int32, device="cuda")
    fused = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=tab_t, link_capsules=lc_t), status=st)
    assert "quad" in eng.last_kernel()
    # the two-kernel flow on the GPU
    pl, po = eng.closest_points(q, eng.obstacles(spheres=tab_t), link_capsules=lc_t)
    two = eng.step(q, qd, goal, obstacles=eng.obstacles(p_link=pl, p_obs=po))
    torch.cuda.synchronize()
    fused_np, two_np = fused.cpu().numpy(), two.cpu().numpy()
    # clearance of every pair (surface to surface): parity is asserted for robots clear of contact, as everywhere
    clr = (torch.linalg.norm(pl - po, dim=-1)).min(dim=1).values.cpu().numpy()
    ok = clr >= 0.05
    n_chk = min(R, 512)
    sub = np.arange(R)[ok][:n_chk]
    assert len(sub) > n_chk // 4, f"only {len(sub)} robots clear of contact"
    T = O.forward_kinematics(desc, s["q"][sub], precision="f64")
    frames = [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]
    pl_ref, po_ref = Cf.pairs_from_link_capsules(T[:, frames], lc, tab)
    ref = O.step(desc, s["q"][sub], s["qd"][sub], s["goal"][sub], p_link=pl_ref.astype(np.float32), p_obs=po_ref.astype(np.float32))
    well = np.linalg.cond(ref["M"]) < 100 if robot == "two_joint" else np.ones(len(sub), bool)
    mag = np.maximum(1.0, np.abs(ref["qdd64"]).max(axis=1))
    err = np.abs(fused_np[sub] - ref["qdd64"]).max(axis=1)
    assert (err[well] <= 3e-5 * mag[well]).all() and well.sum() > len(sub) // 4, f"vs oracle: worst {(err / mag)[well].max():.2e}"
    if not well.all():   # ill-conditioned TwoJoint robots: bounded by the backward error / their fp32 resolution, not exempted
        rest = ~well
        kw = dict(p_link=pl_ref.astype(np.float32)[rest], p_obs=po_ref.astype(np.float32)[rest])
        verdict = O.accuracy_gate(fused_np[sub][rest], {k: ref[k][rest] for k in ("qdd64", "M", "f")},
                                  spread=O.fp32_resolution(desc, s["q"][sub][rest], s["qd"][sub][rest], s["goal"][sub][rest], **kw))
        assert verdict["ok"].all(), f"cond >= 100: {O.gate_summary(verdict)}"
    magf = np.maximum(1.0, np.abs(two_np).max(axis=1))
    # every robot clear of contact is finite in the two-kernel flow too (a non-finite row there is a finding, not a row to drop)
    assert np.isfinite(two_np[ok]).all(), f"stage + explicit pairs: non-finite qdd on clear robots {np.nonzero(ok & ~np.isfinite(two_np).all(axis=1))[0][:8]}"
    okf = ok.copy()
    if robot == "two_joint":
        okf[sub[~well]] = False
        okf[np.setdiff1d(np.arange(R), sub)] = False
    # fused form against the two-kernel flow: each is bounded against the oracle -- the fused form above, the two-kernel flow
    # here on the pairs ITS stage wrote (oracle.accuracy_gate: north-star bound, else backward error / fp32 resolution) --, and
    # the two agree with each other far inside what a wrong control point would cost (> 1e-3, asserted below).  (Round 3 held
    # them to 5e-5 of each other; with the capsules fitted to the Panda's meshes -- 5 to 10 cm radii instead of the 6 cm
    # stand-ins -- more pairs sit at a few centimetres, where two fp32 evaluations differ by more than that.)
    okn = np.arange(R)[okf][:n_chk]
    kw2 = dict(p_link=pl[okn].cpu().numpy(), p_obs=po[okn].cpu().numpy())
    ref2 = O.step(desc, s["q"][okn], s["qd"][okn], s["goal"][okn], **kw2)
    v2 = O.accuracy_gate(two_np[okn], ref2, spread=O.fp32_resolution(desc, s["q"][okn], s["qd"][okn], s["goal"][okn], **kw2))
    assert v2["ok"].all(), f"stage + explicit pairs vs oracle: {O.gate_summary(v2)}"
    errf = np.abs(fused_np - two_np).max(axis=1)
    assert (errf[okf] <= 5e-4 * magf[okf]).all(), f"vs stage + explicit pairs: worst {(errf / magf)[okf].max():.2e}"
    assert ((st.cpu().numpy()[okf] & 1) == 0).all()
    # the control points differ from the frame origins: the plain table mode gives other numbers
    plain = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=tab_t)).cpu().numpy()
    assert np.abs(plain - fused_np)[okf].max() > 1e-3
    # through the fused rollout (general flavour with the rotation records)
    if R < 1000:
        qa, qda = q.clone(), qd.clone()
        for _ in range(3):
            a = eng.step(qa, qda, goal, obstacles=eng.obstacles(spheres=tab_t, link_capsules=lc_t))
            for _ in range(5):
                qda = qda + 0.01 * a
                qa = qa + 0.01 * qda
        qb, qdb = q.clone(), qd.clone()
        eng.rollout(qb, qdb, goal, obstacles=eng.obstacles(spheres=tab_t, link_capsules=lc_t), n_control_steps=3, substeps=5, dt=0.01)
        torch.cuda.synchronize()
        fin = torch.isfinite(qa).all(dim=1) & torch.isfinite(qb).all(dim=1) & torch.from_numpy(okf).cuda()
        assert ((qa - qb).abs().max(dim=1).values[fin] < 1e-4).all()


def test_link_geometry_argument_errors(torch_mod):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    from riemannian_motion_policies_amd import _native
    from riemannian_motion_policies_amd.engine import Engine
    table, desc = Cf.config3()
    eng = Engine(desc, 0)
    rng = np.random.default_rng(1)
    s = Cf.sample_panda_states(rng, 8)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).cuda()
    with pytest.raises(ValueError):
        eng.obstacles(spheres=torch.zeros(4, 4), link_capsules=lc[:3])            # one capsule per distance leaf
    with pytest.raises(ValueError):
        eng.obstacles(p_link=torch.zeros(8, 8, 3), p_obs=torch.zeros(8, 8, 3), link_capsules=lc)
    big = torch.from_numpy(Cf.sample_spheres(rng, 300)).cuda()                      # beyond the LDS-resident table
    # (round 5: beyond the fused form's limits a plain step over a shared table runs as the stage + the explicit-pair step, inside
    #  the library; a ROLLOUT there is still refused)
    staged = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=big, link_capsules=lc))
    pl_, po_ = eng.closest_points(q, eng.obstacles(spheres=big), link_capsules=lc)
    two = eng.step(q, qd, goal, obstacles=eng.obstacles(p_link=pl_, p_obs=po_))
    torch.cuda.synchronize()
    assert torch.equal(staged, two)
    with pytest.raises(_native.Rmp2Error, match="link_capsules"):
        eng.rollout(q.clone(), qd.clone(), goal, obstacles=eng.obstacles(spheres=big, link_capsules=lc), n_control_steps=2)
    # solve = pinv: served since round 4 where the quad mapping certifies full rank per robot (the same numbers as AUTO on these
    # well-conditioned robots); still refused where the strict step is two kernels (here forced: RMP2_STRICT_CERTIFY=0)
    _, dpinv = Cf.config3("pinv")
    ep = Engine(dpinv, 0)
    a = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=big[:8], link_capsules=lc))
    b = ep.step(q, qd, goal, obstacles=ep.obstacles(spheres=big[:8], link_capsules=lc))
    torch.cuda.synchronize()
    assert "certified" in ep.last_kernel() and torch.equal(a, b)
    os.environ["RMP2_STRICT_CERTIFY"] = "0"
    try:
        e2 = Engine(dpinv, 0)
    finally:
        del os.environ["RMP2_STRICT_CERTIFY"]
    c = e2.step(q, qd, goal, obstacles=e2.obstacles(spheres=big[:8], link_capsules=lc))     # (all-Jacobi PINV: stage + explicit pairs)
    torch.cuda.synchronize()
    assert "pinv_kernel" in e2.last_kernel() and (c - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize("case", ["big_table", "all_jacobi_pinv", "cylinders", "empty_lists"])
def test_link_geometry_over_ragged_lists_beyond_the_fused_limits(torch_mod, case):
    """Ragged lists + link geometry where the fused form does not apply (a table beyond 256 primitives, the all-Jacobi PINV, a
    cylinder table): rmp2_step runs the closest-point stage over the whole table, lays out one pair per LIST ENTRY (a repeated
    index counts twice, as the fused list walk counts it; filler pairs far away up to the fleet's longest list) and takes the
    explicit-pair step.  Checked bit for bit against the same three pieces called one by one from the host -- the stage
    (`closest_points`), the gather in numpy, the explicit-pair step -- and against the fused form where both apply."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    from riemannian_motion_policies_amd import _native
    from riemannian_motion_policies_amd.engine import Engine
    rng = np.random.default_rng({"big_table": 1, "all_jacobi_pinv": 2, "cylinders": 3, "empty_lists": 4}[case])
    R = 77
    certify_off = case == "all_jacobi_pinv"
    table, desc = Cf.config3("pinv" if certify_off else "auto")
    if certify_off:
        os.environ["RMP2_STRICT_CERTIFY"] = "0"
    try:
        eng = Engine(desc, 0)
    finally:
        os.environ.pop("RMP2_STRICT_CERTIFY", None)
    s = Cf.sample_panda_states(rng, R)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).cuda()
    n_dist = lc.shape[0]
    K = 300 if case in ("big_table", "empty_lists") else 12   # (a table beyond the fused form's 256: the staged route)
    prim = None
    if case == "cylinders":
        tab = np.stack([Cf.cylinder_record(rng.uniform(-0.6, 0.6, 3) + [0, 0, 0.5], rng.uniform(-1, 1, 3), 0.05, 0.3) for _ in range(K)])
        tab, prim = tab.astype(np.float32), "cylinder"
    else:
        tab = Cf.sample_spheres(rng, K)
        tab[:, 2] += np.float32(0.5)
    counts = rng.integers(0, 9, size=R)
    if case == "empty_lists":
        counts[:] = 0
    else:
        counts[:8] = np.maximum(counts[:8], 2)
    lists = [rng.permutation(K)[:c] for c in counts]
    for r in range(8):
        if len(lists[r]) >= 2:
            lists[r][1] = lists[r][0]                                               # a repeated index: counted twice
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    idx = (np.concatenate(lists) if off[-1] else np.zeros(1)).astype(np.int32)
    kw = dict(primitive=prim) if prim else {}
    tabt = torch.from_numpy(tab).cuda()
    obs = eng.obstacles(spheres=tabt, csr_offset=torch.from_numpy(off), csr_index=torch.from_numpy(idx), link_capsules=lc, **kw)
    got = eng.step(q, qd, goal, obstacles=obs)
    torch.cuda.synchronize()
    # the same three pieces from the host
    pl_all, po_all = eng.closest_points(q, eng.obstacles(spheres=tabt, **kw), link_capsules=lc)   # [R, n_dist * K, 3]
    pl_all, po_all = pl_all.cpu().numpy(), po_all.cpu().numpy()
    L = max(int(counts.max()), 1)
    pl = np.repeat(pl_all.reshape(R, n_dist, K, 3)[:, :, :1], L, axis=2).copy()       # filler: the leaf's first control point ...
    po = pl.copy()
    po[..., 0] += np.float32(1.0e9)                                                    # ... and an obstacle point 1e9 m from it
    for r in range(R):
        for t, b in enumerate(lists[r]):
            pl[r, :, t] = pl_all.reshape(R, n_dist, K, 3)[r, :, b]
            po[r, :, t] = po_all.reshape(R, n_dist, K, 3)[r, :, b]
    two = eng.step(q, qd, goal, obstacles=eng.obstacles(p_link=torch.from_numpy(pl.reshape(R, n_dist * L, 3)).cuda(),
                                                        p_obs=torch.from_numpy(po.reshape(R, n_dist * L, 3)).cuda()))
    torch.cuda.synchronize()
    assert torch.equal(got, two)
    assert torch.isfinite(got).all()
    if case == "empty_lists":
        # nothing in range anywhere: the answer of the set without its distance leaves' obstacles far away
        far = eng.step(q, qd, goal, obstacles=eng.obstacles(p_link=torch.zeros(R, n_dist, 3).cuda(), p_obs=torch.full((R, n_dist, 3), 1.0e3).cuda()))
        torch.cuda.synchronize()
        assert (far - got).abs().max().item() <= 1e-6 * max(1.0, far.abs().max().item())
    if case == "all_jacobi_pinv":
        # the fused form of the certifying PINV handle answers the same lists
        _, dp = Cf.config3("pinv")
        ep = Engine(dp, 0)
        fused = ep.step(q, qd, goal, obstacles=ep.obstacles(spheres=tabt, csr_offset=torch.from_numpy(off), csr_index=torch.from_numpy(idx),
                                                            link_capsules=lc))
        torch.cuda.synchronize()
        # (per robot: the two routes round the closest points differently -- the stage writes fp32 points to HBM, the fused form
        #  keeps the clamped segment parameter in registers -- and a robot in near contact (|qdd| ~ 1e3 here) amplifies a rounding
        #  of its clearance; the well-conditioned robots agree to a few ulps)
        rel = (fused - got).abs().amax(1) / fused.abs().amax(1).clamp(min=1.0)
        print("fused vs staged, per robot:", "median %.2e" % rel.median().item(), "max %.2e" % rel.max().item(),
              "|qdd| of the worst %.1f" % fused.abs().amax(1)[rel.argmax()].item())
        assert (rel <= 2e-5).float().mean().item() >= 0.9 and rel.max().item() <= 1e-3
    # the list lengths are read back: refused inside a stream capture (and the handle stays usable)
    side, g, scratch, refused = torch.cuda.Stream(), torch.cuda.CUDAGraph(), torch.empty(4, device="cuda"), None
    with torch.cuda.graph(g, stream=side):
        scratch.zero_()   # (something to capture: the refused call must leave the capture itself intact)
        try:
            eng.step(q, qd, goal, obstacles=obs)
        except _native.Rmp2Error as e:
            refused = str(e)
    torch.cuda.synchronize()
    assert refused is not None and "stream capture" in refused
    again = eng.step(q, qd, goal, obstacles=obs)
    torch.cuda.synchronize()
    assert torch.equal(again, got)
    # a rollout there is still refused
    with pytest.raises(_native.Rmp2Error, match="link_capsules|cylinder"):
        eng.rollout(q.clone(), qd.clone(), goal, obstacles=obs, n_control_steps=2)


@pytest.mark.parametrize("prim,K", [("spheres", 32), ("spheres", 48), ("capsules", 12), ("spheres", 80)])
@pytest.mark.parametrize("robot,R", [("panda", 333), ("two_joint", 20000)])
def test_link_geometry_over_ragged_lists(torch_mod, prim, K, robot, R):
    """Link geometry inside the step for fleets whose robots see DIFFERENT obstacles (BASELINE config 5's ragged lists; round 3
    took shared tables only): the robot's CSR list as a membership mask over a table of <= 64 primitives, the list walk beyond
    and for a list that repeats an index (the reference would count that obstacle twice).  Oracle: explicit pairs in fp64 numpy
    (configs.pairs_from_link_capsules) holding, per robot and leaf, one pair per LIST ENTRY and far-away filler pairs (metric
    exactly 0) up to the longest list."""
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    from riemannian_motion_policies_amd.engine import Engine
    rng = np.random.default_rng(1000 * K + R)
    if robot == "panda":
        table, desc = Cf.config3()
        s = Cf.sample_panda_states(rng, R)
        lc = U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)
        lift = 0.5
    else:
        table, desc = Cf.config5_two_joint()
        s = Cf.sample_two_joint_states(rng, R)
        lc = U.link_capsules(U.TWO_JOINT_URDF, table, Cf.TWO_JOINT_CONTROL_POINT_FRAMES)
        lift = 0.35
    tab = Cf.sample_spheres(rng, K) if prim == "spheres" else Cf.sample_capsules(rng, K)
    tab[:, 2] += np.float32(lift)
    if prim == "capsules":
        tab[:, 6] += np.float32(lift)
    # ragged lists k_r ~ U{0..min(K, 24)}; the first 16 robots' lists repeat an index (their wave takes the list walk)
    kmax = min(K, 24)
    counts = rng.integers(0, kmax + 1, size=R)
    counts[:16] = np.maximum(counts[:16], 2)
    lists = [rng.permutation(K)[:c] for c in counts]
    for r in range(16):
        lists[r][1] = lists[r][0]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    idx = (np.concatenate(lists) if off[-1] else np.zeros(1)).astype(np.int32)
    eng = Engine(desc, 0)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    obs = eng.obstacles(spheres=torch.from_numpy(tab), csr_offset=torch.from_numpy(off), csr_index=torch.from_numpy(idx),
                        link_capsules=torch.from_numpy(lc))
    got = eng.step(q, qd, goal, obstacles=obs)
    torch.cuda.synchronize()
    assert "quad" in eng.last_kernel()
    # oracle on a sample: the listed pairs, padded with far pairs
    sub = np.unique(np.concatenate([np.arange(32), rng.integers(0, R, 96)]))
    frames = [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]
    T = O.forward_kinematics(desc, s["q"][sub], precision="f64")
    pl_all, po_all = Cf.pairs_from_link_capsules(T[:, frames], lc, tab)          # [n, L*K, 3], leaf-major
    L = len(frames)
    pl = np.zeros((len(sub), L * kmax, 3), np.float32)
    po = np.full((len(sub), L * kmax, 3), 1.0e3, np.float32)                     # filler: a kilometre away, metric exactly 0
    clr = np.full(len(sub), np.inf)
    for n, r in enumerate(sub):
        for l in range(L):
            for t, b in enumerate(lists[r]):
                pl[n, l * kmax + t] = pl_all[n, l * K + b]
                po[n, l * kmax + t] = po_all[n, l * K + b]
                clr[n] = min(clr[n], np.linalg.norm(pl_all[n, l * K + b] - po_all[n, l * K + b]))
    ref = O.step(desc, s["q"][sub], s["qd"][sub], s["goal"][sub], p_link=pl, p_obs=po)
    ok = clr >= 0.05                                                              # parity away from contact, as everywhere
    assert ok.sum() > len(sub) // 3
    kw = dict(p_link=pl[ok], p_obs=po[ok])
    verdict = O.accuracy_gate(got.cpu().numpy()[sub][ok], {k: ref[k][ok] for k in ("qdd64", "M", "f")},
                              spread=O.fp32_resolution(desc, s["q"][sub][ok], s["qd"][sub][ok], s["goal"][sub][ok], **kw))
    assert verdict["ok"].all(), O.gate_summary(verdict)
    assert verdict["a"].mean() > 0.8, O.gate_summary(verdict)
    # the lists matter: the whole table for every robot gives other numbers
    full = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=torch.from_numpy(tab), link_capsules=torch.from_numpy(lc)))
    torch.cuda.synchronize()
    assert (full - got).abs().max().item() > 1e-3

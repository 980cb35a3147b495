"""Self collision on the GPU: the self-pair stage against a float64 numpy restatement, the staged step against the CPU oracle,
its composition with the obstacle stage (bit for bit), and the refusals.

Checker: oracle.forward_kinematics in fp64 plus segment-segment closest points (tests/self_pair_reference.py), and oracle.step on
explicit pairs.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from self_pair_reference import _seg_seg, _world_segments, self_pairs_np  # noqa: E402,F401

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


def _setup(config, solve="auto"):
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D, urdf as U
    table, desc = getattr(Cf, config)(solve)
    leaf_frames = [desc.leaves[i].frame for i in D.distance_leaf_indices(desc)]
    pairs = U.self_collision_pairs(table, leaf_frames)
    caps = U.self_collision_capsules(U.PANDA_URDF, table)
    return table, desc, pairs, caps


@pytest.mark.parametrize("config", ["config3", "exp05_panda"])
def test_stage_geometry(torch_mod, config):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, pairs, caps = _setup(config)
    assert len(pairs) == 44
    eng = _engine(desc)
    eng.set_self_collision(pairs, caps)
    assert eng.self_counts == [5, 4, 4, 5, 4, 6, 8, 8]
    rng = np.random.default_rng(7)
    s = Cf.sample_panda_states(rng, 4096)
    pl, po, dd = (t.cpu().numpy() for t in eng.self_pairs(torch.from_numpy(s["q"])))
    assert pl.shape == (4096, 44, 3) and dd.shape == (4096, 44)
    assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all()
    sub = np.r_[0:64, 4000:4096]     # brute force on a few robots
    rpl, rpo, rdd, gap = self_pairs_np(desc, pairs, caps, s["q"][sub])
    # near-crossing axes make the normal (and an attached point's normal_vec) ill-conditioned: points, not directions, there
    well = np.abs(gap) > 1e-3
    assert np.abs(pl[sub] - rpl).max() <= 1e-5
    assert np.abs(dd[sub] - rdd).max() <= 1e-5
    assert np.abs(po[sub] - rpo)[well].max() <= 1e-5


def test_stage_crossing_axes(torch_mod):
    """A B capsule (the base row) whose axis crosses the leaf link's axis: outputs stay finite, overlap = sum of the radii."""
    torch = torch_mod
    import oracle as O
    table, desc, _, caps = _setup("exp05_panda")
    q = np.asarray([[0.0, -0.3, 0.0, -2.2, 0.0, 2.0, 0.8, 0.02, 0.02]], np.float32)
    T = O.forward_kinematics(desc, q, "f64")[0]
    fa = 4                                                     # panda_joint5: leaf ordinal 3
    A, B, ra = _world_segments(T[None, fa], caps[fa])
    mid = 0.5 * (A[0] + B[0])
    axis = (B[0] - A[0]) / np.linalg.norm(B[0] - A[0])
    perp = np.cross(axis, [1.0, 0.0, 0.0])
    perp /= np.linalg.norm(perp)
    caps = caps.copy()
    caps[-1] = [*(mid - 0.05 * perp), 0.03, *(mid + 0.05 * perp), 0.0]
    for config in ("config3", "exp05_panda"):
        _, desc, _, _ = _setup(config)
        eng = _engine(desc)
        eng.set_self_collision([(3, -1)], caps)
        pl, po, dd = (t.cpu().numpy() for t in eng.self_pairs(torch.from_numpy(q)))
        assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all(), config
        assert abs(dd[0, 0] - (ra + 0.03)) < 1e-4, (config, dd[0, 0])


def _explicit(pl, po, dd, counts, point):
    kw = dict(p_link=pl.astype(np.float32), p_obs=po.astype(np.float32), pair_counts=counts)
    if point:
        kw["dist"] = dd.astype(np.float32)
    return kw


def _gate(qdd, ref, clr, what, spread=None):
    import oracle as O
    ref64 = ref["qdd64"]
    e = np.abs(qdd.astype(np.float64) - ref64).max(axis=1)
    mag = np.maximum(1.0, np.abs(ref64).max(axis=1))
    clear = clr >= 0.05      # (random Panda states: few robots keep 5 cm between their own links)
    assert (e[clear] <= ATOL * mag[clear]).all(), f"{what}: clear robots worst {e[clear].max():.2e}"
    rest = ~clear
    ok = np.ones(len(qdd), bool)
    if rest.any():
        verdict = O.accuracy_gate(qdd[rest], {k: ref[k][rest] for k in ("qdd64", "M", "f")},
                                  spread=None if spread is None else spread[rest])
        ok[rest] = verdict["ok"]
    return ok


@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("kernel", ["hex", "quad", "lane"])
@pytest.mark.parametrize("config", ["config3", "exp05_panda"])
def test_step_vs_oracle(torch_mod, config, kernel, solve):
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, pairs, caps = _setup(config, solve)
    eng = _engine(desc, kernel)
    eng.set_self_collision(pairs, caps)
    rng = np.random.default_rng(11)
    R = 2048
    s = Cf.sample_panda_states(rng, R)
    qdd = eng.step(torch.from_numpy(s["q"]), torch.from_numpy(s["qd"]), torch.from_numpy(s["goal"])).cpu().numpy()
    point = config == "exp05_panda"
    sub = slice(0, 600)
    pl, po, dd, gap = self_pairs_np(desc, pairs, caps, s["q"][sub])
    kw = _explicit(pl, po, dd, eng.self_counts, point)
    args = (desc, s["q"][sub], s["qd"][sub], s["goal"][sub])
    ref = O.step(*args, **kw)
    ok = _gate(qdd[sub], ref, gap.min(axis=1), f"{config}/{kernel}/{solve}", spread=O.fp32_resolution(*args, **kw))
    # Robots in deep self contact: the repulsion (gain 800 over 1 cm) turns the fp32 rounding of the closest points into more
    # than the step's own resolution.  Those are held to the gate on the stage's OWN pairs (the pairs' geometry is pinned to
    # 1e-5 m by test_stage_geometry): what is tested here is the step on the pairs it was given.
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


def _interleave(torch, obs_pl, obs_po, K, self_pl, self_po, counts):
    parts_l, parts_o, off = [], [], 0
    for i, c in enumerate(counts):
        parts_l += [obs_pl[:, i * K:(i + 1) * K], self_pl[:, off:off + c]]
        parts_o += [obs_po[:, i * K:(i + 1) * K], self_po[:, off:off + c]]
        off += c
    return torch.cat(parts_l, dim=1).contiguous(), torch.cat(parts_o, dim=1).contiguous()


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
@pytest.mark.parametrize("R", [1, 3000])
def test_composition_bit_equal(torch_mod, prim, R):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    table, desc, pairs, caps = _setup("config3")
    rng = np.random.default_rng(23 + R)
    s = Cf.sample_panda_states(rng, R)
    tab = Cf.sample_spheres(rng, 32) if prim == "sphere" else Cf.sample_capsules(rng, 32)
    lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, table, Cf.CONTROL_POINT_FRAMES)).cuda()
    eng = _engine(desc)
    eng.set_self_collision(pairs, caps)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    t = torch.from_numpy(tab).cuda()
    got = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=t, link_capsules=lc))
    # host composition: the obstacle stage, the self stage, interleaved per leaf, an explicit-pair step of a plain handle
    opl, opo = eng.closest_points(q, eng.obstacles(spheres=t), link_capsules=lc)
    spl, spo, _ = eng.self_pairs(q)
    counts = eng.self_counts
    pl, po = _interleave(torch, opl, opo, 32, spl, spo, counts)
    plain = _engine(desc)
    want = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=pl, p_obs=po, pair_counts=[32 + c for c in counts]))
    torch.cuda.synchronize()
    assert torch.equal(got, want), (got - want).abs().max().item()
    # and without a table: the self pairs alone
    got0 = eng.step(q, qd, goal)
    want0 = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=spl, p_obs=spo, pair_counts=counts))
    torch.cuda.synchronize()
    assert torch.equal(got0, want0)


def test_refusals(torch_mod):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, descriptor as D
    from riemannian_motion_policies_amd._native import ERR_UNSUPPORTED, Rmp2Error
    table, desc, pairs, caps = _setup("config3")
    rng = np.random.default_rng(5)
    R = 64
    s = Cf.sample_panda_states(rng, R)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    sp = torch.from_numpy(Cf.sample_spheres(rng, 8)).cuda()
    eng = _engine(desc)
    eng.set_self_collision(pairs, caps)

    def refused(fn, words):
        with pytest.raises(Rmp2Error) as e:
            fn()
        assert getattr(e.value, "code", None) == ERR_UNSUPPORTED, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    off = torch.zeros(R + 1, dtype=torch.int32)
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp, csr_offset=off, csr_index=torch.zeros(0))),
            ["self collision", "RAGGED"])
    cyl = torch.from_numpy(Cf.sample_cylinders(rng, 4)).cuda()
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=cyl, primitive="cylinder")), ["self collision", "CYLINDER"])
    pl = torch.zeros((R, 8, 3), device="cuda")
    refused(lambda: eng.step(q, qd, goal, obstacles=eng.obstacles(p_link=pl, p_obs=pl + 1)), ["self collision", "EXPLICIT_PAIRS"])
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
    # a table on a set with attached-point leaves
    _, desc5, pairs5, caps5 = _setup("exp05_panda")
    e5 = _engine(desc5)
    e5.set_self_collision(pairs5, caps5)
    lc5 = torch.zeros((8, 8), device="cuda")
    refused(lambda: e5.step(q, qd, goal, obstacles=e5.obstacles(spheres=sp, link_capsules=lc5)), ["self collision", "attached-point"])
    # argument checks of the list
    from riemannian_motion_policies_amd._native import ERR_INVALID_ARGUMENT
    for bad in ([(0, 1)], [(0, 99)]):      # B = the leaf's own frame; B out of range
        with pytest.raises(Rmp2Error) as e:
            eng.set_self_collision(bad, caps)
        assert e.value.code == ERR_INVALID_ARGUMENT
    arr = np.asarray([[0, 5]] * 257, np.int32)
    assert eng._lib.rmp2_set_self_collision(eng._h, 257, arr.ctypes.data, caps.ctypes.data) == ERR_INVALID_ARGUMENT
    arr = np.asarray([[0, 5]], np.int32)   # leaf 0 is the attractor: no pair data
    assert eng._lib.rmp2_set_self_collision(eng._h, 1, arr.ctypes.data, caps.ctypes.data) == ERR_INVALID_ARGUMENT


def test_off_is_a_fresh_handle(torch_mod):
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    table, desc, pairs, caps = _setup("config3")
    rng = np.random.default_rng(9)
    s = Cf.sample_panda_states(rng, 5000)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    sp = torch.from_numpy(Cf.sample_spheres(rng, 32)).cuda()
    eng, fresh = _engine(desc), _engine(desc)
    eng.set_self_collision(pairs, caps)
    with_self = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp))
    eng.set_self_collision([], None)
    a = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=sp))
    b = fresh.step(q, qd, goal, obstacles=fresh.obstacles(spheres=sp))
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert not torch.equal(with_self, b)
    with pytest.raises(ValueError):
        eng.step(q, qd, goal)        # distance leaves and no obstacles: refused again once the self pairs are off


def test_class_surface(torch_mod, golden_dir):
    """RmpCore.update_distances / Datamanager.update_device with self_collision=True: the holders of each frame hold its K
    obstacle pairs followed by its self pairs; core.evaluate (fused route, explicit route from the holders, one robot from host
    arrays) gives the q'' of the staged rmp2_step."""
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
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    R, K = 2000, 32
    s = Cf.sample_panda_states(rng, R)
    q, qd = torch.from_numpy(s["q"]).to(dev), torch.from_numpy(s["qd"]).to(dev)
    target_rmp.goal = torch.from_numpy(s["goal"]).to(dev)
    tab = torch.from_numpy(Cf.sample_spheres(rng, K)).to(dev)
    lc = torch.from_numpy(U.link_capsules(U.PANDA_URDF, fkine.table, Cf.CONTROL_POINT_FRAMES)).to(dev)
    data_manager.update_device(core, q, tab, link_capsules=lc, self_collision=True)
    fused = core.evaluate(q, qd)
    assert core._stage._arrays is None                     # the step formed every pair itself
    eng = core.engine_for(q)
    counts = eng.self_counts
    assert counts == [5, 4, 4, 5, 4, 6, 8, 8]
    staged = eng.step(q, qd, target_rmp.goal, obstacles=eng.obstacles(spheres=tab, link_capsules=lc))
    torch.cuda.synchronize()
    assert torch.equal(fused, staged)
    for i, fr in enumerate(Cf.CONTROL_POINT_FRAMES):
        st = data_manager[fr]
        assert tuple(st["pos_on_link_in_base_frame"].value.shape) == (R, K + counts[i], 3), fr
        assert tuple(st["distance"].value.shape) == (R, K + counts[i]), fr
        assert tuple(st["relative_position"].value.shape) == (R, K + counts[i], 3), fr
    # the self half of a frame's holder is rmp2_self_pairs' output
    spl, spo, _ = eng.self_pairs(q)
    h0 = data_manager[Cf.CONTROL_POINT_FRAMES[0]]["pos_on_link_in_base_frame"].value
    assert torch.equal(h0[:, K:], spl[:, :counts[0]])
    # explicit route (the holders read): same arrays, same step
    explicit = core.evaluate(q.clone(), qd)
    torch.cuda.synchronize()
    assert torch.equal(explicit, staged)
    # one robot from host arrays, as the reference's loop calls it
    data_manager.update_device(core, q[3], tab, link_capsules=lc, self_collision=True)
    target_rmp.goal = s["goal"][3]
    one = core.evaluate(s["q"][3], s["qd"][3])
    want = staged[3].cpu().numpy()
    assert one.shape == (9,) and np.abs(np.asarray(one) - want).max() <= ATOL * max(1.0, np.abs(want).max())
    # and the core without self collision again: the engine's list is off
    target_rmp.goal = torch.from_numpy(s["goal"]).to(dev)
    data_manager.update_device(core, q, tab, link_capsules=lc)
    plain = core.evaluate(q, qd)
    assert eng.self_counts is None and not torch.equal(plain, staged)

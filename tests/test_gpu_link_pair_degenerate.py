"""Link-capsule pairs at DEGENERATE geometry on every route to the step: a sphere centred on a link's axis, crossing, parallel and
collinear axes, zero-length capsules, endpoint clamps, overlapping shapes -- on exact scenes (tests/link_pair_scene.py), where
|X - Y| is 0 and not 1e-15.  The project's convention for intersecting axes is the fixed normal +z (rmp2_device.h
link_pair_fields / link_normal_length, configs.pairs_from_link_capsules): every route must answer it, finite, without
STATUS_NONFINITE, within the project's bounds for robots clear of contact (the scenes' smallest clearance is 0.0625 >= 0.05) of
oracle.step on the fp64 closed-form pairs.  No robot is exempt; the worst ratio error / bound is printed per route.

Fleets: the scene's rows tiled to R = 1 and R = 67 (16 robots per wave in the quad mapping: a partial last wave).  Tables: the live
record among culled fillers at index 0, 31, 32 and K - 1 for K in {1, 33, 64, 300} (full chunk of the batched range test, partial
chunk, second chunk, beyond the 256-record LDS stage), and eight copies of the live sphere in one chunk (every lane of a quad
takes a trip, one takes two).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import link_pair_scene as S  # noqa: E402

pytestmark = pytest.mark.gpu

FUSED = 3e-5      # test_gpu_capsules.py test_link_geometry_fused_into_the_step: the fused forms against the oracle
EXPLICIT = 1e-5   # the north-star bound of the explicit-pair step (routes that end in it: the stages' pairs fed back)
POINTS = 2e-6     # test_gpu_capsules.py: the stage's points
FORMS = 1e-6      # the two forms of the stage against each other
ROLLOUT = 1e-4    # test_link_geometry_fused_into_the_step: rollout against the loop of plain steps

TABLES = [(1, 0), (33, 0), (33, 31), (33, 32), (64, 0), (64, 31), (64, 32), (64, 63), (300, 0), (300, 31), (300, 32), (300, 299)]
COPIES = (33, [1, 2, 3, 5, 8, 13, 21, 30])   # eight copies of the live record in the first chunk
FLEETS = [1, 67]


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


_SCENES, _REFS = {}, {}


def _scene(robot, solve, R):
    """The tiled scene, computed once and left unchanged."""
    key = (robot, solve, R)
    if key not in _SCENES:
        _SCENES[key] = S.tiled(S.gantry(solve) if robot == "gantry" else S.two_joint(solve), R)
    return _SCENES[key]


def _ref(robot, solve, R, name, table, **kw):
    """oracle.step on the fp64 pairs of (tiled scene, table), computed once per `name`."""
    key = (robot, solve, R, name)
    if key not in _REFS:
        _REFS[key] = S.reference(_scene(robot, solve, R), table, **kw)
    return _REFS[key]


def _dev(torch, s):
    return tuple(torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))


def _ratio(what, got, status, ref, bound, worst):
    """Every robot finite, none flagged non-finite, error <= bound max(1, |qdd64|); records the worst ratio of the route."""
    from riemannian_motion_policies_amd import descriptor as D
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert np.isfinite(got).all(), f"{what}: non-finite qdd on robots {np.nonzero(~np.isfinite(got).all(axis=1))[0][:8]}"
    if status is not None:
        st = status.cpu().numpy()
        assert ((st & D.STATUS_NONFINITE) == 0).all(), f"{what}: STATUS_NONFINITE"
    ref64 = ref["qdd64"]
    err = np.abs(got.astype(np.float64) - ref64).max(axis=1)
    ratio = err / (bound * np.maximum(1.0, np.abs(ref64).max(axis=1)))
    worst[0] = max(worst[0], float(ratio.max()))
    assert ratio.max() <= 1.0, f"{what}: robot {int(ratio.argmax())} at {ratio.max():.2f} of the bound {bound:g}"


def _point_error(a, b):
    """max |a - b| in units that keep the point bounds meaningful on the fillers: the bounds were set for coordinates of about a
    metre (2e-6 = 16 ulp32 there); a filler's points lie at z = 40, where ONE ulp32 is 3.8e-6.  Coordinates beyond 8 are measured
    relative to 8 -- 2e-6 is then 2.6 ulp32 at z = 40, still the stricter bound in ulps; every live pair is held to the plain one."""
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b) / 8.0)).max())


def _tables(live_name):
    """(label, table) of the live record `live_name`: every (K, index) of TABLES, and the eight copies for the sphere."""
    rec = S.LIVE[live_name]
    out = [(f"{live_name} K={K} at {at}", S.table_with(rec, K, at)) for K, at in TABLES]
    if live_name == "sphere":
        out.append((f"{live_name} K={COPIES[0]} x8", S.table_with(rec, *COPIES)))
    return out


def _step(torch, eng, q, qd, goal, **obs):
    st = torch.zeros(q.shape[0], dtype=torch.int32, device="cuda")
    out = eng.step(q, qd, goal, obstacles=eng.obstacles(**{k: (v if hasattr(v, "is_cuda") else torch.from_numpy(np.ascontiguousarray(v)).cuda())
                                                         for k, v in obs.items()}), status=st)
    torch.cuda.synchronize()
    return out, st


def test_scenes_are_what_they_claim(torch_mod):
    """The precondition of everything below: the scenes' kinematics are exact -- the oracle's fp32 frames equal its fp64 frames bit
    for bit, and so do the engine's -- and every row meant to be in range of a live record matters to the oracle."""
    torch = torch_mod
    for solve in ("auto", "pinv"):
        s = S.gantry(solve)
        T64 = S.check_exact_kinematics(s)
        T = _engine(s["desc"]).forward_kinematics(torch.from_numpy(s["q"])).cpu().numpy()
        assert np.array_equal(T.astype(np.float64), T64)
        for name, rec in S.LIVE.items():
            S.rows_in_range(s, S.table_with(rec, 1, 0), S.IN_RANGE[name])
    s = S.two_joint()
    t = s["table"]
    j1, j2 = t.frame_index("joint_1"), t.frame_index("joint_2")
    T64 = S.check_exact_kinematics(s, frames=[j1], origins_only=[j2])
    T = _engine(s["desc"]).forward_kinematics(torch.from_numpy(s["q"])).cpu().numpy()
    assert np.array_equal(T[:, j1].astype(np.float64), T64[:, j1]) and np.array_equal(T[:, j2, :3, 3], T64[:, j2, :3, 3].astype(np.float32))
    ref = S.reference(s, S.TWO_JOINT_SPHERES)
    assert np.linalg.cond(ref["M"]).max() < 100 and np.isfinite(ref["qdd64"]).all()


@pytest.mark.parametrize("R", FLEETS)
@pytest.mark.parametrize("live", list(S.LIVE))
def test_stage_and_explicit_pair_step(torch_mod, live, R):
    """Routes 1 and 2.  eng.closest_points(q, table, link_capsules=) in its default form (rmp2_closest_wave_kernel, a lane per pair)
    and under RMP2_KERNEL=lane (rmp2_closest_kernel, a lane per robot; both in csrc/rmp2_stages.h): the pairs against numpy fp64 at 2e-6, the two forms within
    1e-6 of each other; then those pairs fed to the explicit-pair step, against the oracle on the fp64 pairs at 1e-5."""
    torch = torch_mod
    s = _scene("gantry", "auto", R)
    q, qd, goal = _dev(torch, s)
    lc = torch.from_numpy(s["lc"]).cuda()
    wave, lane = _engine(s["desc"]), _engine(s["desc"], "lane")
    worst_pt, worst = 0.0, [0.0]
    for label, tab in _tables(live):
        pl_ref, po_ref, _ = S.pairs64(s, tab)
        tt = torch.from_numpy(tab).cuda()
        got = {}
        for form, eng in (("wave", wave), ("lane", lane)):
            pl, po = eng.closest_points(q, eng.obstacles(spheres=tt), link_capsules=lc)
            torch.cuda.synchronize()
            got[form] = (pl.cpu().numpy(), po.cpu().numpy())
            assert np.isfinite(got[form][0]).all() and np.isfinite(got[form][1]).all(), f"{label} {form}: non-finite points"
            e = max(_point_error(got[form][0], pl_ref), _point_error(got[form][1], po_ref))
            worst_pt = max(worst_pt, float(e))
            assert e <= POINTS, f"{label} {form}: points off by {e:.2e}"
            out, st = _step(torch, eng, q, qd, goal, p_link=pl, p_obs=po)
            _ratio(f"{label} {form} pairs -> explicit-pair step", out, st, _ref("gantry", "auto", R, label, tab), EXPLICIT, worst)
        assert max(_point_error(got["wave"][0], got["lane"][0]), _point_error(got["wave"][1], got["lane"][1])) <= FORMS, label
    print(f"stage {live} R={R}: worst point error {worst_pt:.2e} (bound {POINTS:g}); explicit-pair step worst ratio {worst[0]:.3f}")


@pytest.mark.parametrize("R", FLEETS)
@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("live", list(S.LIVE))
def test_fused_shared_table(torch_mod, live, solve, R):
    """Route 3: the step forms the pairs itself from (table, link_capsules) -- rmp2_quad.h pair_loop_link for tables the LDS stage
    holds (K <= 256: "quad" in last_kernel), the closest-point stage plus the explicit-pair step inside rmp2_step beyond."""
    torch = torch_mod
    s = _scene("gantry", solve, R)
    q, qd, goal = _dev(torch, s)
    eng = _engine(s["desc"])
    worst, kernels = {"fused": [0.0], "staged": [0.0]}, set()
    for label, tab in _tables(live):
        out, st = _step(torch, eng, q, qd, goal, spheres=tab, link_capsules=s["lc"])
        fused = len(tab) <= 256
        kernels.add(("fused: " if fused else "staged: ") + eng.last_kernel())
        assert not fused or "quad" in eng.last_kernel()
        _ratio(f"{label} {solve}", out, st, _ref("gantry", solve, R, label, tab), FUSED if fused else EXPLICIT, worst["fused" if fused else "staged"])
    print(f"shared table {live} {solve} R={R}: worst ratio fused {worst['fused'][0]:.3f}, staged (K = 300) {worst['staged'][0]:.3f}; {sorted(kernels)}")


def _multi_table(live, K):
    """A table with the four capsule cases (or four copies of the sphere) at index 0, 31, 32 and K - 1 among fillers."""
    recs = [S.LIVE["sphere"]] * 4 if live == "sphere" else [S.LIVE_CAPSULES[n] for n in ("cross", "parallel", "point", "collinear")]
    at = [0, 31, 32, K - 1]
    tab = np.tile(S.filler(len(recs[0])), (K, 1))
    for i, r in zip(at, recs):
        tab[i] = r
    return tab, at


def _lists(R, K, at, repeat):
    """Distinct lists per robot: robot r names ITS case at[(r + r // 10) % 4] (twice when `repeat`; the scene has ten rows, so every
    row meets every case in a fleet of 67) among r % 3 fillers; robot 5 (if any) has an empty list, robot 6 fillers only."""
    fill = [i for i in range(K) if i not in at]
    lists = []
    for r in range(R):
        own = [at[(r + r // 10) % 4]] * (2 if repeat else 1)
        extra = [fill[(r * 7 + j * 3) % len(fill)] for j in range(r % 3)]
        extra = list(dict.fromkeys(extra))
        lst = extra[:1] + own[:1] + extra[1:] + own[1:]
        if r == 5:
            lst = []
        if r == 6:
            lst = fill[3:6]
        lists.append(lst)
    off = np.zeros(R + 1, np.int32)
    off[1:] = np.cumsum([len(l) for l in lists])
    idx = np.asarray([i for l in lists for i in l], np.int32)
    return lists, off, idx, fill[0]


@pytest.mark.parametrize("R", FLEETS)
@pytest.mark.parametrize("live", ["sphere", "capsules"])
@pytest.mark.parametrize("route", ["mask", "walk", "staged"])
def test_ragged_lists(torch_mod, route, live, R):
    """Routes 4, 5 and 6, ragged lists with link geometry.  mask: a table of 64 records, lists without repeats -- taken as a
    membership mask by pair_loop_link.  walk: the same lists with the live index TWICE -- pair_loop_link_list, and the oracle gets
    that pair twice.  staged: lists over a table of 300 records -- the closest-point stage run inside rmp2_step, then the
    explicit-pair step.  Distinct lists per robot, each naming its own case; an empty list and one of fillers only."""
    torch = torch_mod
    K = 300 if route == "staged" else 64
    tab, at = _multi_table(live, K)
    for solve in ("auto", "pinv"):
        s = _scene("gantry", solve, R)
        q, qd, goal = _dev(torch, s)
        eng = _engine(s["desc"])
        lists, off, idx, fill = _lists(R, K, at, repeat=route == "walk")
        out, st = _step(torch, eng, q, qd, goal, spheres=tab, link_capsules=s["lc"], csr_offset=off, csr_index=idx)
        ref = _ref("gantry", solve, R, f"ragged {route} {live}", tab, lists=lists, fill=fill)
        worst = [0.0]
        _ratio(f"ragged {route} {live} {solve}", out, st, ref, EXPLICIT if route == "staged" else FUSED, worst)
        print(f"ragged {route} {live} {solve} R={R}: worst ratio {worst[0]:.3f}; {eng.last_kernel()}")
    if R > 6:   # the empty list and the list of fillers answer what no obstacle at all answers
        none = S.reference(s, S.moved_away(tab))["qdd64"]
        assert np.array_equal(ref["qdd64"][5], none[5]) and np.array_equal(ref["qdd64"][6], none[6])


@pytest.mark.parametrize("R", FLEETS)
@pytest.mark.parametrize("solve", ["auto", "pinv"])
def test_rollout(torch_mod, solve, R):
    """Route 7.  A rollout of one control step, one substep and dt = 0 leaves the state alone and returns the qdd of the fused plain
    step (route 3): held to the oracle at the same bound, and to that step at the bound both meet.  Two control steps with dt = 2^-7
    against the same loop made of plain steps and torch integration, at 1e-4."""
    torch = torch_mod
    s = _scene("gantry", solve, R)
    q, qd, goal = _dev(torch, s)
    eng = _engine(s["desc"])
    lc = torch.from_numpy(s["lc"]).cuda()
    worst = [0.0]
    tables = [t for live in S.LIVE for t in _tables(live) if len(t[1]) in (1, 64) or "x8" in t[0]]
    for label, tab in tables:
        tt = torch.from_numpy(tab).cuda()
        ref = _ref("gantry", solve, R, label, tab)
        st = torch.zeros(R, dtype=torch.int32, device="cuda")
        qa, qda = q.clone(), qd.clone()
        out = eng.rollout(qa, qda, goal, obstacles=eng.obstacles(spheres=tt, link_capsules=lc), n_control_steps=1, substeps=1, dt=0.0, status=st)
        torch.cuda.synchronize()
        assert "quad" in eng.last_kernel()
        assert torch.equal(qa, q) and torch.equal(qda, qd)
        _ratio(f"rollout {label} {solve}", out, st, ref, FUSED, worst)
        plain, _ = _step(torch, eng, q, qd, goal, spheres=tt, link_capsules=lc)
        mag = plain.abs().amax(dim=1).clamp(min=1.0)
        assert ((out - plain).abs().amax(dim=1) <= FUSED * mag).all(), label
        # two control steps
        dt = 2.0 ** -7
        qa, qda = q.clone(), qd.clone()
        for _ in range(2):
            a, _ = _step(torch, eng, qa, qda, goal, spheres=tt, link_capsules=lc)
            qda = qda + dt * a
            qa = qa + dt * qda
        qb, qdb = q.clone(), qd.clone()
        eng.rollout(qb, qdb, goal, obstacles=eng.obstacles(spheres=tt, link_capsules=lc), n_control_steps=2, substeps=1, dt=dt)
        torch.cuda.synchronize()
        assert torch.isfinite(qa).all() and torch.isfinite(qb).all() and torch.isfinite(qdb).all(), label
        assert (qa - qb).abs().max().item() < ROLLOUT and (qda - qdb).abs().max().item() < ROLLOUT, label
    print(f"rollout {solve} R={R}: {len(tables)} tables, worst ratio {worst[0]:.3f}")


@pytest.mark.parametrize("R", FLEETS)
@pytest.mark.parametrize("live", list(S.LIVE))
def test_self_collision_handle(torch_mod, live, R):
    """Route 8.  A handle with set_self_collision (each leaf's link against a base capsule that stays 40 m away) stepping on
    (table, link_capsules): rmp2_self_stage_kernel<OBS, LINK> (csrc/rmp2_stages.h) forms each leaf's [K obstacle pairs | 1 self
    pair] -- its obstacle rows are obstacle_pair_points, the closed form it shares with rmp2_closest_wave_kernel -- and the
    explicit-pair step takes them (stage_self in
    rmp2_hip.hip: a handle with self collision never takes the fused form; last_kernel names the step's kernel only)."""
    torch = torch_mod
    s = _scene("gantry", "auto", R)
    q, qd, goal = _dev(torch, s)
    eng = _engine(s["desc"])
    F = s["table"].n_frames
    caps = np.zeros((F + 1, 8), np.float32)
    for row, fr in zip(s["lc"], S.distance_frames(s["desc"])):
        caps[fr] = row
    caps[F] = [0.0, 0.0, -S.FAR_Z, S.OBS_R, 0.5, 0.0, -S.FAR_Z, 0.0]
    eng.set_self_collision([(0, -1), (1, -1)], caps)
    assert eng.self_counts == [1, 1]
    spl, spo, _ = S.pairs64(s, caps[F:F + 1])       # the base capsule is fixed in the world: a table of one record
    extra = (spl.reshape(R, 2, 1, 3), spo.reshape(R, 2, 1, 3))
    worst = [0.0]
    for label, tab in _tables(live):
        out, st = _step(torch, eng, q, qd, goal, spheres=tab, link_capsules=s["lc"])
        ref = _ref("gantry", "auto", R, "self " + label, tab, extra=extra)
        _ratio(f"self collision {label}", out, st, ref, EXPLICIT, worst)
        # (the far self pair is an exact 0: the reference is the plain one)
        assert np.array_equal(ref["qdd64"], _ref("gantry", "auto", R, label, tab)["qdd64"])
    print(f"self-collision handle {live} R={R}: worst ratio {worst[0]:.3f}; {eng.last_kernel()}")


@pytest.mark.parametrize("R", FLEETS)
@pytest.mark.parametrize("solve", ["auto", "pinv"])
def test_two_joint_routes(torch_mod, solve, R):
    """Routes 3, 4 and 7 on the 2-dof template of the quad kernel: spheres on link 1's axis, on its endpoints, beside it, overlapping
    it, and on the origin of joint_2.  The fixed normal +z pulls back to zero on a planar arm, so this scene checks finiteness,
    status and that the routes agree: each within the fused bound of the oracle (cond(M) <= 7.1 with the damping leaf)."""
    torch = torch_mod
    s = _scene("two_joint", solve, R)
    q, qd, goal = _dev(torch, s)
    eng = _engine(s["desc"])
    lc = torch.from_numpy(s["lc"]).cuda()
    worst = [0.0]
    singles = [(n, S.table_with(S.TWO_JOINT_SPHERES[i], K, at)) for i, n in enumerate(S.TWO_JOINT_SPHERE_NAMES) for K, at in ((1, 0), (33, 32), (64, 31))]
    for label, tab in singles + [("all", S.TWO_JOINT_SPHERES)]:
        tt = torch.from_numpy(tab).cuda()
        ref = _ref("two_joint", solve, R, f"{label} K={len(tab)}", tab)
        out, st = _step(torch, eng, q, qd, goal, spheres=tt, link_capsules=lc)
        assert "quad" in eng.last_kernel()
        _ratio(f"two-joint {label} {solve} shared", out, st, ref, FUSED, worst)
        K = len(tab)
        off = np.arange(R + 1, dtype=np.int32) * K          # every robot lists the whole table, each in an order of its own
        idx = np.concatenate([np.roll(np.arange(K, dtype=np.int32), r) for r in range(R)])
        out4, st4 = _step(torch, eng, q, qd, goal, spheres=tt, link_capsules=lc, csr_offset=off, csr_index=idx)
        _ratio(f"two-joint {label} {solve} mask", out4, st4, ref, FUSED, worst)
        st7 = torch.zeros(R, dtype=torch.int32, device="cuda")
        qa, qda = q.clone(), qd.clone()
        out7 = eng.rollout(qa, qda, goal, obstacles=eng.obstacles(spheres=tt, link_capsules=lc), n_control_steps=1, substeps=1, dt=0.0, status=st7)
        torch.cuda.synchronize()
        assert "quad" in eng.last_kernel()
        _ratio(f"two-joint {label} {solve} rollout", out7, st7, ref, FUSED, worst)
    print(f"two-joint {solve} R={R}: worst ratio {worst[0]:.3f}")


def test_two_joint_pinv_rollout_with_link_geometry(torch_mod):
    """include/rmp2.h promises fused link geometry for 2-dof robots with either resolve, rollouts included: a solve = pinv rollout
    of config5_two_joint with link_capsules takes the quad mapping (its closed-form 2 x 2 resolve is the pseudo-inverse) and
    agrees with the loop of plain steps, on robots clear of contact with cond(M) < 100."""
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    rng = np.random.default_rng(2025)
    R, K = 333, 12
    table, desc = Cf.config5_two_joint("pinv")
    s = Cf.sample_two_joint_states(rng, R)
    lc_np = U.link_capsules(U.TWO_JOINT_URDF, table, Cf.TWO_JOINT_CONTROL_POINT_FRAMES)
    tab = Cf.sample_spheres(rng, K)
    tab[:, 2] += np.float32(0.45)   # (as test_gpu_capsules.py: partly above the arm, a mix of in-range and culled pairs)
    eng = _engine(desc)
    q, qd, goal = _dev(torch, s)
    tt, lc = torch.from_numpy(tab).cuda(), torch.from_numpy(lc_np).cuda()
    obs = lambda: eng.obstacles(spheres=tt, link_capsules=lc)   # noqa: E731
    pl, po = eng.closest_points(q, eng.obstacles(spheres=tt), link_capsules=lc)
    clear = (torch.linalg.norm(pl - po, dim=-1).min(dim=1).values >= 0.05)
    ref = O.step(desc, s["q"], s["qd"], s["goal"], p_link=pl.cpu().numpy(), p_obs=po.cpu().numpy())
    ok = clear & torch.from_numpy(np.linalg.cond(ref["M"]) < 100).cuda()
    assert ok.sum().item() > R // 4, f"only {ok.sum().item()} robots clear of contact and well conditioned"
    qa, qda = q.clone(), qd.clone()
    for _ in range(3):
        a = eng.step(qa, qda, goal, obstacles=obs())
        for _ in range(5):
            qda = qda + 0.01 * a
            qa = qa + 0.01 * qda
    qb, qdb = q.clone(), qd.clone()
    eng.rollout(qb, qdb, goal, obstacles=obs(), n_control_steps=3, substeps=5, dt=0.01)
    torch.cuda.synchronize()
    assert "quad" in eng.last_kernel()
    fin = torch.isfinite(qa).all(dim=1) & torch.isfinite(qb).all(dim=1) & ok
    assert fin.sum().item() > R // 4
    d = (qa - qb).abs().max(dim=1).values[fin]
    print(f"two-joint pinv rollout with link geometry: {int(fin.sum())} robots, worst |q_rollout - q_loop| {d.max().item():.2e}; {eng.last_kernel()}")
    assert (d < ROLLOUT).all()

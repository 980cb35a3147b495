"""The hull self-pair stage (rmp2_set_self_collision_hulls, rmp2_self_pairs, rmp2_self_hull_stage_kernel<0, 1, 2> and its own walk
walk_frame_position) and the link-hull obstacle stage (rmp2_hull_stage_kernel) beyond the Panda and the prismatic gantries: the
eight random trees of tests/self_pair_scene.py with convex polytopes on their links (tests/hull_tree_scene.py) -- revolute axes off
z, 0, 1 and 2 save slots, 7 to 16 dofs, up to 31 frames, joints left out of the order, two root joints, B frames outside the
step's pruned program, attached-point leaves on frames that have turned, leaves without a shape, two leaves on one frame; raw
lists with S_l == 0 beside K > 0, with 29 frame slots (32 robots per wave) and with a hull at RMP2_MAX_HULL_VERTICES.

Reference: tests/hull_pair_reference.py (brute force, fp64) on the oracle's fp64 frames for the first 24 robots and the 8 nearest
to contact of each fleet of 67; oracle.step on its pairs; tests/hull_reference.py for the obstacle half.  Every robot of the 67 is
held without a reference by MEMBERSHIP: both points on their placed hulls, |p_link - p_obs| = dist, and the pair's own direction
separating the two hulls by dist -- which together pin the distance to the bound.

Bound: B = 1e-5 max(1, extent), the project's stage bound (tests/test_gpu_self_hulls.py ATOL) scaled by the largest |coordinate| of
any placed hull vertex over the fleet; the fp32 walk's share of it is at most 0.054 (tests/test_hull_trees_host.py).  Points are
held at B wherever the answer is determined (hull_tree_scene.reference; at most 0.4 % of a scene's entries are not), the direction
at 1e-3 where the hulls are apart by more than 1e-3.  Under the face rule with n* a face of B every vertex of that face is `the
vertex of B attaining the min`: such an entry passes with any of them as p_obs (same n*, same support plane, p_link = p_obs + dist n*).
Observed ratios: profiles/hull_trees.txt.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hull_reference as H  # noqa: E402
import hull_tree_scene as HT  # noqa: E402
import link_pair_scene as LS  # noqa: E402
import self_pair_scene as S  # noqa: E402
from test_gpu_self_collision import _engine, _interleave  # noqa: E402

pytestmark = pytest.mark.gpu

DIRECTION = 1e-3
BEYOND_GATE_CAP = 0.05
NO_CERTIFICATE_CAP = 0.05
KERNEL_NAME = {"hex": "rmp2_step_hex_kernel", "quad": "rmp2_step_quad_kernel", "lane": "one lane per robot"}
TABLE_TREES = [n for n, sp in S.TREES.items() if "p" not in sp["leaves"] and not sp["empty"]]   # all-`d`, every leaf with a hull
K_TABLE = 5


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _stage(torch, eng, q):
    out = eng.self_pairs(torch.from_numpy(np.ascontiguousarray(q)))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _placed(sc, T, e):
    """Vertices of hull entry e placed by frames T [R, F, 4, 4] ([R, V, 3], base coordinates) and its planes."""
    F = sc["table"].n_frames
    V, P = (a.astype(np.float64) for a in sc["hulls"].hull(e))
    if e == F:
        return np.broadcast_to(V, (len(T),) + V.shape), np.broadcast_to(np.eye(4), (len(T), 4, 4)), P
    return np.einsum("rij,vj->rvi", T[:, e, :3, :3], V) + T[:, e, None, :3, 3], T[:, e], P


def _plane_value(P, Tf, x):
    """Largest plane value of base-frame points x [R, 3] against the hull with planes P placed by Tf [R, 4, 4] (0: on the surface)."""
    loc = np.einsum("rji,rj->ri", Tf[:, :3, :3], x - Tf[:, :3, 3])
    return (loc @ P[:, :3].T - P[:, 3]).max(axis=1)


def _membership(sc, got, bound):
    """Every robot, no reference: returns (worst violation / bound, share of entries without a separation certificate).  The
    output in base coordinates is wl, wo = wl - dist n (attached-point leaves: relative_position placed by the fp64 frame, n =
    normal_vec, |n| = 1 held; distance leaves: n = (p_link - p_obs) / dist held by |p_link - p_obs| = dist).  Held: wo on B's
    placed hull.  Where n separates the hulls by dist (min_A n . x - max_B n . y >= dist - bound: the hulls are apart, no nearer
    than dist - bound): wl on A's placed hull too -- two points of the hulls at distance dist, so the distance is pinned to the
    bound.  Elsewhere (the face rule: p_link lies on the plane of n*, not necessarily on the face) the entry is only counted."""
    import oracle as O
    pl, po, dd = (a.astype(np.float64) for a in got)
    T = O.forward_kinematics(sc["desc"], sc["q"][:len(pl)], "f64")
    F = sc["table"].n_frames
    worst, without = 0.0, 0
    for j, (o, b) in enumerate(sc["pairs"]):
        fa = sc["leaf_frames"][o]
        VA, TA, PA = _placed(sc, T, fa)
        VB, TB, PB = _placed(sc, T, F if b < 0 else b)
        d = dd[:, j]
        if sc["kinds"][o] == "p":
            on_frame = np.abs((pl[:, j] @ PA[:, :3].T - PA[:, 3]).max(axis=1))        # relative_position on A, frame coordinates
            n = po[:, j]
            unit = np.abs(np.linalg.norm(n, axis=1) - 1.0)
            wl = np.einsum("rij,rj->ri", TA[:, :3, :3], pl[:, j]) + TA[:, :3, 3]
            wo = wl - d[:, None] * n
        else:
            wl, wo = pl[:, j], po[:, j]
            sep = np.linalg.norm(wl - wo, axis=1)
            unit = np.abs(sep - d)
            n = (wl - wo) / np.where(sep > 0, sep, 1.0)[:, None]
            on_frame = np.zeros(len(d))
        cert = (np.einsum("rvi,ri->rv", VA, n).min(axis=1) - np.einsum("rvi,ri->rv", VB, n).max(axis=1)) >= d - bound
        on_b = np.abs(_plane_value(PB, TB, wo))
        on_a = np.where(cert, np.maximum(np.abs(_plane_value(PA, TA, wl)), on_frame), 0.0)
        worst = max(worst, float(np.maximum(np.maximum(on_a, on_b), unit).max()))
        without += int((~cert).sum())
    return worst / bound, without / dd.size


def _check_against_reference(what, sc, got, rows, ref):
    """Rows `rows` of the output against the restatement: |dist - ref| <= B on every entry; both points within B wherever the
    answer is determined; the direction within DIRECTION where apart by more than DEEP.  Returns the worst ratios."""
    pl, po, dd = (a[rows].astype(np.float64) for a in got)
    rpl, rpo, rdd, gap, face = ref["ref64"]
    bound, det = ref["bound"], ref["det"]
    e_dist = np.abs(dd - rdd) / bound
    assert e_dist.max() <= 1.0, f"{what}: distance at {e_dist.max():.2f} of the bound {bound:.2e} (robot, pair {np.unravel_index(e_dist.argmax(), e_dist.shape)})"
    e_pts = np.maximum(np.abs(pl - rpl).max(-1), np.abs(po - rpo).max(-1)) / bound
    # the face rule with n* a face of B: any vertex of that face is y*.  Same n*, p_obs on the same support plane, the same offset
    other = det & face & (e_pts > 1.0)
    n_other = int(other.sum())
    for r, j in np.argwhere(other):
        o, b = sc["pairs"][j]
        if sc["kinds"][o] == "p":      # (normal_vec = n*, relative_position = y* + dist n* in the frame: held by membership above)
            assert np.abs(po[r, j] - rpo[r, j]).max() <= bound, (what, r, j)
            continue
        rn = (rpl[r, j] - rpo[r, j]) / rdd[r, j]
        assert abs((po[r, j] - rpo[r, j]) @ rn) <= bound, (what, r, j)
        if rdd[r, j] > HT.DEEP:        # (a shallower overlap leaves n* = (p_link - p_obs) / dist to rounding)
            assert np.abs((pl[r, j] - po[r, j]) / dd[r, j] - rn).max() <= 1e-4, (what, r, j)
        VB = _placed(sc, ref["T64"][r:r + 1], sc["table"].n_frames if b < 0 else b)[0][0]
        assert np.abs(VB - po[r, j]).max(axis=1).min() <= bound, (what, r, j)          # a vertex of B
    held = det & ~other
    assert e_pts[held].max(initial=0) <= 1.0, f"{what}: points at {e_pts[held].max():.2f} of the bound {bound:.2e} (robot, pair {np.unravel_index(np.where(held, e_pts, 0).argmax(), e_pts.shape)})"
    apart = ~face & (gap > HT.DEEP)
    point = np.repeat([k == "p" for k in sc["kinds"]], sc["counts"])
    u = np.where(point[None, :, None], po, (pl - po) / np.where(dd > 0, dd, 1.0)[..., None])
    ru = np.where(point[None, :, None], rpo, (rpl - rpo) / np.where(rdd > 0, rdd, 1.0)[..., None])
    e_dir = np.abs(u - ru).max(-1)
    assert e_dir[apart].max(initial=0) <= DIRECTION, f"{what}: direction off by {e_dir[apart].max():.2e}"
    return dict(dist=float(e_dist.max()), points=float(e_pts[held].max(initial=0)), direction=float(e_dir[apart].max(initial=0)),
                determined=float(det.mean()), face=int((face & det).sum()), other_vertex=n_other)


def _run_stage(torch, what, sc, fleets=()):
    """The stage on scene sc: finite, membership on every robot, the restatement on the subset; the first robots of the fleet
    alone (`fleets`) give the same bits."""
    eng = _engine(sc["desc"])
    eng.set_self_collision_hulls(sc["pairs"], sc["hulls"])
    assert eng.self_counts == sc["counts"] and eng.has_self_hulls
    got = _stage(torch, eng, sc["q"])
    assert got[2].shape == (len(sc["q"]), len(sc["pairs"]))
    assert all(np.isfinite(a).all() for a in got), f"{what}: non-finite output"
    rows = HT.subset(sc)
    ref = HT.reference(sc, rows)
    mem, without = _membership(sc, got, ref["bound"])
    assert mem <= 1.0, f"{what}: membership at {mem:.2f} of the bound"
    assert without <= NO_CERTIFICATE_CAP, f"{what}: {without:.1%} of the entries carry no separation certificate"
    w = _check_against_reference(what, sc, got, rows, ref)
    for R in fleets:
        part = _stage(torch, eng, sc["q"][:R])
        for a, b in zip(part, got):
            assert _same_bits(a, b[:R]), f"{what}: R = {R}"
    print(f"hull stage {what}: F = {sc['table'].n_frames}, dofs = {sc['table'].n_dof}, P = {len(sc['pairs'])}, counts {sc['counts']}, frame slots "
          f"{HT.lds_slots(sc)}, bound {ref['bound']:.2e}: worst ratio distance {w['dist']:.3f}, points {w['points']:.3f}, membership {mem:.3f}; "
          f"direction {w['direction']:.1e}; determined {w['determined']:.2%}, face-rule entries held {w['face']} (another vertex of B's face: "
          f"{w['other_vertex']}); without certificate {without:.2%}; subset of {len(rows)}")
    return eng, got


@pytest.mark.parametrize("name", list(S.TREES))
def test_self_stage_on_trees(torch_mod, name):
    """Every tree at R = 67 (one partial wave of 64); fleets of 1, 63, 64 and 65 give the first robots' bits.  Measured on an MI355X,
    worst over the eight trees: 0.040 of the bound on the distance (gaps), 0.051 on the points (sixteen), 0.076 on membership (bush);
    direction off by at most 5.3e-5; 24 face-rule entries held, 7 of them with another vertex of B's face.  A build with the sign
    of the skew matrix's x and y components flipped in walk_frame_position fails all eight (membership at 7.7e4 to 1.8e5 of the
    bound) and passes the Panda's stage tests."""
    _run_stage(torch_mod, name, HT.scene(name), fleets=(1, 63, 64, 65))


@pytest.mark.parametrize("which", HT.LISTS)
def test_self_stage_list_shapes(torch_mod, which):
    """(a) leaves without self pairs, (b) 29 frame slots: 32 robots per wave, fleets of 31, 32, 33 and 67, on the tree with two
    save slots, (c) two leaves on one frame with the same B's in another order: the same rows, bit for bit; a 512-vertex B.
    Measured on an MI355X: at most 0.038 of the bound on the distance, 0.050 on the points, 0.076 on membership; 20 face-rule
    entries held on the halved list."""
    sc = HT.list_scene(which)
    if which == "halved":
        slots = HT.lds_slots(sc)
        assert 4 * 12 * slots * 64 > 65536 >= 4 * 12 * slots * 32 and sc["table"].depth_first_schedule()[3] == 2
    eng, got = _run_stage(torch_mod, f"list {which}", sc, fleets=(31, 32, 33) if which == "halved" else ())
    if which == "twin_shared":
        c = sc["counts"]
        one, two = slice(c[0], c[0] + c[1]), slice(c[0] + c[1], c[0] + c[1] + c[2])
        for a in got:
            assert _same_bits(np.ascontiguousarray(a[:, one]), np.ascontiguousarray(a[:, two][:, ::-1]))


_TABLE_REF = {}


def _table_scene(name):
    return HT.list_scene(name) if name in HT.LISTS else HT.scene(name)


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
@pytest.mark.parametrize("name", TABLE_TREES + ["no_leaf_pairs"])
def test_obstacle_and_self_layout_on_trees(torch_mod, name, prim):
    """[K obstacle pairs | S_l self pairs] per leaf on trees: the staged step = the link-hull stage of a second handle, the self
    pairs, interleaved per leaf, an explicit-pair step of a plain handle -- bit for bit (`no_leaf_pairs`: some S_l == 0).  And the
    obstacle half itself, rmp2_hull_stage_kernel<0, 1, 2> on trees, against tests/hull_reference.py at B on the subset.  Measured
    on an MI355X: bit-equal in all 14 cases; at most 0.031 of the bound on the distance, 0.019 on p_link, 0.059 on p_obs."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    sc = _table_scene(name)
    rng = np.random.default_rng(57)
    tab = Cf.sample_spheres(rng, K_TABLE) if prim == "sphere" else Cf.sample_capsules(rng, K_TABLE)
    eng, lh, plain = _engine(sc["desc"]), _engine(sc["desc"]), _engine(sc["desc"])
    eng.set_self_collision_hulls(sc["pairs"], sc["hulls"])
    leaf_hulls = sc["hulls"].subset(sc["leaf_frames"])
    lh.set_link_hulls(leaf_hulls)
    counts = eng.self_counts
    assert counts == sc["counts"] and (name != "no_leaf_pairs" or 0 in counts)
    q, qd, goal = (torch.from_numpy(sc[k]).cuda() for k in ("q", "qd", "goal"))
    t = torch.from_numpy(tab).cuda()
    got = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=t))
    opl, opo, odd = lh.closest_points_hulls(q, lh.obstacles(spheres=t))
    spl, spo, _ = eng.self_pairs(q)
    pl, po = _interleave(torch, opl, opo, K_TABLE, spl, spo, counts)
    want = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=pl, p_obs=po, pair_counts=[K_TABLE + c for c in counts]))
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, want), (name, prim, (got - want).abs().max().item())
    # the obstacle half against its own reference
    rows = HT.subset(sc)
    key = (name, prim)
    if key not in _TABLE_REF:
        _TABLE_REF[key] = H.stage_np(sc["desc"], leaf_hulls, sc["q"][rows], tab, prim)
    rpl, rpo, rdd, gap = _TABLE_REF[key]
    bound = HT.bound_of(sc)[1]
    gl, go, gd = (a.cpu().numpy().astype(np.float64) for a in (opl, opo, odd))
    assert np.isfinite(gl).all() and np.isfinite(go).all() and np.isfinite(gd).all()
    e_d, e_l = np.abs(gd[rows] - rdd).max() / bound, np.abs(gl[rows] - rpl).max() / bound
    well = np.abs(gap) > 0.1          # tests/test_gpu_link_hulls.py _compare: the obstacle's point where the pair is 10 cm apart or more
    e_o = np.abs(go[rows] - rpo)[well].max(initial=0) / bound
    print(f"link-hull stage {name}/{prim}: L = {len(counts)}, K = {K_TABLE}, slots {sc['table'].depth_first_schedule()[3]}: worst ratio distance "
          f"{e_d:.3f}, p_link {e_l:.3f}, p_obs {e_o:.3f}; overlapping {int((gap < 0).sum())} of {gap.size}")
    assert e_d <= 1.0 and e_l <= 1.0 and e_o <= 1.0, (name, prim, e_d, e_l, e_o)


def test_table_refused_where_a_leaf_has_no_hull(torch_mod):
    """Tree `gaps`: three pair leaves sit on links without a shape, so an obstacle table has no hull to form their pairs on."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd._native import ERR_INVALID_ARGUMENT, Rmp2Error
    sc = HT.scene("gaps")
    eng = _engine(sc["desc"])
    eng.set_self_collision_hulls(sc["pairs"], sc["hulls"])
    q, qd, goal = (torch.from_numpy(sc[k]).cuda() for k in ("q", "qd", "goal"))
    t = torch.from_numpy(Cf.sample_spheres(np.random.default_rng(1), K_TABLE)).cuda()
    with pytest.raises(Rmp2Error) as e:
        eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=t))
    assert e.value.code == ERR_INVALID_ARGUMENT and "empty" in str(e.value), str(e.value)
    assert torch.isfinite(eng.step(q, qd, goal)).all()           # the self pairs alone still step


_STEP_REF = {}


def _step_ref(name, solve):
    import oracle as O
    if (name, solve) not in _STEP_REF:
        sc = HT.scene(name)
        rows = HT.subset(sc)
        ref = HT.reference(sc, rows)
        desc = sc["desc"] if solve == "auto" else sc["desc_pinv"]
        pl, po, dd = ref["ref64"][:3]
        kw = S.explicit_kwargs(sc, pl, po, dd)
        args = (desc, sc["q"][rows], sc["qd"][rows], sc["goal"][rows])
        far = S.far_pairs(sc, pl, po, dd)
        _STEP_REF[(name, solve)] = (rows, O.step(*args, **kw), O.fp32_resolution(*args, **kw), O.step(*args, **S.explicit_kwargs(sc, *far))["qdd64"], far)
    return _STEP_REF[(name, solve)]


@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("name", list(S.TREES))
def test_step_on_trees_vs_oracle(torch_mod, name, solve):
    """The staged step of every tree against oracle.step on the fp64 restatement's pairs through the accuracy gate, on every
    kernel the robot's size admits.  Robots beyond the gate (at most 5 % per case) are re-held to it on the stage's own pairs.  The
    same states with every pair out of range answer differently for the robots in reach.  Measured on an MI355X: no robot beyond
    the gate in any of the 40 (tree, kernel, solve) cases; median |qdd - ref| between 0.003 and 0.134 of 1e-5 max(1, |ref|)."""
    torch = torch_mod
    import oracle as O
    sc = HT.scene(name)
    desc = sc["desc"] if solve == "auto" else sc["desc_pinv"]
    rows, ref, spread, ref_far, far = _step_ref(name, solve)
    n = sc["table"].n_dof
    q, qd, goal = (torch.from_numpy(np.ascontiguousarray(sc[k][rows])).cuda() for k in ("q", "qd", "goal"))
    point = "p" in sc["kinds"]
    in_reach = np.abs(ref["qdd64"] - ref_far).max(axis=1) > LS.MATTERS
    assert in_reach.any()
    for kernel in (("hex", "quad", "lane") if n <= 9 else (None,)):       # (more than 9 dofs: the hex kernel alone takes the robot)
        eng = _engine(desc, kernel)
        eng.set_self_collision_hulls(sc["pairs"], sc["hulls"])
        qdd = eng.step(q, qd, goal).cpu().numpy()
        what = f"{name}/{kernel}/{solve}"
        assert KERNEL_NAME[kernel or "hex"] in eng.last_kernel(), (what, eng.last_kernel())
        assert np.isfinite(qdd).all(), what
        ok = O.accuracy_gate(qdd, {k: ref[k] for k in ("qdd64", "M", "f")}, spread=spread)["ok"]
        bad = ~ok
        e = np.abs(qdd - ref["qdd64"]).max(axis=1) / (HT.ATOL * np.maximum(1.0, np.abs(ref["qdd64"]).max(axis=1)))
        print(f"hull step {what}: {len(rows)} robots, {int(in_reach.sum())} in reach; beyond the gate on fp64 pairs {int(bad.sum())}; median |qdd - ref| / "
              f"(1e-5 max(1, |ref|)) {np.median(e):.3f}; {eng.last_kernel()}")
        assert bad.mean() <= BEYOND_GATE_CAP, f"{what}: {bad.sum()} of {len(bad)} robots beyond the gate on fp64 pairs"
        if bad.any():      # held to the gate on the stage's OWN pairs (pinned by test_self_stage_on_trees), none may fail
            dpl, dpo, ddd = _stage(torch, eng, sc["q"][rows][bad])
            kw = S.explicit_kwargs(sc, dpl, dpo, ddd)
            args = (desc, sc["q"][rows][bad], sc["qd"][rows][bad], sc["goal"][rows][bad])
            ref2 = O.step(*args, **kw)
            ok2 = O.accuracy_gate(qdd[bad], {k: ref2[k] for k in ("qdd64", "M", "f")}, spread=O.fp32_resolution(*args, **kw))["ok"]
            assert ok2.all(), f"{what}: {(~ok2).sum()} robots beyond the gate on the stage's own pairs"
        # every pair out of range: a plain handle on the far pairs
        plain = _engine(desc, kernel)
        fl, fo, fd = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in far)
        away = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=fl, p_obs=fo, pair_counts=sc["counts"], **(dict(dist=fd) if point else {}))).cpu().numpy()
        assert (np.abs(qdd - away).max(axis=1)[in_reach] > 0.5 * LS.MATTERS).all(), what


def _relation(t, joint, frame):
    """'above' (the joint moves the frame), 'below' (the joint sits under the frame) or 'apart' (another branch)."""
    def up(a):
        out = []
        while a >= 0:
            out.append(a)
            a = int(t.parent[a])
        return out
    if frame >= 0 and joint in up(frame):
        return "above"
    return "below" if frame in up(joint) else "apart"


def test_non_finite_q_on_a_tree(torch_mod):
    """Tree `bush`: NaN and Inf in a joint BELOW a pair's two frames and in a joint on ANOTHER BRANCH than both, in robots 0, 31 and
    66: every pair of those robots is NaN -- also the pairs whose frames the joint does not move --, the rest keep the clean bits."""
    torch = torch_mod
    sc = HT.scene("bush")
    t = sc["table"]
    joints = [f for f in range(t.n_frames) if t.q_index[f] >= 0]
    below = apart = None
    for o, b in sc["pairs"]:
        fa = sc["leaf_frames"][o]
        for f in joints if b >= 0 else []:
            rel = {_relation(t, f, fa), _relation(t, f, b)}
            if rel == {"below"}:
                below = below or (f, fa, b)
            if rel == {"apart"}:
                apart = (f, fa, b)            # (the last such joint: another one than `below`, checked next)
    assert below is not None and apart is not None and below[0] != apart[0]
    eng = _engine(sc["desc"])
    eng.set_self_collision_hulls(sc["pairs"], sc["hulls"])
    q = sc["q"].copy()
    bad = np.array([0, 31, 66])
    q[0, t.q_index[below[0]]], q[31, t.q_index[apart[0]]], q[66, t.q_index[below[0]]] = np.nan, np.inf, -np.inf
    clean, got = _stage(torch, eng, sc["q"]), _stage(torch, eng, q)
    ok = np.setdiff1d(np.arange(HT.FLEET), bad)
    for c, g in zip(clean, got):
        assert np.isfinite(c).all() and np.isnan(g[bad]).all(), np.argwhere(~np.isnan(g[bad]))[:4]
        assert _same_bits(c[ok], g[ok])

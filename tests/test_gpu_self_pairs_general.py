"""The capsule self-pair stage (rmp2_set_self_collision, rmp2_self_pairs, rmp2_self_stage_kernel, the staged rmp2_step) beyond the
Panda: random trees with one, two and no save/restore slots, up to 16 dofs and 31 frames, B links the step's pruned program does
not contain, pair leaves without self pairs, attached-point leaves mixed with distance leaves, two leaves on one frame; raw pair
lists of every shape up to the cap of 256; the LDS limit of 64 KiB; and link-versus-link DEGENERATE geometry with a B that moves
(tests/self_pair_scene.py).  Reference: tests/self_pair_reference.py in fp64 on the oracle's fp64 frames, oracle.step on its pairs.

Bounds
  stage on trees   |dist - ref| and |points - ref| <= 1e-5 max(1, extent): the project's stage bound (tests/test_gpu_self_collision.py)
                   scaled by the robot's largest capsule end-point coordinate in the fleet (1.5 .. 3.0 m here).  Envelope, measured
                   on the CPU before any GPU run (tests/test_self_pairs_host.py): the fp32 restatement of the reference uses at
                   most 0.028 of the bound on the distance and 0.103 on the points, <= 0.25, so the bound stands as it is.  The
                   distance is held on EVERY row.  The points are held on every row whose fp32 restatement meets the points bound
                   itself (all of them on these fleets; the share of the others is capped at 5 % per tree), and every row, exempt
                   or not, is held by membership: both points on their capsules' surfaces, p_link - p_obs = dist n, |n| = 1.
  degenerate rows  2e-6 on points and distance (POINTS of tests/test_gpu_link_pair_degenerate.py), exact values where the axes
                   intersect, bit equality of the moving B and the base-row B; the step at 1e-5 max(1, |qdd|) (EXPLICIT), no
                   robot exempt.
  step on trees    robots clear of self contact (5 cm) at 1e-5 max(1, |qdd|), the rest through oracle.accuracy_gate with
                   oracle.fp32_resolution; at most 5 % beyond it on fp64 pairs, each of those re-gated on the stage's own pairs.
Observed ratios: profiles/self_pairs_general.txt.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import self_pair_reference as SR  # noqa: E402
import self_pair_scene as S  # noqa: E402

pytestmark = pytest.mark.gpu

ATOL = 1e-5        # stage bound (x max(1, extent) on the trees) and the step's bound for robots clear of contact
POINTS = 2e-6      # tests/test_gpu_link_pair_degenerate.py POINTS
EXPLICIT = 1e-5    # tests/test_gpu_link_pair_degenerate.py EXPLICIT
EXEMPT_CAP = 0.05
WAVE_EDGES = [1, 15, 16, 17]
POISONED = [0, 15, 16, 66]


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


def _stage(torch, eng, q):
    out = eng.self_pairs(torch.from_numpy(np.ascontiguousarray(q)))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


_REF = {}


def _reference(key, s, pairs=None):
    """(geometry, (p_link, p_obs, dist, gap)) in fp64 and the fp32 restatement's points, computed once per key and left unchanged."""
    if key not in _REF:
        pairs = s["pairs"] if pairs is None else pairs
        g = SR.self_pair_geometry(s["desc"], pairs, s["caps"], s["q"])
        _REF[key] = (g, SR.self_pairs_np(s["desc"], pairs, s["caps"], s["q"], geometry=g),
                     SR.self_pairs_np(s["desc"], pairs, s["caps"], s["q"], np.float32)[:2])
    return _REF[key]


def _membership(g, got, rows=slice(None)):
    """Worst violation, over every (robot, pair) of `rows`, of: p_link on A's surface, p_obs on B's surface, p_link - p_obs =
    dist n with |n| = 1 (attached-point leaves: relative_position taken back to the base frame, p_obs = p_link - dist normal_vec)."""
    pl, po, dd = (a[rows].astype(np.float64) for a in got)
    A, B, C_, D_ = (g[k][rows] for k in "ABCD")
    wl, wo, unit = pl.copy(), po.copy(), np.zeros(dd.shape)
    for j in range(dd.shape[1]):
        if g["point"][j]:
            Tf = g["T"][rows][:, g["frame"][j]]
            wl[:, j] = np.einsum("rij,rj->ri", Tf[:, :3, :3], pl[:, j]) + Tf[:, :3, 3]
            unit[:, j] = np.abs(np.linalg.norm(po[:, j], axis=-1) - 1.0)
            wo[:, j] = wl[:, j] - dd[:, j, None] * po[:, j]
        else:
            unit[:, j] = np.abs(np.linalg.norm(wl[:, j] - wo[:, j], axis=-1) - dd[:, j])
    on_a = np.abs(SR.point_segment_distance(wl, A, B) - g["ra"][None])
    on_b = np.abs(SR.point_segment_distance(wo, C_, D_) - g["rb"][None])
    return np.maximum(np.maximum(on_a, on_b), unit)


def _check_stage(what, s, got, key, pairs=None, rows=None):
    """The stage's output `got` for robots `rows` of scene s against the reference: returns (distance, points, membership) worst
    ratios to the bound 1e-5 max(1, extent)."""
    g, (rpl, rpo, rdd, _), (pl32, po32) = _reference(key, s, pairs)
    rows = slice(None) if rows is None else rows
    pl, po, dd = got
    assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all(), f"{what}: non-finite output"
    assert dd.shape == rdd[rows].shape and pl.shape == rpl[rows].shape
    bound = ATOL * max(1.0, S.extent(s, g))
    e_dist = np.abs(dd - rdd[rows]) / bound
    assert e_dist.max(initial=0) <= 1.0, f"{what}: distance at {e_dist.max():.2f} of the bound {bound:.2e} (robot, pair {np.unravel_index(e_dist.argmax(), e_dist.shape)})"
    exempt = (np.maximum(np.abs(pl32 - rpl).max(axis=-1), np.abs(po32 - rpo).max(axis=-1)) > bound)
    assert exempt.mean() <= EXEMPT_CAP, f"{what}: {exempt.mean():.1%} of the rows exempt"
    e_pts = np.maximum(np.abs(pl - rpl[rows]).max(axis=-1), np.abs(po - rpo[rows]).max(axis=-1)) / bound
    held = ~exempt[rows]
    assert e_pts[held].max(initial=0) <= 1.0, f"{what}: points at {e_pts[held].max():.2f} of the bound {bound:.2e} (robot, pair {np.unravel_index(np.where(held, e_pts, 0).argmax(), e_pts.shape)})"
    e_mem = _membership(g, got, rows) / bound
    assert e_mem.max(initial=0) <= 1.0, f"{what}: membership at {e_mem.max():.2f} of the bound"
    return float(e_dist.max(initial=0)), float(e_pts[held].max(initial=0)), float(e_mem.max(initial=0))


@pytest.mark.parametrize("name", list(S.TREES))
def test_stage_on_trees(torch_mod, name):
    """1 and 2: every tree at R = 67 against the fp64 reference; the same fleet at R = 1, 15, 16 and 17 (rows of the first robots,
    bit for bit) and reversed (rows permute and keep their bits)."""
    torch = torch_mod
    tr = S.tree(name)
    eng = _engine(tr["desc"])
    eng.set_self_collision(tr["pairs"], tr["caps"])
    assert eng.self_counts == tr["counts"]
    full = _stage(torch, eng, tr["q"])
    assert full[2].shape == (S.FLEET, len(tr["pairs"]))
    worst = _check_stage(name, tr, full, ("tree", name))
    print(f"stage {name}: F = {tr['table'].n_frames}, dofs = {tr['table'].n_dof}, P = {len(tr['pairs'])}, counts {tr['counts']}: worst ratio "
          f"distance {worst[0]:.3f}, points {worst[1]:.3f}, membership {worst[2]:.3f}")
    for R in WAVE_EDGES:
        part = _stage(torch, eng, tr["q"][:R])
        for a, b in zip(part, full):
            assert np.array_equal(a, b[:R]), f"{name} R = {R}"
    rev = _stage(torch, eng, tr["q"][::-1])
    for a, b in zip(rev, full):
        assert np.array_equal(a, b[::-1]), f"{name} reversed"


def test_pair_list_shapes(torch_mod):
    """3: raw lists on the 9-dof tree.  Each against the reference; a shuffled list = its sorted form bit for bit; a repeated pair
    gives two identical rows; self_counts = the per-leaf counts; 256 pairs run and are right in the last row; 257 are refused with
    the cap in the message and the previous list stays active."""
    torch = torch_mod
    from riemannian_motion_policies_amd._native import ERR_INVALID_ARGUMENT, Rmp2Error
    tr = S.tree(S.LIST_TREE)
    shapes = S.list_shapes()
    L = len(tr["leaf_frames"])
    eng = _engine(tr["desc"])
    out = {}
    for name, lst in shapes.items():
        if name == "too_many":
            continue
        eng.set_self_collision(lst, tr["caps"])
        assert eng.self_counts == SR.counts_of(lst, L), name
        out[name] = _stage(torch, eng, tr["q"])
        assert out[name][2].shape == (S.FLEET, len(lst))
        worst = _check_stage(f"list {name}", tr, out[name], ("list", name), pairs=lst)
        print(f"list {name}: P = {len(lst)}, counts {eng.self_counts}: worst ratio distance {worst[0]:.3f}, points {worst[1]:.3f}")
    for a, b in zip(out["shuffled"], out["sorted"]):
        # (sorted by leaf, a leaf's pairs in the order given: the shuffled list's layout, re-ordered to the sorted list's)
        lay = SR.layout(shapes["shuffled"])
        cols = [[shapes["shuffled"][k] for k in lay].index(p) for p in shapes["sorted"]]
        assert np.array_equal(a[:, cols], b)
    lay = [shapes["repeated"][k] for k in SR.layout(shapes["repeated"])]
    twice = [j for j, p in enumerate(lay) if p == shapes["repeated"][1]]
    assert len(twice) == 2
    for a in out["repeated"]:
        assert np.array_equal(a[:, twice[0]], a[:, twice[1]])
    # the cap: the last row of 256 is right (checked above with every row); 257 are refused, the list of 256 stays
    eng.set_self_collision(shapes["total_256"], tr["caps"])
    before = _stage(torch, eng, tr["q"])
    g, (rpl, rpo, rdd, _), _ = _reference(("list", "total_256"), tr, shapes["total_256"])
    assert np.abs(before[2][:, 255] - rdd[:, 255]).max() <= ATOL * max(1.0, S.extent(tr, g))
    with pytest.raises(Rmp2Error) as e:
        eng.set_self_collision(shapes["too_many"], tr["caps"])
    assert e.value.code == ERR_INVALID_ARGUMENT and "at most 256" in str(e.value) and "257" in str(e.value), str(e.value)
    assert eng.self_counts == SR.counts_of(shapes["total_256"], L)
    after = _stage(torch, eng, tr["q"])
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_lds_boundary(torch_mod):
    """4: 40 attached-point leaves and 28 B slots on the 16-dof tree: 5 L + 2 n_b = 256 records per robot, 64 KiB for a wave's 16
    robots exactly -- accepted, runs, matches.  One more B slot: refused with the byte count, the accepted list stays active."""
    torch = torch_mod
    from riemannian_motion_policies_amd._native import ERR_UNSUPPORTED, Rmp2Error
    b = S.lds_boundary()
    eng = _engine(b["desc"])
    eng.set_self_collision(b["pairs"], b["caps"])
    assert eng.self_counts == b["counts"]
    got = _stage(torch, eng, b["q"])
    worst = _check_stage("LDS boundary", b, got, ("lds", 0))
    print(f"LDS boundary: L = {S.LDS_LEAVES}, n_b = {b['n_b']}, P = {len(b['pairs'])}, 65536 B of LDS: worst ratio distance {worst[0]:.3f}, "
          f"points {worst[1]:.3f}, membership {worst[2]:.3f}")
    over = S.lds_boundary(1)
    with pytest.raises(Rmp2Error) as e:
        eng.set_self_collision(over["pairs"], over["caps"])
    assert e.value.code == ERR_UNSUPPORTED and str(16 * 16 * 258) in str(e.value) and "LDS" in str(e.value), str(e.value)
    assert eng.self_counts == b["counts"]
    again = _stage(torch, eng, b["q"])
    for x, y in zip(got, again):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("shape", list(S.B_SHAPES))
def test_degenerate_stage(torch_mod, shape):
    """5, the stage: arm B's capsule against arm A's link, exactly crossing, parallel, collinear, of zero length, touching,
    overlapping -- B on its moving frame (the second walk of the kernel), and the same world capsule as the base row."""
    torch = torch_mod
    s = S.two_arm_gantry(shape)
    eng = _engine(s["desc"])
    T = eng.forward_kinematics(torch.from_numpy(s["q"])).cpu().numpy()
    import oracle as O
    assert np.array_equal(T.astype(np.float64), O.forward_kinematics(s["desc"], s["q"], "f64"))
    eng.set_self_collision(s["pairs"], s["caps"])
    assert eng.self_counts == [1, 1]
    got = _stage(torch, eng, s["q"])
    pl, po, dd = got
    assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all()
    g = SR.self_pair_geometry(s["desc"], s["pairs"], s["caps"], s["q"])
    rpl, rpo, rdd, gap = SR.self_pairs_np(s["desc"], s["pairs"], s["caps"], s["q"], geometry=g)
    mem = _membership(g, got)
    axis = np.linalg.norm(g["X"] - g["Y"], axis=-1)
    worst = 0.0
    for r, (name, cls) in enumerate(zip(s["names"], s["classes"])):
        for j in range(2):
            assert abs(dd[r, j] - rdd[r, j]) <= POINTS and mem[r, j] <= POINTS, (name, j, dd[r, j], rdd[r, j], mem[r, j])
            if axis[r, j] == 0:       # intersecting axes: the fixed normal +z, the shapes overlap by the sum of the radii
                assert dd[r, j] == np.float32(g["ra"][j] + g["rb"][j]), (name, j)
                assert np.array_equal(pl[r, j] - po[r, j], np.float32([0, 0, -(g["ra"][j] + g["rb"][j])])), (name, j, pl[r, j] - po[r, j])
            if j == 0 and cls in ("set", "crossing_set"):
                continue              # the nearest pair is a set: distance and membership hold it
            e = max(np.abs(pl[r, j] - rpl[r, j]).max(), np.abs(po[r, j] - rpo[r, j]).max())
            worst = max(worst, float(e))
            assert e <= POINTS, (name, j, e)
        if cls.startswith("crossing"):
            assert (axis[r] == 0).any(), name
    # the same world capsule as the base row: the same bits
    for r, b in enumerate(S.two_arm_gantry(shape, base=True)):
        eng.set_self_collision(b["pairs"], b["caps"])
        fixed = _stage(torch, eng, b["q"])
        for x, y in zip(fixed, got):
            assert np.array_equal(x[0], y[r]), (b["names"], x[0], y[r])
    print(f"degenerate stage {shape}: rows {s['names']}: worst point error {worst:.2e} (bound {POINTS:g}); moving B = base B bit for bit")


_STEP_REF = {}


def _gantry_ref(shape, solve, R):
    key = (shape, solve, R)
    if key not in _STEP_REF:
        s = S.tiled(S.two_arm_gantry(shape, solve), R)
        _STEP_REF[key] = (s, S.reference_step(s))
    return _STEP_REF[key]


@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("kernel", ["hex", "quad", "lane"])
@pytest.mark.parametrize("shape", list(S.B_SHAPES))
def test_degenerate_step(torch_mod, shape, kernel, solve):
    """5, the step: rmp2_step on the two-arm gantry (stage, then the explicit-pair step) against oracle.step on the fp64 pairs."""
    torch = torch_mod
    from riemannian_motion_policies_amd import descriptor as D
    worst = 0.0
    for R in (1, 67):
        s, ref = _gantry_ref(shape, solve, R)
        eng = _engine(s["desc"], kernel)
        eng.set_self_collision(s["pairs"], s["caps"])
        st = torch.zeros(R, dtype=torch.int32, device="cuda")
        out = eng.step(*(torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal")), status=st)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got).all(), (shape, kernel, solve, R)
        assert ((st.cpu().numpy() & D.STATUS_NONFINITE) == 0).all()
        ref64 = ref["qdd64"]
        ratio = np.abs(got - ref64).max(axis=1) / (EXPLICIT * np.maximum(1.0, np.abs(ref64).max(axis=1)))
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, f"{shape} {kernel} {solve} R={R}: row {s['names'][int(ratio.argmax())]} at {ratio.max():.2f} of {EXPLICIT:g}"
    print(f"degenerate step {shape} {kernel} {solve}: worst ratio {worst:.3f}; {eng.last_kernel()}")


_TREE_REF = {}


def _tree_ref(name, solve):
    import oracle as O
    key = (name, solve)
    if key not in _TREE_REF:
        tr = S.tree(name)
        desc = tr["desc"] if solve == "auto" else tr["desc_pinv"]
        pl, po, dd, gap = _reference(("tree", name), tr)[1]
        kw = S.explicit_kwargs(tr, pl, po, dd)
        args = (desc, tr["q"], tr["qd"], tr["goal"])
        _TREE_REF[key] = (O.step(*args, **kw), O.fp32_resolution(*args, **kw), gap.min(axis=1))
    return _TREE_REF[key]


def _gate(qdd, ref, clear, what, spread):
    """The pattern of tests/test_gpu_self_collision.py: clear robots at ATOL max(1, |qdd|), the rest through the accuracy gate."""
    import oracle as O
    ref64 = ref["qdd64"]
    e = np.abs(qdd.astype(np.float64) - ref64).max(axis=1)
    mag = np.maximum(1.0, np.abs(ref64).max(axis=1))
    ratio = float((e[clear] / (ATOL * mag[clear])).max(initial=0.0))
    assert ratio <= 1.0, f"{what}: clear robots at {ratio:.2f} of the bound"
    ok = np.ones(len(qdd), bool)
    rest = ~clear
    if rest.any():
        ok[rest] = O.accuracy_gate(qdd[rest], {k: ref[k][rest] for k in ("qdd64", "M", "f")}, spread=spread[rest])["ok"]
    return ok, ratio


@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("name", list(S.TREES))
def test_step_on_trees_vs_oracle(torch_mod, name, solve):
    """6: the staged step of every tree against oracle.step on the fp64 pairs, every mapping the robot's size admits."""
    torch = torch_mod
    import oracle as O
    tr = S.tree(name)
    desc = tr["desc"] if solve == "auto" else tr["desc_pinv"]
    ref, spread, near = _tree_ref(name, solve)
    clear = near >= S.CLEAR
    n = tr["table"].n_dof
    q, qd, goal = (torch.from_numpy(tr[k]).cuda() for k in ("q", "qd", "goal"))
    for kernel in (("hex", "quad", "lane") if n <= 9 else (None,)):
        eng = _engine(desc, kernel)
        eng.set_self_collision(tr["pairs"], tr["caps"])
        qdd = eng.step(q, qd, goal).cpu().numpy()
        what = f"{name}/{kernel}/{solve}"
        if n > 9:
            assert "rmp2_step_hex_kernel" in eng.last_kernel(), eng.last_kernel()
        ok, ratio = _gate(qdd, ref, clear, what, spread)
        bad = ~ok
        print(f"step {what}: clear robots {clear.sum()} of {len(clear)} at {ratio:.3f} of the bound; beyond the gate on fp64 pairs {bad.sum()}; {eng.last_kernel()}")
        assert bad.mean() <= 0.05, f"{what}: {bad.sum()} robots beyond the gate on fp64 pairs"
        if bad.any():      # held to the gate on the stage's OWN pairs (pinned by test_stage_on_trees), none may fail
            qb = tr["q"][bad]
            dpl, dpo, ddd = _stage(torch, eng, qb)
            kw = S.explicit_kwargs(tr, dpl, dpo, ddd)
            args = (desc, qb, tr["qd"][bad], tr["goal"][bad])
            ok2, _ = _gate(qdd[bad], O.step(*args, **kw), np.zeros(bad.sum(), bool), what + " device pairs", O.fp32_resolution(*args, **kw))
            assert ok2.all(), f"{what}: {(~ok2).sum()} robots beyond the gate on the stage's own pairs"


def _interleave(torch, obs_pl, obs_po, K, self_pl, self_po, counts):
    parts_l, parts_o, off = [], [], 0
    for i, c in enumerate(counts):
        parts_l += [obs_pl[:, i * K:(i + 1) * K], self_pl[:, off:off + c]]
        parts_o += [obs_po[:, i * K:(i + 1) * K], self_po[:, off:off + c]]
        off += c
    return torch.cat(parts_l, dim=1).contiguous(), torch.cat(parts_o, dim=1).contiguous()


@pytest.mark.parametrize("name", list(S.TREES))
def test_composition_bit_equal_on_trees(torch_mod, name):
    """7: eng.step = closest_points, then self_pairs, interleaved per leaf, then the explicit-pair step of a plain handle -- bit
    for bit, with a sphere table, with a capsule table and link capsules, and self pairs alone; the mixed tree refuses a table."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    from riemannian_motion_policies_amd._native import ERR_UNSUPPORTED, Rmp2Error
    tr = S.tree(name)
    rng = np.random.default_rng(41)
    K = 7
    eng, plain = _engine(tr["desc"]), _engine(tr["desc"])
    eng.set_self_collision(tr["pairs"], tr["caps"])
    counts = eng.self_counts
    q, qd, goal = (torch.from_numpy(tr[k]).cuda() for k in ("q", "qd", "goal"))
    spl, spo, sdd = eng.self_pairs(q)
    point = "p" in tr["kinds"]
    # the self pairs alone
    got0 = eng.step(q, qd, goal)
    want0 = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=spl, p_obs=spo, pair_counts=counts, **(dict(dist=sdd) if point else {})))
    torch.cuda.synchronize()
    assert torch.equal(got0, want0), (got0 - want0).abs().max().item()
    lc = torch.from_numpy(np.ascontiguousarray(tr["caps"][tr["leaf_frames"]])).cuda()
    for prim in ("sphere", "capsule"):
        tab = Cf.sample_spheres(rng, K) if prim == "sphere" else Cf.sample_capsules(rng, K)
        t = torch.from_numpy(tab).cuda()
        links = lc if prim == "capsule" else None
        if point:
            with pytest.raises(Rmp2Error) as e:
                eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=t, link_capsules=links))
            assert e.value.code == ERR_UNSUPPORTED and "attached-point" in str(e.value), str(e.value)
            continue
        got = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=t, link_capsules=links))
        opl, opo = eng.closest_points(q, eng.obstacles(spheres=t), link_capsules=links)
        pl, po = _interleave(torch, opl, opo, K, spl, spo, counts)
        want = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=pl, p_obs=po, pair_counts=[K + c for c in counts]))
        torch.cuda.synchronize()
        assert torch.equal(got, want), (name, prim, (got - want).abs().max().item())


@pytest.mark.parametrize("name", ["bush", "mixed", "sixteen"])
def test_containment(torch_mod, name):
    """8: NaN / Inf in q of robots 0, 15, 16 and 66: every other robot's stage rows and step qdd keep their bits; the poisoned
    robots' qdd is non-finite with the step's non-finite status.  R = 0 writes nothing."""
    torch = torch_mod
    from riemannian_motion_policies_amd import descriptor as D
    tr = S.tree(name)
    eng = _engine(tr["desc"])
    eng.set_self_collision(tr["pairs"], tr["caps"])
    q = tr["q"].copy()
    for r, v in zip(POISONED, (np.nan, np.inf, np.nan, -np.inf)):
        q[r, r % q.shape[1]] = v
    others = np.setdiff1d(np.arange(S.FLEET), POISONED)
    clean, dirty = _stage(torch, eng, tr["q"]), _stage(torch, eng, q)
    for a, b in zip(clean, dirty):
        assert np.array_equal(a[others], b[others])
    qd, goal = (torch.from_numpy(tr[k]).cuda() for k in ("qd", "goal"))
    st = torch.zeros(S.FLEET, dtype=torch.int32, device="cuda")
    out_clean = eng.step(torch.from_numpy(tr["q"]).cuda(), qd, goal).cpu().numpy()
    out_dirty = eng.step(torch.from_numpy(q).cuda(), qd, goal, status=st).cpu().numpy()
    status = st.cpu().numpy()
    assert np.array_equal(out_clean[others], out_dirty[others]) and np.isfinite(out_clean).all()
    assert not np.isfinite(out_dirty[POISONED]).any(), out_dirty[POISONED]
    assert ((status[POISONED] & D.STATUS_NONFINITE) != 0).all() and ((status[others] & D.STATUS_NONFINITE) == 0).all()
    # R = 0: accepted, nothing written
    S_ = len(tr["pairs"])
    pl = torch.full((1, S_, 3), 7.0, device="cuda")
    po, dd = pl.clone(), torch.full((1, S_), 7.0, device="cuda")
    qz = torch.from_numpy(tr["q"][:1]).cuda()
    rc = eng._lib.rmp2_self_pairs(eng._h, qz.data_ptr(), pl.data_ptr(), po.data_ptr(), dd.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and (pl == 7.0).all() and (po == 7.0).all() and (dd == 7.0).all()

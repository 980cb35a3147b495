"""The hull closest points at DEGENERATE geometry on the GPU: the catalogue of tests/hull_scene.py -- a centre on a vertex, an
edge, a face and at the centre of the cube, segments parallel to a face and an edge, lying on an edge and in a face plane, touching
at an endpoint, piercing, inside, the grazing pair -- on scenes whose kinematics are exact in fp32, through the hull stage
(rmp2_closest_points_hulls), the hull step on every mapping, and the stages' non-finite contract (include/rmp2.h).

Bounds: the stage against fp64 CLOSED FORMS at the project's stage bound ATOL = 1e-5 (rows whose nearest pair is a set or whose face
rule ties are named in the catalogue and held by membership); every other pair of every robot against the fp64 restatement
(tests/hull_reference.py) at ATOL; the step against oracle.step on the fp64 pairs through oracle.accuracy_gate with
oracle.fp32_resolution, every in-range row, no allowance.  The worst observed ratio to each bound is printed per test and recorded
in profiles/hull_degenerate_ab.txt.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hull_reference as H  # noqa: E402
import hull_scene as HS  # noqa: E402
import link_pair_scene as LS  # noqa: E402

pytestmark = pytest.mark.gpu

ATOL = 1e-5
# rows that cannot matter to a step: the far pair; a sphere of radius 0 ON the hull (distance 0 is the leaves' pole: the oracle
# itself answers NaN)
OUT_OF_RANGE = {"seg_far", "sphere_r0_on_face"}
# ... and, for the FK_DISTANCE leaf only, the two rows the face rule takes 0.5 + r = 0.625 deep: the obstacle leaf's reach ends before
DEEP = {"pt_at_centre", "seg_graze"}


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


_DESC = {}


def _desc(swap, solve="auto"):
    if (swap, solve) not in _DESC:
        _DESC[(swap, solve)] = HS.gantry_desc(swap, solve)
    return _DESC[(swap, solve)]


def _stage(torch, eng, q, table):
    out = eng.closest_points_hulls(torch.from_numpy(np.ascontiguousarray(q)).cuda(),
                                   eng.obstacles(spheres=torch.from_numpy(np.ascontiguousarray(table)).cuda()))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _cut(s, R):
    """The first R robots of a scene."""
    return dict(s, q=s["q"][:R], qd=s["qd"][:R], goal=s["goal"][:R], origin=s["origin"][:R])


def _check_fleet(got, desc, hulls, s, swap, worst):
    """EVERY pair of every robot of the scene `s` against fp64 at ATOL.  Robot k's pair with record k on the cube leaf (k < the
    catalogue rows in the table) against the row's closed form, a named row through its candidates (hull_scene.check_stage_answer:
    the catalogue's own directions, nothing recovered from the answer).  Every other pair against the restatement: gap, p_link
    and p_obs -- except the pairs whose nearest pair is a SET, decided beforehand from the geometry
    (hull_scene.nearest_pair_is_a_set: an ordinary robot beside an axis-parallel record), which are held by membership at ATOL
    with the restatement's direction, unique while the bodies are apart."""
    pl, po, dd = (g.astype(np.float64) for g in got)
    R, K = len(s["q"]), len(s["table"])
    kind = "capsule" if s["table"].shape[1] == 8 else "sphere"
    assert pl.shape == (R, 2 * K, 3) and dd.shape == (R, 2 * K)
    assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all()
    rpl, rpo, rdd, rgap = H.stage_np(desc, hulls, s["q"], s["table"], kind)
    tab = s["table"].astype(np.float64)
    HV = [tuple(x.astype(np.float64) for x in hulls.hull(o)) for o in range(2)]
    for r_ in range(R):
        for p_ in range(2 * K):
            o, k = divmod(p_, K)
            point = swap == (o == 0)
            org = s["origin"][r_] + (np.array([0.5, 0.0, 0.0]) if o == 1 else 0.0)
            a = tab[k, :3] - org
            b = (tab[k, 4:7] if kind == "capsule" else tab[k, :3]) - org
            if o == 0 and k == r_ and r_ < len(s["rows"]):            # the robot's own catalogue pair
                row = s["rows"][r_]
                w = HS.check_stage_answer(HS.candidates(row), HV[0][1], row["a"], row["b"], row["r"], row["sep"] - row["r"], org, point,
                                          pl[r_, p_], po[r_, p_], dd[r_, p_], ATOL, what=(row["name"], swap))
                worst["closed"] = max(worst["closed"], w)
            elif kind == "capsule" and HS.nearest_pair_is_a_set(*HV[o], a, b):
                _, _, u_ref, g_ref = H.hull_closest(*HV[o], a[None], b[None], [tab[k, 3]])
                assert abs(g_ref[0] - rgap[r_, p_]) <= 1e-9
                w = HS.check_stage_answer([(u_ref[0], None, None)], HV[o][1], a, b, tab[k, 3], g_ref[0], org, point,
                                          pl[r_, p_], po[r_, p_], dd[r_, p_], ATOL, what=("set", r_, p_))
                worst["restatement"] = max(worst["restatement"], w)
                worst["sets"] = worst.get("sets", 0) + 1
            else:
                e = max(np.abs(pl[r_, p_] - rpl[r_, p_]).max(), np.abs(po[r_, p_] - rpo[r_, p_]).max(), abs(dd[r_, p_] - rdd[r_, p_]))
                assert e <= ATOL, (r_, p_, e, pl[r_, p_], rpl[r_, p_], po[r_, p_], rpo[r_, p_])
                worst["restatement"] = max(worst["restatement"], e / ATOL)


def test_scenes_are_exact(torch_mod):
    """The precondition: the jr frame (the cube's) of every scene equals the fp64 one bit for bit, in the oracle's fp32 kinematics
    and in the engine's, and sits where the scene says."""
    torch = torch_mod
    import oracle as O
    t, desc = _desc(False)
    eng = _engine(desc)
    jr = t.frame_index("jr")
    for points in (True, False):
        for ch in HS.chunks(HS.gpu_rows(points)):
            s = HS.scene(ch, not points, ordinary=3)
            T64 = O.forward_kinematics(desc, s["q"], "f64")[:, jr]
            assert np.array_equal(O.forward_kinematics(desc, s["q"], "f32")[:, jr].astype(np.float64), T64)
            T = eng.forward_kinematics(torch.from_numpy(s["q"])).cpu().numpy()[:, jr]
            assert np.array_equal(T.astype(np.float64), T64) and np.array_equal(T64[:, :3, 3], s["origin"])
            assert np.array_equal(T64[:, :3, :3], np.broadcast_to(np.eye(3), T64[:, :3, :3].shape))


@pytest.mark.parametrize("swap", [False, True], ids=["cube_distance_leaf", "cube_point_leaf"])
@pytest.mark.parametrize("prim", ["sphere", "capsule"])
def test_stage_catalogue(torch_mod, prim, swap):
    """closest_points_hulls on one robot row per catalogue case, sphere tables (the point rows) and capsule tables (every row, the
    point rows as zero-length records), the cube on an FK_DISTANCE leaf and on an FK_POINT leaf.  Measured on an MI355X: worst
    error against the closed forms 0.12 of ATOL (1.2e-6: the fp32 rounding of surd answers at coordinates up to 40; dyadic answers
    come out exact: 0.001 on the FK_POINT leaf, whose outputs stay in the frame), against the restatement 0.37 of ATOL (the far
    quarter cube's pairs, coordinates up to 80).  No exact row misses ATOL in fp32."""
    torch = torch_mod
    t, desc = _desc(swap)
    hulls = HS.gantry_hulls()
    eng = _engine(desc)
    eng.set_link_hulls(hulls)
    worst = dict(closed=0.0, restatement=0.0)
    rows = HS.gpu_rows(prim == "sphere")
    for ch in HS.chunks(rows):
        s = HS.scene(ch, prim == "capsule")
        _check_fleet(_stage(torch, eng, s["q"], s["table"]), desc, hulls, s, swap, worst)
    assert {r["kind"] for r in rows} == {"unique", "tie"} | ({"set"} if prim == "capsule" else set())
    print(f"hull stage catalogue {prim} swap={swap}: {len(rows)} rows, worst / ATOL: closed forms {worst['closed']:.3f}, restatement {worst['restatement']:.3f}")


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
def test_kernel_shapes_against_the_reference(torch_mod, prim):
    """The hull stage's launch shapes: 16 robots per wave and a lane per (robot, record) pair, it / K with K not a power of two --
    R in {1, 15, 16, 17, 33} x K in {1, 3, 5}, catalogue rows first and ordinary robots (random dyadic positions) behind them,
    EVERY pair of every robot against fp64.  Measured on an MI355X: worst 0.12 of ATOL against the closed forms, 0.38 against the
    restatement; 30 pairs of ordinary robots beside an axis-parallel capsule have a set of nearest pairs (decided beforehand from
    the geometry) and are held by membership with the restatement's direction, at ATOL as well."""
    torch = torch_mod
    hulls = HS.gantry_hulls()
    rows = HS.gpu_rows(prim == "sphere")
    worst = dict(closed=0.0, restatement=0.0)
    n = 0
    for swap in (False, True):
        t, desc = _desc(swap)
        eng = _engine(desc)
        eng.set_link_hulls(hulls)
        for R in (1, 15, 16, 17, 33):
            for K in (1, 3, 5):
                ch = [rows[(n * 5 + j) % len(rows)] for j in range(K)]      # a window that walks through the catalogue
                ch = sorted(ch, key=lambda r: r["name"] != "seg_graze_near")
                n += 1
                s = _cut(HS.scene(ch, prim == "capsule", ordinary=max(R - K, 0), seed=n), R)
                _check_fleet(_stage(torch, eng, s["q"], s["table"]), desc, hulls, s, swap, worst)
    print(f"hull stage shapes {prim}: {n} fleets, worst / ATOL: closed forms {worst['closed']:.3f}, restatement {worst['restatement']:.3f}; "
          f"{worst.get('sets', 0)} pairs of ordinary robots decided beforehand to have a set of nearest pairs, held by membership")


def _moved_away(table):
    tab = np.array(table, np.float32)
    tab[:, :3] += np.float32(1024.0)
    if tab.shape[1] == 8:
        tab[:, 4:7] += np.float32(1024.0)
    return tab


def _reference_pairs(desc, hulls, s, swap, stage):
    """The fp64 pairs of the scene for the oracle: the restatement's, robot k's own pair replaced by its row's closed form -- or, for
    a named row (whose answer is not unique: any member is right), by the stage's own pair, which test_stage_catalogue holds to the
    membership rules."""
    kind = "capsule" if s["table"].shape[1] == 8 else "sphere"
    pl, po, dd, _ = H.stage_np(desc, hulls, s["q"], s["table"], kind)
    for k, row in enumerate(s["rows"]):
        if row["kind"] == "unique":
            pl[k, k], po[k, k], dd[k, k] = HS.expected_pair(row, s["origin"][k], swap)
        else:
            pl[k, k], po[k, k], dd[k, k] = stage[0][k, k], stage[1][k, k], stage[2][k, k]
    return pl.astype(np.float32), po.astype(np.float32), dd.astype(np.float32)


@pytest.mark.parametrize("swap", [False, True], ids=["cube_distance_leaf", "cube_point_leaf"])
@pytest.mark.parametrize("solve", ["auto", "pinv"])
@pytest.mark.parametrize("kernel", ["hex", "quad", "lane"])
def test_step_vs_oracle(torch_mod, kernel, solve, swap):
    """Engine.step with hulls on the catalogue scenes against oracle.step on the fp64 pairs, through oracle.accuracy_gate with
    oracle.fp32_resolution as tests/test_gpu_link_hulls.py test_step_vs_oracle does -- but every row must pass, and every row
    meant to be in range moves the oracle's fp64 qdd by more than MATTERS when the table is moved away.  Measured on an MI355X:
    every row inside the gate on hex, quad and lane; worst |qdd - qdd64| / max(1, |qdd64|) 2.1e-7 (0.02 of the gate's 1e-5)."""
    torch = torch_mod
    import oracle as O
    from riemannian_motion_policies_amd import descriptor as D
    t, desc = _desc(swap, solve)
    hulls = HS.gantry_hulls()
    eng = _engine(desc, kernel)
    eng.set_link_hulls(hulls)
    worst, n = 0.0, 0
    for points in (True, False):
        rows = [r for r in HS.gpu_rows(points) if r["name"] != "sphere_r0_on_face"]
        for ch in HS.chunks(rows):
            s = HS.scene(ch, not points)
            K = len(ch)
            tab = torch.from_numpy(s["table"]).cuda()
            q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
            st = torch.zeros(len(ch), dtype=torch.int32, device="cuda")
            qdd = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=tab), status=st).cpu().numpy()
            assert KERNEL_NAME[kernel] in eng.last_kernel(), (kernel, eng.last_kernel())
            assert np.isfinite(qdd).all() and ((st.cpu().numpy() & D.STATUS_NONFINITE) == 0).all(), [r["name"] for r in ch]
            stage = _stage(torch, eng, s["q"], s["table"])
            pl, po, dd = _reference_pairs(desc, hulls, s, swap, stage)
            args = (desc, s["q"], s["qd"], s["goal"])
            kw = dict(p_link=pl, p_obs=po, dist=dd, pair_counts=[K, K])
            ref = O.step(*args, **kw)
            verdict = O.accuracy_gate(qdd, {k: ref[k] for k in ("qdd64", "M", "f")}, spread=O.fp32_resolution(*args, **kw))
            assert verdict["ok"].all(), (kernel, solve, swap, [r["name"] for r, ok in zip(ch, verdict["ok"]) if not ok])
            worst = max(worst, float((np.abs(qdd - ref["qdd64"]).max(1) / np.maximum(1.0, np.abs(ref["qdd64"]).max(1))).max()))
            # every row meant to be in range matters (as link_pair_scene.rows_in_range)
            far = _stage(torch, eng, s["q"], _moved_away(s["table"]))
            away = O.step(*args, p_link=far[0], p_obs=far[1], dist=far[2], pair_counts=[K, K])["qdd64"]
            moved = np.abs(ref["qdd64"] - away).max(axis=1)
            skip = OUT_OF_RANGE | (set() if swap else DEEP)
            weak = [r["name"] for r, m in zip(ch, moved) if r["name"] not in skip and not m > LS.MATTERS]
            assert not weak, f"rows meant to be in range that do not matter: {weak}"
            n += len(ch)
    print(f"hull step {kernel} {solve} swap={swap}: {n} rows inside the gate, worst |qdd - qdd64| / max(1, |qdd64|) {worst:.2e}; {eng.last_kernel()}")


# ---- non-finite inputs (include/rmp2.h: the hull stages' contract) ------------------------------------------------------------

def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _nan_fleet(prim="capsule"):
    rows = HS.gpu_rows(prim == "sphere")[:5]
    return HS.scene(rows, prim == "capsule", ordinary=28, seed=5)


@pytest.mark.parametrize("swap", [False, True], ids=["cube_distance_leaf", "cube_point_leaf"])
def test_non_finite_q(torch_mod, swap):
    """A fleet of 33 robots with q poisoned in rows 0, 16 and 32 (NaN, +inf, -inf, each in another joint): every pair output of
    those robots is NaN, every other robot's is bit-identical to the clean fleet's; the hull step equals the explicit-pair step on
    the stage's own output bit for bit (NaN for NaN), gives NaN on every joint with RMP2_STATUS_NONFINITE for the poisoned robots
    and the clean fleet's bits for the others."""
    torch = torch_mod
    from riemannian_motion_policies_amd import descriptor as D
    t, desc = _desc(swap)
    eng, plain = _engine(desc), _engine(desc)
    eng.set_link_hulls(HS.gantry_hulls())
    s = _nan_fleet()
    bad = np.array([0, 16, 32])
    q = s["q"].copy()
    q[0, 1], q[16, 3], q[32, 2] = np.nan, np.inf, -np.inf
    clean, got = _stage(torch, eng, s["q"], s["table"]), _stage(torch, eng, q, s["table"])
    ok = np.setdiff1d(np.arange(33), bad)
    for c, g in zip(clean, got):
        assert np.isnan(g[bad]).all(), np.argwhere(~np.isnan(g[bad]))[:4]
        assert _same_bits(c[ok], g[ok])
        assert np.isfinite(c).all()

    def step(e, qq, obs):
        st = torch.zeros(33, dtype=torch.int32, device="cuda")
        out = e.step(torch.from_numpy(qq).cuda(), torch.from_numpy(s["qd"]).cuda(), torch.from_numpy(s["goal"]).cuda(), obstacles=obs, status=st)
        torch.cuda.synchronize()
        return out.cpu().numpy(), st.cpu().numpy()

    tab = torch.from_numpy(s["table"]).cuda()
    a_clean, st_clean = step(eng, s["q"], eng.obstacles(spheres=tab))
    a, st = step(eng, q, eng.obstacles(spheres=tab))
    dev = [torch.from_numpy(g).cuda() for g in got]
    b, st_b = step(plain, q, plain.obstacles(p_link=dev[0], p_obs=dev[1], dist=dev[2]))
    assert _same_bits(a, b) or (np.array_equal(np.isnan(a), np.isnan(b)) and _same_bits(np.nan_to_num(a), np.nan_to_num(b)))
    assert np.array_equal(st, st_b)
    assert np.isnan(a[bad]).all() and ((st[bad] & D.STATUS_NONFINITE) != 0).all()
    assert _same_bits(a[ok], a_clean[ok]) and np.array_equal(st[ok], st_clean[ok]) and np.isfinite(a_clean).all()


@pytest.mark.parametrize("prim", ["sphere", "capsule"])
def test_non_finite_record(torch_mod, prim):
    """One poisoned record in a table of five -- a NaN or an inf in a, in b (capsules), in r, in the capsule record's unused float --:
    p_link, p_obs and dist of that record's pairs are NaN for every robot and both leaves; every other pair is bit-identical to the
    clean table's.  (A NaN in b alone used to be answered as the sphere at a: finite, and wrong.)  The hull step on EACH poisoned
    table equals the explicit-pair step on the stage's own output, NaN for NaN."""
    torch = torch_mod
    t, desc = _desc(False)
    eng, plain = _engine(desc), _engine(desc)
    eng.set_link_hulls(HS.gantry_hulls())
    s = _nan_fleet(prim)
    K = 5
    clean = _stage(torch, eng, s["q"], s["table"])
    assert all(np.isfinite(c).all() for c in clean)
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    cols = [0, 3] + ([4, 6, 7] if prim == "capsule" else [])
    for col in cols:
        for j, val in ((2, np.nan), (0, np.inf), (4, -np.inf)):
            tab = s["table"].copy()
            tab[j, col] = val
            got = _stage(torch, eng, s["q"], tab)
            hit = np.zeros(2 * K, bool)
            hit[[j, K + j]] = True
            for c, g in zip(clean, got):
                assert np.isnan(g[:, hit]).all(), (prim, col, j, val, g[:, hit][~np.isnan(g[:, hit])][:4])
                assert _same_bits(np.ascontiguousarray(c[:, ~hit]), np.ascontiguousarray(g[:, ~hit])), (prim, col, j, val)
            # the hull step on this table against the explicit-pair step on the stage's own output, NaN for NaN
            a_ = eng.step(q, qd, goal, obstacles=eng.obstacles(spheres=torch.from_numpy(tab).cuda()))
            dev = [torch.from_numpy(g).cuda() for g in got]
            b_ = plain.step(q, qd, goal, obstacles=plain.obstacles(p_link=dev[0], p_obs=dev[1], dist=dev[2]))
            torch.cuda.synchronize()
            a_, b_ = a_.cpu().numpy(), b_.cpu().numpy()
            assert np.array_equal(np.isnan(a_), np.isnan(b_)) and _same_bits(np.nan_to_num(a_), np.nan_to_num(b_)), (prim, col, j, val)
            assert np.isnan(a_).any()

def test_non_finite_q_poisons_upstream_leaves(torch_mod, golden_dir):
    """The contract is per ROBOT: on the Panda a NaN in the last joint (a finger) leaves the frames of the seven leaves upstream
    of it finite, and their pairs must be NaN all the same.  33 robots, rows 0, 16 and 32 poisoned; the others keep their bits."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    table, desc = Cf.config3()
    z = np.load(os.path.join(golden_dir, "panda_collision_meshes.npz"))
    meshes = {str(n): (z[f"{n}.vertices"], z[f"{n}.xyz"], z[f"{n}.rpy"]) for n in z["links"]}
    eng = _engine(desc)
    eng.set_link_hulls(U.link_hulls(table, Cf.CONTROL_POINT_FRAMES, meshes))
    rng = np.random.default_rng(41)
    q0 = Cf.sample_panda_states(rng, 33)["q"]
    tab = Cf.sample_capsules(rng, 3)
    q = q0.copy()
    bad = np.array([0, 16, 32])
    q[0, 8], q[16, 7], q[32, 8] = np.nan, np.inf, -np.inf
    clean, got = _stage(torch, eng, q0, tab), _stage(torch, eng, q, tab)
    ok = np.setdiff1d(np.arange(33), bad)
    for c, g in zip(clean, got):
        assert np.isfinite(c).all() and np.isnan(g[bad]).all(), np.argwhere(~np.isnan(g[bad]))[:4]
        assert _same_bits(c[ok], g[ok])


# ---- hull-versus-hull self pairs --------------------------------------------------------------------------------------------------
import hull_pair_reference as HP  # noqa: E402


def _self_expected(row, pA, point):
    """The closed form of a "unique" pair row in the self stage's convention: FK_DISTANCE both points in the base frame, FK_POINT
    relative_position pa (A's frame), normal_vec sign(gap) u, dist |gap|."""
    if point:
        return row["pa"], (1.0 if row["sep"] >= 0 else -1.0) * row["u"], abs(row["sep"])
    return row["pa"] + pA, row["pb"] + pA, abs(row["sep"])


def _check_twin(got, s, swap, worst):
    """Every self pair of the twin gantry against fp64 at ATOL: robot k's catalogue pair against the row (hull_scene.check_self_answer:
    closed form, or the row's own direction(s) and membership), the rest against the restatement (bodies beyond each other's
    corner: unique)."""
    pl, po, dd = (g.astype(np.float64) for g in got)
    assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all()
    rpl, rpo, rdd, rgap, _ = HP.self_hull_pairs_np(s["desc"], s["hulls"], s["pairs"], s["q"])
    own = np.zeros(dd.shape, bool)
    for k, row in enumerate(s["rows"]):
        j = s["own"][k]
        own[k, j] = True
        worst["closed"] = max(worst["closed"], HS.check_self_answer(row, s["pA"][k], swap, pl[k, j], po[k, j], dd[k, j], ATOL))
    rest = ~own
    e = max(np.abs(pl - rpl).max(-1)[rest].max(), np.abs(po - rpo).max(-1)[rest].max(), np.abs(dd - rdd)[rest].max())
    assert e <= ATOL, (e, np.argwhere((np.maximum(np.abs(pl - rpl).max(-1), np.abs(po - rpo).max(-1)) > ATOL) & rest)[:4])
    worst["restatement"] = max(worst["restatement"], e / ATOL)


KERNEL_NAME = {"hex": "rmp2_step_hex_kernel", "quad": "rmp2_step_quad_kernel", "lane": "one lane per robot"}
# self rows that cannot matter to a step: the far pair, and coincident cubes, which the face rule takes a whole cube (1.0) deep
SELF_OUT_OF_RANGE = {"far", "coincident"}


@pytest.mark.parametrize("swap", [False, True], ids=["distance_leaf", "point_leaf"])
def test_self_pairs_catalogue(torch_mod, swap):
    """Engine.self_pairs on the twin gantry (two prismatic branches; a unit cube on one, on the other a unit cube and three more on
    fixed frames turned 45 degrees about z, 45 degrees about y and by the skew-edge rotation; a quarter cube as the base link):
    every row of the hull-pair catalogue -- faces parallel and apart (aligned, offset by half, turned 45 degrees about the normal),
    parallel and skew edges, vertices, touching at a face, an edge and a vertex, an edge resting on a face, coincident, contained
    (link against base), far -- against closed forms at ATOL; then Engine.step on hex, quad and lane against oracle.step on the
    fp64 pairs through the accuracy gate, every robot, every row meant to be in range moving the oracle's qdd by more than MATTERS.
    Measured on an MI355X: worst 0.13 of ATOL against the closed forms, 0.20 against the restatement."""
    torch = torch_mod
    import oracle as O
    s = HS.twin(swap)
    fa = s["frames"][0]
    T64 = O.forward_kinematics(s["desc"], s["q"], "f64")[:, fa]
    assert np.array_equal(O.forward_kinematics(s["desc"], s["q"], "f32")[:, fa].astype(np.float64), T64) and np.array_equal(T64[:, :3, 3], s["pA"])
    eng = _engine(s["desc"])
    eng.set_self_collision_hulls(s["pairs"], s["hulls"])
    assert eng.self_counts == [5, 1] and eng.has_self_hulls
    q, qd, goal = (torch.from_numpy(s[k]).cuda() for k in ("q", "qd", "goal"))
    got = [t.cpu().numpy() for t in eng.self_pairs(q)]
    worst = dict(closed=0.0, restatement=0.0)
    _check_twin(got, s, swap, worst)
    assert {r["kind"] for r in s["rows"]} == {"unique", "set", "tie"} and len(set(s["own"])) == 5
    # the step: reference pairs = the closed forms / the restatement, a named row's pair the stage's own (any member is right)
    rpl, rpo, rdd, _, _ = HP.self_hull_pairs_np(s["desc"], s["hulls"], s["pairs"], s["q"])
    for k, row in enumerate(s["rows"]):
        j = s["own"][k]
        if row["kind"] == "unique":
            rpl[k, j], rpo[k, j], rdd[k, j] = _self_expected(row, s["pA"][k], swap)
        else:
            rpl[k, j], rpo[k, j], rdd[k, j] = got[0][k, j], got[1][k, j], got[2][k, j]
    live = np.array([r["sep"] != 0 for r in s["rows"]])     # (touching: distance 0 is the leaves' pole, the oracle answers NaN)
    names = [r["name"] for r in s["rows"] if r["sep"] != 0]
    f32 = lambda a: np.ascontiguousarray(a[live], np.float32)   # noqa: E731
    kw = dict(p_link=f32(rpl), p_obs=f32(rpo), dist=f32(rdd), pair_counts=[5, 1])
    args = (s["desc"], s["q"][live], s["qd"][live], s["goal"][live])
    ref = O.step(*args, **kw)
    # each row's own pair taken 100 m apart instead: the rows meant to be in range must notice
    apl, apo, add = rpl.copy(), rpo.copy(), rdd.copy()
    for k, j in enumerate(s["own"]):
        add[k, j] = 100.0
        if not swap:
            apo[k, j] = apl[k, j] + np.array([100.0, 0.0, 0.0])
    away = O.step(*args, p_link=f32(apl), p_obs=f32(apo), dist=f32(add), pair_counts=[5, 1])["qdd64"]
    moved = np.abs(ref["qdd64"] - away).max(axis=1)
    weak = [n for n, m in zip(names, moved) if n not in SELF_OUT_OF_RANGE and not m > LS.MATTERS]
    assert not weak, f"rows meant to be in range that do not matter: {weak}"
    spread = O.fp32_resolution(*args, **kw)
    for kernel in ("hex", "quad", "lane"):
        e2 = _engine(s["desc"], kernel)
        e2.set_self_collision_hulls(s["pairs"], s["hulls"])
        qdd = e2.step(q, qd, goal).cpu().numpy()[live]
        assert KERNEL_NAME[kernel] in e2.last_kernel(), (kernel, e2.last_kernel())
        verdict = O.accuracy_gate(qdd, {k: ref[k] for k in ("qdd64", "M", "f")}, spread=spread)
        assert np.isfinite(qdd).all() and verdict["ok"].all(), (kernel, [n for n, ok in zip(names, verdict["ok"]) if not ok])
    print(f"hull self pairs catalogue swap={swap}: {len(s['rows'])} rows, worst / ATOL: closed forms {worst['closed']:.3f}, restatement {worst['restatement']:.3f}")


def test_self_pairs_with_halved_waves(torch_mod):
    """The self-hull stage parks 12 floats per frame slot and robot in LDS; beyond 21 slots 64 robots no longer fit 64 KiB and the
    launch halves its robots per wave.  A robot whose pairs name 23 frames, fleets of 31, 32, 33 and 65 robots (a partial block, a
    full one, one robot in a second block, a third block): EVERY pair against the restatement at ATOL -- the gap, and both points
    wherever the answer is determined: always where the hulls are apart (generic poses), and under the face rule where n* wins by
    more than 1e-3 (HP.face_margin, decided from the restatement alone, as tests/test_gpu_self_hulls.py does).  Measured on an
    MI355X: 78 determined face-rule pairs of 80 compared, worst 0.012 of ATOL."""
    torch = torch_mod
    import oracle as O
    m = HS.many_frames()
    fa = m["desc"].leaves[2].frame
    slots = len({f for _, f in m["pairs"] if f >= 0} | {fa})
    assert slots == m["slots"] == 23 and 4 * 12 * slots * 64 > 64 * 1024 >= 4 * 12 * slots * 32      # the halved path: 32 robots per wave
    eng = _engine(m["desc"])
    eng.set_self_collision_hulls(m["pairs"], m["hulls"])
    q = np.random.default_rng(29).uniform(-0.6, 0.6, (65, 4)).astype(np.float32)
    rpl, rpo, rdd, gap, face = HP.self_hull_pairs_np(m["desc"], m["hulls"], m["pairs"], q)
    T = O.forward_kinematics(m["desc"], q, "f64")
    small = HP.Hull(*HS.HULLS["small"])
    det = ~face
    for r_, j in np.argwhere(face):
        b = m["pairs"][j][1]
        TA, TB = T[r_, fa], (np.eye(4) if b < 0 else T[r_, b])
        det[r_, j] = HP.face_margin(small, small, TA[:3, :3].T @ TB[:3, :3], TA[:3, :3].T @ (TB[:3, 3] - TA[:3, 3])) > 1e-3
    n_face = int((face & det).sum())
    assert n_face >= 40 and (face & det)[:31].sum() >= 10 and (~face).sum() > 1000, (n_face, int(face.sum()))
    worst = 0.0
    for R in (31, 32, 33, 65):
        pl, po, dd = (t.cpu().numpy().astype(np.float64) for t in eng.self_pairs(torch.from_numpy(q[:R])))
        assert np.isfinite(pl).all() and np.isfinite(po).all() and np.isfinite(dd).all()
        e = np.abs(dd - rdd[:R]).max()
        assert e <= ATOL, (R, e)
        d = det[:R]
        e_pts = max(np.abs(pl - rpl[:R]).max(-1)[d].max(), np.abs(po - rpo[:R]).max(-1)[d].max())
        assert e_pts <= ATOL, (R, e_pts, np.argwhere((np.abs(pl - rpl[:R]).max(-1) > ATOL) & d)[:4])
        assert np.abs(np.linalg.norm(pl - po, axis=-1) - rdd[:R]).max() <= ATOL
        worst = max(worst, e / ATOL, e_pts / ATOL)
    print(f"hull self pairs, 23 frame slots (32 robots per wave): {n_face} determined face-rule pairs of {int(face.sum())}, worst / ATOL {worst:.3f}")


def test_self_pairs_non_finite_q(torch_mod):
    """Hull self pairs of a fleet of 33 with q poisoned in rows 0, 16 and 32 -- in a joint of the OTHER branch than the pair's
    frames for (0, base) and (1, base) --: every self pair of those robots is NaN, the others keep the clean fleet's bits; the
    step answers NaN on every joint with RMP2_STATUS_NONFINITE for them and the clean bits for the rest."""
    torch = torch_mod
    from riemannian_motion_policies_amd import descriptor as D
    s = HS.twin(False)
    eng = _engine(s["desc"])
    eng.set_self_collision_hulls(s["pairs"], s["hulls"])
    idx = np.arange(33) % len(s["q"])
    q0, qd, goal = s["q"][idx].copy(), s["qd"][idx].copy(), s["goal"][idx].copy()
    live = np.array([s["rows"][i]["sep"] != 0 for i in idx])
    q = q0.copy()
    bad = np.array([0, 16, 32])
    q[0, 5], q[16, 0], q[32, 4] = np.nan, np.inf, -np.inf
    clean = [t.cpu().numpy() for t in eng.self_pairs(torch.from_numpy(q0))]
    got = [t.cpu().numpy() for t in eng.self_pairs(torch.from_numpy(q))]
    ok = np.setdiff1d(np.arange(33), bad)
    for c, g in zip(clean, got):
        assert np.isfinite(c).all() and np.isnan(g[bad]).all(), np.argwhere(~np.isnan(g[bad]))[:4]
        assert _same_bits(c[ok], g[ok])

    def step(qq):
        st = torch.zeros(33, dtype=torch.int32, device="cuda")
        out = eng.step(torch.from_numpy(qq).cuda(), torch.from_numpy(qd).cuda(), torch.from_numpy(goal).cuda(), status=st)
        torch.cuda.synchronize()
        return out.cpu().numpy(), st.cpu().numpy()

    a0, st0 = step(q0)
    a, st = step(q)
    assert np.isnan(a[bad]).all() and ((st[bad] & D.STATUS_NONFINITE) != 0).all()
    assert _same_bits(a[ok], a0[ok]) and np.array_equal(st[ok], st0[ok]) and np.isfinite(a0[live]).all()

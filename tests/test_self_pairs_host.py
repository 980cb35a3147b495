"""The capsule self-pair stage on general robots, host side (no GPU): the reference of tests/self_pair_reference.py against a dense
sampling of the segments, what the scenes of tests/self_pair_scene.py cover and claim, the host helpers of urdf.py on random
trees, and the fp32 ENVELOPE the bound of tests/test_gpu_self_pairs_general.py is set against.

Envelope (the fp32 restatement -- the reference's closed form in fp32 arithmetic on the oracle's fp32 frames -- against fp64, on
the very fleets the GPU tests use; bound = 1e-5 max(1, extent), extent = the robot's largest capsule end-point coordinate):
worst ratio to the bound 0.028 on the distance and 0.103 on the points (tree `twelve`), no (robot, pair) row beyond the points
bound.  0.103 <= 0.25, so the project's stage bound scaled by the extent stands (the rule K = 4 x envelope is not needed).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import link_pair_scene as LS  # noqa: E402
import self_pair_reference as SR  # noqa: E402
import self_pair_scene as S  # noqa: E402
from test_link_pairs_host import driver, run_driver  # noqa: E402,F401

ATOL = 1e-5               # the project's stage bound (tests/test_gpu_self_collision.py), scaled by max(1, extent) on the trees
ENVELOPE_SHARE = 0.25     # the envelope may use at most this share of the bound, else the bound is set by K = 4 x envelope
EXEMPT_CAP = 0.05         # (robot, pair) rows per tree whose fp32 restatement itself misses the points bound
NEEDED = {"slots_0", "slots_1", "slots_2", "prismatic_above_leaf", "movable_joint_unactuated", "two_root_joints", "pruned_b",
          "empty_first", "empty_middle", "empty_last", "dof_9", "dof_12", "dof_16", "thirty_frames", "mixed_kinds", "two_leaves_one_frame"}


def _gantry_world_rows():
    """(name, A, B, C, D) of every pair of every row of the two-arm gantry, fp64."""
    rows = []
    for shape in S.B_SHAPES:
        s = S.two_arm_gantry(shape)
        g = SR.self_pair_geometry(s["desc"], s["pairs"], s["caps"], s["q"])
        for r, name in enumerate(s["names"]):
            for j in range(2):
                rows.append((f"{name}/{j}", g["A"][r, j], g["B"][r, j], g["C"][r, j], g["D"][r, j]))
    return rows


def test_reference_against_dense_sampling():
    """The closed form of the reference against something that does not share its algebra: 513 x 513 samples of both segments.
    sampled - slack <= reference <= sampled, slack = the grid's Lipschitz bound (half a step on either segment)."""
    rng = np.random.default_rng(2718)
    cases = []
    for k in range(300):
        A, B, C, D = rng.uniform(-1, 1, (4, 3))
        if k % 5 == 1:
            D = C + (B - A) * rng.uniform(0.2, 2.0)            # parallel
        if k % 5 == 2:
            B = A.copy()                                       # zero length
        if k % 5 == 3:
            C = A + rng.uniform(0, 1) * (B - A)                # touching / crossing
        cases.append((f"random {k}", A, B, C, D))
    cases += _gantry_world_rows()
    worst = 0.0
    for name, A, B, C, D in cases:
        X, Y = SR._seg_seg(A[None], B[None], C[None], D[None])
        d = float(np.linalg.norm(X - Y))
        smin, slack = SR.sampled_min(A, B, C, D, 513)
        assert d <= smin + 1e-12, f"{name}: closed form {d} above the sampled minimum {smin}"
        assert d >= smin - slack - 1e-12, f"{name}: closed form {d} below the sampled minimum {smin} by more than {slack}"
        worst = max(worst, smin - d)
    print(f"dense sampling: {len(cases)} pairs, reference below the sampled minimum by at most {worst:.2e}")


def test_reference_layout_and_dtype():
    """Any pair order gives the stage's layout (leaves in ordinal order, a leaf's pairs in the order given); dtype = float32 stays
    in fp32 from the oracle's fp32 frames on; an attached-point leaf's fields are the distance leaf's, re-expressed."""
    tr = S.tree("mixed")
    q = tr["q"][:5]
    base = SR.self_pairs_np(tr["desc"], tr["pairs"], tr["caps"], q)
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(tr["pairs"]))
    shuffled = [tr["pairs"][i] for i in perm]
    lay = SR.layout(shuffled)
    assert [shuffled[k][0] for k in lay] == sorted(o for o, _ in tr["pairs"])
    got = SR.self_pairs_np(tr["desc"], shuffled, tr["caps"], q)
    # the same multiset of rows per leaf, in the order the shuffled list gives them
    want_cols = [tr["pairs"].index(shuffled[k]) for k in lay]
    for a, b in zip(got, base):
        assert np.array_equal(a, b[:, want_cols])
    f32 = SR.self_pairs_np(tr["desc"], tr["pairs"], tr["caps"], q, np.float32)
    assert all(a.dtype == np.float32 for a in f32)
    assert np.abs(f32[2] - base[2]).max() < 1e-5
    # point leaves: p_link back in the base frame lies on A's surface, p_obs is a unit vector, dist = |gap|.  (R^T is not R's inverse
    # to better than the fp32 rounding of the URDF's constant rotations, ~6e-8 per joint: hence 1e-6 and not 1e-12)
    g = SR.self_pair_geometry(tr["desc"], tr["pairs"], tr["caps"], q)
    pt = g["point"]
    assert pt.any() and (~pt).any()
    for j in np.nonzero(pt)[0]:
        Tf = g["T"][:, g["frame"][j]]
        world = np.einsum("rij,rj->ri", Tf[:, :3, :3], base[0][:, j]) + Tf[:, :3, 3]
        assert np.abs(SR.point_segment_distance(world, g["A"][:, j], g["B"][:, j]) - g["ra"][j]).max() < 1e-6
        assert np.abs(np.linalg.norm(base[1][:, j], axis=-1) - 1).max() < 1e-12
        other = world - base[2][:, j, None] * base[1][:, j]
        assert np.abs(SR.point_segment_distance(other, g["C"][:, j], g["D"][:, j]) - g["rb"][j]).max() < 1e-6


def test_trees_cover_what_they_must():
    have = set()
    for name in S.TREES:
        tr = S.tree(name)
        got = S.conditions(tr)
        assert set(S.TREES[name]["want"]) <= got, name
        have |= got
        t = tr["table"]
        assert t.depth_first_schedule()[3] <= 2 and t.n_frames <= 32 and t.n_dof <= 16
        assert 3 <= len(set(tr["leaf_frames"])) <= 6, name
    assert 6 <= len(S.TREES) <= 8
    assert NEEDED <= have, sorted(NEEDED - have)
    # one robot carries all three empty positions: its counts are [0, ., ., 0, ., 0]
    assert [c == 0 for c in S.tree("gaps")["counts"]] == [True, False, False, True, False, True]
    assert S.tree("mixed")["kinds"] == list("dpdpd") and S.tree("twin")["leaf_frames"][2] == S.tree("twin")["leaf_frames"][1]


@pytest.mark.parametrize("name", list(S.TREES))
def test_urdf_helpers_on_trees(name):
    """urdf.self_collision_pairs / self_collision_capsules / base_link_name on a tree with several root joints, links without a
    shape and leaves sharing a frame."""
    from riemannian_motion_policies_amd import urdf as U
    tr = S.tree(name)
    t, pairs, caps, frames = tr["table"], tr["pairs"], tr["caps"], tr["leaf_frames"]
    F = t.n_frames

    def hops(a, b):          # parent hops from a up to b (the base is -1), None if b is no ancestor
        k, e = 0, a
        while e != b:
            if e == -1:
                return None
            e, k = int(t.parent[e]), k + 1
        return k
    for o, b in pairs:
        a = frames[o]
        assert t.has_collision[a] and (b == -1 or t.has_collision[b]) and a != b
        for up in (hops(a, b), hops(b, a) if b >= 0 else None):
            assert up is None or up > 3, (name, o, b)
    # grouping and order: by leaf ordinal, B ascending from -1; and nothing is missing
    assert pairs == sorted(pairs)
    want = [(o, b) for o, a in enumerate(frames) if t.has_collision[a] for b in range(-1, F)
            if (b == -1 or t.has_collision[b]) and b != a and all(up is None or up > 3 for up in (hops(a, b), hops(b, a) if b >= 0 else None))]
    assert pairs == want
    assert tr["counts"] == [sum(1 for o, _ in pairs if o == i) for i in range(len(frames))]
    # capsules
    assert caps.shape == (F + 1, 8) and caps.dtype == np.float32
    assert (~t.has_collision).sum() >= 2
    for f in range(F):
        if not t.has_collision[f]:
            assert not caps[f].any()
            continue
        kids = [c for c in range(F) if t.parent[c] == f]
        end = t.T_const[kids[0], :3, 3] if kids else np.zeros(3, np.float32)
        assert np.array_equal(caps[f], np.float32([0, 0, 0, S.RADIUS, *end, 0])), (name, f)
    assert U.base_link_name(tr["path"], t) == "base"
    assert np.array_equal(caps[F], np.float32([0, 0, 0, S.RADIUS, 0, 0, 0, 0]))      # (the base has no shape: the fallback at its origin)


@pytest.mark.parametrize("name", list(S.TREES))
def test_tree_fleets_matter_and_envelope(name):
    """Per tree: at least a quarter of the fleet has a self pair that moves the oracle's fp64 qdd by more than MATTERS (else the
    step test is vacuous); no state sits on the clear / contact threshold; the fp32 restatement uses at most a quarter of the
    stage's bound and misses the points bound on at most 5 % of the rows; and on robots clear of contact it is within half of the
    step's plain bound."""
    import oracle as O
    tr = S.tree(name)
    moved = np.abs(S.reference_step(tr)["qdd64"] - S.reference_step(tr, away=True)["qdd64"]).max(axis=1)
    assert (moved > S.MATTERS).mean() >= 0.25, f"{name}: only {(moved > S.MATTERS).mean():.0%} of the fleet feels its self pairs"
    g64 = SR.self_pair_geometry(tr["desc"], tr["pairs"], tr["caps"], tr["q"])
    pl, po, dd, gap = SR.self_pairs_np(tr["desc"], tr["pairs"], tr["caps"], tr["q"], geometry=g64)
    near = gap.min(axis=1)
    assert not ((near >= S.CLEAR) & (near < S.CLEAR_MARGIN)).any()
    pl32, po32, dd32, _ = SR.self_pairs_np(tr["desc"], tr["pairs"], tr["caps"], tr["q"], np.float32)
    bound = ATOL * max(1.0, S.extent(tr, g64))
    e_dist = np.abs(dd32 - dd).max() / bound
    e_pts = np.maximum(np.abs(pl32 - pl).max(axis=-1), np.abs(po32 - po).max(axis=-1)) / bound
    exempt = e_pts > 1.0
    args = (tr["desc"], tr["q"], tr["qd"], tr["goal"])
    ref = O.step(*args, **S.explicit_kwargs(tr, pl, po, dd))
    got = O.step(*args, **S.explicit_kwargs(tr, pl32, po32, dd32))["qdd"]
    clear = near >= S.CLEAR
    e_step = (np.abs(got - ref["qdd64"]).max(axis=1) / (ATOL * np.maximum(1.0, np.abs(ref["qdd64"]).max(axis=1))))[clear].max(initial=0.0)
    print(f"envelope {name}: extent {S.extent(tr, g64):.2f} m, bound {bound:.2e}; fp32 restatement / bound: distance {e_dist:.3f}, "
          f"points {e_pts[~exempt].max():.3f}, rows beyond the points bound {exempt.mean():.2%}; feels its self pairs "
          f"{(moved > S.MATTERS).mean():.0%}; clear robots {clear.sum()} of {len(clear)}, their step restatement {e_step:.3f} of 1e-5")
    assert e_dist <= ENVELOPE_SHARE and e_pts[~exempt].max() <= ENVELOPE_SHARE
    assert exempt.mean() <= EXEMPT_CAP
    assert e_step <= 0.5


def test_fleets_are_well_posed():
    """The surface points are X - r n with n = (X - Y) / |X - Y|: the axis points carry about 4 eps32 of the extent each, so n turns
    by 4 eps32 extent / |X - Y| and the points move by r times that.  Kept below a quarter of the bound 1e-5 extent, that asks
    |X - Y| >= 4 * 6e-8 * r / 0.25e-5 = 0.096 r = 4.8 mm at r = 0.05: no (robot, pair) of any fleet has its axes nearer than
    MIN_AXIS = 1 cm (exactly intersecting and touching axes are the business of the exact scene, not of random trees)."""
    assert S.MIN_AXIS >= 2 * 0.096 * S.RADIUS
    cases = [(n, S.tree(n), S.tree(n)["pairs"]) for n in S.TREES]
    cases += [(n, S.tree(S.LIST_TREE), lst) for n, lst in S.list_shapes().items()]
    cases += [(f"lds {e}", S.lds_boundary(e), S.lds_boundary(e)["pairs"]) for e in (0, 1)]
    for name, s, pairs in cases:
        g = SR.self_pair_geometry(s["desc"], pairs, s["caps"], s["q"])
        assert np.linalg.norm(g["X"] - g["Y"], axis=-1).min() >= S.MIN_AXIS, name


def test_list_shapes_are_what_they_claim():
    tr = S.tree(S.LIST_TREE)
    frames, F = tr["leaf_frames"], tr["table"].n_frames
    shapes = S.list_shapes()
    for name, lst in shapes.items():
        assert all(0 <= o < len(frames) and -1 <= b < F and b != frames[o] for o, b in lst), name
    assert sorted(shapes["shuffled"]) == sorted(shapes["sorted"]) and shapes["shuffled"] != shapes["sorted"]
    assert [o for o, _ in shapes["shuffled"]] != sorted(o for o, _ in shapes["shuffled"])          # shuffled ACROSS leaves
    assert len(shapes["repeated"]) == len(set(shapes["repeated"])) + 1
    assert len({b for _, b in shapes["shared_b"]}) == 1 and len(shapes["shared_b"]) == len(frames)
    assert shapes["base_last"][-1][1] == -1 and all(b >= 0 for _, b in shapes["base_last"][:-1])     # the base gets the LAST B slot
    assert shapes["base_only"] == [(1, -1)]
    for P in (1, 63, 64, 65, 128, 256):
        assert len(shapes[f"total_{P}"]) == P
    assert len(shapes["too_many"]) == 257
    assert 0 in SR.counts_of(shapes["total_1"], len(frames))


def test_lds_boundary_is_on_the_boundary():
    for extra, records in ((0, 256), (1, 258)):
        b = S.lds_boundary(extra)
        n_dist = 0                                        # attached-point leaves only
        assert 2 * n_dist + 5 * len(b["counts"]) + 2 * len({x for _, x in b["pairs"]}) == records
        assert len(b["pairs"]) <= 256 and b["desc"].n_leaves <= 48 and b["table"].n_dof == 16
    assert 16 * 16 * 256 == 64 * 1024


@pytest.mark.parametrize("shape", list(S.B_SHAPES))
def test_two_arm_gantry_is_exact(shape):
    """The degenerate scene is what it claims, in fp32: exact kinematics; |X - Y| == 0 on the crossing rows and den == 0 on the
    parallel and collinear rows; arm B's frame is NOT in the step's pruned program; the moving B and the base-row B are the same
    world capsule bit for bit; every row meant to be in range moves the oracle's fp64 qdd by more than MATTERS."""
    import oracle as O
    s = S.two_arm_gantry(shape)
    t = s["table"]
    T32, T64 = O.forward_kinematics(s["desc"], s["q"], "f32"), O.forward_kinematics(s["desc"], s["q"], "f64")
    assert np.array_equal(T32.astype(np.float64), T64)
    assert (t.parent < 0).sum() == 2 and t.parent[t.frame_index("kx")] == -1
    fk_frames = [s["desc"].leaves[i].frame for i in range(s["desc"].n_leaves) if s["desc"].leaves[i].frame >= 0]
    assert s["b_frame"] not in S.kept_frames(t, fk_frames)
    g = SR.self_pair_geometry(s["desc"], s["pairs"], s["caps"], s["q"], np.float32)
    assert g["X"].dtype == np.float32
    nn = np.sqrt(((g["X"] - g["Y"]) ** 2).sum(-1))
    d1, d2 = g["B"] - g["A"], g["D"] - g["C"]
    den = (d1 * d1).sum(-1) * (d2 * d2).sum(-1) - (d1 * d2).sum(-1) ** 2
    assert den.dtype == np.float32
    moved = np.abs(S.reference_step(s)["qdd64"] - S.reference_step(s, away=True)["qdd64"]).max(axis=1)
    for r, (name, cls) in enumerate(zip(s["names"], s["classes"])):
        if cls.startswith("crossing"):
            assert nn[r, 0] == 0 or (name == "both_zero" and nn[r, 1] == 0), name
        if name == "both_zero":
            assert nn[r, 1] == 0 and not d1[r, 1].any() and not d2[r, 1].any()       # the tip against the point B: both of zero length
        if name in ("parallel_beside", "collinear_apart", "collinear_overlap", "touch_end"):
            assert den[r, 0] == 0 and d1[r, 0].any() and d2[r, 0].any(), name
        if cls == "unique":
            assert nn[r, 0] > 0
        assert (moved[r] > S.MATTERS) == (cls != "far"), (name, moved[r])
    # the base variant: the same world capsule, bit for bit
    for b, r in zip(S.two_arm_gantry(shape, base=True), range(len(s["names"]))):
        gb = SR.self_pair_geometry(b["desc"], b["pairs"], b["caps"], b["q"], np.float32)
        for k in "ABCD":
            assert np.array_equal(gb[k][0], g[k][r]), (b["names"], k)
        assert np.array_equal(gb["rb"], g["rb"])


def test_degenerate_catalogue_through_the_device_form(driver, tmp_path):  # noqa: F811
    """rmp2_device.h link_pair_fields -- the routine the stage calls per self pair -- on the CPU (tests/link_pairs_driver.cpp) for
    the world segments of every row of the two-arm gantry, against the reference: distance everywhere, points where they are
    unique, the fixed normal where the axes intersect, membership where the nearest pair is a set."""
    rows, meta = [], []
    for shape in S.B_SHAPES:
        s = S.two_arm_gantry(shape)
        g = SR.self_pair_geometry(s["desc"], s["pairs"], s["caps"], s["q"])
        pl, po, dd, gap = SR.self_pairs_np(s["desc"], s["pairs"], s["caps"], s["q"], geometry=g)
        for r, (name, cls) in enumerate(zip(s["names"], s["classes"])):
            for j in range(2):
                rows.append(np.concatenate([g["A"][r, j], g["B"][r, j], [g["ra"][j]], g["C"][r, j], [g["rb"][j]], g["D"][r, j], [0.0]]))
                meta.append((name, j, cls, pl[r, j], po[r, j], dd[r, j], gap[r, j], g))
    a = np.asarray(rows, np.float32)
    out = run_driver(driver, tmp_path, a[:, 0:3], a[:, 3:6], a[:, 6], a[:, 7:11], a[:, 11:15])
    assert np.isfinite(out["all"]).all()
    n_cross = 0
    for k, (name, j, cls, pl, po, dd, gap, g) in enumerate(meta):
        f_link, f_n, f_d = (out[key][k].astype(np.float64) for key in ("f_link", "f_normal", "f_dist"))
        assert abs(f_d - dd) <= LS_POINTS, (name, j)
        axis = gap + a[k, 6] + a[k, 10]
        if abs(axis) == 0:                     # intersecting axes: normal -z exactly, distance the sum of the radii
            n_cross += 1
            assert np.array_equal(out["f_normal"][k], np.float32([0, 0, -1])) and out["f_dist"][k] == a[k, 6] + a[k, 10], (name, j)
        f_obs = f_link - f_d * f_n
        if j == 0 and cls in ("set", "crossing_set"):
            assert abs(SR.point_segment_distance(f_link, a[k, 0:3], a[k, 3:6]) - a[k, 6]) <= LS_POINTS, name
            assert abs(SR.point_segment_distance(f_obs, a[k, 7:10], a[k, 11:14]) - a[k, 10]) <= LS_POINTS, name
        else:
            assert np.abs(f_link - pl).max() <= LS_POINTS and np.abs(f_obs - po).max() <= LS_POINTS, (name, j)
    assert n_cross >= 9


LS_POINTS = 2e-6          # tests/test_gpu_link_pair_degenerate.py POINTS
assert LS.LINK_R == 0.0625

"""The hull self-pair stage and the link-hull stage on general robots, host side (no GPU): what the scenes of
tests/hull_tree_scene.py are and cover, the fp32 walk's ENVELOPE the bound of tests/test_gpu_hull_trees.py is set against, which
point answers are determined, and a proof on the CPU that the scenes can see three faults of the stage's own walk.

Bound: the project's stage bound B = 1e-5 max(1, extent), extent = the largest |coordinate| of any placed hull vertex over the fleet
(1.5 .. 3.0 m).  Envelope: the restatement of tests/hull_pair_reference.py on the oracle's fp32 frames against the same on its fp64
frames -- the fp32 walk's own share -- is at most 0.054 B on the distance over the eight trees (tree `bush`) and the four raw
lists, under the 0.25 B asked.  At most 0.2 % of a tree's entries are not `determined` (cap 5 %); 24 entries of the eight trees and
48 of the halved list sit under the face rule with a margin above 1e-3; at most 3 robots of 67 per fleet overlap deeper than 1e-3.
Per tree: profiles/hull_trees.txt.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hull_pair_reference as HP  # noqa: E402
import hull_tree_scene as HT  # noqa: E402
import link_pair_scene as LS  # noqa: E402
import self_pair_scene as S  # noqa: E402

UNDETERMINED_CAP = 0.05
NEEDED = {"slots_0", "slots_1", "slots_2", "movable_joint_unactuated", "two_root_joints", "pruned_b", "thirty_frames", "dof_12", "dof_16",
          "two_leaves_one_frame", "mixed_kinds"}
SENSITIVITY_ROBOTS = 4
FAULTS = ("ut_signs", "product_order", "wrong_slot")


def _tilted_revolute(t, actuated=True):
    """Revolute joints whose axis has |x| or |y| above 0.3 (actuated: those in the joint order, which turn)."""
    from riemannian_motion_policies_amd import urdf as U
    return [f for f in range(t.n_frames) if t.joint_type[f] == U.JOINT_REVOLUTE and (t.q_index[f] >= 0 or not actuated)
            and np.abs(t.axis[f][:2]).max() > 0.3]


@pytest.mark.parametrize("name", list(S.TREES))
def test_hulls_are_what_they_claim(name):
    """6 to 24 points per link on the 2^-10 grid within h of the link's centre, exact in fp32; an entry per frame and the base, empty
    exactly where the link has no collision shape; the leaves' entries are urdf.link_hulls bit for bit; the default pair list is
    urdf.self_collision_pairs and names no empty entry."""
    from riemannian_motion_policies_amd import urdf as U
    sc = HT.scene(name)
    t, hulls, F = sc["table"], sc["hulls"], sc["table"].n_frames
    assert len(hulls) == F + 1 and len(hulls.hull(F)[0]) >= 4
    for f in range(F):
        V, P = hulls.hull(f)
        assert (len(V) == 0 and len(P) == 0) == (not t.has_collision[f]), f
    for link, pts in sc["meshes"].items():
        assert 6 <= len(pts) <= 24 and np.array_equal(pts * 1024, np.round(pts * 1024)) and np.ptp(pts, axis=0).max() <= 2 * sc["h"] + HT.GRID
    for e in range(F + 1):
        V = hulls.hull(e)[0]
        assert V.dtype == np.float32 and np.array_equal(V.astype(np.float64) * 1024, np.round(V.astype(np.float64) * 1024))
    with_hull = [f for f in sc["leaf_frames"] if t.has_collision[f]]
    lh = U.link_hulls(t, [t.frame_names[f] for f in with_hull], sc["meshes"])
    sub = hulls.subset(with_hull)
    for a, b in zip((sub.vert_offset, sub.verts, sub.face_offset, sub.planes), (lh.vert_offset, lh.verts, lh.face_offset, lh.planes)):
        assert a.tobytes() == b.tobytes()
    assert sc["pairs"] == U.self_collision_pairs(t, sc["leaf_frames"]) and 0 < len(sc["pairs"]) <= 256
    assert sc["counts"] == S.tree(name)["counts"]
    # the tree's own states wherever no round redrew them
    redrawn = sorted({i for rnd in HT.HULLS[name]["redraw"] for i in rnd})
    kept = np.setdiff1d(np.arange(HT.FLEET), redrawn)
    assert np.array_equal(sc["q"][kept], S.tree(name)["q"][kept]) and sc["q"].shape == (HT.FLEET, t.n_dof)
    # three or more revolute joints off the z axis, two or more of them in the joint order (tree `fork` leaves three of its five
    # out); test_planted_faults_move_the_distances shows that each tree's states make them count
    assert len(_tilted_revolute(t, actuated=False)) >= 3 and len(_tilted_revolute(t)) >= 2, name


def test_trees_cover_what_they_must():
    have = set()
    kinds = set()
    for name in S.TREES:
        have |= S.conditions(HT.scene(name))
        kinds |= set(HT.scene(name)["kinds"])
    assert NEEDED <= have, sorted(NEEDED - have)
    assert "p" in kinds


@pytest.mark.parametrize("name", list(S.TREES))
def test_scene_conditions_envelope_and_determined(name):
    """Per tree, from the fp64 restatement alone: at least half of the (robot, pair) entries are out of the leaves' reach; at least
    10 % of the robots own a pair that moves oracle.step's qdd by more than MATTERS; at most 5 % of the robots overlap deeper than
    1e-3 (the step test's rule); the fp32 walk's share of the bound on the distance is at most 0.25 on EVERY entry; at most 5 % of
    the entries are not determined."""
    sc = HT.scene(name)
    ref = HT.reference(sc)
    gap, face = ref["ref64"][3], ref["ref64"][4]
    assert gap.shape == (HT.FLEET, len(sc["pairs"]))
    out = float((gap >= HT.OUT_OF_REACH).mean())
    moved = np.abs(HT.reference_step(sc, ref)["qdd64"] - HT.reference_step(sc, ref, away=True)["qdd64"]).max(axis=1)
    felt = float((moved > LS.MATTERS).mean())
    deep = HT.deep_robots(ref)
    env = HT.envelope(ref)
    undet = float(1.0 - ref["det"].mean())
    n_face = int((face & (ref["margin"] > HT.DEEP)).sum())
    print(f"hull tree {name}: F = {sc['table'].n_frames}, dofs = {sc['table'].n_dof}, P = {len(sc['pairs'])}, counts {sc['counts']}, "
          f"extent {ref['extent']:.2f} m, bound {ref['bound']:.2e}; out of reach {out:.0%} of the entries; feels its pairs {felt:.0%} of the "
          f"robots; overlapping entries {int(face.sum())}, with margin > 1e-3 {n_face}; robots deeper than 1e-3 {int(deep.sum())}; "
          f"envelope / bound {env.max():.3f}; not determined {undet:.2%}; redrawn {sum(len(r) for r in HT.HULLS[name]['redraw'])}")
    assert out >= 0.5, f"{name}: only {out:.0%} of the entries are out of reach"
    assert felt >= 0.10, f"{name}: only {felt:.0%} of the robots feel their pairs"
    assert deep.mean() <= 0.05 and deep.sum() <= HT.MAX_DEEP, f"{name}: {deep.sum()} robots in deep overlap"
    assert env.max() <= HT.ENVELOPE_SHARE, f"{name}: envelope at {env.max():.3f} of the bound"
    assert undet <= UNDETERMINED_CAP, f"{name}: {undet:.1%} of the entries are not determined"


def test_face_rule_entries_over_the_catalogue():
    n = sum(int((HT.reference(HT.scene(name))["ref64"][4] & (HT.reference(HT.scene(name))["margin"] > HT.DEEP)).sum()) for name in S.TREES)
    assert n >= 20, n


@pytest.mark.parametrize("name", ["twin", "chain9"])
def test_recorded_redraws_are_the_rule(name):
    """HULLS[name]["redraw"] is what the rule of hull_tree_scene.settle gives from the tree's own states (a one-round and a
    two-round tree; the conditions themselves are asserted on every tree above)."""
    assert HT.settle(name) == HT.HULLS[name]["redraw"]


def test_list_scenes_are_what_they_claim():
    from riemannian_motion_policies_amd import urdf as U
    # (a) some leaves have no self pair, and no pair joins two hull-bearing leaves
    a = HT.list_scene("no_leaf_pairs")
    assert a["counts"][0] == 0 and 0 in a["counts"][1:-1] and any(a["counts"])
    assert not any(b in a["leaf_frames"] for _, b in a["pairs"])
    assert all(a["table"].has_collision[f] for f in a["leaf_frames"]) and set(a["kinds"]) == {"d"}     # (takes a table: K > 0)
    # (b) the halved launch: 22 or more frames named on the 2-slot, 16-dof tree
    b = HT.list_scene("halved")
    slots = HT.lds_slots(b)
    assert slots >= 22 and 4 * 12 * slots * 64 > 65536 >= 4 * 12 * slots * 32
    assert b["table"].depth_first_schedule()[3] == 2 and b["table"].n_dof == 16 and len(_tilted_revolute(b["table"])) >= 3
    assert all(bb != b["leaf_frames"][o] for o, bb in b["pairs"]) and any(bb < 0 for _, bb in b["pairs"])
    # (c) two pair leaves on one frame, both with pairs, the same B's in another order
    c = HT.list_scene("twin_shared")
    assert c["leaf_frames"][1] == c["leaf_frames"][2] and c["counts"][1] == c["counts"][2] > 1
    one, two = [bb for o, bb in c["pairs"] if o == 1], [bb for o, bb in c["pairs"] if o == 2]
    assert one == two[::-1] and one != two
    # one hull at the cap
    d = HT.list_scene("cap")
    V, P = d["hulls"].hull(d["cap_entry"])
    assert len(V) == U.MAX_HULL_VERTICES == 512 and len(P) == 1020 <= U.MAX_HULL_FACES
    assert all(bb == d["cap_entry"] for _, bb in d["pairs"]) and len(d["q"]) == HT.CAP_ROBOTS
    for sc in (a, b, c, d):
        ref = HT.reference(sc)
        env, undet = HT.envelope(ref).max(), 1.0 - ref["det"].mean()
        print(f"hull list {sc['key'][1]}: P = {len(sc['pairs'])}, counts {sc['counts']}, frame slots {HT.lds_slots(sc)}; overlapping entries "
              f"{int(ref['ref64'][4].sum())}; envelope / bound {env:.3f}; not determined {undet:.2%}")
        assert env <= HT.ENVELOPE_SHARE and undet <= UNDETERMINED_CAP, sc["key"]


# ---- sensitivity: the stage's own walk, restated, with three planted faults ---------------------------------------------------
def _walk(t, q, fault=None):
    """rmp2_stages.h walk_frame_position over the unpruned depth-first program with its save / restore slots, in fp64: frames
    [R, F, 4, 4].  fault: "ut_signs" (the x and y components of the skew matrix negated), "product_order" (Tc Rv formed as Rv Tc),
    "wrong_slot" (slot 1 restored where slot 0 was saved)."""
    from riemannian_motion_policies_amd import urdf as U
    order, restore, save, _ = t.depth_first_schedule()
    R = len(q)
    T = np.zeros((R, t.n_frames, 4, 4))
    cur, saved = None, {}
    for k, f in enumerate(order):
        if restore[k] >= 0:
            cur = saved[1 if (fault == "wrong_slot" and restore[k] == 0 and 1 in saved) else restore[k]]
        elif restore[k] == -2:
            cur = np.broadcast_to(np.eye(4), (R, 4, 4))
        qv = q[:, t.q_index[f]].astype(np.float64) if t.q_index[f] >= 0 else np.zeros(R)
        Tc, ax = t.T_const[f].astype(np.float64), t.axis[f].astype(np.float64)
        loc = np.broadcast_to(Tc, (R, 4, 4)).copy()
        if t.joint_type[f] == U.JOINT_REVOLUTE:
            sx = -1.0 if fault == "ut_signs" else 1.0
            ut = np.array([[0, -ax[2], sx * ax[1]], [ax[2], 0, -sx * ax[0]], [-sx * ax[1], sx * ax[0], 0]])
            Rv = np.cos(qv)[:, None, None] * np.eye(3) + np.sin(qv)[:, None, None] * ut + (1 - np.cos(qv))[:, None, None] * np.outer(ax, ax)
            loc[:, :3, :3] = Rv @ Tc[:3, :3] if fault == "product_order" else Tc[:3, :3] @ Rv
        elif t.joint_type[f] == U.JOINT_PRISMATIC:
            loc[:, :3, 3] = Tc[:3, 3] + qv[:, None] * (Tc[:3, :3] @ ax)
        cur = cur @ loc
        if save[k] >= 0:
            saved[save[k]] = cur
        T[:, f] = cur
    return T


def test_walk_restatement_is_the_oracles():
    import oracle as O
    for name in S.TREES:
        sc = HT.scene(name)
        assert np.abs(_walk(sc["table"], sc["q"]) - O.forward_kinematics(sc["desc"], sc["q"], "f64")).max() <= 1e-12, name


def test_planted_faults_move_the_distances():
    """Each fault of the walk moves some distance by more than 10 B: the first two on EVERY tree (each has three or more revolute
    joints off the z axis), the third on the trees with two save slots.  On the Panda, whose revolute axes are all (0, 0, 1), the
    first fault changes no frame at all -- which is why the suite could not see it."""
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    moved = {f: {} for f in FAULTS}
    for name in S.TREES:
        sc = HT.scene(name)
        t, q = sc["table"], sc["q"][:SENSITIVITY_ROBOTS]
        bound = HT.bound_of(sc)[1]
        good = HP.self_hull_pairs_np(sc["desc"], sc["hulls"], sc["pairs"], q, T=_walk(t, q))[2]
        for fault in FAULTS:
            if fault == "wrong_slot" and t.depth_first_schedule()[3] < 2:
                continue
            Tf = _walk(t, q, fault)
            named = sorted({sc["leaf_frames"][o] for o, _ in sc["pairs"]} | {b for _, b in sc["pairs"] if b >= 0})
            if np.array_equal(Tf[:, named], _walk(t, q)[:, named]):
                moved[fault][name] = 0.0
                continue
            moved[fault][name] = float(np.abs(HP.self_hull_pairs_np(sc["desc"], sc["hulls"], sc["pairs"], q, T=Tf)[2] - good).max() / bound)
    print("planted faults, largest |dist - clean| / B per tree: " + "; ".join(f"{f}: " + ", ".join(f"{n} {v:.3g}" for n, v in m.items()) for f, m in moved.items()))
    for fault in ("ut_signs", "product_order"):
        assert set(moved[fault]) == set(S.TREES) and min(moved[fault].values()) > 10.0, (fault, moved[fault])
    assert moved["wrong_slot"] and max(moved["wrong_slot"].values()) > 10.0, moved["wrong_slot"]
    tp = U.panda_table()
    qp = Cf.sample_panda_states(np.random.default_rng(1), 16)["q"]
    assert np.array_equal(_walk(tp, qp, "ut_signs"), _walk(tp, qp))
    assert not np.array_equal(_walk(tp, qp, "product_order"), _walk(tp, qp))

"""Self contacts between the robot's own link capsules (include/rmp2.h rmp2_dynamics_step_contacts_self) on the host: the scenes
of tests/contact_self_scene.py meet their stated conditions; the fp32 envelope that the bounds are taken from; the self form of
the device routine of rmp2_contacts.h run on the CPU through tests/contacts_driver.cpp (also under the host sanitizers, as a
stand-alone program) against the fp64 reference of tests/contact_self_reference.py, and BIT FOR BIT against the capsules driver
where the contract promises it; pair indices, the tie between the four kinds, the header, the bindings and
urdf.contact_self_pairs.  No GPU.

The bounds are those of tests/test_contacts_host.py (stationarity, velocity, total constraint torque, linearised gap of the
device's own pairs after one substep; q / qd after STEP_SUBSTEPS), with the K's of these scenes by the same rule: K = 4 x the worst
ratio of the fp32 ENVELOPE against the fp64 reference over the catalogue, rounded up to one significant figure (MEASURED_SELF ->
K_SELF, fixed here from the CPU run before any GPU run; test_envelope_backs_the_bounds measures them again).  Robots held to the
bounds: the kept rule of DESIGN 4.12 (envelope uncapped and within K / 4)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contact_capsules_reference as QR
import contact_planes_reference as PR
import contact_self_reference as SR
import contact_self_scene as SS
import contacts_reference as CR
import test_contact_capsules_host as QH
import test_contact_planes_host as PH
import test_contacts_host as S
from test_contacts_host import D_ACT, DT, ROOT

MEASURED_SELF = dict(res=0.02935, vel=42.55, force=16.78, step=24.10, gap=0.06770)      # the envelope's worst ratios
K_SELF = dict(res=0.2, vel=200.0, force=70.0, step=100.0, gap=0.3)
MAX_SELF_FRAMES = 22
FLOATS = PH.FLOATS
SAN = PH.SAN
NONE4, NONE8, NONE2 = SS.NONE4, SS.NONE8, SS.NONE2
whole_lists, same, by = PH.whole_lists, PH.same, PH.by
PUSHED = ("fold", "tips", "parallel", "branch", "common")


@pytest.fixture(scope="module")
def groups(golden_dir, tmp_path_factory):
    return SS.catalogue(golden_dir, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def slot_groups(tmp_path_factory):
    """The catalogue again on a tree without a save slot and on one with two (contact_self_scene.slot_catalogue)."""
    return SS.slot_catalogue(tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_san", SAN)


@pytest.fixture(scope="module")
def capsules_driver(driver):
    return driver


def run_self(exe, tmp_path, c, substeps=1, lists=None, d_act=D_ACT, **over):
    """The self driver on a group (fields replaced by the keywords: q, qd, u, caps, spheres, planes, capsules, pairs):
    contacts_reference.read_driver_output's dict.  A sanitizer report fails it: exit status 0 and nothing on stderr."""
    SR.write_driver_input(str(tmp_path / "in.bin"), c, substeps, DT, d_act, lists=lists, **over)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "self"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    B = len(over["q"]) if over.get("q") is not None else len(c["q"])
    return CR.read_driver_output(str(tmp_path / "out.bin"), B, c["t"].n_dof)


def row_parts(c):
    """(|J| summed over the link-only dofs, over the partner-only dofs, over every other dof) of the planted pair's fp64 row."""
    t = c["t"]
    f, e = c["planted"]
    m = SS.masks(t)
    J = np.abs(SS.planted_detail(c)["J"])
    part = lambda mm: float(sum(J[k] for k in range(t.n_dof) if (mm >> k) & 1))
    return part(m[f] & ~m[e]), part(m[e] & ~m[f]), part(~(m[f] ^ m[e]))


# ---- 1: the scenes -------------------------------------------------------------------------------------------------------------

def test_scenes_meet_their_stated_conditions(groups, slot_groups):
    names = SS.robots(groups)
    slot_names = SS.robots(slot_groups)
    slot_trees = [SS.for_robot(slot_groups, name)[0]["t"] for name in slot_names]
    assert [int(t.depth_first_schedule()[3]) for t in slot_trees] == [0, 2] and all(3 <= t.n_dof <= 9 for t in slot_trees)
    assert names[:2] == ["two_joint", "panda"] and len(names) == 3
    tree = SS.for_robot(groups, names[2])[0]["t"]
    assert tree.n_dof <= 9 and int(tree.depth_first_schedule()[3]) == 1 and int(SS.for_robot(groups, "panda")[0]["t"].depth_first_schedule()[3]) == 1
    chain = [g for g in SS.GROUPS if g not in ("branch", "common")]
    assert [c["group"] for c in SS.for_robot(groups, "two_joint")] == chain          # (a chain has no branch point)
    assert [c["group"] for c in SS.for_robot(groups, "panda")] == list(SS.GROUPS)
    assert [c["group"] for c in SS.for_robot(groups, names[2])] == list(SS.GROUPS)
    assert [c["group"] for c in SS.for_robot(slot_groups, slot_names[0])] == [g for g in SS.GROUPS if g != "common"]      # (no two frames share a dof)
    assert [c["group"] for c in SS.for_robot(slot_groups, slot_names[1])] == list(SS.GROUPS)
    assert all(len(c["q"]) == SS.VARIANTS for c in groups + slot_groups)
    for c in groups + slot_groups:
        t, ref, what = c["t"], c["ref"], c["label"]
        F, K, P, C = SS.counts(c)
        m = SS.masks(t)
        assert len({e for _, e in SR.roles(t, c["pairs"])}) <= MAX_SELF_FRAMES and all(m[i] != m[j] for i, j in c["pairs"]), what
        assert not ref["capped"].any() and not c["env"]["capped"].any(), what
        kinds = SS.kinds(c)
        if c["planted"] is not None:
            f, e = c["planted"]
            pos = SR.op_order(t)
            assert pos[f] > pos[e] and sorted((f, e)) in [sorted(p) for p in c["pairs"].tolist()], what      # (the later frame is the link)
            d, d32 = SS.planted_detail(c), SS.planted_detail(c, np.float32)
            s, tt, s32, t32, gap = float(d["s"]), float(d["t"]), float(d32["s"]), float(d32["t"]), float(d["gap"])
        if c["group"] in PUSHED:
            assert SS.planted_active(c).all() and 0 < gap <= D_ACT and abs(gap - SS.GAP) < 1e-6, (what, gap)
        if c["group"] in ("fold", "mixed", "buried"):
            assert 0.2 < s < 0.8 and 0.2 < tt < 0.8 and 0.2 < s32 < 0.8 and 0.2 < t32 < 0.8, (what, s, tt, s32, t32)
            assert m[e] & ~m[f] == 0 and m[f] & ~m[e], what          # (a serial pair)
        if c["group"] == "tips":
            assert s in (0.0, 1.0) and tt in (0.0, 1.0) and (s32, t32) == (s, tt), (what, s, tt, s32, t32)
        if c["group"] == "parallel":
            segs = SS.world(c, c["caps"], c["q"][0].astype(np.float64))
            Df, De = segs[f][1], segs[e][1]
            sine = np.linalg.norm(np.cross(Df, De)) / (np.linalg.norm(Df) * np.linalg.norm(De))
            assert sine < 1e-6 and (s, tt) == (s32, t32) == (0.0, 1.0), (what, sine, s, tt, s32, t32)
        if c["group"] == "crossing":
            assert abs(gap + c["caps"][e, 3] + c["caps"][f, 3]) < 1e-6 and 0 < s < 1 and 0 < tt < 1, (what, gap)
            assert all((SR.SELF, f, e, 0) in row for row in kinds) and not c["qd"].any() and not c["u"].any() and c["lim"] is None, what
            if c["exact"]:
                assert (d["X"] == d["Y"]).all() and (d32["X"] == d32["Y"]).all(), what
                assert (d["n"] == [0, 0, 1]).all() and (d32["n"] == [0, 0, 1]).all(), what
        if c["group"] in ("branch", "common"):
            link, partner, rest = row_parts(c)
            assert link > 0.01 and partner > 0.01 and rest == 0.0, (what, link, partner, rest)      # (both terms, nothing else)
        if c["group"] == "common":
            assert c["shared"] and all((m[f] >> k) & (m[e] >> k) & 1 for k in c["shared"]), what
            assert (np.abs(c["qd"][:, c["shared"]]) > 0.1).any(1).all(), what          # (the common ancestors move)
        if c["group"] == "mixed":
            assert all({k[0] for k in row} == {SR.SPHERE, SR.PLANE, SR.CAPSULE, SR.SELF} for row in kinds), (what, kinds)
        if c["group"] == "buried":
            assert gap < -0.01 and all((SR.SELF, f, e, 0) in row for row in kinds), what
        if c["group"] == "overflow":
            assert ref["overflow"].all() and (ref["n_cand"] == 8).all() and C == 9 and len(c["pairs"]) == 2, what
            dd = SS.detail(t, c["caps"], c["pairs"], c["q"][0])
            assert sorted(np.round(dd["gap"][0], 6).tolist()) == [0.001, 0.02], (what, dd["gap"])      # (both qualify in fp64)
            assert all(sum(k[0] == SR.SELF for k in row) == 1 and sum(k[0] == SR.CAPSULE for k in row) == 7 for row in kinds), (what, kinds)
        else:
            assert not ref["overflow"].any(), what
        if c["group"] == "far":
            assert all(k[0] == SR.SPHERE for row in kinds for k in row) and (ref["n_cand"] > 0).all() and len(c["pairs"]) >= 1, what
            assert SS.detail(t, c["caps"], c["pairs"], c["q"][0])["gap"].min() > SS.FAR, what
    # the Panda's branch pair is finger against finger, prismatic on both sides; a tree's self rows have a revolute dof on both
    panda = by(SS.for_robot(groups, "panda"), "branch")[0]
    assert sorted(panda["planted"]) == [9, 10] and S.prismatic_ancestors(panda["t"], 9) and S.prismatic_ancestors(panda["t"], 10)


# ---- 2: the envelope -----------------------------------------------------------------------------------------------------------

def envelope_ratios(groups):
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0, gap=0.0)
    for c in groups:
        ok = ~np.asarray(c["env"]["capped"], bool) & ~np.asarray(c["ref"]["capped"], bool)
        r = SS.per_robot_ratios(c, c["env"])
        for k in ("res", "vel", "force", "gap"):
            worst[k] = max(worst[k], float(r[k][ok].max()))
        ok &= ~np.asarray(c["env_step"]["capped"], bool) & ~np.asarray(c["ref_step"]["capped"], bool)
        worst["step"] = max(worst["step"], float(SS.step_ratios(c, c["env_step"])[ok].max()))
    return worst


def test_envelope_backs_the_bounds_and_keeps_the_robots(groups, slot_groups):
    """The K's are the catalogue's.  The trees of the other two save-slot counts are held to the same K's, none of their own:
    where their envelope is above K / 4 the kept rule leaves the robot out, and at least 90 % of each robot type's stay."""
    worst = envelope_ratios(groups)
    print("envelope worst ratios", worst)
    print("envelope worst ratios on the slot trees", envelope_ratios(slot_groups))
    for k, K in K_SELF.items():
        assert np.isclose(K, S._round_up_1sf(4 * MEASURED_SELF[k])), (k, K, MEASURED_SELF[k])
        assert 4 * worst[k] <= K, (k, worst[k], K)
    for name in SS.robots(groups) + SS.robots(slot_groups):
        gs = SS.for_robot(groups + slot_groups, name)
        keep = np.concatenate([SS.kept(c, K_SELF) for c in gs]), np.concatenate([SS.kept_step(c, K_SELF) for c in gs])
        print(name, "kept", keep[0].mean(), "kept over the step", keep[1].mean())
        assert keep[0].mean() >= 0.9 and keep[1].mean() >= 0.9, (name, keep[0].mean(), keep[1].mean())


# ---- 3: the device routine on the CPU against the reference -------------------------------------------------------------------

def test_device_routine_on_the_cpu_against_the_reference(driver, groups, slot_groups, tmp_path):
    worst, kept = {}, 0
    groups = groups + slot_groups
    for c in groups:
        B, K = len(c["q"]), len(c["spheres"])
        d = run_self(driver, tmp_path, c)
        kept += SS.check_group(c, d, K_SELF, c["label"], worst)
        dl = run_self(driver, tmp_path, c, lists=whole_lists(B, K))      # (the list form on the same records)
        SS.check_group(c, dl, K_SELF, c["label"] + "-lists", worst)
        d4 = run_self(driver, tmp_path, c, substeps=SS.STEP_SUBSTEPS)
        SS.check_group_step(c, d4, K_SELF, c["label"], worst)
        d4 = run_self(driver, tmp_path, c, substeps=SS.STEP_SUBSTEPS, lists=whole_lists(B, K))
        SS.check_group_step(c, d4, K_SELF, c["label"] + "-lists", worst)
        if c["group"] in PUSHED:
            assert SS.planted_active(c, d).all() and ((d["pair"] >= 0).sum(1) == 1).all(), c["label"]
        if c["group"] == "common":      # the dofs common to both links: exactly 0.f in the row, so in the contact torque
            for got in (d, dl):
                assert (got["lam"] > 0).any(1).all() and (got["contact"][:, c["shared"]] == 0).all(), c["label"]
                others = [k for k in range(c["t"].n_dof) if k not in c["shared"]]
                assert (got["contact"][:, others] != 0).any(1).all(), c["label"]
    print("CPU driver worst ratios", worst, "kept", kept)
    assert kept >= 0.9 * sum(len(c["q"]) for c in groups)
    for k, K in K_SELF.items():
        assert worst[k] <= K, (k, worst[k], K)


def test_all_partner_slots_in_use_with_the_solver_running_on_the_last(driver, tmp_path_factory, tmp_path):
    """contact_self_scene.full_store_case: MAX_SELF_FRAMES partners of one link, the stored ends of the last slots lying over the
    solver's Gram factor and multipliers, and the one near pair is the one in the highest slot: the search has read every slot
    before the solver writes a word, in each of the substeps."""
    c = SS.full_store_case(tmp_path_factory.mktemp("long_chain"), MAX_SELF_FRAMES, K_SELF)
    assert SS.kept_step(c, K_SELF).all() and len({e for _, e in SR.roles(c["t"], c["pairs"])}) == MAX_SELF_FRAMES and c["planted"][1] == int(c["pairs"][-1][1])
    for lists in (None, whole_lists(len(c["q"]), 0)):
        d = run_self(driver, tmp_path, c, lists=lists)
        SS.check_group(c, d, K_SELF, c["label"])
        assert SS.planted_active(c, d).all() and ((d["pair"] >= 0).sum(1) == 1).all()
        SS.check_group_step(c, run_self(driver, tmp_path, c, substeps=SS.STEP_SUBSTEPS, lists=lists), K_SELF, c["label"])


# ---- 4: bit for bit -------------------------------------------------------------------------------------------------------------

def test_no_pairs_and_far_pairs_are_the_capsules_call_bit_for_bit(driver, capsules_driver, groups, slot_groups, tmp_path):
    seen = 0
    for c in by(groups + slot_groups, "far") + by(groups, "mixed") + by(groups, "overflow"):
        B, K = len(c["q"]), len(c["spheres"])
        for substeps in (1, 3):
            for lists in (None, whole_lists(B, K)):
                want = QH.run_capsules(capsules_driver, tmp_path, c, substeps=substeps, lists=lists)
                got = run_self(driver, tmp_path, dict(c, pairs=NONE2), substeps=substeps, lists=lists)
                same(got, want, (c["label"], "no pairs"))
                if c["group"] == "far":
                    same(run_self(driver, tmp_path, c, substeps=substeps, lists=lists), want, (c["label"], "far"))
                seen += int((want["pair"] >= 0).sum())
    assert seen >= 100


def test_a_pair_on_a_zero_capsule_row_equals_no_such_pair(driver, groups, slot_groups, tmp_path):
    """Whether it is the link's row or the partner's that is zero."""
    for c in by(groups + slot_groups, "overflow"):
        (x, y), (_, z) = c["pairs"].tolist()
        for gone, left in ((y, [(x, z)]), (z, [(x, y)]), (x, NONE2)):
            caps = c["caps"].copy()
            caps[gone] = 0
            for lists in (None, whole_lists(len(c["q"]), 0)):
                a = run_self(driver, tmp_path, c, substeps=2, caps=caps, lists=lists)
                b = run_self(driver, tmp_path, dict(c, pairs=np.array(left, np.int32).reshape(-1, 2)), substeps=2, caps=caps, lists=lists)
                same(a, b, (c["label"], gone))
                assert (a["pair"] >= 0).any()


def test_a_partner_that_hangs_on_no_dof_is_the_obstacle_capsule_bit_for_bit(driver, capsules_driver, groups, slot_groups, tmp_path):
    """A partner frame that no dof moves, with a capsule whose world segment is the same numbers in fp32 and fp64 (its two ends at
    the frame's origin: A = p, D = 0 in any arithmetic; asserted): the self call equals the capsules call with that segment as an
    obstacle capsule and the partner's own link capsule taken off -- everything but the pair index."""
    seen = 0
    for name in SS.robots(groups + slot_groups):
        c = by(SS.for_robot(groups + slot_groups, name), "fold")[0]
        t = c["t"]
        m, pos = SS.masks(t), SR.op_order(t)
        for e in [g for g in range(t.n_frames) if m[g] == 0]:
            for f in [g for g in range(t.n_frames) if m[g] and pos[g] > pos[e]][:3]:
                # the link's capsule: of three segments the one whose row has the longest lever
                segs = [SS.local_segment(c, f), (np.array([0.15, 0.0, 0.0]), np.array([0.15, 0.1, 0.1])), (np.array([0.0, 0.15, 0.0]), np.array([0.1, 0.15, 0.1]))]
                table = lambda seg: SS.caps_of(c, {e: (np.zeros(3), np.zeros(3)), f: seg}, {e: 0.05, f: 0.05})
                caps = max((table(seg) for seg in segs), key=lambda cp: np.abs(SS.detail(t, cp, [(f, e)], c["q"][0])["J"]).sum())
                w64, w32 = (CR.poses(t, c["q"][:1].astype(dt), dt)[1][e][0] for dt in (np.float64, np.float32))
                assert (w64 == w32).all() and w32.dtype == np.float32          # (the partner's world segment is exact)
                # the pair brought to 0.02 mm by the radii
                d = SS.detail(t, caps, [(f, e)], c["q"][0])
                dist = float(d["gap"][0, 0]) + 0.1
                if not 0.03 < dist < 1.0:
                    continue
                caps[[e, f], 3] = np.float32(0.5 * (dist - 2e-5))
                qd, u = SS.PS._into(np.random.default_rng(7), c, c["q"][0].astype(np.float64), [d["J"][0, 0]])      # (into it)
                obstacle = np.array([[*w32, caps[e, 3], *w32, 0.0]], np.float32)
                alone = caps.copy()
                alone[e] = 0
                cs = dict(c, caps=caps, pairs=np.array([[f, e]], np.int32), spheres=NONE4, planes=NONE4, capsules=NONE8, qd=qd, u=u)
                co = dict(c, caps=alone, capsules=obstacle, spheres=NONE4, planes=NONE4, qd=qd, u=u)
                for substeps in (1, 3):
                    a = run_self(driver, tmp_path, cs, substeps=substeps)
                    b = QH.run_capsules(capsules_driver, tmp_path, co, substeps=substeps)
                    same(a, b, (c["label"], f, e, substeps), pairs=False)
                    F = t.n_frames
                    assert np.array_equal(a["pair"] >= 0, b["pair"] >= 0)
                    assert all(SR.split_pair(p, F, 0, 0, 0) == (SR.SELF, f, e, 0) for p in a["pair"][a["pair"] >= 0])
                    assert all(QR.split_pair(p, F, 0, 0, 1) == (QR.CAPSULE, f, 0, 0) for p in b["pair"][b["pair"] >= 0])
                    seen += int((a["lam"] > 0).sum())
    assert seen >= 4


# ---- 5: pair indices -------------------------------------------------------------------------------------------------------------

def test_pair_indices_decode_to_the_planted_link_and_partner(driver, groups, slot_groups, tmp_path):
    from riemannian_motion_policies_amd import engine as E
    seen = set()
    for c in groups + slot_groups:
        F, K, P, C = SS.counts(c)
        d = run_self(driver, tmp_path, c)
        pr = SR.pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["pairs"], c["q"])
        frames = CR.capsule_frames(c["caps"])
        for r, row in enumerate(d["pair"]):
            for p in row[row >= 0]:
                kind, f, rec, e = E.contact_pair_split(p, F, K, P, C, self_pairs=True)
                assert (kind, f, rec, e) == SR.split_pair(p, F, K, P, C)
                assert f in frames and rec < {E.CONTACT_KIND_SPHERE: K, E.CONTACT_KIND_PLANE: P, E.CONTACT_KIND_CAPSULE: C, E.CONTACT_KIND_SELF: F}[kind]
                if kind == E.CONTACT_KIND_SELF:
                    assert (f, rec) in SR.roles(c["t"], c["pairs"])
                else:
                    assert E.contact_pair_split(p, F, K, P, C) == (kind, f, rec, e)          # (the other kinds: as without the flag)
                assert pr["gap"][r, list(pr["idx"]).index(int(p))] <= D_ACT + 1e-5
                seen.add(kind)
        if c["planted"] is not None and c["group"] != "overflow":
            want = (E.CONTACT_KIND_SELF, *c["planted"], 0)
            assert all(want in {E.contact_pair_split(p, F, K, P, C, self_pairs=True) for p in row} for row in d["pair"]), c["label"]
    assert seen == {0, 1, 2, 3}
    base = 3 * 4 + 2 * 3 * 2 + 3 * 5
    assert E.contact_pair_split(-1, 3, 4, 2, 5, self_pairs=True) is None
    assert E.contact_pair_split(base + 2 * 3 + 1, 3, 4, 2, 5, self_pairs=True) == (3, 2, 1, 0)
    assert E.contact_pair_split(base - 1, 3, 4, 2, 5, self_pairs=True) == (2, 2, 4, 0) == E.contact_pair_split(base - 1, 3, 4, 2, 5)
    assert E.contact_pair_split(3 * 4 + 1, 3, 4, 2, 0, self_pairs=True) == (1, 0, 0, 1)
    assert E.contact_pair_split(3 * 4 + 2 * 3 * 2 + 5, 3, 4, 2, 0, self_pairs=True) == (3, 1, 2, 0)
    with pytest.raises(ValueError):
        E.contact_pair_split(base + 9, 3, 4, 2, 5, self_pairs=True)
    with pytest.raises(ValueError):
        E.contact_pair_split(base, 3, 4, 2, 5)          # (without the flag: as before the self contacts)


def test_pair_split_macros_of_the_header(tmp_path):
    """The RMP2_CONTACT_PAIR_* macros with the self kind, compiled as C, against the reference's split over a whole range."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    src = tmp_path / "split.c"
    src.write_text('#include <stdio.h>\n#include "rmp2.h"\nint main(void) {\n  const int F = 5, K = 3, P = 2, C = 4;\n'
                   '  if (RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C) != F * K + 2 * F * P + F * C) return 1;\n'
                   '  for (int32_t p = 0; p < F * K + 2 * F * P + F * C + F * F; ++p) {\n'
                   '    const int kind = RMP2_CONTACT_PAIR_KIND4(p, F, K, P, C);\n'
                   '    if (kind == RMP2_CONTACT_KIND_SELF)\n'
                   '      printf("%d %d %d %d 0\\n", p, kind, RMP2_CONTACT_PAIR_SELF_LINK(p, F, K, P, C), RMP2_CONTACT_PAIR_SELF_PARTNER(p, F, K, P, C));\n'
                   '    else if (kind == RMP2_CONTACT_KIND_CAPSULE)\n'
                   '      printf("%d %d %d %d 0\\n", p, kind, RMP2_CONTACT_PAIR_CAPSULE_FRAME(p, F, K, P, C), RMP2_CONTACT_PAIR_CAPSULE_RECORD(p, F, K, P, C));\n'
                   '    else\n'
                   '      printf("%d %d %d %d %d\\n", p, kind, RMP2_CONTACT_PAIR_FRAME(p, F, K, P), RMP2_CONTACT_PAIR_RECORD(p, F, K, P),\n'
                   '             RMP2_CONTACT_PAIR_END(p, F, K));\n  }\n  return 0;\n}\n')
    exe = tmp_path / "split"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(lines) == 5 * 3 + 2 * 5 * 2 + 5 * 4 + 5 * 5
    for p, k, f, r, e in lines:
        assert (k, f, r, e) == SR.split_pair(p, 5, 3, 2, 4)
    assert lines[55][1:] == [3, 0, 0, 0] and lines[54][1:] == [2, 4, 3, 0] and lines[-1][1:] == [3, 4, 4, 0]


def tie_case(groups, n_small):
    """tests/test_contact_capsules_host.tie_case with a self pair: the two-joint robot at q = 0 with the tip sphere; n_small planes
    at smaller gaps; a sphere, a plane and a vertical obstacle capsule at the gap 0.09375 - r_tip below the tip to the bit; and
    link 1 carrying a point capsule of the sphere's radius as far ABOVE the tip (its world point exact): the self pair (tip,
    link 1) at the same gap to the bit, and too far from the three obstacles to meet them."""
    c = QH.tie_case([dict(by(SS.for_robot(groups, "two_joint"), "far")[0], group="post")], n_small)      # (the base capsule table)
    caps = c["caps"].copy()
    tip = c["spheres"][0, :3]
    z0 = np.float32(c["t"].T_const[0][2, 3])
    caps[0] = [tip[0], 0.21875, tip[2] - z0, 0.125, tip[0], 0.21875, tip[2] - z0, 0.0]
    return dict(c, caps=caps, pairs=np.array([[0, 2]], np.int32), planted=(2, 0))


def test_a_sphere_a_plane_a_capsule_and_a_self_pair_at_equal_gap_tie_in_that_order(driver, groups, tmp_path):
    for n_small, kept_kinds in ((4, [SR.SPHERE, SR.PLANE, SR.CAPSULE, SR.SELF]), (5, [SR.SPHERE, SR.PLANE, SR.CAPSULE]), (6, [SR.SPHERE, SR.PLANE])):
        c = tie_case(groups, n_small)
        F, K, P, C = SS.counts(c)
        assert (F, K, P, C) == (3, 1, n_small + 1, 1)
        pr = SR.pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["pairs"], c["q"], np.float32)
        gaps = dict(zip(pr["idx"].tolist(), pr["gap"][0].tolist()))
        tied = [2 * K + 0, PR.pair_index(F, K, P, 2, n_small, 0), QR.pair_index(F, K, P, C, 2, 0), SR.pair_index(F, K, P, C, 2, 0)]
        assert len({gaps[i] for i in tied}) == 1 and 0 < gaps[tied[0]] <= D_ACT and tied == sorted(tied), (gaps, tied)
        small = [PR.pair_index(F, K, P, 2, k, 0) for k in range(n_small)]
        assert sorted(i for i, g in gaps.items() if g <= D_ACT) == sorted(small + tied), gaps      # (link 1's point meets no obstacle)
        want = sorted(small + tied[:8 - n_small])
        assert [SR.split_pair(p, F, K, P, C)[0] for p in tied[:8 - n_small]] == kept_kinds
        ref = SR.substep(c["t"], c["inert"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["pairs"], D_ACT, c["q"], c["qd"],
                         c["u"], c["drive"], DT, c["lim"], c["limits"], c["g"], envelope=True)      # (the tie is one of fp32 values)
        for lists in (None, whole_lists(1, K)):
            d = run_self(driver, tmp_path, c, lists=lists)
            assert bool(d["status"][0] & CR.OVERFLOW) == bool(ref["overflow"][0]) == (n_small > 4)
            assert sorted(d["pair"][0]) == want == sorted(ref["pair"][0]), (d["pair"][0], ref["pair"][0], want)


# ---- 6: under the host sanitizers (a stand-alone program; the pair tables hold exactly their records) --------------------------------

def test_driver_under_the_host_sanitizers_equals_the_plain_build(driver, driver_san, groups, tmp_path, tmp_path_factory):
    full = SS.full_store_case(tmp_path_factory.mktemp("long_chain"), MAX_SELF_FRAMES, K_SELF)      # (every slot of the store)
    for c in SS.for_robot(groups, "two_joint") + by(groups, "overflow") + by(groups, "mixed") + by(groups, "common") + [tie_case(groups, 5), full]:
        for lists in (None, whole_lists(len(c["q"]), len(c["spheres"]))):
            same(run_self(driver_san, tmp_path, c, substeps=2, lists=lists), run_self(driver, tmp_path, c, substeps=2, lists=lists), c["label"])
    c = by(groups, "far")[1]
    run_self(driver_san, tmp_path, c, substeps=2)
    run_self(driver_san, tmp_path, dict(c, pairs=NONE2), planes=NONE4, spheres=NONE4, capsules=NONE8)


# ---- 7: the interface --------------------------------------------------------------------------------------------------------------

def test_symbols_declared_and_bound_with_their_constants(hip_lib):
    import ctypes as C
    lib = C.CDLL(hip_lib)
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    for sym in ("rmp2_dynamics_step_contacts_self", "rmp2_set_contact_self_pairs"):
        assert re.search(r"\bint %s\(" % sym, hdr) and hasattr(lib, sym)
    assert "#define RMP2_MAX_CONTACT_SELF_FRAMES 22" in hdr and "#define RMP2_CONTACT_KIND_SELF 3" in hdr
    for macro in ("RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C)", "RMP2_CONTACT_PAIR_SELF_LINK(", "RMP2_CONTACT_PAIR_SELF_PARTNER(",
                  "RMP2_CONTACT_PAIR_CAPSULE_FRAME(", "RMP2_CONTACT_PAIR_KIND3(pair, F, K, P)"):
        assert "#define " + macro in hdr, macro
    assert re.search(r"#define RMP2_ABI_VERSION (\d+)", hdr).group(1) == "5" and lib.rmp2_abi_version() == 5
    from riemannian_motion_policies_amd import _native, engine as E
    assert E.MAX_CONTACT_SELF_FRAMES == MAX_SELF_FRAMES and E.CONTACT_KIND_SELF == 3 == SR.SELF
    assert len(_native.lib().rmp2_dynamics_step_contacts_self.argtypes) == 28 == len(_native.lib().rmp2_dynamics_step_contacts_capsules.argtypes)
    assert len(_native.lib().rmp2_set_contact_self_pairs.argtypes) == 3
    args = [None] * 28
    for k, v in ((4, 0), (9, 0), (13, 0), (15, 0), (16, 0.0), (17, 0.0), (18, 0), (26, 0)):
        args[k] = v
    assert _native.lib().rmp2_dynamics_step_contacts_self(*args) == -1          # (no handle: RMP2_ERR_INVALID_ARGUMENT)
    assert _native.lib().rmp2_set_contact_self_pairs(None, 0, None) == -1
    import __graft_entry__ as g
    names = [u[0] for u in g.HIP_UNITS]
    assert "rmp2_contacts_l0_self" in names and "rmp2_contacts_l1_self" in names and len(names) == len(set(names))
    # the storage the constant is chosen from: 6 words per partner over the solver's words of a 9-dof robot, within 64 KiB
    solver9 = 9 * 9 + 45 + 9
    assert 6 * MAX_SELF_FRAMES <= solver9 < 6 * (MAX_SELF_FRAMES + 1) and (45 + 72 + solver9) * 64 * 4 <= 65536


def test_urdf_contact_self_pairs_on_the_panda_and_a_tree(groups):
    import dataclasses
    from riemannian_motion_policies_amd import urdf as U
    panda = SS.for_robot(groups, "panda")[0]["t"]
    tree = SS.for_robot(groups, SS.robots(groups)[2])[0]["t"]
    if not any(tree.has_collision):      # (the random trees carry no collision shapes: every frame gets one)
        tree = dataclasses.replace(tree, has_collision=np.ones(tree.n_frames, bool))
    for t in (panda, tree):
        m = SS.masks(t)
        pairs = U.contact_self_pairs(t)
        assert pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2 and len(pairs) > 0
        got = {tuple(p) for p in pairs.tolist()}
        assert len(got) == len(pairs) and all(i < j for i, j in got)          # (each unordered pair once)
        want = set()
        for i in range(t.n_frames):
            for j in range(i + 1, t.n_frames):
                near = U._within_neighborhood(t, i, j, 3)
                assert near == U._within_neighborhood(t, j, i, 3)          # (the hop rule in both directions)
                if t.has_collision[i] and t.has_collision[j] and not near and m[i] != m[j]:
                    want.add((i, j))
        assert got == want
        assert all(m[i] != m[j] for i, j in got)          # (no rigid pair)
        assert len({e for _, e in SR.roles(t, pairs)}) <= MAX_SELF_FRAMES          # (the kernel holds the whole set)
        assert len(U.contact_self_pairs(t, n_neighbors=1)) >= len(pairs)
    assert (9, 10) in {tuple(p) for p in U.contact_self_pairs(panda).tolist()}          # (the fingers: siblings, neither a parent of the other)

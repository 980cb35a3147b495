"""Capsule obstacles beside the spheres and the half-spaces (include/rmp2.h rmp2_dynamics_step_contacts_capsules) on the host:
the scenes of tests/contact_capsules_scene.py meet their stated conditions; the fp32 envelope that the bounds are taken from; the
capsule form of the device routine of rmp2_contacts.h run on the CPU through tests/contacts_driver.cpp (also under the host
sanitizers, as a stand-alone program) against the fp64 reference of tests/contact_capsules_reference.py, and BIT FOR BIT against
the planes, sphere and stops drivers where the contract promises it; pair indices, ties between the kinds, poisoning, the header,
the bindings and urdf.capsule_obstacles / urdf.cylinders_as_capsules.  No GPU.

The bounds are those of tests/test_contacts_host.py (stationarity, velocity, total constraint torque, linearised gap of the
device's own pairs after one substep; q / qd after STEP_SUBSTEPS), with the K's of these scenes by the same rule: K = 4 x the worst
ratio of the fp32 ENVELOPE against the fp64 reference over the catalogue, rounded up to one significant figure (MEASURED_CAPSULES
-> K_CAPSULES, fixed here from the CPU run before any GPU run; test_envelope_backs_the_bounds measures them again).  Robots held
to the bounds: the kept rule of DESIGN 4.12 (envelope uncapped and within K / 4)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contact_capsules_reference as QR
import contact_capsules_scene as QS
import contact_planes_reference as PR
import contacts_reference as CR
import test_contact_planes_host as PH
import test_contacts_host as S
from test_contacts_host import D_ACT, DT, ROOT

MEASURED_CAPSULES = dict(res=0.02946, vel=13.46, force=7.132, step=23.68, gap=0.09006)      # the envelope's worst ratios
K_CAPSULES = dict(res=0.2, vel=60.0, force=30.0, step=100.0, gap=0.4)
MAX_CAPSULES = 32
FLOATS = PH.FLOATS
SAN = PH.SAN
NONE4, NONE8 = QS.NONE4, QS.NONE8
whole_lists, same, by = PH.whole_lists, PH.same, PH.by


@pytest.fixture(scope="module")
def groups(golden_dir, tmp_path_factory):
    return QS.catalogue(golden_dir, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def slot_groups(tmp_path_factory):
    """The catalogue again on a tree without a save slot and on one with two (contact_capsules_scene.slot_catalogue)."""
    return QS.slot_catalogue(tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_san", SAN)


@pytest.fixture(scope="module")
def planes_driver(driver):
    return driver


@pytest.fixture(scope="module")
def stops_driver(tmp_path_factory):
    return S._build(tmp_path_factory, "joint_stops_driver.cpp", "joint_stops_driver")


def run_capsules(exe, tmp_path, c, substeps=1, lists=None, d_act=D_ACT, **over):
    """The capsule driver on a group (fields replaced by the keywords: q, qd, u, caps, spheres, planes, capsules):
    contacts_reference.read_driver_output's dict.  A sanitizer report fails it: exit status 0 and nothing on stderr."""
    QR.write_driver_input(str(tmp_path / "in.bin"), c, substeps, DT, d_act, lists=lists, **over)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "capsules"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    B = len(over["q"]) if over.get("q") is not None else len(c["q"])
    return CR.read_driver_output(str(tmp_path / "out.bin"), B, c["t"].n_dof)


# ---- 1: the scenes -------------------------------------------------------------------------------------------------------------

def test_scenes_meet_their_stated_conditions(groups, slot_groups):
    names = QS.robots(groups)
    slot_trees = [QS.for_robot(slot_groups, name)[0]["t"] for name in QS.robots(slot_groups)]
    assert [int(t.depth_first_schedule()[3]) for t in slot_trees] == list(QS.SLOT_COUNTS) == [0, 2]      # (the N = 9 kernels' other two)
    assert all(3 <= t.n_dof <= 9 for t in slot_trees) and [c["group"] for c in slot_groups] == list(QS.GROUPS) * 2
    assert sorted({int(QS.for_robot(groups, n)[0]["t"].depth_first_schedule()[3]) for n in names[1:]} | set(QS.SLOT_COUNTS)) == [0, 1, 2]
    assert names[:2] == ["two_joint", "panda"] and len(names) == 3
    assert [c["group"] for c in groups] == list(QS.GROUPS) * 3
    assert all(len(c["q"]) == QS.VARIANTS for c in groups) and sum(len(c["q"]) for c in groups) <= QS.MIXED_R
    tree = QS.for_robot(groups, names[2])[0]
    assert tree["t"].n_dof <= 9 and int(tree["t"].depth_first_schedule()[3]) >= 1
    for c in groups + slot_groups:
        F, K, P, C = QS.counts(c)
        ref, what = c["ref"], c["label"]
        assert C <= MAX_CAPSULES and (c["capsules"][:, 7] == 0).all() and (c["capsules"][:, 3] > 0).all(), what
        assert not ref["capped"].any() and not c["env"]["capped"].any(), what
        kinds, active = QS.kinds(c), QS.active_kinds(c)
        if c["planted"] is not None:
            d = QS.detail(c, c["q"][0], c["capsules"])
            k = list(d["idx"]).index(QR.pair_index(F, 0, 0, C, *c["planted"]))
            s, t, gap = float(d["s"][0, k]), float(d["t"][0, k]), float(d["gap"][0, k])
            d32 = QS.detail(c, c["q"][0], c["capsules"], dtype=np.float32)
            s32, t32 = float(d32["s"][0, k]), float(d32["t"][0, k])
            a, b = c["capsules"][c["planted"][1], 0:3], c["capsules"][c["planted"][1], 4:7]
        if c["group"] in ("post", "cap", "tip", "point", "parallel", "mixed"):
            assert QS.planted_active(c).all() and 0 < gap <= D_ACT, what      # (approached, the capsule pushing back)
        if c["group"] in ("post", "mixed"):
            assert 0.2 < s < 0.8 and 0.2 < t < 0.8 and 0.2 < s32 < 0.8 and 0.2 < t32 < 0.8 and (a != b).any(), what
        if c["group"] == "cap":
            assert t == 0 and t32 == 0 and 0.2 < s < 0.8 and (a != b).any(), what
        if c["group"] == "tip":
            assert s in (0.0, 1.0) and s32 == s and 0.2 < t < 0.8, what
        if c["group"] == "parallel":
            A, D, _ = QS.segments(c, c["q"][0])[c["planted"][0]]
            sine = np.linalg.norm(np.cross(D, b.astype(np.float64) - a)) / (np.linalg.norm(D) * np.linalg.norm(b - a))
            assert sine < 1e-6, (what, sine)
            if c["exact"]:      # (to the bit: the s = 0 end first, the post covering it)
                assert sine == 0 and s == 0 and s32 == 0 and 0 < t < 1 and 0 < t32 < 1, (what, s, s32, t, t32)
            else:               # (to rounding: end to end)
                assert s == s32 == 1 and t == t32 == 0, (what, s, s32, t, t32)
        if c["group"] == "crossing":
            assert abs(gap + c["capsules"][0, 3] + c["caps"][c["planted"][0], 3]) < 1e-6 and 0 < s < 1 and 0 < t < 1, (what, gap)
            assert all((QR.CAPSULE, *c["planted"], 0) in row for row in kinds), what
            if c["exact"]:
                assert (d["X"][0, k] == d["Y"][0, k]).all() and (d32["X"][0, k] == d32["Y"][0, k]).all(), what
                assert (d["n"][0, k] == [0, 0, 1]).all() and (d32["n"][0, k] == [0, 0, 1]).all(), what
        if c["group"] == "point":
            assert (a == b).all() and t == 0, what
        if c["group"] == "mixed":
            assert all({s[0] for s in row} == {QR.SPHERE, QR.PLANE, QR.CAPSULE} for row in kinds), (what, kinds)
            assert all(QR.CAPSULE in a_ and len(a_) >= 2 for a_ in active), (what, active)      # (the capsule and another kind push)
        if c["group"] == "buried":
            assert gap < -0.01 and all((QR.CAPSULE, *c["planted"], 0) in row for row in kinds), what
        if c["group"] == "overflow":
            assert ref["overflow"].all() and (ref["n_cand"] == 8).all() and C == 9, what
            kept_caps = [sum(s[0] == QR.CAPSULE for s in row) for row in kinds]
            assert all(1 <= n < 9 for n in kept_caps), (what, kept_caps)      # (capsule rows among the kept and the dropped)
            assert all(any(s[0] == QR.SPHERE for s in row) for row in kinds), what
        else:
            assert not ref["overflow"].any(), what
        if c["group"] == "far":
            assert all(s[0] == QR.SPHERE for row in kinds for s in row) and (ref["n_cand"] > 0).all(), what
            assert QS.detail(c, c["q"][0], c["capsules"])["gap"].min() > 40.0 and C == 7, what
    # the tree's capsule rows have a prismatic column
    rows = [s for c in QS.for_robot(groups, names[2]) for row in QS.kinds(c) for s in row if s[0] == QR.CAPSULE]
    assert any(S.prismatic_ancestors(tree["t"], s[1]) for s in rows)


# ---- 2: the envelope -----------------------------------------------------------------------------------------------------------

def envelope_ratios(groups):
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0, gap=0.0)
    for c in groups:
        ok = ~np.asarray(c["env"]["capped"], bool) & ~np.asarray(c["ref"]["capped"], bool)
        r = QS.per_robot_ratios(c, c["env"])
        for k in ("res", "vel", "force", "gap"):
            worst[k] = max(worst[k], float(r[k][ok].max()))
        ok &= ~np.asarray(c["env_step"]["capped"], bool) & ~np.asarray(c["ref_step"]["capped"], bool)
        worst["step"] = max(worst["step"], float(QS.step_ratios(c, c["env_step"])[ok].max()))
    return worst


def test_envelope_backs_the_bounds_and_keeps_the_robots(groups, slot_groups):
    """The K's are the catalogue's.  The trees of the other two save-slot counts are held to the same K's, none of their own:
    where their envelope is above K / 4 the kept rule leaves the robot out, and at least 90 % of each tree's stay."""
    worst = envelope_ratios(groups)
    print("envelope worst ratios", worst)
    print("envelope worst ratios on the slot trees", envelope_ratios(slot_groups))
    for k, K in K_CAPSULES.items():
        assert np.isclose(K, S._round_up_1sf(4 * MEASURED_CAPSULES[k])), (k, K, MEASURED_CAPSULES[k])
        assert 4 * worst[k] <= K, (k, worst[k], K)
    for name in QS.robots(groups) + QS.robots(slot_groups):
        gs = QS.for_robot(groups + slot_groups, name)
        keep = np.concatenate([QS.kept(c, K_CAPSULES) for c in gs]), np.concatenate([QS.kept_step(c, K_CAPSULES) for c in gs])
        print(name, "kept", keep[0].mean(), "kept over the step", keep[1].mean())
        assert keep[0].mean() >= 0.9 and keep[1].mean() >= 0.9, (name, keep[0].mean(), keep[1].mean())


# ---- 3: the device routine on the CPU against the reference -------------------------------------------------------------------

def test_device_routine_on_the_cpu_against_the_reference(driver, groups, slot_groups, tmp_path):
    worst, kept = {}, 0
    groups = groups + slot_groups
    for c in groups:
        B, K = len(c["q"]), len(c["spheres"])
        d = run_capsules(driver, tmp_path, c)
        kept += QS.check_group(c, d, K_CAPSULES, c["label"], worst)
        dl = run_capsules(driver, tmp_path, c, lists=whole_lists(B, K))      # (the list form on the same records)
        QS.check_group(c, dl, K_CAPSULES, c["label"] + "-lists", worst)
        d4 = run_capsules(driver, tmp_path, c, substeps=QS.STEP_SUBSTEPS)
        QS.check_group_step(c, d4, K_CAPSULES, c["label"], worst)
        d4 = run_capsules(driver, tmp_path, c, substeps=QS.STEP_SUBSTEPS, lists=whole_lists(B, K))
        QS.check_group_step(c, d4, K_CAPSULES, c["label"] + "-lists", worst)
        if c["group"] in ("post", "cap", "tip", "point", "parallel"):
            assert QS.planted_active(c, d).all(), c["label"]
    print("CPU driver worst ratios", worst, "kept", kept)
    assert kept >= 0.9 * sum(len(c["q"]) for c in groups)
    for k, K in K_CAPSULES.items():
        assert worst[k] <= K, (k, worst[k], K)


# ---- 4: bit for bit -------------------------------------------------------------------------------------------------------------

def test_no_capsules_and_far_capsules_are_the_planes_call_bit_for_bit(driver, planes_driver, groups, tmp_path):
    seen = 0
    for c in by(groups, "far") + by(groups, "mixed") + by(groups, "overflow"):
        B, K = len(c["q"]), len(c["spheres"])
        for substeps in (1, 3):
            for lists in (None, whole_lists(B, K)):
                want = S.run_driver(planes_driver, tmp_path, c, substeps=substeps, lists=lists, planes=c["planes"])
                same(run_capsules(driver, tmp_path, c, substeps=substeps, lists=lists, capsules=NONE8), want, (c["label"], "C = 0"))
                if c["group"] == "far":
                    same(run_capsules(driver, tmp_path, c, substeps=substeps, lists=lists), want, (c["label"], "far"))
                seen += int((want["pair"] >= 0).sum())
    assert seen >= 100


def test_nothing_at_all_is_the_stops_step_bit_for_bit(driver, stops_driver, groups, tmp_path):
    import test_joint_stops_host as SH
    for c in by(groups, "post") + by(groups, "mixed"):
        for substeps in (1, 3):
            s = SH.run_driver(stops_driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"],
                              substeps, c["g"])
            for lists in (None, whole_lists(len(c["q"]), 0)):
                d = run_capsules(driver, tmp_path, c, substeps=substeps, spheres=NONE4, planes=NONE4, capsules=NONE8, lists=lists)
                for k in ("q", "qd", "qdd", "tau", "stop"):
                    assert S._bits_equal(d[k], s[k]), (c["label"], k)
                assert (d["status"] == s["status"]).all() and (d["contact"] == 0).all() and (d["lam"] == 0).all() and (d["pair"] == -1).all()


def test_a_point_capsule_is_the_sphere_bit_for_bit(driver, groups, tmp_path):
    """a == b: the same call with the record moved into the sphere table -- everything but the pair index."""
    for c in by(groups, "point"):
        F = c["t"].n_frames
        sphere = np.ascontiguousarray(c["capsules"][:, 0:4])
        assert (c["capsules"][:, 0:3] == c["capsules"][:, 4:7]).all() and len(c["spheres"]) == 0
        for substeps in (1, 3):
            for lists, slists in ((None, None), (whole_lists(len(c["q"]), 0), whole_lists(len(c["q"]), 1))):
                a = run_capsules(driver, tmp_path, c, substeps=substeps, lists=lists)
                b = run_capsules(driver, tmp_path, c, substeps=substeps, lists=slists, spheres=sphere, capsules=NONE8)
                same(a, b, (c["label"], substeps), pairs=False)
                ka = [[QR.split_pair(p, F, 0, 0, 1) for p in row] for row in a["pair"]]
                kb = [[QR.split_pair(p, F, 1, 0, 0) for p in row] for row in b["pair"]]
                assert [[s and (QR.SPHERE, *s[1:]) for s in row] for row in ka] == kb and any(s for row in ka for s in row)
                assert all(s is None or s[0] == QR.CAPSULE for row in ka for s in row)


# ---- 5: pair indices -------------------------------------------------------------------------------------------------------------

def test_pair_indices_decode_to_the_planted_frame_and_capsule(driver, groups, tmp_path):
    from riemannian_motion_policies_amd import engine as E
    seen = set()
    for c in groups:
        F, K, P, C = QS.counts(c)
        d = run_capsules(driver, tmp_path, c)
        pr = QR.pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["q"])
        frames = CR.capsule_frames(c["caps"])
        for r, row in enumerate(d["pair"]):
            for p in row[row >= 0]:
                kind, f, rec, e = E.contact_pair_split(p, F, K, P, C)
                assert (kind, f, rec, e) == QR.split_pair(p, F, K, P, C)
                assert f in frames and rec < {E.CONTACT_KIND_SPHERE: K, E.CONTACT_KIND_PLANE: P, E.CONTACT_KIND_CAPSULE: C}[kind]
                k = list(pr["idx"]).index(int(p))          # the pair the index names is within d_act in fp64 (to rounding)
                assert pr["gap"][r, k] <= D_ACT + 1e-5
                seen.add(kind)
        if c["group"] in ("post", "cap", "tip", "point", "parallel", "buried", "crossing"):
            want = (E.CONTACT_KIND_CAPSULE, *c["planted"], 0)
            assert all(want in {E.contact_pair_split(p, F, K, P, C) for p in row} for row in d["pair"]), c["label"]
    assert seen == {0, 1, 2}
    assert E.contact_pair_split(-1, 3, 4, 2, 5) is None and E.contact_pair_split(3 * 4 + 2 * 3 * 2 + 2 * 5 + 4, 3, 4, 2, 5) == (2, 2, 4, 0)
    assert E.contact_pair_split(3 * 4 + 2 * (2 * 2 + 1) + 1, 3, 4, 2, 5) == (1, 2, 1, 1) == E.contact_pair_split(3 * 4 + 2 * (2 * 2 + 1) + 1, 3, 4, 2)
    with pytest.raises(ValueError):
        E.contact_pair_split(3 * 4 + 2 * 3 * 2 + 3 * 5, 3, 4, 2, 5)
    with pytest.raises(ValueError):
        E.contact_pair_split(3 * 4 + 2 * 3 * 2, 3, 4, 2)          # (the default C = 0: as before the capsules)


def test_pair_split_macros_of_the_header(tmp_path):
    """The RMP2_CONTACT_PAIR_* macros with the capsule kind, compiled as C, against the reference's split over a whole range."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    src = tmp_path / "split.c"
    src.write_text('#include <stdio.h>\n#include "rmp2.h"\nint main(void) {\n  const int F = 5, K = 3, P = 2, C = 4;\n'
                   '  for (int32_t p = 0; p < F * K + 2 * F * P + F * C; ++p) {\n'
                   '    const int kind = RMP2_CONTACT_PAIR_KIND3(p, F, K, P);\n'
                   '    if (kind == RMP2_CONTACT_KIND_CAPSULE)\n'
                   '      printf("%d %d %d %d 0\\n", p, kind, RMP2_CONTACT_PAIR_CAPSULE_FRAME(p, F, K, P, C), RMP2_CONTACT_PAIR_CAPSULE_RECORD(p, F, K, P, C));\n'
                   '    else\n'
                   '      printf("%d %d %d %d %d\\n", p, kind, RMP2_CONTACT_PAIR_FRAME(p, F, K, P), RMP2_CONTACT_PAIR_RECORD(p, F, K, P),\n'
                   '             RMP2_CONTACT_PAIR_END(p, F, K));\n  }\n  return 0;\n}\n')
    exe = tmp_path / "split"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(lines) == 5 * 3 + 2 * 5 * 2 + 5 * 4
    for p, k, f, r, e in lines:
        assert (k, f, r, e) == QR.split_pair(p, 5, 3, 2, 4)
    assert lines[35][1:] == [2, 0, 0, 0] and lines[34][1:] == [1, 4, 1, 1] and lines[-1][1:] == [2, 4, 3, 0]


def tie_case(groups, n_small, sphere=True):
    """tests/test_contact_planes_host.tie_case with a capsule: the two-joint robot at q = 0 with the tip sphere as its only link
    capsule; n_small planes with normal +y at smaller gaps; then a sphere below the tip, a plane and a vertical capsule through
    the sphere's centre, all three at the gap 0.09375 - r_tip to the bit."""
    c = by(QS.for_robot(groups, "two_joint"), "post")[0]
    caps = np.zeros_like(c["caps"])
    caps[2] = c["caps"][2]
    q = np.zeros((1, 2), np.float32)
    tip = CR.poses(c["t"], q, np.float32)[1][2][0]
    assert tip[1] == 0 and tip[2] * 8 == round(tip[2] * 8) and (caps[2, 0:3] == caps[2, 4:7]).all()
    c = dict(c, caps=caps, q=q, qd=np.zeros((1, 2), np.float32), u=np.zeros((1, 2), np.float32),
             spheres=np.array([[tip[0], -0.21875, tip[2], 0.125]], np.float32))
    tip = c["spheres"][0, :3]
    planes = np.array([[0.0, 1.0, 0.0, -0.09375 + (k + 1) / 512.0] for k in range(n_small)] + [[0.0, 1.0, 0.0, -0.09375]], np.float32)
    capsules = np.array([[tip[0], tip[1], tip[2] - 0.25, 0.125, tip[0], tip[1], tip[2] + 0.25, 0.0]], np.float32)
    return dict(c, planes=planes, capsules=capsules, spheres=c["spheres"] if sphere else NONE4)


def test_a_sphere_a_plane_and_a_capsule_at_equal_gap_tie_in_that_order(driver, groups, tmp_path):
    for n_small, sphere, kept_kinds in ((6, True, [QR.SPHERE, QR.PLANE]), (7, True, [QR.SPHERE]), (7, False, [QR.PLANE])):
        c = tie_case(groups, n_small, sphere)
        F, K, P, C = QS.counts(c)
        assert (F, P, C) == (3, n_small + 1, 1)
        pr = QR.pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["q"], np.float32)
        gaps = dict(zip(pr["idx"].tolist(), pr["gap"][0].tolist()))
        tied = ([2 * K + 0] if sphere else []) + [PR.pair_index(F, K, P, 2, n_small, 0), QR.pair_index(F, K, P, C, 2, 0)]
        assert len({gaps[i] for i in tied}) == 1 and 0 < gaps[tied[0]] <= D_ACT and tied == sorted(tied), (gaps, tied)
        small = [PR.pair_index(F, K, P, 2, k, 0) for k in range(n_small)]
        want = sorted(small + tied[:8 - n_small])
        assert [QR.split_pair(p, F, K, P, C)[0] for p in tied[:8 - n_small]] == kept_kinds
        ref = QR.substep(c["t"], c["inert"], c["caps"], c["spheres"], c["planes"], c["capsules"], D_ACT, c["q"], c["qd"], c["u"],
                         c["drive"], DT, c["lim"], c["limits"], c["g"], envelope=True)      # (the tie is one of fp32 values)
        for lists in (None, whole_lists(1, K)):
            d = run_capsules(driver, tmp_path, c, lists=lists)
            assert d["status"][0] & CR.OVERFLOW and ref["overflow"][0]
            assert sorted(d["pair"][0]) == want == sorted(ref["pair"][0]), (d["pair"][0], ref["pair"][0], want)


# ---- 6: poisoning ------------------------------------------------------------------------------------------------------------------

def test_a_non_finite_capsule_poisons_the_fleet_and_a_nan_state_only_its_robot(driver, groups, tmp_path):
    for c in by(groups, "post") + by(groups, "mixed") + by(groups, "far"):
        good = run_capsules(driver, tmp_path, c)
        C = len(c["capsules"])
        for value, (p, k) in ((np.nan, (0, 3)), (np.inf, (0, 1)), (-np.inf, (C - 1, 6)), (np.nan, (C - 1, 7))):
            capsules = c["capsules"].copy()
            capsules[p, k] = value
            for lists in (None, whole_lists(len(c["q"]), len(c["spheres"]))):
                d = run_capsules(driver, tmp_path, c, capsules=capsules, lists=lists)
                for key in FLOATS:
                    assert np.isnan(d[key]).all(), (c["label"], key)
                assert (d["pair"] == -1).all()
        q = c["q"].copy()
        q[1, 0] = np.nan
        d = run_capsules(driver, tmp_path, c, q=q)
        others = np.arange(len(q)) != 1
        for key in FLOATS:
            assert np.isnan(d[key][1]).all() and S._bits_equal(d[key][others], good[key][others]), (c["label"], key)
        assert (d["pair"][1] == -1).all() and np.array_equal(d["pair"][others], good["pair"][others])


# ---- 7: under the host sanitizers (a stand-alone program; the capsule buffer holds exactly C records) ------------------------------

def test_driver_under_the_host_sanitizers_equals_the_plain_build(driver, driver_san, groups, tmp_path):
    for c in QS.for_robot(groups, "two_joint") + by(groups, "overflow") + by(groups, "mixed") + [tie_case(groups, 6)]:
        for lists in (None, whole_lists(len(c["q"]), len(c["spheres"]))):
            same(run_capsules(driver_san, tmp_path, c, substeps=2, lists=lists),
                 run_capsules(driver, tmp_path, c, substeps=2, lists=lists), c["label"])
    c = by(groups, "post")[0]
    run_capsules(driver_san, tmp_path, c, planes=NONE4, spheres=NONE4, capsules=NONE8)


# ---- 8: the interface --------------------------------------------------------------------------------------------------------------

def test_symbol_declared_and_bound_with_its_constants(hip_lib):
    import ctypes as C
    lib = C.CDLL(hip_lib)
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    assert re.search(r"\bint rmp2_dynamics_step_contacts_capsules\(", hdr) and hasattr(lib, "rmp2_dynamics_step_contacts_capsules")
    assert "#define RMP2_MAX_OBSTACLE_CAPSULES 32" in hdr and "#define RMP2_CONTACT_KIND_CAPSULE 2" in hdr
    assert "#define RMP2_CONTACT_PAIR_CAPSULE_FRAME(" in hdr and "#define RMP2_CONTACT_PAIR_FRAME(" in hdr
    assert re.search(r"#define RMP2_ABI_VERSION (\d+)", hdr).group(1) == "5" and lib.rmp2_abi_version() == 5
    from riemannian_motion_policies_amd import _native, engine as E, urdf as U
    assert E.MAX_OBSTACLE_CAPSULES == MAX_CAPSULES == U.MAX_OBSTACLE_CAPSULES and E.CONTACT_KIND_CAPSULE == 2 == QR.CAPSULE
    assert len(_native.lib().rmp2_dynamics_step_contacts_capsules.argtypes) == 28
    args = [None] * 28
    for k, v in ((4, 0), (9, 0), (13, 0), (15, 0), (16, 0.0), (17, 0.0), (18, 0), (26, 0)):
        args[k] = v
    assert _native.lib().rmp2_dynamics_step_contacts_capsules(*args) == -1          # (no handle: RMP2_ERR_INVALID_ARGUMENT)
    import __graft_entry__ as g
    names = [u[0] for u in g.HIP_UNITS]
    assert "rmp2_contacts_l0_capsules" in names and "rmp2_contacts_l1_capsules" in names and len(names) == len(set(names))


def test_urdf_capsule_obstacles_converts_and_refuses():
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    rows = Cf.sample_capsules(np.random.default_rng(3), 7).astype(np.float64)
    rows[:, 7] = 5.0
    out = U.capsule_obstacles(rows)
    assert out.dtype == np.float32 and out.shape == (7, 8) and out.flags["C_CONTIGUOUS"] and (out[:, 7] == 0).all()
    assert np.array_equal(out[:, :7], rows[:, :7].astype(np.float32)) and np.array_equal(U.capsule_obstacles(rows[:, :7]), out)
    assert U.capsule_obstacles([]).shape == (0, 8) and len(U.capsule_obstacles(np.tile(rows[:1], (32, 1)))) == 32
    bad = rows.copy()
    bad[2, 3] = -0.01
    nan = rows.copy()
    nan[1, 5] = np.nan
    for b, msg in ((bad, "negative radius"), (nan, "not finite"), (np.tile(rows[:1], (33, 1)), "at most 32"), (rows[:, :6], "rows"),
                   ([[0, 0, 0, np.inf, 0, 0, 1]], "not finite")):
        with pytest.raises(ValueError, match=msg):
            U.capsule_obstacles(b)


def test_cylinders_as_capsules_meet_their_stated_bounds():
    """covering: contains the cylinder, overshoots by at most r;  inscribed (h >= r): inside the cylinder, misses it by at most
    (sqrt 2 - 1) r -- both against configs.point_cylinder_np's signed distance on random points, in numpy."""
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    rng = np.random.default_rng(11)
    cyl = np.concatenate([Cf.sample_cylinders(rng, 7), Cf.EXP06_CYLINDERS, [Cf.cylinder_record([0.1, 0.2, 0.3], [0.3, 0.2, 0.1], 0.2, 0.1)]])

    def capsule_sd(p, rec):
        a, r, b = rec[:, None, 0:3].astype(np.float64), rec[:, None, 3].astype(np.float64), rec[:, None, 4:7].astype(np.float64)
        d = b - a
        dd = (d * d).sum(-1)
        t = np.clip(((p - a) * d).sum(-1) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
        return np.linalg.norm(p - (a + t[..., None] * d), axis=-1) - r

    c, r, h = cyl[:, None, 0:3].astype(np.float64), cyl[:, 3].astype(np.float64), cyl[:, 7].astype(np.float64)
    p = c + rng.normal(size=(len(cyl), 4000, 3)) * (0.6 * (r + h))[:, None, None]
    sd_cyl = Cf.point_cylinder_np(p, cyl[:, None, :])[2]
    eps = 1e-6
    cover, inner = U.cylinders_as_capsules(cyl), U.cylinders_as_capsules(cyl, "inscribed")
    assert cover.shape == inner.shape == (len(cyl), 8) and cover.dtype == np.float32
    sd = capsule_sd(p, cover)
    assert (sd <= sd_cyl + eps).all() and (sd >= sd_cyl - r[:, None] - eps).all()          # contains; by at most r
    tall = h >= r
    assert tall.sum() >= 14 and not tall.all()
    sd = capsule_sd(p, inner)
    assert (sd[tall] >= sd_cyl[tall] - eps).all() and (sd[tall] <= sd_cyl[tall] + ((np.sqrt(2) - 1) * r[tall])[:, None] + eps).all()
    flat = np.nonzero(~tall)[0][0]
    assert (inner[flat, 0:3] == inner[flat, 4:7]).all() and inner[flat, 3] == cyl[flat, 3]          # (h < r: the sphere of radius r)
    assert np.allclose(cover[:, 0:3], cyl[:, 0:3] - cyl[:, 7:8] * cyl[:, 4:7], atol=1e-6)
    assert U.cylinders_as_capsules([]).shape == (0, 8)
    for bad, msg in (("inside", "mode"),):
        with pytest.raises(ValueError, match=msg):
            U.cylinders_as_capsules(cyl, bad)
    zero = cyl.copy()
    zero[0, 4:7] = 0
    with pytest.raises(ValueError, match="zero axis"):
        U.cylinders_as_capsules(zero)

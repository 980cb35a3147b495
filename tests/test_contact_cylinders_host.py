"""Exact flat-capped cylinder obstacles in the contact step (include/rmp2.h rmp2_dynamics_step_contacts_cylinders) on the host: the
scenes of tests/contact_cylinders_scene.py meet their stated conditions; the reference pinned against a brute-force scan; the fp32
envelope that the bounds are taken from; the cylinder form of the device routine of rmp2_contacts.h run on the CPU through
tests/contacts_driver.cpp (also under the host sanitizers, as a stand-alone program, and built without the cull) against
the fp64 reference of tests/contact_cylinders_reference.py, and BIT FOR BIT against the self, capsules and stops drivers where the
contract promises it; pair indices, the five-way tie, the header, the bindings and urdf.cylinder_obstacles.  No GPU.

The bounds are those of tests/test_contacts_host.py with the K's of these scenes by the same rule: K = 4 x the worst ratio of the
fp32 ENVELOPE against the fp64 reference over the catalogue's three robots, rounded up to one significant figure
(MEASURED_CYLINDERS -> K_CYLINDERS, fixed here from the CPU run before any GPU run; test_envelope_backs_the_bounds measures them
again).  Robots held to the bounds: the kept rule of DESIGN 4.12 (envelope uncapped and within K / 4)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contact_cylinders_reference as YR
import contact_cylinders_scene as YS
import contact_self_reference as SR
import contacts_reference as CR
import test_contact_capsules_host as QH
import test_contact_planes_host as PH
import test_contact_self_host as SH
import test_contacts_host as S
from test_contacts_host import D_ACT, DT, ROOT

MEASURED_CYLINDERS = dict(res=0.03194, vel=5.369, force=5.465, step=29.45, gap=0.07286)      # the envelope's worst ratios
K_CYLINDERS = dict(res=0.2, vel=30.0, force=30.0, step=200.0, gap=0.3)
FLOATS = PH.FLOATS
SAN = PH.SAN
NONE4, NONE8, NONE2 = YS.NONE4, YS.NONE8, YS.NONE2
NONE_CYL = np.zeros((0, 8), np.float32)
whole_lists, same, by = PH.whole_lists, PH.same, PH.by


@pytest.fixture(scope="module")
def groups(golden_dir, tmp_path_factory):
    return YS.catalogue(golden_dir, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def slot_groups(tmp_path_factory):
    return YS.slot_catalogue(tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver")


@pytest.fixture(scope="module")
def driver_no_cull(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_no_cull", ("-DRMP2_CYLINDER_NO_CULL",))


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_san", SAN)


@pytest.fixture(scope="module")
def self_driver(driver):
    return driver


@pytest.fixture(scope="module")
def stops_driver(tmp_path_factory):
    return S._build(tmp_path_factory, "joint_stops_driver.cpp", "joint_stops_driver")


@pytest.fixture(scope="module")
def capsules_driver(driver):
    return driver


def run_cyl(exe, tmp_path, c, substeps=1, lists=None, d_act=D_ACT, flag=1, **over):
    """The cylinders driver on a group (fields replaced by the keywords): contacts_reference.read_driver_output's dict.  A
    sanitizer report fails it: exit status 0 and nothing on stderr."""
    YR.write_driver_input(str(tmp_path / "in.bin"), c, substeps, DT, d_act, lists=lists, flag=flag, **over)
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "cylinders"], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    B = len(over["q"]) if over.get("q") is not None else len(c["q"])
    return CR.read_driver_output(str(tmp_path / "out.bin"), B, c["t"].n_dof)


# ---- 1: the reference and the scenes ----------------------------------------------------------------------------------------------

def test_point_cylinder_restatement_equals_the_package_form():
    from riemannian_motion_policies_amd import configs as Cf
    rng = np.random.default_rng(3)
    cyl = np.concatenate([Cf.EXP06_CYLINDERS, Cf.sample_cylinders(rng, 5)]).astype(np.float64)
    cyl[:, 4:7] /= np.linalg.norm(cyl[:, 4:7], axis=1)[:, None]
    for rec in cyl:
        P = rec[0:3] + rng.uniform(-0.4, 0.4, (400, 3))
        Y, n, sd = YR.point_cylinder(P, rec)
        Y2, n2, sd2 = Cf.point_cylinder_np(P, rec[None])
        assert np.abs(sd - sd2).max() < 1e-12 and np.abs(Y - Y2).max() < 1e-12 and np.abs(n - n2).max() < 1e-9
        on = rec[0:3] + rng.uniform(-1.5, 1.5, (8, 1)) * rec[7] * rec[4:7]      # on the axis: the fixed perpendicular
        Y, n, sd = YR.point_cylinder(on, rec)
        assert np.isfinite(Y).all() and np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12


def test_reference_gap_is_the_brute_force_minimum_on_every_planted_pair(groups, slot_groups):
    seen = 0
    for c in groups + slot_groups:
        if c["planted"] is None:
            continue
        f, y = c["planted"]
        A, D, rf = YS.QS.segments(c, c["q"][0].astype(np.float64), c["caps"])[f]
        sd, s = YR.scan_minimum(A, D, c["cylinders"][y].astype(np.float64))
        d = YS.planted_detail(c)
        assert abs((sd - rf) - d["gap"]) < 1e-9, (c["label"], sd - rf, d["gap"], s, d["s"])
        seen += 1
    assert seen >= 40


def test_scenes_meet_their_stated_conditions(groups, slot_groups):
    from riemannian_motion_policies_amd import urdf as U
    names = YS.robots(groups)
    assert names[:2] == ["two_joint", "panda"] and len(names) == 3
    slot_names = YS.robots(slot_groups)
    assert [int(YS.for_robot(slot_groups, n)[0]["t"].depth_first_schedule()[3]) for n in slot_names] == [0, 2]
    for name in names:
        assert [c["group"] for c in YS.for_robot(groups, name)] == list(YS.GROUPS), name
    for name in slot_names:
        assert [c["group"] for c in YS.for_robot(slot_groups, name)] == list(YS.GROUPS), name
    for c in groups + slot_groups:
        ref, what, g = c["ref"], c["label"], c["group"]
        F, K, P, C, Y = YS.counts(c)
        assert not ref["capped"].any() and not c["env"]["capped"].any(), what
        assert np.abs(np.linalg.norm(c["cylinders"][:, 4:7].astype(np.float64), axis=1) - 1).max() < 1e-6, what
        kinds = YS.kinds(c)
        if c["planted"] is None:
            continue
        f, y = c["planted"]
        d, d32 = YS.planted_detail(c), YS.planted_detail(c, np.float32)
        want = (YR.CYLINDER, f, y, 0)
        rf = float(c["caps"][f, 3])
        if g in YS.PUSHED + ("tip", "base", "disc"):
            assert YS.planted_active(c).all() and abs(d["gap"] - YS.GAP) < 2e-6, (what, d["gap"])
        if g in ("side", "buried", "pierced_side"):
            assert 0.2 < d["s"] < 0.8 and abs(d["a"]) < 0.1 * YS.CYL_H and abs(d["nu"]) < 1e-3, (what, d)
        if g in ("cap", "disc", "on_axis", "pierced_cap"):
            assert d["s"] in (0.0, 1.0) and d32["s"] == d["s"] and abs(abs(d["nu"]) - 1) < 1e-6, (what, d["s"], d["nu"])
        if g == "disc":
            assert c["cylinders"][y, 7] == 0, what
        if g == "rim":
            assert 0.2 < d["s"] < 0.8 and abs(abs(d["nu"]) - np.sqrt(0.5)) < 1e-3, (what, d["s"], d["nu"])      # (a mixed normal)
        if g == "tip":
            assert d["s"] == 1.0 == d32["s"], what
        if g == "base":
            assert d["s"] == 0.0 == d32["s"], what
        if g in YS.FLAT:
            assert c["exact"] or c["name"] not in ("two_joint", "panda"), what
            if c["exact"]:      # flat to the bit: the slope is exactly 0 at s = 0 in both arithmetics, the choice is the A end
                assert d["s"] == 0.0 == d32["s"], (what, d["s"], d32["s"])
                A, D, _ = YS.QS.segments(c, c["q"][0].astype(np.float64), c["caps"])[f]
                for s in (0.0, 0.25, 1.0):
                    assert float(YR.point_cylinder((A + s * D)[None], c["cylinders"][y].astype(np.float64))[1][0] @ D) == 0.0, what
            else:      # flat to rounding: at rest
                assert not c["qd"].any() and not c["u"].any() and c["lim"] is None, what
            assert 0 < d["gap"] <= D_ACT, what
        if g == "on_axis":
            w = d["X"] - c["cylinders"][y, 0:3].astype(np.float64)
            rho = np.linalg.norm(w - (w @ c["cylinders"][y, 4:7]) * c["cylinders"][y, 4:7])
            assert (c["exact"] or c["name"] not in ("two_joint", "panda")) and (rho == 0.0 if c["exact"] else rho < 1e-6), (what, rho)
        if g in ("pierced_side", "pierced_cap"):
            assert d["sd"] < -0.009 and d32["sd"] < -0.009 and abs(d["gap"] + 0.01 + rf) < 2e-6, (what, d["sd"])
            assert all(want in row for row in kinds), what
        if g == "buried":
            assert d["gap"] < -0.019 and d["sd"] > 0 and all(want in row for row in kinds), what
        if g == "mixed":
            assert all({k[0] for k in row} == {0, 1, 2, 3, 4} for row in kinds), (what, kinds)
        if g == "overflow":
            assert ref["overflow"].all() and (ref["n_cand"] == 8).all() and Y == 9, what
            assert all(sum(k[0] == YR.CYLINDER for k in row) == 8 for row in kinds), what      # (kept; the ninth is dropped)
        else:
            assert not ref["overflow"].any(), what
        if g == "graze":      # gaps on either side of d_act, L on either side of the cull's threshold, all within the margin
            q32 = c["q"][0]
            lm = [YS.cull_bound(c, q32, c["cylinders"])[(f, k)] for k in range(Y)]
            gaps = [YS.pair_detail(c, q32.astype(np.float64), c["cylinders"][k], f, c["caps"])["gap"] for k in range(Y)]
            # L within m of the threshold d_act + m; the record below d_act 4e-6 further: L <= g < d_act (8e-6 with fp32's rounding)
            assert min(gaps) < D_ACT < sorted(gaps)[1] and all(abs(L - (D_ACT + m)) <= m + (8e-6 if k == 0 else 0.0) for k, (L, m) in enumerate(lm)), (what, gaps, lm)
            assert any(L > D_ACT + m for L, m in lm) and any(L < D_ACT + m for L, m in lm), (what, lm)
            assert all(abs(L - gp) < 5e-6 for (L, m), gp in zip(lm, gaps)), (what, lm, gaps)      # (the diagonal: L is the gap)
        if g in ("cap", "rim"):
            # what the feature is for: the exact gap is neither the covering nor the inscribed capsule's, by more than 10 x the
            # gap bracket (1e-6 + dt x velocity bracket x max(1, |J|_1))
            _, jn = YR.linearised_gaps(c, ref["qd"], ref["pair"], DT)
            bracket = float(YS.gap_bracket(c, jn).max())
            for mode in ("covering", "inscribed"):
                oc = U.cylinders_as_capsules(c["cylinders"][y:y + 1], mode)
                gc = float(SR.QR.capsule_rows(c["t"], c["caps"], oc, 0, 0, c["q"][:1].astype(np.float64))["gap"][0, list(CR.capsule_frames(c["caps"])).index(f)])
                assert abs(gc - d["gap"]) > 10 * bracket, (what, mode, gc, d["gap"], bracket)
    far = by(groups + slot_groups, "far")
    assert len(far) == 5
    for c in far:
        assert all(k[0] != YR.CYLINDER for row in YS.kinds(c) for k in row) and len(c["cylinders"]) == 7, c["label"]
        assert all(L > D_ACT + m for L, m in YS.cull_bound(c, c["q"][0], c["cylinders"]).values()), c["label"]      # (all culled)


# ---- 2: the envelope -----------------------------------------------------------------------------------------------------------

def envelope_ratios(groups):
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0, gap=0.0)
    for c in groups:
        ok = ~np.asarray(c["env"]["capped"], bool) & ~np.asarray(c["ref"]["capped"], bool)
        assert np.array_equal(np.sort(c["env"]["pair"], 1), np.sort(c["ref"]["pair"], 1)), c["label"]      # (the same candidates in fp32)
        r = YS.per_robot_ratios(c, c["env"])
        for k in ("res", "vel", "force", "gap"):
            worst[k] = max(worst[k], float(r[k][ok].max()))
        ok &= ~np.asarray(c["env_step"]["capped"], bool) & ~np.asarray(c["ref_step"]["capped"], bool)
        if ok.any():
            worst["step"] = max(worst["step"], float(YS.step_ratios(c, c["env_step"])[ok].max()))
    return worst


def test_envelope_backs_the_bounds_and_keeps_the_robots(groups, slot_groups):
    worst = envelope_ratios(groups)
    print("envelope worst ratios", worst)
    print("envelope worst ratios on the slot trees", envelope_ratios(slot_groups))
    for k, K in K_CYLINDERS.items():
        assert np.isclose(K, S._round_up_1sf(4 * MEASURED_CYLINDERS[k])), (k, K, MEASURED_CYLINDERS[k])
        assert 4 * worst[k] <= K, (k, worst[k], K)
    for name in YS.robots(groups) + YS.robots(slot_groups):
        gs = YS.for_robot(groups + slot_groups, name)
        keep = np.concatenate([YS.kept(c, K_CYLINDERS) for c in gs]), np.concatenate([YS.kept_step(c, K_CYLINDERS) for c in gs])
        print(name, "kept", keep[0].mean(), "kept over the step", keep[1].mean())
        assert keep[0].mean() >= 0.9 and keep[1].mean() >= 0.9, (name, keep[0].mean(), keep[1].mean())


# ---- 3: the device routine on the CPU against the reference -------------------------------------------------------------------

def test_device_routine_on_the_cpu_against_the_reference(driver, groups, slot_groups, tmp_path):
    worst, kept = {}, 0
    groups = groups + slot_groups
    for c in groups:
        B, K = len(c["q"]), len(c["spheres"])
        d = run_cyl(driver, tmp_path, c)
        kept += YS.check_group(c, d, K_CYLINDERS, c["label"], worst)
        dl = run_cyl(driver, tmp_path, c, lists=whole_lists(B, K))
        YS.check_group(c, dl, K_CYLINDERS, c["label"] + "-lists", worst)
        for lists in (None, whole_lists(B, K)):
            d4 = run_cyl(driver, tmp_path, c, substeps=YS.STEP_SUBSTEPS, lists=lists)
            YS.check_group_step(c, d4, K_CYLINDERS, c["label"] + ("-lists" if lists else ""), worst)
        if c["group"] in YS.PUSHED:
            assert YS.planted_active(c, d).all() and ((d["pair"] >= 0).sum(1) == 1).all(), c["label"]
    print("CPU driver worst ratios", worst, "kept", kept)
    assert kept >= 0.9 * sum(len(c["q"]) for c in groups)
    for k, K in K_CYLINDERS.items():
        assert worst[k] <= K, (k, worst[k], K)


# ---- 4: bit for bit -------------------------------------------------------------------------------------------------------------

def test_no_cylinders_and_far_cylinders_are_the_existing_calls_bit_for_bit(driver, self_driver, capsules_driver, groups, slot_groups,
                                                                           tmp_path):
    """Y = 0 or `far` with the flag on: the self driver; with the flag off: the capsules driver."""
    seen = 0
    for c in by(groups, "far") + by(groups, "mixed"):
        B, K = len(c["q"]), len(c["spheres"])
        for substeps in (1, 3):
            for lists in (None, whole_lists(B, K)):
                want_self = SH.run_self(self_driver, tmp_path, c, substeps=substeps, lists=lists)
                want_caps = QH.run_capsules(capsules_driver, tmp_path, c, substeps=substeps, lists=lists)
                same(run_cyl(driver, tmp_path, c, substeps=substeps, lists=lists, cylinders=NONE_CYL), want_self, (c["label"], "Y = 0, flag 1"))
                same(run_cyl(driver, tmp_path, c, substeps=substeps, lists=lists, cylinders=NONE_CYL, flag=0), want_caps, (c["label"], "Y = 0, flag 0"))
                if c["group"] == "far":
                    same(run_cyl(driver, tmp_path, c, substeps=substeps, lists=lists), want_self, (c["label"], "far, flag 1"))
                    same(run_cyl(driver, tmp_path, c, substeps=substeps, lists=lists, flag=0), want_caps, (c["label"], "far, flag 0"))
                seen += int((want_self["pair"] >= 0).sum())
    assert seen >= 100


def test_nothing_at_all_is_the_stops_step_bit_for_bit(driver, stops_driver, groups, slot_groups, tmp_path):
    import test_joint_stops_host as JH
    for c in by(groups + slot_groups, "side") + by(groups, "mixed"):
        for substeps in (1, 3):
            s = JH.run_driver(stops_driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"],
                              substeps, c["g"])
            for lists in (None, whole_lists(len(c["q"]), 0)):
                for flag in (0, 1):          # (flag 1 with no pairs on the handle)
                    d = run_cyl(driver, tmp_path, c, substeps=substeps, lists=lists, flag=flag, spheres=NONE4, planes=NONE4,
                                capsules=NONE8, pairs=NONE2, cylinders=NONE_CYL)
                    for k in ("q", "qd", "qdd", "tau", "stop"):
                        assert S._bits_equal(d[k], s[k]), (c["label"], k)
                    assert (d["status"] == s["status"]).all() and (d["contact"] == 0).all() and (d["lam"] == 0).all() and (d["pair"] == -1).all()


def test_cull_on_equals_cull_off_bit_for_bit(driver, driver_no_cull, groups, slot_groups, tmp_path):
    for c in groups + slot_groups:
        for substeps in (1, YS.STEP_SUBSTEPS):
            for lists in (None, whole_lists(len(c["q"]), len(c["spheres"]))):
                same(run_cyl(driver, tmp_path, c, substeps=substeps, lists=lists),
                     run_cyl(driver_no_cull, tmp_path, c, substeps=substeps, lists=lists), (c["label"], substeps))


# ---- 5: pair indices -------------------------------------------------------------------------------------------------------------

def test_pair_indices_decode_to_the_planted_frame_and_cylinder(driver, groups, slot_groups, tmp_path):
    from riemannian_motion_policies_amd import engine as E
    seen = set()
    for c in groups + slot_groups:
        F, K, P, C, Y = YS.counts(c)
        d = run_cyl(driver, tmp_path, c)
        for row in d["pair"]:
            for p in row[row >= 0]:
                got = E.contact_pair_split(p, F, K, P, C, self_pairs=True, cylinders=Y)
                assert got == YR.split_pair(p, F, K, P, C, Y), (c["label"], p)
                if got[0] != E.CONTACT_KIND_CYLINDER:
                    assert got == E.contact_pair_split(p, F, K, P, C, self_pairs=True)      # (the other kinds: as without cylinders)
                seen.add(got[0])
        if c["planted"] is not None and c["group"] != "graze":
            want = (E.CONTACT_KIND_CYLINDER, *c["planted"], 0)
            assert all(want in {E.contact_pair_split(p, F, K, P, C, self_pairs=True, cylinders=Y) for p in row} for row in d["pair"]), c["label"]
    assert seen == {0, 1, 2, 3, 4}
    base = 3 * 4 + 2 * 3 * 2 + 3 * 5 + 9
    assert E.contact_pair_split(base + 7 * 2 + 6, 3, 4, 2, 5, cylinders=7) == (4, 2, 6, 0)
    assert E.contact_pair_split(base - 1, 3, 4, 2, 5, self_pairs=True, cylinders=7) == (3, 2, 2, 0)
    with pytest.raises(ValueError):
        E.contact_pair_split(base + 21, 3, 4, 2, 5, cylinders=7)
    with pytest.raises(ValueError):
        E.contact_pair_split(base, 3, 4, 2, 5, self_pairs=True)          # (without cylinders=: as before)


def test_pair_split_macros_of_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    src = tmp_path / "split.c"
    src.write_text('#include <stdio.h>\n#include "rmp2.h"\nint main(void) {\n  const int F = 5, K = 3, P = 2, C = 4, Y = 6;\n'
                   '  if (RMP2_CONTACT_PAIR_CYLINDER_BASE(F, K, P, C) != F * K + 2 * F * P + F * C + F * F) return 1;\n'
                   '  for (int32_t p = 0; p < F * K + 2 * F * P + F * C + F * F + F * Y; ++p) {\n'
                   '    const int kind = RMP2_CONTACT_PAIR_KIND5(p, F, K, P, C);\n'
                   '    if (kind == RMP2_CONTACT_KIND_CYLINDER)\n'
                   '      printf("%d %d %d %d\\n", p, kind, RMP2_CONTACT_PAIR_CYLINDER_FRAME(p, F, K, P, C, Y), RMP2_CONTACT_PAIR_CYLINDER_RECORD(p, F, K, P, C, Y));\n'
                   '    else if (kind == RMP2_CONTACT_KIND_SELF)\n'
                   '      printf("%d %d %d %d\\n", p, kind, RMP2_CONTACT_PAIR_SELF_LINK(p, F, K, P, C), RMP2_CONTACT_PAIR_SELF_PARTNER(p, F, K, P, C));\n'
                   '    else\n      printf("%d %d -1 -1\\n", p, kind);\n  }\n  return 0;\n}\n')
    exe = tmp_path / "split"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(lines) == 15 + 20 + 20 + 25 + 30
    for p, k, f, r in lines:
        want = YR.split_pair(p, 5, 3, 2, 4, 6)
        assert k == want[0] and (k < 3 or (f, r) == want[1:3]), (p, k, f, r, want)
    assert lines[80][1:] == [4, 0, 0] and lines[79][1:] == [3, 4, 4] and lines[-1][1:] == [4, 4, 5]


def tie_case(self_groups, n_small):
    """tests/test_contact_self_host.tie_case (on contact_self_scene's catalogue, self_groups) with a cylinder: its sphere, plane, obstacle capsule and self pair at the gap 0.09375 -
    r_tip below the tip to the bit, and a cylinder with its axis along +y through the tip whose flat end lies in the tied plane
    y = -0.09375 (half height 1/8, radius 1/4, centre at y = -0.21875: every number on a grid): sd = 0.21875 - 0.125 to the bit."""
    c = SH.tie_case(self_groups, n_small)
    tip = c["spheres"][0, :3]
    cyl = np.array([[tip[0], -0.21875, tip[2], 0.25, 0.0, 1.0, 0.0, 0.125]], np.float32)
    return dict(c, cylinders=cyl)


@pytest.fixture(scope="module")
def self_groups(golden_dir, tmp_path_factory):
    """contact_self_scene's catalogue, which test_contact_self_host.tie_case builds on."""
    return YS.SS.catalogue(golden_dir, tmp_path_factory.mktemp("self_trees"))


def test_the_five_kinds_at_equal_gap_tie_in_index_order(driver, self_groups, tmp_path):
    for n_small, kept_kinds in ((3, [0, 1, 2, 3, 4]), (4, [0, 1, 2, 3]), (5, [0, 1, 2])):
        c = tie_case(self_groups, n_small)
        F, K, P, C, Y = YS.counts(c)
        pr = YR.pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["pairs"], c["cylinders"], c["q"], np.float32)
        gaps = dict(zip(pr["idx"].tolist(), pr["gap"][0].tolist()))
        tied = [2 * K + 0, SR.QR.PR.pair_index(F, K, P, 2, n_small, 0), SR.QR.pair_index(F, K, P, C, 2, 0), SR.pair_index(F, K, P, C, 2, 0),
                YR.pair_index(F, K, P, C, Y, 2, 0)]
        assert len({gaps[i] for i in tied}) == 1 and 0 < gaps[tied[0]] <= D_ACT and tied == sorted(tied), (gaps, tied)
        small = [SR.QR.PR.pair_index(F, K, P, 2, k, 0) for k in range(n_small)]
        assert sorted(i for i, g in gaps.items() if g <= D_ACT) == sorted(small + tied), gaps
        want = sorted(small + tied[:8 - n_small])
        assert [YR.split_pair(p, F, K, P, C, Y)[0] for p in tied[:8 - n_small]] == kept_kinds
        for lists in (None, whole_lists(1, K)):
            d = run_cyl(driver, tmp_path, c, lists=lists)
            assert bool(d["status"][0] & CR.OVERFLOW) == (n_small > 3)
            assert sorted(d["pair"][0]) == want, (d["pair"][0], want)


# ---- 6: poisoning and the sanitizers ----------------------------------------------------------------------------------------------

def test_a_non_finite_cylinder_poisons_the_fleet_and_a_nan_state_only_its_robot(driver, groups, tmp_path):
    for c in by(groups, "side") + by(groups, "far"):
        good = run_cyl(driver, tmp_path, c)
        for word in range(8):
            for bad in (np.nan, np.inf):
                cyl = c["cylinders"].copy()
                cyl[-1, word] = bad
                d = run_cyl(driver, tmp_path, c, cylinders=cyl)
                for k in FLOATS:
                    assert np.isnan(d[k]).all(), (c["label"], word, k)
                assert (d["pair"] == -1).all()
        q = c["q"].copy()
        q[1, 0] = np.nan
        d = run_cyl(driver, tmp_path, c, q=q)
        others = np.arange(len(q)) != 1
        for k in FLOATS:
            assert np.isnan(d[k][1]).all() and S._bits_equal(d[k][others], good[k][others]), (c["label"], k)


def test_driver_under_the_host_sanitizers_equals_the_plain_build(driver, driver_san, groups, self_groups, tmp_path):
    for c in YS.for_robot(groups, "two_joint") + by(groups, "overflow") + by(groups, "mixed") + by(groups, "graze") + [tie_case(self_groups, 4)]:
        for lists in (None, whole_lists(len(c["q"]), len(c["spheres"]))):
            same(run_cyl(driver_san, tmp_path, c, substeps=2, lists=lists), run_cyl(driver, tmp_path, c, substeps=2, lists=lists), c["label"])
    c = by(groups, "far")[1]
    run_cyl(driver_san, tmp_path, c, substeps=2, flag=0)
    run_cyl(driver_san, tmp_path, dict(c, pairs=NONE2), planes=NONE4, spheres=NONE4, capsules=NONE8, cylinders=NONE_CYL)


# ---- 7: the interface --------------------------------------------------------------------------------------------------------------

def test_urdf_cylinder_obstacles_converts_and_refuses():
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    out = U.cylinder_obstacles(Cf.EXP06_CYLINDERS)
    assert out.dtype == np.float32 and out.shape == (7, 8) and np.abs(out - Cf.EXP06_CYLINDERS).max() < 1e-6
    rows = Cf.EXP06_CYLINDERS.astype(np.float64).copy()
    rows[:, 4:7] *= 3.0
    got = U.cylinder_obstacles(rows)
    assert np.abs(np.linalg.norm(got[:, 4:7].astype(np.float64), axis=1) - 1).max() < 1e-7 and np.abs(got - out).max() < 1e-6
    assert U.cylinder_obstacles([]).shape == (0, 8) and U.cylinder_obstacles(np.tile(rows[:1], (32, 1))).shape == (32, 8)
    assert U.cylinder_obstacles([[0, 0, 0, 0.1, 0, 0, 1, 0.0]])[0, 7] == 0          # (a disc)
    for bad, msg in ((np.tile(rows[:1], (33, 1)), "at most 32"), (rows[:, :7], "shape"), (rows[0], "shape"),
                     ([[0, 0, 0, 0.1, 0, 0, 0, 0.1]], "zero axis"), ([[0, 0, 0, 0.0, 0, 0, 1, 0.1]], "radius <= 0"),
                     ([[0, 0, 0, -0.1, 0, 0, 1, 0.1]], "radius <= 0"), ([[0, 0, 0, 0.1, 0, 0, 1, -0.1]], "negative half height"),
                     ([[np.nan, 0, 0, 0.1, 0, 0, 1, 0.1]], "not finite"), ([[0, 0, 0, 0.1, 0, np.inf, 1, 0.1]], "not finite")):
        with pytest.raises(ValueError, match=msg):
            U.cylinder_obstacles(bad)


def test_symbol_declared_and_bound_with_its_constants(hip_lib):
    import ctypes as C
    lib = C.CDLL(hip_lib)
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    assert re.search(r"\bint rmp2_dynamics_step_contacts_cylinders\(", hdr) and hasattr(lib, "rmp2_dynamics_step_contacts_cylinders")
    assert "#define RMP2_MAX_OBSTACLE_CYLINDERS 32" in hdr and "#define RMP2_CONTACT_KIND_CYLINDER 4" in hdr
    for macro in ("RMP2_CONTACT_PAIR_CYLINDER_BASE(F, K, P, C)", "RMP2_CONTACT_PAIR_CYLINDER_FRAME(", "RMP2_CONTACT_PAIR_CYLINDER_RECORD(",
                  "RMP2_CONTACT_PAIR_KIND5(pair, F, K, P, C)", "RMP2_CONTACT_PAIR_KIND4(pair, F, K, P, C)", "RMP2_CONTACT_PAIR_SELF_BASE(F, K, P, C)"):
        assert "#define " + macro in hdr, macro
    assert re.search(r"#define RMP2_ABI_VERSION (\d+)", hdr).group(1) == "5" and lib.rmp2_abi_version() == 5
    from riemannian_motion_policies_amd import _native, engine as E, urdf as U
    assert E.MAX_OBSTACLE_CYLINDERS == 32 == U.MAX_OBSTACLE_CYLINDERS and E.CONTACT_KIND_CYLINDER == 4 == YR.CYLINDER
    n = _native.lib()
    assert len(n.rmp2_dynamics_step_contacts_cylinders.argtypes) == 31
    assert len(n.rmp2_dynamics_step_contacts_self.argtypes) == 28 == len(n.rmp2_dynamics_step_contacts_capsules.argtypes)
    args = [None] * 31
    for k, v in ((4, 0), (9, 0), (13, 0), (15, 0), (17, 0), (18, 1), (19, 0.0), (20, 0.0), (21, 0), (29, 0)):
        args[k] = v
    assert n.rmp2_dynamics_step_contacts_cylinders(*args) == -1          # (no handle: RMP2_ERR_INVALID_ARGUMENT)
    import __graft_entry__ as g
    names = [u[0] for u in g.HIP_UNITS]
    assert "rmp2_contacts_l0_cylinders" in names and "rmp2_contacts_l1_cylinders" in names and len(names) == len(set(names))

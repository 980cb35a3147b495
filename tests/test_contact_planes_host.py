"""Half-space obstacles beside the spheres (include/rmp2.h rmp2_dynamics_step_contacts_planes) on the host: the scenes of
tests/contact_planes_scene.py meet their stated conditions; the fp32 envelope that the bounds are taken from; the plane form of
the device routine of rmp2_contacts.h run on the CPU through tests/contacts_driver.cpp (also under the host sanitizers, as
a stand-alone program) against the fp64 reference of tests/contact_planes_reference.py, and BIT FOR BIT against the sphere, list
and stops drivers where the contract promises it; pair indices, poisoning, the header and urdf.contact_planes.  No GPU.

The bounds are those of tests/test_contacts_host.py (stationarity, velocity, total constraint torque, linearised gap of the
device's own pairs after one substep; q / qd after STEP_SUBSTEPS), with the K's of these scenes by the same rule: K = 4 x the worst
ratio of the fp32 ENVELOPE against the fp64 reference over the catalogue, rounded up to one significant figure (MEASURED_PLANES ->
K_PLANES, fixed here before any GPU run; test_envelope_backs_the_bounds measures them again).  Velocity and step are the random
tree's: its floor and wall rows in `corner` share two ancestors, and the Gram matrix of the two multiplies the gap's fp32
rounding / dt by its condition number (tests/test_contacts_host.py K_TREES, for the same reason).  Robots held to the bounds: the
kept rule of DESIGN 4.12 (envelope uncapped and within K / 4); at most 20 % of a group may be left out (asserted)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import contact_planes_reference as PR
import contact_planes_scene as PS
import contacts_reference as CR
import test_contacts_host as S
from test_contacts_host import D_ACT, DT, ROOT

MEASURED_PLANES = dict(res=0.01552, vel=123.2, force=6.692, step=141.5, gap=0.09897)      # the envelope's worst ratios
K_PLANES = dict(res=0.07, vel=500.0, force=30.0, step=600.0, gap=0.4)
MAX_PLANES = 8
FLOATS = ("q", "qd", "qdd", "tau", "stop", "contact", "lam")
SAN = ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g")


@pytest.fixture(scope="module")
def groups(golden_dir, tmp_path_factory):
    return PS.catalogue(golden_dir, tmp_path_factory.mktemp("trees"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver")


@pytest.fixture(scope="module")
def planes_driver(driver):
    return driver


@pytest.fixture(scope="module")
def lists_driver(driver):
    return driver


@pytest.fixture(scope="module")
def planes_driver_san(tmp_path_factory):
    return S._build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_san", SAN)


@pytest.fixture(scope="module")
def stops_driver(tmp_path_factory):
    return S._build(tmp_path_factory, "joint_stops_driver.cpp", "joint_stops_driver")


def whole_lists(B, K):
    """(csr_offset, csr_index): every robot lists the K records in table order."""
    return (K * np.arange(B + 1)).astype(np.int32), np.tile(np.arange(K), B).astype(np.int32)


def run_planes(exe, tmp_path, c, substeps=1, spheres=None, planes=None, lists=None, q=None, d_act=D_ACT):
    """The driver's plane form on a group (fields replaced by the keywords; test_contacts_host.run_driver).  planes = an empty
    table still runs the plane form."""
    return S.run_driver(exe, tmp_path, c, substeps=substeps, spheres=spheres, d_act=d_act, q=q, lists=lists,
                        planes=c["planes"] if planes is None else planes)


def same(a, b, what, pairs=True):
    for k in FLOATS:
        assert S._bits_equal(a[k], b[k]), (what, k)
    assert np.array_equal(a["status"], b["status"]), what
    if pairs:
        assert np.array_equal(a["pair"], b["pair"]), what


def by(groups, group):
    return [c for c in groups if c["group"] == group]


# ---- 1: the scenes -------------------------------------------------------------------------------------------------------------

def test_scenes_meet_their_stated_conditions(groups):
    names = PS.robots(groups)
    assert names[:2] == ["two_joint", "panda"] and len(names) == 3
    assert [c["group"] for c in groups] == list(PS.GROUPS) * 3
    assert all(len(c["q"]) <= 32 for c in groups) and sum(len(c["q"]) for c in groups) <= PS.MIXED_R
    tree = PS.for_robot(groups, names[2])[0]
    assert tree["t"].n_dof <= 9 and int(tree["t"].depth_first_schedule()[3]) >= 1
    for c in groups:
        F, K, P = c["t"].n_frames, len(c["spheres"]), len(c["planes"])
        ref, what = c["ref"], c["label"]
        kinds = [[PR.split_pair(p, F, K, P) for p in row if p >= 0] for row in ref["pair"]]
        plane_gaps = [[g for s, g in zip(row, ref["gap"][r]) if s[0] == PR.PLANE] for r, row in enumerate(kinds)]
        assert not ref["capped"].any() and not c["env"]["capped"].any(), what
        assert np.abs(np.linalg.norm(c["planes"][:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6, what
        active = PS.active_records(c)
        if c["group"] == "floor":          # an end within d_act of the floor, approached, the floor pushing back
            assert all(0 < min(g) <= D_ACT for g in plane_gaps) and all((PR.PLANE, 0) in a for a in active), what
            assert c["lim"] is not None and (ref["qd"] != c["qd"]).any(1).all(), what
        if c["group"] == "flat":
            assert PS.both_ends_active(c).all(), what
        if c["group"] == "corner":
            assert sum({(PR.PLANE, 0), (PR.PLANE, 1)} <= a for a in active) >= 2, (what, active)
        if c["group"] == "mixed" and c["name"] != "two_joint":      # (its plane row alone carries the two-joint robot)
            assert all({k for k, _ in a} == {PR.SPHERE, PR.PLANE} for a in active), (what, active)
        if c["group"] == "buried":
            assert all(min(g) < -0.01 for g in plane_gaps), what
        if c["group"] == "overflow":
            assert ref["overflow"].all() and (ref["n_cand"] == 8).all() and P == MAX_PLANES, what
            assert all({s[0] for s in row} == {PR.SPHERE, PR.PLANE} for row in kinds), what
        else:
            assert not ref["overflow"].any(), what
        if c["group"] == "point":
            f = c["point_frame"]
            assert (c["caps"][f, 0:3] == c["caps"][f, 4:7]).all() and c["caps"][f, 3] > 0
            on_f = [[s for s in row if s[0] == PR.PLANE and s[1] == f] for row in kinds]
            assert all(len(row) == 1 and row[0][3] == 0 for row in on_f), (what, on_f)
        if c["group"] == "far":
            assert all(s[0] == PR.SPHERE for row in kinds for s in row) and (ref["n_cand"] > 0).all(), what
            pr = PR.plane_rows(c["t"], c["caps"], c["planes"], K, c["q"])
            assert pr["gap"].min() > 49.0, what
    # the tree's plane rows have a prismatic column
    rows = [s for c in PS.for_robot(groups, names[2]) for row in c["ref"]["pair"] for s in [PR.split_pair(p, c["t"].n_frames, len(c["spheres"]), len(c["planes"])) for p in row if p >= 0] if s[0] == PR.PLANE]
    assert any(S.prismatic_ancestors(tree["t"], s[1]) for s in rows)


# ---- 2: the envelope -----------------------------------------------------------------------------------------------------------

def envelope_ratios(groups):
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0, gap=0.0)
    for c in groups:
        ok = ~np.asarray(c["env"]["capped"], bool) & ~np.asarray(c["ref"]["capped"], bool)
        r = PS.per_robot_ratios(c, c["env"])
        for k in ("res", "vel", "force", "gap"):
            worst[k] = max(worst[k], float(r[k][ok].max()))
        ok &= ~np.asarray(c["env_step"]["capped"], bool) & ~np.asarray(c["ref_step"]["capped"], bool)
        worst["step"] = max(worst["step"], float(PS.step_ratios(c, c["env_step"])[ok].max()))
    return worst


def test_envelope_backs_the_bounds_and_most_of_every_group_is_kept(groups):
    worst = envelope_ratios(groups)
    print("envelope worst ratios", worst)
    for k, K in K_PLANES.items():
        assert np.isclose(K, S._round_up_1sf(4 * MEASURED_PLANES[k])), (k, K, MEASURED_PLANES[k])
        assert 4 * worst[k] <= K, (k, worst[k], K)
    for c in groups:
        assert PS.kept(c, K_PLANES).mean() >= 0.8 and PS.kept_step(c, K_PLANES).mean() >= 0.8, c["label"]


# ---- 3: the device routine on the CPU against the reference -------------------------------------------------------------------

def test_device_routine_on_the_cpu_against_the_reference(planes_driver, groups, tmp_path):
    worst, kept = {}, 0
    for c in groups:
        B, K = len(c["q"]), len(c["spheres"])
        d = run_planes(planes_driver, tmp_path, c)
        kept += PS.check_group(c, d, K_PLANES, c["label"], worst)
        dl = run_planes(planes_driver, tmp_path, c, lists=whole_lists(B, K))      # (the list form on the same records)
        PS.check_group(c, dl, K_PLANES, c["label"] + "-lists", worst)
        d4 = run_planes(planes_driver, tmp_path, c, substeps=PS.STEP_SUBSTEPS)
        PS.check_group_step(c, d4, K_PLANES, c["label"], worst)
        d4 = run_planes(planes_driver, tmp_path, c, substeps=PS.STEP_SUBSTEPS, lists=whole_lists(B, K))
        PS.check_group_step(c, d4, K_PLANES, c["label"] + "-lists", worst)
    print("CPU driver worst ratios", worst, "kept", kept)
    assert kept >= 0.8 * sum(len(c["q"]) for c in groups)
    for k, K in K_PLANES.items():
        assert worst[k] <= 0.5 * K, (k, worst[k], K)


def check_flat(c, got, what):
    """Both end rows of the flat link carry force, and neither end's linearised gap leaves the gap bound."""
    F, f = c["t"].n_frames, c["flat_frame"]
    want = [PR.pair_index(F, len(c["spheres"]), len(c["planes"]), f, 0, e) for e in (0, 1)]
    lg, jn = PR.linearised_gaps(c, got["qd"], got["pair"], DT)
    br = K_PLANES["gap"] * PS.gap_bracket(c, jn)
    for r in range(len(c["q"])):
        for w in want:
            s = np.nonzero(got["pair"][r] == w)[0]
            assert len(s) == 1 and got["lam"][r, s[0]] > 0, (what, r, w, got["pair"][r], got["lam"][r])
            assert abs(lg[r, s[0]]) <= br[r, s[0]], (what, r, w, lg[r, s[0]], br[r, s[0]])


def test_flat_link_is_held_at_both_ends(planes_driver, groups, tmp_path):
    for c in by(groups, "flat"):
        check_flat(c, run_planes(planes_driver, tmp_path, c), c["label"])


# ---- 4: bit for bit -------------------------------------------------------------------------------------------------------------

def test_no_planes_and_far_planes_are_the_sphere_call_bit_for_bit(planes_driver, driver, lists_driver, groups, tmp_path):
    import test_contacts_lists_host as L
    none = np.zeros((0, 4), np.float32)
    seen = 0
    for c in by(groups, "far") + by(groups, "mixed") + by(groups, "overflow"):
        B, K = len(c["q"]), len(c["spheres"])
        for substeps in (1, 3):
            want = S.run_driver(driver, tmp_path, c, substeps=substeps)
            same(run_planes(planes_driver, tmp_path, c, substeps=substeps, planes=none), want, (c["label"], "P = 0"))
            lists = whole_lists(B, K)
            lwant = L.run_lists(lists_driver, tmp_path, c, c["spheres"], *lists, substeps=substeps)
            same(run_planes(planes_driver, tmp_path, c, substeps=substeps, planes=none, lists=lists), lwant, (c["label"], "P = 0, lists"))
            if c["group"] == "far":
                same(run_planes(planes_driver, tmp_path, c, substeps=substeps), want, (c["label"], "far"))
                same(run_planes(planes_driver, tmp_path, c, substeps=substeps, lists=lists), lwant, (c["label"], "far, lists"))
            seen += int((want["pair"] >= 0).sum())
    assert seen >= 100


def test_no_spheres_and_no_planes_is_the_stops_step_bit_for_bit(planes_driver, stops_driver, groups, tmp_path):
    import test_joint_stops_host as SH
    none = np.zeros((0, 4), np.float32)
    for c in by(groups, "floor") + by(groups, "corner"):
        for substeps in (1, 3):
            s = SH.run_driver(stops_driver, tmp_path, c["t"], c["inert"], c["q"], c["qd"], c["u"], c["drive"], c["lim"], c["limits"],
                              substeps, c["g"])
            for lists in (None, whole_lists(len(c["q"]), 0)):
                d = run_planes(planes_driver, tmp_path, c, substeps=substeps, spheres=none, planes=none, lists=lists)
                for k in ("q", "qd", "qdd", "tau", "stop"):
                    assert S._bits_equal(d[k], s[k]), (c["label"], k)
                assert (d["status"] == s["status"]).all() and (d["contact"] == 0).all() and (d["lam"] == 0).all() and (d["pair"] == -1).all()


# ---- 5: pair indices -------------------------------------------------------------------------------------------------------------

def test_pair_indices_decode_to_the_planted_frame_plane_and_end(planes_driver, groups, tmp_path):
    from riemannian_motion_policies_amd import engine as E
    seen = set()
    for c in groups:
        F, K, P = c["t"].n_frames, len(c["spheres"]), len(c["planes"])
        d = run_planes(planes_driver, tmp_path, c)
        pr = PR.pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["q"])
        frames = CR.capsule_frames(c["caps"])
        for r, row in enumerate(d["pair"]):
            for p in row[row >= 0]:
                kind, f, rec, e = E.contact_pair_split(p, F, K, P)
                assert (kind, f, rec, e) == PR.split_pair(p, F, K, P)
                assert f in frames and rec < (P if kind == E.CONTACT_KIND_PLANE else K) and e in (0, 1)
                k = list(pr["idx"]).index(int(p))          # the pair the index names is within d_act in fp64 (to rounding)
                assert pr["gap"][r, k] <= D_ACT + 1e-5
                if kind == E.CONTACT_KIND_PLANE:           # and it is that end of that frame against that plane
                    X = [x for g, e2, x, _ in PS.ends(c, c["q"][r]) if (g, e2) == (f, e)][0]
                    assert abs(c["planes"][rec, :3].astype(np.float64) @ X - c["planes"][rec, 3] - c["caps"][f, 3] - pr["gap"][r, k]) < 1e-9
                seen.add((kind, e))
        if c["group"] == "flat":
            assert {(E.CONTACT_KIND_PLANE, c["flat_frame"], 0, e) for e in (0, 1)} <= {E.contact_pair_split(p, F, K, P) for p in d["pair"][0]}
    assert seen == {(0, 0), (1, 0), (1, 1)}
    assert E.contact_pair_split(-1, 3, 4, 2) is None and E.contact_pair_split(3 * 4 + 2 * (2 * 2 + 1) + 1, 3, 4, 2) == (1, 2, 1, 1)
    with pytest.raises(ValueError):
        E.contact_pair_split(3 * 4 + 2 * 3 * 2, 3, 4, 2)


def tie_case(groups):
    """The two-joint robot at q = 0 (its links along +x, every y exactly 0) with the tip sphere as its only capsule; seven planes
    with normal +y at gaps below, an eighth at the gap of a sphere below the tip, to the bit: 0.09375 - r_tip in both
    (|0 - (-0.21875)| - 0.125 and 0 - (-0.09375)).  Nine rows qualify; the eighth slot is a tie between the sphere and a plane."""
    c = by(PS.for_robot(groups, "two_joint"), "floor")[0]
    caps = np.zeros_like(c["caps"])
    caps[2] = c["caps"][2]
    q = np.zeros((1, 2), np.float32)
    tip = CR.poses(c["t"], q, np.float32)[1][2][0]
    assert tip[1] == 0
    spheres = np.array([[tip[0], -0.21875, tip[2], 0.125]], np.float32)
    planes = np.array([[0.0, 1.0, 0.0, -0.09375 + (k + 1) / 512.0] for k in range(7)] + [[0.0, 1.0, 0.0, -0.09375]], np.float32)
    return dict(c, caps=caps, q=q, qd=np.zeros((1, 2), np.float32), u=np.zeros((1, 2), np.float32), spheres=spheres, planes=planes)


def test_a_sphere_and_a_plane_at_equal_gap_tie_to_the_sphere(planes_driver, groups, tmp_path):
    c = tie_case(groups)
    F, K, P = 3, 1, 8
    d = run_planes(planes_driver, tmp_path, c)
    ref = PR.substep(c["t"], c["inert"], c["caps"], c["spheres"], c["planes"], D_ACT, c["q"], c["qd"], c["u"], c["drive"], DT, c["lim"],
                     c["limits"], c["g"], envelope=True)      # (the fp32 restatement: the tie is one of fp32 values, asserted next)
    pr = PR.pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["q"], np.float32)
    sphere, plane = 2 * K + 0, PR.pair_index(F, K, P, 2, 7, 0)
    gaps = dict(zip(pr["idx"].tolist(), pr["gap"][0].tolist()))
    assert gaps[sphere] == gaps[plane] and 0 < gaps[sphere] <= D_ACT and sphere < plane
    want = sorted([sphere] + [PR.pair_index(F, K, P, 2, k, 0) for k in range(7)])
    assert d["status"][0] & CR.OVERFLOW and ref["overflow"][0]
    assert sorted(d["pair"][0]) == want == sorted(ref["pair"][0]), (d["pair"][0], ref["pair"][0])


# ---- 6: poisoning ------------------------------------------------------------------------------------------------------------------

def test_a_non_finite_plane_poisons_the_fleet_and_a_nan_state_only_its_robot(planes_driver, groups, tmp_path):
    for c in by(groups, "corner") + by(groups, "mixed"):
        good = run_planes(planes_driver, tmp_path, c)
        for value, (p, k) in ((np.nan, (0, 3)), (np.inf, (0, 1)), (-np.inf, (len(c["planes"]) - 1, 0))):
            planes = c["planes"].copy()
            planes[p, k] = value
            for lists in (None, whole_lists(len(c["q"]), len(c["spheres"]))):
                d = run_planes(planes_driver, tmp_path, c, planes=planes, lists=lists)
                for key in FLOATS:
                    assert np.isnan(d[key]).all(), (c["label"], key)
                assert (d["pair"] == -1).all()
        q = c["q"].copy()
        q[1, 0] = np.nan
        d = run_planes(planes_driver, tmp_path, c, q=q)
        others = np.arange(len(q)) != 1
        for key in FLOATS:
            assert np.isnan(d[key][1]).all() and S._bits_equal(d[key][others], good[key][others]), (c["label"], key)
        assert (d["pair"][1] == -1).all() and np.array_equal(d["pair"][others], good["pair"][others])


# ---- 7: under the host sanitizers (a stand-alone program; the plane buffer holds exactly P records) -------------------------------

def test_driver_under_the_host_sanitizers_equals_the_plain_build(planes_driver, planes_driver_san, groups, tmp_path):
    for c in PS.for_robot(groups, "two_joint") + by(groups, "overflow") + by(groups, "point") + [tie_case(groups)]:
        for lists in (None, whole_lists(len(c["q"]), len(c["spheres"]))):
            same(run_planes(planes_driver_san, tmp_path, c, substeps=2, lists=lists),
                 run_planes(planes_driver, tmp_path, c, substeps=2, lists=lists), c["label"])
    c = by(groups, "floor")[0]
    none = np.zeros((0, 4), np.float32)
    run_planes(planes_driver_san, tmp_path, c, planes=none, spheres=none)


# ---- 8: the interface --------------------------------------------------------------------------------------------------------------

def test_symbol_declared_and_bound_with_its_constants(hip_lib):
    import ctypes as C
    lib = C.CDLL(hip_lib)
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    assert re.search(r"\bint rmp2_dynamics_step_contacts_planes\(", hdr) and hasattr(lib, "rmp2_dynamics_step_contacts_planes")
    assert "#define RMP2_MAX_CONTACT_PLANES 8" in hdr and "#define RMP2_CONTACT_PAIR_FRAME(" in hdr
    assert re.search(r"#define RMP2_ABI_VERSION (\d+)", hdr).group(1) == "5"
    from riemannian_motion_policies_amd import _native, engine as E, urdf as U
    assert E.MAX_CONTACT_PLANES == MAX_PLANES == U.MAX_CONTACT_PLANES
    assert len(_native.lib().rmp2_dynamics_step_contacts_planes.argtypes) == 26
    args = [None] * 26
    for k, v in ((4, 0), (9, 0), (13, 0), (14, 0.0), (15, 0.0), (16, 0), (24, 0)):
        args[k] = v
    assert _native.lib().rmp2_dynamics_step_contacts_planes(*args) == -1          # (no handle: RMP2_ERR_INVALID_ARGUMENT)


def test_pair_split_helper_of_the_header(tmp_path):
    """The RMP2_CONTACT_PAIR_* macros, compiled as C, against the reference's split over a whole index range."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    src = tmp_path / "split.c"
    src.write_text('#include <stdio.h>\n#include "rmp2.h"\nint main(void) {\n  const int F = 5, K = 3, P = 2;\n'
                   '  for (int32_t p = 0; p < F * K + 2 * F * P; ++p)\n'
                   '    printf("%d %d %d %d %d\\n", p, RMP2_CONTACT_PAIR_KIND(p, F, K), RMP2_CONTACT_PAIR_FRAME(p, F, K, P),\n'
                   '           RMP2_CONTACT_PAIR_RECORD(p, F, K, P), RMP2_CONTACT_PAIR_END(p, F, K));\n  return 0;\n}\n')
    exe = tmp_path / "split"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    lines = [list(map(int, l.split())) for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert len(lines) == 5 * 3 + 2 * 5 * 2
    for p, k, f, r, e in lines:
        assert (k, f, r, e) == PR.split_pair(p, 5, 3, 2)
    assert lines[15][1:] == [1, 0, 0, 0] and lines[14][1:] == [0, 4, 2, 0]          # (spheres first, then the planes)


def test_urdf_contact_planes_normalises_and_refuses():
    from riemannian_motion_policies_amd import urdf as U
    rows = [[0.0, 0.0, 2.0, 1.0], [3.0, 0.0, 4.0, -10.0], [1e-20, 0.0, 0.0, 1e-20]]
    out = U.contact_planes(rows)
    assert out.dtype == np.float32 and out.shape == (3, 4) and out.flags["C_CONTIGUOUS"]
    want = np.array([[0, 0, 1, 0.5], [0.6, 0, 0.8, -2.0], [1, 0, 0, 1]])
    assert np.array_equal(out, want.astype(np.float32))                       # (normalised in fp64, rounded once)
    assert U.contact_planes([]).shape == (0, 4) and U.contact_planes(np.zeros((0, 4))).shape == (0, 4)
    assert np.array_equal(U.floor(), np.array([[0, 0, 1, 0]], np.float32)) and np.array_equal(U.floor(-0.25), np.array([[0, 0, 1, -0.25]], np.float32))
    assert len(U.contact_planes(np.tile([0.0, 1.0, 0.0, 0.0], (8, 1)))) == 8
    for bad, msg in (([[0.0, 0.0, 0.0, 1.0]], "zero normal"), ([[np.nan, 0.0, 1.0, 0.0]], "not finite"), ([[0.0, 0.0, 1.0, np.inf]], "not finite"),
                     (np.tile([0.0, 1.0, 0.0, 0.0], (9, 1)), "at most 8"), ([[0.0, 0.0, 1.0]], "rows")):
        with pytest.raises(ValueError, match=msg):
            U.contact_planes(bad)

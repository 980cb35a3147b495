"""The contact step on the GPU at the states where its solver works hardest, in MIXED waves, and on random trees.

1. The stress catalogue of tests/contacts_scene.py (stop-heavy, clustered, buried, overflow, coincident, pocket, axis, locked)
   as ONE fleet of R = 130 per robot and drive -- two full waves and two lanes, neighbouring lanes from different families,
   every fourth lane a clear robot on the fast path -- so that the per-lane LDS arrays with their run-time indices run beside
   lanes on other paths with other trip counts.  A launch shares one table and one box of limits, so the fleet is launched once
   per group of the catalogue (at most 12 per robot and drive) with that group's, and that group's lanes are compared with the
   fp64 reference: the bounds K_RES, K_VEL, K_FORCE, K_GAP and check_device_kkt of tests/test_contacts_host.py, unchanged, on
   the robots KEPT by the reference and the envelope alone (contacts_scene.kept), and the hard invariants on every lane.
2. Isolation, GPU against GPU, bit for bit (status words included): each robot alone (R = 1) against its lane in the fleet; the
   hardest cluster, overflow and pocket robots on the wave edges (lanes 0, 63, 64, 129) between NaN-poisoned and fast-path
   neighbours; the fleet reversed.
3. Four substeps against contacts_reference.dynamics_step within K_STEP.
4. Random trees (test_contacts_host.tree_cases): N = 9 with padded dofs, 0 / 1 / 2 save slots, prismatic ancestor columns;
   the trees' own K's (K_TREES, from the envelope on those fleets).

Measured on an MI355X (worst ratios over the kept lanes: res, vel, force, gap): panda stops 0.075, 0.33, 0.096, 0.015; cluster
0.08, 0.11, 0.067, 0.001; buried 0.013, 0.071, 0.007, 0.002; overflow 0.025, 0.28, 0.067, 0.010; coincident 0.009, 0.095,
0.012, 0.001; locked 0.026, 0.34, 0.24, 0.016; two_joint stops 0.030, 1.12, 0.40, 0.054; cluster 0.024, 0.023, 0.027, 0.001;
buried 0.009, 0.058, 0.081, 0.002; overflow 0.009, 0.033, 0.045, 0.002; coincident 0.013, 1.08, 1.09, 0.045; pocket 0.020, 0.22,
0.13, 0.024.  Four substeps: 3.1 of K_STEP = 70.  Trees: res 0.055, vel 16.8, force 10.3, step 42.9 of 0.3, 200, 50, 200.
Against a library built from the commit before the tie rule, the reference tests fail on the cluster family (panda both
drives, two_joint torque; ratios 1e3 .. 1e7) in one and four substeps; the isolation tests pass on both."""
import numpy as np
import pytest

import contacts_reference as CR
import contacts_scene as CS
import forward_dynamics_reference as FR
import test_contacts_host as S
from test_contacts_host import K_STEP, K_TREES, STEP_SUBSTEPS
from test_gpu_contacts import _bits, _engine, _plain, _step

pytestmark = pytest.mark.gpu

FLEETS = [("panda", FR.ACCEL), ("panda", FR.TORQUE), ("two_joint", FR.ACCEL), ("two_joint", FR.TORQUE)]
FLOATS = ("q", "qd", "qdd", "tau", "stop", "contact", "lam")
# lanes kept per family in one fleet (a robot of the catalogue has one or two lanes; kept is decided by the reference and the
# envelope): what the comparison may not fall below
MIN_KEPT = {"panda": dict(stops=20, cluster=20, buried=12, overflow=6, coincident=6, locked=6),
            "two_joint": dict(stops=20, cluster=20, buried=12, overflow=6, coincident=6, pocket=6)}


@pytest.fixture(scope="module")
def groups(golden_dir):
    return CS.catalogue(golden_dir)


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(c):
        if c["name"] not in cache:
            cache[c["name"]] = _engine(c)
        return cache[c["name"]]
    return get


@pytest.fixture(scope="module")
def mixed(groups, engines):
    """Per robot and drive: (fleet, the device's outputs of the launch of each group)."""
    out = {}
    for name, drive in FLEETS:
        fleet = CS.mixed_fleet(groups, name, drive)
        assert len(fleet["groups"]) <= 12 and len(fleet["q"]) == 130
        fam = [fleet["groups"][g]["family"] if g >= 0 else "clear" for g in fleet["lane_group"]]
        assert all(a != b for a, b in zip(fam[:-1], fam[1:])), fam
        assert (fleet["lane_group"][3::4] == -1).all() and (fleet["lane_group"][np.arange(130) % 4 != 3] >= 0).all()
        out[(name, drive)] = (fleet, [_step(engines(c), CS.launch_case(fleet, g)) for g, c in enumerate(fleet["groups"])])
    return out


def _same(a, b, what):
    for k in FLOATS:
        assert _bits(a[k], b[k]), (what, k)
    assert np.array_equal(a["pair"], b["pair"]) and np.array_equal(a["status"], b["status"]), what


def _rows(d, rows):
    return {k: v[rows] for k, v in d.items()}


@pytest.mark.parametrize("name,drive", FLEETS)
def test_catalogue_in_mixed_waves_against_the_reference(mixed, name, drive):
    fleet, outs = mixed[(name, drive)]
    count, worst = {}, {}
    for g, (c, d) in enumerate(zip(fleet["groups"], outs)):
        lanes, sub = CS.lanes_of(fleet, g)
        got = _rows(d, lanes)
        CS.hard_invariants(sub, got, c["label"])
        keep = CS.kept(sub)
        ratios = CS.check_kept(sub, got, keep, c["label"])
        assert ((got["status"] >> 8) <= 2 * S.WORST_ITERS).all()
        assert (((got["status"] & CR.OVERFLOW) != 0) == sub["ref"]["overflow"]).all(), c["label"]
        count[c["family"]] = count.get(c["family"], 0) + int(keep.sum())
        w = worst.setdefault(c["family"], dict(res=0.0, vel=0.0, force=0.0, gap=0.0))
        for b in w:
            w[b] = max(w[b], float(ratios[b].max(initial=0.0)))
    for fam in worst:
        print(name, "accel" if drive == FR.ACCEL else "torque", fam, "kept", count[fam], {b: round(v, 3) for b, v in worst[fam].items()})
    for fam, least in MIN_KEPT[name].items():
        assert count[fam] >= least, (fam, count[fam])
    assert not any((d["status"][fleet["lane_group"] == g] & CR.CAPPED).any() for g, d in enumerate(outs))


@pytest.mark.parametrize("name,drive", FLEETS)
def test_clear_lanes_take_the_stops_step_bit_for_bit_in_every_launch(mixed, engines, name, drive):
    fleet, outs = mixed[(name, drive)]
    clear = fleet["lane_group"] < 0
    assert clear.sum() == 32
    for g, (c, d) in enumerate(zip(fleet["groups"], outs)):
        lc = CS.launch_case(fleet, g)
        s = _plain(engines(c), lc, 1, c["limits"])
        for k in ("q", "qd", "qdd", "tau", "stop"):
            assert _bits(d[k][clear], s[k][clear]), (c["label"], k)
        assert (d["status"][clear] == s["status"][clear]).all(), c["label"]
        assert (d["pair"][clear] == -1).all() and (d["lam"][clear] == 0).all() and (d["contact"][clear] == 0).all(), c["label"]


@pytest.mark.parametrize("name,drive", FLEETS)
def test_each_robot_alone_has_its_bits_of_the_mixed_fleet(mixed, engines, name, drive):
    fleet, outs = mixed[(name, drive)]
    seen = 0
    for g, (c, d) in enumerate(zip(fleet["groups"], outs)):
        done = set()
        for lane in np.nonzero(fleet["lane_group"] == g)[0]:
            r = int(fleet["lane_robot"][lane])
            if r in done:      # (the robot's second lane: the first lane's bits)
                first = next(l for l in np.nonzero(fleet["lane_group"] == g)[0] if fleet["lane_robot"][l] == r)
                _same(_rows(d, [lane]), _rows(d, [first]), (c["label"], r, "second lane"))
                continue
            done.add(r)
            alone = _step(engines(c), CS.launch_case(fleet, g, slice(lane, lane + 1)))
            _same(alone, _rows(d, [lane]), (c["label"], r))
            seen += 1
    assert seen >= 45


@pytest.mark.parametrize("name,drive", FLEETS)
def test_reversed_fleet_permutes_the_rows_and_keeps_their_bits(mixed, engines, name, drive):
    fleet, outs = mixed[(name, drive)]
    back = dict(fleet, q=fleet["q"][::-1].copy(), qd=fleet["qd"][::-1].copy(), u=fleet["u"][::-1].copy())
    for g, (c, d) in enumerate(zip(fleet["groups"], outs)):
        r = _step(engines(c), CS.launch_case(back, g))
        _same(_rows(r, slice(None, None, -1)), d, c["label"])


@pytest.mark.parametrize("name,drive", FLEETS)
def test_hardest_robots_on_the_wave_edges_between_nan_and_fast_path_lanes(mixed, engines, name, drive):
    """The robot of most reference iterations of the cluster, overflow and pocket families on lanes 0, 63, 64 and 129; lanes
    1, 62, 65 and 128 NaN-poisoned; every other lane a clear robot."""
    fleet, outs = mixed[(name, drive)]
    clear = np.nonzero(fleet["lane_group"] < 0)[0]
    edges, poisoned = [0, 63, 64, 129], [1, 62, 65, 128]
    seen = set()
    for fam in ("cluster", "overflow", "pocket"):
        picks = [(int(c["ref"]["iters"][r]), g, r) for g, c in enumerate(fleet["groups"]) if c["family"] == fam for r in range(len(c["q"]))]
        if not picks:
            continue
        _, g, r = max(picks)
        c = fleet["groups"][g]
        lane = int(np.nonzero((fleet["lane_group"] == g) & (fleet["lane_robot"] == r))[0][0])
        src = np.array([clear[i % len(clear)] for i in range(130)])
        src[edges] = lane
        q, qd, u = fleet["q"][src].copy(), fleet["qd"][src].copy(), fleet["u"][src].copy()
        q[poisoned[0], 0], qd[poisoned[1], -1], u[poisoned[2], 0], q[poisoned[3], -1] = np.nan, np.inf, -np.inf, np.nan
        d = _step(engines(c), CS.launch_case(dict(fleet, q=q, qd=qd, u=u), g))
        for e in edges:
            _same(_rows(d, [e]), _rows(outs[g], [lane]), (c["label"], r, e))
        for k in FLOATS:
            assert np.isnan(d[k][poisoned]).all(), (c["label"], k)
        assert (d["pair"][poisoned] == -1).all()
        rest = np.setdiff1d(np.arange(130), edges + poisoned)
        _same(_rows(d, rest), _rows(outs[g], src[rest]), (c["label"], "clear lanes"))
        seen.add(fam)
    assert {"cluster", "overflow"} <= seen and ("pocket" in seen) == (name == "two_joint")


@pytest.mark.parametrize("name,drive", FLEETS)
def test_mixed_fleet_over_four_substeps(mixed, engines, groups, name, drive):
    CS.with_steps(groups)
    fleet, _ = mixed[(name, drive)]
    kept = 0
    worst = 0.0
    for g, c in enumerate(fleet["groups"]):
        d = _step(engines(c), CS.launch_case(fleet, g), substeps=STEP_SUBSTEPS)
        lanes = np.nonzero(fleet["lane_group"] == g)[0]
        rows = fleet["lane_robot"][lanes]
        got = _rows(d, lanes)
        CS.step_invariants(dict(c, q=c["q"][rows]), got, c["label"])
        keep = CS.kept_step(c)[rows]
        ref = c["ref_step"]
        bq, bqd = CR.step_brackets(ref, S.DT, STEP_SUBSTEPS)
        ratio = np.maximum(np.abs(got["q"] - ref["q"][rows]).max(1) / bq[rows], np.abs(got["qd"] - ref["qd"][rows]).max(1) / bqd[rows])
        print(c["label"], "kept", int(keep.sum()), "of", len(keep), "step", np.round(ratio[keep].max(initial=0.0), 3))
        assert (ratio[keep] <= K_STEP).all(), (c["label"], ratio.tolist())
        assert not (got["status"][keep] & CR.CAPPED).any(), c["label"]
        kept += int(keep.sum())
        worst = max(worst, float(ratio[keep].max(initial=0.0)))
    print(name, "accel" if drive == FR.ACCEL else "torque", "worst step ratio", worst, "kept", kept)
    assert kept >= 70


# ---- random trees ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trees")
    one, four = S.tree_cases(tmp), S.tree_cases(tmp, substeps=STEP_SUBSTEPS)
    S.tree_cover(one)
    return one + four


def test_gpu_contacts_trees(trees):
    """Per tree R = 65, both drives, 1 and 4 substeps: the reference within the trees' K's, the device's own KKT conditions,
    the flags, the fast path bit for bit with the stops' step, each robot alone against its lane."""
    worst = dict(res=0.0, vel=0.0, force=0.0, step=0.0)
    strong = clear_seen = 0
    cache = {}
    for c in trees:
        eng = cache.setdefault(c["name"], _engine(c))
        what = f"{c['name']}-{'accel' if c['drive'] == FR.ACCEL else 'torque'}-s{c['substeps']}"
        d = _step(eng, c, substeps=c["substeps"])
        S.flags_agree(c, d["status"], K_TREES["force"])
        if c["substeps"] == 1:
            res, vel, force, _ = S.one_step_ratios(c, d)
            print(what, "stationarity %.3g velocity %.3g force %.3g" % (res, vel, force))
            worst.update(res=max(worst["res"], res), vel=max(worst["vel"], vel), force=max(worst["force"], force))
            strong += S.check_device_kkt(c, d, what, K_TREES["gap"], K_TREES["force"])
        else:
            step = S.step_ratio(c, d)
            print(what, "step %.3g" % step)
            worst["step"] = max(worst["step"], step)
        s = _plain(eng, c, c["substeps"], c["limits"])
        clear = ~c["ref"]["any_cand"]
        clear_seen += int(clear.sum())
        for k in ("q", "qd", "qdd", "tau", "stop"):
            assert _bits(d[k][clear], s[k][clear]), (what, k)
        assert (d["status"][clear] == s["status"][clear]).all() and (d["pair"][clear] == -1).all() and (d["lam"][clear] == 0).all(), what
        for r in range(len(c["q"])):
            sel = slice(r, r + 1)
            _same(_step(eng, c, substeps=c["substeps"], q=c["q"][sel], qd=c["qd"][sel], u=c["u"][sel]), _rows(d, [r]), (what, r))
    print("worst ratios on the device, trees", worst, "strong contacts", strong)
    assert strong >= 100 and clear_seen >= 100
    for k in worst:
        assert worst[k] <= K_TREES[k], (k, worst[k], K_TREES[k])

"""The contact solver at stop-heavy, clustered and buried states (tests/contacts_scene.py): the device routine of rmp2_contacts.h
run on the CPU through tests/contacts_driver.cpp, group by group, against the fp64 reference -- and its early exits.  No GPU.

Which robots are held to the bounds is decided WITHOUT the device (contacts_scene.kept): the fp32 envelope restatement is
uncapped and within K / 4 of the reference on every bound; at most one fifth of a family may fall out.  On the kept robots the
device routine meets K_RES, K_VEL, K_FORCE, K_GAP and check_device_kkt of tests/test_contacts_host.py, unchanged, and is not
RMP2_STOP_CAPPED; on every robot the hard invariants hold (contacts_scene.hard_invariants).

Early exits.  The ITERATION CAP is reached by a second build of the driver with -DRMP2_CONTACT_MAX_ITER=3: a robot that reports
RMP2_STOP_CAPPED there stopped after exactly 3 iterations at a feasible iterate; every other robot has the production build's
bits.  The REFUSAL of a near-dependent row and the FULL WORKING SET: on the parent commit the routine took the refusal exit at
the start point v = 0 on all five robots of panda-accel-cluster-r32-9-x6 (status: 5 iterations, CAPPED | CONTACT_ACTIVE,
qd = 0) -- rows in penetration tie at alpha = 0, ties went to the lowest row, and the cluster's nearly parallel rows filled
the working set until the fifth was refused.  With ties given to the most violated row no robot of the catalogue takes either
exit (asserted below: nothing is capped in the production build), so neither is shown here; contacts_solve's code for them is
unchanged.

Figures (CPU driver, kept robots / worst ratios res, vel, force, gap):  panda stops 24 of 30 / 0.096, 1.35, 0.40, 0.060;
cluster 28 of 30 / 0.052, 0.16, 0.048, 0.004;  buried 16 / 0.015, 0.079, 0.008, 0.003;  overflow 8 / 0.021, 0.96, 0.24, 0.035;
coincident 8 / 0.018, 0.14, 0.023, 0.001;  locked 8 / 0.018, 0.66, 0.45, 0.028;  two_joint stops 30 / 0.014, 1.12, 0.40, 0.077;
cluster 30 / 0.019, 0.023, 0.022, 0.001;  buried 16 / 0.011, 0.061, 0.11, 0.005;  overflow 8 / 0.011, 0.026, 0.009, 0.001;
coincident 8 / 0.019, 1.07, 1.08, 0.044;  pocket 8 / 0.021, 0.49, 0.14, 0.039.  With a cap of 3: 74 robots capped, 128 untouched.
On the parent commit: the five robots named above miss every bound by factors of 1e3 .. 1e6, panda-torque-cluster-r0-9-x12
ends two robots at the cap of 14 (the reference needs 17 and 19), and the envelope restatement, which shared the tie rule, is
itself refused on seven robots of the cluster family (two_joint-accel-cluster-r0-1-x6 whole)."""
import numpy as np
import pytest

import contacts_reference as CR
import contacts_scene as CS
import test_contacts_host as S
from test_contacts_host import _bits_equal, _build, run_driver

LOW_CAP = 3


@pytest.fixture(scope="module")
def groups(golden_dir):
    return CS.catalogue(golden_dir)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver")


@pytest.fixture(scope="module")
def production(driver, groups, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stress")
    return [run_driver(driver, tmp, c) for c in groups]


def test_catalogue_covers_its_families_and_keeps_four_fifths_of_each(groups):
    """From the reference and the envelope alone."""
    total = {}
    for c in groups:
        assert not c["ref"]["capped"].any(), c["label"]
        if c["hard_only"]:
            continue
        k = (c["name"], c["family"])
        keep = CS.kept(c)
        a, b = total.get(k, (0, 0))
        total[k] = (a + int(keep.sum()), b + len(keep))
    print({f"{n}-{f}": v for (n, f), v in total.items()})
    for name in ("panda", "two_joint"):
        for fam in ("stops", "cluster", "buried", "overflow", "coincident", "locked" if name == "panda" else "pocket"):
            a, b = total[(name, fam)]
            assert b >= 8 and 5 * a >= 4 * b, (name, fam, a, b)
    assert sum(len(c["q"]) for c in groups if c["name"] == "panda" and c["hard_only"]) == 2
    cat = lambda k: np.concatenate([np.asarray(c["ref"][k]) for c in groups])
    # what makes the catalogue hard: working sets that fill, many stops beside contacts, overflow, rows in penetration
    assert (cat("n_stop") >= 5).sum() >= 20 and ((cat("n_stop") >= 1) & (cat("n_contact") >= 1)).sum() >= 40
    assert cat("overflow").sum() >= 20 and cat("iters").max() >= 12
    assert sum(int((c["ref"]["gap"][:, 0] < -0.001).sum()) for c in groups) >= 30


def test_device_routine_on_the_catalogue(groups, production):
    worst, count = {}, {}
    for c, d in zip(groups, production):
        CS.hard_invariants(c, d, c["label"])
        keep = CS.kept(c)
        ratios = CS.check_kept(c, d, keep, c["label"])
        k = f"{c['name']}-{c['family']}"
        count[k] = count.get(k, 0) + int(keep.sum())
        w = worst.setdefault(k, dict(res=0.0, vel=0.0, force=0.0, gap=0.0))
        for b in w:
            w[b] = max(w[b], float(ratios[b].max(initial=0.0)))
        assert ((d["status"] >> 8) <= 2 * S.WORST_ITERS).all()
        assert (((d["status"] & CR.OVERFLOW) != 0) == c["ref"]["overflow"]).all(), c["label"]
    for k in worst:
        print(k, "kept", count[k], {b: round(v, 3) for b, v in worst[k].items()})
    # neither the refusal nor the full working set is taken anywhere in the catalogue (see the head)
    assert not any((d["status"] & CR.CAPPED).any() for d in production)


def test_iteration_cap_leaves_a_feasible_iterate_and_touches_no_other_robot(groups, production, tmp_path_factory, tmp_path):
    low = _build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_cap", (f"-DRMP2_CONTACT_MAX_ITER={LOW_CAP}",))
    capped = free = 0
    for c, p in zip(groups, production):
        d = run_driver(low, tmp_path, c)
        cap = (d["status"] & CR.CAPPED) != 0
        assert ((d["status"] >> 8)[cap] == LOW_CAP).all() and ((p["status"] >> 8)[cap] > LOW_CAP).all(), c["label"]
        assert ((p["status"] >> 8)[~cap] <= LOW_CAP).all(), c["label"]
        CS.hard_invariants(c, d, c["label"] + " capped")
        for k in ("q", "qd", "qdd", "tau", "stop", "contact", "lam"):
            assert _bits_equal(d[k][~cap], p[k][~cap]), (c["label"], k)
        assert np.array_equal(d["pair"], p["pair"]) and (d["status"][~cap] == p["status"][~cap]).all(), c["label"]
        capped, free = capped + int(cap.sum()), free + int((~cap).sum())
    print("capped at", LOW_CAP, ":", capped, "robots; untouched:", free)
    assert capped >= 50 and free >= 50


def test_driver_runs_clean_under_the_host_sanitizers_on_the_catalogue(groups, production, tmp_path_factory, tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined on the host, once on every group."""
    exe = _build(tmp_path_factory, "contacts_driver.cpp", "contacts_driver_san",
                 ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"))
    for c, p in zip(groups, production):
        d = run_driver(exe, tmp_path, c)
        assert (d["status"] == p["status"]).all() and np.isfinite(d["qd"]).all(), c["label"]

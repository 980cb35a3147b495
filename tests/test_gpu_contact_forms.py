"""The four forms of the contact step's one kernel, rmp2_dynamics_step_contacts_kernel<N, SLOTS, LIST, PLANES> (shared table or
per-robot lists, without or with half-spaces), at every (N, SLOTS) the launchers pick: N = 9 with 0, 1 and 2 save slots -- one
random tree of test_contacts_host.tree_cases each -- and N = 2, the two-joint robot.  The list and plane suites reach N = 9 only
with 1 and 2 slots (the Panda, the trees of contact_planes_scene), the table form's reach the others.

Per robot: R = 70 (one full wave and six lanes), two substeps, acceleration drive, a table of 16 spheres, one launch per form.
  lists          every robot lists the whole table in table order: a strictly ascending list, so DESIGN 4.13 promises the table
                 form's results bit for bit, status word and pairs included (the pool is the table: the pair map is the identity).
                 No lane is left to the bounds of tests/test_gpu_contacts_lists.py.  The table form itself is held to the trees'
                 and the two-joint robot's two-substep reference (K_TREES / K_STEP, as tests/test_gpu_contacts_stress.py and
                 tests/test_gpu_contacts.py hold it).
  planes, both   one floor along the robot's main direction (contact_planes_scene.directions) that a fifth of the fleet starts
                 below, one robot 1 mm above and the rest higher: against the fp64 reference of contact_planes_reference after the
                 two substeps within K_PLANES["step"] x forward_dynamics_reference.step_brackets, on the robots kept by DESIGN
                 4.12's rule (reference and envelope uncapped, the envelope within a quarter of the bound); finite, lambda >= 0
                 and inside the limits on every robot.  Each of the two forms is held to the reference on its own; whether
                 their bits agree is printed, not asserted (DESIGN 4.14 promises no bits between plane kernels).
No bound is new."""
import numpy as np
import pytest

import contact_planes_reference as PR
import contact_planes_scene as PS
import contacts_reference as CR
import forward_dynamics_reference as FR
import test_contacts_host as S
from test_contact_planes_host import FLOATS, K_PLANES, whole_lists
from test_contacts_host import D_ACT, DT, K_FORCE, K_STEP, K_TREES
from test_gpu_contact_planes import _same, _step_planes
from test_gpu_contacts import _bits, _engine, _step
from test_gpu_contacts_lists import _step_lists

pytestmark = pytest.mark.gpu

R = 70
SUBSTEPS = 2
BELOW = R // 5      # robots that start with their lowest capsule end under the floor


def with_floor(c):
    """The case with `planes` [1, 4], the floor, and its two-substep references `ref_planes` / `env_planes`."""
    n = PS.directions(c, c["q"][0].astype(np.float64))[0]
    h = np.sort([PS.lowest(c, q, n)[0] for q in c["q"].astype(np.float64)])
    planes = np.array([[*n, h[BELOW] - 1e-3]], np.float32)
    step = lambda env: PR.dynamics_step(c["t"], c["inert"], c["caps"], c["spheres"], planes, D_ACT, c["q"], c["qd"], c["u"], c["drive"],
                                        DT, SUBSTEPS, c["lim"], c["limits"], c["g"], envelope=env)
    return dict(c, planes=planes, ref_planes=step(False), env_planes=step(True))


def form_cases(golden_dir, tmp_dir):
    """[case]: the first tree of 3 .. 9 dofs (N = 9) per save-slot count 0, 1, 2, then the two-joint robot (N = 2)."""
    by_slots = {}
    for c in S.tree_cases(tmp_dir, substeps=SUBSTEPS, R=R):
        if c["drive"] == FR.ACCEL and c["t"].n_dof >= 3:
            by_slots.setdefault(c["slots"], c)
    assert sorted(by_slots) == [0, 1, 2], sorted(by_slots)
    two = [c for c in S.contact_cases(golden_dir, seed=520, fleets=(("two_joint", R),), substeps=SUBSTEPS) if c["drive"] == FR.ACCEL]
    assert two[0]["t"].n_dof == 2
    return [with_floor(dict(c, label=f"{c['name']}-slots{c['slots']}")) for _, c in sorted(by_slots.items())] + \
           [with_floor(dict(two[0], label="two_joint"))]


def step_ratios(ref, got):
    bq, bqd = CR.step_brackets(ref, DT, SUBSTEPS)
    return np.maximum(np.abs(got["q"] - ref["q"]).max(1) / bq, np.abs(got["qd"] - ref["qd"]).max(1) / bqd)


def kept_planes(c):
    ref, env = c["ref_planes"], c["env_planes"]
    return ~np.asarray(ref["capped"], bool) & ~np.asarray(env["capped"], bool) & (step_ratios(ref, env) <= 0.25 * K_PLANES["step"])


def check_planes(c, got):
    """The plane form's outputs against the reference; returns (kept robots, their worst ratio)."""
    for k in FLOATS:
        assert np.isfinite(got[k]).all(), (c["label"], k)
    assert (got["lam"] >= 0).all() and (got["lam"][got["pair"] < 0] == 0).all(), c["label"]
    PS.inside(c, got, c["label"])
    keep = kept_planes(c)
    r = step_ratios(c["ref_planes"], got)
    assert (r[keep] <= K_PLANES["step"]).all(), (c["label"], r.tolist())
    assert not (got["status"][keep] & CR.CAPPED).any(), c["label"]
    return int(keep.sum()), float(r[keep].max(initial=0.0))


def floor_rows(c, d):
    """bool [R]: the robot ends its last substep with a floor row in a slot."""
    return (d["pair"] >= c["t"].n_frames * len(c["spheres"])).any(1)


@pytest.fixture(scope="module")
def cases(golden_dir, tmp_path_factory):
    return form_cases(golden_dir, tmp_path_factory.mktemp("trees"))


def test_the_robots_take_every_instantiation(cases):
    assert [c["t"].depth_first_schedule()[3] for c in cases[:3]] == [0, 1, 2]
    assert all(3 <= c["t"].n_dof <= 9 for c in cases[:3]) and cases[3]["t"].n_dof == 2
    for c in cases:
        assert len(c["q"]) == R and R > 64 and R % 64 and c["substeps"] == SUBSTEPS and len(c["spheres"]) == 16


def test_all_four_forms_per_robot(cases):
    kept = total = pushing = 0
    for c in cases:
        eng = _engine(c)
        lists = whole_lists(R, len(c["spheres"]))
        table = _step(eng, c, substeps=SUBSTEPS)
        _same(_step_lists(eng, c, c["spheres"], *lists, substeps=SUBSTEPS), table, (c["label"], "lists"))
        step = S.step_ratio(c, table)
        print(c["label"], "table form, step ratio", step)
        k_step, k_force = (K_STEP, K_FORCE) if c["label"] == "two_joint" else (K_TREES["step"], K_TREES["force"])
        assert step <= k_step, (c["label"], step, k_step)
        S.flags_agree(c, table["status"], k_force)
        assert (table["pair"] >= 0).any()

        forms = [_step_planes(eng, c, SUBSTEPS, lists=lists) for lists in (False, True)]
        for form, planes in zip(("table", "lists"), forms):
            n, worst = check_planes(c, planes)
            touching = floor_rows(c, planes)
            print(c["label"], "planes,", form, "form: kept", n, "of", R, "worst step ratio", worst, "robots on the floor", int(touching.sum()))
            assert touching.any() and not touching.all(), c["label"]
            pushing += int(((planes["lam"] > 0) & (planes["pair"] >= c["t"].n_frames * len(c["spheres"]))).sum())
            kept += n
            total += R
        print(c["label"], "plane forms bit for bit:", all(_bits(forms[0][k], forms[1][k]) for k in FLOATS))
    assert kept >= 0.8 * total, (kept, total)
    assert pushing >= 8, pushing      # (floor rows with a multiplier > 0 in the last substep, over the robots and forms)

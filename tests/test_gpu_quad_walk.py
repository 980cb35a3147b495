"""The kinematics phase of the quad step kernel -- the local transforms, and the walk with {axis, ctl} two frames ahead and its
records in an even / odd rotation (csrc/rmp2_quad.h kWalkAhead) -- at the programs where its fetches and clamps can go wrong.
Robots, fleets and what the CPU says about them: tests/quad_walk_scenes.py (pinned by tests/test_quad_walk_scenes.py).

The walk's results are visible only through the step.  Every case forces the build (RMP2_KERNEL=quad, RMP2_QUAD_MINW = 2, 3, 4:
the four-wave builds carry the new form, the others the older one, as the control), runs fleets of 1, 17 and 65 robots (a lone
quad, a partial wave, tail quads), asserts the build tag rmp2_last_kernel reports, and holds

  * q-double-dot to the fp64 oracle through oracle.accuracy_gate -- the states are clear of any obstacle, so EVERY robot must be
    admitted by the north-star clause A, |got - ref| <= 1e-5 max(1, |ref|) --,
  * in the general flavour the exported (M, f) to the reference-precision oracle.

The nine-dof cases run tests/test_gpu_quad_builds.py test_plain_step and test_general_flavour themselves on the sets of this
module: the bound on (M, f), the tag check and the gate are the ones written there; the gate is wrapped to ask for clause A."""
import numpy as np
import pytest

import quad_walk_scenes as W
import test_gpu_quad_builds as QB
from test_gpu_quad_builds import torch_mod  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
MINW = [2, 3, 4]
NAN_SETS = ("len3", "len5", "len13", "tree2")   # (every clamp active; odd tail; the long chain; both slots)


@pytest.fixture(scope="module")
def cases():
    """The shape tests/test_gpu_quad_builds.py keeps its cases in: references and engines filled in on first use."""
    return {"tables": {"far": W.FAR}, "sets": W.make_sets(), "kw": {}, "ref": {}, "roll": {}, "engines": {}}


@pytest.fixture
def on_these_sets(monkeypatch):
    """test_gpu_quad_builds.py reads a set's form (symmetric: no JointLimitAvoidance leaf) and engine environment from its scenes
    module, and gates q-double-dot with the fp32 envelope.  For the duration of a test: the sets of this module beside them, and
    clause A on top of the gate."""
    import oracle as O
    monkeypatch.setattr(QB.S, "SETS", {**QB.S.SETS, **{name: (True, {}) for name in W.ROBOTS}})
    gate = QB._gate

    def north_star_gate(out, exact, env, R, what, rows=None):
        gate(out, exact, env, R, what, rows=rows)
        ex = {k: (v[:R] if isinstance(v, np.ndarray) and v.shape[:1] == (W.R_MAX,) else v) for k, v in exact.items()}
        verdict = O.accuracy_gate(out, ex, truth=ex["qdd64"], envelope=env[:R])
        assert verdict["a"].all(), f"{what}, R = {R}: clause A admits {int(verdict['a'].sum())} of {R}: {O.gate_summary(verdict)}"

    monkeypatch.setattr(QB, "_gate", north_star_gate)


def _assert_slots(cases, name, minw):
    """The build ran the slot count the scene is there for (the tag names the SLOTS template argument)."""
    tag = cases["engines"][(name, minw, False)].last_kernel()
    assert f"[build n9 s{W.PROGRAMS[name][1]} w{minw} " in tag, tag


@pytest.mark.parametrize("minw", MINW)
@pytest.mark.parametrize("name", list(W.ROBOTS))
def test_plain_step(torch_mod, cases, on_these_sets, name, minw):   # noqa: F811
    """The plain control step (the headline's flavour): q-double-dot, clause A for every robot."""
    QB.test_plain_step(torch_mod, cases, name, "none", minw)
    _assert_slots(cases, name, minw)


@pytest.mark.parametrize("minw", MINW)
@pytest.mark.parametrize("name", list(W.ROBOTS))
def test_general_flavour(torch_mod, cases, on_these_sets, name, minw):   # noqa: F811
    """The step with M= and f=: the exported system at the bound test_gpu_quad_builds.py holds it to, q-double-dot as above."""
    QB.test_general_flavour(torch_mod, cases, name, "none", minw)
    _assert_slots(cases, name, minw)


@pytest.mark.parametrize("minw", MINW)
@pytest.mark.parametrize("name", W.TWO_DOF)
def test_two_dof_template(torch_mod, cases, name, minw):   # noqa: F811
    """The TwoJoint sets of configs.py (the two-dof template; the identity set has no frame to walk at all): plain step and
    general flavour, the same two checks."""
    import oracle as O
    torch = torch_mod
    desc, s = cases["sets"][name]
    kw = W.obstacle_kwargs(name)
    exact = O.step(desc, s["q"], s["qd"], s["goal"], precision="f64", **kw)
    ref32 = O.step(desc, s["q"], s["qd"], s["goal"], **kw)
    env = O.fp32_envelope(desc, s["q"], s["qd"], s["goal"], **kw)
    eng = QB._engine_env(desc, RMP2_KERNEL="quad", RMP2_QUAD_MINW=minw)
    for R in W.FLEETS:
        q, qd, goal = QB._states(torch, s, R)
        obs = eng.obstacles(**{k: torch.from_numpy(v) for k, v in kw.items()}) if kw else None
        ex = {k: (v[:R] if isinstance(v, np.ndarray) and v.shape[:1] == (W.R_MAX,) else v) for k, v in exact.items()}
        for flavour in ("plain", "general"):
            M = torch.full((R, 2, 2), float("nan"), dtype=torch.float64, device="cuda")
            f = torch.full((R, 2), float("nan"), dtype=torch.float64, device="cuda")
            out = eng.step(q, qd, goal, obstacles=obs, **({"M": M, "f": f} if flavour == "general" else {}))
            torch.cuda.synchronize()
            tag = eng.last_kernel()
            assert "quad" in tag and f"[build n2 s0 w{minw} {flavour} " in tag, tag
            verdict = O.accuracy_gate(out.cpu().numpy(), ex, truth=ex["qdd64"], envelope=env[:R])
            print(f"QW gate {name} {flavour} minw {minw} R {R}: {O.gate_summary(verdict)}")
            assert verdict["ok"].all() and verdict["a"].all(), f"{name} {flavour} minw {minw} R {R}: {O.gate_summary(verdict)}"
            if flavour == "general":
                eM, ef = np.abs(M.cpu().numpy() - ref32["M"][:R]).max(), np.abs(f.cpu().numpy() - ref32["f"][:R]).max()
                tM, tf = W.system_bound(ref32["M"][:R]), W.system_bound(ref32["f"][:R])
                print(f"QW system {name} minw {minw} R {R}: |M - ref| {eM:.3e} of bound {tM:.3e}, |f - ref| {ef:.3e} of bound {tf:.3e}")
                assert eM <= tM and ef <= tf, f"{name} minw {minw} R {R}: M {eM:.3e} / {tM:.3e}, f {ef:.3e} / {tf:.3e}"


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("flavour", ["plain", "general"])
@pytest.mark.parametrize("name", NAN_SETS)
def test_a_nan_robot_stays_in_its_quad(torch_mod, cases, name, flavour, minw):   # noqa: F811
    """17 robots, q of robot 5 not a number: every other robot's results are the clean run's bit for bit, robot 5 carries the
    non-finite status.  (The quarantine reads the tile the local transforms read.)"""
    torch = torch_mod
    desc, s = cases["sets"][name]
    n, R = desc.robot.n_dof, 17
    eng = QB._engine_env(desc, RMP2_KERNEL="quad", RMP2_QUAD_MINW=minw)
    runs = []
    for poison in (False, True):
        q = s["q"][:R].copy()
        if poison:
            q[5, 0] = np.nan
        q, qd, goal = torch.from_numpy(q).cuda(), torch.from_numpy(s["qd"][:R]).cuda(), torch.from_numpy(s["goal"][:R]).cuda()
        st = torch.zeros(R, dtype=torch.int32, device="cuda")
        res = {}
        if flavour == "general":
            res["M"] = torch.zeros((R, n, n), dtype=torch.float64, device="cuda")
            res["f"] = torch.zeros((R, n), dtype=torch.float64, device="cuda")
            res["qdd"] = eng.step(q, qd, goal, status=st, M=res["M"], f=res["f"])
        else:
            res["qdd"] = eng.step(q, qd, goal, status=st)
        torch.cuda.synchronize()
        assert f" w{minw} {flavour} " in eng.last_kernel(), eng.last_kernel()
        runs.append(({k: v.cpu().numpy().copy() for k, v in res.items()}, st.cpu().numpy().copy()))
    (clean, st_clean), (dirty, st_dirty) = runs
    others = np.arange(R) != 5
    assert np.isfinite(clean["qdd"]).all() and not (st_clean & QB.D_STATUS_NONFINITE).any()
    for k in clean:
        assert np.array_equal(clean[k][others].view(np.uint8), dirty[k][others].view(np.uint8)), f"{k} of a neighbour of the NaN robot changed"
    assert np.array_equal(st_clean[others], st_dirty[others])
    assert st_dirty[5] & QB.D_STATUS_NONFINITE and np.isnan(dirty["qdd"][5]).all()

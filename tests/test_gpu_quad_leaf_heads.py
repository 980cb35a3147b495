"""The FK-leaf heads of the four-wave quad builds against the fp64 oracle, on small fleets.

The plain four-wave builds of the nine-dof template are the ones whose frame loop is reshaped for speed (csrc/rmp2_quad.h
kRegionPullback, kWalkAhead, kAncAtUse: the tests on a frame's dof mask made behind the pair loop).  What such a shape can get wrong
is which leaf's head or which frame's mask a frame works with; a head from the wrong frame is a wrong parameter set on a leaf and
shows only where neighbouring leaves differ, so the sets of tests/quad_leaf_head_scenes.py (pinned on the CPU by
tests/test_quad_leaf_head_scenes.py) give every obstacle leaf its own parameters.  Mechanics as in tests/test_gpu_quad_builds.py:
RMP2_KERNEL=quad and RMP2_QUAD_MINW=4 forced (2 as the control), fleets of 1, 17 and 65 robots, the build tag asserted for every
case, q-double-dot through oracle.accuracy_gate against the fp64 oracle and exported (M, f) against that module's bounds."""
import numpy as np
import pytest

import quad_build_scenes as S
import quad_leaf_head_scenes as H
import test_gpu_quad_builds as QB

pytestmark = pytest.mark.gpu
FLEETS, R_MAX = S.FLEETS, S.R_MAX
SYM = True   # every set here is symmetric

PLAIN_CASES = [(s, "33") for s in H.SETS] + [("differ", t) for t in ("far", "ragged", "capsule")] + [("AABA", "ragged"), ("ABB", "capsule")]
GENERAL_CASES = [("differ", "33"), ("AABA", "33"), ("one-da", "33"), ("two-targets", "33")]
ROLLOUT_CASES = [("differ", "33"), ("ABB", "33"), ("target-between", "ragged")]


def _tag(flavor, table, minw):
    obs = "any" if flavor == "general" else QB.OBS_OF_TABLE[table]
    return QB._tag(minw, flavor, obs, SYM, table == "capsule")


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def cases():
    tables = S.make_tables()
    return {"tables": tables, "sets": H.make_sets(tables), "kw": {}, "ref": {}, "engines": {}}


def _engine(cases, set_name, minw):
    key = (set_name, minw)
    if key not in cases["engines"]:
        cases["engines"][key] = QB._engine_env(cases["sets"][set_name][0], RMP2_KERNEL="quad", RMP2_QUAD_MINW=minw)
    return cases["engines"][key]


def _kw(cases, set_name, table):
    key = (set_name, table)
    if key not in cases["kw"]:
        desc, s = cases["sets"][set_name]
        cases["kw"][key] = S.obstacle_kwargs("panda", desc, s, cases["tables"], table)
    return cases["kw"][key]


def _reference(cases, set_name, table):
    import oracle as O
    key = (set_name, table)
    if key not in cases["ref"]:
        desc, s = cases["sets"][set_name]
        kw = _kw(cases, set_name, table)
        cases["ref"][key] = (O.step(desc, s["q"], s["qd"], s["goal"], precision="f64", **kw),
                             O.fp32_envelope(desc, s["q"], s["qd"], s["goal"], **kw),
                             O.step(desc, s["q"], s["qd"], s["goal"], **kw))
    return cases["ref"][key]


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("set_name,table", PLAIN_CASES)
def test_plain_step(torch_mod, cases, set_name, table, minw):
    """One control step, no debug outputs, every set over the 33-sphere table (a second chunk); the differing-heads set also over a
    table wholly out of range, ragged lists (an empty one among them) and a capsule table."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    exact, env, _ = _reference(cases, set_name, table)
    eng = _engine(cases, set_name, minw)
    for R in FLEETS:
        q, qd, goal = QB._states(torch, s, R)
        out = eng.step(q, qd, goal, obstacles=QB._obstacles(torch, eng, _kw(cases, set_name, table), R))
        torch.cuda.synchronize()
        QB._assert_tag(eng.last_kernel(), _tag("plain", table, minw))
        QB._gate(out.cpu().numpy(), exact, env, R, f"leaf heads plain {set_name} {table} minw {minw} [{eng.last_kernel().split('[build')[-1]}")


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("set_name,table", GENERAL_CASES)
def test_general_flavour(torch_mod, cases, set_name, table, minw):
    """The step with M= and f=: M and f against the reference-precision oracle at 5e-6 * max(1, max |ref|) (the bound of
    tests/test_gpu_quad_builds.py test_general_flavour), q-double-dot through the gate."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    n = desc.robot.n_dof
    exact, env, ref32 = _reference(cases, set_name, table)
    eng = _engine(cases, set_name, minw)
    for R in FLEETS:
        q, qd, goal = QB._states(torch, s, R)
        M = torch.full((R, n, n), float("nan"), dtype=torch.float64, device="cuda")
        f = torch.full((R, n), float("nan"), dtype=torch.float64, device="cuda")
        out = eng.step(q, qd, goal, obstacles=QB._obstacles(torch, eng, _kw(cases, set_name, table), R), M=M, f=f)
        torch.cuda.synchronize()
        name = eng.last_kernel()
        QB._assert_tag(name, _tag("general", table, minw))
        M, f = M.cpu().numpy(), f.cpu().numpy()
        eM, ef = np.abs(M - ref32["M"][:R]).max(), np.abs(f - ref32["f"][:R]).max()
        tM, tf = 5e-6 * max(1.0, np.abs(ref32["M"][:R]).max()), 5e-6 * max(1.0, np.abs(ref32["f"][:R]).max())
        print(f"LH system general {set_name} {table} minw {minw} R {R}: |M - ref| {eM:.3e} of bound {tM:.3e}, |f - ref| {ef:.3e} of bound {tf:.3e}")
        assert eM <= tM and ef <= tf, f"{set_name} {table} minw {minw} R {R}: M {eM:.3e} / {tM:.3e}, f {ef:.3e} / {tf:.3e}"
        assert np.array_equal(M, M.transpose(0, 2, 1))
        QB._gate(out.cpu().numpy(), exact, env, R, f"leaf heads general {set_name} {table} minw {minw} [{name.split('[build')[-1]}")


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("set_name,table", ROLLOUT_CASES)
def test_fused_rollout_is_three_single_steps(torch_mod, cases, set_name, table, minw):
    """A fused rollout of three control steps against three rollouts of one control step each, chained on the host -- the same
    build, the same plant arithmetic: bit for bit.  The frame loop starts over with every control step, and whatever a kernel
    keeps or fetches ahead across frames must start over with it.  The first control step's q-double-dot goes through the gate."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    sub, dt = S.ROLLOUT["substeps"], S.ROLLOUT["dt"]
    exact, env, _ = _reference(cases, set_name, table)
    eng = _engine(cases, set_name, minw)
    for R in FLEETS:
        obs = QB._obstacles(torch, eng, _kw(cases, set_name, table), R)
        q0, qd0, goal = QB._states(torch, s, R)
        qf, qdf = q0.clone(), qd0.clone()
        last_f = eng.rollout(qf, qdf, goal, obstacles=obs, n_control_steps=3, substeps=sub, dt=dt)
        torch.cuda.synchronize()
        QB._assert_tag(eng.last_kernel(), _tag("rollout", table, minw))
        last_f = last_f.clone()
        q, qd = q0.clone(), qd0.clone()
        for k in range(3):
            last = eng.rollout(q, qd, goal, obstacles=obs, n_control_steps=1, substeps=sub, dt=dt)
            torch.cuda.synchronize()
            if k == 0:
                QB._gate(last.cpu().numpy(), exact, env, R, f"leaf heads rollout, first control step, {set_name} {table} minw {minw}")
        QB._assert_tag(eng.last_kernel(), _tag("rollout", table, minw))
        for a, b, what in ((qf, q, "q"), (qdf, qd, "qd"), (last_f, last, "qdd")):
            assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)), f"{set_name} {table} minw {minw} R {R}: {what}"
        assert torch.isfinite(qf).all() and (qf - q0).abs().max().item() > 1e-5   # the fleet moved


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("flavour,set_name", [("plain", "differ"), ("plain", "AABA"), ("general", "differ"), ("rollout", "ABB")])
def test_a_nan_robot_stays_in_its_quad(torch_mod, cases, flavour, set_name, minw):
    """17 robots, q of robot 5 not a number: every other robot's results are the clean run's bit for bit, and robot 5 carries the
    non-finite status."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    n, R, table = desc.robot.n_dof, 17, "33"
    eng = _engine(cases, set_name, minw)
    obs = QB._obstacles(torch, eng, _kw(cases, set_name, table), R)
    runs = []
    for poison in (False, True):
        q = s["q"][:R].copy()
        if poison:
            q[5, 2] = np.nan
        q, qd, goal = torch.from_numpy(q).cuda(), torch.from_numpy(s["qd"][:R]).cuda(), torch.from_numpy(s["goal"][:R]).cuda()
        st = torch.zeros(R, dtype=torch.int32, device="cuda")
        res = {}
        if flavour == "rollout":
            res["qdd"] = eng.rollout(q, qd, goal, obstacles=obs, status=st, **S.ROLLOUT)
            res["q"], res["qd"] = q, qd
        elif flavour == "general":
            res["M"] = torch.zeros((R, n, n), dtype=torch.float64, device="cuda")
            res["f"] = torch.zeros((R, n), dtype=torch.float64, device="cuda")
            res["qdd"] = eng.step(q, qd, goal, obstacles=obs, status=st, M=res["M"], f=res["f"])
        else:
            res["qdd"] = eng.step(q, qd, goal, obstacles=obs, status=st)
        torch.cuda.synchronize()
        QB._assert_tag(eng.last_kernel(), _tag(flavour, table, minw))
        runs.append(({k: v.cpu().numpy().copy() for k, v in res.items()}, st.cpu().numpy().copy()))
    (clean, st_clean), (dirty, st_dirty) = runs
    others = np.arange(R) != 5
    assert np.isfinite(clean["qdd"]).all() and not (st_clean & QB.D_STATUS_NONFINITE).any()
    for k in clean:
        assert np.array_equal(clean[k][others].view(np.uint8), dirty[k][others].view(np.uint8)), f"{k} of a neighbour of the NaN robot changed"
    assert np.array_equal(st_clean[others], st_dirty[others])
    assert st_dirty[5] & QB.D_STATUS_NONFINITE and np.isnan(dirty["qdd"][5]).all()

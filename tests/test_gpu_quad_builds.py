"""Every four-wave build of the quad step kernel against the fp64 oracle, on small fleets.

The builds with MINW == 4 (128 registers, four waves per SIMD) carry their own pull-back (csrc/rmp2_quad.h kRegionPullback: one
region per row block, ladder entries on DPP operands, the columns of a skipped row block left undefined).  The dispatch gives them
to fleets of 49 153 robots and more, for which there is no oracle; so the build is forced (RMP2_KERNEL=quad, RMP2_QUAD_MINW, read
at rmp2_create), the fleets are small -- 1, 17 and 65 robots: one quad, a full wave and one robot, tail quads -- and every case
asserts the build tag rmp2_last_kernel reports (csrc/rmp2_host.h quad_build_tag) so that it proves which instantiation it ran.
MINW == 2 (and 3 where such a build exists) runs beside it as the control.

Sets, tables and what the CPU says about them: tests/quad_build_scenes.py (pinned by tests/test_quad_build_scenes.py).

The kRegionPullback instantiations launch_quad can launch for N == 9, and the case that reaches each (tags without the slot count;
sym: config3-auto / config3-pinv / tree / free3, gen: config3-gen / arm7 / config2):

  w4 plain none sym | gen                 test_plain_step  [free3 | config2, none]
  w4 plain shared sym | gen sph           test_plain_step  [config3-*, tree | config3-gen, arm7; 33 and far]
  w4 plain ragged sym | gen sph           test_plain_step  [.., ragged]
  w4 plain explicit sym | gen sph         test_plain_step  [.., explicit33]
  w4 plain explicit-stream sym | gen sph  test_plain_step  [config3-auto, config3-pinv | config3-gen; explicit32]
  w4 plain shared sym | gen cap           test_plain_step  [.., capsule]
  w4 general any sym | gen sph            test_general_flavour  [config3-*, tree, free3, rank1-* | config3-gen, arm7, config2]
  w4 general any sym | gen cap            test_general_flavour  [config3-auto | config3-gen; capsule]
  w4 rollout none sym | gen sph           test_plain_rollout  [free3 | config2]
  w4 rollout shared sym | gen sph         test_plain_rollout  [config3-*, tree | config3-gen, arm7; 33]
  w4 rollout ragged sym | gen sph         test_plain_rollout  [.., ragged]

test_the_cases_name_every_region_pullback_build holds this list to the parameter tables below.  Lines starting with "QB" are what
profiles/quad_builds.txt records."""
import os

import numpy as np
import pytest

import quad_build_scenes as S

pytestmark = pytest.mark.gpu
D_STATUS_NONFINITE = 1   # include/rmp2.h RMP2_STATUS_NONFINITE
FLEETS, R_MAX = S.FLEETS, S.R_MAX

OBS_OF_TABLE = {"none": "none", "33": "shared", "far": "shared", "ragged": "ragged", "capsule": "shared", "explicit33": "explicit",
                "explicit32": "explicit"}
PLAIN_CASES = [(s, t) for s in S.DISTANCE_SETS for t in ("33", "far", "ragged", "capsule", "explicit33")] + \
              [(s, "explicit32") for s in ("config3-auto", "config3-pinv", "config3-gen")] + [("free3", "none"), ("config2", "none")]
GENERAL_CASES = [(s, "33") for s in S.DISTANCE_SETS] + [("config3-auto", "capsule"), ("config3-gen", "capsule")] + \
                [(s, "none") for s in ("free3", "config2", "rank1-panda", "rank1-tree")]
ROLLOUT_CASES = [(s, t) for s in S.DISTANCE_SETS for t in ("33", "ragged")] + [("free3", "none"), ("config2", "none")]
MEASURED_BOUND = ("arm7", "tree")   # rollout bound measured from the oracle's own fp32 error (test_plain_rollout)


def _tag(minw, flavor, obs, sym, cap):
    return f" w{minw} {flavor} {obs} {'sym' if sym else 'gen'} {'cap' if cap else 'sph'}]"


def _plain_tag(set_name, table, minw):
    if table == "explicit32" and minw == 4:   # (32 aligned pairs per leaf under RMP2_EXPLICIT_STREAM=1: the streamed build)
        return _tag(4, "plain", "explicit-stream", S.SETS[set_name][0], False)
    return _tag(minw, "plain", OBS_OF_TABLE[table], S.SETS[set_name][0], table == "capsule")


def _general_tag(set_name, table, minw):
    return _tag(minw, "general", "any", S.SETS[set_name][0], table == "capsule")


def _rollout_tag(set_name, table, minw):
    return _tag(minw, "rollout", OBS_OF_TABLE[table], S.SETS[set_name][0], False)


def _assert_tag(name, want):
    assert "quad" in name and "[build n9 s" in name and name.endswith(want), f"ran {name!r}, expected a build ending in {want!r}"


def test_the_cases_name_every_region_pullback_build():
    """launch_quad's four-wave launches for N == 9 (rmp2_quad_tu.hip: RMP2_QUAD_PLAIN(4), RMP2_QUAD_BY_CAP(4, false),
    RMP2_QUAD_ROLL_SYM(4, .) and the streamed explicit-pair build), and the tags the cases below assert at minw = 4."""
    every = {_tag(4, "plain", o, y, False) for o in ("none", "shared", "ragged", "explicit", "explicit-stream") for y in (True, False)}
    every |= {_tag(4, "plain", "shared", y, True) for y in (True, False)}
    every |= {_tag(4, "general", "any", y, c) for y in (True, False) for c in (True, False)}
    every |= {_tag(4, "rollout", o, y, False) for o in ("none", "shared", "ragged") for y in (True, False)}
    named = {_plain_tag(s, t, 4) for s, t in PLAIN_CASES} | {_general_tag(s, t, 4) for s, t in GENERAL_CASES} | \
            {_rollout_tag(s, t, 4) for s, t in ROLLOUT_CASES}
    assert len(every) == 22 and named == every, sorted(every ^ named)


def _engine_env(desc, **env):
    """Engine created with diagnostic environment knobs (read at rmp2_create) set, restored afterwards."""
    from riemannian_motion_policies_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Engine(desc, 0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Sets and tables of the 65-robot fleet; references and engines filled in on first use."""
    tables = S.make_tables()
    return {"tables": tables, "sets": S.make_sets(tmp_path_factory.mktemp("tree"), tables), "kw": {}, "ref": {}, "roll": {}, "engines": {}}


def _engine(cases, set_name, minw, stream=False):
    key = (set_name, minw, stream)
    if key not in cases["engines"]:
        env = dict(S.SETS[set_name][1], RMP2_KERNEL="quad", RMP2_QUAD_MINW=minw)
        if stream:
            env["RMP2_EXPLICIT_STREAM"] = 1
        cases["engines"][key] = _engine_env(cases["sets"][set_name][0], **env)
    return cases["engines"][key]


def _kw(cases, set_name, table):
    """Obstacle arguments of the 65-robot fleet (numpy)."""
    key = (set_name, table)
    if key not in cases["kw"]:
        desc, s = cases["sets"][set_name]
        cases["kw"][key] = S.obstacle_kwargs(set_name, desc, s, cases["tables"], table)
    return cases["kw"][key]


def _kw_rows(kw, R):
    """... of its first R robots."""
    out = dict(kw)
    if "csr_offset" in kw:
        out["csr_offset"] = kw["csr_offset"][:R + 1]
        out["csr_index"] = kw["csr_index"][:max(int(kw["csr_offset"][R]), 1)]
    for k in ("p_link", "p_obs"):
        if k in kw:
            out[k] = kw[k][:R]
    return out


def _obstacles(torch, eng, kw, R):
    if not kw:
        return None
    return eng.obstacles(**{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in _kw_rows(kw, R).items()})


def _reference(cases, set_name, table):
    """The step of the 65-robot fleet: fp64 evaluation of the reference's formulae, the fp32 envelope, and the
    reference-precision evaluation (fp32 leaves, fp64 sum: what M and f are held to).  Once per (set, table)."""
    import oracle as O
    key = (set_name, table)
    if key not in cases["ref"]:
        desc, s = cases["sets"][set_name]
        kw = _kw(cases, set_name, table)
        cases["ref"][key] = (O.step(desc, s["q"], s["qd"], s["goal"], precision="f64", **kw),
                             O.fp32_envelope(desc, s["q"], s["qd"], s["goal"], **kw),
                             O.step(desc, s["q"], s["qd"], s["goal"], **kw))
    return cases["ref"][key]


def _gate(out, exact, env, R, what, rows=None):
    """q-double-dot through the accuracy gate with the fp32 envelope, as bench.py's result check holds the timed buffers to it: no
    robot is rejected and none exempted.  (rows: robot r is row rows[r] of the 65-robot reference; the first R rows otherwise.)"""
    import oracle as O
    rows = np.arange(R) if rows is None else rows
    ex = {k: (v[rows] if isinstance(v, np.ndarray) and v.shape[:1] == (R_MAX,) else v) for k, v in exact.items()}
    verdict = O.accuracy_gate(out, ex, truth=ex["qdd64"], envelope=env[rows])
    summary = O.gate_summary(verdict)
    print(f"QB gate {what} R {R}: {summary}")
    assert np.isfinite(out).all() and verdict["ok"].all() and summary["rejected"] == 0, f"{what}, R = {R}: {summary}"


def _states(torch, s, R):
    return tuple(torch.from_numpy(s[k][:R]).cuda() for k in ("q", "qd", "goal"))


@pytest.mark.parametrize("minw", [2, 3, 4])
@pytest.mark.parametrize("set_name,table", PLAIN_CASES)
def test_plain_step(torch_mod, cases, set_name, table, minw):
    """(a) One control step, no debug outputs: the per-mode plain builds -- no obstacle data, a shared sphere table (33 spheres: a
    partial second chunk; one sphere a kilometre away: S = h = 0), per-robot lists over the table, explicit pairs in the single loop
    (33 per leaf) and streamed (32 per leaf, aligned), a capsule table."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    exact, env, _ = _reference(cases, set_name, table)
    eng = _engine(cases, set_name, minw, stream=(table == "explicit32" and minw == 4))
    for R in FLEETS:
        q, qd, goal = _states(torch, s, R)
        out = eng.step(q, qd, goal, obstacles=_obstacles(torch, eng, _kw(cases, set_name, table), R))
        torch.cuda.synchronize()
        _assert_tag(eng.last_kernel(), _plain_tag(set_name, table, minw))
        _gate(out.cpu().numpy(), exact, env, R, f"plain {set_name} {table} minw {minw} [{eng.last_kernel().split('[build')[-1]}")


@pytest.mark.parametrize("minw", [2, 3, 4])
@pytest.mark.parametrize("set_name,table", GENERAL_CASES)
def test_general_flavour(torch_mod, cases, set_name, table, minw):
    """(b) The step with M= and f=: the general flavour (everything at run time).  M and f against the reference-precision oracle
    at 5e-6 * max(1, max |ref|), the tolerance test_gpu_random_robots.py holds these robots to; q-double-dot through the gate;
    the symmetric build's M is its upper triangle mirrored.  The rank1 sets have no inertia leaf: their step is two kernels, the
    quad half -- this flavour -- stops behind (M, f) and runs the rank-one form of S col inside the region pull-back."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    n = desc.robot.n_dof
    exact, env, ref32 = _reference(cases, set_name, table)
    eng = _engine(cases, set_name, minw)
    for R in FLEETS:
        q, qd, goal = _states(torch, s, R)
        M = torch.full((R, n, n), float("nan"), dtype=torch.float64, device="cuda")
        f = torch.full((R, n), float("nan"), dtype=torch.float64, device="cuda")
        out = eng.step(q, qd, goal, obstacles=_obstacles(torch, eng, _kw(cases, set_name, table), R), M=M, f=f)
        torch.cuda.synchronize()
        name = eng.last_kernel()
        _assert_tag(name, _general_tag(set_name, table, minw))
        assert ("rmp2_pinv_kernel" in name) == set_name.startswith("rank1"), name
        M, f = M.cpu().numpy(), f.cpu().numpy()
        eM, ef = np.abs(M - ref32["M"][:R]).max(), np.abs(f - ref32["f"][:R]).max()
        tM, tf = 5e-6 * max(1.0, np.abs(ref32["M"][:R]).max()), 5e-6 * max(1.0, np.abs(ref32["f"][:R]).max())
        print(f"QB system general {set_name} {table} minw {minw} R {R}: |M - ref| {eM:.3e} of bound {tM:.3e}, |f - ref| {ef:.3e} of bound {tf:.3e}")
        assert eM <= tM and ef <= tf, f"{set_name} {table} minw {minw} R {R}: M {eM:.3e} / {tM:.3e}, f {ef:.3e} / {tf:.3e}"
        if S.SETS[set_name][0]:
            assert np.array_equal(M, M.transpose(0, 2, 1)), "the symmetric build's matrix is its upper triangle, mirrored"
        _gate(out.cpu().numpy(), exact, env, R, f"general {set_name} {table} minw {minw} [{name.split('[build')[-1]}")


def _rollout_reference(cases, set_name, table):
    """The oracle's closed loop on the 65-robot fleet, reference precision and fp64: once per (set, table)."""
    key = (set_name, table)
    if key not in cases["roll"]:
        desc, s = cases["sets"][set_name]
        cases["roll"][key] = S.oracle_rollout_pair(desc, s, _kw(cases, set_name, table))
    return cases["roll"][key]


def _rollout_bounds(set_name, ref32, ref64):
    """Per robot and component: 1e-5 * max(1, |.|_inf of the robot) -- the K = 3 row of test_gpu_dropin.py
    test_fused_rollout_against_the_oracle.  For the 7-dof arm and the tree that row has not been established: there the bound is
    the larger of it and 4 x |oracle in fp32 - oracle in fp64| (the margin tests/test_gpu_forward_dynamics.py gives an fp32
    envelope), measured on the reference alone."""
    out = []
    for a32, a64 in zip(ref32[:2], ref64[:2]):
        b = np.broadcast_to(1e-5 * np.maximum(1.0, np.abs(a32).max(axis=1))[:, None], a32.shape).copy()
        if set_name in MEASURED_BOUND:
            with np.errstate(invalid="ignore"):
                b = np.fmax(b, 4.0 * np.abs(a32 - a64))
        out.append(b)
    return out


def _check_rollout(torch, cases, eng, set_name, table, R, s, what, step_loop=True, row_of=None):
    """One fused rollout of the first R robots of s (row_of: robot r of s is row row_of[r] of the 65-robot reference) against
    the oracle's closed loop, and against the host-driven step loop of the same engine.  Then the rollout build's control step on
    its own -- one control step, one tick: the q-double-dot it returns is the plain step's in exact arithmetic -- through the gate
    test_plain_step holds the plain build to.  (Over 0.12 s of plant time an error e of q-double-dot moves qd by 0.12 e and q by
    0.007 e: the closed loop's 1e-5 sees e from 1e-4 on, the gate from 1e-5 on or from twice the fp32 envelope.)
    Returns (rollout tag, step tag)."""
    K, sub, dt = (S.ROLLOUT[k] for k in ("n_control_steps", "substeps", "dt"))
    ref32, ref64 = _rollout_reference(cases, set_name, table)
    bq, bv = _rollout_bounds(set_name, ref32, ref64)
    rows = np.arange(R) if row_of is None else row_of
    kw = _kw(cases, set_name, table)
    obs = _obstacles(torch, eng, kw, R)
    q0, qd0, goal = _states(torch, s, R)
    qf, qdf = q0.clone(), qd0.clone()
    st = torch.zeros(R, dtype=torch.int32, device="cuda")
    eng.rollout(qf, qdf, goal, obstacles=obs, n_control_steps=K, substeps=sub, dt=dt, status=st)
    torch.cuda.synchronize()
    roll_name = eng.last_kernel()
    tame = S.tame(*ref32)[rows]
    assert S.tame(*ref32).mean() >= 0.95
    got_q, got_v = qf.cpu().numpy(), qdf.cpu().numpy()
    with np.errstate(invalid="ignore"):
        rq = (np.abs(got_q - ref32[0][rows]) / bq[rows]).max(axis=1)
        rv = (np.abs(got_v - ref32[1][rows]) / bv[rows]).max(axis=1)
    print(f"QB rollout {what} R {R}: tame {int(tame.sum())} of {R}; worst error / bound on the tame robots: q {rq[tame].max() if tame.any() else 0.0:.2e}, "
          f"qd {rv[tame].max() if tame.any() else 0.0:.2e}; largest bound / (1e-5 scale): "
          f"q {(bq[rows][tame] / (1e-5 * np.maximum(1.0, np.abs(ref32[0][rows][tame]).max(axis=1))[:, None])).max() if tame.any() else 1.0:.2f}, "
          f"qd {(bv[rows][tame] / (1e-5 * np.maximum(1.0, np.abs(ref32[1][rows][tame]).max(axis=1))[:, None])).max() if tame.any() else 1.0:.2f}")
    assert np.isfinite(got_q[tame]).all() and np.isfinite(got_v[tame]).all() and not (st.cpu().numpy()[tame] & D_STATUS_NONFINITE).any()
    assert (rq[tame] <= 1.0).all() and (rv[tame] <= 1.0).all(), \
        f"{what} R {R}: error / bound q {rq[tame].max():.3f}, qd {rv[tame].max():.3f} (robot {int(np.argmax(np.where(tame, np.fmax(rq, rv), 0)))})"
    if R == R_MAX and row_of is None:
        assert np.abs(ref32[0][tame] - s["q"][:R][tame]).max() > 1e-3   # the fleet moved
    exact, env, _ = _reference(cases, set_name, table)
    q1, qd1 = q0.clone(), qd0.clone()
    first = eng.rollout(q1, qd1, goal, obstacles=obs, n_control_steps=1, substeps=1, dt=dt)
    torch.cuda.synchronize()
    assert eng.last_kernel() == roll_name
    _gate(first.cpu().numpy(), exact, env, R, f"rollout, first control step, {what} [{roll_name.split('[build')[-1]}", rows=rows)
    step_name = None
    if step_loop:
        q, qd = q0.clone(), qd0.clone()
        for _ in range(K):
            qdd = eng.step(q, qd, goal, obstacles=obs)
            for _ in range(sub):
                qd = qd + dt * qdd
                q = q + dt * qd
        torch.cuda.synchronize()
        step_name = eng.last_kernel()
        eq, ev = (qf - q).abs().max().item(), (qdf - qd).abs().max().item()
        print(f"QB rollout-vs-step-loop {what} R {R}: |q| {eq:.3e} (< 1e-5), |qd| {ev:.3e} (< 1e-4)")
        assert torch.isfinite(q).all() and torch.isfinite(qf).all()
        assert eq < 1e-5 and ev < 1e-4, f"{what} R {R}: rollout against the step loop, q {eq:.3e}, qd {ev:.3e}"
    return roll_name, step_name


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("set_name,table", ROLLOUT_CASES)
def test_plain_rollout(torch_mod, cases, set_name, table, minw):
    """(c) The fused rollout (3 control steps of 4 plant ticks), the lean rollout builds (they exist at two and four waves).
    First against the ORACLE's closed loop, on the robots whose oracle trajectory is tame (finite, peak |qdd| <= 20; at least 0.95
    of the fleet, which tests/test_quad_build_scenes.py establishes on the CPU); then against the host-driven step loop of the
    same engine -- another build (the tags differ), which test_plain_step holds to the oracle."""
    desc, s = cases["sets"][set_name]
    eng = _engine(cases, set_name, minw)
    for R in FLEETS:
        roll, step = _check_rollout(torch_mod, cases, eng, set_name, table, R, s, f"{set_name} {table} minw {minw}")
        _assert_tag(roll, _rollout_tag(set_name, table, minw))
        _assert_tag(step, _plain_tag(set_name, table, minw))
        assert roll.split("[build")[-1] != step.split("[build")[-1]


@pytest.mark.parametrize("R", [65, 49153])
def test_rollout_register_caps(torch_mod, cases, R):
    """(d) The rollout half of test_gpu_kernel_variants.py test_quad_register_caps_agree_bitwise_at_fleet_sizes with caps that are
    two builds, (2, 4): at 65 robots and at 49 153 -- the first fleet size the dispatch itself gives four waves; 3 072 full waves
    and one robot.  Both are held to the oracle and to the step loop as in test_plain_rollout, not to each other: the contraction
    order of the pull-back is the compiler's per build, so bitwise agreement across caps is only observed (printed).  The large
    fleet is the 65-robot fleet over and over (65 and 16 are coprime: every robot meets every quad of a wave), so the 65-robot
    reference covers all of it."""
    torch = torch_mod
    set_name, table = "config3-auto", "33"
    desc, s65 = cases["sets"][set_name]
    row_of = np.arange(R) % R_MAX
    s = s65 if R == R_MAX else {k: np.ascontiguousarray(v[row_of]) for k, v in s65.items()}
    finals, tags = [], []
    for minw in (2, 4):
        eng = _engine(cases, set_name, minw)
        roll, _ = _check_rollout(torch, cases, eng, set_name, table, R, s, f"caps {set_name} {table} minw {minw}", row_of=row_of)
        _assert_tag(roll, _rollout_tag(set_name, table, minw))
        tags.append(roll.split("[build")[-1])
    assert tags[0] != tags[1]
    if R != R_MAX:   # what the dispatch picks at this size, unforced: the four-wave build
        eng = _engine_env(desc, RMP2_KERNEL="quad")
        roll, _ = _check_rollout(torch, cases, eng, set_name, table, R, s, f"caps {set_name} {table} dispatched", step_loop=False, row_of=row_of)
        _assert_tag(roll, _rollout_tag(set_name, table, 4))


NAN_CASES = [("rollout", "config3-auto"), ("rollout", "tree"), ("general", "config3-auto"), ("general", "tree"), ("general", "rank1-tree"),
             ("plain", "tree")]


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("flavour,set_name", NAN_CASES)
def test_a_nan_robot_stays_in_its_quad(torch_mod, cases, flavour, set_name, minw):
    """(e) 17 robots, q of robot 5 not a number: every other robot's results are the clean run's bit for bit, and robot 5 carries
    the non-finite status.  In the region pull-back the columns of a skipped row block are undefined registers; a reader that did
    not re-test anc_mask would pick up whatever they hold -- the NaN robot's values among them -- and an undefined register reaches
    a neighbour only through a quad broadcast.  The tree is the robot with skipped row blocks."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    n, R = desc.robot.n_dof, 17
    table = "none" if set_name.startswith("rank1") else "33"
    eng = _engine(cases, set_name, minw)
    obs = _obstacles(torch, eng, _kw(cases, set_name, table), R)
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
            want = _rollout_tag(set_name, table, minw)
        elif flavour == "general":
            res["M"] = torch.zeros((R, n, n), dtype=torch.float64, device="cuda")
            res["f"] = torch.zeros((R, n), dtype=torch.float64, device="cuda")
            res["qdd"] = eng.step(q, qd, goal, obstacles=obs, status=st, M=res["M"], f=res["f"])
            want = _general_tag(set_name, table, minw)
        else:
            res["qdd"] = eng.step(q, qd, goal, obstacles=obs, status=st)
            want = _plain_tag(set_name, table, minw)
        torch.cuda.synchronize()
        _assert_tag(eng.last_kernel(), want)
        runs.append(({k: v.cpu().numpy().copy() for k, v in res.items()}, st.cpu().numpy().copy()))
    (clean, st_clean), (dirty, st_dirty) = runs
    others = np.arange(R) != 5
    assert np.isfinite(clean["qdd"]).all() and not (st_clean & D_STATUS_NONFINITE).any()
    for k in clean:
        assert np.array_equal(clean[k][others].view(np.uint8), dirty[k][others].view(np.uint8)), f"{k} of a neighbour of the NaN robot changed"
    assert np.array_equal(st_clean[others], st_dirty[others])
    assert st_dirty[5] & D_STATUS_NONFINITE and np.isnan(dirty["qdd"][5]).all()

"""Every leaf policy AT its branch points and poles, on every mapping of robots to lanes and both resolves: the edge catalogue of
tests/leaf_edge_cases.py (fleets of R = 130: a partial last wave at 64, 16 and 4 robots per wave) against the CPU oracle.

The engine never decides what a row is: its class (pole / regular / stiff) comes from the two oracle builds
(tests/test_leaf_edges_host.py pins it), and every bound is a function of the oracle alone --

  exported system (`alone` sets)   |M_dev - M_64|_ij <= max(2 envM_ij, 1e-5 min(max_k |M_64|_ik, max_k |M_64|_kj)),
                                   |f_dev - f_64|_i <= max(2 envf_i, 1e-5 max_k |f_64|_k): leaf_edge_cases.system_envelope is the
                                   (M, f) analogue of oracle.fp32_envelope, 2 accuracy_gate's envelope_factor, 1e-5 the north star at
                                   the entry's own row and column scale; a row or column that is exactly 0 in fp64 is exactly 0 here
  qdd                              regular rows: clause A, B or E of oracle.accuracy_gate (and D for `alone` sets), at most 5 % of a
                                   fleet's regular rows through E or D; stiff rows: E; clause C is not offered
  poles                            non-finite on EVERY joint with RMP2_STATUS_NONFINITE, in every mapping, both resolves, both shapes

-- plus the exact structure the formulae have (listed at test_exact_structure), isolation of the ordinary rows from the edge rows
beside them, and equality of the answers with and without the export, through a rollout of dt = 0 and through the leaf protocol.
Each (fleet, mapping, resolve, shape, export) is launched once and shared by the tests that read it; the worst ratios per leaf and
mapping are printed by test_coverage (profiles/leaf_edges.txt keeps them).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import leaf_edge_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

FLEETS = list(L.BUILDERS)
KERNELS = ["", "hex", "quad", "lane"]
SOLVES = ["auto", "pinv"]
CASES = [(k, s) for k in FLEETS for s in L.fleet(k).shapes]
FINITE = [k for k in FLEETS if k != "joint_limits_coincide"]          # (that fleet has pole rows only: no system, no neighbours)
NEED_ENVELOPE = 0.05     # at most this share of a fleet's regular rows may need clause E or D

_RUNS = {}       # (key, kernel, solve, shape, export, plain, tag) -> dict(qdd, status, M, f, kernel, mapping)
_WORST = {}      # (fleet key, mapping) -> {"system": ratio, "qdd": ratio}


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def yardsticks():
    """(fleet, shape, solve) -> dict(r32, r64, env (qdd, M, f), cls, spread): the oracle's side, computed once per fleet and shape."""
    import oracle as O
    cache = {}

    def get(key, shape, solve):
        k = (key, shape, solve)
        if k not in cache:
            r32, r64 = L.references(key, shape, solve)
            cache[k] = dict(r32=r32, r64=r64, env=L.envelopes(key, shape, solve), cls=L.fleet(key).expected(shape),
                            spread=O.system_resolution(r32) if shape == "alone" else None)
        return cache[k]
    return get


def _engine(desc, kernel):
    """An engine under RMP2_KERNEL=kernel (read when the handle is created; '' = the dispatch by fleet size)."""
    from riemannian_motion_policies_amd.engine import Engine
    old = os.environ.get("RMP2_KERNEL")
    if kernel:
        os.environ["RMP2_KERNEL"] = kernel
    else:
        os.environ.pop("RMP2_KERNEL", None)
    try:
        return Engine(desc, 0)
    finally:
        if old is None:
            os.environ.pop("RMP2_KERNEL", None)
        else:
            os.environ["RMP2_KERNEL"] = old


def mapping_of(kernel_name):
    if "rmp2_step_hex_kernel" in kernel_name:
        return "hex"
    if "rmp2_step_quad_kernel" in kernel_name:
        return "quad"
    assert "rmp2_step_kernel" in kernel_name, kernel_name
    return "lane"


def _dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(torch, key, kernel, solve, shape, export, plain=False, obs=None, tag=None):
    """One launch of a fleet, made once: dict(qdd, status, M, f, kernel, mapping)."""
    k = (key, kernel, solve, shape, export, plain, tag)
    if k not in _RUNS:
        fl = L.fleet(key)
        q, qd, goal = (_dev(torch, a) for a in fl.inputs(plain))
        n = fl.n
        eng = _engine(fl.desc(shape, solve), kernel)          # (an error of the library on these descriptors fails the test)
        st = torch.zeros(L.R, dtype=torch.int32, device="cuda")
        M = torch.full((L.R, n, n), 7.0, dtype=torch.float64, device="cuda") if export else None
        f = torch.full((L.R, n), 7.0, dtype=torch.float64, device="cuda") if export else None
        o = fl.obstacles(plain) if obs is None else obs
        out = eng.step(q, qd, goal, obstacles=eng.obstacles(**{a: _dev(torch, v) for a, v in o.items()}) if o else None, status=st, M=M, f=f)
        torch.cuda.synchronize()
        name = eng.last_kernel()
        _RUNS[k] = dict(qdd=out.cpu().numpy(), status=st.cpu().numpy().astype(np.uint32), kernel=name, mapping=mapping_of(name),
                        M=None if M is None else M.cpu().numpy(), f=None if f is None else f.cpu().numpy())
    return _RUNS[k]


def _worst(key, mapping, what, ratio):
    w = _WORST.setdefault((key, mapping), {"system": 0.0, "qdd": 0.0})
    w[what] = max(w[what], float(ratio))


def _check_poles(what, run, cls):
    from riemannian_motion_policies_amd import descriptor as D
    pole = cls == "pole"
    got, st = run["qdd"], run["status"]
    bad = np.nonzero(pole & np.isfinite(got).any(axis=1))[0]
    assert bad.size == 0, f"{what}: pole rows {bad[:8]} answer a finite joint: {got[bad[:2]]} [{run['kernel']}]"
    bad = np.nonzero(pole & ((st & D.STATUS_NONFINITE) == 0))[0]
    assert bad.size == 0, f"{what}: pole rows {bad[:8]} without RMP2_STATUS_NONFINITE [{run['kernel']}]"
    bad = np.nonzero(~pole & (((st & D.STATUS_NONFINITE) != 0) | ~np.isfinite(got).all(axis=1)))[0]
    assert bad.size == 0, f"{what}: rows {bad[:8]} of a finite system answer non-finite or flagged [{run['kernel']}]"


def _check_qdd(what, key, run, y, shape):
    """The qdd clauses on one launch; returns the gate's summary."""
    import oracle as O
    cls = y["cls"]
    _check_poles(what, run, cls)
    g = O.accuracy_gate(run["qdd"], y["r32"], truth=y["r64"]["qdd64"], envelope=y["env"]["qdd"], system_spread=y["spread"])
    each = g["each"]
    regular, stiff = cls == "regular", cls == "stiff"
    ok_regular = each["a"] | each["b"] | each["e"] | each["d"]
    bad = np.nonzero(regular & ~ok_regular)[0]
    with np.errstate(invalid="ignore"):
        err = np.abs(run["qdd"] - y["r64"]["qdd64"]).max(axis=1)
        ratio = np.where(cls != "pole", err / np.maximum(np.maximum(2.0 * y["env"]["qdd"], 1e-5 * np.maximum(1.0, np.abs(y["r64"]["qdd64"]).max(axis=1))), 1e-300), 0.0)
    _worst(key, run["mapping"], "qdd", np.nanmax(ratio))
    names = L.fleet(key).names
    assert bad.size == 0, (f"{what}: regular rows outside A, B, E" + (", D" if shape == "alone" else "") +
                           f": {[(int(i), names[i], float(err[i]), float(y['env']['qdd'][i])) for i in bad[:6]]} [{run['kernel']}]")
    bad = np.nonzero(stiff & ~each["e"])[0]
    assert bad.size == 0, f"{what}: stiff rows outside E: {[(int(i), names[i], float(err[i]), float(y['env']['qdd'][i])) for i in bad[:6]]} [{run['kernel']}]"
    need = int((regular & ~(each["a"] | each["b"])).sum())
    s = O.gate_summary(g)
    print(f"{what} [{run['kernel']}]: {s}; regular rows through E / D: {need} of {int(regular.sum())}; worst |qdd - qdd64| / max(2 env, 1e-5 scale) {np.nanmax(ratio):.3f}")
    assert need <= NEED_ENVELOPE * regular.sum(), f"{what}: {need} of {int(regular.sum())} regular rows need clause E or D [{run['kernel']}]"
    return s


# ---- the exported system ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", SOLVES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key", FINITE)
def test_exported_system(torch_mod, yardsticks, key, kernel, solve):
    """`alone` sets: M= / f= of Engine.step is the leaf's own pulled-back system, entrywise against the fp64 oracle."""
    y = yardsticks(key, "alone", solve)
    run = _run(torch_mod, key, kernel, solve, "alone", export=True)
    fl = L.fleet(key)
    rows = y["cls"] != "pole"
    M64, f64 = y["r64"]["M"], y["r64"]["f"]
    bM, bf = L.system_bounds(y["r64"], y["env"]["M"], y["env"]["f"])
    with np.errstate(invalid="ignore"):
        eM, ef = np.abs(run["M"] - M64), np.abs(run["f"] - f64)
    assert np.isfinite(run["M"][rows]).all() and np.isfinite(run["f"][rows]).all(), f"{key}: non-finite exported system on a finite row [{run['kernel']}]"
    with np.errstate(invalid="ignore", divide="ignore"):
        rM = np.where(eM[rows] > 0, eM[rows] / bM[rows], 0.0)
        rf = np.where(ef[rows] > 0, ef[rows] / bf[rows], 0.0)
    worst = max(float(rM.max()), float(rf.max()))
    _worst(key, run["mapping"], "system", worst)
    print(f"{key} RMP2_KERNEL={kernel!r} {solve} [{run['kernel']}]: worst |M - M64| / bound {rM.max():.3f}, |f - f64| / bound {rf.max():.3f}")
    idx = np.nonzero(rows)[0]
    if rM.max() > 1.0:
        r, i, j = np.unravel_index(rM.argmax(), rM.shape)
        raise AssertionError(f"{key}: M[{i}][{j}] of row {idx[r]} {fl.names[idx[r]]!r} is {run['M'][idx[r], i, j]!r}, fp64 {M64[idx[r], i, j]!r}, "
                             f"{rM.max():.2f} of the bound {bM[idx[r], i, j]:.3e} [{run['kernel']}]")
    if rf.max() > 1.0:
        r, i = np.unravel_index(rf.argmax(), rf.shape)
        raise AssertionError(f"{key}: f[{i}] of row {idx[r]} {fl.names[idx[r]]!r} is {run['f'][idx[r], i]!r}, fp64 {f64[idx[r], i]!r}, "
                             f"{rf.max():.2f} of the bound {bf[idx[r], i]:.3e} [{run['kernel']}]")
    # a row or column that is exactly zero in fp64 AND in the plain fp32-leaf evaluation of the oracle is exactly zero on the device.
    # (Zero in fp64 alone is not asked at ONE place, by the oracle's own verdict: JointLimitAvoidance's band-edge rows, where the
    # fp32-leaf build -- like the lane kernel, which divides as it does -- lands 1e-8 inside the double root of the spline that fp64
    # puts it outside of; that flip is held by the envelope above.)
    M32, f32 = y["r32"]["M"], y["r32"]["f"]
    zrow = (M64 == 0).all(axis=2) & (M32 == 0).all(axis=2) & rows[:, None]
    zcol = (M64 == 0).all(axis=1) & (M32 == 0).all(axis=1) & rows[:, None]
    assert (run["M"][zrow] == 0).all(), f"{key}: a row of M that is 0 in fp64 is not on the device [{run['kernel']}]"
    assert (np.swapaxes(run["M"], 1, 2)[zcol] == 0).all(), f"{key}: a column of M that is 0 in fp64 is not on the device [{run['kernel']}]"
    zf = (f64 == 0).all(axis=1) & (f32 == 0).all(axis=1) & rows
    assert (run["f"][zf] == 0).all(), f"{key}: an f that is 0 in fp64 is not on the device [{run['kernel']}]"


@pytest.mark.parametrize("solve", SOLVES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_structure(torch_mod, kernel, solve):
    """What the formulae give exactly, bit for bit on the exported system: JointDamping at rest M == P[2] I, f == 0; the velocity cap
    with every joint below the cutoff f == 0; TargetPolicy on the identity map at the goal and at rest M == I, f == 0;
    JointLimitAvoidance: the column of every joint outside its band is 0; ConfigurationSpaceBiasing at the goal and at rest f == 0."""
    from riemannian_motion_policies_amd import configs as Cf
    torch = torch_mod
    run = _run(torch, "joint_damping", kernel, solve, "alone", export=True)
    rows = L.fleet("joint_damping").groups["at_rest"]
    assert np.array_equal(run["M"][rows], np.broadcast_to(float(np.float32(Cf.JOINT_DAMPING_PARAMS[2])) * np.eye(9), (len(rows), 9, 9))), run["kernel"]
    assert (run["f"][rows] == 0).all(), run["kernel"]
    for key in ("velocity_cap", "velocity_cap_gantry", "velocity_cap_two_joint"):
        run = _run(torch, key, kernel, solve, "alone", export=True)
        rows = L.fleet(key).groups["below_cutoff"]
        assert (run["f"][rows] == 0).all(), (key, run["kernel"], run["f"][rows])
        M = run["M"][rows]
        assert (M[:, ~np.eye(L.fleet(key).n, dtype=bool)] == float(np.float32(Cf.JOINT_VELOCITY_CAP_PARAMS[3]))).all(), (key, run["kernel"])   # quirk Q4
    run = _run(torch, "target_policy_identity", kernel, solve, "alone", export=True)
    rows = L.fleet("target_policy_identity").groups["identity_metric_zero_force"]
    assert np.array_equal(run["M"][rows], np.broadcast_to(np.eye(9), (len(rows), 9, 9))) and (run["f"][rows] == 0).all(), run["kernel"]
    run = _run(torch, "config_space_biasing", kernel, solve, "alone", export=True)
    assert (run["f"][L.fleet("config_space_biasing").groups["zero_force"]] == 0).all(), run["kernel"]
    for key in ("joint_limits", "joint_limits_band_free"):
        fl = L.fleet(key)
        run = _run(torch, key, kernel, solve, "alone", export=True)
        span = fl.hi - fl.lo
        d = np.minimum((fl.hi - fl.q) / span, (fl.q - fl.lo) / span)          # fp32, as the leaf forms it
        outside = d > np.float32(0.15) * (1 + 1e-5)                             # clear of the rounding of d at the band's edge
        cols = np.broadcast_to(outside[:, None, :], run["M"].shape)
        assert (run["M"][cols] == 0).all(), f"{key}: a column of a joint outside its band is not 0 [{run['kernel']}]"
        assert outside.all(axis=1).sum() >= 2      # (rows with no joint in a band at all: M == 0)


@pytest.mark.parametrize("solve", SOLVES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", list(L.OBSTACLE_TABLES))
def test_an_obstacle_out_of_reach_contributes_exactly_nothing(torch_mod, name, kernel, solve):
    """At and beyond the modulation radius, and for a point that recedes with z > 25 ln 2: M and f (alone) and qdd (beside the
    damping leaf) equal, bit for bit, those of the same fleet with the table moved away."""
    import link_pair_scene as S
    torch = torch_mod
    key = "obstacle_" + name
    fl = L.fleet(key)
    rows = fl.groups["zero_leaf"]
    if "spheres" in fl.obs:
        away = dict(fl.obs, spheres=S.moved_away(fl.obs["spheres"]))
    else:
        away = dict(p_link=fl.obs["p_link"], p_obs=fl.obs["p_obs"] + np.array([0, 0, S.FAR_Z], np.float32))
    a = _run(torch, key, kernel, solve, "alone", export=True)
    b = _run(torch, key, kernel, solve, "alone", export=True, obs=away, tag="away")
    assert (b["M"] == 0).all() and (b["f"] == 0).all() and (b["qdd"] == 0).all(), b["kernel"]
    assert (a["M"][rows] == 0).all() and (a["f"][rows] == 0).all(), (key, [fl.names[i] for i in rows], a["M"][rows].max(axis=(1, 2)), a["kernel"])
    assert np.array_equal(a["qdd"][rows], b["qdd"][rows])
    a = _run(torch, key, kernel, solve, "damped", export=False)
    b = _run(torch, key, kernel, solve, "damped", export=False, obs=away, tag="away")
    assert a["kernel"] == b["kernel"]
    assert np.array_equal(a["qdd"][rows].view(np.uint32), b["qdd"][rows].view(np.uint32)), (key, a["kernel"])
    assert np.array_equal(a["status"][rows], b["status"][rows])


# ---- qdd, poles -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", SOLVES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key,shape", CASES)
def test_qdd_and_poles(torch_mod, yardsticks, key, shape, kernel, solve):
    """The plain step: every regular row within A, B or E (D for `alone` sets), every stiff row within E, every pole row NaN on every
    joint with RMP2_STATUS_NONFINITE; and the export does not change the answer -- bit for bit where rmp2_last_kernel names the same
    kernel, each held to the clauses on its own where the dispatch moves the exporting call to another one.  (The quad mapping's
    structured identity loop and its general loop count as different kernels: an exporting call keeps the general loop, whose
    arithmetic is another; the four structured kinds are therefore held to the clauses there, not to the bits.)"""
    y = yardsticks(key, shape, solve)
    what = f"{key} {shape} RMP2_KERNEL={kernel!r} {solve}"
    run = _run(torch_mod, key, kernel, solve, shape, export=False)
    _check_qdd(what, key, run, y, shape)
    exp = _run(torch_mod, key, kernel, solve, shape, export=True)
    if exp["kernel"] == run["kernel"]:
        assert np.array_equal(exp["qdd"].view(np.uint32), run["qdd"].view(np.uint32)), f"{what}: the export changes qdd [{run['kernel']}]"
        assert np.array_equal(exp["status"], run["status"]), f"{what}: the export changes the status [{run['kernel']}]"
    else:
        _check_qdd(what + " with export", key, exp, y, shape)


@pytest.mark.parametrize("solve", SOLVES)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("key,shape", [c for c in CASES if c[0] in FINITE])
def test_edge_rows_do_not_touch_their_neighbours(torch_mod, key, shape, kernel, solve):
    """The same fleet with every edge row replaced by an ordinary one: the ordinary rows' qdd, status, M and f keep their bits (for
    joint_limits_band_free the edge rows are the ONE row per quad wave that is inside a band: the wave-wide column skip)."""
    fl = L.fleet(key)
    export = shape == "alone"
    a = _run(torch_mod, key, kernel, solve, shape, export=export)
    b = _run(torch_mod, key, kernel, solve, shape, export=export, plain=True)
    rest = ~fl.edge
    assert a["kernel"] == b["kernel"]
    assert np.isfinite(b["qdd"]).all(), f"{key} {shape}: the plain fleet has a non-finite row [{b['kernel']}]"
    for name in ("qdd", "status") + (("M", "f") if export else ()):
        x, z = a[name][rest], b[name][rest]
        same = np.array_equal(x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64), z.view(np.uint32 if z.dtype.itemsize == 4 else np.uint64))
        assert same, f"{key} {shape} RMP2_KERNEL={kernel!r} {solve}: {name} of ordinary rows {np.nonzero((x != z).reshape(len(x), -1).any(axis=1))[0][:8]} (among the ordinary ones) moves with the edge rows [{a['kernel']}]"


# ---- rollout ----------------------------------------------------------------------------------------------------------------------
ROLLOUT_FLEETS = ["velocity_cap", "joint_damping", "cspace_biasing", "config_space_biasing", "joint_limits", "target_policy_identity",
                  "obstacle_K1", "obstacle_K64_last"]


@pytest.mark.parametrize("solve", SOLVES)
@pytest.mark.parametrize("kernel", ["", "hex", "quad"])
@pytest.mark.parametrize("key", ROLLOUT_FLEETS)
def test_rollout_of_no_time_is_the_plain_step(torch_mod, yardsticks, key, kernel, solve):
    """Engine.rollout(n_control_steps=1, substeps=1, dt=0.0) leaves q and qd of every row with a finite answer alone and returns the plain step's qdd -- bit for bit
    where the same kernel ran, pole rows included; where the rollout takes another kernel than the plain step, held to the clauses.
    The state of a POLE row is not asked to stay: qd + 0 * NaN is NaN, and that is the contract -- a robot whose answer is NaN has no
    next state -- rather than an accident of the integrator."""
    torch = torch_mod
    fl = L.fleet(key)
    shape = "damped" if "damped" in fl.shapes else "alone"
    plain = _run(torch, key, kernel, solve, shape, export=False)
    q, qd, goal = (_dev(torch, a) for a in fl.inputs())
    q0, qd0 = q.clone(), qd.clone()
    eng = _engine(fl.desc(shape, solve), kernel)
    st = torch.zeros(L.R, dtype=torch.int32, device="cuda")
    out = eng.rollout(q, qd, goal, obstacles=eng.obstacles(**{a: _dev(torch, v) for a, v in fl.obs.items()}) if fl.obs else None,
                      n_control_steps=1, substeps=1, dt=0.0, status=st)
    torch.cuda.synchronize()
    name = eng.last_kernel()
    # (a pole row's qd + 0 * NaN is NaN: it has no next state; every other row keeps its bits)
    keep = torch.from_numpy(fl.expected(shape) != "pole").cuda()
    # (by value: qd = -0 comes back as -0 + 0 * qdd = +0)
    assert torch.equal(q[keep], q0[keep]) and torch.equal(qd[keep], qd0[keep])
    run = dict(qdd=out.cpu().numpy(), status=st.cpu().numpy().astype(np.uint32), kernel=name, mapping=mapping_of(name))
    print(f"rollout {key} {shape} RMP2_KERNEL={kernel!r} {solve}: [{name}] against the plain step's [{plain['kernel']}]")
    if name == plain["kernel"]:
        assert np.array_equal(run["qdd"].view(np.uint32), plain["qdd"].view(np.uint32)), f"rollout {key}: qdd differs from the plain step's [{name}]"
        assert np.array_equal(run["status"], plain["status"])
    else:
        _check_qdd(f"rollout {key} {shape} RMP2_KERNEL={kernel!r} {solve}", key, run, yardsticks(key, shape, solve), shape)


# ---- the leaf protocol --------------------------------------------------------------------------------------------------------------
def _leaf(key):
    from riemannian_motion_policies_amd import configs as Cf, rmp, rmp2
    fl = L.fleet(key)
    return {
        "velocity_cap": lambda: rmp2.JointVelocityCap(*Cf.JOINT_VELOCITY_CAP_PARAMS),
        "joint_damping": lambda: rmp2.JointDamping(*Cf.JOINT_DAMPING_PARAMS),
        "cspace_biasing": lambda: rmp2.CSpaceBiasing(Cf.CSPACE_BIASING_GOAL, *Cf.CSPACE_BIASING_PARAMS),
        "joint_limits": lambda: rmp.JointLimitAvoidance(fl.lo, fl.hi, *Cf.JOINT_LIMIT_PARAMS),
        "joint_limits_band_free": lambda: rmp.JointLimitAvoidance(fl.lo, fl.hi, *Cf.JOINT_LIMIT_PARAMS),
        "config_space_biasing": lambda: rmp.ConfigurationSpaceBiasing(*Cf.PANDA04_CONFIG_SPACE_BIASING_PARAMS[:2], q0=Cf.PANDA04_Q0, name="csb",
                                                                      w=Cf.PANDA04_CONFIG_SPACE_BIASING_PARAMS[2]),
    }[key]()


@pytest.mark.parametrize("key", ["velocity_cap", "joint_damping", "cspace_biasing", "config_space_biasing", "joint_limits", "joint_limits_band_free"])
def test_leaf_protocol_at_the_edges(torch_mod, yardsticks, key):
    """rmp2_leaf_evaluate (the rmp2.* / rmp.* leaf classes' evaluate) on the identity-map fleets: on the identity map the `alone`
    system IS the leaf's (A, A xdd), so A is held to M's bounds and A xdd (formed in fp64 from the device's A and xdd) to f's; pole
    rows answer a non-finite A or xdd."""
    y = yardsticks(key, "alone", "auto")
    fl = L.fleet(key)
    xdd, A = _leaf(key).evaluate(fl.q, fl.qd)
    xdd, A = (np.asarray(v.cpu() if hasattr(v, "cpu") else v, np.float64) for v in (xdd, A))
    A = np.broadcast_to(A, (L.R, fl.n, fl.n))
    pole = y["cls"] == "pole"
    assert (~(np.isfinite(A).all(axis=(1, 2)) & np.isfinite(xdd).all(axis=1)))[pole].all(), f"{key}: a pole row with finite leaf values"
    rows = ~pole
    assert np.isfinite(A[rows]).all() and np.isfinite(xdd[rows]).all()
    bM, bf = L.system_bounds(y["r64"], y["env"]["M"], y["env"]["f"])
    eM = np.abs(A - y["r64"]["M"])[rows]
    ef = np.abs(np.einsum("rij,rj->ri", np.where(rows[:, None, None], A, 0.0), np.where(rows[:, None], xdd, 0.0)) - y["r64"]["f"])[rows]
    with np.errstate(invalid="ignore", divide="ignore"):
        rM = np.where(eM > 0, eM / bM[rows], 0.0)
        rf = np.where(ef > 0, ef / bf[rows], 0.0)
    _worst(key, "leaf protocol", "system", max(rM.max(), rf.max()))
    print(f"leaf protocol {key}: worst |A - M64| / bound {rM.max():.3f}, |A xdd - f64| / bound {rf.max():.3f}")
    assert rM.max() <= 1.0 and rf.max() <= 1.0, (key, float(rM.max()), float(rf.max()), np.nonzero(rows)[0][np.unravel_index(rM.argmax(), rM.shape)[0]])


def _leaf_reference(fn, arrays, rows_alone):
    """(xdd64, A64, env_xdd, env_A) of a leaf function of the autograd oracle on fp32 inputs: its fp64 evaluation, and the largest
    |fp32 evaluation - fp64 evaluation| over the plain inputs and 16 draws moved by one unit-scale fp32 rounding (oracle.fp32_envelope's
    jiggle, seed 0).  rows_alone: the reference's norms are global (TargetPolicy) -- one row per call."""
    import torch
    rng = np.random.default_rng(0)
    eps = np.float64(2.0 ** -23)

    def jiggle(a):
        a = a.astype(np.float64)
        return (a + rng.choice(np.array([-1.0, 1.0]), a.shape) * eps * np.maximum(np.abs(a), 1.0)).astype(np.float32)

    def ev(arrs, dtype):
        ts = [torch.tensor(np.asarray(a), dtype=dtype) for a in arrs]
        if rows_alone:
            outs = [fn(*[t[b:b + 1] for t in ts]) for b in range(len(ts[0]))]
            return tuple(np.concatenate([np.asarray(o[i].numpy(), np.float64) for o in outs]) for i in (0, 1))
        o = fn(*ts)
        return np.asarray(o[0].numpy(), np.float64), np.asarray(o[1].numpy(), np.float64)

    x64, A64 = ev(arrays, torch.float64)
    ex, eA = np.zeros_like(x64), np.zeros_like(A64)
    for draw in range(17):
        x32, A32 = ev(arrays if draw == 0 else [jiggle(a) for a in arrays], torch.float32)
        with np.errstate(invalid="ignore"):
            ex, eA = np.fmax(ex, np.abs(x32 - x64)), np.fmax(eA, np.abs(A32 - A64))
    return x64, A64, ex, eA


@pytest.mark.parametrize("kind", ["obstacle_avoidance", "target_attractor", "target_policy"])
def test_leaf_protocol_of_the_distance_and_position_leaves(torch_mod, kind):
    """The 1-d leaf (ObstacleAvoidance on a distance and its rate) and the 3-d leaves (TargetAttractor, TargetPolicy on a position)
    through rmp2_leaf_evaluate at their edges -- d == 0, negative (clamped), at and 2^-10 beyond the modulation radius, xd == 0,
    z = xd / gate_len 64 steps either side of 25 ln 2; x == goal, 2^-20 beside it, at rest -- between seeded ordinary rows, against the
    fp64 evaluation of the autograd oracle's leaf function, entrywise within max(2 x envelope, 1e-5 x the row's scale).  None of these
    is a pole of the LEAF (the poles of a distance leaf are its task map's); every value must be finite."""
    import torch_autodiff_oracle as TA
    from riemannian_motion_policies_amd import configs as Cf, rmp, rmp2, taskmap
    F = np.float32
    rng = np.random.default_rng(31)
    ident = taskmap.IdentityTaskmap()
    f32p = lambda P: [float(F(p)) for p in P]  # noqa: E731
    if kind == "obstacle_avoidance":
        P = Cf.OBSTACLE_AVOIDANCE_PARAMS
        x = rng.uniform(0.01, 0.7, (L.R, 1)).astype(F)
        v = rng.uniform(-0.3, 0.3, (L.R, 1)).astype(F)
        gate = F(F(P[4]) * L.Z_GATE)
        edges = [(0.0, -0.25), (0.0, 0.0), (-0.0625, -0.25), (0.5, -0.25), (F(0.5) + F(2.0 ** -10), -0.25), (L.steps(0.5, -1), -0.25),
                 (0.25, 0.0), (0.25, -0.0), (0.25, L.steps(gate, -64)), (0.25, L.steps(gate, 64)), (0.001, -0.3), (0.25, -3.0)]
        for k, (d, dd) in enumerate(edges):
            x[L.slot(k), 0], v[L.slot(k), 0] = F(d), F(dd)
        leaf = rmp2.ObstacleAvoidance(*P, taskmap=ident, name="oa")
        fn, arrays, alone = (lambda a, b: TA.obstacle_avoidance(f32p(P), a, b)), [x, v], False
        zero = (x[:, 0] > F(0.5)) | (v[:, 0] > gate)
    else:
        goal = np.array([0.375, -0.25, 0.5], F)
        x = (goal + rng.uniform(-0.6, 0.6, (L.R, 3))).astype(F)
        v = rng.uniform(-0.3, 0.3, (L.R, 3)).astype(F)
        z3 = np.zeros(3, F)
        edges = [(goal, None), (goal, z3), (goal + F(2.0 ** -20), None), (goal + np.array([0, 2.0 ** -20, 0], F), z3), (None, z3),
                 (goal + np.array([1e-20, 0, 0], F), None), (goal - F(2.0 ** -20), -z3)]
        for k, (xx, vv) in enumerate(edges):
            if xx is not None:
                x[L.slot(k)] = xx
            if vv is not None:
                v[L.slot(k)] = vv
        if kind == "target_attractor":
            P = Cf.TARGET_ATTRACTOR_PARAMS
            leaf = rmp2.TargetAttractor(list(goal), *P, taskmap=ident)
            fn, alone = (lambda a, b: TA.target_attractor(f32p(P), goal, a, b)), False
        else:
            P = Cf.TARGET_POLICY_PARAMS
            leaf = rmp.TargetPolicy(*P, goal=list(goal), taskmap=ident)
            fn, alone = (lambda a, b: TA.target_policy(f32p(P), goal, a, b)), True
        arrays, zero = [x, v], None
    xdd, A = leaf.evaluate(x, v)
    xdd, A = (np.asarray(t.cpu() if hasattr(t, "cpu") else t, np.float64) for t in (xdd, A))
    x64, A64, ex, eA = _leaf_reference(fn, arrays, alone)
    xdd, A = xdd.reshape(x64.shape), A.reshape(A64.shape)
    assert np.isfinite(xdd).all() and np.isfinite(A).all() and np.isfinite(x64).all() and np.isfinite(A64).all(), kind
    bx = np.fmax(2.0 * ex, 1e-5 * np.abs(x64).reshape(L.R, -1).max(axis=1).reshape((L.R,) + (1,) * (x64.ndim - 1)))
    bA = np.fmax(2.0 * eA, 1e-5 * np.abs(A64).reshape(L.R, -1).max(axis=1).reshape((L.R,) + (1,) * (A64.ndim - 1)))
    with np.errstate(invalid="ignore", divide="ignore"):
        rx = np.where(np.abs(xdd - x64) > 0, np.abs(xdd - x64) / bx, 0.0)
        rA = np.where(np.abs(A - A64) > 0, np.abs(A - A64) / bA, 0.0)
    _worst(kind, "leaf protocol", "system", max(rx.max(), rA.max()))
    print(f"leaf protocol {kind}: worst |xdd - xdd64| / bound {rx.max():.3f} (row {np.unravel_index(rx.argmax(), rx.shape)[0]}), "
          f"|A - A64| / bound {rA.max():.3f} (row {np.unravel_index(rA.argmax(), rA.shape)[0]})")
    assert rx.max() <= 1.0 and rA.max() <= 1.0, (kind, float(rx.max()), float(rA.max()))
    if zero is not None:      # beyond the modulation radius, or receding beyond the gate: the metric is an exact 0
        assert (A.reshape(L.R)[zero] == 0).all() and zero.sum() >= 3


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solve", SOLVES)
def test_coverage(torch_mod, solve):
    """Every (leaf kind, mapping) pair include/rmp2.h says is carried -- the hex, quad and lane mappings carry every kind of the
    catalogue -- runs, judged by rmp2_last_kernel, and the quad mapping's structured identity loop runs for the four structured kinds
    (beside the damping leaf on the Panda, no export).  The launches are the module's own (made here where another test has not made
    them yet: the test does not depend on which tests ran before it).  Prints what ran and the worst ratios recorded so far."""
    from riemannian_motion_policies_amd import descriptor as D
    from test_gpu_identity_leaf_paths import STRUCTURED
    ran, structured = {}, {}
    for key in FLEETS:
        fl = L.fleet(key)
        for shape in fl.shapes:
            for kernel in KERNELS:
                run = _run(torch_mod, key, kernel, solve, shape, export=False)
                for kind in fl.kinds:
                    ran.setdefault((kind, run["mapping"]), set()).add(run["kernel"])
                if key in L.STRUCTURED and kernel == "quad" and shape == fl.shapes[-1]:
                    structured[key] = run["kernel"]
    kinds = {D.LEAF_TARGET_ATTRACTOR: "TargetAttractor", D.LEAF_JOINT_VELOCITY_CAP: "JointVelocityCap", D.LEAF_JOINT_DAMPING: "JointDamping",
             D.LEAF_OBSTACLE_AVOIDANCE: "ObstacleAvoidance", D.LEAF_CSPACE_BIASING: "CSpaceBiasing", D.LEAF_TARGET_POLICY: "TargetPolicy",
             D.LEAF_JOINT_LIMIT_AVOIDANCE: "JointLimitAvoidance", D.LEAF_CONFIG_SPACE_BIASING: "ConfigurationSpaceBiasing",
             D.LEAF_COLLISION_AVOIDANCE: "CollisionAvoidance"}
    missing = []
    for kind, label in kinds.items():
        for m in ("hex", "quad", "lane"):
            names = ran.get((kind, m), set())
            print(f"coverage {solve} {label:26s} {m:5s}: {sorted(names) if names else 'NOT RUN'}")
            if not names:
                missing.append((label, m))
    for key in L.STRUCTURED:
        print(f"coverage {solve} structured loop, {key}: {structured[key]}")
        if STRUCTURED not in structured[key]:
            missing.append((key, "quad, structured loop"))
    for (key, m), w in sorted(_WORST.items()):
        print(f"worst ratio {key:28s} {m:14s}: system {w['system']:.3f}  qdd {w['qdd']:.3f}")
    assert not missing, f"(leaf kind, mapping) pairs that never ran: {missing}"

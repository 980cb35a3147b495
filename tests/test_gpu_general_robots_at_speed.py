"""The step kernels' own kinematics -- hex: pointer jumping with ancestor sums, quad: quad permutes, lane: the walk; none of them
the oracle's recursion -- on general robots at |qd| <= 2, where the curvature term c = Jdot qd dominates the pulled-back force
(every other general-robot test draws qd from +-0.1, where it is 1e-3 of it).  The oracle they are compared with is pinned on these
robots by tests/test_kinematics_reference_host.py.

Robots: the seed-0 random trees with at most 9 dofs, the prismatic sandwich, the 32-frame chain with its order cut to 9 dofs, and
(hex only) the 16-dof tree.  Leaves: a target attractor on the deepest frame, a target policy on a frame of another branch where
there is one, joint damping, an obstacle-avoidance distance leaf on each of two frames with six spheres.  Fleet: 130 robots, 8
distinct states tiled and permuted; state 0 is at rest (qd = 0, so c = 0): a failure at speed that vanishes at rest points at the
curvature term."""
import os

import numpy as np
import pytest

import kinematics_reference as KR

pytestmark = pytest.mark.gpu

R = 130
DISTINCT = 8
NAMES = {"hex": "rmp2_step_hex_kernel", "quad": "rmp2_step_quad_kernel", "lane": "rmp2_step_kernel ("}
# robots a mapping declines (another mapping answers, or the step is refused as unsupported): none of these robots
DECLINED = {"hex": [], "quad": [], "lane": []}
ATT = [0.3, 0.6, 0.075, 0.05, 0.03, 1.0, 0.5, 1.0, 0.02]
OA = [0.0, 50.0, 0.04, 0.01, 0.01, 800.0, 0.01, 0.5, 1.0, 0.02, 0.001]


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _leaf_frames(table):
    """(deepest frame, a frame of another branch or None, second obstacle frame)."""
    chain = lambda f: KR._chain({"parent": [int(p) for p in table.parent]}, f)
    F = table.n_frames
    deepest = max(range(F), key=lambda f: (len(chain(f)), f))
    on_chain = set(chain(deepest))
    others = [f for f in range(F) if f not in on_chain and table.ancestor_dof_mask(f) & 0xFFFF]
    other = max(others, key=lambda f: (len(chain(f)), f)) if others else None
    c = chain(deepest)
    second = other if other is not None else c[(len(c) - 1) // 2]
    return deepest, other, second


def build_cases(tmp_dir):
    """name -> dict(desc, q, qd, goal, sph, n, hex_only); the oracle's side is added by the `cases` fixture."""
    import dynamics_reference as DR
    from riemannian_motion_policies_amd import descriptor as D, urdf as U
    out = {}
    for sc in KR.scenes(tmp_dir):
        order = sc.order
        if sc.name == "wrist":
            continue
        if sc.name == "chain32":
            order = order[:9]
        elif sc.n_dof > 9 and sc.name != "dof16":
            continue
        table = U.compile_urdf(sc.path, order)
        n = table.n_dof
        deepest, other, second = _leaf_frames(table)
        specs = [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, deepest, ATT, goal_len=3)]
        if other is not None:
            specs.append(D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_FK_POSITION, other, [0.1, 0.5, 0.1], goal_len=3))
        specs.append(D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, [1.0, 0.005, 0.3]))
        specs += [D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, fr, OA) for fr in (deepest, second)]
        desc = D.build_desc(table, specs)
        rng = np.random.default_rng(500 + len(out))
        q8, qd8, _ = DR.random_states(rng, table, DISTINCT, qd_max=KR.QD_MAX)
        qd8[0] = 0.0
        g8 = rng.uniform(-0.5, 0.5, (DISTINCT, desc.goal_floats)).astype(np.float32)
        idx = rng.permutation(np.arange(R) % DISTINCT)
        sph = np.concatenate([rng.uniform(-1, 1, (6, 3)) + [0, 0, 6.0], rng.uniform(0.05, 0.1, (6, 1))], axis=1).astype(np.float32)
        out[sc.name] = dict(desc=desc, q=q8[idx], qd=qd8[idx], goal=g8[idx], sph=sph, n=n, rest=idx == 0, hex_only=n > 9,
                            frames=(deepest, other, second), n_frames=table.n_frames)
    return out


def oracle_side(case):
    """The oracle's reference-precision step, its fp64 step, the bound on f, and the gate's resolutions."""
    import oracle as O
    c = case
    ref = O.step(c["desc"], c["q"], c["qd"], c["goal"], spheres=c["sph"])
    r64 = O.step(c["desc"], c["q"], c["qd"], c["goal"], precision="f64", spheres=c["sph"])
    # f: 4 x what the oracle's own f32 build misses its f64 build by on this fleet, floored at 5e-6 max(1, |f|)
    f_tol = max(4.0 * np.abs(ref["f"] - r64["f"]).max(), 5e-6 * max(1.0, np.abs(ref["f"]).max()))
    res = O.fp32_resolution(c["desc"], c["q"], c["qd"], c["goal"], spheres=c["sph"])
    return dict(ref=ref, r64=r64, f_tol=f_tol, res=res, sys_res=O.system_resolution(ref))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    out = build_cases(tmp_path_factory.mktemp("speed"))
    for c in out.values():
        c.update(oracle_side(c))
    return out


def _engine(desc, kernel):
    from riemannian_motion_policies_amd.engine import Engine
    old = os.environ.get("RMP2_KERNEL")
    os.environ["RMP2_KERNEL"] = kernel
    try:
        return Engine(desc, 0)
    finally:
        if old is None:
            del os.environ["RMP2_KERNEL"]
        else:
            os.environ["RMP2_KERNEL"] = old


def test_the_fleets_are_what_they_claim(cases):
    """What the file is for: fast states on every robot, rows at rest beside them, the deep chain, both trees."""
    assert len(cases) >= 8 and "sandwich" in cases and "chain32" in cases and "dof16" in cases
    assert cases["chain32"]["n_frames"] == 32 and cases["chain32"]["n"] == 9 and cases["dof16"]["n"] == 16
    assert sum(c["frames"][1] is not None for c in cases.values()) >= 4     # robots with a policy on another branch
    for name, c in cases.items():
        assert np.abs(c["qd"]).max() > 1.0 and c["rest"].sum() >= 10 and not c["qd"][c["rest"]].any(), name


@pytest.mark.parametrize("kernel", ["hex", "quad", "lane"])
def test_step_at_speed(torch_mod, cases, kernel):
    import oracle as O
    from riemannian_motion_policies_amd import _native
    torch = torch_mod
    ran, declined, problems, worst = [], [], [], dict(M=0.0, f=0.0, aside=0.0)
    for name, c in cases.items():
        if c["hex_only"] and kernel != "hex":
            continue
        n = c["n"]
        eng = _engine(c["desc"], kernel)
        M = torch.empty((R, n, n), dtype=torch.float64, device="cuda")
        f = torch.empty((R, n), dtype=torch.float64, device="cuda")
        try:
            out = eng.step(torch.from_numpy(c["q"]), torch.from_numpy(c["qd"]), torch.from_numpy(c["goal"]),
                           obstacles=eng.obstacles(spheres=torch.from_numpy(c["sph"])), M=M, f=f)
            torch.cuda.synchronize()
        except _native.Rmp2Error as e:
            if e.code != _native.ERR_UNSUPPORTED:
                raise
            declined.append(name)
            eng.close()
            continue
        named = eng.last_kernel()
        got, Mg, fg = out.cpu().numpy(), M.cpu().numpy(), f.cpu().numpy()
        eng.close()
        if NAMES[kernel] not in named:
            declined.append(name)
            continue
        ran.append(name)
        ref, rest = c["ref"], c["rest"]

        def split(err_rows, tol):   # "at speed" / "at rest" verdict for the message
            bad = err_rows > tol
            return f"{int((bad & ~rest).sum())} robots at speed, {int((bad & rest).sum())} at rest (qd = 0: c = 0) outside"

        eM = np.abs(Mg - ref["M"]).reshape(R, -1).max(axis=1)
        tM = 5e-6 * max(1.0, np.abs(ref["M"]).max())
        ef = np.abs(fg - ref["f"]).max(axis=1)
        worst["M"] = max(worst["M"], eM.max() / tM)
        worst["f"] = max(worst["f"], ef.max() / c["f_tol"])
        print(f"{kernel} {name}: n {n}, M err {eM.max():.2e} (bound {tM:.2e}), f err {ef.max():.2e} (bound {c['f_tol']:.2e})")
        if not (eM <= tM).all():
            problems.append(f"{name}: M {eM.max():.3e} > {tM:.3e}; {split(eM, tM)}")
        if not (ef <= c["f_tol"]).all():
            where = split(ef, c["f_tol"])
            hint = " -- vanishes at rest: the curvature term c = Jdot qd" if not (ef > c["f_tol"])[rest].any() else ""
            problems.append(f"{name}: f {ef.max():.3e} > {c['f_tol']:.3e}; {where}{hint}")
        v = O.accuracy_gate(got, ref, spread=c["res"], system_spread=c["sys_res"])
        aside = 1.0 - v["a"].mean()
        worst["aside"] = max(worst["aside"], aside)
        if not v["ok"].all():
            problems.append(f"{name}: qdd outside the gate: {O.gate_summary(v)}; {split(~v['ok'] * 1.0, 0.5)}")
        if aside > 0.05:
            problems.append(f"{name}: {aside:.1%} of the robots beyond the gate's north star (cap 5 %): {O.gate_summary(v)}")
    print(f"{kernel}: ran {len(ran)} robots {ran}, declined {declined}; worst M {worst['M']:.2f} x bound, f {worst['f']:.2f} x bound, "
          f"set aside {worst['aside']:.1%}")
    assert not problems, problems
    assert declined == DECLINED[kernel], declined
    assert len(ran) >= 6, ran

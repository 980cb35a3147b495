"""The tail of the quad step -- structured identity leaves, elimination, certificate -- of the four-wave builds against the fp64
oracle, on small fleets.

The four-wave lean builds carry their own form of the identity phase (csrc/rmp2_quad.h kTailOpaqueDof: the general identity loop,
the cold side of the branch between the two loops, reads n_dof through a laundered copy), and the tail is where reshaping for speed is
tried (tools/experiments/README.md).  The dispatch gives these builds to large fleets only, so the build is forced (RMP2_KERNEL=quad,
RMP2_QUAD_MINW, read at rmp2_create) and every case asserts the build tag rmp2_last_kernel reports, as tests/test_gpu_quad_builds.py does; the
two-wave build, which keeps the older form, runs beside it as the control.

Scenes and what the CPU says about them: tests/quad_tail_scenes.py (pinned by tests/test_quad_tail_scenes.py).  Lines starting
with "QT" are measurements."""
import numpy as np
import pytest

import quad_tail_scenes as T
from test_gpu_quad_builds import _assert_tag, _engine_env, _tag

pytestmark = pytest.mark.gpu
FLEETS, R_MAX = T.FLEETS, T.R_MAX
D_STATUS_NONFINITE, D_STATUS_PINV_PATH, D_STATUS_JACOBI = 1, 4, 8   # include/rmp2.h
STRUCTURED = "identity leaves: structured loop, full width"
# the velocity cap ALONE is no inertia leaf: such a set is not given the plain build -- its step is the quad kernel up to (M, f) and
# rmp2_pinv_kernel (csrc/rmp2_hip.hip dispatch_solve), whatever RMP2_KERNEL says.  It is held to the same gate on that path.
TWO_KERNELS = ("cap",)
SCENES = list(T.order_sets()) + ["cap-edges", "cap-edges-pinv", "cspace-edges", "span", "span-auto", "nonfinite"] + list(T.GENERAL_LOOP)


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def scenes():
    return {"scenes": T.make_scenes(), "ref": {}, "engines": {}}


def _reference(cases, name):
    if name not in cases["ref"]:
        cases["ref"][name] = T.references(cases["scenes"][name])
    return cases["ref"][name]


def _engine(cases, name, minw):
    if (name, minw) not in cases["engines"]:
        cases["engines"][(name, minw)] = _engine_env(cases["scenes"][name]["desc"], RMP2_KERNEL="quad", RMP2_QUAD_MINW=minw)
    return cases["engines"][(name, minw)]


def _inputs(torch, eng, sc, R):
    q, qd, goal = (torch.from_numpy(np.ascontiguousarray(sc["s"][k][:R])).cuda() for k in ("q", "qd", "goal"))
    return q, qd, goal, eng.obstacles(spheres=torch.from_numpy(sc["kw"]["spheres"]))


def _gate(out, exact, env, R, what):
    """Every robot through the accuracy gate with the fp32 envelope; a robot the oracle resolves to NaN must be NaN in every dof."""
    import oracle as O
    ex = {k: (v[:R] if isinstance(v, np.ndarray) and v.shape[:1] == (R_MAX,) else v) for k, v in exact.items()}
    verdict = O.accuracy_gate(out, ex, truth=ex["qdd64"], envelope=env[:R])
    summary = O.gate_summary(verdict)
    print(f"QT gate {what} R {R}: {summary}")
    clean = np.isfinite(ex["qdd64"]).all(axis=1)
    assert np.isfinite(out[clean]).all() and verdict["ok"].all() and summary["rejected"] == 0, f"{what}, R = {R}: {summary}"


@pytest.mark.parametrize("name", SCENES)
def test_plain_step(torch_mod, scenes, name):
    """One control step of the plain build over the shared table: the four-wave build and the
    two-wave control, at 1, 17 and 65 robots, every robot through oracle.accuracy_gate; and the status words of the two builds
    agree robot by robot -- the robots the elimination does not settle (not finite: NONFINITE; not certified: JACOBI under
    solve = pinv) are the same."""
    torch = torch_mod
    sc = scenes["scenes"][name]
    exact, env, _ = _reference(scenes, name)
    status = {}
    for minw in (4, 2):
        eng = _engine(scenes, name, minw)
        for R in FLEETS:
            q, qd, goal, obs = _inputs(torch, eng, sc, R)
            st = torch.zeros(R, dtype=torch.int32, device="cuda")
            out = eng.step(q, qd, goal, obstacles=obs, status=st)
            torch.cuda.synchronize()
            kernel = eng.last_kernel()
            if name in TWO_KERNELS:
                _assert_tag(kernel, _tag(minw, "general", "any", True, False))
                assert "rmp2_pinv_kernel" in kernel, kernel
            else:
                _assert_tag(kernel, _tag(minw, "plain", "shared", True, False))
                # (the scenes of T.GENERAL_LOOP run the OTHER loop of the same build: the cold side, whose tests against n_dof the
                # four-wave builds form from a laundered copy)
                assert (STRUCTURED in kernel) == (name not in T.GENERAL_LOOP), kernel
            _gate(out.cpu().numpy(), exact, env, R, f"plain {name} minw {minw}")
            status[(minw, R)] = st.cpu().numpy().copy()
    for R in FLEETS:
        assert np.array_equal(status[(4, R)], status[(2, R)]), (name, R, status[(4, R)], status[(2, R)])
    st = status[(4, R_MAX)]
    if name == "nonfinite":
        bad = np.zeros(R_MAX, bool)
        bad[[T.NAN_ROBOT, T.INF_ROBOT]] = True
        assert ((st & D_STATUS_NONFINITE) != 0).tolist() == bad.tolist(), st
    else:
        assert not (st & D_STATUS_NONFINITE).any(), st
    if name == "span":
        print(f"QT status span: robots on the Jacobi path {np.nonzero(st & D_STATUS_JACOBI)[0].tolist()}")
        assert (st[3::4] & D_STATUS_JACOBI).all() and not (st & D_STATUS_JACOBI).all()


@pytest.mark.parametrize("name", SCENES)
def test_general_flavour(torch_mod, scenes, name):
    """The step with M= and f=: the general flavour in front of the same resolve.  M and f against the reference-precision oracle at
    5e-6 * max(1, max |ref|), the tolerance tests/test_gpu_quad_builds.py holds the exported system to (on the robots whose
    system the oracle finds finite; the others' must hold a non-finite entry); q-double-dot through the gate."""
    torch = torch_mod
    sc = scenes["scenes"][name]
    n = sc["desc"].robot.n_dof
    exact, env, ref32 = _reference(scenes, name)
    for minw in (4, 2):
        eng = _engine(scenes, name, minw)
        for R in FLEETS:
            q, qd, goal, obs = _inputs(torch, eng, sc, R)
            M = torch.full((R, n, n), float("nan"), dtype=torch.float64, device="cuda")
            f = torch.full((R, n), float("nan"), dtype=torch.float64, device="cuda")
            out = eng.step(q, qd, goal, obstacles=obs, M=M, f=f)
            torch.cuda.synchronize()
            _assert_tag(eng.last_kernel(), _tag(minw, "general", "any", True, False))
            assert ("rmp2_pinv_kernel" in eng.last_kernel()) == (name in TWO_KERNELS), eng.last_kernel()
            M, f = M.cpu().numpy(), f.cpu().numpy()
            rM, rf = ref32["M"][:R], ref32["f"][:R]
            fin = np.isfinite(rM).all(axis=(1, 2)) & np.isfinite(rf).all(axis=1)
            eM, ef = np.abs(M[fin] - rM[fin]).max(), np.abs(f[fin] - rf[fin]).max()
            tM, tf = 5e-6 * max(1.0, np.abs(rM[fin]).max()), 5e-6 * max(1.0, np.abs(rf[fin]).max())
            print(f"QT system {name} minw {minw} R {R}: |M - ref| {eM:.3e} of bound {tM:.3e}, |f - ref| {ef:.3e} of bound {tf:.3e}")
            assert eM <= tM and ef <= tf, f"{name} minw {minw} R {R}: M {eM:.3e} / {tM:.3e}, f {ef:.3e} / {tf:.3e}"
            for r in np.nonzero(~fin)[0]:
                assert not (np.isfinite(M[r]).all() and np.isfinite(f[r]).all()), (name, r)
            assert np.array_equal(M[fin], M[fin].transpose(0, 2, 1)), "the symmetric build's matrix is its upper triangle, mirrored"
            _gate(out.cpu().numpy(), exact, env, R, f"general {name} minw {minw}")

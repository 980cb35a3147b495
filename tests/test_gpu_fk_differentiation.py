"""Engine.differentiate / Engine.differentiate_euler (rmp2_diff_kernel) against the fp64 autograd reference of
tests/kinematics_reference.py -- not against the oracle -- on general robots at |qd| <= 2: every frame of the 22 random trees
(the 32-frame chain and the 16-dof tree among them), of the z-y-x wrist and of the prismatic sandwich, 4 states per scene, tiled
into fleets of 1, 130 and 65 robots on one handle in that order (the scratch buffer grows, then is reused larger than needed; a
partial last wave; two blocks).

No bound is taken from the device.  Each is 4 x the deviation of the oracle's own fp32 build from the reference, as
`python tests/kinematics_reference.py --measure` records it in profiles/kinematics_reference.json (f32_4x4 and
f32_euler_fp32_scaling; the margin is for the device's sincosf and contraction over chains of up to 32 joints):
  4x4:    |got - ref| / max(1, |ref|) per array;
  Euler:  x cy, xd cy^2, J cy^2, c cy^3 with cy = |cos theta_y| -- an fp32 evaluation loses one more power of cy than an fp64 one
          (its r20 carries 6e-8, theta_y = -asin(r20) then 6e-8 / cy, and each derivative another 1 / cy) -- on the cases with
          cy >= 1e-2.  Below, theta_x and theta_z of an fp32 rotation are noise on both sides and nothing is asserted on them
          ("The pole rule")."""
import json

import numpy as np
import pytest

import kinematics_reference as KR

pytestmark = pytest.mark.gpu

# 4 x (measured deviation of the f32 oracle, profiles/kinematics_reference.json), per output (x, xd, J, c)
BOUND_4X4 = (4 * 5.601e-07, 4 * 5.745e-07, 4 * 6.3e-07, 4 * 8.215e-07)
BOUND_EULER = (4 * 2.574e-07, 4 * 1.694e-06, 4 * 7.935e-07, 4 * 5.856e-06)   # x cy, xd cy^2, J cy^2, c cy^3
FLEETS = (1, 130, 65)


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _run(torch, eng, q, qd, frame, euler):
    fn = eng.differentiate_euler if euler else eng.differentiate
    out = fn(torch.from_numpy(np.ascontiguousarray(q)), torch.from_numpy(np.ascontiguousarray(qd)), frame)
    return tuple(t.cpu().numpy() for t in out)


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def world(torch_mod, tmp_path_factory):
    """Scenes; the reference of every frame at the scene's 4 states, computed once; the device's answers: every state run alone
    (on a handle of its own, so that the fleet handle sees exactly R = 1, 130, 65) and the three fleets."""
    from riemannian_motion_policies_amd.engine import Engine
    scs = KR.scenes(tmp_path_factory.mktemp("kinref"))
    ref, alone, fleets = {}, {}, {}
    for sc in scs:
        consts = KR.constants(sc.desc)
        for fr in range(sc.n_frames):
            for eu in (False, True):
                ref[sc.name, fr, eu] = KR.differentiate_batch(sc.desc, sc.q, sc.qd, fr, eu, consts)
        solo, eng = Engine(sc.desc, 0), Engine(sc.desc, 0)
        for fr in range(sc.n_frames):
            for eu in (False, True):
                rows = [_run(torch_mod, solo, sc.q[b:b + 1], sc.qd[b:b + 1], fr, eu) for b in range(KR.STATES)]
                alone[sc.name, fr, eu] = tuple(np.concatenate([r[i] for r in rows]) for i in range(4))
        for R in FLEETS:
            idx = np.arange(R) % KR.STATES
            for fr in range(sc.n_frames):
                for eu in (False, True):
                    fleets[sc.name, fr, eu, R] = _run(torch_mod, eng, sc.q[idx], sc.qd[idx], fr, eu)
        solo.close()
        eng.close()
    return scs, ref, alone, fleets


def test_bounds_are_four_times_the_recorded_measurement():
    with open(KR.PROFILE) as f:
        prof = json.load(f)
    for key, bound in (("f32_4x4", BOUND_4X4), ("f32_euler_fp32_scaling", BOUND_EULER)):
        for name, b in zip(KR.NAMES, bound):
            assert b == pytest.approx(4 * prof[key][name], rel=1e-12), (key, name)


def test_fleet_rows_have_the_bits_of_the_state_run_alone(world):
    scs, _, alone, fleets = world
    for sc in scs:
        for fr in range(sc.n_frames):
            for eu in (False, True):
                for R in FLEETS:
                    idx = np.arange(R) % KR.STATES
                    want = tuple(a[idx] for a in alone[sc.name, fr, eu])
                    assert _same_bits(fleets[sc.name, fr, eu, R], want), (sc.name, fr, eu, R)


def _sweep(world, euler, bound, powers):
    scs, ref, alone, _ = world
    worst, where = [0.0] * 4, [None] * 4
    held = cases = 0
    for sc in scs:
        for fr in range(sc.n_frames):
            r, got = ref[sc.name, fr, euler], alone[sc.name, fr, euler]
            cy = KR.euler_cy(r[0]) if euler else np.ones(KR.STATES)
            for b in range(KR.STATES):
                cases += 1
                if euler and cy[b] < KR.CY_HELD_F32:
                    continue
                held += 1
                dev = KR.deviation([g[b] for g in got], [a[b] for a in r], cy[b], powers)
                for i in range(4):
                    if not dev[i] <= worst[i]:
                        worst[i], where[i] = dev[i], (sc.name, fr, b)
    print(f"device {'euler' if euler else '4x4'}: worst " + ", ".join(f"{n} {w:.3e} (bound {b:.3e})" for n, w, b in zip(KR.NAMES, worst, bound)))
    for i, nm in enumerate(KR.NAMES):
        assert worst[i] <= bound[i], f"{nm}: {worst[i]:.3e} > {bound[i]:.3e} at (scene, frame, state) {where[i]}"
    return held, cases


def test_differentiate_against_reference(world):
    held, cases = _sweep(world, False, BOUND_4X4, KR.POWERS_4X4)
    assert held == cases == 880


def test_differentiate_euler_against_reference(world):
    held, cases = _sweep(world, True, BOUND_EULER, KR.POWERS_EULER_F32)
    assert cases == 880 and held >= 0.95 * cases, (held, cases)


# ---- the wrist: closed form, and the pole ---------------------------------------------------------------------------------

def _wrist(world):
    return next(s for s in world[0] if s.name == "wrist")


def test_wrist_closed_form(torch_mod, world):
    """x = (q_x, q_y, q_z), J the anti-diagonal permutation, c = 0 at cos theta_y = 0.5, 1e-1, 1e-2, under the Euler scalings."""
    from riemannian_motion_policies_amd.engine import Engine
    wrist = _wrist(world)
    q, qd = KR.wrist_states((0.5, 1e-1, 1e-2, 0.5, 1e-1, 1e-2), seed=11)
    want = KR.wrist_closed_form(q, qd)
    cy = np.cos(q[:, 1].astype(np.float64))
    eng = Engine(wrist.desc, 0)
    for fr in (KR.WRIST_TIP - 1, KR.WRIST_TIP):
        got = _run(torch_mod, eng, q, qd, fr, True)
        for b in range(len(q)):
            dev = KR.deviation([g[b] for g in got], [w[b] for w in want], cy[b], KR.POWERS_EULER_F32)
            print(f"wrist frame {fr} cy {cy[b]:.1e}: " + ", ".join(f"{n} {d:.3e}" for n, d in zip(KR.NAMES, dev)))
            for nm, d, bd in zip(KR.NAMES, dev, BOUND_EULER):
                assert d <= bd, (fr, cy[b], nm, d, bd)


def test_wrist_pole_robots_leave_their_wave_alone(torch_mod, world):
    """At cos theta_y = 1e-3 and at the fp32 pole (q_y = fl(pi / 2), cos theta_y = -4.4e-8) theta_x and theta_z are individually
    undefined and the map's derivatives unbounded, as the reference's are: nothing is asserted on them.  theta_y itself is held
    (asin's slope is 1 / cy: 6e-8 of r20 is at most 3.5e-4 of theta_y at the pole), and every other robot of the wave has the
    bits it has in a fleet without the pole robots."""
    from riemannian_motion_policies_amd.engine import Engine
    wrist = _wrist(world)
    R = 70
    q, qd = KR.wrist_states(tuple([0.5, 1e-1, 1e-2, 0.9, 0.3] * (R // 5)), seed=13)
    half_pi = np.float32(np.pi / 2)
    poles = {5: np.float32(np.arccos(1e-3)), 17: -np.float32(np.arccos(1e-3)), 33: half_pi, 40: -half_pi, 66: half_pi}
    qp = q.copy()
    for r, v in poles.items():
        qp[r, 1] = v
    eng = Engine(wrist.desc, 0)
    others = np.array([r for r in range(R) if r not in poles])
    for fr in (KR.WRIST_TIP - 1, KR.WRIST_TIP):
        clean = _run(torch_mod, eng, q, qd, fr, True)
        got = _run(torch_mod, eng, qp, qd, fr, True)
        assert _same_bits([g[others] for g in got], [c[others] for c in clean]), fr
        for r, v in poles.items():
            assert abs(float(got[0][r, 1]) - float(v)) <= 1e-3, (fr, r, got[0][r], v)


# ---- other checks ---------------------------------------------------------------------------------------------------------

def test_non_finite_q_leaves_the_neighbours_alone(torch_mod, world):
    from riemannian_motion_policies_amd.engine import Engine
    sc = next(s for s in world[0] if s.name == "sandwich")
    R = 70
    idx = np.arange(R) % KR.STATES
    q, qd = sc.q[idx].copy(), sc.qd[idx].copy()
    bad = q.copy()
    bad[3, 0], bad[64, 1], bad[66, 2] = np.nan, np.inf, -np.inf
    others = np.array([r for r in range(R) if r not in (3, 64, 66)])
    eng = Engine(sc.desc, 0)
    for eu in (False, True):
        fr = sc.n_frames - 1
        clean = _run(torch_mod, eng, q, qd, fr, eu)
        got = _run(torch_mod, eng, bad, qd, fr, eu)
        assert _same_bits([g[others] for g in got], [c[others] for c in clean]), eu
        assert all(np.isfinite(c).all() for c in clean)
        assert not np.isfinite(got[0][3]).all()


def test_frame_out_of_range_is_refused(torch_mod, world):
    from riemannian_motion_policies_amd import _native
    from riemannian_motion_policies_amd.engine import Engine
    sc = next(s for s in world[0] if s.name == "sandwich")
    eng = Engine(sc.desc, 0)
    q, qd = torch_mod.from_numpy(sc.q), torch_mod.from_numpy(sc.qd)
    for fn in (eng.differentiate, eng.differentiate_euler):
        for fr in (-1, sc.n_frames, 99):
            with pytest.raises(_native.Rmp2Error) as e:
                fn(q, qd, fr)
            assert e.value.code == _native.ERR_INVALID_ARGUMENT
        fn(q, qd, sc.n_frames - 1)   # ... and the handle still serves a valid call
    torch_mod.cuda.synchronize()

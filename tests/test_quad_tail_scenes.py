"""No GPU: the scenes of tests/test_gpu_quad_tail.py (tests/quad_tail_scenes.py) do what its cases rely on.  Every branch of the
velocity cap and of the c-space biasing is taken by at least one robot of every fleet that is meant to take it, counted from the
fp32 intermediates of the reference's formulae and again from the oracle's own values (its system of that leaf alone); the "span" fleet holds certified and uncertified robots in every wave, by the
certificate restated in tests/test_certificate_math.py on the oracle's own systems; and the oracle's reference-precision
evaluation passes the accuracy gate against its fp64 evaluation on every scene, no robot exempted."""
import numpy as np
import pytest

import quad_tail_scenes as T
from test_certificate_math import certificate


@pytest.fixture(scope="module")
def scenes():
    return T.make_scenes()


@pytest.fixture(scope="module")
def refs(scenes):
    return {name: T.references(sc) for name, sc in scenes.items()}


def test_the_orders_are_all_there(scenes):
    """Each kind alone, the 12 orders of two and the 24 of three different kinds, one set with a kind twice; every set is taken
    whole by the structured loop (all identity leaves structured, nine dofs)."""
    from riemannian_motion_policies_amd import descriptor as D
    names = T.order_sets()
    assert sorted(len(k) for k in names.values()) == [1] * 4 + [2] * 12 + [3] * 24 + [4]
    assert len(set(names.values())) == 41
    for name, kinds in names.items():
        desc = scenes[name]["desc"]
        ident = [int(desc.leaves[i].kind) for i in range(desc.n_leaves) if desc.leaves[i].taskmap == D.TASKMAP_IDENTITY]
        want = {"damping": D.LEAF_JOINT_DAMPING, "cspace": D.LEAF_CSPACE_BIASING, "config_space": D.LEAF_CONFIG_SPACE_BIASING,
                "cap": D.LEAF_JOINT_VELOCITY_CAP}
        assert ident == [want[k] for k in kinds], name
        assert desc.robot.n_dof == 9
    assert {scenes[n]["solve"] for n in names} == {"auto", "pinv"}


@pytest.mark.parametrize("R", T.FLEETS[1:])
def test_every_branch_of_the_velocity_cap_is_taken(scenes, R):
    """17 and 65 robots: a joint below, exactly at and above the cutoff; dv on the last fp32 step in front of rlimit and beyond it; zero, negative and
    positive velocities.  (The lone robot of the smallest fleet has all joints below the cutoff, both signs.)"""
    for name in ("cap-edges", "cap-edges-pinv"):
        b = T.cap_branches(scenes[name]["s"]["qd"][:R])
        counts = {k: int(v.sum()) for k, v in b.items()}
        print(f"QT cap branches {name} R {R}: {counts}")
        assert all(c >= 1 for c in counts.values()), counts
        # ... and the oracle's own intermediates (the cap's diagonal and acceleration, from its system of that leaf alone) say the same
        sR = {k: v[:R] for k, v in scenes[name]["s"].items()}
        o = T.cap_branches_from_oracle(sR)
        print(f"QT cap branches from the oracle {name} R {R}: " + str({k: int(v.sum()) for k, v in o.items() if k != "pushes_back"}))
        for k in ("below", "at", "above", "dv_at_rlimit", "dv_beyond_rlimit"):
            assert np.array_equal(o[k], b[k]), (name, k)
        assert o["pushes_back"]
    one = T.cap_branches(scenes["cap-edges"]["s"]["qd"][:1])
    assert one["below"].all() and one["negative"].any() and one["positive"].any()


@pytest.mark.parametrize("R", T.FLEETS[1:])
def test_every_branch_of_the_cspace_biasing_is_taken(scenes, R):
    """The norm of q - goal exactly 0, below the threshold P[3] and above it."""
    from riemannian_motion_policies_amd import configs as Cf
    nrm = T.cspace_norm(scenes["cspace-edges"]["s"]["q"][:R])
    thr = np.float32(Cf.CSPACE_BIASING_PARAMS[3])
    counts = {"zero": int((nrm == 0).sum()), "near": int(((nrm > 0) & (nrm < thr)).sum()), "far": int((nrm >= thr).sum())}
    print(f"QT cspace branches R {R}: {counts}; closest to the threshold {np.abs(nrm - thr).min():.3e}")
    assert all(c >= 1 for c in counts.values()), counts
    o = T.cspace_sides_from_oracle({k: v[:R] for k, v in scenes["cspace-edges"]["s"].items()})   # the oracle's own values say the same
    assert np.array_equal(o["zero"], nrm == 0) and np.array_equal(o["near"], (nrm > 0) & (nrm < thr)) and np.array_equal(o["far"], nrm >= thr)
    assert T.cspace_norm(scenes["cspace-edges"]["s"]["q"][:1])[0] == 0   # the lone robot sits at the goal


def test_the_span_fleet_mixes_certified_and_uncertified_robots_in_every_wave(scenes, refs):
    """By the kernels' certificate on the oracle's reference-precision systems: every full wave of the strict span fleet (and the
    first 16 of the 17-robot fleet) holds robots the certificate accepts and robots it turns away; the accepted ones span condition
    numbers from below 1e2 to above 1e4, positive definite and indefinite; the ones turned away are as well conditioned -- what
    fails is the elimination order (a first pivot of 2e-4 under a column of 0.05)."""
    M = refs["span"][2]["M"]
    cert = np.array([certificate(M[r], True)[0] for r in range(T.R_MAX)])
    cond = np.linalg.cond(M)
    print(f"QT span: certified {int(cert.sum())} of {T.R_MAX}; condition numbers {cond.min():.2e} .. {cond.max():.2e}, "
          f"of the certified {cond[cert].min():.2e} .. {cond[cert].max():.2e}")
    for w in range(T.R_MAX // 16):
        c = cert[16 * w:16 * w + 16]
        assert c.any() and not c.all(), (w, c)
    assert cond[cert].min() < 1e2 and cond[cert].max() > 1e4 and cond[~cert].max() < 1e5
    assert np.allclose(M[3::4, 0, 0], T.SMALL_PIVOT, rtol=1e-2)
    definite = np.array([(np.linalg.eigvalsh(0.5 * (m + m.T)) > 0).all() for m in M])
    assert definite[cert].any() and not definite[cert].all()


def test_the_general_loop_scenes_are_symmetric_sets_outside_the_structured_loop(scenes):
    """What sends a lean build through the general identity loop: a dense identity leaf in a set of nine dofs, or fewer dofs than the
    template with structured leaves only.  Both sets carry an inertia leaf and no JointLimitAvoidance (the symmetric builds), and
    their velocities meet every branch of the cap."""
    from riemannian_motion_policies_amd import descriptor as D
    structured = {D.LEAF_JOINT_DAMPING, D.LEAF_CSPACE_BIASING, D.LEAF_CONFIG_SPACE_BIASING, D.LEAF_JOINT_VELOCITY_CAP}
    for name, n_dof, all_structured in (("general-dense", 9, False), ("general-arm7", 7, True)):
        desc = scenes[name]["desc"]
        ident = [int(desc.leaves[i].kind) for i in range(desc.n_leaves) if desc.leaves[i].taskmap == D.TASKMAP_IDENTITY]
        assert desc.robot.n_dof == n_dof and all(k in structured for k in ident) == all_structured, (name, ident)
        assert D.LEAF_JOINT_DAMPING in ident and D.LEAF_JOINT_LIMIT_AVOIDANCE not in ident
        assert scenes[name]["s"]["goal"].shape[1] == desc.goal_floats
        b = T.cap_branches(scenes[name]["s"]["qd"][:17])
        assert all(int(v.sum()) >= 1 for v in b.values()), name


def test_the_nonfinite_robots_are_two_and_their_neighbours_are_clean(scenes, refs):
    s = scenes["nonfinite"]["s"]
    bad = ~(np.isfinite(s["q"]).all(axis=1) & np.isfinite(s["qd"]).all(axis=1))
    assert sorted(np.nonzero(bad)[0]) == [T.NAN_ROBOT, T.INF_ROBOT] and max(T.NAN_ROBOT, T.INF_ROBOT) < 16
    exact = refs["nonfinite"][0]["qdd64"]
    assert np.isnan(exact[bad]).all() and np.isfinite(exact[~bad]).all()


def test_the_oracle_passes_the_gate_on_every_scene(scenes, refs):
    """The reference-precision evaluation (fp32 leaves) against the fp64 one through oracle.accuracy_gate with the fp32 envelope:
    nothing rejected on any scene -- what the GPU cases ask of the kernel, the reference's own formulae can deliver."""
    import oracle as O
    for name in scenes:
        exact, env, ref32 = refs[name]
        verdict = O.accuracy_gate(ref32["qdd64"], exact, truth=exact["qdd64"], envelope=env)
        summary = O.gate_summary(verdict)
        assert verdict["ok"].all(), (name, summary)

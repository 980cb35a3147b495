"""No GPU: the scenes of tests/test_gpu_quad_builds.py (tests/quad_build_scenes.py) do what its cases are named for.  Oracle
forward kinematics and the oracle's closed loop only; the figures are pinned so that a change of a generator does not hollow the
GPU tests out unnoticed."""
import numpy as np
import pytest

import quad_build_scenes as S


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tables = S.make_tables()
    return tables, S.make_sets(tmp_path_factory.mktemp("tree"), tables)


# in-range share of the pairs a step evaluates, per (set, table): |p - c| <= radius + margin + modulation radius, fp64
PINNED_SHARE = {
    "config3": {"33": 0.2298, "ragged": 0.2267, "capsule": 0.3963, "explicit33": 0.2298, "explicit32": 0.2885},
    "arm7": {"33": 0.2061, "ragged": 0.1970, "capsule": 0.3822, "explicit33": 0.2061, "explicit32": 0.3438},
    "tree": {"33": 0.4272, "ragged": 0.4308, "capsule": 0.3066, "explicit33": 0.4272, "explicit32": 0.4254},
}


def test_in_range_pair_shares(scenes):
    """The shared, ragged and capsule tables (and the explicit pairs made of the sphere tables) put at least a tenth of their
    pairs in range of some control point -- the pair loops have work in every wave --, the far table none."""
    tables, sets = scenes
    for name in S.DISTANCE_SETS:
        desc, s = sets[name]
        for table in S.TABLES:
            share = S.in_range_share(name, desc, s, tables, table)
            if table == "far":
                assert share == 0.0
                continue
            assert share >= 0.1, (name, table, share)
            assert abs(share - PINNED_SHARE[name.split("-")[0]][table]) < 1e-4, (name, table, round(share, 4))
    clr = S.origins(sets["config3-auto"][0], sets["config3-auto"][1]["q"])
    sph = tables["33"]
    clr = (np.linalg.norm(clr[:, :, None, :] - sph[None, None, :, :3], axis=-1) - sph[None, None, :, 3]).min(axis=(1, 2))
    assert S.CLEAR <= clr.min() < 2 * S.CLEAR          # filtered, and still close
    cap = S.capsule_clearance(S.origins(*[sets["config3-auto"][0], sets["config3-auto"][1]["q"]]), tables["capsule"])
    assert S.CLEAR <= cap.min() < 2 * S.CLEAR          # the lifted capsules likewise


def test_ragged_lists(scenes):
    """An empty list and a full one inside the 17-robot fleet; every list a set (the membership-mask form)."""
    off, idx = scenes[0]["ragged"]
    n = np.diff(off)
    assert len(off) == S.R_MAX + 1 and n[2] == 0 and n[3] == 33 and off[-1] == len(idx) and idx.min() == 0 and idx.max() == 32
    assert all(len(set(idx[off[r]:off[r + 1]])) == n[r] for r in range(S.R_MAX))


def test_oracle_rollouts_are_tame(scenes):
    """The closed loops test_gpu_quad_builds.py test_plain_rollout compares against: every robot of every fleet tame (finite,
    peak |qdd| <= 20; the GPU tests need 0.95) in the ORACLE's own evaluation, the fleet moves, and the oracle's fp32 and fp64 loops agree far inside the 1e-5 the kernels are held
    to (so that the measured bound of the 7-dof arm and the tree, max(1e-5 scale, 4 |fp32 - fp64|), stays near 1e-5 too)."""
    from test_gpu_quad_builds import ROLLOUT_CASES
    tables, sets = scenes
    for name, table in ROLLOUT_CASES:
        desc, s = sets[name]
        ref32, ref64 = S.oracle_rollout_pair(desc, s, S.obstacle_kwargs(name, desc, s, tables, table))
        tame = S.tame(*ref32)
        assert tame.all(), (name, table, int(tame.sum()))
        assert np.abs(ref32[0][tame] - s["q"][tame]).max() > 1e-3
        for a32, a64 in zip(ref32[:2], ref64[:2]):
            rel = np.abs(a32 - a64)[tame].max(axis=1) / np.maximum(1.0, np.abs(a32[tame]).max(axis=1))
            assert rel.max() < 1e-6, (name, table, rel.max())


def test_the_oracle_resolves_the_exported_systems(scenes):
    """test_gpu_quad_builds.py test_general_flavour holds M and f to 5e-6 * max(1, max |ref|), a tolerance established on scenes
    without contact (tests/test_gpu_random_robots.py).  It can hold a kernel on these scenes only while the reference itself
    resolves that much there: the oracle's reference-precision and fp64 evaluations agree to a quarter of the tolerance (the
    margin tests/test_gpu_forward_dynamics.py gives an fp32 envelope).  With control points 4 cm from a sphere they did not -- f of
    one robot was 0.8 of the tolerance off --, which is what set CLEAR."""
    import oracle as O
    from test_gpu_quad_builds import GENERAL_CASES
    tables, sets = scenes
    for name, table in GENERAL_CASES:
        desc, s = sets[name]
        kw = S.obstacle_kwargs(name, desc, s, tables, table)
        a, b = (O.step(desc, s["q"], s["qd"], s["goal"], precision=p, **kw) for p in ("f32", "f64"))
        for k in ("M", "f"):
            assert np.abs(a[k] - b[k]).max() <= 0.25 * 5e-6 * max(1.0, np.abs(a[k]).max()), (name, table, k)


def test_the_cases_name_every_build():
    """The parameter tables of the GPU module name every four-wave instantiation (no GPU needed to check the list)."""
    from test_gpu_quad_builds import test_the_cases_name_every_region_pullback_build as check
    check()

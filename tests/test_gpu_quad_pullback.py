"""The pull-back of the quad step kernel (csrc/rmp2_quad.h: Jacobian columns of a lane's rows -> u = S col, f -> the column
ladder of J^T S J) at the smallest shapes at which it can go wrong.

Small fleets never reach the 128-register build the large ones run, so the mapping and its register cap are forced
(RMP2_KERNEL=quad, RMP2_QUAD_MINW = 2 | 4, read at rmp2_create).  Fleets of 1, 16, 17 and 65 robots: one quad, one full wave,
a partial last wave, tail quads.  Sets: the cluttered Panda set under both resolves (prismatic rows 7 and 8, row blocks
0 - 2, frames with 1 ... 8 ancestors), the TwoJoint half of the mixed fleet (the other template size; no inertia leaf: the
rank-one form of S col), a tree-shaped robot whose joint order runs from the leaves to the root (save / restore slots,
ancestor sets that are not prefixes, frames whose low row blocks hold no ancestor while later ones do -- the row blocks the
kernel skips whole).  Tables of 32 spheres (one full chunk), 33 (a partial second chunk) and a single sphere 1 km away (every
pair out of range: S = h = 0, the pull-back adds exact zeros).

The references are computed once per (set, table) on the 65-robot fleet; the smaller fleets are its first rows (robots are
independent)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
D_STATUS_NONFINITE = 1   # include/rmp2.h RMP2_STATUS_NONFINITE
FLEETS = (1, 16, 17, 65)
R_MAX = max(FLEETS)
TABLES = ("32", "33", "far")
SETS = ("config3-pinv", "config3-auto", "two-joint", "tree")


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


def _quad_engine(desc, minw):
    return _engine_env(desc, RMP2_KERNEL="quad", RMP2_QUAD_MINW=minw)


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _tree_robot(path):
    """A 9-dof tree from the generator of test_gpu_random_robots.py, its joints ordered from the leaves to the root: the dofs
    of a frame near the root are the LAST ones, so its low row blocks hold no ancestor."""
    from test_gpu_random_robots import _write_urdf
    from riemannian_motion_policies_amd import descriptor as D, urdf
    rng = np.random.default_rng(4003)
    movable = _write_urdf(path, rng, 12, branch_prob=0.3)
    t = urdf.compile_urdf(path, movable[:9][::-1])
    n = t.n_dof
    masks = [t.ancestor_dof_mask(f) for f in range(t.n_frames)]
    low_empty = [f for f, m in enumerate(masks) if m and not (m & 0xf)]
    not_prefix = [f for f, m in enumerate(masks) if (m & 0xf) and (m & (m + 1))]
    deepest = max(range(t.n_frames), key=lambda f: bin(masks[f]).count("1"))
    # what this robot is here for (properties of the fixed seed, checked so that a change of the generator does not hollow the test)
    assert n == 9 and 1 <= t.depth_first_schedule()[3] <= 2 and len(low_empty) >= 2 and not_prefix
    assert any((masks[f] & 0xf0) and (masks[f] & 0xf00) for f in low_empty), "a frame that skips block 0 and keeps 1 and 2"
    frames = sorted({deepest, *low_empty[:3], *not_prefix[:2]})
    specs = [D.LeafSpec(D.LEAF_TARGET_ATTRACTOR, D.TASKMAP_FK_POSITION, deepest,
                        [0.3, 0.6, 0.075, 0.05, 0.03, 1.0, 0.5, 1.0, 0.02], goal_len=3),
             D.LeafSpec(D.LEAF_JOINT_DAMPING, D.TASKMAP_IDENTITY, -1, [1.0, 0.005, 0.3]),
             D.LeafSpec(D.LEAF_CSPACE_BIASING, D.TASKMAP_IDENTITY, -1, [0.005, 1.0, 2.0, 0.5, 0.0001],
                        vec_a=rng.uniform(-0.5, 0.5, n)),
             D.LeafSpec(D.LEAF_TARGET_POLICY, D.TASKMAP_FK_POSITION, low_empty[0], [0.1, 0.5, 0.1], goal_len=3)]
    for fr in frames:
        specs.append(D.LeafSpec(D.LEAF_OBSTACLE_AVOIDANCE, D.TASKMAP_FK_DISTANCE, int(fr),
                                [0.0, 50.0, 0.04, 0.01, 0.01, 800.0, 0.01, 0.5, 1.0, 0.02, 0.001]))
    s = {"q": rng.uniform(-1.0, 1.0, (R_MAX, n)).astype(np.float32),
         "qd": rng.uniform(-0.1, 0.1, (R_MAX, n)).astype(np.float32),
         "goal": rng.uniform(-0.5, 0.5, (R_MAX, 6)).astype(np.float32)}
    return D.build_desc(t, specs, "pinv"), s


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """Per set: (descriptor, states of the 65-robot fleet); per table: the sphere array; references filled in on first use."""
    from riemannian_motion_policies_amd import configs as Cf
    rng = np.random.default_rng(20)
    panda = Cf.sample_panda_states(rng, R_MAX)
    sets = {"config3-pinv": (Cf.config3("pinv")[1], panda), "config3-auto": (Cf.config3("auto")[1], panda),
            "two-joint": (Cf.config5_two_joint("pinv")[1], Cf.sample_two_joint_states(rng, R_MAX)),
            "tree": _tree_robot(str(tmp_path_factory.mktemp("tree") / "tree.urdf"))}
    tables = {"32": Cf.sample_spheres(rng, 32), "33": Cf.sample_spheres(rng, 33),
              "far": np.array([[1000.0, 0.0, 0.0, 0.1]], dtype=np.float32)}
    return {"sets": sets, "tables": tables, "ref": {}, "engines": {}}


def _table(cases, set_name, table):
    """The set's sphere table.  (The tree's frames crowd around its base: the table's centres are drawn in by 0.4 for it, which
    puts a good part of its pairs in range -- at full scale the obstacle leaves moved its M by 1e-4 at the most.)"""
    sph = cases["tables"][table]
    if set_name == "tree" and table != "far":
        sph = sph.copy()
        sph[:, :3] *= np.float32(0.4)
    return sph


def _reference(cases, set_name, table):
    """fp64 evaluation of the reference's formulae and the fp32 envelope of the 65-robot fleet: once per (set, table)."""
    import oracle as O
    key = (set_name, table)
    if key not in cases["ref"]:
        desc, s = cases["sets"][set_name]
        sph = _table(cases, set_name, table)
        exact = O.step(desc, s["q"], s["qd"], s["goal"], precision="f64", spheres=sph)
        env = O.fp32_envelope(desc, s["q"], s["qd"], s["goal"], spheres=sph)
        cases["ref"][key] = (exact, env)
    return cases["ref"][key]


def _engine(cases, set_name, minw):
    key = (set_name, minw)
    if key not in cases["engines"]:
        cases["engines"][key] = _quad_engine(cases["sets"][set_name][0], minw)
    return cases["engines"][key]


def _first_rows(exact, env, R):
    return {k: (v[:R] if isinstance(v, np.ndarray) and v.shape[:1] == (R_MAX,) else v) for k, v in exact.items()}, env[:R]


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("set_name", SETS)
def test_qdd_against_the_fp64_oracle(torch_mod, cases, set_name, table, minw):
    """q-double-dot through the accuracy gate with the fp32 envelope, as bench.py's result check holds the timed buffers to it:
    no robot may be rejected."""
    torch = torch_mod
    import oracle as O
    desc, s = cases["sets"][set_name]
    sph = torch.from_numpy(_table(cases, set_name, table))
    exact, env = _reference(cases, set_name, table)
    eng = _engine(cases, set_name, minw)
    for R in FLEETS:
        out = eng.step(torch.from_numpy(s["q"][:R]), torch.from_numpy(s["qd"][:R]), torch.from_numpy(s["goal"][:R]),
                       obstacles=eng.obstacles(spheres=sph))
        torch.cuda.synchronize()
        assert "quad" in eng.last_kernel(), eng.last_kernel()
        ex, en = _first_rows(exact, env, R)
        verdict = O.accuracy_gate(out.cpu().numpy(), ex, truth=ex["qdd64"], envelope=en)
        summary = O.gate_summary(verdict)
        print(f"{set_name} table {table} minw {minw} R {R}: {summary}")
        assert verdict["ok"].all(), f"{set_name}, table {table}, minw {minw}, R = {R}: {summary}"


@pytest.mark.parametrize("minw", [2, 4])
def test_exported_system_on_the_golden_inputs(torch_mod, golden_dir, minw):
    """(M, f) of the cluttered set on tests/golden/config3.npz (asking for them runs the general flavour of the kernel), to the
    tolerance tests/test_gpu_parity.py holds that fixture to; the symmetric build's M is exactly symmetric."""
    torch = torch_mod
    from riemannian_motion_policies_amd import configs as Cf
    g = np.load(os.path.join(golden_dir, "config3.npz"))
    eng = _quad_engine(Cf.config3()[1], minw)
    R, n = g["q"].shape
    M = torch.empty((R, n, n), dtype=torch.float64, device="cuda")
    f = torch.empty((R, n), dtype=torch.float64, device="cuda")
    eng.step(torch.from_numpy(g["q"]), torch.from_numpy(g["qd"]), torch.from_numpy(g["goal"]),
             obstacles=eng.obstacles(spheres=torch.from_numpy(g["spheres"])), M=M, f=f)
    torch.cuda.synchronize()
    assert "quad" in eng.last_kernel(), eng.last_kernel()
    M, f = M.cpu().numpy(), f.cpu().numpy()
    print(f"minw {minw}: |M - golden| {np.abs(M - g['M']).max():.3e} of {np.abs(g['M']).max():.3e}, "
          f"|f - golden| {np.abs(f - g['f']).max():.3e} of {np.abs(g['f']).max():.3e}")
    assert np.abs(M - g["M"]).max() < 1e-4 * np.abs(g["M"]).max()
    assert np.abs(f - g["f"]).max() < 1e-4 * np.abs(g["f"]).max()
    assert np.array_equal(M, M.transpose(0, 2, 1)), "the symmetric build's matrix is its upper triangle, mirrored"


@pytest.mark.parametrize("minw", [2, 4])
@pytest.mark.parametrize("set_name", ["config3-pinv", "config3-auto"])
def test_a_nan_robot_stays_in_its_quad(torch_mod, cases, set_name, minw):
    """17 robots, q of robot 5 not a number: every other robot's q-double-dot is the run's without the NaN, bit for bit (a quad
    broadcast never leaves its quad), and robot 5 carries the non-finite status."""
    torch = torch_mod
    desc, s = cases["sets"][set_name]
    eng = _engine(cases, set_name, minw)
    sph = torch.from_numpy(cases["tables"]["32"])
    R = 17
    outs = []
    for poison in (False, True):
        q = s["q"][:R].copy()
        if poison:
            q[5, 2] = np.nan
        st = torch.zeros(R, dtype=torch.int32, device="cuda")
        out = eng.step(torch.from_numpy(q), torch.from_numpy(s["qd"][:R]), torch.from_numpy(s["goal"][:R]),
                       obstacles=eng.obstacles(spheres=sph), status=st)
        torch.cuda.synchronize()
        assert "quad" in eng.last_kernel(), eng.last_kernel()
        outs.append((out.cpu().numpy().copy(), st.cpu().numpy().copy()))
    (clean, st_clean), (dirty, st_dirty) = outs
    others = np.arange(R) != 5
    assert np.isfinite(clean).all() and not (st_clean & D_STATUS_NONFINITE).any()
    assert np.array_equal(clean[others].view(np.uint32), dirty[others].view(np.uint32))
    assert np.array_equal(st_clean[others], st_dirty[others])
    assert st_dirty[5] & D_STATUS_NONFINITE and np.isnan(dirty[5]).all()

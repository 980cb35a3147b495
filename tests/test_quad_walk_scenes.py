"""No GPU: the robots of tests/test_gpu_quad_walk.py (tests/quad_walk_scenes.py) have the programs its cases are named for, and
the reference resolves their steps far inside what the kernels are held to.  Pinned so that a change of a generator or of the
pruning rule cannot quietly take a scene off its edge."""
import numpy as np
import pytest

import quad_walk_scenes as W


@pytest.fixture(scope="module")
def sets():
    return W.make_sets()


def test_programs():
    """Frame counts, slot counts and where each program returns to the base or to a slot."""
    for name in W.ROBOTS:
        t, leaf_frames = W.tables(name)
        frames, restore, save, slots = W.program(t, leaf_frames)
        assert (len(frames), slots, restore, save) == W.PROGRAMS[name], (name, frames, restore, save, slots)
    n = {name: p[0] for name, p in W.PROGRAMS.items()}
    assert [n[k] for k in ("len1", "len2", "len3")] == [1, 2, 3]              # shorter than the two-ahead fetch and its clamps
    assert n["len4"] % 2 == 0 and n["len5"] % 2 == 1 and n["tree2"] % 2 == 1   # both rotation tails
    assert n["len5"] == 4 + 1                                                  # one group of four lanes and one frame
    assert n["len13"] == 13                                                  # longer than the Panda's eleven: four frames for a lane
    assert sorted({p[1] for p in W.PROGRAMS.values()}) == [0, 1, 2]            # every SLOTS instantiation
    r, s = W.PROGRAMS["forest0"][2:]
    assert r[0] == r[1] == r[-1] == -2 and set(s) == {-1}                      # base on the first, second and last frame
    assert W.PROGRAMS["tree1a"][3][0] == 0 and W.PROGRAMS["tree1a"][2][-1] == 0    # saved on the first, restored on the last
    assert W.PROGRAMS["tree1b"][3][1] == 0 and W.PROGRAMS["tree1b"][2][-1] == 0    # saved on the second, restored on the last
    assert W.PROGRAMS["tree2"][3][:2] == (0, 1) and W.PROGRAMS["tree2"][2][-2:] == (1, 0)


def test_joint_types_share_a_group_of_four():
    """Revolute, prismatic and fixed joints among the first four frames of a program (one per lane of the local-transform phase)."""
    from riemannian_motion_policies_amd import urdf
    for name in ("len3", "len4", "len5", "len13"):
        t, leaf_frames = W.tables(name)
        first = {int(t.joint_type[f]) for f in W.program(t, leaf_frames)[0][:4]}
        assert first == {urdf.JOINT_REVOLUTE, urdf.JOINT_PRISMATIC, urdf.JOINT_FIXED}, (name, first)
    t, leaf_frames = W.tables("len13")
    frames = W.program(t, leaf_frames)[0]
    assert sum(1 for f in frames if t.joint_type[f] != urdf.JOINT_FIXED and t.q_index[f] < 0) == 2   # movable, held at q = 0


def test_slow_sincos_robots(sets):
    """A joint angle beyond 8 192 rad on a revolute joint of the program, inside the 17-robot and inside the 65-robot fleet only."""
    from riemannian_motion_policies_amd import urdf
    assert [r for r, _, _ in W.SLOW_SINCOS] == [3, 20]
    for name in W.ROBOTS:
        t, leaf_frames = W.tables(name)
        frames = W.program(t, leaf_frames)[0]
        q = sets[name][1]["q"]
        hit = [(r, j) for r, j, a in W.SLOW_SINCOS if j < t.n_dof and abs(q[r, j]) > 8192.0 and
               any(t.q_index[f] == j and t.joint_type[f] == urdf.JOINT_REVOLUTE for f in frames)]
        assert hit, name
        assert (np.abs(np.delete(q, [r for r, _, _ in W.SLOW_SINCOS], axis=0)) <= 1.0).all()


def test_the_oracle_resolves_every_set(sets):
    """The oracle's reference-precision and fp64 evaluations agree to a quarter of the bound on the exported (M, f) and to a
    quarter of clause A on q-double-dot: the bounds can hold a kernel on these scenes."""
    import oracle as O
    assert set(sets) == set(W.ROBOTS) | set(W.TWO_DOF)
    for name, (desc, s) in sets.items():
        kw = W.obstacle_kwargs(name)
        a, b = (O.step(desc, s["q"], s["qd"], s["goal"], precision=p, **kw) for p in ("f32", "f64"))
        for k in ("M", "f"):
            assert np.abs(a[k] - b[k]).max() <= 0.25 * W.system_bound(a[k]), (name, k)
        err = np.abs(a["qdd64"] - b["qdd64"]).max(axis=1)
        assert np.isfinite(b["qdd64"]).all() and (err <= 0.25 * 1e-5 * np.maximum(1.0, np.abs(b["qdd64"]).max(axis=1))).all(), name

"""No GPU: the sets of tests/test_gpu_quad_leaf_heads.py (tests/quad_leaf_head_scenes.py) do what its cases are named for.  The
descriptors alone say in which pattern consecutive leaf frames repeat and change their heads, and the oracle's forward kinematics
alone says that a head taken from the wrong frame would show: pairs in range on at least two leaf frames with different heads."""
import numpy as np
import pytest

import quad_build_scenes as S
import quad_leaf_head_scenes as H
from riemannian_motion_policies_amd import configs as Cf, descriptor as D


@pytest.fixture(scope="module")
def scenes():
    tables = S.make_tables()
    return tables, H.make_sets(tables)


def test_head_patterns(scenes):
    """Which leaf frames share a head, frame by frame: every obstacle leaf its own; A A B A and A B B over consecutive frames; one
    leaf-bearing frame (two leaves on it, both orders), two and nine; the target leaf last, first and between distance frames."""
    for name, (desc, _) in scenes[1].items():
        assert H.head_pattern(desc) == H.PATTERN[name], (name, H.head_pattern(desc))
    assert sorted(len(p.split("|")) for p in H.PATTERN.values())[::len(H.PATTERN) - 1] == [1, 9]
    # the cluttered set itself: eight equal heads in a row and the attractor's
    assert H.head_pattern(Cf.config3()[1]) in ("A|A|A|A|A|A|A|A|B", "A|A|A|A|A|A|B|A|A", "A|A|A|A|A|A|A|B|A")
    # two target leaves read their goals at different offsets
    desc = scenes[1]["two-targets"][0]
    offs = [desc.leaves[i].goal_offset for i in range(desc.n_leaves) if desc.leaves[i].taskmap == D.TASKMAP_FK_POSITION]
    assert sorted(offs) == [0, 3] and desc.goal_floats == 6


def test_the_heads_differ_in_every_field_a_leaf_computes_with(scenes):
    """Margin, the damping gains, P[3], P[5], the modulation radius P[7], P[8] and P[10] differ between any two variants; the
    full-mantissa set has low mantissa bits in use in (nearly) every parameter."""
    for i in range(1, 9):
        for j in range(i + 1, 9):
            a, b = np.array(H.oa_params(i), np.float32), np.array(H.oa_params(j), np.float32)
            assert all(a[k] != b[k] for k in (0, 1, 3, 5, 7, 8, 10)), (i, j)
    desc = scenes[1]["differ-full"][0]
    low = [np.array(list(desc.leaves[i].params), np.float32).view(np.uint32) & 0xFF for i in D.distance_leaf_indices(desc)]
    assert len(low) == 8 and all((l != 0).sum() >= 8 for l in low)
    for name in H.SETS:   # every variant keeps the reference's signs and a positive reach
        desc = scenes[1][name][0]
        for i in D.distance_leaf_indices(desc):
            p = list(desc.leaves[i].params)
            assert p[0] >= 0.0 and all(x > 0.0 for x in p[1:11]) and p[0] + p[7] > 0.2, (name, i)


def test_differing_heads_are_visible(scenes):
    """By the oracle's forward kinematics alone: on every fleet, the lone robot of the smallest included, every differing-heads set
    has pairs in range on at least two leaf frames whose heads differ; the far table puts none in range."""
    tables, sets = scenes
    for name in H.DIFFERING:
        desc, s = sets[name]
        for R in S.FLEETS:
            frames = H.in_range_frames(desc, s, tables["33"], R)
            heads = {tuple(desc.leaves[i].params) for i in D.distance_leaf_indices(desc) if int(desc.leaves[i].frame) in frames}
            print(f"LH in range {name} R {R}: frames {sorted(frames)}, distinct heads {len(heads)}")
            assert len(frames) >= 2 and len(heads) >= 2, (name, R, sorted(frames))
        assert not H.in_range_frames(desc, s, tables["far"], S.R_MAX)


def test_states_keep_their_clearance_with_the_widest_margin(scenes):
    """The states were filtered for the cluttered set's margin (0); the variants add up to 16 mm of margin: the control points
    still stay outside every margin-inflated sphere (the oracle's q-double-dot stays tame)."""
    tables, sets = scenes
    desc, s = sets["differ"]
    org = S.origins(desc, s["q"])
    sph = np.asarray(tables["33"], np.float64)
    clr = (np.linalg.norm(org[:, :, None, :] - sph[None, None, :, :3], axis=-1) - sph[None, None, :, 3]).min(axis=(1, 2))
    assert clr.min() - 0.016 >= 0.05

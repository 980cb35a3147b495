"""Self collision, host side: the pair rule (simulation.py:411-441 with helper/pybullet_helper.py:46-68), the capsule table and
the C entry point's argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

from riemannian_motion_policies_amd import configs as Cf
from riemannian_motion_policies_amd import descriptor as D
from riemannian_motion_policies_amd import urdf as U

# the reference's rule for config 3's leaf frames (1, 2, 3, 4, 6, 8, 9, 10) as (leaf ordinal, frame B), pinned
CONFIG3_PAIRS = [(0, 5), (0, 6), (0, 8), (0, 9), (0, 10), (1, 6), (1, 8), (1, 9), (1, 10), (2, -1), (2, 8), (2, 9), (2, 10),
                 (3, -1), (3, 0), (3, 8), (3, 9), (3, 10), (4, -1), (4, 0), (4, 1), (4, 2), (5, -1), (5, 0), (5, 1), (5, 2),
                 (5, 3), (5, 4), (6, -1), (6, 0), (6, 1), (6, 2), (6, 3), (6, 4), (6, 5), (6, 10), (7, -1), (7, 0), (7, 1),
                 (7, 2), (7, 3), (7, 4), (7, 5), (7, 9)]
# over every link of the Panda (frames 0 .. 11, leaf ordinal = frame): frames A, B as (A, B)
ALL_LINKS_PAIRS = [(0, 4), (0, 5), (0, 6), (0, 8), (0, 9), (0, 10), (1, 5), (1, 6), (1, 8), (1, 9), (1, 10), (2, 6), (2, 8),
                   (2, 9), (2, 10), (3, -1), (3, 8), (3, 9), (3, 10), (4, -1), (4, 0), (4, 8), (4, 9), (4, 10), (5, -1),
                   (5, 0), (5, 1), (5, 9), (5, 10), (6, -1), (6, 0), (6, 1), (6, 2), (8, -1), (8, 0), (8, 1), (8, 2), (8, 3),
                   (8, 4), (9, -1), (9, 0), (9, 1), (9, 2), (9, 3), (9, 4), (9, 5), (9, 10), (10, -1), (10, 0), (10, 1),
                   (10, 2), (10, 3), (10, 4), (10, 5), (10, 9)]


def _neighbours(parent, a, b, n):
    """check_link_neighborhood restated from its loop: walk up to n parents from each of the two links."""
    if a == b:
        return True
    for x, y in ((a, b), (b, a)):
        e = x
        for _ in range(n):
            if e == -1:
                break
            e = int(parent[e])
            if e == y:
                return True
    return False


def _reference_pairs(table, leaf_frames, n=3):
    out = []
    for i, a in enumerate(leaf_frames):
        for b in range(-1, table.n_frames):
            col_a = bool(table.has_collision[a])
            col_b = True if b == -1 else bool(table.has_collision[b])
            if col_a and col_b and not (_neighbours(table.parent, a, b, n) or _neighbours(table.parent, b, a, n)):
                out.append((i, b))
    return out


def test_config3_pairs_pinned():
    t = U.panda_table()
    frames = [t.frame_index(f) for f in Cf.CONTROL_POINT_FRAMES]
    assert frames == [1, 2, 3, 4, 6, 8, 9, 10]
    got = U.self_collision_pairs(t, frames)
    assert got == CONFIG3_PAIRS
    assert len(got) == 44
    assert got == _reference_pairs(t, frames)
    # hand vs link5 and left vs right finger are pairs
    assert (5, 4) in got and (6, 10) in got and (7, 9) in got


def test_all_links_pairs_pinned():
    t = U.panda_table()
    frames = list(range(t.n_frames))
    got = U.self_collision_pairs(t, frames)
    assert len(got) == 55
    assert [(frames[i], b) for i, b in got] == ALL_LINKS_PAIRS
    assert got == _reference_pairs(t, frames)
    # links without a collision shape (panda_link8, panda_grasptarget) never appear, on either side
    assert all(frames[i] not in (7, 11) and b not in (7, 11) for i, b in got)


def test_neighbourhood_width():
    t = U.panda_table()
    frames = list(range(t.n_frames))
    for n in (0, 1, 2, 4):
        assert U.self_collision_pairs(t, frames, n_neighbors=n) == _reference_pairs(t, frames, n)
    assert len(U.self_collision_pairs(t, frames, n_neighbors=1)) > 55


def test_two_joint_has_no_pairs():
    t = U.two_joint_table()
    assert U.self_collision_pairs(t, [0, 1, 2]) == []
    assert U.self_collision_pairs(t, [0, 1, 2], n_neighbors=2) == _reference_pairs(t, [0, 1, 2], 2) == [(2, -1)]
    assert U.self_collision_pairs(t, [0, 1, 2], n_neighbors=1) == _reference_pairs(t, [0, 1, 2], 1) == [(0, 2), (1, -1), (2, -1), (2, 0)]


def test_base_link():
    t = U.panda_table()
    frames = [t.frame_index(f) for f in Cf.CONTROL_POINT_FRAMES]
    got = U.self_collision_pairs(t, frames)
    # the base is B = -1 for every leaf more than 3 hops from it (link4 onward), never for link2 .. link3
    assert [i for i, b in got if b == -1] == [2, 3, 4, 5, 6, 7]
    assert all(b != -1 for i, b in U.self_collision_pairs(t, frames, base_has_collision=False))
    assert U.base_link_name(U.PANDA_URDF, t) == "panda_link0"
    caps = U.self_collision_capsules(U.PANDA_URDF, t)
    link0 = U.fitted_link_capsules(U.PANDA_URDF)["panda_link0"]
    np.testing.assert_allclose(caps[-1], [*link0["a"], link0["r"], *link0["b"], 0.0], rtol=0, atol=1e-7)
    t2 = U.two_joint_table()
    assert U.base_link_name(U.TWO_JOINT_URDF, t2) == "base_link"
    # base_link: a cylinder of length 0.05, radius 0.075 at z = 0.025 -> a capsule of zero length
    np.testing.assert_allclose(U.self_collision_capsules(U.TWO_JOINT_URDF, t2)[-1], [0, 0, 0.025, 0.075, 0, 0, 0.025, 0], atol=1e-7)


@pytest.mark.parametrize("robot", ["panda", "two_joint"])
def test_capsules_match_link_capsules(robot):
    t, path = (U.panda_table(), U.PANDA_URDF) if robot == "panda" else (U.two_joint_table(), U.TWO_JOINT_URDF)
    caps = U.self_collision_capsules(path, t)
    assert caps.shape == (t.n_frames + 1, 8) and caps.dtype == np.float32
    for f in range(t.n_frames):
        if t.has_collision[f]:
            np.testing.assert_array_equal(caps[f], U.link_capsules(path, t, [t.frame_names[f]])[0])
        else:
            assert not caps[f].any()
    if robot == "panda":
        fitted = U.fitted_link_capsules(path)
        for f in range(t.n_frames):
            cap = fitted.get(t.link_names[f])
            if t.has_collision[f] and cap is not None:
                np.testing.assert_allclose(caps[f], [*cap["a"], cap["r"], *cap["b"], 0.0], atol=1e-7)


def test_link_capsules_unchanged():
    """link_capsules (the obstacle stage's rows) after its body was shared with self_collision_capsules: pinned values."""
    t = U.panda_table()
    lc = U.link_capsules(U.PANDA_URDF, t, Cf.CONTROL_POINT_FRAMES)
    fitted = U.fitted_link_capsules(U.PANDA_URDF)
    for i, fr in enumerate(Cf.CONTROL_POINT_FRAMES):
        cap = fitted[t.link_names[t.frame_index(fr)]]
        np.testing.assert_allclose(lc[i], [*cap["a"], cap["r"], *cap["b"], 0.0], atol=1e-7)
    t2 = U.two_joint_table()
    np.testing.assert_allclose(U.link_capsules(U.TWO_JOINT_URDF, t2, ["joint_1"])[0], [0.05, 0, 0, 0.05, 0.95, 0, 0, 0], atol=1e-7)


def test_c_entry_points_without_device(hip_lib):
    import torch  # noqa: F401  (one HIP runtime per process: PyTorch's, as the package loads it)
    lib = C.CDLL(hip_lib)
    assert lib.rmp2_abi_version() == D.ABI_VERSION == 5
    lib.rmp2_set_self_collision.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.rmp2_self_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    pairs = np.zeros((1, 2), np.int32)
    caps = np.zeros((13, 8), np.float32)
    assert lib.rmp2_set_self_collision(None, 1, pairs.ctypes.data, caps.ctypes.data) == -1
    assert lib.rmp2_set_self_collision(None, 0, None, None) == -1
    assert lib.rmp2_self_pairs(None, None, None, None, None, 1, None) == -1
    with open(U.os.path.join(U.os.path.dirname(U.os.path.dirname(U.os.path.abspath(U.__file__))), "include", "rmp2.h")) as f:
        assert "#define RMP2_MAX_SELF_PAIRS 256" in f.read()

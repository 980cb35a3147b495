"""The link-capsule closest-point closed forms of rmp2_device.h (segment_segment, link_pair_fields, link_normal_length) run on the
CPU through tests/link_pairs_driver.cpp against numpy fp64 (tests/link_pair_scene.py capsule_pair_np): every pair of the two
exact scenes, random capsule pairs, and an adversarial set of the closed form's special cases.  No GPU.

Bounds are the project's (tests/test_gpu_capsules.py test_closest_points_link_geometry): 2e-6 on the distance everywhere, 2e-6 on
the points of the exact scenes and the adversarial set, 2e-5 on the points of random pairs.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "riemannian_motion_policies_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import link_pair_scene as S  # noqa: E402

EXACT = 2e-6
RANDOM_POINT = 2e-5
DIST = 2e-6


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("driver") / "link_pairs_driver")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "link_pairs_driver.cpp")], check=True, timeout=900)
    return exe


def run_driver(exe, tmp_path, A, B, lr, ca, cb):
    """fp32 inputs [N, 3], [N, 3], [N], [N, 4], [N, 4] -> dict of the driver's outputs."""
    n = len(A)
    rec = np.concatenate([A, B, np.reshape(lr, (n, 1)), ca, cb], axis=1).astype(np.float32)
    assert rec.shape == (n, 15)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.int32(n).tobytes())
        f.write(np.ascontiguousarray(rec).tobytes())
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    o = np.fromfile(tmp_path / "out.bin", dtype=np.float32).reshape(n, 15)
    return dict(s=o[:, 0], t=o[:, 1], f_link=o[:, 2:5], f_normal=o[:, 5:8], f_dist=o[:, 8], s_link=o[:, 9:12], s_obs=o[:, 12:15], all=o)


def errors(out, A, B, lr, ca, cb):
    """(point error, distance error) [N] of the driver's outputs against fp64 on the SAME fp32 inputs: both forms' surface points
    (link_pair_fields' p_obs is p_link - dist normal) and both forms' distance."""
    ref = S.capsule_pair_np(A, B, lr, ca[:, :3], cb[:, :3], ca[:, 3])
    o = {k: v.astype(np.float64) for k, v in out.items()}
    f_obs = o["f_link"] - o["f_dist"][:, None] * o["f_normal"]
    pt = np.max([np.abs(o["f_link"] - ref["p_link"]).max(axis=1), np.abs(f_obs - ref["p_obs"]).max(axis=1),
                 np.abs(o["s_link"] - ref["p_link"]).max(axis=1), np.abs(o["s_obs"] - ref["p_obs"]).max(axis=1)], axis=0)
    ds = np.maximum(np.abs(o["f_dist"] - ref["dist"]), np.abs(np.linalg.norm(o["s_link"] - o["s_obs"], axis=1) - ref["dist"]))
    return pt, ds, ref


def scene_pairs():
    """Every (row, distance leaf, live record) of the two scenes as fp32 driver inputs: the links' world segments from the oracle's
    fp64 frames (exact in fp32 on the gantry and on the two-joint arm's first link)."""
    import oracle as O
    rows = []
    for s, records in ((S.gantry(), list(S.LIVE.values())), (S.two_joint(), list(S.TWO_JOINT_SPHERES))):
        T = O.forward_kinematics(s["desc"], s["q"], "f64")[:, S.distance_frames(s["desc"])]
        lc = s["lc"].astype(np.float64)
        A = T[:, :, :3, 3] + np.einsum("rcij,cj->rci", T[:, :, :3, :3], lc[:, 0:3])
        B = T[:, :, :3, 3] + np.einsum("rcij,cj->rci", T[:, :, :3, :3], lc[:, 4:7])
        for rec in records:
            ca = rec[:4]
            cb = rec[4:8] if len(rec) == 8 else rec[:4]
            for r in range(A.shape[0]):
                for c in range(A.shape[1]):
                    rows.append(np.concatenate([A[r, c], B[r, c], [lc[c, 3]], ca, cb]))
    a = np.asarray(rows, np.float32)
    return a[:, 0:3], a[:, 3:6], a[:, 6], a[:, 7:11], a[:, 11:15]


def test_numpy_forms_agree_on_the_scenes():
    """link_pair_scene.capsule_pair_np (the reference of this file) and configs.pairs_from_link_capsules (the reference of the GPU
    tests) are two statements of the same closed form: identical on every pair of the gantry scene, crossing ones included."""
    s = S.gantry()
    n_cross = 0
    for rec in S.LIVE.values():
        tab = S.table_with(rec, 1, 0)
        pl, po, gap = S.pairs64(s, tab)
        d = np.linalg.norm(pl.astype(np.float64) - po, axis=-1)
        near = np.abs(gap) < 1                                 # (the pairs are returned in fp32: the far row's carry 4e-7)
        assert np.abs(d - np.abs(gap))[near].max() <= 1e-7
        n_cross += int((gap == -(S.LINK_R + S.OBS_R)).sum())
        cross = gap == -(S.LINK_R + S.OBS_R)
        # the convention's value: p_link - p_obs = -(r + lr) z where the axes intersect
        assert np.array_equal((pl - po)[cross], np.tile(np.float32([0, 0, -(S.LINK_R + S.OBS_R)]), (cross.sum(), 1)))
    assert n_cross >= 12


def test_exact_scenes(driver, tmp_path):
    """Measured worst over the 154 pairs (32 with intersecting axes): points 5.7e-7, distance 2.2e-7 (bound 2e-6 each)."""
    args = scene_pairs()
    out = run_driver(driver, tmp_path, *args)
    assert np.isfinite(out["all"]).all()
    pt, ds, ref = errors(out, *args)
    crossing = ref["axis"] == 0
    print(f"exact scenes: {len(pt)} pairs, {crossing.sum()} with intersecting axes; worst point {pt.max():.2e}, distance {ds.max():.2e}")
    assert crossing.sum() >= 20
    assert pt.max() <= EXACT and ds.max() <= EXACT
    # intersecting axes: the convention's value, exactly -- the normal is -z and the shapes overlap by the sum of the radii
    assert np.array_equal(out["f_normal"][crossing], np.tile(np.float32([0, 0, -1]), (crossing.sum(), 1)))
    assert np.array_equal(out["f_dist"][crossing], (args[2] + args[3][:, 3])[crossing])


def test_random_pairs(driver, tmp_path):
    """10 000 random capsule pairs (endpoints uniform in [-1, 1]^3, radii up to 0.15).  The distance bound covers EVERY pair.  Two
    classes are held to other point checks than the 2e-5 bound, because no fp32 evaluation can meet it there:
      * nearly parallel axes (within 1e-3 rad): the normal equations are ill conditioned, any point along the overlap is as near;
      * nearly INTERSECTING axes (closer than 4e-3): the surface points are X - r n, and the direction n = (X - Y) / |X - Y| of a
        vector of length dn carries the axis points' own rounding, ~ 4 eps32 = 5e-7 at unit coordinates, as 5e-7 / dn rad; times
        r = 0.15 that is 2e-5 at dn = 4e-3.  (Measured without this class: 5.5e-5 at dn = 3.4e-4.)  Their AXIS points are held
        to the bound, and their surface points to lying r from them, at 2e-6; the exactly intersecting case is test_exact_scenes'.
    The share of each class is printed and capped at 1 %."""
    rng = np.random.default_rng(20260)
    n = 10000
    A, B, Cc, Dd = (rng.uniform(-1, 1, (n, 3)).astype(np.float32) for _ in range(4))
    lr = rng.uniform(0.02, 0.1, n).astype(np.float32)
    ca = np.concatenate([Cc, rng.uniform(0.02, 0.15, (n, 1)).astype(np.float32)], axis=1)
    cb = np.concatenate([Dd, np.zeros((n, 1), np.float32)], axis=1)
    out = run_driver(driver, tmp_path, A, B, lr, ca, cb)
    assert np.isfinite(out["all"]).all()
    pt, ds, ref = errors(out, A, B, lr, ca, cb)
    d1, d2 = (B - A).astype(np.float64), (Dd - Cc).astype(np.float64)
    sin = np.linalg.norm(np.cross(d1, d2), axis=1) / (np.linalg.norm(d1, axis=1) * np.linalg.norm(d2, axis=1))
    parallel = sin < 1e-3
    crossing = ~parallel & (ref["axis"] < 4e-3)
    held = ~parallel & ~crossing
    print(f"random pairs: nearly parallel {parallel.mean():.4%}, nearly intersecting {crossing.mean():.4%}; worst point "
          f"{pt[held].max():.2e}, distance {ds.max():.2e}")
    assert parallel.mean() <= 0.01 and crossing.mean() <= 0.01
    assert ds.max() <= DIST
    assert pt[held].max() <= RANDOM_POINT
    # the axis points, from segment_segment's parameters: every pair that is not nearly parallel
    X = A + out["s"][:, None].astype(np.float64) * d1
    Y = Cc + out["t"][:, None].astype(np.float64) * d2
    ax = np.maximum(np.abs(X - ref["X"]).max(axis=1), np.abs(Y - ref["Y"]).max(axis=1))
    print(f"              worst axis point {ax[~parallel].max():.2e}")
    assert ax[~parallel].max() <= RANDOM_POINT
    for key_l, key_o in (("f_link", None), ("s_link", "s_obs")):
        pl = out[key_l].astype(np.float64)
        po = out[key_o].astype(np.float64) if key_o else pl - out["f_dist"][:, None].astype(np.float64) * out["f_normal"]
        assert np.abs(np.linalg.norm(pl - ref["X"], axis=1) - lr)[crossing].max(initial=0) <= DIST
        assert np.abs(np.linalg.norm(po - ref["Y"], axis=1) - ca[:, 3])[crossing].max(initial=0) <= DIST


def adversarial_pairs():
    """The closed form's special cases on dyadic coordinates: (name, A, B, C, D, points_unique)."""
    z = 0.5
    cases = [
        ("parallel_offset", (0, 0, z), (1, 0, z), (0.25, 0.5, z), (1.25, 0.5, z), False),
        ("parallel_disjoint", (0, 0, z), (1, 0, z), (2, 0.5, z), (3, 0.5, z), True),
        ("antiparallel", (0, 0, z), (1, 0, z), (1.25, 0.5, z), (0.25, 0.5, z), False),
        ("collinear_disjoint", (0, 0, z), (1, 0, z), (1.5, 0, z), (2.5, 0, z), True),
        ("collinear_overlap", (0, 0, z), (1, 0, z), (0.5, 0, z), (1.5, 0, z), False),
        ("collinear_touch", (0, 0, z), (1, 0, z), (1, 0, z), (2, 0, z), True),
        ("zero_link", (0.5, 0.25, z), (0.5, 0.25, z), (0, 0, z), (1, 0, z), True),
        ("zero_link_on_axis", (0.5, 0, z), (0.5, 0, z), (0, 0, z), (1, 0, z), True),
        ("zero_obstacle", (0, 0, z), (1, 0, z), (0.5, 0.25, z), (0.5, 0.25, z), True),
        ("zero_obstacle_on_axis", (0, 0, z), (1, 0, z), (0.25, 0, z), (0.25, 0, z), True),
        ("both_zero", (0, 0, z), (0, 0, z), (0.5, 0.25, z), (0.5, 0.25, z), True),
        ("both_zero_coincident", (0.5, 0.25, z), (0.5, 0.25, z), (0.5, 0.25, z), (0.5, 0.25, z), True),
        ("t_clamped_0", (0, 0, z), (1, 0, z), (0.5, 0.25, z), (0.5, 1.25, z), True),
        ("t_clamped_1", (0, 0, z), (1, 0, z), (0.5, -1.25, z), (0.5, -0.25, z), True),
        ("s_clamped_0", (0, 0, z), (1, 0, z), (-0.5, -1, z + 0.25), (-0.5, 1, z + 0.25), True),
        ("s_clamped_1", (0, 0, z), (1, 0, z), (1.5, -1, z + 0.25), (1.5, 1, z + 0.25), True),
        ("both_clamped", (0, 0, z), (1, 0, z), (1.5, 0.5, z + 0.25), (2.5, 1.5, z + 0.75), True),
        ("crossing_interior", (0, 0, z), (1, 0, z), (0.5, -0.5, z), (0.5, 0.5, z), True),
        ("crossing_at_ends", (0, 0, z), (1, 0, z), (1, 0, z), (1, 1, z), True),
        ("skew", (0, 0, z), (1, 0, z), (0.5, -0.5, z + 0.25), (0.5, 0.5, z + 0.25), True),
    ]
    return cases


def test_adversarial_pairs(driver, tmp_path):
    cases = adversarial_pairs()
    A, B, Cc, Dd = (np.asarray([c[k] for c in cases], np.float32) for k in (1, 2, 3, 4))
    n = len(cases)
    lr = np.full(n, S.LINK_R, np.float32)
    ca = np.concatenate([Cc, np.full((n, 1), S.OBS_R, np.float32)], axis=1)
    cb = np.concatenate([Dd, np.zeros((n, 1), np.float32)], axis=1)
    out = run_driver(driver, tmp_path, A, B, lr, ca, cb)
    assert np.isfinite(out["all"]).all(), [cases[i][0] for i in np.nonzero(~np.isfinite(out["all"]).all(axis=1))[0]]
    assert ((out["s"] >= 0) & (out["s"] <= 1) & (out["t"] >= 0) & (out["t"] <= 1)).all()
    pt, ds, ref = errors(out, A, B, lr, ca, cb)
    unique = np.asarray([c[5] for c in cases])
    print("adversarial:", {c[0]: (float(f"{p:.1e}"), float(f"{d:.1e}")) for c, p, d in zip(cases, pt, ds)})
    assert ds.max() <= DIST, cases[int(ds.argmax())][0]
    assert pt[unique].max() <= EXACT, cases[int(np.where(unique, pt, 0).argmax())][0]
    # where the nearest points are not unique (overlapping parallel axes) both forms still give A pair at the right distance, on
    # the two surfaces: the points lie on their capsules
    for k in np.nonzero(~unique)[0]:
        for key in ("f_link", "s_link"):
            _, Y = S.seg_seg_np(out[key][k:k + 1], out[key][k:k + 1], A[k:k + 1], B[k:k + 1])   # (nearest point of the link's axis)
            assert abs(np.linalg.norm(out[key][k].astype(np.float64) - Y[0]) - S.LINK_R) <= EXACT, cases[k][0]
    # the clamps are what their names say
    by = {c[0]: i for i, c in enumerate(cases)}
    assert out["t"][by["t_clamped_0"]] == 0 and out["t"][by["t_clamped_1"]] == 1
    assert out["s"][by["s_clamped_0"]] == 0 and out["s"][by["s_clamped_1"]] == 1
    assert out["s"][by["both_clamped"]] == 1 and out["t"][by["both_clamped"]] == 0
    for name in ("zero_link_on_axis", "zero_obstacle_on_axis", "both_zero_coincident", "crossing_interior", "crossing_at_ends", "collinear_touch"):
        assert ref["axis"][by[name]] == 0 and np.array_equal(out["f_normal"][by[name]], np.float32([0, 0, -1])), name

"""Hull-versus-hull self pairs on the host: the hull table urdf.self_collision_hulls builds, the fp64 restatement
(tests/hull_pair_reference.py) on pinned answers, the device routine rmp2_hull.h hull_pair_closest run on the CPU through a small
driver against that restatement, and the new C symbol.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hull_pair_reference as HP  # noqa: E402
import hull_scene as HS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "riemannian_motion_policies_amd", "csrc")
needs_hipcc = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc is not installed")


@pytest.fixture(scope="module")
def self_hull_driver(tmp_path_factory):
    """tests/self_hull_driver.cpp compiled for the host once: run(hulls [(V, P)], queries [(A, B, Rm, t)]) -> [N, 12] = pa, pb, u,
    gap, iters, face."""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("self_hull_driver")
    exe = str(d / "self_hull_driver")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "self_hull_driver.cpp")], check=True, timeout=600)
    count = [0]

    def run(hulls, queries):
        count[0] += 1
        fin, fout = str(d / f"in{count[0]}.bin"), str(d / f"out{count[0]}.bin")
        with open(fin, "wb") as f:
            np.array([len(hulls)], np.int32).tofile(f)
            for V, P in hulls:
                np.array([len(V), len(P)], np.int32).tofile(f)
                np.ascontiguousarray(V, np.float32).tofile(f)
                np.ascontiguousarray(P, np.float32).tofile(f)
            np.array([len(queries)], np.int32).tofile(f)
            for ia, ib, Rm, t in queries:
                np.array([ia, ib], np.int32).tofile(f)
                np.ascontiguousarray(Rm, np.float64).tofile(f)
                np.ascontiguousarray(t, np.float64).tofile(f)
        subprocess.run([exe, fin, fout], check=True, timeout=300)
        return np.fromfile(fout, np.float64).reshape(len(queries), 12)

    return run


def _meshes(golden_dir):
    z = np.load(os.path.join(golden_dir, "panda_collision_meshes.npz"))
    return {str(n): (z[f"{n}.vertices"], z[f"{n}.xyz"], z[f"{n}.rpy"]) for n in z["links"]}


def test_self_collision_hulls_layout(golden_dir):
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    t = U.panda_table()
    meshes = _meshes(golden_dir)
    h = U.self_collision_hulls(U.PANDA_URDF, t, meshes)
    F = t.n_frames
    assert len(h) == F + 1
    # the pair leaves' rows are bit for bit link_hulls
    frames = Cf.CONTROL_POINT_FRAMES
    lh = U.link_hulls(t, frames, meshes)
    for i, fr in enumerate(frames):
        for a, b in zip(h.hull(t.frame_index(fr)), lh.hull(i)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), fr
    sub = h.subset([t.frame_index(fr) for fr in frames])
    for a, b in zip((sub.vert_offset, sub.verts, sub.face_offset, sub.planes), (lh.vert_offset, lh.verts, lh.face_offset, lh.planes)):
        assert a.tobytes() == b.tobytes()
    # the base row is link 0 in base coordinates, placed as link_hulls places a link
    V, xyz, rpy = meshes["panda_link0"]
    want_v, want_p = U.convex_hull(V @ U.rotation_from_rpy_reference_order(rpy).astype(np.float64).T + xyz)
    bv, bp = h.hull(F)
    assert bv.tobytes() == want_v.astype(np.float32).tobytes() and bp.tobytes() == want_p.astype(np.float32).tobytes()
    # collision-less frames are empty, every other one is not
    for f in range(F):
        nv, nf = len(h.hull(f)[0]), len(h.hull(f)[1])
        assert (nv == 0 and nf == 0) == (not t.has_collision[f]), f
    # the sizes of the issue: links 1-5 152 / 300, link 6 260 / 516, link 0, 7, hand 102 / 200, fingers 18 / 32
    sizes = {t.link_names[f]: (len(h.hull(f)[0]), len(h.hull(f)[1])) for f in range(F) if t.has_collision[f]}
    sizes["panda_link0"] = (len(bv), len(bp))
    for i in range(1, 6):
        assert sizes[f"panda_link{i}"] == (152, 300)
    assert sizes["panda_link6"] == (260, 516)
    for n in ("panda_link0", "panda_link7", "panda_hand"):
        assert sizes[n] == (102, 200)
    assert sizes["panda_leftfinger"] == sizes["panda_rightfinger"] == (18, 32)
    assert h.vert_offset[-1] == 1362 and h.face_offset[-1] == 2680
    assert max(s[0] for s in sizes.values()) <= U.MAX_HULL_VERTICES and max(s[1] for s in sizes.values()) <= U.MAX_HULL_FACES


def test_self_collision_hulls_refusals(golden_dir):
    from riemannian_motion_policies_amd import urdf as U
    t = U.panda_table()
    meshes = _meshes(golden_dir)
    for missing in ("panda_link3", "panda_link0"):
        m = dict(meshes)
        del m[missing]
        with pytest.raises(ValueError, match="no collision mesh"):
            U.self_collision_hulls(U.PANDA_URDF, t, m)
    rng = np.random.default_rng(0)
    sphere = rng.normal(size=(4000, 3))
    sphere /= np.linalg.norm(sphere, axis=1, keepdims=True)
    with pytest.raises(ValueError, match="at most"):
        U.self_collision_hulls(U.PANDA_URDF, t, dict(meshes, panda_link2=sphere))


CUBE = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)


def _cube():
    from riemannian_motion_policies_amd import urdf as U
    return HP.Hull(*U.convex_hull(CUBE))


def test_restatement_pinned_on_unit_cubes():
    A = _cube()
    # separated face to face: B one unit plus 0.5 above A
    pa, pb, u, g, face = HP.pair_closest(A, A, np.eye(3), [0.0, 0.0, 1.5])
    assert not face and np.isclose(g, 0.5) and np.allclose(u, [0, 0, -1])
    assert np.isclose(pa[2], 1.0) and np.isclose(pb[2], 1.5) and np.allclose(pa[:2], pb[:2])
    # edge to edge, skew: A's edge x = z = 1 (along y) against B's edge (0, 0, 0)-(1, 0, 0), B turned so that that edge runs
    # along a = (1, 0, -1) / sqrt2 with its outward bisector -(y + z) / sqrt2 facing -n, n = (1, 0, 1) / sqrt2, and its midpoint
    # placed h along n from the midpoint of A's edge: the common perpendicular is n, the distance h
    h = 0.3
    a_, n_, ey = np.array([1.0, 0, -1]) / np.sqrt(2), np.array([1.0, 0, 1]) / np.sqrt(2), np.array([0.0, 1, 0])
    Rm = np.stack([a_, (n_ + ey) / np.sqrt(2), (n_ - ey) / np.sqrt(2)], axis=1)
    assert np.allclose(Rm @ Rm.T, np.eye(3)) and np.isclose(np.linalg.det(Rm), 1.0)
    mid = np.array([1.0, 0.5, 1.0])
    t = mid + h * n_ - 0.5 * a_
    pa, pb, u, g, face = HP.pair_closest(A, A, Rm, t)
    assert not face and np.isclose(g, h) and np.allclose(pa, mid) and np.allclose(pb, mid + h * n_) and np.allclose(u, -n_)
    # overlap along +x: B shifted by 0.8 in x overlaps A by 0.2: A's +x face (s = 0.8 - 1 = -0.2) is the least penetration
    pa, pb, u, g, face = HP.pair_closest(A, A, np.eye(3), [0.8, 0.1, 0.2])
    assert face and np.isclose(g, -0.2) and np.allclose(u, [-1, 0, 0])
    assert np.isclose(pb[0], 0.8) and np.isclose(pa[0], 1.0) and np.allclose(pa[1:], pb[1:])
    # overlap along -x: B shifted by -0.7 overlaps A by 0.3 along x: A's -x face (s = min -y - max -x = -0.3 - 0) is the
    # least penetration, n* = -x, y* = B's vertex of largest x (0.3)
    pa, pb, u, g, face = HP.pair_closest(A, A, np.eye(3), [-0.7, 0.1, 0.2])
    assert face and np.isclose(g, -0.3) and np.allclose(u, [1, 0, 0]) and np.isclose(pb[0], 0.3) and np.isclose(pa[0], 0.0)
    # containment: a small cube deep inside: the face rule still gives the least translation
    small = HP.Hull(CUBE * 0.1, np.array([[1, 0, 0, 0.1], [-1, 0, 0, 0], [0, 1, 0, 0.1], [0, -1, 0, 0], [0, 0, 1, 0.1],
                                          [0, 0, -1, 0]], float))
    pa, pb, u, g, face = HP.pair_closest(A, small, np.eye(3), [0.85, 0.45, 0.45])
    assert face and np.isclose(g, -(1.0 - 0.85)) and np.allclose(u, [-1, 0, 0])


def _panda_hulls(golden_dir):
    from riemannian_motion_policies_amd import urdf as U
    t = U.panda_table()
    return t, U.self_collision_hulls(U.PANDA_URDF, t, _meshes(golden_dir))


def _random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


@needs_hipcc
def test_device_routine_on_the_cpu_against_the_restatement(golden_dir, self_hull_driver):
    t, h = _panda_hulls(golden_dir)
    entries = [e for e in range(len(h)) if len(h.hull(e)[0])]
    rng = np.random.default_rng(7)
    N = 5000
    ia, ib = rng.choice(entries, N), rng.choice(entries, N)
    Rm = _random_rotations(rng, N)
    # B's centroid placed at a random offset from A's: sized by the two hulls so that about a third overlap
    cen = {e: h.hull(e)[0].astype(np.float64).mean(0) for e in entries}
    rad = {e: np.linalg.norm(h.hull(e)[0].astype(np.float64) - cen[e], axis=1).max() for e in entries}
    dirs = rng.normal(size=(N, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    reach = np.array([rad[a] + rad[b] for a, b in zip(ia, ib)]) * rng.uniform(0.2, 1.2, N)
    t = np.array([cen[a] - Rm[k] @ cen[b] for k, (a, b) in enumerate(zip(ia, ib))]) + dirs * reach[:, None]
    # (empty entries are never queried: give the driver a placeholder)
    packed = [h.hull(e) if len(h.hull(e)[0]) else (np.zeros((1, 3), np.float32), np.array([[0, 0, 1, 0]], np.float32)) for e in range(len(h))]
    out = self_hull_driver(packed, [(ia[k], ib[k], Rm[k], t[k]) for k in range(N)])
    cache = {e: HP.Hull(*h.hull(e)) for e in entries}
    n_face = 0
    for k in range(N):
        pa, pb, u, g, face = HP.pair_closest(cache[ia[k]], cache[ib[k]], Rm[k], t[k])
        dpa, dpb, du, dg, iters, dface = out[k, 0:3], out[k, 3:6], out[k, 6:9], out[k, 9], out[k, 10], out[k, 11]
        assert iters < 64, k                                        # stays under the cap (kPairGjkIters)
        assert bool(dface) == face, (k, g, dg)
        assert abs(dg - g) <= 1e-9, (k, g, dg)
        n_face += face
        if face and HP.face_margin(cache[ia[k]], cache[ib[k]], Rm[k], t[k]) < 1e-9:
            continue   # (two faces tie: either n* is the rule's answer)
        assert np.abs(dpa - pa).max() <= 1e-9 and np.abs(dpb - pb).max() <= 1e-9, (k, face, dpa - pa, dpb - pb)
        assert np.abs(du - u).max() <= 1e-6, (k, du, u)
    assert 0.1 * N < n_face < 0.7 * N                               # both regimes are covered


def test_symbol_declared_and_bound(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    assert "int rmp2_set_self_collision_hulls(rmp2_handle *h, int32_t n_pairs, const int32_t *pairs, int32_t n_hulls," in hdr
    assert "#define RMP2_ABI_VERSION 5" in hdr
    src = open(os.path.join(ROOT, "riemannian_motion_policies_amd", "_native.py")).read()
    assert "l.rmp2_set_self_collision_hulls.argtypes" in src
    import torch  # noqa: F401  (one HIP runtime per process: PyTorch's first, as _native.lib loads it)
    lib = C.CDLL(hip_lib)
    assert hasattr(lib, "rmp2_set_self_collision_hulls")
    lib.rmp2_set_self_collision_hulls.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
    assert lib.rmp2_set_self_collision_hulls(None, 0, None, 0, None, None, None, None) == -1   # a NULL handle, before any device work


# ---- the degenerate catalogue: exact cubes against closed forms --------------------------------------------------------------
def test_pair_catalogue_gaps_agree_with_the_restatement():
    """The hand-written gaps of the hull-pair catalogue against the restatement (no device answer is looked at)."""
    for row in HS.pair_catalogue():
        A, B = HP.Hull(*HS.HULLS[row["A"]]), HP.Hull(*HS.HULLS[row["B"]])
        g = HP.pair_closest(A, B, row["Rm"], row["t"])[3]
        assert abs(g - row["sep"]) <= 1e-12, (row["name"], g, row["sep"])


@needs_hipcc
def test_degenerate_pair_catalogue_on_the_cpu(self_hull_driver):
    """hull_pair_closest on exact cubes against CLOSED FORMS at 1e-12: faces parallel and apart (aligned, offset by half, turned
    45 degrees about the normal), parallel and skew edges apart, vertices apart, touching at a face, an edge and a vertex, an edge
    resting on a face, coincident, contained and far.  Rows whose nearest pair is a set and rows whose face rule ties are named
    in the catalogue (tests/hull_scene.py) and held by membership.  Measured: worst error 4.4e-16 (4.4e-4 of the bound) over the 13 rows, at
    most 3 iterations of 64."""
    rows = HS.pair_catalogue()
    names = sorted({r["A"] for r in rows} | {r["B"] for r in rows})
    out = self_hull_driver([HS.HULLS[n] for n in names], [(names.index(r["A"]), names.index(r["B"]), r["Rm"], r["t"]) for r in rows])
    worst, iters = 0.0, 0
    for row, o in zip(rows, out):
        assert o[10] < 64, row["name"]
        iters = max(iters, int(o[10]))
        assert bool(o[11]) == (row["sep"] <= 1e-7), (row["name"], o[11])        # the face rule exactly where the hulls touch or overlap
        worst = max(worst, HS.check_pair_row(row, o[0:3], o[3:6], o[6:9], o[9], 1e-12))
    assert {r["kind"] for r in rows} == {"unique", "set", "tie"}
    print(f"hull_pair_closest degenerate catalogue, {len(rows)} rows: worst error / 1e-12 = {worst:.2e}, iterations {iters} of 64")


@needs_hipcc
def test_non_finite_placement_on_the_cpu(self_hull_driver):
    """include/rmp2.h: a non-finite frame (a robot's non-finite q) makes the pair NaN -- never gap = -1e300 beside a finite u."""
    rows = HS.nonfinite_pair_rows()
    out = self_hull_driver([HS.HULLS["cube"]], [(0, 0, Rm, t) for _, Rm, t in rows])
    for (name, *_), o in zip(rows, out):
        assert np.isnan(o[:10]).all(), (name, o)
    o = self_hull_driver([HS.HULLS["cube"]], [(0, 0, np.eye(3), [1.5, 1.5, 1.5])])[0]
    assert abs(o[9] - HS.S3 / 2) <= 1e-15 and np.array_equal(o[0:6], [1, 1, 1, 1.5, 1.5, 1.5])

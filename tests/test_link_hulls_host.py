"""Convex-hull link geometry on the host: the hulls urdf.link_hulls compiles from the Panda's collision meshes, the fp64
restatement of the hull stage (tests/hull_reference.py) on pinned answers, collision_meshes on a small URDF, and the new C
symbols.  No GPU."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hull_reference as H  # noqa: E402
import hull_scene as HS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "riemannian_motion_policies_amd", "csrc")
needs_hipcc = pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "hipcc")) is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                 reason="hipcc is not installed")


def _meshes(golden_dir):
    z = np.load(os.path.join(golden_dir, "panda_collision_meshes.npz"))
    return {str(n): (z[f"{n}.vertices"], z[f"{n}.xyz"], z[f"{n}.rpy"]) for n in z["links"]}


def test_panda_hulls(golden_dir):
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    meshes = _meshes(golden_dir)
    t = U.panda_table()
    frames = Cf.CONTROL_POINT_FRAMES + ["panda_joint1", "panda_joint6"]
    hulls = U.link_hulls(t, frames, meshes)
    assert len(hulls) == len(frames)
    caps = json.load(open(os.path.join(ROOT, "riemannian_motion_policies_amd", "robots", "panda_link_capsules.json")))["links"]
    for i, fr in enumerate(frames):
        link = t.link_names[t.frame_index(fr)]
        V, xyz, rpy = meshes[link]
        Rc = U.rotation_from_rpy_reference_order(rpy).astype(np.float64)
        P = V @ Rc.T + xyz                                     # mesh vertices in the frame's coordinates
        hv, hp = hulls.hull(i)
        hv, hp = hv.astype(np.float64), hp.astype(np.float64)
        assert 4 <= len(hv) <= U.MAX_HULL_VERTICES and 4 <= len(hp) <= U.MAX_HULL_FACES
        n, d = hp[:, :3], hp[:, 3]
        assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6                 # unit normals
        # every mesh vertex satisfies every plane (fp32 storage of the planes: 1e-7 m of rounding on top of 1e-9)
        assert (P @ n.T - d).max() <= 1e-9 + 2e-7, fr
        # every hull vertex is a mesh vertex
        dmin = np.sqrt(((hv[:, None, :] - P[None]) ** 2).sum(-1)).min(axis=1)
        assert dmin.max() <= 1e-6, fr
        # outward: the hull's centroid is strictly inside every plane
        assert (hv.mean(0) @ n.T - d).max() < -1e-4, fr
        # each plane touches the hull
        assert np.abs((hv @ n.T - d).max(axis=0)).max() <= 1e-6, fr
        # the hull lies inside the fitted capsule of the same link
        c = caps[link]
        a, b = np.asarray(c["a"]), np.asarray(c["b"])
        ab = b - a
        s = np.clip(((hv - a) @ ab) / max(float(ab @ ab), 1e-30), 0.0, 1.0)
        assert np.linalg.norm(hv - (a + np.outer(s, ab)), axis=1).max() <= c["r"] + 1e-6, fr


def test_link_hulls_refuses_missing_and_large(golden_dir):
    from riemannian_motion_policies_amd import urdf as U
    t = U.panda_table()
    meshes = _meshes(golden_dir)
    with pytest.raises(ValueError, match="no collision mesh"):
        U.link_hulls(t, ["panda_joint2"], {})
    # a caller-supplied vertex set in link coordinates is taken as is
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64) * 0.1
    h = U.link_hulls(t, ["panda_joint2"], {"panda_link2": cube})
    assert len(h.hull(0)[0]) == 8 and len(h.hull(0)[1]) == 6           # coplanar triangles merged: six faces
    rng = np.random.default_rng(0)
    sphere = rng.normal(size=(4000, 3))
    sphere /= np.linalg.norm(sphere, axis=1, keepdims=True)
    with pytest.raises(ValueError, match="at most"):
        U.link_hulls(t, ["panda_joint2"], {"panda_link2": sphere})
    assert len(U.link_hulls(t, ["panda_joint2"], meshes).hull(0)[0]) == 152


CUBE = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)


def _cube():
    from riemannian_motion_policies_amd import urdf as U
    return U.convex_hull(CUBE)


def test_restatement_pinned_on_a_unit_cube():
    V, P = _cube()
    q = lambda *p: np.asarray([p], dtype=np.float64)           # noqa: E731
    r = 0.1
    # outside a face
    hp, xp, u, g = H.hull_closest(V, P, q(0.5, 0.5, 1.5), q(0.5, 0.5, 1.5), [r])
    assert np.allclose(hp, [[0.5, 0.5, 1.0]]) and np.allclose(u, [[0, 0, -1]]) and np.isclose(g[0], 0.5 - r)
    # outside an edge
    hp, xp, u, g = H.hull_closest(V, P, q(1.3, 0.5, 1.4), q(1.3, 0.5, 1.4), [r])
    assert np.allclose(hp, [[1.0, 0.5, 1.0]]) and np.isclose(g[0], 0.5 - r)
    assert np.allclose(u, [[-0.6, 0.0, -0.8]])
    # outside a corner
    hp, xp, u, g = H.hull_closest(V, P, q(-1, -2, -2), q(-1, -2, -2), [r])
    assert np.allclose(hp, [[0, 0, 0]]) and np.isclose(g[0], 3.0 - r)
    # a point inside: the face of least translation (x = 0.9: the +x face, t = 0.1)
    hp, xp, u, g = H.hull_closest(V, P, q(0.9, 0.5, 0.4), q(0.9, 0.5, 0.4), [r])
    assert np.allclose(hp, [[1.0, 0.5, 0.4]]) and np.allclose(xp, [[0.9, 0.5, 0.4]]) and np.allclose(u, [[-1, 0, 0]])
    assert np.isclose(g[0], -(0.1 + r))
    # a segment piercing the cube along z: the +x face needs 0.2, the +z face (min endpoint z = -1) 2.0 -> +x, at endpoint a
    hp, xp, u, g = H.hull_closest(V, P, q(0.8, 0.5, -1.0), q(0.8, 0.5, 2.0), [r])
    assert np.allclose(u, [[-1, 0, 0]]) and np.isclose(g[0], -(0.2 + r))
    assert np.allclose(xp, [[0.8, 0.5, -1.0]]) and np.allclose(hp, [[1.0, 0.5, -1.0]])
    # a segment passing beside an edge: its nearest pair is the segment's interior against the edge
    hp, xp, u, g = H.hull_closest(V, P, q(1.5, -1.0, 1.5), q(1.5, 2.0, 1.5), [r])
    assert np.allclose(hp[0, [0, 2]], [1.0, 1.0]) and np.allclose(xp[0, [0, 2]], [1.5, 1.5])
    assert np.isclose(g[0], np.sqrt(0.5) - r)


def test_restatement_against_dense_sampling():
    """The brute-force outside case against the distance to a dense sampling of the cube's surface (an independent bound)."""
    V, P = _cube()
    rng = np.random.default_rng(1)
    c = rng.uniform(-1.0, 2.0, size=(300, 3))
    hp, xp, u, g = H.hull_closest(V, P, c, c, np.zeros(300))
    s = np.linspace(0, 1, 41)
    A, B = np.meshgrid(s, s)
    pts = []
    for ax in range(3):
        for side in (0.0, 1.0):
            f = np.zeros((A.size, 3))
            f[:, ax] = side
            f[:, (ax + 1) % 3], f[:, (ax + 2) % 3] = A.ravel(), B.ravel()
            pts.append(f)
    pts = np.concatenate(pts)
    dmin = np.sqrt(((c[:, None] - pts[None]) ** 2).sum(-1)).min(1)
    outside = (c < 0).any(1) | (c > 1).any(1)
    assert (g[outside] <= dmin[outside] + 1e-12).all() and (dmin[outside] - g[outside]).max() <= 0.02


def test_collision_meshes_round_trip(tmp_path):
    from riemannian_motion_policies_amd import urdf as U
    (tmp_path / "meshes").mkdir()
    with open(tmp_path / "meshes" / "box.obj", "w") as f:
        f.write("# box\n")
        for v in CUBE * 0.2:
            f.write(f"v {v[0]} {v[1]} {v[2]}\n")
        f.write("vn 0 0 1\nf 1 2 3\n")
    urdf = tmp_path / "r.urdf"
    urdf.write_text("""<robot name="r">
  <link name="base"/>
  <link name="arm"><collision><origin xyz="0.1 0 0.2" rpy="0 0 1.5707963"/>
    <geometry><mesh filename="package://meshes/box.obj"/></geometry></collision></link>
  <link name="tip"><collision><geometry><sphere radius="0.1"/></geometry></collision></link>
  <joint name="j1" type="revolute"><parent link="base"/><child link="arm"/><axis xyz="0 0 1"/>
    <limit lower="-1" upper="1" effort="1" velocity="1"/></joint>
  <joint name="j2" type="fixed"><parent link="arm"/><child link="tip"/><origin xyz="0 0 0.5"/></joint>
</robot>""")
    m = U.collision_meshes(str(urdf))
    assert list(m) == ["arm"]
    V, xyz, rpy = m["arm"]
    assert np.allclose(V, CUBE * 0.2) and np.allclose(xyz, [0.1, 0, 0.2]) and np.allclose(rpy, [0, 0, 1.5707963])
    t = U.compile_urdf(str(urdf), ["j1"])
    h = U.link_hulls(t, ["j1"], m)
    hv = h.hull(0)[0].astype(np.float64)
    Rc = U.rotation_from_rpy_reference_order(rpy).astype(np.float64)
    want = CUBE * 0.2 @ Rc.T + xyz
    assert len(hv) == 8 and np.sqrt(((hv[:, None] - want[None]) ** 2).sum(-1)).min(1).max() <= 1e-6
    assert U.collision_meshes(U.PANDA_URDF) == {}          # the package's kinematics-only URDF has no meshes


def test_symbols_declared_and_bound(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "rmp2.h")).read()
    for sym in ("rmp2_set_link_hulls", "rmp2_closest_points_hulls", "RMP2_MAX_HULL_VERTICES", "RMP2_MAX_HULL_FACES"):
        assert sym in hdr, sym
    assert "#define RMP2_ABI_VERSION 5" in hdr
    from riemannian_motion_policies_amd import urdf as U
    assert f"#define RMP2_MAX_HULL_VERTICES {U.MAX_HULL_VERTICES}" in hdr
    assert f"#define RMP2_MAX_HULL_FACES {U.MAX_HULL_FACES}" in hdr
    import torch  # noqa: F401  (one HIP runtime per process: PyTorch's first, as _native.lib loads it)
    lib = C.CDLL(hip_lib)
    for sym in ("rmp2_set_link_hulls", "rmp2_closest_points_hulls"):
        assert hasattr(lib, sym), sym
    # the package's declarations (riemannian_motion_policies_amd/_native.py) name both, with the C argument counts
    src = open(os.path.join(ROOT, "riemannian_motion_policies_amd", "_native.py")).read()
    assert "l.rmp2_set_link_hulls.argtypes" in src and "l.rmp2_closest_points_hulls.argtypes" in src
    lib.rmp2_set_link_hulls.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rmp2_closest_points_hulls.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.c_void_p]
    # a NULL handle is refused before any device work
    assert lib.rmp2_set_link_hulls(None, 0, None, None, None, None) == -1
    assert lib.rmp2_closest_points_hulls(None, None, None, None, None, None, 1, None) == -1


# ---- the device routine hull_closest on the CPU ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def link_hull_driver(tmp_path_factory):
    """tests/link_hull_driver.cpp compiled for the host once: run(hulls [(V, P)], queries [(hull, a, b, r)]) -> [N, 11] =
    hp, xp, u, gap, iters."""
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("link_hull_driver")
    exe = str(d / "link_hull_driver")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "link_hull_driver.cpp")], check=True, timeout=600)
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
            for h, a, b, r in queries:
                np.array([h], np.int32).tofile(f)
                np.array([*a, *b, r], np.float64).tofile(f)
        subprocess.run([exe, fin, fout], check=True, timeout=300)
        return np.fromfile(fout, np.float64).reshape(len(queries), 11)

    return run


def _link_face_margin(P, a, b):
    """Second-smallest minus smallest t_f of the face rule (how well f*, and with it the points, are determined)."""
    P = np.asarray(P, np.float64)
    t = np.sort(P[:, 3] - np.minimum(P[:, :3] @ a, P[:, :3] @ b))
    return t[1] - t[0]


@needs_hipcc
def test_device_routine_on_the_cpu_against_the_restatement(golden_dir, link_hull_driver):
    """rmp2_hull.h hull_closest, compiled for the host, on 6 000 point and 6 000 segment queries against the Panda's hulls: the
    brute-force restatement at 1e-9 m (gap, both points) and 1e-6 (u), and the iteration cap is not reached -- a pair that ran
    into it would silently keep the best simplex found.  Measured: worst gap error 8.3e-17 m and worst point error 1.0e-13 m
    (1e-4 of the bound 1e-9), worst u error 1.3e-12 (1e-6 of its bound), at most 13 iterations of 32."""
    from riemannian_motion_policies_amd import configs as Cf, urdf as U
    hulls = U.link_hulls(U.panda_table(), Cf.CONTROL_POINT_FRAMES, _meshes(golden_dir))
    HV = [tuple(x.astype(np.float64) for x in hulls.hull(i)) for i in range(len(hulls))]
    rng = np.random.default_rng(17)
    N = 6000
    worst = dict(gap=0.0, pts=0.0, u=0.0, iters=0)
    for seg in (False, True):
        hi = rng.integers(0, len(HV), N)
        cen = np.array([HV[h][0].mean(0) for h in hi])
        rad = np.array([np.linalg.norm(HV[h][0] - HV[h][0].mean(0), axis=1).max() for h in hi])
        d = rng.normal(size=(N, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        a = cen + d * (rad * rng.uniform(0.0, 1.5, N))[:, None]
        if seg:
            e = rng.normal(size=(N, 3))
            e /= np.linalg.norm(e, axis=1, keepdims=True)
            b = a + e * rng.uniform(0.02, 0.3, N)[:, None]
        else:
            b = a.copy()
        r = rng.uniform(0.0, 0.1, N)
        out = link_hull_driver(HV, [(int(hi[k]), a[k], b[k], r[k]) for k in range(N)])
        n_meet = 0
        for h in range(len(HV)):
            m = np.nonzero(hi == h)[0]
            hp, xp, u, g = H.hull_closest(HV[h][0], HV[h][1], a[m], b[m], r[m])
            for j, k in enumerate(m):
                dhp, dxp, du, dg, iters = out[k, 0:3], out[k, 3:6], out[k, 6:9], out[k, 9], out[k, 10]
                assert iters < 32, (k, iters)                            # under the cap (kHullGjkIters)
                worst["iters"] = max(worst["iters"], int(iters))
                assert abs(dg - g[j]) <= 1e-9, (seg, k, g[j], dg)
                worst["gap"] = max(worst["gap"], abs(dg - g[j]))
                meets = g[j] + r[k] <= H.TOUCH
                n_meet += meets
                if meets and _link_face_margin(HV[h][1], a[k], b[k]) < 1e-9:
                    continue   # (two faces tie: either is the rule's answer)
                e_pts = max(np.abs(dhp - hp[j]).max(), np.abs(dxp - xp[j]).max())
                assert e_pts <= 1e-9, (seg, k, meets, dhp - hp[j], dxp - xp[j])
                assert np.abs(du - u[j]).max() <= 1e-6, (seg, k, du, u[j])
                worst["pts"], worst["u"] = max(worst["pts"], e_pts), max(worst["u"], np.abs(du - u[j]).max())
        assert 0.2 * N < n_meet < 0.5 * N, n_meet                        # both regimes, roughly a third meeting the hull
    print(f"hull_closest on the host, {2 * N} queries: worst gap {worst['gap']:.2e} / 1e-9, points {worst['pts']:.2e} / 1e-9, "
          f"u {worst['u']:.2e} / 1e-6, iterations {worst['iters']} of 32")


def test_catalogue_gaps_agree_with_the_restatement():
    """The catalogue's closed forms are independent of both implementations; its GAPS (unique whatever the points do) are checked
    here against the restatement, so that a slip in a hand-written row is caught without any device answer being looked at."""
    for row in HS.link_catalogue():
        V, P = HS.HULLS[row["hull"]]
        _, _, _, g = H.hull_closest(V, P, row["a"][None], row["b"][None], [row["r"]])
        assert abs(g[0] - (row["sep"] - row["r"])) <= 1e-12, (row["name"], g[0], row["sep"] - row["r"])


@needs_hipcc
def test_degenerate_catalogue_on_the_cpu(link_hull_driver):
    """hull_closest on the exact hulls of tests/hull_scene.py against CLOSED FORMS at 1e-12 (DESIGN 4.7's figure for the host
    build): points on a vertex, an edge, a face and at the centre, feet on an edge and a corner, segments parallel to a face and
    an edge, collinear with an edge, lying on an edge and in a face plane, touching at an endpoint, piercing, inside, and the
    grazing pair.  Rows whose nearest pair is a set or whose face rule ties are named in the catalogue and held by membership.
    Measured: worst error 3.3e-16 (3.3e-4 of the bound) over the 33 rows, at most 3 iterations of 32."""
    rows = HS.link_catalogue()
    names = sorted({r["hull"] for r in rows})
    out = link_hull_driver([HS.HULLS[n] for n in names], [(names.index(r["hull"]), r["a"], r["b"], r["r"]) for r in rows])
    worst, iters = 0.0, 0
    for row, o in zip(rows, out):
        assert o[10] < 32, row["name"]
        iters = max(iters, int(o[10]))
        worst = max(worst, HS.check_link_row(row, o[0:3], o[3:6], o[6:9], o[9], 1e-12))
    by = {r["name"]: o for r, o in zip(rows, out)}
    # the grazing jump: the touching axis answers the face rule's -(0.5 + r), 2e-7 m further out GJK's 2e-7 - r
    assert abs(by["seg_graze"][9] + 0.5 + HS.R_OBS) <= 1e-12 and abs(by["seg_graze_near"][9] - (HS.GRAZE_EPS / HS.S2 - HS.R_OBS)) <= 1e-12
    assert {r["kind"] for r in rows} == {"unique", "set", "tie"}
    print(f"hull_closest degenerate catalogue, {len(rows)} rows: worst error / 1e-12 = {worst:.2e}, iterations {iters} of 32")


@needs_hipcc
def test_non_finite_axis_on_the_cpu(link_hull_driver):
    """include/rmp2.h: a non-finite value anywhere in an obstacle record makes its pairs NaN -- never a finite distance (a NaN in
    a capsule's second endpoint used to answer the sphere at the first), never +-inf beside finite points."""
    rows = HS.nonfinite_link_rows()
    out = link_hull_driver([HS.HULLS["cube"]], [(0, a, b, r) for _, a, b, r in rows])
    for (name, *_), o in zip(rows, out):
        assert np.isnan(o[:10]).all(), (name, o)
    # and the finite neighbour is untouched by the selects
    o = link_hull_driver([HS.HULLS["cube"]], [(0, (0.5, 0.5, 1.5), (1.5, 0.5, 1.5), HS.R_OBS)])[0]
    assert o[9] == 0.5 - HS.R_OBS and np.array_equal(o[6:9], [0, 0, -1])

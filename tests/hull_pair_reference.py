"""fp64 numpy restatement of the hull self-pair stage (include/rmp2.h rmp2_set_self_collision_hulls), by brute force:

  * distance: the minimum over three cases -- the vertices of A against the triangles of B, the vertices of B against the
    triangles of A, the edges of A against the edges of B (feature pairs that cannot beat the best vertex pair are skipped by a
    bounding-sphere test, which drops nothing that could win);
  * overlap (an edge of either hull meets the other, or the two lie within 1e-7 m): the face rule over A's face normals and
    B's negated face normals, s(n) = min_{y in B} n . y - max_{x in A} n . x, n* = argmax s (A's faces first), y* the vertex of
    B attaining the min; p_b = y*, p_a = y* - s n*, gap = s, u = -n*.

No GJK here: the device's method is checked against a different one.  Helpers for the tests of the feature only.
"""
import numpy as np

import hull_reference as H

TOUCH = 1e-7


class Hull:
    """One hull with what the brute force needs: vertices, planes (n, d), triangles and edges, all fp64."""

    def __init__(self, verts, planes):
        from scipy.spatial import ConvexHull
        self.V = np.asarray(verts, np.float64)
        self.P = np.asarray(planes, np.float64)
        tri = ConvexHull(self.V).simplices
        self.T = self.V[tri]                                            # [T, 3, 3]
        e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
        self.E = self.V[np.unique(e, axis=0)]                           # [E, 2, 3] unique edges
        self.tc = self.T.mean(1)
        self.tr = np.linalg.norm(self.T - self.tc[:, None], axis=2).max(1)
        self.em = self.E.mean(1)
        self.eh = 0.5 * np.linalg.norm(self.E[:, 1] - self.E[:, 0], axis=1)


def _pt_tri(p, A, B, C):
    """Nearest points of p on triangles A, B, C, row by row ([M, 3] each; Ericson 5.1.5, as hull_reference.point_triangle)."""
    ab, ac, ap = B - A, C - A, p - A
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - B
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - C
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        den = va + vb + vc
        v = np.where(den != 0, vb / den, 0.0)
        w = np.where(den != 0, vc / den, 0.0)
        out = A + v[:, None] * ab + w[:, None] * ac
        t_bc = np.where((d4 - d3) + (d5 - d6) != 0, (d4 - d3) / ((d4 - d3) + (d5 - d6)), 0.0)
        t_ac = np.where(d2 - d6 != 0, d2 / (d2 - d6), 0.0)
        t_ab = np.where(d1 - d3 != 0, d1 / (d1 - d3), 0.0)
    out = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[:, None], B + t_bc[:, None] * (C - B), out)
    out = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[:, None], A + t_ac[:, None] * ac, out)
    out = np.where(((d6 >= 0) & (d5 <= d6))[:, None], C, out)
    out = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[:, None], A + t_ab[:, None] * ab, out)
    out = np.where(((d3 >= 0) & (d4 <= d3))[:, None], B, out)
    return np.where(((d1 <= 0) & (d2 <= 0))[:, None], A, out)


def _vertex_triangle(P, T, tc, tr, bound):
    """Best (point of P, point on a triangle of T) with a candidate test against `bound`."""
    d = np.linalg.norm(P[:, None] - tc[None], axis=2) - tr[None]
    i, j = np.nonzero(d <= bound + 1e-12)
    if len(i) == 0:
        return np.inf, None, None
    q = _pt_tri(P[i], T[j, 0], T[j, 1], T[j, 2])
    dd = np.linalg.norm(P[i] - q, axis=1)
    k = int(np.argmin(dd))
    return dd[k], P[i[k]], q[k]


def pair_closest(A: Hull, B: Hull, Rm, t):
    """(pa, pb, u, gap, face) of hulls A and B, B placed in A's coordinates by y = Rm y_B + t, fp64."""
    Rm, t = np.asarray(Rm, np.float64), np.asarray(t, np.float64)
    VB = B.V @ Rm.T + t
    TB = B.T @ Rm.T + t
    EB = B.E @ Rm.T + t
    tcB, emB = B.tc @ Rm.T + t, B.em @ Rm.T + t
    # an upper bound: the best vertex pair
    dv = np.linalg.norm(A.V[:, None] - VB[None], axis=2)
    i, j = np.unravel_index(int(np.argmin(dv)), dv.shape)
    best, pa, pb = dv[i, j], A.V[i], VB[j]
    d1, a1, b1 = _vertex_triangle(A.V, TB, tcB, B.tr, best)
    if d1 < best:
        best, pa, pb = d1, a1, b1
    d2, b2, a2 = _vertex_triangle(VB, A.T, A.tc, A.tr, best)
    if d2 < best:
        best, pa, pb = d2, a2, b2
    lb = np.linalg.norm(A.em[:, None] - emB[None], axis=2) - A.eh[:, None] - B.eh[None]
    i, j = np.nonzero(lb <= best + 1e-12)
    if len(i):
        x, y = H.segment_segment(A.E[i, 0][:, None], A.E[i, 1][:, None], EB[j, 0][:, None], EB[j, 1][:, None])
        x, y = x[:, 0], y[:, 0]
        dd = np.linalg.norm(x - y, axis=1)
        k = int(np.argmin(dd))
        if dd[k] < best:
            best, pa, pb = dd[k], x[k], y[k]
    # apart when the pair's own direction separates the hulls (a certificate); else overlap iff an edge of either meets the other
    if best > TOUCH:
        u = (pa - pb) / best
        apart = (A.V @ u).min() - (VB @ u).max() >= best - 1e-9
        if not apart:
            PB = np.concatenate([B.P[:, :3] @ Rm.T, (B.P[:, 3] + (B.P[:, :3] @ Rm.T) @ t)[:, None]], axis=1)
            apart = not (H._meets(PB, A.E[:, 0], A.E[:, 1]).any() or H._meets(A.P, EB[:, 0], EB[:, 1]).any())
        if apart:
            return pa, pb, u, best, False
    nA, dA = A.P[:, :3], A.P[:, 3]
    sA = (VB @ nA.T).min(0) - dA                                        # min_y n . y - max_x n . x (= d for A's own faces)
    rm = B.P[:, :3] @ Rm.T                                              # R m per face of B (A's coordinates)
    sB = -B.P[:, 3] - rm @ t + (A.V @ rm.T).min(0)
    s = np.concatenate([sA, sB])
    k = int(np.argmax(s))
    n = nA[k] if k < len(sA) else -rm[k - len(sA)]
    y = VB[int(np.argmin(VB @ n))]
    return y - s[k] * n, y, -n, s[k], True


def face_margin(A: Hull, B: Hull, Rm, t):
    """Best minus second-best s over the face rule's normals (how well n*, and with it the overlap points, are determined)."""
    Rm, t = np.asarray(Rm, np.float64), np.asarray(t, np.float64)
    VB = B.V @ Rm.T + t
    sA = (VB @ A.P[:, :3].T).min(0) - A.P[:, 3]
    rm = B.P[:, :3] @ Rm.T
    sB = -B.P[:, 3] - rm @ t + (A.V @ rm.T).min(0)
    s = np.sort(np.concatenate([sA, sB]))
    return s[-1] - s[-2]


def self_hull_pairs_np(desc, hulls, pairs, q, T=None):
    """(p_link, p_obs, dist, gap, face) [R, S, 3], [R, S, 3], [R, S], [R, S], [R, S] in fp64 in rmp2_self_pairs' layout for
    self pairs [(leaf ordinal, frame B or -1)] on `hulls` (urdf.self_collision_hulls).  Distance leaves: the two points in the
    base frame; attached-point leaves: relative_position (frame), normal_vec = sign(gap) u (base), distance |gap|.  T: the
    frames [R, F, 4, 4] to place the hulls by (default: the oracle's fp64 frames; its fp32 frames give the fp32 walk's share)."""
    import oracle as O
    from riemannian_motion_policies_amd import descriptor as D
    if T is None:
        T = O.forward_kinematics(desc, np.asarray(q, np.float32), "f64")
    T = np.asarray(T, np.float64)
    dl = D.distance_leaf_indices(desc)
    F = desc.robot.n_frames
    cache = {}

    def hull(e):
        if e not in cache:
            cache[e] = Hull(*hulls.hull(e))
        return cache[e]

    R, S = len(q), len(pairs)
    pl, po = np.empty((R, S, 3)), np.empty((R, S, 3))
    gap, face = np.empty((R, S)), np.zeros((R, S), bool)
    for j, (o, b) in enumerate(pairs):
        leaf = desc.leaves[dl[o]]
        fa = leaf.frame
        HA, HB = hull(fa), hull(F if b < 0 else b)
        for r in range(R):
            TA = T[r, fa]
            TB = np.eye(4) if b < 0 else T[r, b]
            RA, pA = TA[:3, :3], TA[:3, 3]
            Rm, t = RA.T @ TB[:3, :3], RA.T @ (TB[:3, 3] - pA)
            pa, pb, u, g, fc = pair_closest(HA, HB, Rm, t)
            gap[r, j], face[r, j] = g, fc
            if leaf.taskmap == D.TASKMAP_FK_POINT:
                pl[r, j] = pa
                po[r, j] = np.sign(g if g != 0 else 1.0) * (RA @ u)
            else:
                pl[r, j] = RA @ pa + pA
                po[r, j] = RA @ pb + pA
    return pl, po, np.abs(gap), gap, face

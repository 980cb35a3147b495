"""fp64 restatement, and fp32 envelope, of the contact step with half-space obstacles beside the spheres (include/rmp2.h
rmp2_dynamics_step_contacts_planes), built on tests/contacts_reference.py: its sphere rows followed by the plane rows, its
candidate rule, its QP, its landing and its brackets.

Plane rows, per frame f with a non-zero capsule row (world end points X_0 = A, X_1 = A + D, radius r_f), plane p = (n, d) and end e:
    g = n . X_e - d - r_f,   J[j] = n . (z_j x (X_e - o_j)) (revolute ancestor dof j), n . z_j (prismatic),   b = -max(g, 0) / dt;
a capsule with D == 0 exactly gives the row e = 0 only;  pair index F K + 2 (f P + p) + e (F frames, K spheres), after every
sphere pair f K + k.  The normal is used as given."""
from __future__ import annotations

import numpy as np

import contacts_reference as CR
import forward_dynamics_reference as FR
from riemannian_motion_policies_amd import urdf as U

SPHERE, PLANE = 0, 1
_sphere_rows = CR.pair_rows          # (the original, whatever _rows_with has put in its place)


def pair_index(F, K, P, f, p, e):
    return F * K + 2 * (f * P + p) + e


def split_pair(pair, F, K, P):
    """(kind, frame, record, end) of a pair index; None for -1."""
    pair = int(pair)
    if pair < 0:
        return None
    if pair < F * K:
        return SPHERE, pair // K, pair % K, 0
    r = pair - F * K
    assert r < 2 * F * P, (pair, F, K, P)
    return PLANE, (r >> 1) // P, (r >> 1) % P, r & 1


def plane_rows(table, caps, planes, K, q, dtype=np.float64):
    """The plane rows of a fleet, contacts_reference.pair_rows' dict (idx, gap, J, X, n) in `dtype`.  The row e = 1 of a robot
    whose capsule has D == 0 has gap +inf: it is never a candidate."""
    dtype = np.dtype(dtype)
    q = np.atleast_2d(np.asarray(q, dtype))
    B, n = q.shape
    caps = np.asarray(caps, dtype)
    pl = np.asarray(planes, dtype).reshape(-1, 4)
    P, F = len(pl), table.n_frames
    R, p, z = CR.poses(table, q, dtype)
    idx, gaps, rows, Xs, ns = [], [], [], [], []
    for f in CR.capsule_frames(caps):
        A = FR._mv(R[f], np.broadcast_to(caps[f, 0:3], (B, 3))) + p[f]
        D = FR._mv(R[f], np.broadcast_to(caps[f, 4:7] - caps[f, 0:3], (B, 3)))
        point = (D == 0).all(-1)
        anc, g = [], f
        while g >= 0:
            jt, j = int(table.joint_type[g]), int(table.q_index[g])
            if jt != U.JOINT_FIXED and j >= 0:
                anc.append((j, g, jt))
            g = int(table.parent[g])
        for k in range(P):
            nu = np.broadcast_to(pl[k, :3], (B, 3))
            for e in (0, 1):
                X = (A + D if e else A).astype(dtype)
                with np.errstate(invalid="ignore"):
                    gap = ((nu * X).sum(-1, dtype=dtype) - pl[k, 3] - caps[f, 3]).astype(dtype)
                if e:
                    gap = np.where(point, dtype.type(np.inf), gap)
                J = np.zeros((B, n), dtype)
                for (j, gfr, jt) in anc:
                    J[:, j] = (nu * FR._cross(z[gfr], X - p[gfr])).sum(-1) if jt == U.JOINT_REVOLUTE else (nu * z[gfr]).sum(-1)
                idx.append(pair_index(F, K, P, f, k, e))
                gaps.append(gap)
                rows.append(J)
                Xs.append(X)
                ns.append(np.array(nu, dtype))
    if not idx:
        return dict(idx=np.zeros(0, int), gap=np.zeros((B, 0), dtype), J=np.zeros((B, 0, n), dtype), X=np.zeros((B, 0, 3), dtype),
                    n=np.zeros((B, 0, 3), dtype))
    return dict(idx=np.array(idx), gap=np.stack(gaps, 1), J=np.stack(rows, 1), X=np.stack(Xs, 1), n=np.stack(ns, 1))


def pair_rows(table, caps, spheres, planes, q, dtype=np.float64):
    """contacts_reference.pair_rows' sphere rows followed by the plane rows."""
    sph = np.asarray(spheres, np.float64).reshape(-1, 4)
    a = _sphere_rows(table, caps, sph, q, dtype)
    b = plane_rows(table, caps, planes, len(sph), q, dtype)
    return {k: np.concatenate([a[k], b[k]], 0 if k == "idx" else 1) for k in a}


class _rows_with:
    """Within the block contacts_reference forms its rows with `planes` as well: its substep -- candidates, solve_qp, landing --
    runs on the concatenated rows, unchanged."""

    def __init__(self, planes):
        self.planes = planes

    def __enter__(self):
        self.saved = CR.pair_rows
        CR.pair_rows = lambda table, caps, spheres, q, dtype=np.float64: pair_rows(table, caps, spheres, self.planes, q, dtype)

    def __exit__(self, *exc):
        CR.pair_rows = self.saved


def substep(table, inert, caps, spheres, planes, d_act, q, qd, u, drive, dt, lim, limits, gravity=(0.0, 0.0, -9.81), envelope=False):
    """contacts_reference.substep with planes: the same dict."""
    with _rows_with(planes):
        return CR.substep(table, inert, caps, spheres, d_act, q, qd, u, drive, dt, lim, limits, gravity, envelope)


def dynamics_step(table, inert, caps, spheres, planes, d_act, q, qd, u, drive, dt, substeps, lim, limits, gravity=(0.0, 0.0, -9.81),
                  envelope=False):
    """contacts_reference.dynamics_step with planes: the same dict."""
    with _rows_with(planes):
        return CR.dynamics_step(table, inert, caps, spheres, d_act, q, qd, u, drive, dt, substeps, lim, limits, gravity, envelope)


def linearised_gaps(c, got_qd, pair, dt):
    """test_contacts_host.linearised_gaps over sphere and plane pairs: max(g, 0) + dt J v per slot [B, 8] in fp64 at the case's
    state (nan in empty slots), and the rows' 1-norms."""
    pr = pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["q"])
    pos = {int(i): k for k, i in enumerate(pr["idx"])}
    out, jn = np.full(pair.shape, np.nan), np.zeros(pair.shape)
    for r in range(len(pair)):
        for s in range(pair.shape[1]):
            if pair[r, s] >= 0:
                k = pos[int(pair[r, s])]
                out[r, s] = max(pr["gap"][r, k], 0.0) + dt * (pr["J"][r, k] @ np.asarray(got_qd[r], np.float64))
                jn[r, s] = np.abs(pr["J"][r, k]).sum()
    return out, jn


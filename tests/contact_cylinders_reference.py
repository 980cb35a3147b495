"""fp64 restatement, and fp32 envelope, of the contact step with exact flat-capped cylinder obstacles (include/rmp2.h
rmp2_dynamics_step_contacts_cylinders), built on tests/contact_self_reference.py the way that one is built on
tests/contact_capsules_reference.py: its sphere, plane, capsule and self rows followed by the cylinder rows, its candidate rule,
its QP, its landing and its brackets.

Cylinder rows, per frame f with a non-zero link capsule row (world segment A, A + D, radius r_f) and record y = (centre c, radius r,
unit axis u, half height h):
    point_cylinder(p), case by case: a = (p - c) . u, rho = |(p - c) - a u|, e the unit radial direction (on the axis: the cross
    product of u with the coordinate axis it is least aligned with, normalised); da = |a| - h, dr = rho - r.
      inside (da <= 0 and dr <= 0), side nearer (dr >= da):   Y = c + a u + r e,        n = e,          sd = dr;
      inside, cap nearer:                                      Y = c + sgn(a) h u + rho e, n = sgn(a) u,  sd = da;
      outside: ac = clamp(a, -h, h), rc = min(rho, r), ga = a - ac, gr = rho - rc:
                                                                Y = c + ac u + rc e,  sd = sqrt(ga^2 + gr^2),  n = (ga u + gr e) / sd.
    segment_cylinder: with slope(s) = n(A + s D) . D -- s = 0 where not slope(0) < 0; else s = 1 where not slope(1) > 0; else the
    midpoint after HALVINGS bisections of [0, 1] on the sign of the slope (60 in fp64, as configs.pairs_from_link_capsules_cylinders;
    24 in the fp32 envelope, as rmp2_device.h).  X = A + s D, n and sd from point_cylinder(X).
    g = sd - r_f;  J[j] = n . (z_j x (X - o_j)) (n . z_j prismatic) over the ancestors' dofs;  b = -max(g, 0) / dt;
pair index F K + 2 F P + F C + F F + f Y + y: after every sphere, plane, capsule and self pair, the self block of F F values being
reserved whether or not self pairs are on."""
from __future__ import annotations

import numpy as np

import contact_self_reference as SR
import contacts_reference as CR
import forward_dynamics_reference as FR
from riemannian_motion_policies_amd import urdf as U

SPHERE, PLANE, CAPSULE, SELF, CYLINDER = 0, 1, 2, 3, 4
NONE2 = np.zeros((0, 2), np.int32)
HALVINGS = {np.dtype(np.float64): 60, np.dtype(np.float32): 24}


def cylinder_base(F, K, P, C):
    return SR.self_base(F, K, P, C) + F * F


def pair_index(F, K, P, C, Y, f, y):
    return cylinder_base(F, K, P, C) + f * Y + y


def split_pair(pair, F, K, P, C, Y):
    """(kind, frame, record, end) of a pair index of the cylinders call ((CYLINDER, frame, cylinder, 0) for a cylinder pair); None
    for -1."""
    pair = int(pair)
    if pair < 0:
        return None
    base = cylinder_base(F, K, P, C)
    if pair < base:
        return SR.split_pair(pair, F, K, P, C)
    assert pair < base + F * Y, (pair, F, K, P, C, Y)
    return CYLINDER, (pair - base) // Y, (pair - base) % Y, 0


def _perpendicular(u, dtype):
    """point_cylinder's fixed perpendicular of the axes u [..., 3]."""
    ax = np.abs(u)
    kx = (ax[..., 0] <= ax[..., 1]) & (ax[..., 0] <= ax[..., 2])
    ky = ~kx & (ax[..., 1] <= ax[..., 2])
    t = np.stack([kx, ky, ~kx & ~ky], -1).astype(dtype)
    c = np.cross(u, t).astype(dtype)
    with np.errstate(all="ignore"):
        return (c / np.sqrt((c * c).sum(-1, dtype=dtype))[..., None]).astype(dtype)


def point_cylinder(p, rec, dtype=np.float64):
    """rmp2_device.h point_cylinder on points p [B, 3] against one record rec [8], or one record each rec [B, 8], in `dtype`:
    (Y [B, 3], n [B, 3], sd [B])."""
    dtype = np.dtype(dtype)
    p = np.asarray(p, dtype)
    rec = np.broadcast_to(np.asarray(rec, dtype), (len(p), 8))
    c, r, u, h = rec[:, 0:3], rec[:, 3], rec[:, 4:7], rec[:, 7]
    zero, one = dtype.type(0), dtype.type(1)
    with np.errstate(all="ignore"):
        w = (p - c).astype(dtype)
        a = (w * u).sum(-1, dtype=dtype)
        rv = (w - a[:, None] * u).astype(dtype)
        rho = np.sqrt((rv * rv).sum(-1, dtype=dtype)).astype(dtype)
        e = np.where((rho > 0)[:, None], rv / np.where(rho > 0, rho, one)[:, None], _perpendicular(u, dtype)).astype(dtype)
        sa = np.where(a < 0, -one, one).astype(dtype)
        da, dr = (np.abs(a) - h).astype(dtype), (rho - r).astype(dtype)
        inside = (da <= 0) & (dr <= 0)
        side = inside & (dr >= da)
        cap = inside & ~side
        ac_out, rc_out = np.clip(a, -h, h).astype(dtype), np.minimum(rho, r).astype(dtype)
        ga, gr = (a - ac_out).astype(dtype), (rho - rc_out).astype(dtype)
        sd_out = np.sqrt(ga * ga + gr * gr).astype(dtype)
        n_out = ((ga[:, None] * u + gr[:, None] * e) / sd_out[:, None]).astype(dtype)
        ac = np.where(side, a, np.where(cap, sa * h, ac_out)).astype(dtype)
        rc = np.where(side, r, np.where(cap, rho, rc_out)).astype(dtype)
        sd = np.where(side, dr, np.where(cap, da, sd_out)).astype(dtype)
        n = np.where(side[:, None], e, np.where(cap[:, None], sa[:, None] * u, n_out)).astype(dtype)
        Y = (c + ac[:, None] * u + rc[:, None] * e).astype(dtype)
    return Y, n, sd


def segment_cylinder(A, D, rec, dtype=np.float64, halvings=None):
    """rmp2_device.h segment_cylinder on segments A, D [B, 3]: dict(s [B], X, Y, n [B, 3], sd [B]) in `dtype`."""
    dtype = np.dtype(dtype)
    A, D = np.asarray(A, dtype), np.asarray(D, dtype)
    halvings = HALVINGS[dtype] if halvings is None else halvings
    zero, one, half = dtype.type(0), dtype.type(1), dtype.type(0.5)

    def slope(s):
        X = (A + s[:, None] * D).astype(dtype)
        with np.errstate(all="ignore"):
            return (point_cylinder(X, rec, dtype)[1] * D).sum(-1, dtype=dtype)

    B = len(A)
    with np.errstate(invalid="ignore"):
        at_a = ~(slope(np.full(B, zero, dtype)) < 0)
        at_b = ~at_a & ~(slope(np.full(B, one, dtype)) > 0)
    lo, hi = np.full(B, zero, dtype), np.full(B, one, dtype)
    for _ in range(halvings):
        mid = (half * (lo + hi)).astype(dtype)
        with np.errstate(invalid="ignore"):
            neg = slope(mid) < 0
        lo, hi = np.where(neg, mid, lo).astype(dtype), np.where(neg, hi, mid).astype(dtype)
    s = np.where(at_a, zero, np.where(at_b, one, half * (lo + hi))).astype(dtype)
    X = (A + s[:, None] * D).astype(dtype)
    Y, n, sd = point_cylinder(X, rec, dtype)
    return dict(s=s, X=X, Y=Y, n=n, sd=sd)


def scan_minimum(A, D, rec, points=2001, levels=4):
    """The smallest signed distance over the segment A + s D by brute force, fp64: a scan of `points` values of s, then of the two
    cells around the best one again, `levels` times (the distance is convex in s).  (sd, s) of one segment A, D [3]."""
    lo, hi = 0.0, 1.0
    for _ in range(levels):
        s = np.linspace(lo, hi, points)
        sd = point_cylinder(A[None] + s[:, None] * D[None], rec)[2]
        k = int(np.argmin(sd))
        lo, hi = s[max(k - 1, 0)], s[min(k + 1, points - 1)]
    return float(sd[k]), float(s[k])


def cylinder_rows(table, caps, cylinders, K, P, C, q, dtype=np.float64, detail=False):
    """The cylinder rows of a fleet, contacts_reference.pair_rows' dict (idx, gap, J, X, n) in `dtype`, frame by frame in
    contacts_reference.capsule_frames' order; detail: also s [B, rows] and Y [B, rows, 3]."""
    dtype = np.dtype(dtype)
    q = np.atleast_2d(np.asarray(q, dtype))
    B, n = q.shape
    caps = np.asarray(caps, dtype)
    cy = np.asarray(cylinders, dtype).reshape(-1, 8)
    Yn, F = len(cy), table.n_frames
    R, p, z = CR.poses(table, q, dtype)
    idx, gaps, rows, Xs, ns, ss, Ys = [], [], [], [], [], [], []
    frames = CR.capsule_frames(caps) if Yn else []
    As, Ds = [], []
    for f in frames:
        As.append((FR._mv(R[f], np.broadcast_to(caps[f, 0:3], (B, 3))) + p[f]).astype(dtype))
        Ds.append(FR._mv(R[f], np.broadcast_to(caps[f, 4:7] - caps[f, 0:3], (B, 3))).astype(dtype))
    if frames:      # one bisection for every (frame, cylinder, robot): the rows' arithmetic is element-wise
        n_f = len(frames)
        A_all = np.broadcast_to(np.stack(As)[:, None], (n_f, Yn, B, 3)).reshape(-1, 3)
        D_all = np.broadcast_to(np.stack(Ds)[:, None], (n_f, Yn, B, 3)).reshape(-1, 3)
        rec_all = np.broadcast_to(cy[None, :, None, :], (n_f, Yn, B, 8)).reshape(-1, 8)
        d_all = {k: v.reshape((n_f, Yn, B) + v.shape[1:]) for k, v in segment_cylinder(A_all, D_all, rec_all, dtype).items()}
    for i, f in enumerate(frames):
        anc = SR.ancestors(table, f)
        for y in range(Yn):
            d = {k: v[i, y] for k, v in d_all.items()}
            X, nu = d["X"], d["n"]
            J = np.zeros((B, n), dtype)
            for (j, gfr, jt) in anc:
                J[:, j] = (nu * FR._cross(z[gfr], X - p[gfr])).sum(-1) if jt == U.JOINT_REVOLUTE else (nu * z[gfr]).sum(-1)
            idx.append(pair_index(F, K, P, C, Yn, f, y))
            gaps.append((d["sd"] - caps[f, 3]).astype(dtype))
            rows.append(J)
            Xs.append(X), ns.append(nu), ss.append(d["s"]), Ys.append(d["Y"])
    if not idx:
        out = dict(idx=np.zeros(0, int), gap=np.zeros((B, 0), dtype), J=np.zeros((B, 0, n), dtype), X=np.zeros((B, 0, 3), dtype),
                   n=np.zeros((B, 0, 3), dtype))
        return dict(out, s=np.zeros((B, 0), dtype), Y=np.zeros((B, 0, 3), dtype)) if detail else out
    out = dict(idx=np.array(idx), gap=np.stack(gaps, 1), J=np.stack(rows, 1), X=np.stack(Xs, 1), n=np.stack(ns, 1))
    return dict(out, s=np.stack(ss, 1), Y=np.stack(Ys, 1)) if detail else out


def pair_rows(table, caps, spheres, planes, capsules, pairs, cylinders, q, dtype=np.float64):
    """contact_self_reference.pair_rows' sphere, plane, capsule and self rows followed by the cylinder rows."""
    sph = np.asarray(spheres, np.float64).reshape(-1, 4)
    pl = np.asarray(planes, np.float64).reshape(-1, 4)
    oc = np.asarray(capsules, np.float64).reshape(-1, 8)
    a = SR.pair_rows(table, caps, sph, pl, oc, pairs, q, dtype)
    b = cylinder_rows(table, caps, cylinders, len(sph), len(pl), len(oc), q, dtype)
    return {k: np.concatenate([a[k], b[k]], 0 if k == "idx" else 1) for k in a}


class _rows_with:
    """Within the block contacts_reference forms its rows with planes, capsules, self pairs and cylinders as well: its substep --
    candidates, solve_qp, landing -- runs on the concatenated rows, unchanged."""

    def __init__(self, planes, capsules, pairs, cylinders):
        self.args = planes, capsules, pairs, cylinders

    def __enter__(self):
        self.saved = CR.pair_rows
        pl, oc, pairs, cy = self.args
        CR.pair_rows = lambda table, caps, spheres, q, dtype=np.float64: pair_rows(table, caps, spheres, pl, oc, pairs, cy, q, dtype)

    def __exit__(self, *exc):
        CR.pair_rows = self.saved


def dynamics_step(table, inert, caps, spheres, planes, capsules, pairs, cylinders, d_act, q, qd, u, drive, dt, substeps, lim, limits,
                  gravity=(0.0, 0.0, -9.81), envelope=False, flag=True):
    """contacts_reference.dynamics_step with planes, capsules, self pairs (flag) and cylinders: the same dict."""
    with _rows_with(planes, capsules, pairs if flag else NONE2, cylinders):
        return CR.dynamics_step(table, inert, caps, spheres, d_act, q, qd, u, drive, dt, substeps, lim, limits, gravity, envelope)


def linearised_gaps(c, got_qd, pair, dt):
    """contact_self_reference.linearised_gaps over the five kinds of pairs."""
    pr = pair_rows(c["t"], c["caps"], c["spheres"], c["planes"], c["capsules"], c["pairs"], c["cylinders"], c["q"])
    pos = {int(i): k for k, i in enumerate(pr["idx"])}
    out, jn = np.full(pair.shape, np.nan), np.zeros(pair.shape)
    for r in range(len(pair)):
        for s in range(pair.shape[1]):
            if pair[r, s] >= 0:
                k = pos[int(pair[r, s])]
                out[r, s] = max(pr["gap"][r, k], 0.0) + dt * (pr["J"][r, k] @ np.asarray(got_qd[r], np.float64))
                jn[r, s] = np.abs(pr["J"][r, k]).sum()
    return out, jn


def write_driver_input(path, c, substeps, dt, d_act, lists=None, flag=1, **over):
    """Input file of tests/contacts_driver.cpp's cylinder form: contact_self_reference.write_driver_input's, followed by int32 Y, float
    cylinders[Y][8], int32 self_pairs (the call's flag).  over: fields of the group replaced."""
    g = dict(c, **{k: v for k, v in over.items() if v is not None})
    SR.write_driver_input(path, g, substeps, dt, d_act, lists=lists)
    cy = np.ascontiguousarray(g["cylinders"], np.float32).reshape(-1, 8)
    with open(path, "ab") as f:
        np.array([len(cy)], np.int32).tofile(f)
        cy.tofile(f)
        np.array([int(flag)], np.int32).tofile(f)

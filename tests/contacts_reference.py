"""fp64 restatement of the plant's step with obstacle contacts (include/rmp2.h rmp2_dynamics_step_contacts) for the tests, built on
tests/forward_dynamics_reference.py and tests/joint_stops_reference.py, a brute-force check of it, and an fp32 ENVELOPE: the same
quantities restated in float32 numpy in this file's own arithmetic (an fp32 pose chain, forward_dynamics_reference's fp32 mass
matrix and Cholesky, the active-set loop below run on float32 arrays) -- not the device routine.  The envelope's error against
the fp64 reference is the measure the GPU bounds are taken from (K = 4 x its worst ratio, tests/test_contacts_host.py).

Semantics, per substep at (q, qd):  a, tau_applied, v* = qd + dt a and the box (l, h) as joint_stops_reference;  for each frame f
with a non-zero capsule row and each sphere k:  X = the point of the capsule's world segment nearest c_k,  n = (X - c_k) / |X - c_k|
(+z where X = c_k),  g = |X - c_k| - r_k - r_f,  J[j] = n . (z_j x (X - o_j)) (revolute ancestor dof j), n . z_j (prismatic),
b = -max(g, 0) / dt;  candidates: g <= d_act, the MAX_CONTACTS smallest (gap, pair index f K + k);
    v = argmin 1/2 (v - v*)^T M (v - v*)  s.t.  l <= v <= h,  J_c v >= b_c;    M (v - v*) = sigma + sum_c lambda_c J_c^T
    qd <- v;  q <- q + dt v (the stops' landing);  qdd_out = a + (v - v*) / dt,  stop = sigma / dt,  contact = J^T lambda / dt.
"""
from __future__ import annotations

import itertools

import numpy as np

import dynamics_reference as DR
import forward_dynamics_reference as FR
import joint_stops_reference as JR
from riemannian_motion_policies_amd import urdf as U

MAX_CONTACTS = 8
STOP_ACTIVE, CAPPED, CONTACT_ACTIVE, OVERFLOW = 1, 2, 4, 8
REFERENCE_CAP = 1000
PIVOT = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 2.4e-7}    # relative Gram pivot below which a row is refused
TOL = {np.dtype(np.float64): 1e-13, np.dtype(np.float32): 1e-5}        # relative size below which a row neither blocks nor moves


# ---- kinematics: poses, rows and gaps ----------------------------------------------------------------------------------------

def poses(table, q, dtype=np.float64):
    """(R [F][B, 3, 3], p [F][B, 3], z [F][B, 3]) of every frame in `dtype`: fp64 on dynamics_reference.model (orthonormal
    T_const), fp32 on the table as it is, every operation a float32 numpy operation."""
    dtype = np.dtype(dtype)
    q = np.atleast_2d(np.asarray(q, dtype))
    B = q.shape[0]
    F = table.n_frames
    if dtype == np.float64:
        Rc, tc, ax = DR.model(table)
    else:
        Rc, tc, ax = table.T_const[:, :3, :3].astype(dtype), table.T_const[:, :3, 3].astype(dtype), table.axis.astype(dtype)
    qf = DR._joint_values(table, q).astype(dtype)
    eye = np.eye(3, dtype=dtype)
    one = dtype.type(1)
    R, p, z = [None] * F, [None] * F, [None] * F
    for f in range(F):
        jt, pr, u = int(table.joint_type[f]), int(table.parent[f]), ax[f]
        Rl = np.broadcast_to(Rc[f], (B, 3, 3))
        tl = np.broadcast_to(tc[f], (B, 3))
        if jt == U.JOINT_REVOLUTE:
            c, s = np.cos(qf[:, f])[:, None, None], np.sin(qf[:, f])[:, None, None]
            K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]], dtype)
            Rl = FR._mm(Rl, c * eye + s * K + (one - c) * np.outer(u, u).astype(dtype))
        elif jt == U.JOINT_PRISMATIC:
            tl = tl + FR._mv(Rl, qf[:, f:f + 1] * u)
        Rp = R[pr] if pr >= 0 else np.broadcast_to(eye, (B, 3, 3))
        pp = p[pr] if pr >= 0 else np.zeros((B, 3), dtype)
        R[f] = FR._mm(Rp, Rl)
        p[f] = pp + FR._mv(Rp, tl)
        z[f] = FR._mv(R[f], np.broadcast_to(u, (B, 3)))
    assert all(x.dtype == dtype for x in R + p + z)
    return R, p, z


def capsule_frames(caps):
    return [f for f in range(len(caps)) if np.any(np.asarray(caps[f]) != 0)]


def pair_rows(table, caps, spheres, q, dtype=np.float64):
    """Every (capsule frame, sphere) pair of a fleet: dict(idx [P] = f K + k, gap [B, P], J [B, P, n], X [B, P, 3], n [B, P, 3])
    in `dtype`."""
    dtype = np.dtype(dtype)
    q = np.atleast_2d(np.asarray(q, dtype))
    B, n = q.shape
    caps = np.asarray(caps, dtype)
    sph = np.asarray(spheres, dtype).reshape(-1, 4)
    K = len(sph)
    R, p, z = poses(table, q, dtype)
    idx, gaps, rows, Xs, ns = [], [], [], [], []
    zero, one = dtype.type(0), dtype.type(1)
    for f in capsule_frames(caps):
        A = FR._mv(R[f], np.broadcast_to(caps[f, 0:3], (B, 3))) + p[f]
        D = FR._mv(R[f], np.broadcast_to(caps[f, 4:7] - caps[f, 0:3], (B, 3)))
        dd = (D * D).sum(-1)
        inv = np.where(dd > 0, one / np.where(dd > 0, dd, one), zero).astype(dtype)
        anc, g = [], f
        while g >= 0:
            jt, j = int(table.joint_type[g]), int(table.q_index[g])
            if jt != U.JOINT_FIXED and j >= 0:
                anc.append((j, g, jt))
            g = int(table.parent[g])
        for k in range(K):
            c, rk = sph[k, :3], sph[k, 3]
            with np.errstate(invalid="ignore"):
                t = np.clip(((c - A) * D).sum(-1) * inv, zero, one)
                X = A + t[:, None] * D
                nv = X - c
                dn = np.sqrt((nv * nv).sum(-1))
                cross = dn == 0
                nv = np.where(cross[:, None], np.array([0, 0, 1], dtype), nv)
                nu = nv / np.where(cross, one, dn)[:, None]
                gap = dn - rk - caps[f, 3]
            J = np.zeros((B, n), dtype)
            for (j, gfr, jt) in anc:
                J[:, j] = (nu * FR._cross(z[gfr], X - p[gfr])).sum(-1) if jt == U.JOINT_REVOLUTE else (nu * z[gfr]).sum(-1)
            idx.append(f * K + k)
            gaps.append(gap.astype(dtype))
            rows.append(J)
            Xs.append(X)
            ns.append(nu.astype(dtype))
    if not idx:
        return dict(idx=np.zeros(0, int), gap=np.zeros((B, 0), dtype), J=np.zeros((B, 0, n), dtype), X=np.zeros((B, 0, 3), dtype),
                    n=np.zeros((B, 0, 3), dtype))
    return dict(idx=np.array(idx), gap=np.stack(gaps, 1), J=np.stack(rows, 1), X=np.stack(Xs, 1), n=np.stack(ns, 1))


def candidates(idx, gap, d_act):
    """Of one robot: (positions into idx of the kept pairs, in (gap, idx) order; the number that qualified beyond them)."""
    with np.errstate(invalid="ignore"):
        ok = np.nonzero(gap <= d_act)[0]
    order = sorted(ok, key=lambda i: (gap[i], idx[i]))
    return np.array(order[:MAX_CONTACTS], int), max(len(order) - MAX_CONTACTS, 0)


# ---- the QP ------------------------------------------------------------------------------------------------------------------

def _minv(M, a):
    if M.dtype == np.float64:
        return np.linalg.solve(M, a)
    return FR._cholesky_solve32(M[None], a[None])[0]


def _gram_factor(G, pivot):
    """Row-by-row Cholesky of G in its dtype: (L, refused)."""
    dtype = G.dtype
    m = len(G)
    L = np.zeros((m, m), dtype)
    refused = False
    with np.errstate(all="ignore"):
        for i in range(m):
            for k in range(i + 1):
                s = G[i, k]
                for p in range(k):
                    s = dtype.type(s - L[i, p] * L[k, p])
                if k < i:
                    L[i, k] = s / L[k, k]
                else:
                    if not (s > dtype.type(pivot) * G[i, i]) or not np.isfinite(s):
                        refused = True
                    L[i, i] = np.sqrt(s)
    return L, refused


def _gram_solve(L, r):
    dtype = L.dtype
    m = len(r)
    y = np.zeros(m, dtype)
    for i in range(m):
        y[i] = dtype.type(r[i] - (L[i, :i] * y[:i]).sum(dtype=dtype)) / L[i, i]
    for i in reversed(range(m)):
        y[i] = dtype.type(y[i] - (L[i + 1:, i] * y[i + 1:]).sum(dtype=dtype)) / L[i, i]
    return y


def solve_qp(M, vstar, l, h, J, b, cap=REFERENCE_CAP):
    """The primal active-set method over the rows +e_j v >= l_j (ids 0 .. n-1), -e_j v >= -h_j (n .. 2n-1), J_c v >= b_c (2n + c)
    from v = 0, in the dtype of the arrays (float64: the reference; float32: the envelope).  Returns dict(v, sigma [n], lam [nc],
    W (row ids), iters, capped)."""
    dtype = vstar.dtype
    n, nc = len(vstar), len(b)
    pivot, tol = PIVOT[dtype], dtype.type(TOL[dtype])
    zero, one = dtype.type(0), dtype.type(1)
    A = np.concatenate([np.eye(n, dtype=dtype), -np.eye(n, dtype=dtype), np.asarray(J, dtype).reshape(nc, n)])
    beta = np.concatenate([l, -h, np.asarray(b, dtype)]).astype(dtype)
    v = np.zeros(n, dtype)
    vmax = np.abs(vstar).max()          # the velocity scale of the problem
    W, Y, mu = [], [], np.zeros(0, dtype)
    it, capped = 0, False
    while True:
        if it >= cap:
            capped = True
            break
        it += 1
        m = len(W)
        if m:
            Ym = np.stack(Y, 1)
            G = (A[W][:, None, :] * Ym.T[None, :, :]).sum(-1, dtype=dtype)
            L, refused = _gram_factor(G, pivot)
            if refused:
                W.pop(), Y.pop()
                mu = mu[:len(W)]
                capped = True
                break
            r = (beta[W] - (A[W] * vstar[None, :]).sum(-1, dtype=dtype)).astype(dtype)
            mu = _gram_solve(L, r)
            x = (vstar + (Ym * mu[None, :]).sum(-1, dtype=dtype)).astype(dtype)
        else:
            mu = np.zeros(0, dtype)
            x = vstar.copy()
        for r_ in W:
            if r_ < n:
                x[r_] = l[r_]
            elif r_ < 2 * n:
                x[r_ - n] = h[r_ - n]
        if len(W) == n:          # (W spans the dofs: the equality problem's solution is v itself; x differs by rounding only)
            x = v.copy()
        alpha, brow, bval, viol = dtype.type(2), -1, zero, zero      # (ties go to the row x violates most, relative to |a_i|_1)
        inbox = np.zeros(n, bool)
        for r_ in W:
            if r_ < 2 * n:
                inbox[r_ % n] = True
        pvec = x - v
        with np.errstate(all="ignore"):
            for j in range(n):
                below, above = x[j] < l[j] - tol * vmax, x[j] > h[j] + tol * vmax
                if not inbox[j] and (below or above):
                    bb = l[j] if below else h[j]
                    a_ = max((bb - v[j]) / (x[j] - v[j]), zero)
                    w_ = abs(x[j] - bb)
                    if a_ < alpha or (a_ == alpha and w_ > viol):
                        alpha, brow, bval, viol = a_, (j if below else n + j), bb, w_
            for c in range(nc):
                if 2 * n + c in W:
                    continue
                row = A[2 * n + c]
                jx, jv, jp = (row * x).sum(dtype=dtype), (row * v).sum(dtype=dtype), (row * pvec).sum(dtype=dtype)
                scale = np.abs(row).sum(dtype=dtype) * vmax
                if jx < beta[2 * n + c] - tol * (scale + abs(beta[2 * n + c])) and jp < -tol * scale:
                    a_ = max((jv - beta[2 * n + c]) / -jp, zero)
                    w_ = (beta[2 * n + c] - jx) / np.abs(row).sum(dtype=dtype)
                    if a_ < alpha or (a_ == alpha and w_ > viol):
                        alpha, brow, viol = a_, 2 * n + c, w_
        if brow >= 0:
            alpha = min(max(alpha, zero), one)
            vn = np.clip(v + alpha * pvec, l, h)
            vn = np.where(inbox, v, vn)
            if brow < 2 * n:
                vn[brow % n] = bval
            v = vn.astype(dtype)
            if len(W) >= n:
                capped = True
                break
            W.append(brow)
            Y.append(_minv(M, A[brow]).astype(dtype))
            mu = np.concatenate([mu, np.zeros(1, dtype)])
            continue
        v = np.clip(x, l, h).astype(dtype)          # (a rounding, below the tolerance, must not leave the box)
        worst, drop = zero, -1
        for i, r_ in enumerate(W):
            locked = r_ < 2 * n and l[r_ % n] == h[r_ % n]
            if not locked and mu[i] < worst:
                worst, drop = mu[i], i
        if drop < 0:
            break
        W.pop(drop), Y.pop(drop)
        mu = np.delete(mu, drop)
    sigma, lam = np.zeros(n, dtype), np.zeros(nc, dtype)
    for i, r_ in enumerate(W):
        if r_ < n:
            sigma[r_] += mu[i]
        elif r_ < 2 * n:
            sigma[r_ - n] -= mu[i]
        else:
            lam[r_ - 2 * n] = max(mu[i], zero)
    assert v.dtype == dtype
    return dict(v=v, sigma=sigma, lam=lam, W=list(W), iters=it, capped=capped)


def kkt_residual(M, vstar, l, h, J, b, s):
    """The largest violated KKT condition of solve_qp's result s, relative to max|M| max(|v*|, 1e-300) (torques) and to
    max(|v|, |b|, 1e-300) (velocities): stationarity, primal and dual feasibility, complementarity."""
    v, sigma, lam = s["v"], s["sigma"], s["lam"]
    J = np.asarray(J, np.float64).reshape(len(b), len(v))
    scale = max(np.abs(M).max() * max(np.abs(vstar).max(), np.abs(v).max()), 1e-300)
    stat = np.abs(M @ (v - vstar) - sigma - J.T @ lam).max() / scale
    vs = max(np.abs(v).max(), np.abs(b).max() if len(b) else 0.0, np.abs(vstar).max(), 1e-300)
    slack = J @ v - b if len(b) else np.zeros(0)
    primal = max(np.maximum(l - v, 0).max(), np.maximum(v - h, 0).max(), np.maximum(-slack, 0).max() if len(b) else 0.0) / vs
    dual = (np.maximum(-lam, 0).max() if len(b) else 0.0) / scale
    at_l, at_h = v == l, v == h
    sg = np.where(at_l & at_h, 0.0, np.where(at_l, np.maximum(-sigma, 0), np.where(at_h, np.maximum(sigma, 0), np.abs(sigma))))
    comp = (np.abs(lam * slack).max() if len(b) else 0.0) / (scale * vs)
    return max(stat, primal, dual, sg.max() / scale, comp)


def brute_force(M, vstar, l, h, J, b):
    """The minimiser by enumeration of every working set of at most n rows (each dof free, on l or on h; each contact row on or
    off): the feasible point with multipliers of the right sign and least objective.  Small problems only."""
    n, nc = len(vstar), len(b)
    J = np.asarray(J, np.float64).reshape(nc, n)
    A = np.concatenate([np.eye(n), -np.eye(n), J])
    beta = np.concatenate([l, -h, b])
    best, best_f = None, np.inf
    Mi = np.linalg.inv(M)
    for choice in itertools.product((0, 1, 2), repeat=n):
        for cs in itertools.product((0, 1), repeat=nc):
            W = [j if c == 1 else n + j for j, c in enumerate(choice) if c] + [2 * n + c for c in range(nc) if cs[c]]
            if len(W) > n or any(np.isinf(beta[r]) for r in W):
                continue
            if W:
                AW = A[W]
                G = AW @ Mi @ AW.T
                if np.linalg.matrix_rank(G, tol=1e-10 * max(np.abs(G).max(), 1e-300)) < len(W):
                    continue
                mu = np.linalg.solve(G, beta[W] - AW @ vstar)
                v = vstar + Mi @ AW.T @ mu
            else:
                mu, v = np.zeros(0), vstar.copy()
            tolv = 1e-10 * (1 + np.abs(v).max())
            if (A @ v < np.where(np.isinf(beta), -np.inf, beta) - tolv).any():
                continue
            f = 0.5 * (v - vstar) @ M @ (v - vstar)
            if f < best_f:
                best, best_f = v, f
    return best


# ---- the step ----------------------------------------------------------------------------------------------------------------

def _limits(table, limits):
    if limits is None:
        return np.full(table.n_dof, -np.inf, np.float32), np.full(table.n_dof, np.inf, np.float32)
    return np.asarray(limits[0]), np.asarray(limits[1])


def substep(table, inert, caps, spheres, d_act, q, qd, u, drive, dt, lim, limits, gravity=(0.0, 0.0, -9.81), envelope=False):
    """One substep on a fleet [B, n]: dict(q, qd, qdd, tau, stop, contact, lam [B, 8], pair [B, 8] (-1: empty), overflow [B],
    n_cand [B], n_contact [B] (lambda > 0), n_stop [B] (sigma != 0), iters [B], capped [B], M, a, vstar, gap / J [B, 8, ...] of
    the candidates).  envelope: the float32 restatement."""
    dtype = np.dtype(np.float32 if envelope else np.float64)
    q, qd, u = (np.atleast_2d(np.asarray(x, dtype)) for x in (q, qd, u))
    lo, hi = _limits(table, limits)
    own = FR.owned_dofs(table)
    if envelope:
        a, tapp = FR.envelope_evaluate(table, inert, q, qd, u, drive, lim, gravity)
        M = FR.envelope_terms(table, inert, q, 0 * qd, 0 * qd, (0.0, 0.0, 0.0))[0]
    else:
        a, tapp = FR.evaluate(table, inert, q, qd, u, drive, lim, gravity)
        M = FR.mass_matrix(table, inert, q)
    B, n = q.shape
    h_ = dtype.type(dt)
    vstar = (qd + h_ * a).astype(dtype)
    pr = pair_rows(table, caps, spheres, q, dtype)
    out = dict(q=np.empty_like(q), qd=np.empty_like(q), qdd=np.empty_like(q), stop=np.zeros_like(q), contact=np.zeros_like(q),
               lam=np.zeros((B, MAX_CONTACTS), dtype), pair=np.full((B, MAX_CONTACTS), -1, int), overflow=np.zeros(B, bool),
               n_cand=np.zeros(B, int), n_contact=np.zeros(B, int), n_stop=np.zeros(B, int), iters=np.zeros(B, int),
               capped=np.zeros(B, bool), tau=tapp, a=a, vstar=vstar, M=M, gap=np.zeros((B, MAX_CONTACTS), dtype),
               J=np.zeros((B, MAX_CONTACTS, n), dtype))
    for r in range(B):
        l, h = JR.velocity_box(q[r], dt, lo, hi, own)
        keep, excess = candidates(pr["idx"], pr["gap"][r], dtype.type(d_act))
        out["overflow"][r] = excess > 0
        out["n_cand"][r] = len(keep)
        if len(keep) == 0:
            if not ((vstar[r] < l) | (vstar[r] > h)).any():
                v, sigma = vstar[r], np.zeros(n, dtype)
            else:
                s = JR.solve_box(M[r], vstar[r], l, h)
                v, sigma = s["v"], np.where(s["W"], s["lam"], dtype.type(0))
                out["iters"][r], out["capped"][r] = s["iters"], s["capped"]
                out["n_stop"][r] = int((sigma != 0).sum())
            lam = np.zeros(0, dtype)
            Jc = np.zeros((0, n), dtype)
        else:
            Jc = pr["J"][r][keep]
            gc = pr["gap"][r][keep]
            b = (-np.maximum(gc, dtype.type(0)) / h_).astype(dtype)
            s = solve_qp(M[r], vstar[r], l, h, Jc, b)
            v, sigma, lam = s["v"], s["sigma"], s["lam"]
            out["iters"][r], out["capped"][r] = s["iters"], s["capped"]
            out["n_stop"][r] = int((sigma != 0).sum())
            out["n_contact"][r] = int((lam > 0).sum())
            out["lam"][r, :len(keep)] = lam / h_
            out["pair"][r, :len(keep)] = pr["idx"][keep]
            out["gap"][r, :len(keep)] = gc
            out["J"][r, :len(keep)] = Jc
            out["contact"][r] = (Jc * lam[:, None]).sum(0, dtype=dtype) / h_
        q1 = q[r] + h_ * v
        if len(keep) or out["iters"][r]:
            on_l, on_h = own & (v != 0) & (v == l), own & (v != 0) & (v == h)
            q1 = np.where(on_l, lo.astype(dtype), np.where(on_h, hi.astype(dtype), q1))
            q1 = np.where(own & (q[r] >= lo) & (q1 < lo), lo.astype(dtype), q1)
            q1 = np.where(own & (q[r] <= hi) & (q1 > hi), hi.astype(dtype), q1)
        out["q"][r], out["qd"][r] = q1, v
        out["qdd"][r] = a[r] + (v - vstar[r]) / h_
        out["stop"][r] = sigma / h_
    return out


def dynamics_step(table, inert, caps, spheres, d_act, q, qd, u, drive, dt, substeps, lim, limits, gravity=(0.0, 0.0, -9.81),
                  envelope=False):
    """The literal substep loop: the last substep's dict (q, qd advanced over all of them), `iters` the largest count, capped /
    overflow or-ed, `any_contact` / `any_stop` / `any_cand` [B] over the substeps."""
    acc = None
    for _ in range(substeps):
        s = substep(table, inert, caps, spheres, d_act, q, qd, u, drive, dt, lim, limits, gravity, envelope)
        q, qd = s["q"], s["qd"]
        cur = dict(iters=s["iters"], capped=s["capped"], overflow=s["overflow"], any_contact=s["n_contact"] > 0,
                   any_stop=s["n_stop"] > 0, any_cand=s["n_cand"] > 0)
        if acc is None:
            acc = cur
        else:
            acc = {k: (np.maximum(acc[k], cur[k]) if k == "iters" else acc[k] | cur[k]) for k in acc}
    s.update(acc)
    return s


# ---- the bounds' brackets (the factor K in front of them comes from the envelope: tests/test_contacts_host.py) ---------------

def _force_scale(ref):
    both = np.maximum(np.abs(np.nan_to_num(ref["stop"])).max(1), np.abs(np.nan_to_num(ref["contact"])).max(1))
    return np.maximum(both, np.abs(np.nan_to_num(ref["stop"] + ref["contact"])).max(1))


def residual_bracket(table, inert, q, qd, ref, gravity=(0.0, 0.0, -9.81)):
    """joint_stops_reference.residual_bracket, its scale extended by max|contact_ref|."""
    base = FR.residual_bracket(table, inert, q, qd, ref["qdd"], ref["tau"], gravity)
    return np.maximum(base, 1e-4 + 1e-5 * _force_scale(ref))


def residual(table, inert, q, qd, qdd, tapp, stop, contact, gravity=(0.0, 0.0, -9.81)):
    """Per robot max_j |rnea64(q, qd, qdd) - tau_applied - stop - contact|_j over the owned dofs."""
    return FR.residual(table, inert, q, qd, qdd, np.asarray(tapp, np.float64) + np.asarray(stop, np.float64)
                       + np.asarray(contact, np.float64), gravity)


def velocity_bracket(ref, qd0, dt):
    return JR.velocity_bracket(ref, qd0, dt)


def force_bracket(ref):
    """Per robot 1e-4 + 1e-5 s, s = max(max|stop_ref|, max|contact_ref|, max_j sum_k |M_jk| |qdd_ref_k|): the bracket of the
    total constraint torque stop + contact."""
    s = np.maximum(_force_scale(ref), np.einsum("bjk,bk->bj", np.abs(ref["M"]), np.abs(np.nan_to_num(ref["qdd"]))).max(1))
    return 1e-4 + 1e-5 * s


def step_brackets(ref, dt, substeps):
    return FR.step_brackets(ref["q"], ref["qd"], ref["qdd"], dt, substeps)


# ---- the host driver's input -------------------------------------------------------------------------------------------------

def write_driver_input(path, table, inert, caps, spheres, d_act, q, qd, u, drive, lim, limits, dt, substeps,
                       gravity=(0.0, 0.0, -9.81), lists=None, planes=None):
    """Input file of tests/contacts_driver.cpp: forward_dynamics_reference.write_driver_input's (mode 2) followed by int32
    has_limits, float lower[n_dof], upper[n_dof], float caps[F][8], int32 K, float d_act, float spheres[K][4], int32 has_lists,
    [int32 offset [B + 1], int32 n_index, int32 index] with lists = (csr_offset, csr_index), int32 has_planes, [int32 P, float
    planes [P][4]] with planes = an array (an empty one too: the plane form on no planes)."""
    FR.write_driver_input(path, table, inert, q, qd, u, 2, drive=drive, lim=lim, dt=dt, substeps=substeps, gravity=gravity)
    lo, hi = _limits(table, limits)
    sph = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    with open(path, "ab") as f:
        np.array([0 if limits is None else 1], np.int32).tofile(f)
        np.ascontiguousarray(lo, np.float32).tofile(f)
        np.ascontiguousarray(hi, np.float32).tofile(f)
        np.ascontiguousarray(caps, np.float32).tofile(f)
        np.array([len(sph)], np.int32).tofile(f)
        np.array([d_act], np.float32).tofile(f)
        sph.tofile(f)
        np.array([0 if lists is None else 1], np.int32).tofile(f)
        if lists is not None:
            off, idx = (np.ascontiguousarray(x, np.int32) for x in lists)
            assert len(off) == len(q) + 1
            off.tofile(f)
            np.array([len(idx)], np.int32).tofile(f)
            idx.tofile(f)
        np.array([0 if planes is None else 1], np.int32).tofile(f)
        if planes is not None:
            pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
            np.array([len(pl)], np.int32).tofile(f)
            pl.tofile(f)


def read_driver_output(path, B, n):
    """dict(q, qd, qdd, tau, stop, contact [B, n], lam [B, 8], pair [B, 8], status [B]) of tests/contacts_driver.cpp."""
    raw = np.fromfile(path, np.uint8)
    off = 0
    out = {}
    for k in ("q", "qd", "qdd", "tau", "stop", "contact"):
        out[k] = raw[off:off + 4 * B * n].view(np.float32).reshape(B, n)
        off += 4 * B * n
    out["lam"] = raw[off:off + 4 * B * MAX_CONTACTS].view(np.float32).reshape(B, MAX_CONTACTS)
    off += 4 * B * MAX_CONTACTS
    out["pair"] = raw[off:off + 4 * B * MAX_CONTACTS].view(np.int32).reshape(B, MAX_CONTACTS)
    off += 4 * B * MAX_CONTACTS
    out["status"] = raw[off:off + 4 * B].view(np.uint32)
    assert off + 4 * B == len(raw)
    return out

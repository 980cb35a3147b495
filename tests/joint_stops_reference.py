"""fp64 restatement of the plant's step with joint-limit stops (include/rmp2.h rmp2_dynamics_step_stops) for the tests, built on
tests/forward_dynamics_reference.py, a brute-force check of it, and an fp32 ENVELOPE: the same quantities restated in float32
numpy in this file's own arithmetic (forward_dynamics_reference's fp32 walk, mass matrix and Cholesky; the active-set loop below
run on float32 arrays) -- not the device routine.  The envelope's error against the fp64 reference is the measure the GPU bounds
are taken from (K = 4 x its worst ratio, tests/test_joint_stops_host.py).

Semantics, per substep at (q, qd):  a, tau_applied = forward_dynamics_reference.evaluate;  v* = qd + dt a;  per owned dof
    l_j = min((lo_j - q_j) / dt, 0),  h_j = max((hi_j - q_j) / dt, 0)      (no bound on an unowned dof)
    v = argmin 1/2 (v - v*)^T M (v - v*)  s.t.  l <= v <= h;   lambda = M (v - v*)
    qd <- v;  q <- q + dt v;   qdd_out = a + (v - v*) / dt,  stop_out = lambda / dt.
"""
from __future__ import annotations

import itertools

import numpy as np

import forward_dynamics_reference as FR
from riemannian_motion_policies_amd import urdf as U

ACTIVE, CAPPED = 1, 2
REFERENCE_CAP = 1000      # of the fp64 loop: never reached on the test fleets (asserted)


def table_limits(table):
    """(lower, upper) float32 [n]: the table's joint limits per dof, -inf / +inf where it has none or no joint owns the dof."""
    lo = np.full(table.n_dof, -np.inf, np.float32)
    hi = np.full(table.n_dof, np.inf, np.float32)
    for f in range(table.n_frames):
        j = int(table.q_index[f])
        if j >= 0 and table.joint_type[f] != U.JOINT_FIXED:
            if np.isfinite(table.limits_lower[f]):
                lo[j] = table.limits_lower[f]
            if np.isfinite(table.limits_upper[f]):
                hi[j] = table.limits_upper[f]
    return lo, hi


def velocity_box(q, dt, lo, hi, own):
    """(l, h) of one state, in q's dtype."""
    dtype = q.dtype
    with np.errstate(invalid="ignore"):
        l = np.minimum((lo.astype(dtype) - q) / dtype.type(dt), dtype.type(0))
        h = np.maximum((hi.astype(dtype) - q) / dtype.type(dt), dtype.type(0))
    l = np.where(own, l, dtype.type(-np.inf)).astype(dtype)
    h = np.where(own, h, dtype.type(np.inf)).astype(dtype)
    return l, h


def _solve64(A, b):
    return np.linalg.solve(A, b)


def _solve32(A, b):
    return FR._cholesky_solve32(A[None], b[None])[0]


def solve_box(M, vstar, l, h, cap=REFERENCE_CAP):
    """The primal active-set method, one bound at a time, in the dtype of the arrays (float64: the reference; float32: the
    envelope).  Returns dict(v, lam (= M (v - v*), whole), W (final working set), iters, capped, released (a dof that the
    initial clip had put in W was dropped), active0 (the initial clip's W))."""
    dtype = vstar.dtype
    solve = _solve64 if dtype == np.float64 else _solve32
    n = len(vstar)
    v = np.clip(vstar, l, h)
    W = (vstar < l) | (vstar > h)
    upper = vstar > h
    W0 = W.copy()
    released = capped = False
    it = 0
    zero, one = dtype.type(0), dtype.type(1)
    eye = np.eye(n, dtype=dtype)
    lam = np.zeros(n, dtype)
    while W0.any():      # (entered only from a clipped start; W may empty and fill again on the way)
        if it >= cap:
            capped = True
            break
        it += 1
        d = np.where(W, v - vstar, zero)
        pin = W[:, None] | W[None, :]
        A = np.where(pin, eye, M)
        rhs = np.where(W, d, -(M * d[None, :]).sum(1, dtype=dtype))
        x = solve(A, rhs)
        vhat = np.where(W, v, vstar + x)
        below, above = ~W & (vhat < l), ~W & (vhat > h)
        viol = below | above
        if viol.any():
            b = np.where(below, l, h)
            with np.errstate(all="ignore"):
                alpha = np.where(viol, (b - v) / (vhat - v), dtype.type(np.inf))
            j = int(np.argmin(alpha))
            a = min(max(alpha[j], zero), one)
            vn = np.clip(v + a * (vhat - v), l, h)
            vn = np.where(W, v, vn)
            vn[j] = b[j]
            v = vn.astype(dtype)
            W[j] = True
            upper[j] = above[j]
            continue
        v = vhat.astype(dtype)
        lam = (M * (v - vstar)[None, :]).sum(1, dtype=dtype)
        wrong = W & (l < h) & np.where(upper, lam > 0, lam < 0)
        if not wrong.any():
            break
        j = int(np.argmax(np.where(wrong, np.abs(lam), -one)))
        W[j] = False
        released = released or bool(W0[j])
    lam = (M * (v - vstar)[None, :]).sum(1, dtype=dtype)
    assert v.dtype == dtype and lam.dtype == dtype
    return dict(v=v, lam=lam, W=W, upper=upper, iters=it, capped=capped, released=released, active0=W0)


def kkt_residual(M, vstar, l, h, v):
    """max over the dofs of the violated KKT condition, in units of lambda, relative to max|M| max|v*| (1 where that is 0)."""
    lam = M @ (v - vstar)
    scale = max(np.abs(M).max() * np.abs(vstar).max(), 1e-300)
    at_l, at_h = v == l, v == h
    r = np.where(at_l & at_h, 0.0, np.where(at_l, np.maximum(-lam, 0.0), np.where(at_h, np.maximum(lam, 0.0), np.abs(lam))))
    box = np.maximum(np.maximum(l - v, v - h), 0.0) * np.abs(M).max()
    return max(r.max(), box.max()) / scale


def brute_force(M, vstar, l, h):
    """The minimiser by enumeration of every working set (each dof free, on l or on h): the feasible KKT point of least
    objective.  n <= 4."""
    n = len(vstar)
    best, best_f = None, np.inf
    for choice in itertools.product((0, 1, 2), repeat=n):
        c = np.array(choice)
        if (np.isinf(l) & (c == 1)).any() or (np.isinf(h) & (c == 2)).any():
            continue
        W = c > 0
        v = np.where(c == 1, l, np.where(c == 2, h, 0.0))
        F = ~W
        if F.any():
            d = np.where(W, v - vstar, 0.0)
            x = np.linalg.solve(M[np.ix_(F, F)], -(M[np.ix_(F, W)] @ d[W]))
            v[F] = vstar[F] + x
        if (v < l - 1e-12 * (1 + np.abs(l))).any() or (v > h + 1e-12 * (1 + np.abs(h))).any():
            continue
        f = 0.5 * (v - vstar) @ M @ (v - vstar)
        if f < best_f:
            best, best_f = v, f
    return best


def substep(table, inert, q, qd, u, drive, dt, lim, limits, gravity=(0.0, 0.0, -9.81), envelope=False):
    """One substep on a fleet [B, n]: dict(q, qd, qdd, tau, stop, a, vstar, iters [B], capped, released, n_active (strictly
    active stops: in the final W with a multiplier of the right sign and non-zero), fast [B] (v* in the box)).  envelope: the
    float32 restatement."""
    dtype = np.dtype(np.float32 if envelope else np.float64)
    q, qd, u = (np.atleast_2d(np.asarray(x, dtype)) for x in (q, qd, u))
    lo, hi = limits
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
    out = dict(q=np.empty_like(q), qd=np.empty_like(q), qdd=np.empty_like(q), stop=np.zeros_like(q), tau=tapp, a=a, vstar=vstar,
               iters=np.zeros(B, int), capped=np.zeros(B, bool), released=np.zeros(B, bool), n_active=np.zeros(B, int),
               fast=np.zeros(B, bool), strict=np.zeros((B, n), int), M=M)
    for b in range(B):
        l, h = velocity_box(q[b], dt, np.asarray(lo), np.asarray(hi), own)
        if not ((vstar[b] < l) | (vstar[b] > h)).any():       # (also a NaN row: the plant's own step)
            out["fast"][b] = True
            out["qd"][b] = vstar[b]
            out["q"][b] = q[b] + h_ * vstar[b]
            out["qdd"][b] = a[b]
            continue
        s = solve_box(M[b], vstar[b], l, h)
        v, lam = s["v"], np.where(s["W"], s["lam"], dtype.type(0))
        q1 = q[b] + h_ * v
        on_l, on_h = own & (v != 0) & (v == l), own & (v != 0) & (v == h)
        q1 = np.where(on_l, lo.astype(dtype), np.where(on_h, hi.astype(dtype), q1))
        q1 = np.where(own & (q[b] >= lo) & (q1 < lo), lo.astype(dtype), q1)
        q1 = np.where(own & (q[b] <= hi) & (q1 > hi), hi.astype(dtype), q1)
        out["q"][b], out["qd"][b] = q1, v
        out["qdd"][b] = a[b] + (v - vstar[b]) / h_
        out["stop"][b] = lam / h_
        out["iters"][b], out["capped"][b], out["released"][b] = s["iters"], s["capped"], s["released"]
        strict = s["W"] & (l < h) & np.where(s["upper"], lam < 0, lam > 0)
        out["strict"][b] = np.where(strict, np.where(s["upper"], -1, 1), 0)     # the sign stop_out must have there
        out["n_active"][b] = int((s["W"] & (lam != 0)).sum())
    return out


def dynamics_step(table, inert, q, qd, u, drive, dt, substeps, lim, limits, gravity=(0.0, 0.0, -9.81), envelope=False):
    """The literal substep loop: the last substep's dict (q, qd advanced over all of them), `iters` the largest count and
    capped / released or-ed over the substeps, `any_active` [B]."""
    any_active = None
    most = capped = released = None
    for _ in range(substeps):
        s = substep(table, inert, q, qd, u, drive, dt, lim, limits, gravity, envelope)
        q, qd = s["q"], s["qd"]
        any_active = ~s["fast"] if any_active is None else any_active | ~s["fast"]
        most = s["iters"] if most is None else np.maximum(most, s["iters"])
        capped = s["capped"] if capped is None else capped | s["capped"]
        released = s["released"] if released is None else released | s["released"]
    s.update(iters=most, capped=capped, released=released, any_active=any_active)
    return s


# ---- the bounds' brackets (the factor K in front of them comes from the envelope: tests/test_joint_stops_host.py) -----------

def residual_bracket(table, inert, q, qd, ref, gravity=(0.0, 0.0, -9.81)):
    """forward_dynamics_reference.residual_bracket with the stop's term: 1e-4 + 1e-5 s, s extended by max|stop_ref|."""
    base = FR.residual_bracket(table, inert, q, qd, ref["qdd"], ref["tau"], gravity)
    return np.maximum(base, 1e-4 + 1e-5 * np.abs(np.nan_to_num(ref["stop"])).max(1))


def residual(table, inert, q, qd, qdd, tapp, stop, gravity=(0.0, 0.0, -9.81)):
    """Per robot max_j |rnea64(q, qd, qdd) - tau_applied - stop|_j over the owned dofs."""
    return FR.residual(table, inert, q, qd, qdd, np.asarray(tapp, np.float64) + np.asarray(stop, np.float64), gravity)


def velocity_bracket(ref, qd0, dt):
    """Per robot, of the K_QDD form at the velocity's level: dt x qdd_bracket(qdd_ref) + 2^-23 max(|qd|, |v|) (qdd_out = a +
    (v - v*) / dt: an error e of v is e / dt of qdd_out)."""
    return dt * FR.qdd_bracket(ref["qdd"]) + 2.0 ** -23 * np.maximum(np.abs(qd0).max(1), np.abs(ref["qd"]).max(1))


def stop_bracket(ref):
    """Per robot 1e-4 + 1e-5 s, s = max(max|stop_ref|, max_j sum_k |M_jk| |qdd_ref_k|): stop = M (v - v*) / dt is a torque at
    the system's scale, and so is its error."""
    s = np.maximum(np.abs(ref["stop"]).max(1), np.einsum("bjk,bk->bj", np.abs(ref["M"]), np.abs(np.nan_to_num(ref["qdd"]))).max(1))
    return 1e-4 + 1e-5 * s


def step_brackets(ref, dt, substeps):
    return FR.step_brackets(ref["q"], ref["qd"], ref["qdd"], dt, substeps)


# ---- the host driver's input -------------------------------------------------------------------------------------------------

def write_driver_input(path, table, inert, q, qd, u, drive, lim, limits, dt, substeps, gravity=(0.0, 0.0, -9.81)):
    """Input file of tests/joint_stops_driver.cpp: forward_dynamics_reference.write_driver_input's (mode 2) followed by float
    lower[n_dof], upper[n_dof]."""
    FR.write_driver_input(path, table, inert, q, qd, u, 2, drive=drive, lim=lim, dt=dt, substeps=substeps, gravity=gravity)
    with open(path, "ab") as f:
        np.ascontiguousarray(limits[0], np.float32).tofile(f)
        np.ascontiguousarray(limits[1], np.float32).tofile(f)

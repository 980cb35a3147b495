// rmp2_forward_dynamics.h -- the plant of one fixed-base robot: joint-space mass matrix, forward dynamics and the torque-driven
// step (include/rmp2.h rmp2_mass_matrix / rmp2_forward_dynamics / rmp2_dynamics_step).
//
// After the torques (rmp2_dynamics.h) the reference calls p.stepSimulation: the robot's equations of motion answer them.  For a
// state (q, qd), an input acceleration qdd_in and an applied torque tau_app this is
//     qdd = qdd_in + M(q)^-1 (tau_app - tau_id(qdd_in)),      tau_id(a) = M a + C qd + G  (inverse_dynamics_robot's model)
// with qdd_in = 0 for a torque drive (plain forward dynamics) and qdd_in = qdd_des, tau_app = clamp(tau_id(qdd_des)) for the
// acceleration drive of simulation.step; where nothing saturates the correction is exactly zero and the solve is skipped.
//
// One forward walk over the unpruned program, as in rmp2_dynamics.h, and no backward sweep.  The walk carries qdd_in and sums
// tau_id from inverse_dynamics_robot's link wrenches; in the same visit it sums M from the stored joint axes z_j and origins o_j:
// at frame f, with the link's mass m, world centre of mass c, world tensor I_w and wrench (F, N about c), for the ancestor dofs
// i <= j of DevOp::anc_mask
//     M_ij += m v_i . v_j + w_i . (I_w w_j),   tau_id_j += v_j . F + w_j . N,
//     v_j = z_j x (c - o_j), w_j = z_j (revolute);  v_j = z_j, w_j = 0 (prismatic)   -- the motion of c per unit rate of dof j.
// (Lever arms from the joints' own origins: about the world origin, as inverse_dynamics_robot's screws are, v_j would cancel
// metres to get centimetres, and M^-1 multiplies that error by the condition number.)
// The mask is wave-uniform, so the pair loop is scalar branches around straight-line code; every index into the per-lane arrays
// is a compile-time constant after unrolling (joint values are picked by an unrolled compare, not by an indexed read).  Then an
// fp32 Cholesky M = U^T U on the packed upper triangle and two triangular solves, all over the compile-time N.
//
// A dof that no joint of the program owns (also j >= n_dof of the template size) takes no part: its row of M is e_j and its
// qdd is 0.  A pivot that is <= 0 or not finite makes every qdd of the robot NaN.  Host-compilable like rmp2_dynamics.h
// (tests/forward_dynamics_driver.cpp).
#pragma once
#include <float.h>

#include "rmp2_dynamics.h"

namespace rmp2 {

constexpr int fd_tri(int n) { return n * (n + 1) / 2; }
// packed upper triangle of an N x N matrix: row i, column j >= i
template <int N>
__host__ __device__ constexpr int fd_idx(int i, int j) { return i * N - i * (i - 1) / 2 + (j - i); }

// The walk.  q / qd / qdd: the robot's rows in registers (0 beyond n_dof).  DYN: sum tau_id(qdd) into tid as well (false: the
// mass matrix alone; tid stays 0).  M: packed upper triangle.  Returns the mask of the dofs some joint of the program owns.
template <int N, int SLOTS, bool DYN>
__host__ __device__ inline uint32_t fd_walk(const DevOp* ops, int n_ops, const float* inert, const float base_acc[3],
                                            const float (&q)[N], const float (&qd)[N], const float (&qdd)[N], float (&tid)[N],
                                            float (&M)[fd_tri(N)]) {
  float ax[N][3], org[N][3];   // the joints' world axes and origins
#pragma unroll
  for (int j = 0; j < N; ++j) {
    tid[j] = 0.f;
    for (int k = 0; k < 3; ++k) ax[j][k] = org[j][k] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < fd_tri(N); ++k) M[k] = 0.f;
  uint32_t owned = 0u, revolute = 0u;   // dofs a joint owns; those of them that are revolute (wave-uniform)
  IdState cur;
  IdState slot[SLOTS > 0 ? SLOTS : 1];
  for (int k = 0; k < n_ops; ++k) {
    const DevOp& op = ops[k];
    if (SLOTS > 0 && op.restore >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.restore == s) cur = slot[s];
    }
    const int qi = op.qidx;
    float qv = 0.f, qdv = 0.f, qddv = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j == qi) {
        qv = q[j];
        if (DYN) {
          qdv = qd[j];
          qddv = qdd[j];
        }
      }
    float z[3];
    id_visit(cur, op, qv, qdv, qddv, op.restore == -2, base_acc, z);
    if (SLOTS > 0 && op.save >= 0) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (op.save == s) slot[s] = cur;
    }
    if (qi >= 0) {   // this joint's axis and origin, kept for the frames below it
      owned |= 1u << qi;
      if (op.jtype == RMP2_JOINT_REVOLUTE) revolute |= 1u << qi;
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (j == qi)
          for (int c = 0; c < 3; ++c) {
            ax[j][c] = z[c];
            org[j][c] = cur.p[c];
          }
    }
    const float* in = inert + (size_t)op.frame * kInertialFloats;
    const float m = in[0];
    const float cl[3] = {in[1], in[2], in[3]};
    const float I[9] = {in[4], in[7], in[8], in[7], in[5], in[9], in[8], in[9], in[6]};
    float cw[3], cb[3];
    for (int i = 0; i < 3; ++i) {
      cw[i] = cur.R[3 * i + 0] * cl[0] + cur.R[3 * i + 1] * cl[1] + cur.R[3 * i + 2] * cl[2];
      cb[i] = cur.p[i] + cw[i];
    }
    float F[3] = {0.f, 0.f, 0.f}, Nw[3] = {0.f, 0.f, 0.f};
    if (DYN) {   // the link's wrench: F = m a_c, N = I_w dw + w x I_w w about c (inverse_dynamics_robot's, in world axes)
      float wl[3], dwl[3];
      for (int i = 0; i < 3; ++i) {
        wl[i] = cur.R[i] * cur.w[0] + cur.R[3 + i] * cur.w[1] + cur.R[6 + i] * cur.w[2];
        dwl[i] = cur.R[i] * cur.dw[0] + cur.R[3 + i] * cur.dw[1] + cur.R[6 + i] * cur.dw[2];
      }
      float t1[3], t2[3], t3[3];
      id_cross(cur.dw, cw, t1);
      id_cross(cur.w, cw, t2);
      id_cross(cur.w, t2, t3);
      for (int i = 0; i < 3; ++i) F[i] = m * (cur.a[i] + t1[i] + t3[i]);
      float Iw[3], Idw[3], gyr[3], Nl[3];
      for (int i = 0; i < 3; ++i) {
        Iw[i] = I[3 * i + 0] * wl[0] + I[3 * i + 1] * wl[1] + I[3 * i + 2] * wl[2];
        Idw[i] = I[3 * i + 0] * dwl[0] + I[3 * i + 1] * dwl[1] + I[3 * i + 2] * dwl[2];
      }
      id_cross(wl, Iw, gyr);
      for (int i = 0; i < 3; ++i) Nl[i] = Idw[i] + gyr[i];
      for (int i = 0; i < 3; ++i) Nw[i] = cur.R[3 * i + 0] * Nl[0] + cur.R[3 * i + 1] * Nl[1] + cur.R[3 * i + 2] * Nl[2];
    }
    // the link's share of tau_id and of M over its ancestor dofs.  v_j: the velocity of c per unit rate of dof j, taken about
    // the joint's own origin (z_j x (c - o_j)): a lever arm from the world origin would cancel metres to get centimetres.
    const uint32_t mask = op.anc_mask;
#pragma unroll
    for (int j = 0; j < N; ++j)
      if ((mask >> j) & 1u) {
        const bool rev_j = (revolute >> j) & 1u;
        float vj[3], mv[3], Ia[3] = {0.f, 0.f, 0.f};
        if (rev_j) {
          const float d[3] = {cb[0] - org[j][0], cb[1] - org[j][1], cb[2] - org[j][2]};
          id_cross(ax[j], d, vj);
          float al[3], Il[3];   // I_w z_j = R (I (R^T z_j))
          for (int i = 0; i < 3; ++i) al[i] = cur.R[i] * ax[j][0] + cur.R[3 + i] * ax[j][1] + cur.R[6 + i] * ax[j][2];
          for (int i = 0; i < 3; ++i) Il[i] = I[3 * i + 0] * al[0] + I[3 * i + 1] * al[1] + I[3 * i + 2] * al[2];
          for (int i = 0; i < 3; ++i) Ia[i] = cur.R[3 * i + 0] * Il[0] + cur.R[3 * i + 1] * Il[1] + cur.R[3 * i + 2] * Il[2];
        } else {
          for (int i = 0; i < 3; ++i) vj[i] = ax[j][i];
        }
        for (int i = 0; i < 3; ++i) mv[i] = m * vj[i];
        if (DYN) tid[j] += id_dot(vj, F) + (rev_j ? id_dot(ax[j], Nw) : 0.f);
        M[fd_idx<N>(j, j)] += id_dot(vj, mv) + (rev_j ? id_dot(ax[j], Ia) : 0.f);
#pragma unroll
        for (int i = 0; i < j; ++i)
          if ((mask >> i) & 1u) {
            if ((revolute >> i) & 1u) {
              const float d[3] = {cb[0] - org[i][0], cb[1] - org[i][1], cb[2] - org[i][2]};
              float vi[3];
              id_cross(ax[i], d, vi);
              M[fd_idx<N>(i, j)] += id_dot(vi, mv) + id_dot(ax[i], Ia);
            } else {
              M[fd_idx<N>(i, j)] += id_dot(ax[i], mv);
            }
          }
      }
  }
  return owned;
}

// M = U^T U in place on the packed upper triangle; the diagonal is left holding 1 / U_kk.  False when a pivot is <= 0 or not
// finite (M not numerically positive definite).
template <int N>
__host__ __device__ inline bool fd_cholesky(float (&M)[fd_tri(N)]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float d = M[fd_idx<N>(k, k)];
    ok = ok && d > 0.f && d <= FLT_MAX;
    const float r = 1.f / sqrtf(d);
    M[fd_idx<N>(k, k)] = r;
#pragma unroll
    for (int j = k + 1; j < N; ++j) M[fd_idx<N>(k, j)] *= r;
#pragma unroll
    for (int i = k + 1; i < N; ++i)
#pragma unroll
      for (int j = i; j < N; ++j) M[fd_idx<N>(i, j)] -= M[fd_idx<N>(k, i)] * M[fd_idx<N>(k, j)];
  }
  return ok;
}

// b <- (U^T U)^-1 b with fd_cholesky's factor
template <int N>
__host__ __device__ inline void fd_solve(const float (&U)[fd_tri(N)], float (&b)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float s = b[k];
#pragma unroll
    for (int p = 0; p < k; ++p) s -= U[fd_idx<N>(p, k)] * b[p];
    b[k] = s * U[fd_idx<N>(k, k)];
  }
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    float s = b[k];
#pragma unroll
    for (int j = k + 1; j < N; ++j) s -= U[fd_idx<N>(k, j)] * b[j];
    b[k] = s * U[fd_idx<N>(k, k)];
  }
}

// One evaluation of the plant at (q, qd) under the held input u: qdd and the applied torque tapp.  accel: u is qdd_des and
// tapp = clamp(tau_id(u)); else u is the torque, clamped.  lim: [n_dof] or null (read at uniform addresses).
template <int N, int SLOTS>
__host__ __device__ inline void fd_evaluate(const DevOp* ops, int n_ops, int n_dof, const float* inert, const float base_acc[3],
                                            const float (&q)[N], const float (&qd)[N], const float (&u)[N], bool accel,
                                            const float* lim, float (&qdd)[N], float (&tapp)[N]) {
  float qin[N], tid[N], M[fd_tri(N)];
#pragma unroll
  for (int j = 0; j < N; ++j) qin[j] = accel ? u[j] : 0.f;
  const uint32_t owned = fd_walk<N, SLOTS, true>(ops, n_ops, inert, base_acc, q, qd, qin, tid, M);
  float delta[N];
  bool any = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float t = accel ? tid[j] : u[j];
    if (lim && j < n_dof) {   // (written so that a NaN stays a NaN)
      const float L = lim[j];
      t = t < -L ? -L : (t > L ? L : t);
    }
    tapp[j] = t;
    const bool own = (owned >> j) & 1u;
    if (!own) M[fd_idx<N>(j, j)] = 1.f;   // its row of M is e_j
    delta[j] = own ? t - tid[j] : 0.f;
    any = any || delta[j] != 0.f;          // (true for a NaN as well)
  }
  if (any) {   // where nothing saturates the acceleration drive skips this: qdd = qdd_des bit for bit
    const bool ok = fd_cholesky<N>(M);
    fd_solve<N>(M, delta);
#pragma unroll
    for (int j = 0; j < N; ++j) qdd[j] = ok ? qin[j] + delta[j] : NAN;
  } else {
#pragma unroll
    for (int j = 0; j < N; ++j) qdd[j] = qin[j];
  }
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (!((owned >> j) & 1u)) qdd[j] = 0.f;
}

// rmp2_dynamics_step of one robot: q, qd advanced in place over `substeps` evaluations when integrate (else one evaluation and
// q, qd only read: rmp2_forward_dynamics); qdd_out / tau_out (null or the robot's rows) get the last evaluation's.  A
// non-finite value anywhere in the robot's q, qd or u rows makes every output of the robot NaN.
template <int N, int SLOTS>
__host__ __device__ inline void dynamics_step_robot(const DevOp* ops, int n_ops, int n_dof, const float* inert,
                                                    const float base_acc[3], float* q_io, float* qd_io, const float* u_in,
                                                    bool accel, const float* lim, float dt, int substeps, bool integrate,
                                                    float* qdd_out, float* tau_out) {
  float q[N], qd[N], u[N], qdd[N], tapp[N];
  float poison = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[j] = j < n_dof ? q_io[j] : 0.f;
    qd[j] = j < n_dof ? qd_io[j] : 0.f;
    u[j] = j < n_dof ? u_in[j] : 0.f;
    poison += q[j] * 0.f + qd[j] * 0.f + u[j] * 0.f;
  }
  for (int s = 0; s < substeps; ++s) {
    fd_evaluate<N, SLOTS>(ops, n_ops, n_dof, inert, base_acc, q, qd, u, accel, lim, qdd, tapp);
    if (integrate) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        qd[j] += dt * qdd[j];
        q[j] += dt * qd[j];
      }
    }
  }
  const bool bad = !(poison == 0.f);
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n_dof) {
      if (integrate) {
        q_io[j] = bad ? NAN : q[j];
        qd_io[j] = bad ? NAN : qd[j];
      }
      if (qdd_out) qdd_out[j] = bad ? NAN : qdd[j];
      if (tau_out) tau_out[j] = bad ? NAN : tapp[j];
    }
}

// rmp2_mass_matrix of one robot: M_out [n_dof][n_dof], both triangles from the one upper triangle (symmetric bit for bit);
// a non-finite q makes every entry NaN.
template <int N, int SLOTS>
__host__ __device__ inline void mass_matrix_robot(const DevOp* ops, int n_ops, int n_dof, const float* inert, const float* q_in,
                                                  float* M_out) {
  float q[N], zero[N], tid[N], M[fd_tri(N)];
  float poison = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[j] = j < n_dof ? q_in[j] : 0.f;
    zero[j] = 0.f;
    poison += q[j] * 0.f;
  }
  const float still[3] = {0.f, 0.f, 0.f};
  const uint32_t owned = fd_walk<N, SLOTS, false>(ops, n_ops, inert, still, q, zero, zero, tid, M);
  const bool bad = !(poison == 0.f);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (!((owned >> i) & 1u)) M[fd_idx<N>(i, i)] = 1.f;
#pragma unroll
    for (int j = i; j < N; ++j)
      if (j < n_dof) {
        const float v = bad ? NAN : M[fd_idx<N>(i, j)];
        M_out[i * n_dof + j] = v;
        M_out[j * n_dof + i] = v;
      }
  }
}

}  // namespace rmp2

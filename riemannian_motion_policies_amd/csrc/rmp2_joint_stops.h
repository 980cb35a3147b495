// rmp2_joint_stops.h -- the plant's step with joint-limit stops (include/rmp2.h rmp2_dynamics_step_stops).
//
// Per substep, at the state (q, qd): a = the acceleration of fd_evaluate (either drive, tau_limit), v* = qd + dt a, and per dof
// the velocity box  l_j = min((lo_j - q_j) / dt, 0),  h_j = max((hi_j - q_j) / dt, 0)  (no bound on a dof no joint owns).  The
// step's velocity is the box-constrained minimiser in the kinetic-energy metric,
//     v = argmin 1/2 (v - v*)^T M(q) (v - v*)   subject to   l <= v <= h,        lambda = M (v - v*),
// found by the primal active-set method, one bound at a time, from the feasible start v = clip(v*, l, h):
//   solve the equality problem of the working set W with fd_cholesky / fd_solve on a copy of M whose rows and columns of W are
//   e_j (the unowned-dof trick), right-hand side d_j = v_j - v*_j on W and -sum_{a in W} M_ja d_a elsewhere;
//   if the solution leaves the box on a free dof: go to the first blocking bound on the segment, put that dof on its bound
//   exactly, add it to W;  else take it, form lambda = M (v - v*) from the whole M, drop from W the wrong-signed multiplier of
//   largest magnitude (never a dof with l_j == h_j), and stop when there is none.
// Every iterate is feasible and the objective never increases, so the iteration cap (kStopMaxIter) leaves a valid in-limits
// velocity; it is reported (RMP2_STOP_CAPPED).  A robot whose v* lies in the box runs none of this: its integration is
// dynamics_step_robot's own expression and its results are those of rmp2_dynamics_step bit for bit.
//
// fd_evaluate factors M in place, and the loop needs M whole at every iteration beside the work triangle: fd_evaluate_saved is
// fd_evaluate with the packed triangle stored first, through pointer + stride -- on the device LDS, lane-interleaved (word k of
// lane l at k * 64 + l: consecutive lanes on consecutive banks), on the host a local array.  Every index into the per-lane
// arrays is a compile-time constant after unrolling: the blocking and the dropped dof are chosen by unrolled compares and live
// in bit masks.  Host-compilable like rmp2_forward_dynamics.h (tests/joint_stops_driver.cpp).
#pragma once
#include "rmp2_forward_dynamics.h"

namespace rmp2 {

// Twice the worst iteration count of the fp64 restatement over every test fleet (tests/test_joint_stops_host.py).
constexpr int kStopMaxIter = 10;

// fd_evaluate, with M (unowned rows already e_j) stored to Ms[k * stride] before anything factors it.
template <int N, int SLOTS>
__host__ __device__ inline uint32_t fd_evaluate_saved(const DevOp* ops, int n_ops, int n_dof, const float* inert,
                                                      const float base_acc[3], const float (&q)[N], const float (&qd)[N],
                                                      const float (&u)[N], bool accel, const float* lim, float (&qdd)[N],
                                                      float (&tapp)[N], float* Ms, int stride) {
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
#pragma unroll
  for (int k = 0; k < fd_tri(N); ++k) Ms[k * stride] = M[k];
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
  return owned;
}

// out = M d from the stored triangle
template <int N>
__host__ __device__ inline void stops_matvec(const float* Ms, int stride, const float (&d)[N], float (&out)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) out[j] = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) {
      const float m = Ms[fd_idx<N>(i, j) * stride];
      out[i] += m * d[j];
      if (j > i) out[j] += m * d[i];
    }
}

// The box-constrained velocity of one substep.  vstar, lb, ub: v*, l, h.  v: in: clip(v*, l, h), out: the minimiser (or the
// feasible iterate the cap left; NaN where a factorisation failed).  W / upper: in: the clipped dofs and which of them sit on h.
// lam: M (v - v*) on the dofs of the final W, 0 elsewhere.  Returns the number of iterations; capped: the cap ended them.
template <int N>
__host__ __device__ inline int stops_solve(const float* Ms, int stride, const float (&vstar)[N], const float (&lb)[N],
                                           const float (&ub)[N], float (&v)[N], uint32_t W, uint32_t upper, float (&lam)[N],
                                           bool& capped) {
  int it = 0;
  capped = false;
  bool failed = false;
  for (;;) {
    if (it >= kStopMaxIter) {
      capped = true;
      break;
    }
    ++it;
    // the equality problem of W
    float d[N], x[N], A[fd_tri(N)];
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] = (W >> j) & 1u ? v[j] - vstar[j] : 0.f;
    stops_matvec<N>(Ms, stride, d, x);
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = (W >> j) & 1u ? d[j] : -x[j];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i; j < N; ++j) {
        const bool pin = ((W >> i) | (W >> j)) & 1u;
        A[fd_idx<N>(i, j)] = pin ? (i == j ? 1.f : 0.f) : Ms[fd_idx<N>(i, j) * stride];
      }
    if (!fd_cholesky<N>(A)) {
      failed = true;
      break;
    }
    fd_solve<N>(A, x);
    // the first bound a free dof meets on the way from v to v* + x
    float alpha = 2.f, bval = 0.f;
    uint32_t bbit = 0u, bup = 0u;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      x[j] = (W >> j) & 1u ? v[j] : vstar[j] + x[j];   // (a dof of W stays on its bound exactly)
      const bool below = x[j] < lb[j], above = x[j] > ub[j];
      if (!((W >> j) & 1u) && (below || above)) {
        const float b = below ? lb[j] : ub[j];
        const float a = (b - v[j]) / (x[j] - v[j]);
        if (a < alpha) {
          alpha = a;
          bval = b;
          bbit = 1u << j;
          bup = above ? 1u << j : 0u;
        }
      }
    }
    if (bbit) {
      alpha = alpha < 0.f ? 0.f : (alpha > 1.f ? 1.f : alpha);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        float t = v[j] + alpha * (x[j] - v[j]);
        t = t < lb[j] ? lb[j] : (t > ub[j] ? ub[j] : t);   // (a rounding must not leave the box)
        v[j] = (bbit >> j) & 1u ? bval : ((W >> j) & 1u ? v[j] : t);
      }
      W |= bbit;
      upper = (upper & ~bbit) | bup;
      continue;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      v[j] = x[j];
      d[j] = v[j] - vstar[j];
    }
    stops_matvec<N>(Ms, stride, d, lam);
    float worst = 0.f;
    uint32_t dbit = 0u;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool up = (upper >> j) & 1u;
      const bool wrong = ((W >> j) & 1u) && lb[j] < ub[j] && (up ? lam[j] > 0.f : lam[j] < 0.f);
      const float mag = fabsf(lam[j]);
      if (wrong && mag > worst) {
        worst = mag;
        dbit = 1u << j;
      }
    }
    if (!dbit) break;
    W &= ~dbit;
  }
  if (capped) {   // the multipliers of the iterate the cap left
    float d[N];
#pragma unroll
    for (int j = 0; j < N; ++j) d[j] = v[j] - vstar[j];
    stops_matvec<N>(Ms, stride, d, lam);
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (!((W >> j) & 1u)) lam[j] = 0.f;
    if (failed) v[j] = lam[j] = NAN;
  }
  return it;
}

// rmp2_dynamics_step_stops of one robot: dynamics_step_robot with the stops.  qlo / qhi: [n_dof], read at uniform addresses.
// stop_out (null or the robot's row): lambda / dt of the last substep; status_out (null or the robot's word): RMP2_STOP_* flags
// over the substeps, and in bits 8.. the largest iteration count of a substep.  Ms / stride: room for fd_tri(N) floats.
template <int N, int SLOTS>
__host__ __device__ inline void dynamics_step_stops_robot(const DevOp* ops, int n_ops, int n_dof, const float* inert,
                                                          const float base_acc[3], float* q_io, float* qd_io, const float* u_in,
                                                          bool accel, const float* lim, const float* qlo, const float* qhi,
                                                          float dt, int substeps, float* qdd_out, float* tau_out, float* stop_out,
                                                          uint32_t* status_out, float* Ms, int stride) {
  float q[N], qd[N], u[N], qdd[N], tapp[N], stop[N];
  float poison = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[j] = j < n_dof ? q_io[j] : 0.f;
    qd[j] = j < n_dof ? qd_io[j] : 0.f;
    u[j] = j < n_dof ? u_in[j] : 0.f;
    poison += q[j] * 0.f + qd[j] * 0.f + u[j] * 0.f;
  }
  uint32_t status = 0u;
  int most = 0;
  for (int s = 0; s < substeps; ++s) {
    const uint32_t owned = fd_evaluate_saved<N, SLOTS>(ops, n_ops, n_dof, inert, base_acc, q, qd, u, accel, lim, qdd, tapp, Ms, stride);
    float vstar[N], lb[N], ub[N], v[N];
    uint32_t W = 0u, upper = 0u;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      vstar[j] = qd[j] + dt * qdd[j];
      lb[j] = -INFINITY;
      ub[j] = INFINITY;
      if (j < n_dof && ((owned >> j) & 1u)) {
        lb[j] = fminf((qlo[j] - q[j]) / dt, 0.f);
        ub[j] = fmaxf((qhi[j] - q[j]) / dt, 0.f);
      }
      const bool below = vstar[j] < lb[j], above = vstar[j] > ub[j];
      v[j] = below ? lb[j] : (above ? ub[j] : vstar[j]);
      if (below || above) W |= 1u << j;
      if (above) upper |= 1u << j;
    }
    if (!W) {   // v* is in the box: the step of dynamics_step_robot, in its own words
#pragma unroll
      for (int j = 0; j < N; ++j) {
        qd[j] += dt * qdd[j];
        q[j] += dt * qd[j];
        stop[j] = 0.f;
      }
      continue;
    }
    bool capped;
    const int it = stops_solve<N>(Ms, stride, vstar, lb, ub, v, W, upper, stop, capped);
    status |= RMP2_STOP_ACTIVE | (capped ? RMP2_STOP_CAPPED : 0u);
    most = it > most ? it : most;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      qdd[j] += (v[j] - vstar[j]) / dt;
      stop[j] /= dt;
      qd[j] = v[j];
      const float q0 = q[j];
      float q1 = q0 + dt * v[j];
      if (j < n_dof && ((owned >> j) & 1u)) {
        const float lo = qlo[j], hi = qhi[j];
        // a dof on a bound that its limit set lands on the limit; a rounding takes no dof that was inside outside
        if (v[j] != 0.f && v[j] == lb[j]) q1 = lo;
        if (v[j] != 0.f && v[j] == ub[j]) q1 = hi;
        if (q0 >= lo && q1 < lo) q1 = lo;
        if (q0 <= hi && q1 > hi) q1 = hi;
      }
      q[j] = q1;
    }
  }
  const bool bad = !(poison == 0.f);
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j < n_dof) {
      q_io[j] = bad ? NAN : q[j];
      qd_io[j] = bad ? NAN : qd[j];
      if (qdd_out) qdd_out[j] = bad ? NAN : qdd[j];
      if (tau_out) tau_out[j] = bad ? NAN : tapp[j];
      if (stop_out) stop_out[j] = bad ? NAN : stop[j];
    }
  if (status_out) *status_out = status | ((uint32_t)most << 8);
}

#if defined(__HIPCC__)
// One lane per robot, as rmp2_dynamics_step_kernel; the saved M of the wave's 64 robots in LDS, lane-interleaved.
template <int N, int SLOTS>
__global__ void __launch_bounds__(kWave)
rmp2_dynamics_step_stops_kernel(const DevProgram* __restrict__ prog, const float* __restrict__ inert, float ax, float ay, float az,
                                float* q, float* qd, const float* __restrict__ u, int accel, const float* __restrict__ lim,
                                const float* __restrict__ qlo, const float* __restrict__ qhi, float dt, int substeps,
                                float* __restrict__ qdd_out, float* __restrict__ tau_out, float* __restrict__ stop_out,
                                uint32_t* __restrict__ status_out, int R) {
  __shared__ float Ms[fd_tri(N) * kWave];
  const int robot = blockIdx.x * kWave + threadIdx.x;
  if (robot >= R) return;
  const int n_dof = prog->n_dof;
  const size_t row = (size_t)robot * n_dof;
  const float base_acc[3] = {ax, ay, az};
  dynamics_step_stops_robot<N, SLOTS>(prog->ops, prog->n_ops, n_dof, inert, base_acc, q + row, qd + row, u + row, accel != 0, lim,
                                      qlo, qhi, dt, substeps, qdd_out ? qdd_out + row : nullptr, tau_out ? tau_out + row : nullptr,
                                      stop_out ? stop_out + row : nullptr, status_out ? status_out + robot : nullptr,
                                      Ms + threadIdx.x, kWave);
}
#endif

}  // namespace rmp2
